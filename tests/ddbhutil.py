"""Seeded DDBH cases shared by tests/golden/make_golden20.py and the tests, and a float64 restatement of the base-point loss, the
quantisation term, the trainer's five-term sum and their gradients, written from the definition (reference train/DDBH/loss.py:5-101,
train/DDBH/hash_train.py:64-78):

  s = (y y^T > 0), inner = u v^T; a row is active when it has a similar and a dissimilar column (the diagonal counts)
  meanS = clamp(mean S, 0, ub), dMax = mean of the n_d - int(n_d percent) largest of D, BP = meanS - (ub - meanS)/ub |meanS - dMax|
  meanDS = clamp(mean D, 0, ub), sMin = mean of the n_s - int(n_s percent) smallest of S, BP_ds = meanDS - meanDS/ub |meanDS - sMin|
  c = ln(y_p / (99 (1 - y_p))) / right, d = ln((1 - y_p)/y_p) - c P, a = -ln(99 y_p/(1 - y_p)) / (left c), g = ln((1 - y_p)/y_p) - a c P
  similar:    x > BP: f = c x + d;    x < BP: f = a c x + g;       element f + log(1 + e^-f)
  dissimilar: x < BP_ds: f = c x + d; x > BP_ds: f = a c x + g;    element log(1 + e^-f)
  an entry equal to its base point is not kept; row terms are means over the kept entries; loss = (sum pos + sum neg) / active rows

The four means are rounded to float32 (upstream they are float32 values read as doubles); BP, BP_ds and the six coefficients are rounded
to float32 once, where torch rounds them upstream (a double against a float32 tensor); everything else is float64, and log(1 + e^-f) is max(-f, 0) + log1p(e^-|f|).

One batch cannot hold rows without labels AND rows similar to every column (a column without labels is similar to no row), so the
32 x 32 x 6 mixture of inactive and active rows is two cases: `mix_a` has rows without labels next to active rows, `mix_b` rows similar to every column next to active rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipe  # noqa: E402

# (B, K, C, kind, seed): the seeds are the first from 91 on whose cases (intra and cross) pass make_golden20.py's gap condition
CASES = [(8, 16, 4, "p0.3", 91), (37, 64, 24, "p0.1", 91), (65, 128, 80, "p0.03", 91), (128, 64, 24, "p0.1", 124),
         (12, 16, 3, "zero", 91), (32, 32, 6, "mix_a", 91), (32, 32, 6, "mix_b", 91)]
MODES = ("intra", "cross")
F32 = np.float32


def scalars(bit):
    """BPLoss(bit)'s attributes (loss.py:8-13): y_p, right, left, lowerBound, upperBound, percent"""
    return (0.5, bit / 6, bit / 6 / 2, 0, bit / 4, 9 / 10)


def _labels(B, C, kind, seed, tag):
    if kind == "zero":
        return np.zeros((B, C), F32)
    if kind == "mix_a":                       # rows 0-5 without labels; the others one or two of six classes: active
        lab = np.zeros((B, C), F32)
        for i in range(6, B):
            lab[i, i % C] = 1.0
            if i % 5 == 0:
                lab[i, (i + 2) % C] = 1.0
        return lab
    if kind == "mix_b":                       # rows 0-3 carry classes 0 and 1 and every other row one of the two: 0-3 see no dissimilar column
        lab = np.zeros((B, C), F32)
        lab[:4, :2] = 1.0
        for i in range(4, B):
            lab[i, i % 2] = 1.0
            lab[i, 2 + i % 4] = 1.0           # (classes 2-5 change nothing about who is similar to rows 0-3)
        return lab
    return recipe.labels(B, C, seed, p=float(kind[1:]), tag=f"ddbh_lab_{tag}")


def ddbh_case(B, K, C, kind, seed):
    tag = f"B{B}_K{K}_C{C}_{kind}"
    return dict(tag=tag, u=np.tanh(recipe.features(B, K, seed, f"ddbh_u_{tag}")), v=np.tanh(recipe.features(B, K, seed, f"ddbh_v_{tag}")),
                lab=_labels(B, C, kind, seed, tag))


def _softplus_neg(f):
    return np.maximum(-f, 0.0) + np.log1p(np.exp(-np.abs(f)))


def _sigmoid(f):
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def coefficients(P, sc):
    y_p, right, left = sc[0], sc[1], sc[2]
    c = 1 / right * np.log(y_p / (99 * (1 - y_p)))                  # (the order of the operations is upstream's, loss.py:92-99)
    a = -1 / (left * c) * np.log(99 * y_p / (1 - y_p))
    l2 = np.log((1 - y_p) / y_p)
    return c, a * c, l2 - c * P, l2 - a * c * P                     # c, a c, d, g


def bp_loss(u, v, y, sc, inner=None, round_means=True):
    """-> dict(loss, du, dv, bp, bpds, active, gap): float64; du, dv the gradients of the two roles (u is v: their sum is the gradient).
    round_means: the four means are float32 values upstream (read as doubles); False leaves them float64, which with inner = a float32
    matrix product gives the generator the two views it compares."""
    u, v, y = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(y, np.float64)
    B = u.shape[0]
    lower, upper, percent = float(sc[3]), float(sc[4]), sc[5]
    s = (y @ y.T) > 0
    inner = u @ v.T if inner is None else np.asarray(inner, np.float64)
    rm = (lambda m: float(F32(m))) if round_means else float
    G = np.zeros((B, B))
    bps, bpdss, active = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, bool)
    pos = neg = 0.0
    gap = np.inf
    for i in range(B):
        S, D = inner[i][s[i]], inner[i][~s[i]]
        if S.size == 0 or D.size == 0:
            continue
        active[i] = True
        mean_s = rm(np.clip(rm(S.mean()), lower, upper))
        d_max = rm(np.sort(D)[int(D.size * percent):].mean())
        bp = mean_s - (upper - mean_s) / upper * abs(mean_s - d_max)
        mean_d = rm(np.clip(rm(D.mean()), lower, upper))
        s_min = rm(np.sort(S)[::-1][int(S.size * percent):].mean())
        bpds = mean_d - mean_d / upper * abs(mean_d - s_min)
        bps[i], bpdss[i] = bp, bpds
        gap = min(gap, np.abs(S - bp).min(), np.abs(D - bpds).min())
        x, g = inner[i], np.zeros(B)
        for sim, P in ((True, bp), (False, bpds)):
            c, ac, d, gg = (float(F32(t)) for t in coefficients(P, sc))
            P32 = float(F32(P))
            mine = s[i] if sim else ~s[i]
            easy = mine & ((x > P32) if sim else (x < P32))
            hard = mine & ((x < P32) if sim else (x > P32))
            f = np.where(easy, c * x + d, ac * x + gg)
            kept = easy | hard
            m = int(kept.sum())
            elem = (f if sim else 0.0) + _softplus_neg(f)
            term = elem[kept].sum() / m if m else np.nan             # the mean of nothing upstream
            w = _sigmoid(f) if sim else -_sigmoid(-f)
            if m:
                g += np.where(kept, np.where(easy, c, ac) * w / m, 0.0)
            if sim:
                pos += term
            else:
                neg += term
        G[i] = g
    count = int(active.sum())
    if count == 0:
        return dict(loss=0.0, du=np.zeros_like(u), dv=np.zeros_like(v), bp=bps, bpds=bpdss, active=active, gap=gap)
    G /= count
    return dict(loss=pos / count + neg / count, du=G @ v, dv=G.T @ u, bp=bps, bpds=bpdss, active=active, gap=gap)


def quant_loss(h, y):
    """mean(s @ (h - sign h)^2) over [B, K] and its gradient"""
    h, y = np.asarray(h, np.float64), np.asarray(y, np.float64)
    s = ((y @ y.T) > 0).astype(np.float64)
    r = h - np.sign(h)
    return float((s @ r ** 2).mean()), 2.0 * r * s.sum(0)[:, None] / h.size


def step_loss(hi, ht, y, sc):
    """bp(hi, hi) + bp(ht, ht) + bp(hi, ht) + 0.1 (q(hi) + q(ht)) -> loss, d/dhi, d/dht"""
    a, b, c = bp_loss(hi, hi, y, sc), bp_loss(ht, ht, y, sc), bp_loss(hi, ht, y, sc)
    qi, gi = quant_loss(hi, y)
    qt, gt = quant_loss(ht, y)
    loss = (a["loss"] + b["loss"] + c["loss"]) + 0.1 * (qi + qt)
    return loss, a["du"] + a["dv"] + c["du"] + 0.1 * gi, b["du"] + b["dv"] + c["dv"] + 0.1 * gt


# ---- the training trajectory (make_golden20.py and the GPU test): tiny CLIP and optimiser of dchmtutil, LinearHash heads, batch 8
TRAJ_K, TRAJ_STEPS = 16, 3
TRAJ_SEEDS = (7, 17, 37)                      # the batch of step k is dchmtutil.batch's with this seed


def traj_batch(step):
    import torch
    import dchmtutil as du
    seed = TRAJ_SEEDS[step]
    img = torch.from_numpy(recipe.images(du.B, du.CFG["image_resolution"], seed))
    txt = torch.from_numpy(recipe.captions(du.B, du.L, du.CFG["vocab_size"], seed))
    lab = torch.from_numpy(recipe.labels(du.B, du.C, seed, p=0.25, tag=f"ddbh_traj_{step}"))
    return img, txt, lab


def fill_linear_head(head, seed):
    """deterministic weights for a LinearHash head (fc), the same for the reference's and this project's class"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(head.named_parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.01))


# ---- edges (the GPU test): codes in {-1, +1}, so inner products are exact integers and ties at the tail cut are real
def group_labels(sizes):
    """one class per group of consecutive rows: a row of a group of g sees n_s = g and n_d = B - g"""
    lab = np.zeros((sum(sizes), len(sizes)), F32)
    lab[np.arange(sum(sizes)), np.repeat(np.arange(len(sizes)), sizes)] = 1.0
    return lab


def edge_case(B, K, C, seed, p=0.3):
    tag = f"edge_B{B}_K{K}_C{C}"
    return dict(u=recipe.sign_codes(B, K, seed, f"ddbh_eu_{tag}"), v=recipe.sign_codes(B, K, seed, f"ddbh_ev_{tag}"),
                lab=recipe.labels(B, C, seed, p=p, tag=f"ddbh_el_{tag}"))


def tied_tail_case(K=16, seed=5, empty_kept=False):
    """groups of 4 and 26 rows: row 0 has n_s = 4, n_d = 26 (a tail of 3).  v_4 .. v_9 are one code at inner product K - 4 with u_0, every
    other dissimilar v_j lies below: the whole tail is one tied value, with more ties beyond the cut.  empty_kept: the tied value and all
    four similar entries of row 0 are the integer 2, so BP = 2 and no similar entry is kept (the mean of nothing: NaN)."""
    sizes = [4, 26]
    B = sum(sizes)
    u, v = recipe.sign_codes(B, K, seed, "ddbh_tie_u"), recipe.sign_codes(B, K, seed, "ddbh_tie_v")
    top = 2 if empty_kept else K - 4
    near = u[0].copy()
    near[:(K - top) // 2] *= -1.0                                   # u_0 . near = top
    for j in range(4, B):
        if j < 10:
            v[j] = near
        elif float(u[0] @ v[j]) >= top:
            v[j] = -v[j]
    if empty_kept:
        v[:4] = near
    return dict(u=u, v=v, lab=group_labels(sizes))


def saturated_case(K=128, seed=9):
    """u = v: row 0 = (+1 .. +1) with class 0, row 1 its negation with class 0, rows 2-5 = row 0's code with class 1, then random rows.
    Row 0: S = {K, -K} (sMin = -K), mean D clamps to ub, BP_ds = ub - (ub + K) = -K, and its dissimilar entries K are hard with
    f = a c (K - BP_ds) = 2 a c K = -110 at K = 128: log(1 + e^-f) overflows float32 in the reference's form."""
    B = 16
    u = recipe.sign_codes(B, K, seed, "ddbh_sat_u")
    lab = np.zeros((B, 3), F32)
    u[0], u[1], u[2:6] = 1.0, -1.0, 1.0
    lab[0, 0] = lab[1, 0] = 1.0
    lab[2:6, 1] = 1.0
    lab[np.arange(6, B), np.arange(6, B) % 3] = 1.0
    return dict(u=u, v=u, lab=lab)
