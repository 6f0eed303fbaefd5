"""Seeded DDWSH cases shared by tests/golden/make_golden23.py and the tests, and a float64 restatement of the distance-weighted sampler and
the margin loss with per-class boundaries, written from the definition (reference train/DDWSH/loss.py:16-128, the step's sum
train/DDWSH/hash_train.py:68):

  x^ = x / max(|x|, 1e-12) per row, y^ likewise;  D_ij = max(|x^_i - y^_j|, 1e-8), the difference taken directly
  mining matrix, "distances" (what the reference runs: it hands the miner D as its batch): M_ij = max(sqrt(max(|D_i: - D_j:|^2, 1e-4)), cutoff),
  dim = B;  "embeddings": M = max(D, cutoff), dim = K
  anchor i: pos_j = (Y_j . Y_i > 0); valid when sum(pos) > 1 and sum(pos) < B
  log w_j = (2 - dim) log M_ij - ((dim - 3) / 2) log max(1 - M_ij^2 / 4, 1e-8), 0 on pos before the maximum; w = exp(log w - max), 0 on pos
  negative: the first j with cdf_j > u_n total over the ascending running sum of w (the last j of positive weight if there is none);
  positive: the floor(u_p n)-th of the n positives other than i, in index order
  beta_i = sum_c Y_ic beta_c / sum_c Y_ic;  pos_i = relu(D[i, p_i] - beta_i + m), neg_i = relu(beta_i - D[i, n_i] + m)
  count = #{i: pos_i > 0 or neg_i > 0};  loss = sum (pos + neg) / max(count, 1)

With D=None every value is float64.  With D= a given distance matrix the relu thresholds are decided in THAT matrix's arithmetic
(float32 differences against a float32 beta_i for a float32 matrix, as the reference and the kernel decide them); sums and gradients
stay float64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipe  # noqa: E402

F32 = np.float32
MARGIN, BETA, CUTOFF = 0.2, 1.2, 0.5
SPACES = ("distances", "embeddings")
MODES = ("intra", "cross")
# (B, K, C, seed, label density).  The sizes are the issue's; the density is chosen so that most anchors have at least 2 other positives
# and at least 4 eligible negatives (B = 5 cannot: an anchor with 2 other positives has 2 negatives left), and the seeds are the first
# from 101 on whose cases (both modes, the step's three calls) pass make_golden23.py's gap condition with at least B / 2 valid anchors.
CASES = [(5, 8, 3, 103, 0.4), (12, 16, 4, 101, 0.3), (26, 16, 5, 101, 0.25), (33, 16, 5, 101, 0.25), (65, 128, 70, 101, 0.04)]
# max |w / sum w - the reference's q| over the valid anchors, the float64 restatement against the reference's float32 run
# (make_golden23.py prints them; tests/test_ddwsh_host.py measures them again; tests/test_gpu_ddwsh.py allows the kernel twice the
# CASE's figure, the largest of its three, and prints the mode's own next to what the kernel shows: in the `embeddings` space, where
# no diagonal enters, the kernel's float32 distances alone put it at 0.4 .. 2.3 times the mode's own figure).
# Intra-modal calls above 25 rows carry the reference's own diagonal of D (7e-4 .. 9e-4 where the direct form gives the 1e-8 clamp).
Q_DEV = {"B5_K8_C3": dict(intra=1.75e-7, cross=2.52e-6, emb=2.34e-7), "B12_K16_C4": dict(intra=2.04e-6, cross=2.65e-5, emb=5.73e-7),
         "B26_K16_C5": dict(intra=8.31e-4, cross=2.81e-5, emb=9.31e-7), "B33_K16_C5": dict(intra=1.12e-3, cross=6.30e-5, emb=3.95e-7),
         "B65_K128_C70": dict(intra=2.15e-3, cross=2.35e-3, emb=3.17e-6)}
BETA_SEED = 5


def case_beta(C, seed=BETA_SEED):
    """per-class boundaries away from the constant initial value, so that the average over an anchor's labels matters"""
    return (BETA + 0.1 * recipe._rng(seed, f"ddwsh_beta_{C}").standard_normal(C)).astype(F32)


def ddwsh_case(B, K, C, seed, p):
    tag = f"B{B}_K{K}_C{C}"
    return dict(tag=tag, seed=seed, x=np.tanh(recipe.features(B, K, seed, f"ddwsh_x_{tag}")), y=np.tanh(recipe.features(B, K, seed, f"ddwsh_y_{tag}")),
                lab=recipe.labels(B, C, seed, p=p, tag=f"ddwsh_lab_{tag}"), beta=case_beta(C))


def group_labels(sizes, C=None):
    """one class per group of consecutive rows"""
    lab = np.zeros((sum(sizes), C or len(sizes)), F32)
    lab[np.arange(sum(sizes)), np.repeat(np.arange(len(sizes)), sizes)] = 1.0
    return lab


def special_cases():
    """built by hand: an anchor with no other positive (row 0 of `lonely`), an anchor that shares a label with every item (row 0 of
    `shares_all`), a batch with no valid anchor at all (`no_anchor`: every item its own class)"""
    out = []
    for name, lab in (("lonely", group_labels([1, 3, 3])), ("shares_all", None), ("no_anchor", group_labels([1] * 6))):
        if lab is None:
            lab = group_labels([4, 3], 3)
            lab[0] = 1.0                                            # row 0 carries every class
        B, C = lab.shape
        tag = f"{name}_B{B}_K8_C{C}"
        out.append(dict(tag=tag, seed=11, x=np.tanh(recipe.features(B, 8, 11, f"ddwsh_x_{tag}")), y=np.tanh(recipe.features(B, 8, 11, f"ddwsh_y_{tag}")),
                        lab=lab, beta=case_beta(C)))
    return out


def all_cases():
    return [ddwsh_case(*c) for c in CASES] + special_cases()


# ---- distances and the mining matrix
def _unit(x):
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    return x / n, n


def _sqdist(a, b):
    """sum_k (a_ik - b_jk)^2 in float64.  Small shapes take the difference directly; above 4M differences the expansion
    n_i + n_j - 2 a . b is used: in float64 its cancellation error is about 1e-16 (|a_i|^2 + |b_j|^2), at most 1e-12 for the rows of
    a distance matrix at B = 1024, against squared distances that are clamped at 1e-4 and lie near 1"""
    if a.shape[0] * b.shape[0] * a.shape[1] <= 1 << 22:
        d = a[:, None, :] - b[None, :, :]
        return (d * d).sum(2)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)


def distances(x, y):
    """D [B, B] float64 = max(|x^_i - y^_j|, 1e-8), the difference taken directly: an intra-modal diagonal is the clamp exactly"""
    xn, yn = _unit(np.asarray(x, np.float64))[0], _unit(np.asarray(y, np.float64))[0]
    D = np.maximum(np.sqrt(_sqdist(xn, yn)), 1e-8)
    if x is y:
        np.fill_diagonal(D, 1e-8)                                  # (the expansion of a large case leaves rounding there)
    return D


def mining_matrix(D, K, cutoff=CUTOFF, space="distances"):
    """-> (M float64 [B, B], dim)"""
    assert space in SPACES
    D = np.asarray(D, np.float64)
    if space == "embeddings":
        return np.maximum(D, cutoff), K
    return np.maximum(np.sqrt(np.maximum(_sqdist(D, D), 1e-4)), cutoff), D.shape[0]


def positives(lab):
    """pos [B, B] bool (the diagonal included where the row has a label) and the valid flag per anchor"""
    lab = np.asarray(lab, np.float64)
    pos = (lab @ lab.T) > 0
    n = pos.sum(1)
    return pos, (n > 1) & (n < lab.shape[0])


def sphere_weights(M, lab, dim):
    """w float64 [B, B]: exp(log w - max) with zeros on the positives; zero rows for anchors that are not valid"""
    pos, valid = positives(lab)
    M = np.asarray(M, np.float64)
    logw = (2.0 - dim) * np.log(M) - ((dim - 3.0) / 2.0) * np.log(np.maximum(1.0 - 0.25 * M * M, 1e-8))
    logw[pos] = 0.0
    w = np.exp(logw - logw.max(1, keepdims=True))
    w[pos] = 0.0
    w[~valid] = 0.0
    return w


def pick_negative(w_row, u):
    """-> (j, margin): the inverse-cdf pick on the ascending running sum, and how far u total lies from the nearest cdf boundary
    as a fraction of the total"""
    cdf = np.cumsum(np.asarray(w_row, np.float64))
    total = cdf[-1]
    target = float(u) * total
    hit = np.flatnonzero(cdf > target)
    j = int(hit[0]) if hit.size else int(np.flatnonzero(np.asarray(w_row) > 0)[-1])
    return j, float(np.abs(cdf - target).min() / total)


def pick_positive(pos_row, i, u):
    cand = np.flatnonzero(pos_row & (np.arange(pos_row.size) != i))
    return int(cand[min(int(float(u) * cand.size), cand.size - 1)])


def mine(w, lab, uniforms):
    """-> (triplets int32 [B, 2] = (positive, negative) or (-1, -1), the smallest boundary margin per anchor (inf where not valid))"""
    pos, valid = positives(lab)
    B = pos.shape[0]
    trip, margin = np.full((B, 2), -1, np.int32), np.full(B, np.inf)
    for i in np.flatnonzero(valid):
        if not w[i].sum() > 0:
            continue
        n, margin[i] = pick_negative(w[i], uniforms[i, 1])
        trip[i] = (pick_positive(pos[i], i, uniforms[i, 0]), n)
    return trip, margin


# ---- the loss on given triplets
def margin_loss(x, y, lab, beta, trip, margin=MARGIN, D=None):
    """-> dict(loss, count, dx, dy (the gradients of the two roles: x is y -> their sum is the gradient), dbeta, gap, D).
    gap: the smallest |D_ap - beta_i + m| and |beta_i - D_an + m| over the triplets (inf without any)"""
    x, y, lab = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(lab, np.float64)
    beta = np.asarray(beta, np.float64)
    (xn, nx), (yn, ny) = _unit(x), _unit(y)
    exact = distances(x, y)
    Dd = exact if D is None else np.asarray(D)
    kind = Dd.dtype.type
    B = x.shape[0]
    dD, dbeta = np.zeros((B, B)), np.zeros_like(beta)
    total, count, gap, rows = 0.0, 0, np.inf, []
    for i in range(B):
        p, n = int(trip[i, 0]), int(trip[i, 1])
        if p < 0 or n < 0:
            continue
        bi = kind((lab[i] * beta).sum() / lab[i].sum())
        lp, ln = (Dd[i, p] - bi) + kind(margin), (bi - Dd[i, n]) + kind(margin)
        gap = min(gap, abs(float(lp)), abs(float(ln)))
        fp, fn = lp > 0, ln > 0
        total += (float(lp) if fp else 0.0) + (float(ln) if fn else 0.0)
        count += int(fp or fn)
        rows.append((i, p, n, fp, fn))
    c = max(count, 1)
    for i, p, n, fp, fn in rows:
        if fp and Dd[i, p] > 1e-8:
            dD[i, p] += 1.0 / c
        if fn and Dd[i, n] > 1e-8:
            dD[i, n] -= 1.0 / c
        dbeta += (float(fn) - float(fp)) / c * lab[i] / lab[i].sum()
    G = dD / exact                                                  # d loss / d D / D;  d D_ij / d x^_i = (x^_i - y^_j) / D_ij
    gx = G.sum(1, keepdims=True) * xn - G @ yn
    gy = G.sum(0)[:, None] * yn - G.T @ xn
    back = lambda g, u, nrm: (g - u * (u * g).sum(1, keepdims=True)) / nrm
    return dict(loss=total / c, count=count, dx=back(gx, xn, nx), dy=back(gy, yn, ny), dbeta=dbeta, gap=gap, D=exact)


def step_loss(hi, ht, lab, beta, trips, margin=MARGIN):
    """L(hi) + L(ht) + L(hi, y=ht) on trips [3, B, 2] -> loss, d/dhi, d/dht, d/dbeta"""
    a, b, c = (margin_loss(u, v, lab, beta, tr, margin) for (u, v), tr in zip(((hi, hi), (ht, ht), (hi, ht)), trips))
    return (a["loss"] + b["loss"] + c["loss"], a["dx"] + a["dy"] + c["dx"], b["dx"] + b["dy"] + c["dy"], a["dbeta"] + b["dbeta"] + c["dbeta"])


def case_uniforms(n, B, seed, tag="u"):
    """the committed uniforms of the sampler tests: float32 [n, B, 2] in [0, 1)"""
    return recipe._rng(seed, f"ddwsh_uniforms_{tag}_{n}_{B}").random((n, B, 2)).astype(F32).clip(0.0, np.nextafter(F32(1), F32(0)))


# ---- the training trajectory (make_golden23.py and the GPU test): ddbhutil's tiny CLIP, heads, optimiser and batches
TRAJ_NP_SEED = 23                                                   # np.random.seed(TRAJ_NP_SEED + step) before a step's three calls


def traj_beta(C):
    return case_beta(C, BETA_SEED + 1)


# ---- edges (the GPU test)
def edge_case(B, K, C, seed, p=0.1):
    tag = f"edge_B{B}_K{K}_C{C}"
    return dict(tag=tag, x=np.tanh(recipe.features(B, K, seed, f"ddwsh_ex_{tag}")), y=np.tanh(recipe.features(B, K, seed, f"ddwsh_ey_{tag}")),
                lab=recipe.labels(B, C, seed, p=p, tag=f"ddwsh_el_{tag}"), beta=case_beta(C))
