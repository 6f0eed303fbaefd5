"""Seeded MSCH cases shared by tests/golden/make_golden21.py and the tests, and a float64 restatement of the all-triplets margin loss and
its gradients, written from the definition (reference train/DPSIH/Loss.py:78-137, the step's sum :61-62):

  n(x) = x / max(|x|, 1e-12) per row with `normalize`, x otherwise;  s = -n(u) n(v)^T
  same = (y y^T > 0) without its diagonal; diff = not (y y^T > 0), taken before the diagonal leaves.  The reference clears the diagonal
  of every square mask (:107-108), and the cross-modal call of a step is square too: it loses its diagonal as the intra-modal one does.
  eligible (a, p, n): same[a, p] and diff[a, n];  tm = s_an - s_ap;  active: tm <= m ("all"), 0 < tm <= m ("semi-hard")
  loss = sum_active relu((s_ap - s_an) + m) / count;  count = 0: loss 0 and zero gradients
  coef[a, p] = +#{active n: violation > 0}, coef[a, n] = -#{active p: violation > 0};  d loss / d s = coef / count

It walks anchor by anchor over a [positives, negatives] block (never [B, B, B]).  With s=None every value is float64.  With s= a given
similarity matrix the triplets are decided in THAT matrix's arithmetic (float32 differences for a float32 matrix, as the reference and
the kernel decide them); sums and gradients stay float64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipe  # noqa: E402

# (B, K, C, seed, normalisations): the seeds are the first from 91 on whose cases (both rules, both modes, every listed normalisation)
# pass make_golden21.py's gap condition.  At B = 64 the smallest gap is near 1e-5 and no seed up to 6000 passes with AND without
# normalisation: that case is committed without it, which is what DPSIH runs (train/DPSIH/Loss.py:39)
CASES = [(5, 8, 3, 91, (False, True)), (33, 16, 5, 94, (False, True)), (64, 16, 5, 1672, (False,))]
RULES = ("all", "semi-hard")
MODES = ("intra", "cross")
MARGIN, SCALE = 0.25, 100.0
F32 = np.float32


def msch_case(B, K, C, seed, p=0.3):
    tag = f"B{B}_K{K}_C{C}"
    return dict(tag=tag, u=np.tanh(recipe.features(B, K, seed, f"msch_u_{tag}")), v=np.tanh(recipe.features(B, K, seed, f"msch_v_{tag}")),
                lab=recipe.labels(B, C, seed, p=p, tag=f"msch_lab_{tag}"))


def _unit(x, normalize):
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12) if normalize else np.ones((x.shape[0], 1))
    return x / n, n


def _unit_backward(g, x, xn, n, normalize):
    if not normalize:
        return g
    proj = np.where(np.sqrt((x * x).sum(1, keepdims=True)) > 1e-12, (xn * g).sum(1, keepdims=True), 0.0)
    return (g - xn * proj) / n


def msc_loss(u, v, y, margin=MARGIN, rule="all", normalize=False, s=None):
    """-> dict(loss, count, coef int64 [B, B], du, dv, gap, s): du, dv the gradients of the two roles (u is v: their sum is the
    gradient); gap = the smallest |tm - m| over the eligible triplets, under semi-hard also the smallest |tm| (inf without any)"""
    assert rule in RULES
    u, v, y = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(y, np.float64)
    B = u.shape[0]
    un, nu = _unit(u, normalize)
    vn, nv = _unit(v, normalize)
    s = -(un @ vn.T) if s is None else np.asarray(s)
    m = s.dtype.type(margin)
    sim = (y @ y.T) > 0
    same, diff = sim & ~np.eye(B, dtype=bool), ~sim
    coef = np.zeros((B, B), np.int64)
    total, count, gap = 0.0, 0, np.inf
    for a in range(B):
        P, N = np.flatnonzero(same[a]), np.flatnonzero(diff[a])
        if P.size == 0 or N.size == 0:
            continue
        ap, an = s[a, P][:, None], s[a, N][None, :]
        tm = an - ap
        gap = min(gap, float(np.abs(tm.astype(np.float64) - float(m)).min()))
        act = tm <= m
        if rule == "semi-hard":
            act &= tm > 0
            gap = min(gap, float(np.abs(tm).min()))
        viol = (ap - an) + m
        strict = act & (viol > 0)
        count += int(act.sum())
        total += float(np.where(strict, viol, 0).astype(np.float64).sum())
        coef[a, P] = strict.sum(1)
        coef[a, N] = -strict.sum(0)
    if count == 0:
        return dict(loss=0.0, count=0, coef=coef, du=np.zeros_like(u), dv=np.zeros_like(v), gap=gap, s=s)
    G = coef / count                                                # d loss / d s;  s = -un vn^T
    du = _unit_backward(-G @ vn, u, un, nu, normalize)
    dv = _unit_backward(-G.T @ un, v, vn, nv, normalize)
    return dict(loss=total / count, count=count, coef=coef, du=du, dv=dv, gap=gap, s=s)


def step_loss(hi, ht, y, margin=MARGIN, rule="all", scale=SCALE, symmetric=False):
    """scale (L(hi, hi) + L(ht, ht) + L(hi, ht) [+ L(ht, hi)]) -> loss, d/dhi, d/dht"""
    a, b, c = msc_loss(hi, hi, y, margin, rule), msc_loss(ht, ht, y, margin, rule), msc_loss(hi, ht, y, margin, rule)
    loss, gi, gt = a["loss"] + b["loss"] + c["loss"], a["du"] + a["dv"] + c["du"], b["du"] + b["dv"] + c["dv"]
    if symmetric:
        d = msc_loss(ht, hi, y, margin, rule)
        loss, gi, gt = loss + d["loss"], gi + d["dv"], gt + d["du"]
    return scale * loss, scale * gi, scale * gt


# ---- the training trajectory (make_golden21.py and the GPU test): ddbhutil's tiny CLIP, heads, optimiser and batches
TRAJ_STRIDE = 16


def cut(a):
    """dchmtutil.cut, and of a long parameter every sixteenth of what that keeps: the fixture stays at tens of KB"""
    import dchmtutil as du
    a = du.cut(a)
    return a[::TRAJ_STRIDE].copy() if a.size > 2000 else a


# ---- edges (the GPU test)
def edge_case(B, K, C, seed, p=0.3, signs=False):
    tag = f"edge_B{B}_K{K}_C{C}"
    if signs:
        u, v = recipe.sign_codes(B, K, seed, f"msch_eu_{tag}"), recipe.sign_codes(B, K, seed, f"msch_ev_{tag}")
    else:
        u, v = np.tanh(recipe.features(B, K, seed, f"msch_eu_{tag}")), np.tanh(recipe.features(B, K, seed, f"msch_ev_{tag}"))
    return dict(u=u, v=v, lab=recipe.labels(B, C, seed, p=p, tag=f"msch_el_{tag}"))


def group_labels(sizes):
    """one class per group of consecutive rows"""
    lab = np.zeros((sum(sizes), len(sizes)), F32)
    lab[np.arange(sum(sizes)), np.repeat(np.arange(len(sizes)), sizes)] = 1.0
    return lab


def tie_case(K=16):
    """Codes in {-1, +1} whose inner products with anchor 0 are chosen: groups of 4 (rows 0-3) and 8 (rows 4-11).  With s = -u v^T and
    the integer margin 4, anchor 0 has positives at s = -8 (v_1), -4 (v_2) and 0 (v_3) and negatives at s = -8 (v_4, v_5), -4 (v_6, v_7),
    0 (v_8, v_9) and 4 (v_10, v_11): tm = s_an - s_ap takes the values m = 4 and 0 exactly, several times each.  u = v off row 0's
    partners does not matter: rows 1 .. 11 of u are the same codes, so the other anchors have integer ties of their own."""
    def code(dot):                                                  # a code with inner product `dot` against (+1 .. +1)
        c = np.ones(K, F32)
        c[:(K - dot) // 2] = -1.0
        return c
    v = np.stack([code(16)] + [code(d) for d in (8, 4, 0)] + [code(d) for d in (8, 8, 4, 4, 0, 0, -4, -4)])
    return dict(u=v.copy(), v=v, lab=group_labels([4, 8]), margin=4.0)
