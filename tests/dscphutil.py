"""Seeded DScPH cases shared by tests/golden/make_golden22.py and the tests, and a float64 restatement of the proxy-fusion (CPF) loss,
the step's quantisation terms and their gradients, written from the definition (reference train/DScPH/CPF_loss.py:24-54,
train/DScPH/hash_train.py:64-70):

  n(x) = x / max(|x|, 1e-12) per row;  c = n(h) n(W)^T per modality
  tp = 2 sum max(c, 0) Y + b;  lp = sum (1 - c) exp((1 - c) sp) Y;  ln = sum_{c > tau} (c - psi) exp((c - mu) sn) (1 - Y)
  L = 1 - tp / D, D = tp + lp + ln;  CPF = L(image) + L(text);  q = mean(sigma(z) (1 - sigma(z))), z = n(h)
  d L / d c = -2 (lp + ln) / D^2 Y [c >= 0] + tp / D^2 (-exp((1 - c) sp) Y + [c > tau] exp((c - mu) sn) (1 - Y))
  d n(h) = G n(W);  d n(W) = G_img^T n(h_img) + G_txt^T n(h_txt);  dx = (g - n (n . g)) / max(|x|, 1e-12)

The exponentials are detached in the reference and are constants here; clamp(min=0) passes its gradient at c == 0.  With cos=None
every decision (c >= 0, c > tau) is taken on the float64 cosines.  With cos= a given float32 [2, B, C] array the two masks are taken
on THAT array in its own arithmetic (tau rounded to float32, as torch compares a float32 tensor with a Python number); every value
stays float64.

Standard normal inputs put no cosine near 0.9, so the cases are built around the proxies: a row of h is a scaled unit proxy of a drawn
class plus noise of a drawn size, and that class is labelled positive for about half the rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipe  # noqa: E402

SCALARS = dict(tau=0.9, psi=0.7, sp=1.3, sn=1.3, mu=1.0, b=2.0)
QUANT_WEIGHT = 1.0
F32 = np.float32
# (B, K, C, seed): the first seed from 11 on whose case passes make_golden22.py's gap condition (--search)
CASES = [(1, 8, 1, 11), (5, 16, 3, 11), (33, 64, 24, 11), (64, 128, 80, 91), (130, 65, 21, 21)]
SPECIALS = ("none_above", "all_neg_above", "zero_labels", "row_ones", "zero_cos")


def _unit(x):
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    return x / n, n


def _unit_backward(g, x, xn, n):
    proj = np.where(np.sqrt((x * x).sum(1, keepdims=True)) > 1e-12, (xn * g).sum(1, keepdims=True), 0.0)
    return (g - xn * proj) / n


def around_proxies(B, K, C, seed, tag, lo=0.2, hi=0.8, p=0.15):
    """hi, ht [B, K], W [C, K], lab [B, C]: see the module docstring; noise sizes in (lo, hi) put the drawn class's cosine between
    1 / sqrt(1 + hi^2) and 1 / sqrt(1 + lo^2) - on either side of tau for the defaults"""
    rng = recipe._rng(seed, f"dscph_{tag}")
    W = recipe.features(C, K, seed, f"dscph_w_{tag}")
    Wn = W / np.sqrt((W * W).sum(1, keepdims=True))
    cls = rng.integers(0, C, size=B)
    lab = recipe.labels(B, C, seed, p=p, tag=f"dscph_lab_{tag}")
    lab[np.arange(B), cls] = (rng.random(B) < 0.5).astype(F32)
    out = []
    for _ in range(2):
        noise = rng.standard_normal((B, K))
        noise *= rng.uniform(lo, hi, size=(B, 1)) / np.sqrt((noise * noise).sum(1, keepdims=True))
        out.append((rng.uniform(0.5, 2.0, size=(B, 1)) * (Wn[cls] + noise)).astype(F32))
    return dict(hi=out[0], ht=out[1], W=W.astype(F32), lab=lab.astype(F32))


def dscph_case(B, K, C, seed):
    tag = f"B{B}_K{K}_C{C}"
    return dict(around_proxies(B, K, C, seed, tag), tag=tag)


def special_case(name, seed=5):
    """the cases the goldens hold besides CASES (B, K, C small)"""
    B, K, C = 6, 16, 4
    c = around_proxies(B, K, C, seed, name)
    if name == "none_above":                                      # plain features: every cosine is far below tau
        c["hi"], c["ht"] = recipe.features(B, K, seed, "dscph_na_i"), recipe.features(B, K, seed, "dscph_na_t")
    elif name == "all_neg_above":                                 # proxies and rows all near one direction: every cosine is above tau
        base = recipe.features(1, K, seed, "dscph_base")
        c["W"] = (base + 0.05 * recipe.features(C, K, seed, "dscph_an_w")).astype(F32)
        c["hi"] = (base + 0.05 * recipe.features(B, K, seed, "dscph_an_i")).astype(F32)
        c["ht"] = (base + 0.05 * recipe.features(B, K, seed, "dscph_an_t")).astype(F32)
    elif name == "zero_labels":
        c["lab"] = np.zeros((B, C), F32)
    elif name == "row_ones":
        c["lab"][2] = 1.0
    elif name == "zero_cos":                                      # rows on different axes: c[0, 0] == 0 exactly, on a positive label
        c["hi"][0] = 0.0
        c["hi"][0, 0] = 2.0
        c["W"][0] = 0.0
        c["W"][0, 1] = 0.5
        c["lab"][0, 0] = 1.0
    else:
        raise KeyError(name)
    return dict(c, tag=name)


def all_cases():
    return [dscph_case(*a) for a in CASES] + [special_case(n) for n in SPECIALS]


def sigma_var(z):
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1.0 - s), s


def cpf_step(hi, ht, W, lab, scalars=None, quant_weight=QUANT_WEIGHT, cos=None):
    """-> dict(L [2], q [2], cpf, step, cos [2, B, C] float64, pos / above [2, B, C] the two masks, gap, g_cpf / g_step = (d hi, d ht, d W)
    of the CPF part / of the whole step).  gap = the smallest of |c - tau| and |c| over both modalities, over the cosines that are not
    exactly zero (an exactly zero cosine is zero in float32 too: there is nothing to decide)"""
    s = dict(SCALARS, **(scalars or {}))
    h = [np.asarray(hi, np.float64), np.asarray(ht, np.float64)]
    W, Y = np.asarray(W, np.float64), np.asarray(lab, np.float64)
    B, K = h[0].shape
    Wn, nW = _unit(W)
    L, q, cs, pos, above, G, gq, units = [], [], [], [], [], [], [], []
    gap = np.inf
    for m in range(2):
        hn, nh = _unit(h[m])
        c = hn @ Wn.T
        nz = np.abs(c[c != 0.0])
        gap = min([gap] + ([float(nz.min()), float(np.abs(c - s["tau"]).min())] if nz.size else [float(np.abs(c - s["tau"]).min())]))
        if cos is None:
            p_m, a_m = c >= 0.0, c > s["tau"]
        else:
            given = np.asarray(cos[m])
            p_m, a_m = given >= given.dtype.type(0), given > given.dtype.type(s["tau"])
        e1, e2 = np.exp((1.0 - c) * s["sp"]), np.exp((c - s["mu"]) * s["sn"])
        tp = 2.0 * (np.where(p_m, c, 0.0) * Y).sum() + s["b"]
        lp = ((1.0 - c) * e1 * Y).sum()
        ln = (np.where(a_m, (c - s["psi"]) * e2, 0.0) * (1.0 - Y)).sum()
        D = tp + lp + ln
        L.append(1.0 - tp / D)
        G.append(-2.0 * (lp + ln) / D ** 2 * Y * p_m + tp / D ** 2 * (-e1 * Y + a_m * e2 * (1.0 - Y)))
        v, sg = sigma_var(hn)
        q.append(v.mean())
        gq.append(v * (1.0 - 2.0 * sg) / (B * K))
        cs.append(c); pos.append(p_m); above.append(a_m); units.append((hn, nh))
    g_w = _unit_backward(G[0].T @ units[0][0] + G[1].T @ units[1][0], W, Wn, nW)
    g_cpf = tuple(_unit_backward(G[m] @ Wn, h[m], *units[m]) for m in range(2)) + (g_w,)
    g_step = tuple(_unit_backward(G[m] @ Wn + quant_weight * gq[m], h[m], *units[m]) for m in range(2)) + (g_w,)
    cpf = L[0] + L[1]
    return dict(L=np.array(L), q=np.array(q), cpf=cpf, step=cpf + quant_weight * (q[0] + q[1]), cos=np.stack(cs), pos=np.stack(pos),
                above=np.stack(above), gap=gap, g_cpf=g_cpf, g_step=g_step)


STEP_GRAD_MAX_B = 33                                              # dscph.npz holds the whole step's gradients up to this batch


def step_grad(g, tag, side):
    """the reference's gradient of the whole step for `side` (gi, gt): stored for the small cases, else the sum of its two stored parts
    (the reference's own autograd of the CPF loss and of q_img + q_txt), in float64"""
    key = f"{tag}_step_{side}"
    return g[key].astype(np.float64) if key in g.files else g[f"{tag}_cpf_{side}"].astype(np.float64) + g[f"{tag}_q_{side}"]


# ---- the training trajectory (make_golden22.py and the GPU test): ddbhutil's tiny CLIP, heads, optimiser and batches, and the proxies
PROXY_SEED = 3


def traj_proxies():
    """the [C, K] start of the class proxies for the trajectory (both sides overwrite their xavier draw with it)"""
    import ddbhutil as dd
    import dchmtutil as du
    return recipe.features(du.C, dd.TRAJ_K, PROXY_SEED, "dscph_traj_w")


# ---- edges (the GPU test)
def edge_case(B, K, C, seed, p=0.1):
    return around_proxies(B, K, C, seed, f"edge_B{B}_K{K}_C{C}", p=p)
