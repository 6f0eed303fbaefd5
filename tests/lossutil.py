"""Plain torch statements of the loss and head operations behind csrc/losses.hip, heads_bwd.hip, heads2.hip, qmi.hip and msl.hip
(spl_*), written from the formulas in those files' header comments and the reference's loss files cited there, plus the inputs and
the case tables of tests/test_loss_edges_host.py and tests/test_gpu_loss_edges.py.  Imports no GPU code.

Every reference takes the tensors it differentiates first and computes in their dtype; `evaluate(fn, tensors, dtype)` makes the
leaves of that dtype, so the same formula runs in float64 (the reference) and in float32 on the CPU (`spread`: the e32 a float32
evaluation of the formula shows by itself).  Gradients come from autograd.

Inputs of the thresholded losses (HyP, DCHMT): relu / clamp make the gradient jump where a cosine or a distance crosses a threshold,
and a float32 kernel and a float64 reference may then legitimately disagree on an entry that sits on it.  So their rows are distinct
random sign vectors in {-1, +1}^K times a per-row magnitude: every cosine lies on the lattice (K - 2h) / K, every distance (at
magnitude 1) is 2 sqrt(h), and the thresholds are chosen off the lattice.  `*_guard` returns the smallest |value - threshold| over
every comparison of the float64 reference whose outcome changes a gradient; the host test asserts it is >= GUARD for every case."""
import math

import torch
import torch.nn.functional as F

GUARD = 1e-4


# ------------------------------------------------------------------------------------------------------------------ inputs
def gen(*key):
    """a generator seeded from the case's numbers"""
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def sign_rows(n, K, g, magnitudes=True):
    """n DISTINCT rows of {-1, +1}^K (float32), each times a magnitude in [0.5, 2] (or 1)"""
    if K <= 24:
        codes = torch.randperm(2 ** K, generator=g)[:n]
        bits = (codes[:, None] >> torch.arange(K)[None, :]) & 1
    else:
        bits = torch.randint(0, 2, (n, K), generator=g)
        assert torch.unique(bits, dim=0).shape[0] == n
    rows = (2 * bits - 1).float()
    if magnitudes:
        rows = rows * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
    return rows


def labels(B, C, p, g, no_empty_row=False):
    """Bernoulli(p) multi-hot rows; row 0 all-zero, row 1 carrying three ones (as test_hyp_loss_backward) and the LAST row the last two
    classes - multi-label and disjoint from row 1, so the one row of a last window / tile is part of the pair term; or - for the
    losses that divide by a row's positives - no all-zero row: an empty row gets class (row mod C)"""
    lab = (torch.rand(B, C, generator=g) < p).float()
    if no_empty_row:
        empty = torch.nonzero(lab.sum(1) == 0).flatten()
        lab[empty, empty % C] = 1.0
    else:
        lab[0] = 0
        lab[1, :3] = 1
        lab[B - 1] = 0
        lab[B - 1, C - 2:] = 1
    return lab


def evaluate(fn, tensors, dtype=torch.float64, upstream=1.0, which=0):
    """fn(*leaves) -> value or tuple of values; backward of upstream * value[which].  -> (values as floats, gradients)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    outs = out if isinstance(out, tuple) else (out,)
    (upstream * outs[which]).backward()
    return [float(o.detach()) for o in outs], [l.grad for l in leaves]


def spread(fn, tensors, upstream=1.0, which=0):
    """e32 of every output of `evaluate`: max |float32 - float64| / max |float64|, the value first, then each gradient"""
    v32, g32 = evaluate(fn, tensors, torch.float32, upstream, which)
    v64, g64 = evaluate(fn, tensors, torch.float64, upstream, which)
    e = [abs(v32[which] - v64[which]) / max(abs(v64[which]), 1e-300)]
    e += [float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)) for a, b in zip(g32, g64)]
    return e


# ------------------------------------------------------------------------------------------------------------------ HyP
def hyp_loss(x, y, p, label, thr, alpha):
    """HyP.forward (train/DSPH/loss.py:22-72); the dtype is that of x"""
    cos = F.normalize(x, dim=1) @ F.normalize(p, dim=1).T
    cos_t = F.normalize(y, dim=1) @ F.normalize(p, dim=1).T
    lab = label.to(x.dtype)
    P, Nn = (lab != 0).sum(), (lab == 0).sum()
    tot = ((1 - cos)[lab == 1].sum() + (1 - cos_t)[lab == 1].sum()) / P + (F.relu(cos - thr)[lab == 0].sum() + F.relu(cos_t - thr)[lab == 0].sum()) / Nn
    if alpha > 0:
        idx = lab.sum(1) > 1
        l_ = lab[idx]
        cs = l_ @ l_.T
        if (cs == 0).sum() > 0:
            xn, tn = F.normalize(x[idx], dim=1), F.normalize(y[idx], dim=1)
            Z = (cs == 0).sum()
            for s in (xn @ xn.T, tn @ tn.T, xn @ tn.T):
                tot = tot + (alpha * F.relu(s - thr))[cs == 0].sum() / Z
    return tot


def hyp_decisions(x, y, p, label, thr, alpha):
    """every cosine the float64 reference compares with thr -> (proxy cosines at label == 0, pair cosines at disjoint multi-label
    pairs or None)"""
    x, y, p, lab = x.double(), y.double(), p.double(), label.double()
    pn = F.normalize(p, dim=1)
    prox = torch.cat(((F.normalize(x, dim=1) @ pn.T)[lab == 0], (F.normalize(y, dim=1) @ pn.T)[lab == 0]))
    pair = None
    if alpha > 0:
        idx = lab.sum(1) > 1
        cs = lab[idx] @ lab[idx].T
        if (cs == 0).sum() > 0:
            xn, tn = F.normalize(x[idx], dim=1), F.normalize(y[idx], dim=1)
            pair = torch.cat([s[cs == 0] for s in (xn @ xn.T, tn @ tn.T, xn @ tn.T)])
    return prox, pair


def hyp_guard(x, y, p, label, thr, alpha):
    prox, pair = hyp_decisions(x, y, p, label, thr, alpha)
    every = prox if pair is None else torch.cat((prox, pair))
    return float((every - thr).abs().min())


# (B, K, C, alpha, p): the edge each one is there for is in the table of tests/test_gpu_loss_edges.py
HYP_THR = 0.05
HYP_CASES = [(65, 65, 5, 0.8, 0.3), (63, 130, 24, 0.8, 0.12), (129, 192, 70, 0.8, 0.04), (129, 192, 70, 0.0, 0.04), (130, 257, 24, 0.8, 0.12),
             (3, 512, 6, 0.8, None), (1024, 16, 24, 0.8, 0.1), (1025, 64, 24, 0.8, 0.1)]


def hyp_case(B, K, C, alpha, p):
    g = gen(1, B, K, C, int(alpha * 10))
    rows = sign_rows(2 * B + C, K, g)
    if p is None:                       # labels by hand: row 0 empty, rows 1 and 2 multi-label and disjoint
        lab = torch.zeros(B, C)
        lab[1, :3] = 1
        lab[2, 3:5] = 1
    else:
        lab = labels(B, C, p, g)
    return dict(x=rows[:B], y=rows[B:2 * B], prox=rows[2 * B:], lab=lab, thr=HYP_THR, alpha=alpha)


# ------------------------------------------------------------------------------------------------------------------ DCHMT
def dchmt_similarity(a, b, similarity):
    if similarity == "cosine":          # utils/utils.py:58-63: rows / |row| (no eps) unless the matrix is identically zero
        a = a / a.norm(dim=-1, keepdim=True) if bool((a != 0).any()) else a
        b = b / b.norm(dim=-1, keepdim=True) if bool((b != 0).any()) else b
        return 1 - a @ b.T
    return torch.cdist(a, b, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")     # zero distance -> zero gradient


def dchmt_loss(img, txt, label, output_dim, similarity, loss_type, vartheta, sim_threshold):
    """our_loss (train/DCHMT/hash_train.py:82-150) for the select head: three similarity_loss terms, each positive + negative mean"""
    same = ((label.double() @ label.double().T) > 0).to(img.dtype)
    thr = sim_threshold if sim_threshold != 0 else 0.05
    total = 0
    for a, b in ((img, txt), (img, img), (txt, txt)):
        s = dchmt_similarity(a, b, similarity)
        pos, neg = s * same, s * (1 - same)
        if similarity == "cosine":
            pos = pos.clamp(min=thr) - thr
            neg = (1 - same) - neg.clamp(max=1.0)
        else:
            maxv = float(output_dim * 2 * vartheta) ** 0.5
            neg = maxv * (1 - same) - neg.clamp(max=maxv)
        if loss_type == "l2":
            pos, neg = pos ** 2, neg ** 2
        total = total + pos.mean() + neg.mean()
    return total


def dchmt_decisions(img, txt, label, output_dim, similarity, vartheta, sim_threshold):
    """-> list of (values, threshold) the float64 reference compares: similar pairs against thr (cosine) or against 0 (euclidean,
    the zero-distance convention; exact zeros - a row with itself - are the same 0 in every precision and left out), dissimilar
    pairs against 1 (cosine) or maxv (euclidean)"""
    img, txt = img.double(), txt.double()
    same = (label.double() @ label.double().T) > 0
    thr = sim_threshold if sim_threshold != 0 else 0.05
    out = []
    for a, b in ((img, txt), (img, img), (txt, txt)):
        s = dchmt_similarity(a, b, similarity)
        if similarity == "cosine":
            out += [(s[same], thr), (s[~same], 1.0)]
        else:
            sp = s[same]
            out += [(sp[sp != 0], 0.0), (s[~same], float(output_dim * 2 * vartheta) ** 0.5)]
    return out


def dchmt_guard(img, txt, label, output_dim, similarity, loss_type, vartheta, sim_threshold):
    """l1: every comparison above flips a gradient between 0 and +-1/B^2.  l2: the hinges are squared, so the gradient is 0 on both
    sides of each threshold and 2 a - 2 b is smooth through zero distance: no comparison changes a gradient, the guard is infinite."""
    if loss_type == "l2":
        return math.inf
    return min(float((v - t).abs().min()) for v, t in dchmt_decisions(img, txt, label, output_dim, similarity, vartheta, sim_threshold)
               if v.numel())


# (B, D, C, similarity, loss_type, output_dim, vartheta, sim_threshold, p).  Cosine: 1 - cos = 2h / D against sim_threshold and 1 (l1:
# D odd, so never 1; 0.1 D / 2 is no integer for D = 65, and D = 100 takes 0.13).  Euclidean (magnitude 1): distance^2 = 4h against
# maxv^2 = 2 output_dim vartheta = 1026 (D = 512) and 514 (D = 257): near the typical 4h = 2D, so both sides are populated, and no
# multiple of 4.
DCHMT_CASES = [(65, 65, 70, "cosine", "l1", 32, 0.5, 0.1, 0.02), (33, 100, 24, "cosine", "l2", 50, 0.5, 0.13, 0.08),
               (17, 512, 5, "euclidean", "l2", 256, 1026 / 512, 0.1, 0.3), (130, 257, 24, "euclidean", "l1", 128, 514 / 256, 0.1, 0.08)]


def dchmt_case(B, D, C, similarity, loss_type, output_dim, vartheta, sim_threshold, p):
    g = gen(2, B, D, C)
    rows = sign_rows(2 * B, D, g, magnitudes=similarity == "cosine")
    return dict(img=rows[:B], txt=rows[B:], lab=labels(B, C, p, g), cfg=(output_dim, similarity, loss_type, vartheta, sim_threshold))


# ------------------------------------------------------------------------------------------------------------------ DNPH (TOMM)
def dnph_loss(hi, ht, pi, pt, prox, label, noise_i=None, noise_t=None, mrg=1.0, noise_weight=0.1):
    """DNPH_out.forward (train/DNPH_TOMM/loss.py:14-32) + the step's noise term (hash_train.py:65-81)
    -> (loss1 - noise_weight * noise, loss1 = p_loss + d_loss, noise)"""
    dt = hi.dtype
    la = torch.cat((label, label)).to(dt)
    f = F.normalize(torch.cat((hi, ht)), p=2, dim=-1)
    pn = F.normalize(prox, p=2, dim=-1)
    D = ((f[:, None, :] - pn[None, :, :]) ** 2).sum(-1) + mrg * (la == 1).to(dt)
    p_loss = -(la * F.log_softmax(-D, dim=1)).sum(1).mean()
    first = label.argmax(-1)                                   # of a multi-hot row: the first maximum
    d_loss = F.cross_entropy(pi, first) + F.cross_entropy(pt, first)
    loss1 = p_loss + d_loss
    if noise_i is None:
        return loss1, loss1, torch.zeros((), dtype=dt)
    noise = (hi * noise_i.to(dt)).sum(-1).mean() + (ht * noise_t.to(dt)).sum(-1).mean()
    return loss1 - noise_weight * noise, loss1, noise


# (B, K, C, noise, p)
DNPH_CASES = [(33, 65, 65, True, 0.05), (129, 512, 24, False, 0.12), (7, 257, 130, True, 0.03), (8, 64, 4096, False, 0.001)]


def dnph_case(B, K, C, noise, p):
    g = gen(3, B, K, C)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(hi=torch.tanh(r(B, K)), ht=torch.tanh(r(B, K)), pi=r(B, C), pt=r(B, C), prox=r(C, K) / 4, lab=labels(B, C, p, g),
             noise_i=None, noise_t=None)
    if noise:
        c["noise_i"], c["noise_t"] = (torch.where(r(B, K) >= 0, 1.0, -1.0) for _ in range(2))
    return c


# ------------------------------------------------------------------------------------------------------------------ QMI
def qmi_loss(x, t, label, eps=1e-8):
    """qmi_loss (train/DNpH_TMM/loss.py:5-72) with its defaults: cosine kernels, square clamp, M = B^2 / sum(D)"""
    xh, th = x / (x.norm(dim=1, keepdim=True) + eps), t / (t.norm(dim=1, keepdim=True) + eps)
    D = ((label.double() @ label.double().T) > 0).to(x.dtype)
    inv_m = D.sum() / D.shape[1] ** 2
    total = 0
    for S in (0.5 * (xh @ xh.T + 1), 0.5 * (th @ th.T + 1), 0.5 * (xh @ th.T + 1)):
        total = total + ((D * S - 1) ** 2 + inv_m * S ** 2).sum()
    return total


QMI_CASES = [(257, 65, 33, 0.05), (300, 257, 24, 0.08), (65, 1024, 512, 0.004)]          # (B, K, C, p)


def feature_case(tag, B, K, C, p):
    """tanh(randn) features for the losses without thresholds; no all-zero label row"""
    g = gen(tag, B, K, C)
    return dict(x=torch.tanh(torch.randn(B, K, generator=g)), y=torch.tanh(torch.randn(B, K, generator=g)),
                lab=labels(B, C, p, g, no_empty_row=True))


# ------------------------------------------------------------------------------------------------------------------ SPL (DHaPH)
def spl_loss(a, b, label, temperature, delta):
    """MSLoss.forward (train/DHaPH/MSLoss.py:13-33) with delta already formed (:23-27; 0 = not self-paced).  b may be a itself."""
    same = ((label.double() @ label.double().T) > 0).to(a.dtype)
    s = F.normalize(a, dim=1) @ F.normalize(b, dim=1).T
    e = torch.exp(s / temperature)
    sd = s.detach()                                            # the self-paced weights are constants
    P = (same * e * torch.exp((-1 - sd) * (delta / 4))).sum(1)
    Nn = ((1 - same) * e * torch.exp((-1 + sd) * delta)).sum(1)
    return -torch.log(P / (P + Nn)).mean()


SPL_TEMPERATURE = 0.3
SPL_CASES = [(257, 65, 24, 0.5, 0.08), (300, 513, 80, 1.0, 0.03), (65, 1024, 1024, 0.25, 0.002)]     # (B, K, C, delta, p)


# ------------------------------------------------------------------------------------------------------------------ LinearHash
def linear_act(x, w, b, act, mask, p_drop):
    """y = act((x W^T + b) * mask * keep), keep = 1 / (1 - p) (model/modelbase.py:25-35); act 0 none, 1 tanh, 2 relu"""
    z = x @ w.T + b
    if mask is not None:
        z = z * mask.to(x.dtype) / (1.0 - p_drop)
    return torch.tanh(z) if act == 1 else (torch.relu(z) if act == 2 else z)


LINEAR_SHAPES = [(67, 5, 260), (9, 64, 513)]                 # (M, N, K)
LINEAR_DROP = 0.2


def linear_case(M, N, K, act, use_mask):
    g = gen(6, M, N, K, act, use_mask)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(M, K), w=r(N, K) * 0.05, b=r(N), dy=r(M, N), mask=(torch.rand(M, N, generator=g) >= LINEAR_DROP).float() if use_mask else None)


# ------------------------------------------------------------------------------------------------------------------ BatchNorm1d
def batchnorm_train(x, w, b, eps):
    """nn.BatchNorm1d in training mode: batch mean and BIASED variance"""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def batchnorm_running(x, running_mean, running_var, momentum):
    """the module's side effect: (1 - momentum) old + momentum batch statistic, the variance UNBIASED"""
    B = x.shape[0]
    mean = x.mean(0)
    unbiased = ((x - mean) ** 2).sum(0) / max(B - 1, 1)
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * unbiased


BATCHNORM_SHAPES = [(65, 7), (3, 130), (256, 513)]           # (B, d)
BATCHNORM_EPS, BATCHNORM_MOMENTUM = 1e-5, 0.1


def batchnorm_case(B, d):
    g = gen(7, B, d)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(B, d) * 2 + 0.5, w=1 + 0.2 * r(d), b=0.1 * r(d), dy=r(B, d), rm=0.3 * r(d), rv=1 + 0.5 * torch.rand(d, generator=g))


# ------------------------------------------------------------------------------------------------------------------ problems
UPSTREAM = {"hyp": 1.7, "dchmt": 1.7, "dnph": 2.0, "qmi": 2.0, "spl": 2.0}      # the factor on the loss before backward()


def problem(family, case, variant=None):
    """-> (c, fn, tensors, names): the case's inputs c, the scalar fn of the differentiated tensors, those tensors and their names.
    variant: spl "same" (a is b) / "cross"."""
    if family == "hyp":
        c = hyp_case(*case)
        return c, (lambda x, y, p: hyp_loss(x, y, p, c["lab"], c["thr"], c["alpha"])), [c["x"], c["y"], c["prox"]], ["dx", "dy", "dproxies"]
    if family == "dchmt":
        c = dchmt_case(*case)
        return c, (lambda i, t: dchmt_loss(i, t, c["lab"], *c["cfg"])), [c["img"], c["txt"]], ["dimg", "dtxt"]
    if family == "dnph":
        c = dnph_case(*case)
        fn = lambda hi, ht, pi, pt, prox: dnph_loss(hi, ht, pi, pt, prox, c["lab"], c["noise_i"], c["noise_t"], 1.0, 0.1)
        return c, fn, [c[k] for k in ("hi", "ht", "pi", "pt", "prox")], ["dhash_img", "dhash_txt", "dpre_img", "dpre_txt", "dproxies"]
    if family == "qmi":
        c = feature_case(4, *case)
        return c, (lambda x, t: qmi_loss(x, t, c["lab"])), [c["x"], c["y"]], ["dimg", "dtxt"]
    if family == "spl":
        B, K, C, delta, p = case
        c = feature_case(5, B, K, C, p)
        if variant == "same":
            return c, (lambda a: spl_loss(a, a, c["lab"], SPL_TEMPERATURE, delta)), [c["x"]], ["da"]
        return c, (lambda a, b: spl_loss(a, b, c["lab"], SPL_TEMPERATURE, delta)), [c["x"], c["y"]], ["da", "db"]
    raise KeyError(family)


CASES = {"hyp": HYP_CASES, "dchmt": DCHMT_CASES, "dnph": DNPH_CASES, "qmi": QMI_CASES, "spl": SPL_CASES}
