"""Plain torch statements of the operations behind csrc/mith.hip and of the DMsH-LN multi-similarity loss of csrc/msl.hip, written
from those files' header comments and the reference's formulas cited there (model/MITH.py:249-376, train/MITH/hash_train.py:80-201,
train/DMsH_LN/MSLOSS.py:13-57), plus the inputs and the case tables of tests/test_mith_edges_host.py and
tests/test_gpu_mith_edges.py.  Imports no GPU code.  `gen`, `evaluate`, `spread` and `GUARD` are those of tests/lossutil.py.

Every reference computes in the dtype of the tensors it differentiates, so the same formula runs in float64 (the reference) and in
float32 on the CPU (the e32 of the formula itself).  Gradients come from autograd except where it is ambiguous: the norm of a row at
or under the eps clamp (l2norm_dx states the gradient; the multi-similarity loss holds the clamped denominator constant).

Settled decisions.  LocalizedTokenAggregation compares raw inputs only (v > 0, >= the top_k-th value, == -inf): on the same float32
similarities the float64 reference takes the same decisions, and ties are built by copying values.  The Bayesian loss keeps every
|bank . batch| at least 1 away from the +-64 clamp (bayes_guard) with labels in {0, 1}.  mith_mix keeps |v| >= GUARD or v exactly 0
by construction.  The multi-similarity loss mines relative to each row's extrema: its features are sign vectors in {-1, +1}^K and
its label codes sign vectors of odd length, so every product S_ij is an integer held exactly in float32, code_i . code_j is never 0
and each decision hinges on where 0.1 |S_i| falls between integers; msl_guard returns the smallest distance of any compared
similarity from its threshold and the seeds in MSL_CASES were picked for guard >= GUARD (tests/test_mith_edges_host.py asserts it)."""
import math

import torch
import torch.nn.functional as F

from lossutil import GUARD, evaluate, gen, spread  # noqa: F401

NEG_INF = float("-inf")
LOSS_BOUND, TENSOR_BOUND = 1e-5, 1e-4       # the bound of tests/test_gpu_loss_edges.py, shared with the sensitivity checks of the host test


# ------------------------------------------------------------------------------------------------------------------ measures
def loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def of_max(got, ref):
    """max |got - ref| / max |ref| (NaN anywhere: inf); an all-zero reference: 0 if got is all zero too, else inf"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    if bool(torch.isnan(got).any()):
        return math.inf
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if not bool(got.any()) else math.inf
    return float((got - ref).abs().max()) / top


def per_row(got, ref):
    """the worst row of of_max, every row relative to its own maximum"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return max(of_max(g, r) for g, r in zip(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])))


# ------------------------------------------------------------------------------------------------------------------ LTA
def lta_weights(sim, kpm, l0, L, top_k, dtype=torch.float64, tie="ge", nan_to_zero=True, use_l0=True):
    """steps 1-3 of LocalizedTokenAggregation.forward (model/MITH.py:343-367), batch-major: sim [B, Ltot, K] (tokens l0 .. l0 + L take
    part), kpm [B, L] bool or None -> (w [B, L, K], info).  Padded and non-positive entries become -inf; a token keeps the entries >=
    its top_k-th largest value counted WITH multiplicity (ties keep more; fewer than top_k positives: the value is -inf and all are
    kept); softmax over the tokens of every concept; a concept without a surviving token is NaN upstream and replaced by 0.
    tie / nan_to_zero / use_l0 state the ways a kernel could get this wrong ("gt": > for >=; "distinct": the top_k-th DISTINCT value)."""
    start = l0 if use_l0 else 0
    s = sim[:, start:start + L].to(dtype)
    if kpm is not None:
        s = torch.where(kpm.bool()[:, :, None], torch.full_like(s, NEG_INF), s)
    s = torch.where(s > 0, s, torch.full_like(s, NEG_INF))
    positives = (s > 0).sum(-1)
    srt = torch.sort(s, dim=-1, descending=True).values
    if tie == "distinct":
        first = torch.ones_like(srt, dtype=torch.bool)
        first[..., 1:] = srt[..., 1:] != srt[..., :-1]
        rank = first.cumsum(-1)                                   # 1-based rank among the distinct values
        kth = torch.where((rank == top_k) & first, srt, torch.full_like(srt, NEG_INF)).max(-1, keepdim=True).values
    else:
        kth = srt[..., top_k - 1:top_k]
    keep = (s > kth) if tie == "gt" else (s >= kth)
    s = torch.where(keep, s, torch.full_like(s, NEG_INF))
    kept = (s > 0).sum(-1)
    dead = (s == NEG_INF).all(1)                                  # [B, K]: no token survives in this concept
    w = torch.softmax(s, dim=1)
    if nan_to_zero:
        w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return w, dict(positives=positives, kept=kept, dead=dead, mask=s > 0)


def lta_forward(tokens, sim, kpm, l0, L, top_k, **how):
    """merge[b, k, :] = sum_l w[b, l, k] tokens[b, l0 + l, :] (:370-375); the dtype is that of tokens.  The weights carry no gradient."""
    w, _ = lta_weights(sim, kpm, l0, L, top_k, dtype=tokens.dtype, **how)
    start = l0 if how.get("use_l0", True) else 0
    return torch.einsum("blk,bld->bkd", w, tokens[:, start:start + L])


# (B, Ltot, l0, L, K, D, top_k, kpm): the edge each one is there for is in the table of tests/test_gpu_mith_edges.py
LTA_CASES = [(3, 80, 0, 80, 128, 260, 8, True), (2, 50, 1, 49, 16, 512, 8, False), (5, 7, 0, 7, 4, 65, 1, True), (2, 9, 2, 6, 12, 64, 3, True)]
LTA_HAND = LTA_CASES[3]


def _hand_sim():
    """sample 0 of the hand-built case, its six tokens of the slice: every value a literal, ties are the SAME literal"""
    n = -0.5
    rows = [
        [0.9, 0.8, 0.7, 0.7, 0.3, n, n, n, n, n, n, n],          # third largest 0.7 twice: keeps 4; column 4 (0.3) is cut
        [n, n, n, n, n, 0.6, 0.5, 0.4, 0.4, 0.4, n, n],          # third largest 0.4 three times: keeps 5
        [0.2, n, n, n, n, n, n, n, n, n, 0.3, n],                # two positives < top_k: both kept
        [n, -0.1, n, 0.0, n, n, -0.9, n, n, n, n, n],            # none (0.0 is not positive)
        [0.65, 0.65, 0.6, 0.1, n, n, n, n, n, n, n, n],          # the largest twice: the third WITH multiplicity is 0.6, column 3 is cut
        [0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1],      # masked by the key padding
    ]
    return torch.tensor(rows, dtype=torch.float32)


def lta_case(B, Ltot, l0, L, K, D, top_k, with_kpm):
    g = gen(11, B, Ltot, l0, L, K, D, top_k)
    r = lambda *s: torch.randn(*s, generator=g)
    tokens, sim = r(B, Ltot, D), torch.tanh(r(B, Ltot, K))
    kpm = torch.zeros(B, L, dtype=torch.bool) if with_kpm else None
    if (B, Ltot, l0, L, K, D, top_k, with_kpm) == LTA_HAND:
        sim[:, :l0] = 0.99                                        # rows outside the slice would win every top-k if they were read
        sim[:, l0 + L:] = 0.99
        sim[0, l0:l0 + L] = _hand_sim()                           # columns 4 and 11 of sample 0: no survivor
        kpm[0, 5] = True
        kpm[1, 4] = True
    elif with_kpm:
        kpm[1] = True                                             # a fully masked sample: its output is exact zeros
        kpm[B - 1, L // 2] = True                                 # one token inside another sample
        if B > 3:
            kpm[2, L - 2:] = True                                 # a padded tail
    return dict(tokens=tokens, sim=sim, kpm=kpm, dmerge=r(B, K, D), geom=(l0, L, top_k))


# ------------------------------------------------------------------------------------------------------------------ heads
def bithash(x, w, b):
    """BitwiseHashing.forward (model/MITH.py:287-293), batch-major: x [B, K, D], w [K, D], b [K] -> tanh(x[b, k] . w[k] + b[k])"""
    return torch.tanh(torch.einsum("bkd,kd->bk", x, w) + b)


BITHASH_CASES = [(3, 5, 260), (1, 1, 4), (5, 16, 512), (261, 4, 68)]              # (B, K, D)


def bithash_case(B, K, D):
    g = gen(12, B, K, D)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(B, K, D), w=r(K, D) / D ** 0.5, b=0.1 * r(K), dy=r(B, K))


L2_EPS = 1e-12


def l2norm(x, clamp=True):
    """F.normalize(x, dim=-1): x / max(|x|, 1e-12)"""
    n = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    return x / (n.clamp_min(L2_EPS) if clamp else n)


def l2norm_dx(x, dy):
    """the gradient by formula: (dy - y (y . dy)) / |x| above the clamp; at or under it y = x / eps is linear: dy / eps"""
    n = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    y = x / n.clamp_min(L2_EPS)
    return torch.where(n > L2_EPS, (dy - y * (y * dy).sum(-1, keepdim=True)) / n.clamp_min(L2_EPS), dy / L2_EPS)


L2NORM_CASES = [(5, 65), (3, 7), (4, 128)]                                        # (R, D)


def l2norm_case(R, D):
    g = gen(13, R, D)
    x, dy = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    if (R, D) == (4, 128):
        x[1] = 0.0
        x[2] = 1e-20 * x[3]                                       # |row| ~ 1e-19 < eps: clamped, and not zero
    return dict(x=x, dy=dy)


MIX_LAMBDA = 0.8


def mith_mix(ic, it, tc, tt, lam):
    """B = sign(lam ic + (1 - lam) it + lam tc + (1 - lam) tt), H_i = (ic + it) / 2, H_t = (tc + tt) / 2 (hash_train.py:80-83, 179-180)
    -> (v, B, H_i, H_t)"""
    v = (ic * lam + it * (1 - lam)) + (tc * lam + tt * (1 - lam))
    return v, torch.sign(v), 0.5 * ic + 0.5 * it, 0.5 * tc + 0.5 * tt


def mix_case(n=257):
    g = gen(14, n)
    ic, it, tc, tt = (torch.tanh(torch.randn(n, generator=g)) for _ in range(4))
    near = mith_mix(ic.double(), it.double(), tc.double(), tt.double(), MIX_LAMBDA)[0].abs() < 1e-2
    for t in (ic, it, tc, tt):
        t[near] = 0.5                                             # no element near the sign's jump ...
    for t in (ic, it, tc, tt):
        t[::16] = 0.0                                             # ... exact zeros: all four inputs 0 ...
    tc[5::16], tt[5::16] = -ic[5::16], -it[5::16]                 # ... and the text side the negative of the image side
    tc[n - 1], tt[n - 1] = -ic[n - 1], -it[n - 1]                 # (the one element of the second block among them)
    return dict(ic=ic, it=it, tc=tc, tt=tt)


def add_positional(x, pe):
    """x[b, t, :] + pe[t, :] (model/MITH.py:270-273)"""
    return x + pe[None, :x.shape[1], :]


def gelu_case(n=257):
    g = gen(15, n)
    x = 2.5 * torch.randn(n, generator=g)
    x[0], x[1], x[2], x[n - 1] = 0.0, 6.0, -6.0, 1.5
    dy = torch.randn(n, generator=g)
    dy[n - 1] = 2.0                                               # the one element of the second block weighs in
    return dict(x=x, dy=dy)


SQ_GRID = 262144                                                  # threads of the largest sq_diff launch: 1024 workgroups of 256
SQDIFF_SIZES = [1, SQ_GRID + 257]


def sqdiff_case(n):
    g = gen(16, n)
    return dict(a=torch.tanh(torch.randn(n, generator=g)), b=torch.sign(torch.randn(n, generator=g)))


# ------------------------------------------------------------------------------------------------------------------ Bayesian loss
def bayes_loss(batch, bank, bank_label, label, clamp=True):
    """bayesian_loss (hash_train.py:138-144) with label_sim = (bank_label . label > 0); the dtype is that of batch"""
    d = bank.to(batch.dtype) @ batch.T
    s = 0.5 * (d.clamp(-64, 64) if clamp else d)
    ls = ((bank_label.double() @ label.double().T) > 0).to(batch.dtype)
    return -(ls * s - torch.log(1 + torch.exp(s))).mean()


def bayes_guard(bank, batch):
    """-> (the smallest | |bank_m . batch_b| - 64 |, the largest |bank_m . batch_b|)"""
    d = (bank.double() @ batch.double().T).abs()
    return float((d - 64).abs().min()), float(d.max())


# (Mb, B, K, C): kernel forms in the table of tests/test_gpu_mith_edges.py
BAYES_CASES = [(1023, 17, 16, 5), (1025, 17, 16, 5), (5, 3, 16, 1), (10257, 17, 16, 5), (33, 5, 5, 1), (300, 37, 24, 21), (70, 9, 128, 130)]
BAYES_TOO_LARGE = 65537
BAYES_SLICES, BAYES_CHUNK = 16, 640
BAYES_SALT = {(70, 9, 128, 130): 1}                                # the draw that keeps every product 1 away from the clamp


def bayes_case(Mb, B, K, C):
    """the inputs of test_bayesian_loss_on_the_matrix_pipe: tanh(randn) codes, one bank row and one batch row of 4.0 (their product
    16 K is far beyond the clamp), Bernoulli labels"""
    g = gen(17, Mb, B, K, C, BAYES_SALT.get((Mb, B, K, C), 0))
    bank, batch = torch.randn(Mb, K, generator=g).tanh(), torch.randn(B, K, generator=g).tanh()
    bank[3] = 4.0
    batch[min(5, B - 1)] = 4.0
    p = 0.15 if C >= 5 else 0.5
    bank_label, label = (torch.rand(Mb, C, generator=g) < p).float(), (torch.rand(B, C, generator=g) < p).float()
    bank_label[3] = 0.0                                           # the clamped pair is a dissimilar one: the clamp shows in value and gradient
    if C > 64:                                                    # one pair whose only common class is the last one (the last lane trip)
        bank_label[Mb - 1], label[B - 1] = 0.0, 0.0
        bank_label[Mb - 1, C - 1] = label[B - 1, C - 1] = 1.0
    return dict(bank=bank, batch=batch, bank_label=bank_label, label=label)


# ------------------------------------------------------------------------------------------------------------------ InfoNCE
NCE_TEMPERATURE = 0.07


def info_nce(a, b, G, temperature=NCE_TEMPERATURE, drop_last=False):
    """info_nce_loss (G = R) / info_nce_loss_bmm (hash_train.py:103-136): rows in groups of G, diagonal targets, both directions.
    drop_last: the last candidate of every group is left out of the log-sum-exps (a lane trip cut short)"""
    D = a.shape[-1]
    sc = torch.einsum("gid,gjd->gij", a.view(-1, G, D), b.view(-1, G, D)) / temperature
    diag = sc.diagonal(dim1=1, dim2=2)
    if drop_last and G > 1:
        return 0.5 * ((torch.logsumexp(sc[:, :, :-1], 2) - diag).mean() + (torch.logsumexp(sc[:, :-1, :], 1) - diag).mean())
    return 0.5 * ((torch.logsumexp(sc, 2) - diag).mean() + (torch.logsumexp(sc, 1) - diag).mean())


NCE_CASES = [(130, 65, 64), (10, 5, 64), (130, 65, 100), (12, 1, 65)]             # (R, G, D)


def nce_case(R, G, D):
    g = gen(18, R, G, D)
    return dict(a=F.normalize(torch.randn(R, D, generator=g), dim=-1), b=F.normalize(torch.randn(R, D, generator=g), dim=-1))


# ------------------------------------------------------------------------------------------------------------------ multi-similarity loss
MSL_THRESH, MSL_MARGIN, MSL_POS, MSL_NEG, MSL_EPS = 0.5, 0.1, 2.0, 40.0, 1e-5


def msl_parts(x, y, code, clamp=True, drop_col=None):
    """MultiSimilarityLoss.forward (train/DMsH_LN/MSLOSS.py:13-57) in the branch the trainer takes, every row at once; y is x itself
    when feat2 is None.  -> dict of the similarities, the masks and the two log terms per row.  A row whose norm is under the eps of
    F.normalize is divided by the eps, a constant (clamp=False divides by the norm itself).  drop_col: that column is left out of
    every row (the last entry of a j trip missed)."""
    S = x @ y.T
    B = S.shape[0]
    norm = torch.linalg.vector_norm(S, dim=1, keepdim=True)
    if drop_col is not None:
        cols = torch.ones(B, dtype=torch.bool)
        cols[drop_col] = False
        norm = torch.linalg.vector_norm(S[:, cols], dim=1, keepdim=True)
    sim = S / (torch.where(norm < 1e-12, torch.full_like(norm, 1e-12), norm) if clamp else norm)
    same = (code.double() @ code.double().T) > 0
    pos_, neg_ = same & (sim.detach() < 1 - MSL_EPS), ~same
    if drop_col is not None:
        pos_, neg_ = pos_ & cols[None, :], neg_ & cols[None, :]
    inf = torch.full_like(sim.detach(), math.inf)
    min_pos = torch.where(pos_, sim.detach(), inf).min(1, keepdim=True).values
    max_neg = torch.where(neg_, sim.detach(), -inf).max(1, keepdim=True).values
    has = pos_.any(1) & neg_.any(1)
    neg = neg_ & (sim.detach() + MSL_MARGIN > min_pos)
    pos = pos_ & (sim.detach() - MSL_MARGIN < max_neg)
    valid = has & neg.any(1) & pos.any(1)
    zero = torch.zeros_like(sim)
    pos_term = torch.log1p(torch.where(pos, torch.exp(-MSL_POS * (sim - MSL_THRESH)), zero).sum(1)) / MSL_POS
    neg_term = torch.log1p(torch.where(neg, torch.exp(MSL_NEG * (sim - MSL_THRESH)), zero).sum(1)) / MSL_NEG
    return dict(sim=sim, same=same, pos_=pos_, neg_=neg_, pos=pos, neg=neg, has=has, valid=valid, min_pos=min_pos, max_neg=max_neg,
                pos_term=pos_term, neg_term=neg_term, norm=norm)


def msl_loss(x, y, code, term="both", **how):
    p = msl_parts(x, y, code, **how)
    rows = {"both": p["pos_term"] + p["neg_term"], "pos": p["pos_term"], "neg": p["neg_term"]}[term]
    return torch.where(p["valid"], rows, torch.zeros_like(rows)).sum() / x.shape[0]


def msl_guard(x, y, code):
    """the smallest distance of a compared similarity from its threshold, over the decisions of the float64 reference: a similar pair
    against 1 - 1e-5, and in the rows that have both kinds a dissimilar one against min(pos_) - 0.1, a similar one against max(neg_) + 0.1"""
    p = msl_parts(x.double(), y.double(), code)
    sim, has = p["sim"], p["has"][:, None]
    d = [(sim - (1 - MSL_EPS)).abs()[p["same"]]]
    d.append((sim + MSL_MARGIN - p["min_pos"]).abs()[p["neg_"] & has])
    d.append((sim - MSL_MARGIN - p["max_neg"]).abs()[p["pos_"] & has])
    return float(torch.cat(d).min())


# (B, K, Kl, seed when feat2 is None, seed when feat2 is given)
MSL_CASES = [(257, 65, 33, 1, 3), (300, 257, 5, 0, 9), (7, 1024, 1023, 0, 1), (65, 16, 3, 0, 0), (5, 16, 3, 0, 0)]
MSL_ZERO_ROW = (5, 16, 3)


def msl_case(B, K, Kl, seed, cross):
    """rows from 4 class prototypes with 30 % of the signs flipped, label codes from 4 prototypes with 10 % flipped; the (5, 16, 3) case
    with row 0 of the features zero (its similarity row is the clamped one)"""
    g = gen(19, B, K, Kl, seed, int(cross))
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
    flip = lambda t, p: torch.where(torch.rand(t.shape, generator=g) < p, -t, t)
    cls = torch.randint(0, 4, (B,), generator=g)
    px, pc = sign(4, K), sign(4, Kl)
    x, y, code = flip(px[cls], 0.3), flip(px[cls], 0.3), flip(pc[cls], 0.1)
    if (B, K, Kl) == MSL_ZERO_ROW:
        x[0] = 0.0
    return dict(x=x, y=y if cross else None, code=code)


def msl_problem(case, cross):
    """-> (c, fn, tensors, names) in the manner of lossutil.problem"""
    B, K, Kl, s_self, s_cross = case
    c = msl_case(B, K, Kl, s_cross if cross else s_self, cross)
    if cross:
        return c, (lambda x, y, **how: msl_loss(x, y, c["code"], **how)), [c["x"], c["y"]], ["dfeats", "dfeat2"]
    return c, (lambda x, **how: msl_loss(x, x, c["code"], **how)), [c["x"]], ["dfeats"]


UPSTREAM = {"lta": 1.7, "bithash": 1.7, "l2norm": 0.3, "gelu": 0.3, "addpos": 1.7, "sqdiff": 0.3, "bayes": 0.3, "nce": 1.7, "msl": 1.7}


# ------------------------------------------------------------------------------------------------------------------ golden anchor
ANCHOR_LTA = [(2, 6, 8, 16, 3, False, True), (3, 7, 8, 16, 8, True, False), (2, 5, 12, 8, 3, False, False)]     # (B, L, K, D, top_k, kpm, ties)


def anchor_lta_case(i):
    """the tiny inputs tests/golden/make_golden19.py feeds to the reference's LocalizedTokenAggregation"""
    B, L, K, D, top_k, with_kpm, ties = ANCHOR_LTA[i]
    g = gen(20, i, B, L, K, D)
    tokens, sim = torch.randn(B, L, D, generator=g), torch.tanh(torch.randn(B, L, K, generator=g))
    kpm = None
    if ties:                                                      # every token: its largest value twice, its third largest three times
        for b in range(B):
            for l in range(L):
                order = torch.argsort(sim[b, l], descending=True)
                sim[b, l, order[1]] = sim[b, l, order[0]]
                sim[b, l, order[3]] = sim[b, l, order[2]]
                sim[b, l, order[4]] = sim[b, l, order[2]]
    if with_kpm:
        kpm = torch.zeros(B, L, dtype=torch.bool)
        kpm[0, L - 2:] = True
        kpm[1, 0] = True
        sim[0, :L - 2, 3] = -sim[0, :L - 2, 3].abs()              # concept 3 of sample 0: positive only under the padding -> emptied
        sim[0, L - 2:, 3] = 0.8
    return dict(tokens=tokens, sim=sim, kpm=kpm, dmerge=torch.randn(B, K, D, generator=g), geom=(0, L, top_k))


def anchor_bithash_case():
    return bithash_case(3, 6, 20)
