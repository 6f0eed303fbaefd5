"""Shared by the BertAdam tests: the seeded tensors / gradients of tests/golden/make_golden4.py and an oracle driver."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden4 as mg  # noqa: E402  (only its seeded-input helpers; nothing of the reference is imported here)

CONFIGS = {
    "trainer": dict(lr=1e-3, warmup=0.1, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, t_total=10, weight_decay=0.2,
                    max_grad_norm=1.0),
    "plain": dict(lr=5e-4, warmup=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6, t_total=-1, weight_decay=0.0,
                  max_grad_norm=-1),
}
GROUP0_LR = 1e-5        # the first half of the tensors sits in a group with its own lr (like clip_lr)


def run_oracle(tag):
    """-> lists p, g, m, v (float32 arrays) after mg.STEPS steps of oracle.adam_oracle on the seeded problem."""
    import oracle.adam_oracle as ao
    kw = CONFIGS[tag]
    ps = [t.numpy().copy() for t in mg.tensors(3)]
    ms = [np.zeros_like(p) for p in ps]
    vs = [np.zeros_like(p) for p in ps]
    gs = [None] * len(ps)
    half = len(ps) // 2
    for s in range(mg.STEPS):
        for i, g in enumerate(mg.grads(3, s)):
            lr = GROUP0_LR if i < half else kw["lr"]
            ps[i], gs[i], ms[i], vs[i] = ao.step(ps[i], g.numpy(), ms[i], vs[i], s, lr, kw["b1"], kw["b2"], kw["e"],
                                                 kw["weight_decay"], kw["max_grad_norm"], kw["t_total"], kw["warmup"],
                                                 kw["schedule"])
    return ps, gs, ms, vs


def cut(a):
    a = np.asarray(a).reshape(-1)
    return a[::mg.SLICE] if a.size > 2000 else a


def atol(ref):
    """a few ulps of the array's largest magnitude (see test_oracle_adam.py)"""
    return 4e-7 * float(np.abs(np.asarray(ref)).max())


# ---- the fused step driven tensor by tensor and held to the oracle bit for bit (test_gpu_adam_edges.py, test_gpu_adam_bf16.py) ----
DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.98, 1e-6
PAD = 8                 # slack elements before and after every view (the allocator's blocks are 16-byte aligned, and so is PAD * 4)
GUARD = -7.25           # what the slack holds
COEF_ULPS = 16          # how far from the oracle's clip coefficient the kernel's is looked for (test_gpu_adam_edges.py)
STREAMS = "pgmv"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want, what):
    """float32 arrays equal as bit patterns (so -0 != +0 and a NaN equals itself), with the first offender in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ, first at [{bad[0]}]: got {got.reshape(-1)[bad[0]]!r}, "
                           f"want {want.reshape(-1)[bad[0]]!r}; last at [{bad[-1]}]")


def ulp_step(c, k):
    """the float32 k ulps away from a positive finite float32 c"""
    return (np.float32(c).view(np.int32) + np.int32(k)).view(np.float32)


def recover_coef(g0, g1, centre, radius=COEF_ULPS):
    """The clip coefficient the kernel used: the float32 c <= 1 within `radius` ulps of `centre` (the oracle's coefficient, not yet
    clamped) for which g1 is fl(g0 * c) on EVERY element -> (c, |distance in ulps|), or (None, None).  c == 1 means `g1 is g0`: it is
    taken whenever the gradient's bits did not move.  Several c can reproduce a short gradient; they give the same step, since m, v and
    p depend on the clipped gradient only, and the nearest one is reported."""
    g0, g1 = np.asarray(g0, np.float32).reshape(-1), np.asarray(g1, np.float32).reshape(-1)
    head = slice(0, 4096)
    for d in sorted(range(-radius, radius + 1), key=abs):
        c = min(ulp_step(centre, d), np.float32(1.0))
        if np.array_equal(bits(g0[head] * c), bits(g1[head])) and np.array_equal(bits(g0 * c), bits(g1)):
            return c, abs(d)
    return None, None


class Slot:
    """One tensor of a fused step: p / g / m / v as views into four device buffers with PAD elements of slack on both sides, each
    view `off` elements (0: 16-byte aligned, 1: 4-byte aligned only) behind the slack; the per-tensor scalars of cmh_adam_tensor."""

    def __init__(self, n, lr=1e-3, wd=0.2, mx=1.0, off=(0, 0, 0, 0), seed=0, gscale=1.0, p=None, first_step=True):
        self.n, self.lr, self.wd, self.mx, self.off, self.seed, self.gscale = n, lr, wd, mx, off, seed, gscale
        rng = np.random.default_rng([seed, n])
        init = {"p": rng.standard_normal(n).astype(np.float32) if p is None else np.asarray(p, np.float32),
                "g": np.zeros(n, np.float32), "m": np.zeros(n, np.float32), "v": np.zeros(n, np.float32)}
        self.base, self.view = {}, {}
        for k, o in zip(STREAMS, off):
            host = np.full(n + 2 * PAD + 1, GUARD, np.float32)
            host[PAD + o:PAD + o + n] = init[k]
            self.base[k] = torch.from_numpy(host).to(DEV)
            self.view[k] = self.base[k][PAD + o:PAD + o + n]
            assert self.base[k].data_ptr() % 16 == 0 and self.view[k].data_ptr() % 16 == 4 * o
        self.steps = 0
        self.dist = []          # ulp distance of each recovered clip coefficient
        self.coefs = []

    def gradient(self, g=None):
        """a fresh gradient for the next step (seeded by the step number), or the given one"""
        if g is None:
            g = np.random.default_rng([self.seed, self.n, 1 + self.steps]).standard_normal(self.n).astype(np.float32) * np.float32(self.gscale)
        self.view["g"].copy_(torch.from_numpy(np.ascontiguousarray(g, np.float32)))
        return self

    def entry(self):
        v = self.view
        return (v["p"], v["g"], v["m"], v["v"], self.lr, self.wd, self.mx)

    def host(self):
        return {k: self.base[k].cpu().numpy() for k in STREAMS}

    def verify(self, before, after, b1=B1, b2=B2, e=EPS, what=""):
        """`before` / `after`: host() around ONE step.  The slack is untouched; an unclipped tensor's gradient keeps its bits; a
        clipped one yields the kernel's coefficient; p, m, v (and g) equal the oracle's, run with that coefficient, bit for bit."""
        import oracle.adam_oracle as ao
        what = f"{what} n={self.n} off={self.off} lr={self.lr} wd={self.wd} mx={self.mx} step={self.steps}"
        old, new = {}, {}
        for k, o in zip(STREAMS, self.off):
            lo, hi = PAD + o, PAD + o + self.n
            same_bits(after[k][:lo], before[k][:lo], f"{what}: slack before {k}")
            same_bits(after[k][hi:], before[k][hi:], f"{what}: slack after {k}")
            old[k], new[k] = before[k][lo:hi], after[k][lo:hi]
        if self.mx > 0:
            centre = ao.clip_coef(old["g"], self.mx)
            if np.array_equal(bits(old["g"]), bits(new["g"])):
                c, d = np.float32(1.0), (0 if centre >= 1 else int(np.float32(1.0).view(np.int32)) - int(centre.view(np.int32)))
                assert d <= COEF_ULPS, (f"{what}: the gradient was left as it is, but the oracle clips it with {centre!r} "
                                        f"({d} ulps below 1)")
            else:
                c, d = recover_coef(old["g"], new["g"], centre)
                assert c is not None, (f"{what}: no float32 within {COEF_ULPS} ulps of the oracle's coefficient {centre!r} turns the "
                                       "gradient into the one the kernel left")
                assert c < 1, f"{what}: the gradient's bits moved under a coefficient of 1"
            self.dist.append(d)
        else:
            c = np.float32(1.0)
            same_bits(new["g"], old["g"], f"{what}: g of a tensor without clipping")
        self.coefs.append(c)
        rp, rg, rm, rv = ao.step(old["p"], old["g"], old["m"], old["v"], 0, self.lr, b1, b2, e, self.wd, self.mx, coef=c)
        for k, ref in zip(STREAMS, (rp, rg, rm, rv)):
            same_bits(new[k], ref, f"{what}: {k} vs oracle (coefficient {c!r})")
        self.steps += 1
        return c


def run_steps(N, slots, steps=2, b1=B1, b2=B2, e=EPS, what="", grads=None):
    """`steps` fused steps over all slots in one call each, every tensor verified after every step -> the largest ulp distance of a
    recovered clip coefficient (0 when nothing had a max_grad_norm)."""
    for s in range(steps):
        for i, sl in enumerate(slots):
            sl.gradient(None if grads is None else grads[s][i])
        before = [sl.host() for sl in slots]
        N.bert_adam_step([sl.entry() for sl in slots], b1, b2, e)
        torch.cuda.synchronize()
        for sl, bf in zip(slots, before):
            sl.verify(bf, sl.host(), b1, b2, e, what)
    return max([d for sl in slots for d in sl.dist], default=0)


# ---- f32 -> bf16: bit patterns at which a round-to-nearest-even can go wrong ----
CRAFTED_BITS = (
    0x3f808000, 0x3f818000,             # ties: to even (down to 0x3f80), to even (up to 0x3f82)
    0x3f807fff, 0x3f808001,             # one below and one above a tie
    0xbf808000, 0xbf818000,             # the ties, negative
    0x00000000, 0x80000000,             # +-0
    0x7f7fffff, 0xff7fffff,             # the largest finite f32: rounds to +-inf
    0x7f7f7fff, 0xff7f7fff,             # the largest that stays finite (0x7f7f8000 is a tie that goes up to inf)
    0x7f7f8000,                         # ... that tie
    0x00800000, 0x80800000,             # the smallest normal
    0x007fffff,                         # the largest denormal: rounds up to the smallest normal
    0x00000001, 0x00008000, 0x00008001, # denormals below the smallest bf16 denormal: to 0, tie to 0, up to 0x0001
    0x00018000, 0x00408001, 0x80018000, # a denormal tie to even (0x0002), one above a tie, the tie negative
    0x7f800000, 0xff800000,             # +-inf
)
assert len(CRAFTED_BITS) % 2 == 0       # crafted_vector's period 2 K + 1 is odd: coprime to 4


def crafted_vector(n, rot=0, seed=0):
    """float32 [n]: the crafted values alternate with random ones in a sequence of odd period 2 K + 1 (c0 r c1 r ... cK-1 r r), so
    over 4 periods every crafted value falls on every position mod 4; `rot` shifts the sequence, which moves other values into the
    last n % 4 elements (the tail of a float4 loop)."""
    K = len(CRAFTED_BITS)
    period = 2 * K + 1
    x = (np.random.default_rng([seed, n, rot]).standard_normal(n) * 3).astype(np.float32)
    j = (np.arange(n) + rot) % period
    put = (j % 2 == 0) & (j < 2 * K)
    x[put] = np.array(CRAFTED_BITS, np.uint32).view(np.float32)[j[put] // 2]
    return x


def crafted_rotations(n):
    """rotations after which every crafted value has stood in each of the last 3 elements of an n-element vector"""
    return range(0, 2 * len(CRAFTED_BITS) + 1)


def bf16_bits(t):
    """a bf16 tensor's bit patterns as an int16 CPU tensor"""
    return t.detach().contiguous().view(torch.int16).cpu()


def rne_bf16_bits(x):
    """int16 bit patterns of torch's round-to-nearest-even f32 -> bf16 cast, made on the CPU"""
    return x.detach().cpu().contiguous().to(torch.bfloat16).view(torch.int16)
