"""TEST INFRASTRUCTURE ONLY — CPU restatement (numpy, fp32 arithmetic in the reference's operation order) of one step of the
reference's BertAdam for ONE parameter tensor (model/base/optimization.py:103-168).  Pinned by tests/golden/adam.npz, which
was produced by running the reference's own BertAdam (tests/golden/make_golden4.py)."""
import math

import numpy as np

f32 = np.float32


def schedule(name, x, warmup):
    """optimization.py:26-43"""
    if x < warmup:
        return x / warmup
    if name == "warmup_cosine":
        return 0.5 * (1.0 + math.cos(math.pi * x))
    if name == "warmup_constant":
        return 1.0
    return max((x - 1.) / (warmup - 1.), 0)


def fma32(x, y, z):
    """fl32(x * y + z) with ONE rounding, for float32 arrays / scalars: the f32 fused multiply-add.
    x * y is exact in f64 (24 x 24 bits).  The f64 add s = fl64(xy + z) may be inexact, and rounding s to f32 then rounds twice: when
    s lands on an f32 tie that the exact sum only comes near, the second rounding goes the wrong way (about once in 2^29 elements).
    So the add's error is recovered exactly (Knuth's two-sum) and, where it is not zero, s is moved to the neighbour with the odd
    mantissa on the error's side (round to odd): 53 >= 24 + 2 bits, so the f32 cast of that value is the correctly rounded sum."""
    a = np.asarray(x, f32).astype(np.float64) * np.asarray(y, f32).astype(np.float64)
    b = np.asarray(z, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b
        bb = s - a
        err = (a - (s - bb)) + (b - bb)                                 # a + b == s + err exactly (s finite)
    s = np.atleast_1d(s).copy()
    err = np.atleast_1d(err)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        toward = np.where((err > 0) == (s > 0), 1, -1)                  # |s| grows when the error has s's sign
        s.view(np.int64)[fix] += toward[fix]                            # (s == 0 with err != 0 cannot happen: a sum that is 0 is exact)
    with np.errstate(over="ignore"):
        return s.astype(f32).reshape(np.broadcast(a, b).shape)


def fma32_two_roundings(x, y, z):
    """the emulation this module used before fma32: exact f64 product, one f64 add, round to f32 (kept for tests/test_oracle_adam.py)"""
    return (np.asarray(x, f32).astype(np.float64) * np.asarray(y, f32).astype(np.float64)
            + np.asarray(z, f32).astype(np.float64)).astype(f32)


def clip_coef(g, max_grad_norm):
    """max_norm / (||g||_2 + 1e-6) as clip_grad_norm_ forms it, NOT yet clamped to 1 (f32)."""
    total = f32(np.sqrt(np.sum(np.asarray(g, f32).astype(np.float64) ** 2)))
    return f32(max_grad_norm) / (total + f32(1e-6))


def step(p, g, m, v, step_no, lr, b1, b2, e, weight_decay, max_grad_norm, t_total=-1, warmup=-1, sched="warmup_linear", coef=None):
    """-> (p, g, m, v) after one step; inputs are float32 arrays (not modified).  `coef`: a clip coefficient (already clamped to
    <= 1) to use in place of the norm-derived one - the only part of the step whose value depends on a summation order."""
    p, g, m, v = (np.array(a, f32) for a in (p, g, m, v))
    if coef is not None:
        g = g * f32(coef)
    elif max_grad_norm > 0:                                             # :135-136 clip_grad_norm_(p, max_grad_norm)
        g = g * min(clip_coef(g, max_grad_norm), f32(1.0))
    # :141 next_m.mul_(b1).add_(grad, alpha=1-b1): ATen's add(alpha) is a fused multiply-add (vec::fmadd), i.e. ONE rounding of
    # m*b1 (already rounded) + alpha*g
    m = fma32(g, f32(1.0 - b1), m * f32(b1))
    v = v * f32(b2) + (f32(1.0 - b2) * g) * g                           # :143
    upd = m / (np.sqrt(v) + f32(e))                                     # :144
    if weight_decay > 0.0:
        upd = upd + f32(weight_decay) * p                               # :153-154
    lr_s = lr * schedule(sched, step_no / t_total, warmup) if t_total != -1 else lr   # :156-161 (python double)
    p = p + (-(f32(lr_s) * upd))                                        # :163-164
    return p, g, m, v
