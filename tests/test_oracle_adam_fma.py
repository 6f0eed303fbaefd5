"""oracle.adam_oracle.fma32 - the emulation of ATen's f32 fused multiply-add inside the `m` update - against exact rational arithmetic.
The earlier emulation (one f64 add, then a round to f32: fma32_two_roundings) rounds twice; the tests of the fused kernel that demand
bit-equality (test_gpu_adam_edges.py) need the single rounding."""
from fractions import Fraction

import numpy as np

import oracle.adam_oracle as ao

f32 = np.float32


def rne_f32(x: Fraction) -> np.float32:
    """the float32 nearest to a rational, ties to even (finite results only)"""
    if x == 0:
        return f32(0)
    a, e = abs(x), 0
    while a >= 1 << 24:
        a, e = a / 2, e + 1
    while a < 1 << 23 and e > -149:
        a, e = a * 2, e - 1
    n = a.numerator // a.denominator
    rem = a - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return f32(np.ldexp(np.float64(n), e)) * f32(1 if x > 0 else -1)


def exact(x, y, z):
    return rne_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))


def test_rne_helper_against_numpy_on_doubles():
    rng = np.random.default_rng(0)
    for d in np.concatenate([rng.standard_normal(200) * 10.0 ** rng.integers(-44, 30, 200), [2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150]]):
        assert rne_f32(Fraction(float(d))).view(np.uint32) == f32(d).view(np.uint32), d


def test_fma32_rounds_once_where_the_f64_add_rounds_twice():
    """z = 2^26 + 8 has an odd f32 mantissa; x * y = 4 (1 - 2^-46), so the exact sum lies 2^-44 below the f32 tie z + 4.  The f64 add
    rounds it onto the tie, and ties-to-even then picks z + 8; one rounding gives z.  Mirrored in sign and in direction too."""
    cases = [(f32(4) * (f32(1) + f32(2.0 ** -23)), f32(1) - f32(2.0 ** -23), f32(2.0 ** 26 + 8)),
             (-f32(4) * (f32(1) + f32(2.0 ** -23)), f32(1) - f32(2.0 ** -23), -f32(2.0 ** 26 + 8)),
             (-f32(4) * (f32(1) + f32(2.0 ** -23)), f32(1) - f32(2.0 ** -23), f32(2.0 ** 26 + 8)),     # 2^-44 above the tie z - 4: the tie goes to 2^26
             (f32(4) * (f32(1) + f32(2.0 ** -23)), f32(1) - f32(2.0 ** -23), -f32(2.0 ** 26 + 8))]
    for x, y, z in cases:
        want = exact(x, y, z)
        got = ao.fma32(np.array([x]), y, np.array([z]))[0]
        assert got.view(np.uint32) == want.view(np.uint32), (x, y, z, got, want)
        assert ao.fma32_two_roundings(x, y, z).view(np.uint32) != want.view(np.uint32), "this case no longer separates the two emulations"
    assert float(ao.fma32(cases[0][0], cases[0][1], cases[0][2])) == 2.0 ** 26 + 8


def test_fma32_equals_the_exact_sum_on_random_and_edge_operands():
    rng = np.random.default_rng(1)
    n = 400
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 8, n)).astype(f32)
    y = np.full(n, f32(1.0 - 0.9))
    z = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 8, n)).astype(f32)
    z[:40] = -(x[:40].astype(np.float64) * np.float64(y[0])).astype(f32)        # cancellation: the sum is far below both operands
    x[40:50], z[40:50] = 0, rng.standard_normal(10).astype(f32)
    z[50:60] = (rng.standard_normal(10) * 1e-42).astype(f32)                    # denormal addend
    x[60:70] = (rng.standard_normal(10) * 1e-41).astype(f32)                    # product below the f32 range
    got = ao.fma32(x, y, z)
    for i in range(n):
        assert got[i].view(np.uint32) == exact(x[i], y[i], z[i]).view(np.uint32), (i, x[i], y[i], z[i])


def test_fma32_agrees_with_the_earlier_formula_wherever_the_f64_add_is_exact():
    rng = np.random.default_rng(2)
    n = 200000
    m = rng.standard_normal(n).astype(f32) * f32(0.9)
    g = rng.standard_normal(n).astype(f32)
    w = f32(1.0 - 0.9)
    a, b = g.astype(np.float64) * np.float64(w), m.astype(np.float64)
    s = a + b
    bb = s - a
    exact_add = ((a - (s - bb)) + (b - bb)) == 0
    assert exact_add.sum() > n // 100 and (~exact_add).sum() > n // 100          # both kinds are present
    new, old = ao.fma32(g, w, m), ao.fma32_two_roundings(g, w, m)
    assert np.array_equal(new[exact_add].view(np.uint32), old[exact_add].view(np.uint32))
    # elsewhere the two may differ only where the f64 sum sits exactly on an f32 tie: far rarer than this sample can show
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
    assert np.isinf(ao.fma32(f32(3e38), f32(2), f32(3e38))) and np.isnan(ao.fma32(f32(np.inf), f32(1), f32(-np.inf)))


def test_step_takes_a_given_clip_coefficient():
    rng = np.random.default_rng(3)
    p, g = rng.standard_normal(50).astype(f32), rng.standard_normal(50).astype(f32) * 3
    z = np.zeros(50, f32)
    c = min(ao.clip_coef(g, 1.0), f32(1))
    assert c < 1
    ref = ao.step(p, g, z, z, 0, 1e-3, 0.9, 0.98, 1e-6, 0.2, 1.0)
    for mx in (1.0, 0, -1):                                                    # the given coefficient replaces the norm-derived one
        out = ao.step(p, g, z, z, 0, 1e-3, 0.9, 0.98, 1e-6, 0.2, mx, coef=c)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out, ref))
    unclipped = ao.step(p, g, z, z, 0, 1e-3, 0.9, 0.98, 1e-6, 0.2, 1.0, coef=f32(1))
    assert np.array_equal(unclipped[1].view(np.uint32), g.view(np.uint32))
    assert np.array_equal(ao.step(p, g, z, z, 0, 1e-3, 0.9, 0.98, 1e-6, 0.2, -1)[0].view(np.uint32), unclipped[0].view(np.uint32))
