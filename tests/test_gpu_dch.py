"""The supervised training-free fit on the GPU (csrc/dch.hip, utils/dch.py, train/DCH) against the NumPy fp64 restatement of
tests/dchutil.py: every kernel on its own within the bound its arithmetic allows, the fit end to end with exact codes on the fixtures
that tests/test_dch_host.py shows robust, the f32 heads against the fit, and the trainer through main.py, query.py and retrieve.py.

Bounds.  A sum of n terms in any order is within n eps sum|terms| of the exact one; two orders differ by twice that, and the tests
ask 8 n eps sum|terms| ("the summation-order bound", tests/test_gpu_itq.py's).  B^T B, 1^T B and the flips are integers: exact.  The
coordinate descent runs the restatement's chain term for term, so its bits, flips and smallest |t| are the restatement's.  A
Cholesky solve is backward stable: the error against LAPACK's LU is asked within 64 K eps cond_2(A + shift I) max|W|.

Measured on MI355X (this file's prints): see DESIGN.md §7.11."""
import numpy as np
import pytest
import torch

import dchutil as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = U.EPS
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_after_module():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _get(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _codes(b):
    return _dev(b, torch.int8)


# ---------------------------------------------------------------------------------------------------- the coordinate descent
DCC_SHAPES = [(1, 1), (63, 8), (65, 33), (257, 64), (2049, 128)]      # one lane, a wave edge, a bit-word crossing, the largest K and more than one block


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("n,k", DCC_SHAPES)
def test_dcc_reproduces_the_restatement_bit_for_bit(n, k, rounds):
    import cmh_native as N
    q, g, b0, refs = _get(("dcc", n, k), lambda: U.dcc_case(n, k, 31 + n + k))
    rb, rflips, rleast = refs[rounds]
    assert rleast >= U.MARGIN_FLOOR                                         # from the restatement alone
    B = _codes(b0)
    flips, least = N.dch_dcc(_dev(q.T), _dev(g), B, rounds)
    assert np.array_equal(_np(B).astype(np.float64), rb), int((_np(B) != rb).sum())
    assert _np(flips).tolist() == rflips.tolist()
    assert abs(float(least) - rleast) <= 1e-12 * rleast
    B2 = _codes(b0)
    again = N.dch_dcc(_dev(q.T), _dev(g), B2, rounds)
    assert torch.equal(B, B2) and torch.equal(flips, again[0]) and torch.equal(least, again[1])
    print(f"\ndcc ({n}, {k}), {rounds} rounds: flips {rflips.tolist()}, smallest |t| {rleast:.3e} (kernel {float(least):.3e})")


def test_dcc_keeps_the_bit_where_t_is_zero():
    """Integers throughout (G, Q, so every t), many of them zero: the case that tells "t == 0 keeps the bit" from "t >= 0 sets +1"."""
    import cmh_native as N
    n, k = 300, 37
    rng = np.random.default_rng(5)
    g = rng.integers(-2, 3, size=(k, k)).astype(np.float64)
    g = np.triu(g) + np.triu(g, 1).T
    q = rng.integers(-4, 5, size=(n, k)).astype(np.float64)
    b0 = U.random_codes(n, k, 6)
    rb, rflips, rleast = U.dcc(q, g, b0, 2)
    other = U.dcc(q, g, b0, 2, keep_on_zero=False)[0]
    assert rleast == 0.0 and int((rb != other).sum()) > 100                 # the rule matters on this case
    B = _codes(b0)
    flips, least = N.dch_dcc(_dev(q.T), _dev(g), B, 2)
    assert np.array_equal(_np(B).astype(np.float64), rb) and _np(flips).tolist() == rflips.tolist() and float(least) == 0.0


# ---------------------------------------------------------------------------------------------------- X^T B and B^T B
@pytest.mark.parametrize("n", [1, 2047, 2049, 5000])                       # around the chunk of 2048 rows
def test_xtb_and_btb(n):
    import cmh_native as N
    rng = np.random.default_rng(n)
    worst = 0.0
    for k in (1, 33, 128):
        b = U.random_codes(n, k, 100 + n + k)
        B = _codes(b)
        btb = N.dch_btb(B)
        assert np.array_equal(_np(btb).astype(np.int64), b.astype(np.int64).T @ b.astype(np.int64))      # exact
        assert torch.equal(btb, N.dch_btb(B)) and torch.equal(btb, btb.t())
        for dx in (1, 24, 65):
            x = (rng.standard_normal((n, dx)) + 8.0 * rng.standard_normal(dx)).astype(np.float32)
            X = _dev(x)
            out, bsum = N.dch_xtb(X, B, want_bsum=True)
            again = N.dch_xtb(X, B, want_bsum=True)
            assert torch.equal(out, again[0]) and torch.equal(bsum, again[1])
            assert torch.equal(out, N.dch_xtb(X, B))                       # without the column sums: the same bits
            x64 = x.astype(np.float64)
            ref, bound = x64.T @ b, U.order_bound(n, np.abs(x64).sum(0))[:, None] * np.ones((1, k))
            assert np.all(np.abs(_np(out) - ref) <= bound)
            assert np.array_equal(_np(bsum), b.sum(0))                     # integers: exact
            worst = max(worst, float((np.abs(_np(out) - ref) / bound).max()))
            N.dch_xtb(X, B, want_bsum=True, into=(out, bsum))               # accumulate: twice the rows
            assert np.all(np.abs(_np(out) - 2 * ref) <= 2 * bound) and np.array_equal(_np(bsum), 2 * b.sum(0))
    print(f"\nxtb N = {n}: worst error / bound {worst:.3f}")


def test_xtb_streamed_in_unequal_batches_matches_the_whole():
    import cmh_native as N
    n, dx, k = 5000, 40, 16
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((n, dx)) + 8.0).astype(np.float32)
    b = U.random_codes(n, k, 10)
    cuts, into = [0, 4100, 4163, n], None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        into = N.dch_xtb(_dev(x[lo:hi]), _codes(b[lo:hi]), want_bsum=True, into=into)
    ref = x.astype(np.float64).T @ b
    assert np.all(np.abs(_np(into[0]) - ref) <= U.order_bound(n, np.abs(x.astype(np.float64)).sum(0))[:, None])
    assert np.array_equal(_np(into[1]), b.sum(0))


@pytest.mark.parametrize("d", [1, 33, 65])                                  # one column, inside a tile, past a tile of 64
@pytest.mark.parametrize("n", [1, 2047, 2049, 4100])                       # around the chunk of 2048 rows, and three chunks
def test_the_products_are_the_unsupervised_fits_bit_for_bit(n, d):
    """X^T B, B^T B and 1^T B are one chunked product and one column sum (csrc/fit_common.h) with itq_moments / itq_cross_moments:
    the casts of +-1 from int8 and from f32 to f64 are both exact, and each output element is one fma chain in row order, then the
    chunks in chunk order, so the two families agree to the bit - as long as the product is written once.  K = D."""
    import cmh_native as N
    rng = np.random.default_rng(1000 * d + n)
    x = (rng.standard_normal((n, d)) + 8.0 * rng.standard_normal(d)).astype(np.float32)
    X, B = _dev(x), _codes(U.random_codes(n, d, 200 + n + d))
    Bf = B.float()
    out, bsum = N.dch_xtb(X, B, want_bsum=True)
    cross, sums, btb = N.itq_cross_moments(X, Bf), N.itq_moments(Bf), N.dch_btb(B)
    assert torch.equal(out, cross)
    assert torch.equal(btb, sums[1])
    assert torch.equal(bsum, sums[0])
    N.dch_xtb(X, B, want_bsum=True, into=(out, bsum))                       # one accumulate step on either side
    assert N.itq_cross_moments(X, Bf, cross=cross) is cross and N.itq_moments(Bf, sums=sums) is sums
    assert torch.equal(out, cross)
    assert torch.equal(bsum, sums[0])
    assert torch.equal(btb + btb, sums[1])                                  # dch_btb does not accumulate; integers, so the sum is exact


# ---------------------------------------------------------------------------------------------------- the label regression's solve
SOLVE_C = [1, 7, 130]
SOLVE_CASES = [("random", k) for k in (1, 2, 33, 64, 128)] + [("equal_columns", k) for k in (2, 33, 64, 128)]


def _solve_case(kind, k):
    """A = B^T B and R = B^T Y for every C of SOLVE_C (B itself is not kept).  random: 4 K + 3 rows.  equal_columns: 100 000 rows
    and two equal bit columns, so B^T B is singular with entries of size N and only the shift of 1 makes it definite."""
    rng = np.random.default_rng(1000 + k)
    n = 100000 if kind == "equal_columns" else 4 * k + 3
    b = U.random_codes(n, k, 7 + k)
    if kind == "equal_columns":
        b[:, k - 1] = b[:, 0]
    return b.T @ b, {c: b.T @ (rng.random((n, c)) < 0.2).astype(np.float64) for c in SOLVE_C}


@pytest.mark.parametrize("c", SOLVE_C)
@pytest.mark.parametrize("kind,k", SOLVE_CASES)
def test_solve_against_lapack(kind, k, c):
    import cmh_native as N
    a, rs = _get(("solve", kind, k), lambda: _solve_case(kind, k))
    r, shift = rs[c], 1.0
    full = a + shift * np.eye(k)
    ref = np.linalg.solve(full, r)
    cond = np.linalg.cond(full)
    W, info = N.dch_solve(_dev(a), _dev(r), shift)
    W2, _ = N.dch_solve(_dev(a), _dev(r), shift)
    assert int(info) == 0 and torch.equal(W, W2)
    err, bound = np.abs(_np(W) - ref).max(), 64 * k * EPS * cond * np.abs(ref).max()
    print(f"\nsolve {kind} K = {k}, C = {c}: cond {cond:.2e}, error {err:.2e}, bound {bound:.2e}, ratio {err / bound:.4f}")
    assert err <= bound
    if kind == "equal_columns":
        assert cond >= 1e5                                                  # entries of size N against the shift of 1


def test_solve_reports_a_pivot_that_is_not_positive():
    import cmh_native as N
    for a, first in ((np.array([[1.0, 2.0], [2.0, 1.0]]), 2), (-np.eye(3), 1), (np.array([[np.nan]]), 1), (np.zeros((4, 4)), 1)):
        W, info = N.dch_solve(_dev(a), _dev(np.ones((a.shape[0], 5))), 0.0)
        assert int(info) == first and not bool(W.any())
    W, info = N.dch_solve(_dev(np.zeros((4, 4))), _dev(np.ones((4, 5))), 2.0)   # the shift alone makes it definite
    assert int(info) == 0 and np.allclose(_np(W), 0.5, atol=1e-15)
    flag = torch.full((3,), -7, dtype=torch.int32, device=DEV)              # a slice of a longer record is written alone
    N.dch_solve(_dev(-np.eye(2)), _dev(np.ones((2, 2))), 0.0, info=flag[1:2])
    assert flag.tolist() == [-7, 1, -7]


# ---------------------------------------------------------------------------------------------------- targets and objective
@pytest.mark.parametrize("n,k,c", [(65, 8, 1), (300, 16, 5), (257, 33, 7), (1000, 128, 40), (130, 64, 70)])
def test_targets_and_objective(n, k, c):
    import cmh_native as N
    rng = np.random.default_rng(n + k + c)
    y = (rng.random((n, c)) < 0.3).astype(np.float64)
    y[n // 2] = 0.0                                                         # an item without a label
    b = U.random_codes(n, k, n + 1)
    w = rng.standard_normal((k, c)) / np.sqrt(k)
    z_i, z_t = b * 0.6 + 0.5 * rng.standard_normal((n, k)), b * 0.4 + 0.5 * rng.standard_normal((n, k))
    mu, lam = 0.37, 1.3
    ops = (_dev(y, torch.float32), _codes(b), _dev(w), _dev(z_i), _dev(z_t))
    Qt, obj2 = N.dch_targets(*ops, mu, lam)
    again = N.dch_targets(*ops, mu, lam)
    assert torch.equal(Qt, again[0]) and torch.equal(obj2, again[1])
    none, alone = N.dch_targets(*ops, mu, lam, want_q=False)
    assert none is None and torch.equal(alone, obj2)                        # the objective does not depend on whether Q is written
    ref_q = U.targets(y, w, z_i, z_t, mu)
    q_bound = U.order_bound(c + 2, np.abs(y) @ np.abs(w).T + mu * np.abs(z_i) + mu * np.abs(z_t))
    assert tuple(Qt.shape) == (k, n) and np.all(np.abs(_np(Qt).T - ref_q) <= q_bound)
    # the objective: a sum of N (C + 2 K) + K C squares, each residual itself a K-term sum
    resid = y - b @ w
    terms = n * (c + 2 * k) + k * c
    ref_obj = U.objective(y, b, w, z_i, z_t, lam, mu)
    inner = 2 * (np.abs(resid) * U.order_bound(k, np.abs(y) + np.ones((n, k)) @ np.abs(w))).sum()
    o = _np(obj2)
    print(f"\ntargets ({n}, {k}, {c}): Q worst error / bound {(np.abs(_np(Qt).T - ref_q) / q_bound).max():.3f}, objective error "
          f"{abs(o[0] - ref_obj):.2e}, bound {U.order_bound(terms, ref_obj) + inner:.2e}")
    assert abs(o[0] - ref_obj) <= U.order_bound(terms, ref_obj) + inner
    zz = (z_i ** 2).sum() + (z_t ** 2).sum()
    assert abs(o[1] - zz) <= U.order_bound(2 * n * k, zz)


def test_start_center_and_covariance():
    import cmh_native as N
    rng = np.random.default_rng(3)
    za, zb = rng.standard_normal((70, 9)), rng.standard_normal((70, 9))
    za[0, 0], zb[0, 0] = 0.5, -0.5                                          # a sum of exactly zero is +1
    za[1, 1], zb[1, 1] = -0.0, 0.0
    B = N.dch_start(_dev(za), _dev(zb))
    assert B.dtype == torch.int8 and np.array_equal(_np(B), np.where(za + zb >= 0, 1, -1)) and int(B[0, 0]) == 1 and int(B[1, 1]) == 1
    d, k, n = 24, 8, 300
    t, bsum, mean = rng.standard_normal((d, k)) * n, rng.integers(-n, n, k).astype(np.float64), rng.standard_normal(d)
    alpha = np.array([0.7])
    u = _np(N.dch_center(_dev(t), _dev(bsum), _dev(mean), _dev(alpha), n))
    ref = alpha[0] * (t - np.outer(mean, bsum)) / n
    assert np.all(np.abs(u - ref) <= 8 * EPS * alpha[0] * (np.abs(t) + np.abs(np.outer(mean, bsum))) / n)
    f = (rng.standard_normal((n, d)) + 8.0).astype(np.float32)
    sums = N.itq_moments(_dev(f))
    mu_i, _, a2, _ = N.itq_covariance(sums, sums, n)
    S = N.dch_covariance(sums[1], mu_i, a2[0:1], n)
    x = f.astype(np.float64)
    cov = x.T @ x / n - np.outer(x.mean(0), x.mean(0))
    assert torch.equal(S, S.t()) and abs(float(S.diagonal().sum()) - 1.0) <= 1e-9
    assert np.abs(_np(S) - cov / np.trace(cov)).max() <= 1e-9                # the cancellation of E[f f^T] - mu mu^T at an offset of 8


# ---------------------------------------------------------------------------------------------------- end to end
ITERS, ROUNDS, MU = 5, 3, 0.01


def _ref(fix):
    return _get(("ref", fix), lambda: U.fit(*U.fixture(fix)[0], fix[3], iters=ITERS, rounds=ROUNDS, mu=MU))


def _gpu_fit(fix, cached=True):
    from utils.dch import fit_supervised_heads

    def make():
        fi, ft, y = U.fixture(fix)[0]
        return fit_supervised_heads(_dev(fi), _dev(ft), _dev(y, torch.float32), fix[3], iters=ITERS, rounds=ROUNDS, mu=MU)
    return _get(("gpu", fix), make) if cached else make()


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_fit_reproduces_the_restatements_codes(fix):
    ref, got = _ref(fix), _gpu_fit(fix)
    assert ref["min_margin"].min() >= U.MARGIN_FLOOR and ref["min_start"] >= U.MARGIN_FLOOR
    B = _np(got["B"]).astype(np.float64)
    assert B.shape == (fix[0], fix[3]) and np.array_equal(B, ref["B"]), int((B != ref["B"]).sum())
    obj = _np(got["objective"])
    assert obj.shape == (ITERS + 1,) and np.allclose(obj, ref["objective"], rtol=1e-9, atol=0)
    assert np.array_equal(_np(got["flips"]), ref["flips"])
    margins = _np(got["min_margin"])
    # t is a sum of K + C + 1 terms of size 10 at most, from W, Z and G that agree with LAPACK's to about 1e-12: 1e-10 is generous
    assert margins.min() >= U.MARGIN_FLOOR and np.abs(margins - ref["min_margin"]).max() <= 1e-10
    assert _np(got["solve_info"]).tolist() == [0] * (ITERS + 1) and got["eigh_converged"]
    assert float(got["scale"]) == pytest.approx(ref["scale"], rel=1e-9)
    assert np.abs(_np(got["W"]) - ref["W"]).max() <= 1e-9 * np.abs(ref["W"]).max()
    print(f"\nfit {fix}: objective {obj[0]:.6g} -> {obj[-1]:.6g}, flips {_np(got['flips']).sum(1).tolist()}, smallest |t| {margins.min():.2e}, "
          f"Jacobi sweeps {got['eigh_sweeps']}")
    second = _gpu_fit(fix, cached=False)
    for key in ("B", "P_i", "P_t", "W", "objective", "flips", "min_margin", "scale", "W_i", "b_i", "W_t", "b_t"):
        assert torch.equal(got[key], second[key]), key


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_streamed_moments_give_the_same_codes(fix):
    """The trainer's path: the moments arrive in batches of 128.  Only their last bits differ from the one-shot sums, and the
    fixtures' margins cover that."""
    from utils.dch import fit_from_moments, supervised_moments
    from utils.itq import MomentStream
    fi, ft, y = (_dev(a) for a in U.fixture(fix)[0])
    stream = MomentStream()
    for lo in range(0, fix[0], 128):
        stream.add(fi[lo:lo + 128], ft[lo:lo + 128])
    got = fit_from_moments(fi, ft, y.float(), supervised_moments(stream), fix[3], iters=ITERS, rounds=ROUNDS, mu=MU)
    assert torch.equal(got["B"], _gpu_fit(fix)["B"]) and torch.equal(got["flips"], _gpu_fit(fix)["flips"])


# 10 x the worst |z_head - s z_fit| measured on these fixtures on MI355X: 4.05e-6 (f32 head against the f64 fit, (1000, 64, 10, 32); the
# test prints each case's).  The heads' rounding, eps_f32 sum_d |W_kd f_d| with the offset 8 per feature: ~2e-6, as for ITQ's heads.
# tests/test_dch_host.py holds the same number and asserts that the restatement leaves at most CAP of its entries under it.
TAU = 10 * 4.05e-6
CAP = 1e-3


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_f32_heads_give_the_fits_codes(fix):
    import cmh_native as N
    from model.modelbase import LinearHash
    from utils.itq import load_heads
    n, d, _, k, _ = fix
    got = _gpu_fit(fix)
    fi, ft, _ = U.fixture(fix)[0]
    s = float(got["scale"])
    z_fit = s * np.concatenate([_np(N.itq_project(_dev(f), got[f"mu_{m}"], got["alpha"][j:j + 1], got[f"P_{m}"]))
                                for j, (m, f) in enumerate((("i", fi), ("t", ft)))])

    class Pair(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.image_hash, self.text_hash = LinearHash(d, k), LinearHash(d, k)
    pair = Pair().to(DEV).eval()
    load_heads(pair, got)                                                   # utils.itq.load_heads works on the result unchanged
    pre, codes = [], []
    for head, f in ((pair.image_hash, fi), (pair.text_hash, ft)):
        with torch.no_grad():
            x = _dev(f)
            codes.append(_np(N.sign_codes(head(x))))
            pre.append(_np(N.linear_act(x, head.fc.weight, head.fc.bias, N.ACT_NONE)).astype(np.float64))
    pre, codes = np.concatenate(pre), np.concatenate(codes)
    worst = np.abs(pre - z_fit).max()
    compared = np.abs(z_fit) > TAU
    print(f"\nheads {fix}: worst |z_head - s z_fit| {worst:.2e}, tau {TAU:.1e}, excluded share {1 - compared.mean():.2e}, "
          f"rms(pre-activation) - 0.5 = {np.sqrt((pre ** 2).mean()) - 0.5:.2e}")
    assert 1 - compared.mean() <= CAP
    assert np.array_equal(codes[compared], np.where(z_fit >= 0, 1.0, -1.0)[compared])
    assert abs(np.sqrt((pre ** 2).mean()) - 0.5) <= 1e-6
    ref = _ref(fix)
    assert np.array_equal(np.where(z_fit >= 0, 1.0, -1.0)[compared], ref["codes"][compared])
    for key in ("W_i", "W_t", "b_i", "b_t"):                                # the restatement's heads, to f32 rounding of the entries
        assert np.abs(_np(got[key]) - ref[key]).max() <= 1e-6 * np.abs(ref[key]).max(), key


# ---------------------------------------------------------------------------------------------------- the trainer and the consumers
def test_trainer_fits_saves_and_serves_queries(tmp_path, monkeypatch, capsys):
    """main.trainers["DCH"] with a tiny random CLIP state dict on the synthetic set (16 bits, 64 train items, batch 16): model-0.pth,
    which loads as DCH and as DSPH; QueryEncoder("DCH") on a caption and a picture, codes and soft outputs; retrieve.py --text
    against a saved index.  Random towers: no claim on cross-modal mAP."""
    import argparse
    import os
    import sys
    import main
    import recipe
    import retrieve
    from query import QueryEncoder
    from utils.retrieval import CodeIndex
    merges = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_bpe_merges_48894.txt.gz")
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(dict(recipe.CLIP_TINY, vocab_size=49408), 7).items()}, ck)
    run = tmp_path / "run"
    base = ["main.py", "-clip-path", str(ck), "--save-dir", str(run), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
            "--max-words", "16", "--query-num", "32", "--train-num", "64", "--synthetic-size", "128", "--dch-iters", "4"]
    monkeypatch.setattr(sys, "argv", base)
    torch.manual_seed(0)
    tr = main.trainers["DCH"](argparse.Namespace(method="DCH", dataset="synthetic", output_dim=16, is_train=True), 0)
    model_file = run / "DCH" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists()
    fit = tr.last_fit
    obj = _np(fit["objective"])
    assert fit["n"] == 64 and obj.shape == (5,) and np.all(np.isfinite(obj)) and tuple(fit["flips"].shape) == (4, 3)
    assert tuple(fit["B"].shape) == (64, 16) and set(fit["B"].unique().tolist()) <= {-1, 1} and _np(fit["solve_info"]).tolist() == [0] * 5
    state = torch.load(model_file, map_location="cpu")
    assert torch.equal(state["image_hash.fc.weight"], fit["W_i"].cpu()) and torch.equal(state["text_hash.fc.bias"], fit["b_t"].cpu())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for method in ("DCH", "DSPH"):                                          # the evaluation entry of the saved checkpoint
        monkeypatch.setattr(sys, "argv", base + ["--pretrained", str(model_file), "--save-dir", str(tmp_path / f"eval_{method}")])
        ev = main.trainers[method](argparse.Namespace(method=method, dataset="synthetic", output_dim=16, is_train=False), 0)
        maps = [float(v) for v in ev.valid(0)]
        assert len(maps) == 4 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in maps), maps
        e_img, e_txt, _ = ev.get_code(ev.query_loader, ev.args.query_num)
        assert torch.equal(e_img, q_img) and torch.equal(e_txt, q_txt)
    enc = QueryEncoder("DCH", str(model_file), str(ck), 16, max_words=16, resolution=64, bpe_path=merges)
    for batch in tr.query_loader:
        image, text, index = batch[0].to(DEV), batch[1], batch[-1]
        with torch.no_grad():
            assert torch.equal(enc.rule(enc.model.encode_image(image)), q_img[index.to(DEV)])
        assert torch.equal(enc.encode_tokens(text), q_txt[index.to(DEV)])
    caption = "a dog on a beach"
    picture = np.random.default_rng(5).integers(0, 256, (48, 80, 3), dtype=np.uint8)
    for codes, soft in ((enc.encode_text(caption), enc.encode_text(caption, soft=True)), (enc.encode_image([picture]), enc.encode_image([picture], soft=True))):
        assert tuple(codes.shape) == tuple(soft.shape) == (1, 16) and bool(torch.isfinite(soft).all())
        assert torch.equal(torch.sign(soft)[soft != 0], codes[soft != 0])
    r_img, _, _ = tr.get_code(tr.retrieval_loader, tr.args.retrieval_num)
    CodeIndex(r_img).save(tmp_path / "db.npz")
    capsys.readouterr()
    assert retrieve.main(["--text", caption, "--index", str(tmp_path / "db.npz"), "--k", "5", "--method", "DCH", "--pretrained", str(model_file),
                          "-clip-path", str(ck), "--output-dim", "16", "--max-words", "16", "--resolution", "64", "--bpe-path", merges]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    idx, dist = (t.cpu().numpy() for t in CodeIndex.load(tmp_path / "db.npz").search(enc.encode_text(caption), 5)[:2])
    assert lines[0] == f"query 0 text: {caption}" and [int(ln.split()[1]) for ln in lines[1:6]] == idx[0].tolist()
    assert [float(ln.split()[2]) for ln in lines[1:6]] == [float(f"{v:g}") for v in dist[0]]
