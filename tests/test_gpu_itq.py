"""The training-free fit on the GPU (csrc/itq.hip, utils/itq.py, train/ITQ) against the NumPy fp64 restatement of tests/itqutil.py:
every kernel on its own within the bound its arithmetic allows, the fit end to end with exact codes on the fixtures that
tests/test_itq_host.py shows robust, the f32 heads against the fit, and the trainer through main.py.

Bounds.  A sum of n terms in any order is within n eps sum|terms| of the exact one; two orders differ by twice that, and the tests
ask 8 n eps sum|terms| ("the summation-order bound").  Jacobi's backward error is a small multiple of D eps |C|_F: 64 D eps.  An
eigenvector moves by the backward error over its eigenvalue's gap, so the entrywise check on the robust fixtures allows
2 * 64 D eps |C|_F / gap_j per column (both solvers' errors).  The polar factor's condition is cond(M): 1e3 eps cond(M).

Measured on MI355X (this file's prints): see DESIGN.md, "Training-free heads"."""
import numpy as np
import pytest
import torch

import itqutil as U

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


def _pair(n, d, seed):
    return _get(("pair", n, d, seed), lambda: U.make_pair(n, d, seed))


def _ref(fix, projection="pca", rotation="itq"):
    n, d, k, seed = fix
    return _get(("ref", fix, projection, rotation), lambda: U.fit(*_pair(n, d, seed), k, projection, rotation, 50, seed=seed))


def _gpu_fit(fix, projection="pca", rotation="itq", cached=True):
    from utils.itq import fit_hash_heads
    n, d, k, seed = fix

    def make():
        fi, ft = (torch.from_numpy(a).to(DEV) for a in _pair(n, d, seed))
        return fit_hash_heads(fi, ft, k, projection, rotation, 50, seed=seed)
    return _get(("gpu", fix, projection, rotation), make) if cached else make()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------- moments
MOMENT_SHAPES = [(1, 8), (63, 24), (300, 24), (517, 40), (257, 65)]


@pytest.mark.parametrize("n,d", MOMENT_SHAPES)
def test_moments_within_the_summation_order_bound_and_bit_stable(n, d):
    import cmh_native as N
    f = _pair(n, d, 5)[0]
    s, q = N.itq_moments(_dev(f))
    s2, q2 = N.itq_moments(_dev(f))
    assert torch.equal(s, s2) and torch.equal(q, q2)
    rs, rq = U.moments(f)
    bs, bq = U.moments_bound(f)
    assert np.all(np.abs(_np(s) - rs) <= bs) and np.all(np.abs(_np(q) - rq) <= bq)
    assert torch.equal(q, q.t())                                               # symmetric bit for bit
    print(f"\nmoments ({n}, {d}): worst error / bound {max((np.abs(_np(s) - rs) / bs).max(), (np.abs(_np(q) - rq) / bq).max()):.3f}")


def test_moments_streamed_in_three_unequal_batches():
    import cmh_native as N
    n, d = 5000, 40                                                            # more than one chunk of 2048 rows in the first batch
    f = _pair(n, d, 6)[0]
    cuts = [0, 4100, 4163, n]
    sums = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        sums = N.itq_moments(_dev(f[a:b]), sums)
    again = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        again = N.itq_moments(_dev(f[a:b]), again)
    assert torch.equal(sums[0], again[0]) and torch.equal(sums[1], again[1])
    rs, rq = U.moments(f)
    bs, bq = U.moments_bound(f)
    assert np.all(np.abs(_np(sums[0]) - rs) <= bs) and np.all(np.abs(_np(sums[1]) - rq) <= bq)
    whole = N.itq_moments(_dev(f))
    assert np.all(np.abs(_np(whole[1]) - rq) <= bq)


def test_covariance_against_the_restatement():
    import cmh_native as N
    n, d, _, seed = U.FIXTURES[1]
    fi, ft = _pair(n, d, seed)
    mu_i, mu_t, alpha, cov = N.itq_covariance(N.itq_moments(_dev(fi)), N.itq_moments(_dev(ft)), n)
    r_mu_i, r_mu_t, r_alpha, r_cov = U.covariance(U.moments(fi), U.moments(ft), n)
    # C = E[f f^T] - mu mu^T cancels: the absolute error is that of the two terms, 8 N eps of their size each
    xi, xt = np.abs(fi.astype(np.float64)), np.abs(ft.astype(np.float64))
    size = 0.5 * (r_alpha[0] ** 2 * (xi.T @ xi / n + np.outer(np.abs(r_mu_i), np.abs(r_mu_i)))
                  + r_alpha[1] ** 2 * (xt.T @ xt / n + np.outer(np.abs(r_mu_t), np.abs(r_mu_t))))
    assert np.all(np.abs(_np(cov) - r_cov) <= 16 * n * EPS * size)
    assert np.abs(_np(mu_i) - r_mu_i).max() <= 8 * n * EPS * xi.mean(0).max()
    assert np.abs(_np(alpha) / r_alpha - 1).max() <= 1e-10                     # alpha's own cancellation: (mean / spread)^2 eps
    assert torch.equal(cov, cov.t())


# ---------------------------------------------------------------------------------------------------- eigen-solver
def _eigh_case(name):
    if name == "rank":
        return U.low_rank_covariance(20, 48, 3)
    if name == "repeated":
        return U.repeated_eigenvalue_matrix(33, 4)
    return U.spd_matrix(int(name), 7, decay=0.9 if int(name) <= 128 else 0.99)


@pytest.mark.parametrize("name", ["1", "2", "24", "40", "65", "128", "512", "rank", "repeated"])
def test_eigh_gap_free_checks_and_conventions(name):
    import cmh_native as N
    c = _eigh_case(name)
    evals, evecs, sweeps, converged = N.itq_eigh(_dev(c))
    w, v = _np(evals), _np(evecs)
    orth, resid, lam, bound = U.eigh_checks(c, w, v)
    print(f"\neigh {name}: D = {c.shape[0]}, sweeps {sweeps}, converged {converged}; |V^T V - I| {orth:.2e}, |C V - V L| / |C|_F {resid:.2e}, "
          f"eigenvalues against LAPACK {lam:.2e}; bound {bound:.2e}")
    assert converged and 1 <= sweeps <= 60
    assert orth <= bound and resid <= bound and lam <= bound
    assert U.conventions_hold(w, v)
    again = N.itq_eigh(_dev(c))
    assert torch.equal(again[0], evals) and torch.equal(again[1], evecs)


def test_eigh_repeated_eigenvalue_spans_the_right_spaces():
    import cmh_native as N
    c = U.repeated_eigenvalue_matrix(33, 4)
    evals, evecs, _, _ = N.itq_eigh(_dev(c))
    w, v = _np(evals), _np(evecs)
    assert np.abs(w[:3] - 3.0).max() < 1e-13 and np.abs(w[3:5] - 1.0).max() < 1e-13
    _, rv = U.eigh(c)
    for lo, hi in ((0, 3), (3, 5)):                                            # the invariant subspaces agree, whatever basis each solver picks
        proj, rproj = v[:, lo:hi] @ v[:, lo:hi].T, rv[:, lo:hi] @ rv[:, lo:hi].T
        assert np.abs(proj - rproj).max() < 1e-12


def test_eigh_reads_the_upper_triangle_and_sorts_ties_by_index():
    import cmh_native as N
    c = np.diag([2.0, 5.0, 2.0, 7.0])
    lower_garbage = c + np.tril(np.full((4, 4), 9.0), -1)
    evals, evecs, sweeps, converged = N.itq_eigh(_dev(lower_garbage))
    assert _np(evals).tolist() == [7.0, 5.0, 2.0, 2.0] and converged and sweeps == 1
    assert np.array_equal(_np(evecs), np.eye(4)[:, [3, 1, 0, 2]])              # the two 2s in index order
    a = np.array([[2.0, -1.0], [-1.0, 2.0]])
    evals, evecs, _, _ = N.itq_eigh(_dev(a))
    assert np.allclose(_np(evals), [3.0, 1.0], atol=1e-15)
    assert np.allclose(_np(evecs), np.array([[1.0, 1.0], [-1.0, 1.0]]) / np.sqrt(2), atol=1e-15)     # lowest row on a tie is positive


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_eigenvectors_match_the_restatement_on_the_robust_fixtures(fix):
    import cmh_native as N
    ref = _ref(fix)
    c = ref["C"]
    evals, evecs, _, _ = N.itq_eigh(_dev(c))
    w, v = _np(evals), _np(evecs)
    rw, rv = U.eigh(c)
    d = c.shape[0]
    gaps = np.array([np.abs(np.delete(rw, j) - rw[j]).min() for j in range(d)])
    tol = 2 * 64 * d * EPS * np.linalg.norm(c) / gaps
    err = np.abs(v - rv).max(0)
    print(f"\neigenvectors {fix}: worst entry error {err.max():.2e}, worst error / tolerance {(err / tol).max():.3f}")
    assert np.all(err <= tol)


# ---------------------------------------------------------------------------------------------------- polar factor
def _fixture_m(k, seed=9):
    """M = B^T V of a fixture-style projected set at K bits (one pass from R = I)."""
    n, d = 300, max(k, 24)
    fi, ft = U.make_pair(n, d, seed)
    ref = U.fit(fi, ft, k, "pca", "none")
    return U.step(ref["V"], np.eye(k))[2]


@pytest.mark.parametrize("k", [1, 2, 8, 16, 33, 128])
def test_polar_factor_on_fixture_matrices(k):
    import cmh_native as N
    m = _fixture_m(k)
    cond = np.linalg.cond(m)
    assert cond <= 1e6, cond
    r, sweeps = N.itq_polar(_dev(m), want_sweeps=True)
    r2 = N.itq_polar(_dev(m))
    assert torch.equal(r, r2)
    r = _np(r)
    orth, err = np.abs(r.T @ r - np.eye(k)).max(), np.abs(r - U.polar_t(m)).max()
    print(f"\npolar K = {k}: cond(M) {cond:.2e}, sweeps {int(sweeps)}, |R^T R - I| {orth:.2e} (bound {64 * k * EPS:.2e}), "
          f"|R - ref| {err:.2e} (bound {1e3 * EPS * cond:.2e})")
    assert orth <= 64 * k * EPS
    assert err <= 1e3 * EPS * cond
    assert 1 <= int(sweeps) < 60 or k == 1


def test_polar_factor_of_a_diagonal_with_mixed_signs():
    import cmh_native as N
    diag = np.array([2.0, -3.0, 0.5, -1e-3, 7.0])
    r = _np(N.itq_polar(_dev(np.diag(diag))))
    assert np.abs(r - np.diag(np.sign(diag))).max() <= 4 * EPS and np.array_equal(r != 0, np.eye(5) != 0)
    m = np.diag(diag)[:, [1, 0, 2, 4, 3]]                                     # a signed permutation is its own polar factor
    assert np.abs(_np(N.itq_polar(_dev(m))) - np.sign(m).T).max() <= 64 * 5 * EPS


@pytest.mark.parametrize("case", ["equal_rows", "rank10", "zero", "scalar_zero"])
def test_polar_factor_of_a_singular_matrix_is_still_orthogonal(case):
    """Two bits that agree on every item make B^T V singular (clustered data gets there within a few ITQ iterations).  The polar
    factor is then not unique, but R must stay orthogonal, R M must be the symmetric positive semi-definite factor, and the
    Jacobi sweeps must end on their own instead of rotating rounding noise up to the cap."""
    import cmh_native as N
    rng = np.random.default_rng(21)
    if case == "equal_rows":
        m = rng.standard_normal((8, 8))
        m[5] = m[2]
    elif case == "rank10":
        m = rng.standard_normal((16, 10)) @ rng.standard_normal((10, 16))
    elif case == "zero":
        m = np.zeros((4, 4))
    else:
        m = np.zeros((1, 1))
    k = m.shape[0]
    r, sweeps = N.itq_polar(_dev(m), want_sweeps=True)
    assert torch.equal(r, N.itq_polar(_dev(m)))
    r = _np(r)
    h = r @ m
    scale = max(np.linalg.norm(m), 1.0)
    print(f"\npolar, singular ({case}): sweeps {int(sweeps)}, |R^T R - I| {np.abs(r.T @ r - np.eye(k)).max():.2e}, |R M - (R M)^T| {np.abs(h - h.T).max():.2e}")
    assert int(sweeps) < 30
    assert np.abs(r.T @ r - np.eye(k)).max() <= 64 * k * EPS
    assert np.abs(h - h.T).max() <= 64 * k * EPS * scale
    assert np.linalg.eigvalsh((h + h.T) / 2).min() >= -64 * k * EPS * scale
    if case == "zero":
        assert np.array_equal(r, np.eye(4))


# ---------------------------------------------------------------------------------------------------- projection and one ITQ step
@pytest.mark.parametrize("n,d,k", [(300, 24, 8), (517, 40, 16), (257, 65, 33)])
def test_projection_within_the_summation_order_bound(n, d, k):
    import cmh_native as N
    fi, ft = _pair(n, d, 5)
    mu_i, _, alpha, cov = U.covariance(U.moments(fi), U.moments(ft), n)
    p = U.eigh(cov)[1][:, :k].copy()
    v = N.itq_project(_dev(fi), _dev(mu_i), _dev(alpha[0:1]), _dev(p))
    v2 = N.itq_project(_dev(fi), _dev(mu_i), _dev(alpha[0:1]), _dev(p))
    assert torch.equal(v, v2)
    x = fi.astype(np.float64) - mu_i
    bound = 8 * d * EPS * alpha[0] * (np.abs(x) @ np.abs(p))
    assert np.all(np.abs(_np(v) - U.project(fi, mu_i, alpha[0], p)) <= bound)


@pytest.mark.parametrize("n,d,k", [(300, 24, 8), (517, 40, 16), (257, 65, 33), (2300, 24, 8)])
def test_one_itq_step(n, d, k):
    import cmh_native as N
    fi, ft = _pair(n, d, 5)
    v = U.fit(fi, ft, k, "pca", "none")["V"]
    r = np.linalg.qr(np.random.default_rng(k).standard_normal((k, k)))[0]
    Z, B, M, obj2 = N.itq_step(_dev(v), _dev(r))
    again = N.itq_step(_dev(v), _dev(r))
    assert all(torch.equal(a, b) for a, b in zip((Z, B, M, obj2), again))
    rz, rb, rm, robj = U.step(v, r)
    zb = 8 * k * EPS * (np.abs(v) @ np.abs(r))
    assert np.all(np.abs(_np(Z) - rz) <= zb)
    sure = np.abs(rz) > zb
    b = _np(B).astype(np.float64)
    assert set(np.unique(b).tolist()) <= {-1.0, 1.0} and np.array_equal(b[sure], rb[sure])
    assert np.array_equal(b, np.where(_np(Z) >= 0, 1.0, -1.0))                 # B is the sign of the kernel's own Z
    rows = v.shape[0]
    mb = 8 * rows * EPS * (np.ones((k, rows)) @ np.abs(v))
    unsure = (~sure).astype(np.float64)
    assert np.all(np.abs(_np(M) - rm) <= mb + 2 * unsure.T @ np.abs(v))        # a B that may differ moves M by 2 |v|
    o = _np(obj2)
    assert abs(o[0] - robj) <= 8 * rows * k * EPS * ((1 + np.abs(rz)) ** 2).sum() + 4 * (unsure * np.abs(rz)).sum()
    assert abs(o[1] - (rz ** 2).sum()) <= 8 * rows * k * EPS * (rz ** 2).sum() + 2 * (zb * np.abs(rz)).sum()


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("projection,rotation", [("pca", "itq"), ("pca", "none"), ("random", "none")])
@pytest.mark.parametrize("fix", U.FIXTURES)
def test_fit_reproduces_the_restatements_codes(fix, projection, rotation):
    ref = _ref(fix, projection, rotation)
    got = _gpu_fit(fix, projection, rotation)
    Z = _np(got["V"]) @ _np(got["R"])
    codes = np.where(Z >= 0, 1.0, -1.0)
    assert codes.shape == ref["codes"].shape == (2 * fix[0], fix[2])
    assert np.array_equal(codes, ref["codes"]), int((codes != ref["codes"]).sum())
    obj = _np(got["objective"])
    assert obj.shape == ((51,) if rotation == "itq" else (1,))
    assert np.all(np.diff(obj) <= 1e-9 * obj[0])                               # monotone (to rounding of the sums)
    assert np.allclose(obj, ref["objective"], rtol=1e-9)
    assert float(got["scale"]) == pytest.approx(ref["scale"], rel=1e-9)
    second = _gpu_fit(fix, projection, rotation, cached=False)
    for key in ("P", "R", "V", "objective", "scale", "W_i", "b_i", "W_t", "b_t"):
        assert torch.equal(got[key], second[key]), key
    if projection == "pca":
        assert got["eigh_converged"] and torch.equal(got["evals"], second["evals"])


def test_itq_ends_at_or_below_pcah_on_the_gpu():
    for fix in U.FIXTURES:
        assert float(_gpu_fit(fix)["objective"][-1]) <= float(_gpu_fit(fix, "pca", "none")["objective"][0])
        assert float(_gpu_fit(fix)["objective"][0]) == float(_gpu_fit(fix, "pca", "none")["objective"][0])


# ---------------------------------------------------------------------------------------------------- the heads
# 10 x the worst |z_head - s z_fit| measured on these fixtures on MI355X: 3.14e-6 (f32 head against the f64 fit, (1000, 64, 32)
# random+none; the test prints each case's).  The heads' rounding, eps_f32 sum_d |W_kd f_d| with the offset 8 per feature: ~2e-6.
TAU = 10 * 3.14e-6


@pytest.mark.parametrize("projection,rotation", [("pca", "itq"), ("random", "none")])
@pytest.mark.parametrize("fix", U.FIXTURES)
def test_f32_heads_give_the_fits_codes(fix, projection, rotation):
    import cmh_native as N
    from model.modelbase import LinearHash
    n, d, k, seed = fix
    got = _gpu_fit(fix, projection, rotation)
    s = float(got["scale"])
    z_fit = s * (_np(got["V"]) @ _np(got["R"]))
    pre, codes = [], []
    for side, f in zip("it", _pair(n, d, seed)):
        head = LinearHash(d, k).to(DEV).eval()
        with torch.no_grad():
            head.fc.weight.copy_(got[f"W_{side}"])
            head.fc.bias.copy_(got[f"b_{side}"])
            x = _dev(f)
            codes.append(_np(N.sign_codes(head(x))))
            pre.append(_np(N.linear_act(x, head.fc.weight, head.fc.bias, N.ACT_NONE)).astype(np.float64))
    pre, codes = np.concatenate(pre), np.concatenate(codes)
    worst = np.abs(pre - z_fit).max()
    compared = np.abs(z_fit) > TAU
    print(f"\nheads {fix} {projection}+{rotation}: worst |z_head - s z_fit| {worst:.2e}, tau {TAU:.1e}, excluded share {1 - compared.mean():.2e}, "
          f"rms(pre-activation) - 0.5 = {np.sqrt((pre ** 2).mean()) - 0.5:.2e}")
    assert 1 - compared.mean() <= 0.01
    assert np.array_equal(codes[compared], np.where(z_fit >= 0, 1.0, -1.0)[compared])
    assert abs(np.sqrt((pre ** 2).mean()) - 0.5) <= 1e-6
    # the restatement's heads, to f32 rounding of the entries
    ref = _ref(fix, projection, rotation)
    for key in ("W_i", "W_t", "b_i", "b_t"):
        assert np.abs(_np(got[key]) - ref[key]).max() <= 1e-6 * np.abs(ref[key]).max(), key


# ---------------------------------------------------------------------------------------------------- the trainer
def test_trainer_fits_saves_and_serves_queries(tmp_path, monkeypatch):
    """main.trainers["ITQ"] with a tiny random CLIP state dict on the synthetic set (16 bits, 64 train items, batch 16): model-0.pth,
    QueryEncoder("ITQ") and QueryEncoder("DSPH") on it, test() with four finite mAPs, CodeIndex.search.  Random towers: no claim on
    cross-modal mAP."""
    import argparse
    import sys
    import main
    import recipe
    import dataset.synthetic as ds
    from query import QueryEncoder
    from utils.retrieval import CodeIndex
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510)
    monkeypatch.setattr(ds, "EOT", 511)
    run = tmp_path / "run"
    base = ["main.py", "-clip-path", str(ck), "--save-dir", str(run), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
            "--max-words", "16", "--query-num", "32", "--train-num", "64", "--synthetic-size", "128", "--itq-iters", "10"]
    monkeypatch.setattr(sys, "argv", base)
    torch.manual_seed(0)
    tr = main.trainers["ITQ"](argparse.Namespace(method="ITQ", dataset="synthetic", output_dim=16, is_train=True), 0)
    model_file = run / "ITQ" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists()
    fit = tr.last_fit
    obj = _np(fit["objective"])
    assert fit["n"] == 64 and obj.shape == (11,) and np.all(np.diff(obj) <= 1e-9 * obj[0]) and fit["eigh_converged"]
    state = torch.load(model_file, map_location="cpu")
    assert torch.equal(state["image_hash.fc.weight"], fit["W_i"].cpu()) and torch.equal(state["text_hash.fc.bias"], fit["b_t"].cpu())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for method in ("ITQ", "DSPH"):
        enc = QueryEncoder(method, str(model_file), str(ck), 16, max_words=16, resolution=64)
        for batch in tr.query_loader:
            image, text, index = batch[0].to(DEV), batch[1], batch[-1]
            with torch.no_grad():
                got_i = enc.rule(enc.model.encode_image(image))
            assert torch.equal(got_i, q_img[index.to(DEV)]) and torch.equal(enc.encode_tokens(text), q_txt[index.to(DEV)])
    # the evaluation entry of a saved checkpoint, as ITQ and as DSPH
    for method in ("ITQ", "DSPH"):
        monkeypatch.setattr(sys, "argv", base + ["--pretrained", str(model_file), "--save-dir", str(tmp_path / f"eval_{method}")])
        ev = main.trainers[method](argparse.Namespace(method=method, dataset="synthetic", output_dim=16, is_train=False), 0)
        maps = [float(v) for v in ev.valid(0)]
        assert len(maps) == 4 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in maps), maps
        e_img, e_txt, _ = ev.get_code(ev.query_loader, ev.args.query_num)
        assert torch.equal(e_img, q_img) and torch.equal(e_txt, q_txt)
    r_img, _, _ = tr.get_code(tr.retrieval_loader, tr.args.retrieval_num)
    idx, dist = CodeIndex(r_img).search(q_txt[:4], 5)
    assert tuple(idx.shape) == (4, 5) and bool((dist[:, 1:] >= dist[:, :-1]).all())
