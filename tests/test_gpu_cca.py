"""The CCA projections of the training-free fit on the GPU (csrc/itq.hip, utils/itq.py, train/ITQ with --projection cca) against the
NumPy fp64 restatement of tests/ccautil.py: the cross moments and the dense product within the bound their arithmetic allows and
bit-stable, the whitening and the canonical directions within the bounds ccautil derives from the restatement's conditioning, the
fit end to end with exact codes on the fixtures that tests/test_cca_host.py shows robust, the f32 heads against the fit, the
existing projections untouched, and the trainer through main.py.

Measured on MI355X (this file's prints): see DESIGN.md, "CCA projections"."""
import numpy as np
import pytest
import torch

import ccautil as CU
import itqutil as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = U.EPS
_CACHE = {}
E2E = [("pair",) + f for f in U.FIXTURES] + [("gap", 600, 48, 8, 7), ("gap", 600, 48, 12, 7)]


@pytest.fixture(scope="module", autouse=True)
def _release_after_module():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _get(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data(kind, n, d, seed):
    return _get(("data", kind, n, d, seed), lambda: U.make_pair(n, d, seed) if kind == "pair" else CU.gap_pair(n, d, seed))


def _ref(case, rotation="itq"):
    kind, n, d, k, seed = case
    return _get(("ref", case, rotation), lambda: CU.fit(*_data(kind, n, d, seed), k, rotation, 50))


def _gpu_fit(case, rotation="itq", cached=True):
    from utils.itq import fit_hash_heads
    kind, n, d, k, seed = case

    def make():
        fi, ft = (torch.from_numpy(a).to(DEV) for a in _data(kind, n, d, seed))
        return fit_hash_heads(fi, ft, k, "cca", rotation, 50)
    return _get(("gpu", case, rotation), make) if cached else make()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------- cross moments
@pytest.mark.parametrize("n,d", [(1, 1), (2047, 24), (2049, 65), (4100, 40)])       # 1, 1, 2 and 3 chunks of 2048 rows
def test_cross_moments_within_the_summation_order_bound_and_bit_stable(n, d):
    import cmh_native as N
    fi, ft = _data("pair", n, d, 5)
    x, x2 = N.itq_cross_moments(_dev(fi), _dev(ft)), N.itq_cross_moments(_dev(fi), _dev(ft))
    assert torch.equal(x, x2) and tuple(x.shape) == (d, d)
    ref, bound = CU.cross_moment(fi, ft), CU.cross_bound(fi, ft)
    assert np.all(np.abs(_np(x) - ref) <= bound)
    print(f"\ncross moments ({n}, {d}): worst error / bound {(np.abs(_np(x) - ref) / bound).max():.4f}")
    # the transposed pairing is the transposed sum, bit for bit: the same products in the same row order
    assert torch.equal(N.itq_cross_moments(_dev(ft), _dev(fi)), x.t())


def test_cross_moments_streamed_in_three_unequal_batches():
    import cmh_native as N
    n, d = 5000, 40                                                            # more than one chunk of 2048 rows in the first batch
    fi, ft = _data("pair", n, d, 6)
    cuts = [0, 4100, 4163, n]

    def streamed():
        x = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            x = N.itq_cross_moments(_dev(fi[a:b]), _dev(ft[a:b]), x)
        return x
    x = streamed()
    assert torch.equal(x, streamed())
    ref, bound = CU.cross_moment(fi, ft), CU.cross_bound(fi, ft)
    whole = _np(N.itq_cross_moments(_dev(fi), _dev(ft)))
    assert np.all(np.abs(_np(x) - ref) <= bound) and np.all(np.abs(whole - ref) <= bound) and np.all(np.abs(_np(x) - whole) <= bound)


def test_cca_covariances_against_the_restatement():
    import cmh_native as N
    from utils.itq import MomentStream
    kind, n, d, _, seed = E2E[1]
    fi, ft = _data(kind, n, d, seed)
    mu_i, mu_t, alpha, s_ii, s_tt, s_it = MomentStream(cross=True).add(_dev(fi), _dev(ft)).finish_cca()
    r_mu_i, r_mu_t, r_alpha, r_ii, r_tt, r_it = CU.covariances(fi, ft)
    # S = alpha alpha' (E[f f'^T] - mu mu'^T) cancels: the absolute error is that of the two terms, 8 N eps of their size each
    xi, xt = np.abs(fi.astype(np.float64)), np.abs(ft.astype(np.float64))
    for got, ref, a, x, y, mx, my in ((s_ii, r_ii, r_alpha[0] ** 2, xi, xi, r_mu_i, r_mu_i), (s_tt, r_tt, r_alpha[1] ** 2, xt, xt, r_mu_t, r_mu_t),
                                      (s_it, r_it, r_alpha[0] * r_alpha[1], xi, xt, r_mu_i, r_mu_t)):
        size = a * (x.T @ y / n + np.outer(np.abs(mx), np.abs(my)))
        assert np.all(np.abs(_np(got) - ref) <= 16 * n * EPS * size)
    assert torch.equal(s_ii, s_ii.t()) and torch.equal(s_tt, s_tt.t()) and not torch.equal(s_it, s_it.t())
    assert abs(float(s_ii.diagonal().sum()) - 1) <= 1e-10 and abs(float(s_tt.diagonal().sum()) - 1) <= 1e-10
    # mu and alpha are the pooled path's, bit for bit
    p_mu_i, p_mu_t, p_alpha, _ = MomentStream().add(_dev(fi), _dev(ft)).finish()
    assert torch.equal(mu_i, p_mu_i) and torch.equal(mu_t, p_mu_t) and torch.equal(alpha, p_alpha)


# ---------------------------------------------------------------------------------------------------- the dense product
@pytest.mark.parametrize("m,n,kc", [(1, 1, 1), (63, 65, 17), (64, 64, 16), (65, 129, 33), (129, 8, 128)])
def test_dense_product_in_all_four_layouts_with_and_without_the_diagonal(m, n, kc):
    import cmh_native as N
    rng = np.random.default_rng(m + 7 * n + 31 * kc)
    a, b, d, cs = rng.standard_normal((m, kc)), rng.standard_normal((kc, n)), rng.standard_normal(kc), rng.standard_normal(n)
    worst = 0.0
    for diag in (None, d):
        ref = (a if diag is None else a * diag) @ b
        bound = 8 * kc * EPS * ((np.abs(a) if diag is None else np.abs(a * diag)) @ np.abs(b))
        dd = None if diag is None else _dev(diag)
        plain = N.itq_matmul(_dev(a), _dev(b), d=dd)
        for ta in (False, True):
            for tb in (False, True):
                sa, sb = _dev(a.T if ta else a), _dev(b.T if tb else b)
                got = N.itq_matmul(sa, sb, d=dd, trans_a=ta, trans_b=tb)
                assert tuple(got.shape) == (m, n)
                assert torch.equal(got, N.itq_matmul(sa, sb, d=dd, trans_a=ta, trans_b=tb))              # repetition
                assert torch.equal(got, plain), (ta, tb)                      # a transposed operand = its materialised transpose
                err = np.abs(_np(got) - ref)
                assert np.all(err <= bound), (ta, tb, diag is not None)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        scaled = N.itq_matmul(_dev(a), _dev(b), d=dd, col_scale=_dev(cs))
        assert np.all(np.abs(_np(scaled) - ref * cs) <= (bound + EPS * np.abs(ref)) * np.abs(cs))
        # A diag A^T is symmetric bit for bit, from either layout
        for stored, ta in ((a, False), (a.T, True)):
            sym = N.itq_matmul(_dev(stored), _dev(stored), d=dd, trans_a=ta, trans_b=not ta)
            assert tuple(sym.shape) == (m, m) and torch.equal(sym, sym.t())
    print(f"\ndense product ({m}, {n}, {kc}): worst error / bound {worst:.4f}")


def test_inverse_square_roots():
    import cmh_native as N
    v = np.array([4.0, 1.0, 0.25, 2.0 ** -100, 0.0, -1e-15, -2.0])
    out, root = N.itq_inv_sqrt(_dev(v), 0.0, want_root=True)
    assert _np(out).tolist() == [0.5, 1.0, 2.0, 2.0 ** 50, 0.0, 0.0, 0.0] and _np(root).tolist() == [2.0, 1.0, 0.5, 2.0 ** -50, 0.0, 0.0, 0.0]
    shifted = _np(N.itq_inv_sqrt(_dev(v), 0.01))
    assert np.abs(shifted[:6] * np.sqrt(v[:6] + 0.01) - 1).max() <= 4 * EPS and shifted[6] == 0.0


# ---------------------------------------------------------------------------------------------------- whitening and canonical directions
@pytest.mark.parametrize("n,d,k,seed", U.FIXTURES + [(30, 48, 8, 4), (2000, 512, 64, 5)])
def test_whitening_and_canonical_directions(n, d, k, seed):
    """From the restatement's covariances (uploaded), so that both sides start from the same numbers: the identities of
    tests/test_cca_host.py on the GPU's outputs and the correlations against LAPACK's SVD, within ccautil's bounds."""
    from utils.itq import cca_directions
    fi, ft = _data("pair", n, d, seed)
    mu_i, mu_t, alpha, s_ii, s_tt, s_it = CU.covariances(fi, ft)
    ref = CU.directions(s_ii, s_tt, s_it, k)
    ref.update(S_ii=s_ii, S_tt=s_tt)
    got = cca_directions(_dev(s_ii), _dev(s_tt), _dev(s_it), k)
    again = cca_directions(_dev(s_ii), _dev(s_tt), _dev(s_it), k)
    for key in ("P_i", "P_t", "correlations", "H_i", "H_t", "T", "U"):
        assert torch.equal(got[key], again[key]), key
    assert got["eigh_converged"] and all(1 <= s <= 60 for s in got["eigh_sweeps"])
    r, eye = ref["r"], np.eye(d)
    h_i, h_t, p_i, p_t, sigma = (_np(got[key]) for key in ("H_i", "H_t", "P_i", "P_t", "correlations"))
    wb_i, wb_t = CU.whiten_bound(s_ii, ref["lam_i"], r), CU.whiten_bound(s_tt, ref["lam_t"], r)
    b_i, b_t, b_corr, b_sigma = CU.direction_bounds(ref, k)
    w_i, w_t = np.abs(h_i @ (s_ii + r * eye) @ h_i - eye).max(), np.abs(h_t @ (s_tt + r * eye) @ h_t - eye).max()
    o_i = np.abs(p_i.T @ (s_ii + r * eye) @ p_i - np.eye(k)).max()
    o_t = np.abs(p_t.T @ (s_tt + r * eye) @ p_t - np.eye(k)).max()
    corr = np.abs(p_i.T @ s_it @ p_t - np.diag(sigma[:k])).max()
    sig = np.abs(sigma[:k] - ref["sigma"][:k]).max()
    print(f"\ncca directions (N, D, K) = ({n}, {d}, {k}): kappa {CU.kappa(ref['lam_i'], r):.1f} / {CU.kappa(ref['lam_t'], r):.1f}, sweeps {got['eigh_sweeps']}, "
          f"sigma_1 {sigma[0]:.4f}, sigma_K {sigma[k - 1]:.4f}; |H(S+rI)H - I| {w_i:.2e} / {w_t:.2e} (bounds {wb_i:.2e} / {wb_t:.2e}), "
          f"|P^T(S+rI)P - I| {o_i:.2e} / {o_t:.2e} (bounds {b_i:.2e} / {b_t:.2e}), |P_i^T S_it P_t - diag sigma| {corr:.2e} (bound {b_corr:.2e}), "
          f"|sigma - ref| {sig:.2e} (bound {b_sigma:.2e})")
    assert w_i <= wb_i and w_t <= wb_t
    assert o_i <= b_i and o_t <= b_t
    assert corr <= b_corr
    assert sig <= b_sigma
    assert torch.equal(got["H_i"], got["H_i"].t()) and torch.equal(got["H_t"], got["H_t"].t())      # a b d: symmetric bit for bit
    assert np.all(np.diff(sigma) <= 0) and np.all(sigma >= 0)
    u = _np(got["U"])
    for j in range(k):
        assert u[int(np.argmax(np.abs(u[:, j]))), j] > 0


def test_more_bits_than_correlated_directions_is_refused_with_the_count():
    from utils.itq import fit_hash_heads
    fi, ft = (_dev(a) for a in CU.rank5_pair())
    with pytest.raises(ValueError, match=r"cca: 5 canonical directions .* 16 bits were asked"):
        fit_hash_heads(fi, ft, 16, "cca")
    assert tuple(fit_hash_heads(fi, ft, 5, "cca")["W_i"].shape) == (5, 24)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("rotation", ["itq", "none"])
@pytest.mark.parametrize("case", E2E)
def test_fit_reproduces_the_restatements_codes(case, rotation):
    ref, got = _ref(case, rotation), _gpu_fit(case, rotation)
    n, k = case[1], case[3]
    Z = _np(got["V"]) @ _np(got["R"])
    codes = np.where(Z >= 0, 1.0, -1.0)
    assert codes.shape == ref["codes"].shape == (2 * n, k)
    assert np.array_equal(codes, ref["codes"]), int((codes != ref["codes"]).sum())
    obj = _np(got["objective"])
    assert obj.shape == ((51,) if rotation == "itq" else (1,))
    assert np.all(np.diff(obj) <= 1e-9 * obj[0])
    assert np.allclose(obj, ref["objective"], rtol=1e-9)
    assert float(got["scale"]) == pytest.approx(ref["scale"], rel=1e-9)
    assert np.abs(_np(got["correlations"])[:k] - ref["sigma"][:k]).max() <= 1e-9
    assert got["reg"] == 0.1 and got["n"] == n and got["eigh_converged"] and len(got["eigh_sweeps"]) == 3
    assert tuple(got["correlations"].shape) == (case[2],) and "P" not in got
    second = _gpu_fit(case, rotation, cached=False)
    tensors = [key for key, v in got.items() if torch.is_tensor(v)]
    assert set(tensors) == {"mu_i", "mu_t", "alpha", "P_i", "P_t", "correlations", "R", "V", "objective", "scale", "W_i", "b_i", "W_t", "b_t"}
    for key in tensors:
        assert torch.equal(got[key], second[key]), key
    assert got["eigh_sweeps"] == second["eigh_sweeps"]


@pytest.mark.parametrize("k", [8, 12])
def test_pair_agreement_on_the_gap_fixture(k):
    from utils.code_stats import code_stats
    case = ("gap", 600, 48, k, 7)
    ref, got = _ref(case), _gpu_fit(case)
    codes = torch.where(got["V"] @ got["R"] >= 0, 1.0, -1.0).float()
    agree = CU.pair_agreement(_np(codes))
    assert agree == CU.pair_agreement(ref["codes"]) and agree >= 0.95
    stats = code_stats(codes[:600].contiguous(), paired=codes[600:].contiguous())
    assert stats["mean_agreement"] == pytest.approx(agree, abs=1e-12)
    print(f"\ngap fixture, {k} bits: pair agreement of the GPU's cca+itq codes {agree:.4f}")


# 10 x the worst |z_head - s z_fit| measured on these fixtures on MI355X: 6.65e-6 (f32 head against the f64 fit, (1000, 64, 32); the
# test prints each case's).  The heads' rounding, eps_f32 sum_d |W_kd f_d| with the offset 8 per feature, is of that size.
TAU = 10 * 6.65e-6


@pytest.mark.parametrize("case", E2E)
def test_f32_heads_give_the_fits_codes(case):
    import cmh_native as N
    from model.modelbase import LinearHash
    kind, n, d, k, seed = case
    got = _gpu_fit(case)
    s = float(got["scale"])
    z_fit = s * (_np(got["V"]) @ _np(got["R"]))
    pre, codes = [], []
    for side, f in zip("it", _data(kind, n, d, seed)):
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
    print(f"\ncca heads {case}: worst |z_head - s z_fit| {worst:.2e}, tau {TAU:.1e}, excluded share {1 - compared.mean():.2e}, "
          f"rms(pre-activation) - 0.5 = {np.sqrt((pre ** 2).mean()) - 0.5:.2e}")
    assert 1 - compared.mean() <= 0.01
    assert np.array_equal(codes[compared], np.where(z_fit >= 0, 1.0, -1.0)[compared])
    assert abs(np.sqrt((pre ** 2).mean()) - 0.5) <= 1e-6
    ref = _ref(case)
    for key in ("W_i", "W_t", "b_i", "b_t"):
        assert np.abs(_np(got[key]) - ref[key]).max() <= 1e-6 * np.abs(ref[key]).max(), key
    assert not torch.equal(got["W_i"], got["W_t"])


def test_heads_pair_with_one_projection_is_the_existing_entry_bit_for_bit():
    import cmh_native as N
    got = _gpu_fit(E2E[0])
    n, k = E2E[0][1], E2E[0][3]
    zz = (got["V"] @ got["R"]).square().sum().reshape(1)
    one = N.itq_heads(got["P_i"], got["R"], got["mu_i"], got["mu_t"], got["alpha"], zz, 2 * n)
    pair = N.itq_heads_pair(got["P_i"], got["P_i"], got["R"], got["mu_i"], got["mu_t"], got["alpha"], zz, 2 * n)
    assert all(torch.equal(a, b) for a, b in zip(one, pair))
    both = N.itq_heads_pair(got["P_i"], got["P_t"], got["R"], got["mu_i"], got["mu_t"], got["alpha"], zz, 2 * n)
    assert torch.equal(both[0], one[0]) and torch.equal(both[1], one[1]) and not torch.equal(both[2], one[2])
    assert tuple(both[2].shape) == (k, E2E[0][2])


# ---------------------------------------------------------------------------------------------------- the existing projections
def test_pca_fit_is_the_same_bits_whether_or_not_the_stream_kept_the_cross_sum():
    from utils.itq import MomentStream, fit_from_moments, fit_hash_heads
    n, d, k, seed = U.FIXTURES[0]
    fi, ft = (_dev(a) for a in _data("pair", n, d, seed))
    plain = fit_hash_heads(fi, ft, k, "pca", "itq", 50)
    stream = MomentStream(cross=True).add(fi, ft)
    with_cross = fit_from_moments(fi, ft, stream.finish(), k, "pca", "itq", 50)
    for key in ("W_i", "b_i", "W_t", "b_t", "P", "R", "V", "objective", "evals"):
        assert torch.equal(plain[key], with_cross[key]), key
    assert stream.cross is not None and MomentStream().add(fi, ft).cross is None


# ---------------------------------------------------------------------------------------------------- the trainer
def test_trainer_fits_saves_and_serves_queries(tmp_path, monkeypatch, caplog):
    """main.trainers["ITQ"] with --projection cca and a tiny random CLIP state dict on the synthetic set (16 bits, 64 train items,
    batch 16): the log's correlations, model-0.pth, the checkpoint as --method DSPH --is-train false, QueryEncoder("ITQ").  Random
    towers: no claim on cross-modal mAP."""
    import argparse
    import logging
    import sys
    import main
    import recipe
    import dataset.synthetic as ds
    from query import QueryEncoder
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510)
    monkeypatch.setattr(ds, "EOT", 511)
    run = tmp_path / "run"
    base = ["main.py", "-clip-path", str(ck), "--save-dir", str(run), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
            "--max-words", "16", "--query-num", "32", "--train-num", "64", "--synthetic-size", "128", "--itq-iters", "10"]
    monkeypatch.setattr(sys, "argv", base + ["--projection", "cca"])
    torch.manual_seed(0)
    with caplog.at_level(logging.INFO):
        tr = main.trainers["ITQ"](argparse.Namespace(method="ITQ", dataset="synthetic", output_dim=16, is_train=True), 0)
    model_file = run / "ITQ" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists()
    fit = tr.last_fit
    obj = _np(fit["objective"])
    assert fit["n"] == 64 and obj.shape == (11,) and np.all(np.diff(obj) <= 1e-9 * obj[0]) and fit["eigh_converged"]
    sigma = _np(fit["correlations"])
    assert sigma.shape == (64,) and np.all(np.diff(sigma) <= 0) and 0 < sigma[15] <= sigma[0] < 1
    logged = [r.getMessage() for r in caplog.records if "canonical correlations kept" in r.getMessage()]
    log_file_text = "".join(open(p).read() for p in run.rglob("*.log"))
    assert logged or "canonical correlations kept" in log_file_text
    assert f"first {sigma[0]:.6f}, last {sigma[15]:.6f}, mean {sigma[:16].mean():.6f}" in ("".join(logged) + log_file_text)
    state = torch.load(model_file, map_location="cpu")
    assert torch.equal(state["image_hash.fc.weight"], fit["W_i"].cpu()) and torch.equal(state["text_hash.fc.bias"], fit["b_t"].cpu())
    w_i, w_t = fit["W_i"].double().flatten(), fit["W_t"].double().flatten()
    cosine = float(torch.dot(w_i, w_t) / (w_i.norm() * w_t.norm()))
    assert abs(cosine) < 0.999, cosine                                         # W_i is not a multiple of W_t
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    enc = QueryEncoder("ITQ", str(model_file), str(ck), 16, max_words=16, resolution=64)
    for batch in tr.query_loader:
        image, text, index = batch[0].to(DEV), batch[1], batch[-1]
        with torch.no_grad():
            got_i = enc.rule(enc.model.encode_image(image))
        assert torch.equal(got_i, q_img[index.to(DEV)]) and torch.equal(enc.encode_tokens(text), q_txt[index.to(DEV)])
    monkeypatch.setattr(sys, "argv", base + ["--pretrained", str(model_file), "--save-dir", str(tmp_path / "eval_DSPH")])
    ev = main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
    e_img, e_txt, _ = ev.get_code(ev.query_loader, ev.args.query_num)
    assert torch.equal(e_img, q_img) and torch.equal(e_txt, q_txt)
