"""CPU checks around the CCA projections of the training-free fit (csrc/itq.hip, utils/itq.py, projection="cca"): the fixtures'
robustness (the condition that lets tests/test_gpu_cca.py ask for exact codes), the restatement's own properties (tests/ccautil.py),
what the feature is for as a property of the gap fixture, the flags, and the host-side refusals of every new entry point (nothing
is launched, so no GPU is needed)."""
import argparse
import re
import sys

import numpy as np
import pytest

import ccautil as CU
import itqutil as U
from conftest import ROOT

NEW = ["cmh_itq_heads_pair", "cmh_itq_cross_moments_workspace_bytes", "cmh_itq_cross_moments", "cmh_itq_cca_covariance", "cmh_itq_inv_sqrt",
       "cmh_itq_matmul"]
CASES = [("pair", n, d, k, seed) for n, d, k, _ in U.FIXTURES for seed in (1, 2, 3)] \
    + [("gap", 600, 48, k, seed) for k in CU.GAP_BITS for seed in CU.GAP_SEEDS]
_DATA, _FITS = {}, {}


def _data(kind, n, d, seed):
    if (kind, n, d, seed) not in _DATA:
        _DATA[(kind, n, d, seed)] = U.make_pair(n, d, seed) if kind == "pair" else CU.gap_pair(n, d, seed)
    return _DATA[(kind, n, d, seed)]


def _fit(kind, n, d, k, seed, rotation="itq"):
    key = (kind, n, d, k, seed, rotation)
    if key not in _FITS:
        _FITS[key] = CU.fit(*_data(kind, n, d, seed), k, rotation, 50)
    return _FITS[key]


# ---------------------------------------------------------------------------------------------------- the restatement and its fixtures
@pytest.mark.parametrize("kind,n,d,k,seed", CASES)
def test_fixture_codes_survive_perturbed_covariances(kind, n, d, k, seed):
    """The restatement rerun with S_ii, S_tt, S_it + 1e-10 max|S| of noise gives the same codes for all 2N rows, over 50 ITQ
    iterations and without a rotation."""
    fi, ft = _data(kind, n, d, seed)
    for rotation in ("itq", "none"):
        base = _fit(kind, n, d, k, seed, rotation)
        for noise_seed in (11, 12):
            other = CU.fit(fi, ft, k, rotation, 50, perturb=(1e-10, noise_seed))
            assert np.array_equal(base["codes"], other["codes"]), (rotation, noise_seed, int((base["codes"] != other["codes"]).sum()))
    z, sig = _fit(kind, n, d, k, seed)["Z"], _fit(kind, n, d, k, seed)["sigma"][:k]
    print(f"\n{kind} (N, D, K) = ({n}, {d}, {k}), seed {seed}: min|Z| / rms(Z) = {np.abs(z).min() / np.sqrt((z ** 2).mean()):.2e}, "
          f"smallest gap between kept correlations {np.abs(np.diff(sig)).min():.2e}, sigma_1 {sig[0]:.4f}, sigma_K {sig[-1]:.4f}")


@pytest.mark.parametrize("kind,n,d,k,seed", [("pair",) + f for f in U.FIXTURES] + [("gap", 600, 48, 12, 7), ("pair", 30, 48, 8, 4)])
def test_restatement_properties(kind, n, d, k, seed):
    fi, ft = _data(kind, n, d, seed)
    ref = _fit(kind, n, d, k, seed)
    obj = ref["objective"]
    assert obj.shape == (51,) and np.all(np.diff(obj) <= 1e-9 * obj[0]), np.diff(obj).max()
    r, eye = ref["r"], np.eye(d)
    assert r == pytest.approx(0.1 / d)
    assert np.trace(ref["S_ii"]) == pytest.approx(1.0, abs=1e-12) and np.trace(ref["S_tt"]) == pytest.approx(1.0, abs=1e-12)
    for side, s in (("i", ref["S_ii"]), ("t", ref["S_tt"])):
        h, p = ref[f"H_{side}"], ref[f"P_{side}"]
        assert np.abs(h @ (s + r * eye) @ h - eye).max() < 1e-10
        assert np.abs(p.T @ (s + r * eye) @ p - np.eye(k)).max() < 1e-10
    assert np.abs(ref["P_i"].T @ ref["S_it"] @ ref["P_t"] - np.diag(ref["sigma"][:k])).max() < 1e-10
    assert np.all(np.diff(ref["sigma"]) <= 0) and ref["sigma"][0] < 1.0
    for j in range(k):
        assert ref["U"][int(np.argmax(np.abs(ref["U"][:, j]))), j] > 0
    # the heads restate the fit
    pre = np.concatenate([fi.astype(np.float64) @ ref["W_i"].T + ref["b_i"], ft.astype(np.float64) @ ref["W_t"].T + ref["b_t"]])
    assert np.abs(pre - ref["scale"] * ref["Z"]).max() < 1e-9
    assert np.sqrt((pre ** 2).mean()) == pytest.approx(0.5, abs=1e-9)
    # the T T^T route: the eigenvectors of G with the product's sign rule are LAPACK's left singular vectors on the kept directions
    g = ref["T"] @ ref["T"].T
    w, u = U.eigh(g)
    assert np.abs(np.sqrt(np.maximum(w[:k], 0)) - ref["sigma"][:k]).max() < 1e-12
    assert np.abs(u[:, :k] - ref["U"][:, :k]).max() < 1e-9
    v = ref["T"].T @ u[:, :k] / np.sqrt(w[:k])
    assert np.abs(v - ref["Vfull"][:, :k]).max() < 1e-9 and np.abs(v.T @ v - np.eye(k)).max() < 1e-12


def test_the_default_ridge_keeps_a_fit_with_fewer_pairs_than_dimensions_away_from_saturation():
    fi, ft = _data("pair", 30, 48, 4)
    mu_i, mu_t, alpha, s_ii, s_tt, s_it = CU.covariances(fi, ft)
    default, tiny = CU.directions(s_ii, s_tt, s_it, 8)["sigma"], CU.directions(s_ii, s_tt, s_it, 8, reg=1e-3)["sigma"]
    print(f"\nN = 30, D = 48: leading correlations at reg 0.1 {default[:3]}, at reg 1e-3 {tiny[:3]}")
    assert default[0] < 0.999 and tiny[0] > 0.999


# ---------------------------------------------------------------------------------------------------- what the feature is for
@pytest.mark.parametrize("k", CU.GAP_BITS)
@pytest.mark.parametrize("seed", CU.GAP_SEEDS)
def test_pooled_pca_is_at_chance_on_the_gap_fixture_and_cca_is_not(seed, k):
    fi, ft = _data("gap", 600, 48, seed)
    pca = CU.pair_agreement(U.fit(fi, ft, k, "pca", "itq", 50)["codes"])
    cca = CU.pair_agreement(_fit("gap", 600, 48, k, seed)["codes"])
    print(f"\ngap fixture seed {seed}, {k} bits: pair agreement pca+itq {pca:.3f}, cca+itq {cca:.3f}")
    assert pca <= 0.55
    assert cca >= 0.95


# ---------------------------------------------------------------------------------------------------- flags and refusals of the fit
def _args(monkeypatch, *cli):
    from train.ITQ.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", *cli])
    return get_args(argparse.Namespace(method="ITQ", dataset="synthetic", output_dim=16, is_train=True))


def test_flags(monkeypatch):
    a = _args(monkeypatch, "--projection", "cca", "--cca-reg", "0.5")
    assert (a.projection, a.cca_reg, a.rotation, a.itq_iters) == ("cca", 0.5, "itq", 50)
    b = _args(monkeypatch)
    assert (b.projection, b.rotation, b.itq_iters, b.fit_num, b.cca_reg) == ("pca", "itq", 50, 0, 0.1)
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--projection", "svd")
    from utils.itq import CCA_FLOOR, CCA_REG, PROJECTIONS
    assert PROJECTIONS == ("pca", "random", "cca") and CCA_REG == 0.1 and CCA_FLOOR == CU.FLOOR


def test_the_ridge_must_be_positive_and_the_moments_must_carry_the_cross_sum():
    import torch
    from utils.itq import MomentStream, fit_from_moments, fit_hash_heads
    f = torch.zeros(4, 8)
    for reg in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="reg"):
            fit_from_moments(f, f, None, 4, projection="cca", reg=reg)
        with pytest.raises(ValueError, match="reg"):
            fit_hash_heads(f, f, 4, projection="cca", reg=reg)
        with pytest.raises(ValueError, match="reg"):
            CU.directions(np.eye(4), np.eye(4), np.eye(4), 2, reg=reg)
    with pytest.raises(ValueError, match="projection"):
        fit_from_moments(f, f, None, 4, projection="svd")
    with pytest.raises(ValueError, match="bits = 9"):
        fit_from_moments(f, f, None, 9, projection="cca")
    with pytest.raises(ValueError, match="cross"):
        fit_from_moments(f, f, (None,) * 4, 4, projection="cca")
    with pytest.raises(ValueError, match="cross"):
        MomentStream().finish_cca()


def test_a_non_positive_ridge_is_refused_by_the_trainer_before_any_data(monkeypatch, tmp_path):
    import main
    monkeypatch.setattr(sys, "argv", ["main.py", "--projection", "cca", "--cca-reg", "0", "--save-dir", str(tmp_path / "run"),
                                      "--data-dir", str(tmp_path / "missing")])
    with pytest.raises(ValueError, match="cca-reg"):
        main.trainers["ITQ"](argparse.Namespace(method="ITQ", dataset="flickr", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


def test_more_bits_than_correlated_directions_is_refused_with_the_count():
    fi, ft = CU.rank5_pair()
    assert fi.shape == (64, 24)
    assert np.array_equal(fi, np.round(fi)) and np.abs(fi.mean(0)).max() == 0.0 and np.abs(ft.mean(0)).max() == 0.0
    mu_i, mu_t, alpha, s_ii, s_tt, s_it = CU.covariances(fi, ft)
    sigma = CU.directions(s_ii, s_tt, s_it, 5)["sigma"]
    print(f"\nrank-5 fixture: sigma_5 / sigma_1 = {sigma[4] / sigma[0]:.3e}, sigma_6 / sigma_1 = {sigma[5] / sigma[0]:.3e}")
    assert sigma[5] / sigma[0] < 1e-8 and sigma[4] / sigma[0] > 1e-2
    with pytest.raises(ValueError, match=r"cca: 5 canonical directions .* 16 bits were asked"):
        CU.fit(fi, ft, 16)
    assert CU.fit(fi, ft, 5)["codes"].shape == (128, 5)


# ---------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_in_binding_and_header():
    import os
    import cmh_native as N
    raw = open(os.path.join(ROOT, "include", "cmh.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name             # one ctypes row per parameter
    assert N.ABI_VERSION == 6
    src = open(os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "cmh_native.py")).read()
    for name in NEW:
        assert re.search(r'"%s":.*no upstream counterpart' % name, src), name


def test_workspace_query():
    import cmh_native as N
    q = N.lib().cmh_itq_cross_moments_workspace_bytes
    assert q(1, 8) >= 8 * 8 * 8 and q(5000, 512) >= 3 * 512 * 512 * 8 and q(300, 24) % 256 == 0
    for rows, size in ((0, 8), (-1, 8), (8, 0), (8, -3), (8, 1025), (65535 * 2048 + 1, 8)):
        assert q(rows, size) == 0


def test_host_side_refusals_before_any_launch():
    """Null pointers, D = 0 and 1025, K = 0, K > D and 129, N = 0, and a workspace one byte short: CMH_ERR_INVALID with a message that
    names the call, and nothing launched (the pointers are not addresses of anything)."""
    import cmh_native as N
    lib = N.lib()
    one, big = 1, 1 << 40

    def refused(rc, *words):
        msg = lib.cmh_last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    # cross moments
    for n, d in ((0, 8), (8, 0), (8, 1025)):
        refused(lib.cmh_itq_cross_moments(one, one, n, d, one, 0, one, big, None), b"itq_cross_moments", b"need")
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        refused(lib.cmh_itq_cross_moments(ptrs[0], ptrs[1], 8, 8, ptrs[2], 0, ptrs[3], big, None), b"itq_cross_moments", b"null")
    refused(lib.cmh_itq_cross_moments(one, one, 300, 24, one, 0, one, lib.cmh_itq_cross_moments_workspace_bytes(300, 24) - 1, None),
            b"itq_cross_moments", b"workspace")
    # covariances
    for n, d in ((0, 8), (8, 0), (8, 1025)):
        refused(lib.cmh_itq_cca_covariance(*([one] * 5), n, d, *([one] * 6), None), b"itq_cca_covariance", b"need")
    for hole in range(11):
        ptrs = [one] * 11
        ptrs[hole] = None
        refused(lib.cmh_itq_cca_covariance(*ptrs[:5], 8, 8, *ptrs[5:], None), b"itq_cca_covariance", b"null")
    # the spectrum vectors
    for n in (0, -1, 1025):
        refused(lib.cmh_itq_inv_sqrt(one, n, 0.1, one, None, None), b"itq_inv_sqrt", b"need")
    for shift in (-1e-3, float("nan")):
        refused(lib.cmh_itq_inv_sqrt(one, 8, shift, one, None, None), b"itq_inv_sqrt", b"shift")
    refused(lib.cmh_itq_inv_sqrt(None, 8, 0.1, one, None, None), b"itq_inv_sqrt", b"null")
    refused(lib.cmh_itq_inv_sqrt(one, 8, 0.1, None, one, None), b"itq_inv_sqrt", b"null")
    # the dense product
    two = 2
    for m, n, kc in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (-1, 8, 8)):
        refused(lib.cmh_itq_matmul(one, one, None, None, m, n, kc, 0, 0, two, None), b"itq_matmul", b"need")
    for ta, tb in ((2, 0), (0, -1)):
        refused(lib.cmh_itq_matmul(one, one, None, None, 8, 8, 8, ta, tb, two, None), b"itq_matmul", b"need")
    for a, b, c in ((None, one, two), (one, None, two), (one, one, None)):
        refused(lib.cmh_itq_matmul(a, b, None, None, 8, 8, 8, 0, 0, c, None), b"itq_matmul", b"null")
    refused(lib.cmh_itq_matmul(one, two, None, None, 8, 8, 8, 0, 0, one, None), b"itq_matmul", b"operand")
    refused(lib.cmh_itq_matmul(one, two, None, None, 8, 8, 8, 0, 0, two, None), b"itq_matmul", b"operand")
    # heads with one projection per modality
    for rows, d, k in ((0, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 9), (8, 512, 129)):
        refused(lib.cmh_itq_heads_pair(*([one] * 7), rows, d, k, one, one, one, one, None, None), b"itq_heads", b"need")
    for hole in range(11):
        ptrs = [one] * 11
        ptrs[hole] = None
        refused(lib.cmh_itq_heads_pair(*ptrs[:7], 8, 8, 4, *ptrs[7:], None, None), b"itq_heads", b"null")


def test_cpu_tensors_are_refused():
    import torch
    import cmh_native as N
    f, m = torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(N.NativeError):
        N.itq_cross_moments(f, f)
    with pytest.raises(N.NativeError):
        N.itq_matmul(m, m)
    with pytest.raises(N.NativeError, match="f64"):
        N.itq_matmul(m.float(), m)
    with pytest.raises(N.NativeError):
        N.itq_inv_sqrt(m[0])
    with pytest.raises(N.NativeError):
        N.itq_cca_covariance((m[0], m), (m[0], m), m, 4)
    with pytest.raises(N.NativeError):
        N.itq_heads_pair(m, m, m, m[0], m[0], m[0, :2], m[0, :1], 8)
