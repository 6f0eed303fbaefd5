"""CPU checks around the training-free fit (LSH / PCAH / ITQ heads, csrc/itq.hip): the fixtures' robustness and the restatement's own
properties (tests/itqutil.py), the registry, query and code-rule rows, the trainer's flags, and the host-side refusals of every
cmh_itq_* entry point (nothing is launched, so no GPU is needed)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

import itqutil as U
from conftest import ROOT

NEW = ["cmh_itq_moments_workspace_bytes", "cmh_itq_moments", "cmh_itq_covariance", "cmh_itq_eigh_workspace_bytes", "cmh_itq_eigh",
       "cmh_itq_project", "cmh_itq_step_workspace_bytes", "cmh_itq_step", "cmh_itq_polar_workspace_bytes", "cmh_itq_polar",
       "cmh_itq_rotate_workspace_bytes", "cmh_itq_rotate", "cmh_itq_heads"]
_FITS = {}


def _fit(n, d, k, seed):
    if (n, d, k, seed) not in _FITS:
        _FITS[(n, d, k, seed)] = U.fit(*U.make_pair(n, d, seed), k, "pca", "itq", 50)
    return _FITS[(n, d, k, seed)]


# ---------------------------------------------------------------------------------------------------- the restatement and its fixtures
@pytest.mark.parametrize("n,d,k", [f[:3] for f in U.FIXTURES])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fixture_codes_survive_a_perturbed_covariance(n, d, k, seed):
    """The condition that lets the GPU tests ask for exact codes: the restatement rerun with C + 1e-10 max|C| (symmetric noise) gives
    the same codes for all 2N rows over 50 iterations - and PCAH's (no rotation) as well."""
    fi, ft = U.make_pair(n, d, seed)
    base = _fit(n, d, k, seed)
    for noise_seed in (11, 12):
        other = U.fit(fi, ft, k, "pca", "itq", 50, perturb=(1e-10, noise_seed))
        assert np.array_equal(base["codes"], other["codes"]), (n, d, k, seed, int((base["codes"] != other["codes"]).sum()))
    plain, plain_p = U.fit(fi, ft, k, "pca", "none"), U.fit(fi, ft, k, "pca", "none", perturb=(1e-10, 11))
    assert np.array_equal(plain["codes"], plain_p["codes"])
    z = base["Z"]
    print(f"\n(N, D, K) = ({n}, {d}, {k}), seed {seed}: min|Z| / rms(Z) = {np.abs(z).min() / np.sqrt((z ** 2).mean()):.2e}")


@pytest.mark.parametrize("n,d,k,seed", U.FIXTURES)
def test_objective_descends_and_itq_ends_below_pcah(n, d, k, seed):
    fi, ft = U.make_pair(n, d, seed)
    itq = _fit(n, d, k, seed)
    pcah = U.fit(fi, ft, k, "pca", "none")
    obj = itq["objective"]
    assert obj.shape == (51,) and pcah["objective"].shape == (1,)
    assert np.all(np.diff(obj) <= 1e-9 * obj[0]), np.diff(obj).max()
    assert obj[0] == pytest.approx(pcah["objective"][0], rel=1e-12) and obj[-1] <= pcah["objective"][0]
    r = itq["R"]
    assert np.abs(r.T @ r - np.eye(k)).max() < 1e-12
    # the heads restate the fit: sign(W f + b) is the code wherever |Z| is not at rounding level, and rms(pre-activation) = 0.5
    pre = np.concatenate([fi.astype(np.float64) @ itq["W_i"].T + itq["b_i"], ft.astype(np.float64) @ itq["W_t"].T + itq["b_t"]])
    assert np.abs(pre - itq["scale"] * itq["Z"]).max() < 1e-9
    assert np.sqrt((pre ** 2).mean()) == pytest.approx(0.5, abs=1e-9)


def test_generator_offsets_the_mean_far_beyond_the_spread():
    for n, d, k, seed in U.FIXTURES:
        for f in U.make_pair(n, d, seed):
            x = f.astype(np.float64)
            assert np.linalg.norm(x.mean(0)) > 3 * np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean())


def test_conventions_of_the_restatement():
    c = U.spd_matrix(12, 4)
    w, v = U.eigh(c)
    assert U.conventions_hold(w, v) and np.abs(c @ v - v * w).max() < 1e-13
    w2, v2 = U.order_and_sign(np.array([1.0, 2.0, 2.0]), -np.eye(3))
    assert w2.tolist() == [2.0, 2.0, 1.0] and np.array_equal(v2, np.eye(3)[:, [1, 2, 0]])
    m = np.diag([2.0, -3.0, 0.5])
    assert np.array_equal(U.polar_t(m), np.diag([1.0, -1.0, 1.0]))
    assert U.step(np.array([[0.0, -0.0, 1e-300, -1e-300]]), np.eye(4))[1].tolist() == [[1.0, 1.0, 1.0, -1.0]]     # Z >= 0, so -0 is +1
    p, q = U.random_projection(6, 3, 5), U.random_projection(6, 3, 5)
    assert np.array_equal(p, q) and not np.array_equal(p, U.random_projection(6, 3, 6))


# ---------------------------------------------------------------------------------------------------- registration
def test_registry_query_and_rule_rows():
    import main
    from code_rules import CODE_RULES, SOFT_RULES, code_rule, sign_code, soft_output, soft_rule
    import query
    assert main.trainers["ITQ"].__name__ == "ITQTrainer"
    assert main._REGISTRY["ITQ"] == ("train.ITQ.hash_train", "ITQTrainer")
    query.check_method("ITQ")
    assert query.MODELS["ITQ"] == ("model.ITQ", "MITQ")
    assert CODE_RULES["ITQ"] is sign_code and SOFT_RULES["ITQ"] is soft_output
    assert code_rule("ITQ") is sign_code and soft_rule("ITQ") is soft_output
    from model.ITQ import MITQ
    from model.modelbase import Baseclip
    assert issubclass(MITQ, Baseclip)
    import utils
    from utils.itq import fit_hash_heads
    assert utils.fit_hash_heads is fit_hash_heads


def _args(monkeypatch, *cli):
    from train.ITQ.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", *cli])
    return get_args(argparse.Namespace(method="ITQ", dataset="synthetic", output_dim=16, is_train=True))


def test_flag_defaults_and_choices(monkeypatch):
    a = _args(monkeypatch)
    assert (a.projection, a.rotation, a.itq_iters, a.fit_num) == ("pca", "itq", 50, 0)
    assert a.save_dir.endswith(os.path.join("ITQ", "synthetic", "16"))
    b = _args(monkeypatch, "--projection", "random", "--rotation", "none", "--itq-iters", "7", "--fit-num", "100")
    assert (b.projection, b.rotation, b.itq_iters, b.fit_num) == ("random", "none", 7, 100)
    for bad in (("--projection", "svd"), ("--rotation", "procrustes")):
        with pytest.raises(SystemExit):
            _args(monkeypatch, *bad)


def test_more_than_one_rank_is_refused_by_name_before_any_data(monkeypatch, tmp_path):
    import dist_utils as du
    import main
    monkeypatch.setattr(du, "world_size", lambda: 2)
    monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path / "run"), "--data-dir", str(tmp_path / "missing")])
    with pytest.raises(NotImplementedError, match="ITQ: the fit runs on one rank"):
        main.trainers["ITQ"](argparse.Namespace(method="ITQ", dataset="flickr", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


def test_fit_refuses_sizes_and_names_before_any_launch():
    import torch
    from utils.itq import fit_from_moments
    f = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="projection"):
        fit_from_moments(f, f, None, 4, projection="svd")
    with pytest.raises(ValueError, match="bits = 9"):
        fit_from_moments(f, f, None, 9)
    with pytest.raises(ValueError, match="D = 1025"):
        fit_from_moments(torch.zeros(4, 1025), torch.zeros(4, 1025), None, 4)


# ---------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_in_binding_and_header():
    import cmh_native as N
    raw = open(os.path.join(ROOT, "include", "cmh.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name             # one ctypes row per parameter
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", header) and N.ABI_VERSION == 6
    assert "No upstream counterpart" in raw
    src = open(os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "cmh_native.py")).read()
    for name in NEW:
        assert re.search(r'"%s":.*no upstream counterpart' % name, src), name


def test_workspace_queries():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_itq_moments_workspace_bytes(1, 8) >= 8 * 9 * 8
    assert lib.cmh_itq_moments_workspace_bytes(5000, 512) >= 3 * 512 * 513 * 8                     # three chunks of 2048 rows
    assert lib.cmh_itq_eigh_workspace_bytes(512, 60) >= 3 * 512 * 512 * 8 + 60 * 4
    assert lib.cmh_itq_step_workspace_bytes(5000, 64) >= 3 * (64 * 64 + 2) * 8
    assert lib.cmh_itq_polar_workspace_bytes(128) >= (2 * 128 * 128 + 128) * 8
    assert lib.cmh_itq_rotate_workspace_bytes(5000, 64) >= 5000 * 64 * 9 + 64 * 64 * 8 + lib.cmh_itq_step_workspace_bytes(5000, 64) \
        + lib.cmh_itq_polar_workspace_bytes(64)
    for q in (lib.cmh_itq_moments_workspace_bytes, lib.cmh_itq_step_workspace_bytes, lib.cmh_itq_rotate_workspace_bytes):
        for rows, size in ((0, 8), (-1, 8), (8, 0), (8, -3)):
            assert q(rows, size) == 0
    assert lib.cmh_itq_moments_workspace_bytes(8, 1025) == 0
    assert lib.cmh_itq_step_workspace_bytes(8, 129) == 0 and lib.cmh_itq_rotate_workspace_bytes(8, 129) == 0
    for k in (0, -1, 129):
        assert lib.cmh_itq_polar_workspace_bytes(k) == 0
    for d, sweeps in ((0, 30), (-2, 30), (1025, 30), (8, 0), (8, -1)):
        assert lib.cmh_itq_eigh_workspace_bytes(d, sweeps) == 0
    for q in (lib.cmh_itq_moments_workspace_bytes(300, 24), lib.cmh_itq_eigh_workspace_bytes(24, 60), lib.cmh_itq_polar_workspace_bytes(33)):
        assert q % 256 == 0


def test_host_side_refusals_before_any_launch():
    """Null pointers, D = 0 and 1025, K = 0, K > D and 129, N = 0, and a workspace one byte short: CMH_ERR_INVALID with a message that
    names the call, and nothing launched (the pointers are not addresses of anything)."""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    one, big = 1, 1 << 40
    info = (C.c_int32 * 2)(0, 0)

    def refused(rc, *words):
        msg = lib.cmh_last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    # moments
    for n, d in ((0, 8), (8, 0), (8, 1025)):
        refused(lib.cmh_itq_moments(one, n, d, one, one, 0, one, big, None), b"itq_moments", b"need")
    for args in ((None, 8, 8, one, one), (one, 8, 8, None, one), (one, 8, 8, one, None)):
        refused(lib.cmh_itq_moments(*args, 0, one, big, None), b"itq_moments", b"null")
    refused(lib.cmh_itq_moments(one, 8, 8, one, one, 0, None, big, None), b"null")
    refused(lib.cmh_itq_moments(one, 300, 24, one, one, 0, one, lib.cmh_itq_moments_workspace_bytes(300, 24) - 1, None), b"itq_moments", b"workspace")
    # covariance
    for n, d in ((0, 8), (8, 0), (8, 1025)):
        refused(lib.cmh_itq_covariance(one, one, one, one, n, d, one, one, one, one, None), b"itq_covariance", b"need")
    for hole in range(8):
        ptrs = [one] * 8
        ptrs[hole] = None
        refused(lib.cmh_itq_covariance(*ptrs[:4], 8, 8, *ptrs[4:], None), b"itq_covariance", b"null")
    # eigh
    for d, sweeps in ((0, 30), (1025, 30), (8, 0), (8, 1025)):
        refused(lib.cmh_itq_eigh(one, d, sweeps, one, one, info, one, big, None), b"itq_eigh", b"need")
    refused(lib.cmh_itq_eigh(None, 8, 30, one, one, info, one, big, None), b"null")
    refused(lib.cmh_itq_eigh(one, 8, 30, None, one, info, one, big, None), b"null")
    refused(lib.cmh_itq_eigh(one, 8, 30, one, None, info, one, big, None), b"null")
    refused(lib.cmh_itq_eigh(one, 8, 30, one, one, None, one, big, None), b"null")
    refused(lib.cmh_itq_eigh(one, 8, 30, one, one, info, None, big, None), b"null")
    refused(lib.cmh_itq_eigh(one, 24, 60, one, one, info, one, lib.cmh_itq_eigh_workspace_bytes(24, 60) - 1, None), b"itq_eigh", b"workspace")
    # project
    for n, d, k in ((0, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 9), (8, 512, 129)):
        refused(lib.cmh_itq_project(one, n, d, k, one, one, one, one, None), b"itq_project", b"need")
    for hole in range(5):
        ptrs = [one] * 5
        ptrs[hole] = None
        refused(lib.cmh_itq_project(ptrs[0], 8, 8, 4, *ptrs[1:], None), b"itq_project", b"null")
    # step
    for rows, k in ((0, 8), (8, 0), (8, 129)):
        refused(lib.cmh_itq_step(one, rows, k, one, one, one, one, one, one, big, None), b"itq_step", b"need")
    for hole in range(6):
        ptrs = [one] * 6
        ptrs[hole] = None
        refused(lib.cmh_itq_step(ptrs[0], 8, 8, *ptrs[1:], one, big, None), b"itq_step", b"null")
    refused(lib.cmh_itq_step(one, 8, 8, one, one, one, one, one, None, big, None), b"null")
    refused(lib.cmh_itq_step(one, 600, 16, one, one, one, one, one, one, lib.cmh_itq_step_workspace_bytes(600, 16) - 1, None), b"itq_step", b"workspace")
    # polar
    for k in (0, 129):
        refused(lib.cmh_itq_polar(one, k, one, None, one, big, None), b"itq_polar", b"need")
    refused(lib.cmh_itq_polar(None, 8, one, None, one, big, None), b"null")
    refused(lib.cmh_itq_polar(one, 8, None, None, one, big, None), b"null")
    refused(lib.cmh_itq_polar(one, 8, one, None, None, big, None), b"null")
    refused(lib.cmh_itq_polar(one, 33, one, None, one, lib.cmh_itq_polar_workspace_bytes(33) - 1, None), b"itq_polar", b"workspace")
    # rotate
    for rows, k, iters in ((0, 8, 5), (8, 0, 5), (8, 129, 5), (8, 8, -1)):
        refused(lib.cmh_itq_rotate(one, rows, k, one, iters, one, one, one, one, big, None), b"itq_rotate", b"need")
    for hole in range(5):
        ptrs = [one] * 5
        ptrs[hole] = None
        refused(lib.cmh_itq_rotate(ptrs[0], 8, 8, ptrs[1], 5, *ptrs[2:], one, big, None), b"itq_rotate", b"null")
    refused(lib.cmh_itq_rotate(one, 8, 8, one, 5, one, one, one, None, big, None), b"null")
    refused(lib.cmh_itq_rotate(one, 600, 16, one, 5, one, one, one, one, lib.cmh_itq_rotate_workspace_bytes(600, 16) - 1, None), b"itq_rotate", b"workspace")
    # heads
    for rows, d, k in ((0, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 9), (8, 512, 129)):
        refused(lib.cmh_itq_heads(*([one] * 6), rows, d, k, one, one, one, one, None, None), b"itq_heads", b"need")
    for hole in range(10):
        ptrs = [one] * 10
        ptrs[hole] = None
        refused(lib.cmh_itq_heads(*ptrs[:6], 8, 8, 4, *ptrs[6:], None, None), b"itq_heads", b"null")


def test_cpu_tensors_are_refused():
    import torch
    import cmh_native as N
    with pytest.raises(N.NativeError):
        N.itq_moments(torch.zeros(4, 8))
    with pytest.raises(N.NativeError):
        N.itq_polar(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(N.NativeError, match="f64"):
        N.itq_polar(torch.zeros(4, 4))
