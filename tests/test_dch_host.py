"""CPU checks around the supervised training-free fit (DCH heads, csrc/dch.hip): the restatement's own properties and the fixtures'
robustness (tests/dchutil.py), its retrieval quality against the label-free ITQ fit, the registry, query and code-rule rows, the
trainer's flags, and the host-side refusals of every cmh_dch_* entry point (nothing is launched, so no GPU is needed)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

import dchutil as U
import itqutil as IU
from conftest import ROOT

NEW = ["cmh_dch_covariance", "cmh_dch_start", "cmh_dch_xtb_workspace_bytes", "cmh_dch_xtb", "cmh_dch_btb_workspace_bytes", "cmh_dch_btb",
       "cmh_dch_center", "cmh_dch_solve", "cmh_dch_targets_workspace_bytes", "cmh_dch_targets", "cmh_dch_dcc_workspace_bytes", "cmh_dch_dcc"]
MUS = [1.0, 0.1, 0.01]
# The f32 heads against the f64 fit, |z_head - s z_fit|: tests/test_gpu_dch.py measures it on the GPU (worst 4.05e-6) and keeps 10 x
# that as TAU; entries under it are left out of the head-code comparison, and at most HEAD_CAP of the entries may be.
TAU = 10 * 4.05e-6
HEAD_CAP = 1e-3
_FITS = {}


def _fit(fix, mu):
    if (fix, mu) not in _FITS:
        _FITS[(fix, mu)] = U.fit(*U.fixture(fix)[0], fix[3], iters=5, rounds=3, mu=mu)
    return _FITS[(fix, mu)]


# ---------------------------------------------------------------------------------------------------- the restatement and its fixtures
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("fix", U.FIXTURES)
def test_objective_never_rises(fix, mu):
    """Each iteration re-fits W and P_m to the B it starts from and the coordinate descent lowers the same expression bit by bit.
    The allowance is the rounding of the objective's own sum (N (C + 2 K) terms), not a tolerance on the descent."""
    r = _fit(fix, mu)
    obj = r["objective"]
    n, _, c, k, _ = fix
    assert obj.shape == (6,) and r["flips"].shape == (5, 3) and r["min_margin"].shape == (5,)
    assert np.all(np.diff(obj) <= 8 * n * (c + 2 * k) * U.EPS * obj[0]), np.diff(obj).max()
    assert obj[-1] < obj[0]
    assert r["flips"].min() >= 0 and r["flips"][0].sum() > 0
    print(f"\n{fix}, mu {mu}: objective {obj[0]:.6g} -> {obj[-1]:.6g}, flips per iteration {r['flips'].sum(1).tolist()}")


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("fix", U.FIXTURES)
def test_fixture_decisions_stand_clear_of_zero(fix, mu):
    """What lets the GPU tests ask for exact codes: every decision of the coordinate descent and every entry of the start stands
    1e-9 or more from zero, seven orders above f64 rounding of sums of this size."""
    r = _fit(fix, mu)
    print(f"\n{fix}, mu {mu}: smallest |t| {r['min_margin'].min():.2e}, smallest start entry {r['min_start']:.2e}")
    assert r["min_margin"].min() >= U.MARGIN_FLOOR and r["min_start"] >= U.MARGIN_FLOOR


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_labels_lift_held_out_map_over_itq(fix):
    """mu = 0.01, 5 iterations: the held-out queries' mAP over the whole database, both directions, against tests/itqutil.py's
    pca + itq fit of the same rows.  Both sides are deterministic CPU restatements; the gap asked for, 0.1, is under half of
    the measured one (0.21 to 0.25)."""
    fit_set, queries = U.fixture(fix)
    dch = U.held_out_map(_fit(fix, 0.01), fit_set, queries)
    itq = U.held_out_map(IU.fit(fit_set[0], fit_set[1], fix[3], "pca", "itq", 50), fit_set, queries)
    print(f"\n{fix}: mAP i->t / t->i  DCH {dch[0]:.4f} / {dch[1]:.4f}, ITQ {itq[0]:.4f} / {itq[1]:.4f}")
    assert dch[0] >= itq[0] + 0.1 and dch[1] >= itq[1] + 0.1


@pytest.mark.parametrize("fix", U.FIXTURES)
def test_heads_restate_the_fit_and_few_entries_lie_under_tau(fix):
    fit_set, _ = U.fixture(fix)
    r = _fit(fix, 0.01)
    pre = np.concatenate([fit_set[0].astype(np.float64) @ r["W_i"].T + r["b_i"], fit_set[1].astype(np.float64) @ r["W_t"].T + r["b_t"]])
    assert np.abs(pre - r["scale"] * r["Z"]).max() < 1e-9
    assert np.sqrt((pre ** 2).mean()) == pytest.approx(0.5, abs=1e-9)
    under = float((np.abs(r["scale"] * r["Z"]) <= TAU).mean())
    print(f"\n{fix}: share of |s z| <= tau = {TAU:.1e}: {under:.2e}; head codes equal to B: {(r['codes'] == np.concatenate([r['B'], r['B']])).mean():.4f}")
    assert under <= HEAD_CAP


def test_conventions_of_the_restatement():
    # t == 0 keeps the bit, whatever it is; t > 0 sets +1, t < 0 sets -1
    g = np.array([[1.0, 1.0], [1.0, 1.0]])
    q = np.array([[1.0, 0.0], [-1.0, 0.0], [3.0, -5.0]])
    b, flips, least = U.dcc(q, g, np.array([[1.0, 1.0], [-1.0, -1.0], [-1.0, 1.0]]), 1)
    #  row 0: t_0 = 1 - 1 = 0 keeps +1; t_1 = 0 - 1 < 0 -> -1.   row 1: t_0 = -1 + 1 = 0 keeps -1; t_1 = 0 + 1 > 0 -> +1
    #  row 2: t_0 = 3 - 1 > 0 -> +1; t_1 = -5 - 1 < 0 -> -1
    assert b.tolist() == [[1.0, -1.0], [-1.0, 1.0], [1.0, -1.0]] and flips.tolist() == [4] and least == 0.0
    y = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    bb = np.array([[1.0], [-1.0], [1.0]])
    w = U.label_regression(bb, y, 1.0)
    assert np.allclose(w, (bb.T @ y) / 4.0)
    z = np.zeros((3, 1))
    assert U.objective(y, bb, w, z, z, 1.0, 0.5) == pytest.approx(((y - bb @ w) ** 2).sum() + (w ** 2).sum() + 0.5 * 6)
    assert np.array_equal(U.targets(y, w, bb, 2 * bb, 0.5), y @ w.T + 1.5 * bb)
    # the generator: multi-hot labels without an empty row, an offset far beyond the spread
    xi, xt, lab = U.make_labelled(500, 24, 5, 1)
    assert lab.sum(1).min() >= 1 and set(np.unique(lab).tolist()) == {0.0, 1.0} and xi.dtype == np.float32
    for f in (xi, xt):
        x = f.astype(np.float64)
        assert np.linalg.norm(x.mean(0)) > 3 * np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean())
    # the score: a perfect ranking scores 1, and ties go in database order
    codes = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]])
    labels = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
    assert U.mean_average_precision(codes[:1], labels[:1], codes, labels) == pytest.approx((1 + 2 / 3) / 2)


# ---------------------------------------------------------------------------------------------------- registration
def test_registry_query_and_rule_rows():
    import main
    from code_rules import CODE_RULES, SOFT_RULES, code_rule, sign_code, soft_output, soft_rule
    import query
    assert main.trainers["DCH"].__name__ == "DCHTrainer"
    assert main._REGISTRY["DCH"] == ("train.DCH.hash_train", "DCHTrainer")
    query.check_method("DCH")
    assert query.MODELS["DCH"] == ("model.DCH", "MDCH")
    assert CODE_RULES["DCH"] is sign_code and SOFT_RULES["DCH"] is soft_output
    assert code_rule("DCH") is sign_code and soft_rule("DCH") is soft_output
    assert set(CODE_RULES) == set(SOFT_RULES) == set(query.MODELS)
    from model.DCH import MDCH
    from model.modelbase import Baseclip
    assert issubclass(MDCH, Baseclip)
    import utils
    from utils.dch import fit_supervised_heads
    assert utils.fit_supervised_heads is fit_supervised_heads
    from utils.itq import PROJECTIONS
    assert PROJECTIONS == ("pca", "random", "cca")                         # the unsupervised fit's choices are as they were


def _args(monkeypatch, *cli):
    from train.DCH.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", *cli])
    return get_args(argparse.Namespace(method="DCH", dataset="synthetic", output_dim=16, is_train=True))


def test_flag_defaults_match_the_fits(monkeypatch):
    from utils import dch
    a = _args(monkeypatch)
    assert (a.dch_iters, a.dch_rounds, a.dch_lambda, a.dch_mu, a.dch_reg, a.fit_num) == (10, 3, 1.0, 0.01, 0.1, 0)
    assert (a.dch_iters, a.dch_rounds, a.dch_lambda, a.dch_mu, a.dch_reg) == (dch.DCH_ITERS, dch.DCH_ROUNDS, dch.DCH_LAMBDA, dch.DCH_MU, dch.DCH_REG)
    assert a.save_dir.endswith(os.path.join("DCH", "synthetic", "16"))
    b = _args(monkeypatch, "--dch-iters", "4", "--dch-rounds", "2", "--dch-lambda", "0.5", "--dch-mu", "0.1", "--dch-reg", "0.2", "--fit-num", "100")
    assert (b.dch_iters, b.dch_rounds, b.dch_lambda, b.dch_mu, b.dch_reg, b.fit_num) == (4, 2, 0.5, 0.1, 0.2, 100)
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--dch-iters", "many")


def test_more_than_one_rank_is_refused_by_name_before_any_data(monkeypatch, tmp_path):
    import dist_utils as du
    import main
    monkeypatch.setattr(du, "world_size", lambda: 2)
    monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path / "run"), "--data-dir", str(tmp_path / "missing")])
    with pytest.raises(NotImplementedError, match="DCH: the fit runs on one rank"):
        main.trainers["DCH"](argparse.Namespace(method="DCH", dataset="flickr", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


def test_trainer_refuses_bad_parameters_by_name(monkeypatch, tmp_path):
    import main
    for bad in (("--dch-rounds", "0"), ("--dch-lambda", "0"), ("--dch-mu", "-1"), ("--dch-reg", "0"), ("--dch-iters", "-1")):
        monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path / "run"), *bad])
        with pytest.raises(ValueError, match="DCH: --dch-"):
            main.trainers["DCH"](argparse.Namespace(method="DCH", dataset="synthetic", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


def test_fit_refuses_sizes_and_parameters_before_any_launch():
    import torch
    from utils.dch import fit_from_moments
    f, y = torch.zeros(4, 8), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="bits = 9"):
        fit_from_moments(f, f, y, None, 9)
    with pytest.raises(ValueError, match="D = 1025"):
        fit_from_moments(torch.zeros(4, 1025), torch.zeros(4, 1025), y, None, 4)
    with pytest.raises(ValueError, match="labels"):
        fit_from_moments(f, f, torch.zeros(5, 3), None, 4)
    with pytest.raises(ValueError, match="C = 1025"):
        fit_from_moments(f, f, torch.zeros(4, 1025), None, 4)
    with pytest.raises(ValueError, match="paired"):
        fit_from_moments(f, torch.zeros(4, 9), y, None, 4)
    for kw in ({"rounds": 0}, {"rounds": 65}, {"iters": -1}, {"lam": 0.0}, {"mu": -0.1}, {"reg": 0.0}):
        with pytest.raises(ValueError, match="need"):
            fit_from_moments(f, f, y, None, 4, **kw)


# ---------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_in_binding_and_header():
    import cmh_native as N
    raw = open(os.path.join(ROOT, "include", "cmh.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(cmh_dch_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW)
    for name in NEW:
        assert name in N.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name             # one ctypes row per parameter
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", header) and N.ABI_VERSION == 6
    assert N.lib().cmh_version() == 6                                                    # entry points were added, nothing else changed
    src = open(os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "cmh_native.py")).read()
    for name in NEW:
        assert re.search(r'"%s":.*no upstream counterpart' % name, src), name


def test_workspace_queries():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_dch_xtb_workspace_bytes(1, 8, 4) >= 9 * 4 * 8
    assert lib.cmh_dch_xtb_workspace_bytes(5000, 512, 64) >= 3 * 513 * 64 * 8                       # three chunks of 2048 rows
    assert lib.cmh_dch_btb_workspace_bytes(5000, 64) >= 3 * 64 * 64 * 8
    assert lib.cmh_dch_targets_workspace_bytes(5000) >= (2 * 79 + 20) * 8                           # 79 blocks of 64 items, 20 of 256
    assert lib.cmh_dch_dcc_workspace_bytes(5000, 3) >= 20 * (3 + 1) * 8
    for q in (lib.cmh_dch_xtb_workspace_bytes(300, 24, 8), lib.cmh_dch_btb_workspace_bytes(300, 8), lib.cmh_dch_targets_workspace_bytes(300),
              lib.cmh_dch_dcc_workspace_bytes(300, 3)):
        assert q > 0 and q % 256 == 0
    too_many = 65535 * 2048 + 1
    for n, dx, k in ((0, 8, 4), (-1, 8, 4), (too_many, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 129)):
        assert lib.cmh_dch_xtb_workspace_bytes(n, dx, k) == 0
    for n, k in ((0, 8), (too_many, 8), (8, 0), (8, 129), (8, -1)):
        assert lib.cmh_dch_btb_workspace_bytes(n, k) == 0
    for n in (0, -5, too_many):
        assert lib.cmh_dch_targets_workspace_bytes(n) == 0
    for n, rounds in ((0, 3), (too_many, 3), (8, 0), (8, 65), (8, -1)):
        assert lib.cmh_dch_dcc_workspace_bytes(n, rounds) == 0


def test_host_side_refusals_before_any_launch():
    """Null pointers, sizes out of range and a workspace one byte short: CMH_ERR_INVALID with a message that names the call, and
    nothing launched (the operands are host addresses the call never reads)."""
    import cmh_native as N
    lib = N.lib()
    one, big, too_many = 1, 1 << 40, 65535 * 2048 + 1

    def refused(rc, *words):
        msg = lib.cmh_last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def holes(count):
        for hole in range(count):
            ptrs = [one] * count
            ptrs[hole] = None
            yield ptrs

    # covariance
    for n, d in ((0, 8), (8, 0), (8, 1025)):
        refused(lib.cmh_dch_covariance(one, one, one, n, d, one, None), b"dch_covariance", b"need")
    for p in holes(4):
        refused(lib.cmh_dch_covariance(*p[:3], 8, 8, p[3], None), b"dch_covariance", b"null")
    # start
    for n, k in ((0, 8), (too_many, 8), (8, 0), (8, 129)):
        refused(lib.cmh_dch_start(one, one, n, k, one, None), b"dch_start", b"need")
    for p in holes(3):
        refused(lib.cmh_dch_start(p[0], p[1], 8, 8, p[2], None), b"dch_start", b"null")
    # xtb
    for n, dx, k in ((0, 8, 4), (too_many, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 129)):
        refused(lib.cmh_dch_xtb(one, one, n, dx, k, one, one, 0, one, big, None), b"dch_xtb", b"need")
    for p in holes(3):
        refused(lib.cmh_dch_xtb(p[0], p[1], 8, 8, 4, p[2], None, 0, one, big, None), b"dch_xtb", b"null")
    refused(lib.cmh_dch_xtb(one, one, 8, 8, 4, one, one, 0, None, big, None), b"dch_xtb", b"null")
    refused(lib.cmh_dch_xtb(one, one, 300, 24, 8, one, one, 0, one, lib.cmh_dch_xtb_workspace_bytes(300, 24, 8) - 1, None), b"dch_xtb", b"workspace")
    # btb
    for n, k in ((0, 8), (too_many, 8), (8, 0), (8, 129)):
        refused(lib.cmh_dch_btb(one, n, k, one, one, big, None), b"dch_btb", b"need")
    refused(lib.cmh_dch_btb(None, 8, 8, one, one, big, None), b"dch_btb", b"null")
    refused(lib.cmh_dch_btb(one, 8, 8, None, one, big, None), b"dch_btb", b"null")
    refused(lib.cmh_dch_btb(one, 8, 8, one, None, big, None), b"dch_btb", b"null")
    refused(lib.cmh_dch_btb(one, 300, 8, one, one, lib.cmh_dch_btb_workspace_bytes(300, 8) - 1, None), b"dch_btb", b"workspace")
    # center
    for n, d, k in ((0, 8, 4), (8, 0, 4), (8, 1025, 4), (8, 8, 0), (8, 8, 9), (8, 512, 129)):
        refused(lib.cmh_dch_center(one, one, one, one, n, d, k, one, None), b"dch_center", b"need")
    for p in holes(5):
        refused(lib.cmh_dch_center(*p[:4], 8, 8, 4, p[4], None), b"dch_center", b"null")
    # solve
    for k, c in ((0, 4), (129, 4), (8, 0), (8, 1025)):
        refused(lib.cmh_dch_solve(one, 1.0, one, k, c, 2, one, None), b"dch_solve", b"need")
    for shift in (-1.0, float("nan")):
        refused(lib.cmh_dch_solve(one, shift, one, 8, 4, 2, one, None), b"dch_solve", b"shift")
    for a, r, w, info in ((None, one, 2, one), (one, None, 2, one), (one, one, None, one), (one, one, 2, None)):
        refused(lib.cmh_dch_solve(a, 1.0, r, 8, 4, w, info, None), b"dch_solve", b"null")
    refused(lib.cmh_dch_solve(one, 1.0, one, 8, 4, one, one, None), b"dch_solve", b"operand")
    # targets
    for n, k, c in ((0, 8, 4), (too_many, 8, 4), (8, 0, 4), (8, 129, 4), (8, 8, 0), (8, 8, 1025)):
        refused(lib.cmh_dch_targets(one, one, one, one, one, 0.01, 1.0, n, k, c, one, one, one, big, None), b"dch_targets", b"need")
    for p in holes(6):
        refused(lib.cmh_dch_targets(*p[:5], 0.01, 1.0, 8, 8, 4, one, p[5], one, big, None), b"dch_targets", b"null")
    refused(lib.cmh_dch_targets(one, one, one, one, one, 0.01, 1.0, 8, 8, 4, one, one, None, big, None), b"dch_targets", b"null")
    refused(lib.cmh_dch_targets(one, one, one, one, one, 0.01, 1.0, 300, 8, 4, one, one, one, lib.cmh_dch_targets_workspace_bytes(300) - 1, None),
            b"dch_targets", b"workspace")
    # dcc
    for n, k, rounds in ((0, 8, 3), (too_many, 8, 3), (8, 0, 3), (8, 129, 3), (8, 8, 0), (8, 8, 65)):
        refused(lib.cmh_dch_dcc(one, one, one, n, k, rounds, one, one, one, big, None), b"dch_dcc", b"need")
    for p in holes(5):
        refused(lib.cmh_dch_dcc(*p[:3], 8, 8, 3, p[3], p[4], one, big, None), b"dch_dcc", b"null")
    refused(lib.cmh_dch_dcc(one, one, one, 8, 8, 3, one, one, None, big, None), b"dch_dcc", b"null")
    refused(lib.cmh_dch_dcc(one, one, one, 300, 8, 3, one, one, one, lib.cmh_dch_dcc_workspace_bytes(300, 3) - 1, None), b"dch_dcc", b"workspace")


def test_cpu_tensors_and_wrong_types_are_refused():
    import torch
    import cmh_native as N
    b = torch.ones(4, 8, dtype=torch.int8)
    with pytest.raises(N.NativeError):
        N.dch_btb(b)
    with pytest.raises(N.NativeError, match="int8"):
        N.dch_btb(torch.ones(4, 8))
    with pytest.raises(N.NativeError):
        N.dch_xtb(torch.zeros(4, 8), b)
    with pytest.raises(N.NativeError, match="f64"):
        N.dch_solve(torch.zeros(4, 4), torch.zeros(4, 2))
    with pytest.raises(N.NativeError):
        N.dch_solve(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64))
