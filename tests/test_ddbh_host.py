"""DDBH without a GPU: the float64 restatement of tests/ddbhutil.py against the REFERENCE's own losses and autograd gradients
(tests/golden/make_golden20.py), the registry rows, and the host-side refusals of the new entry points (nothing is launched)."""
import argparse
import ctypes as C
import sys

import numpy as np
import pytest

import ddbhutil as dd

INVALID = -1                                                                      # CMH_ERR_INVALID (include/cmh.h)


def _close(got, want, what):
    scale = max(np.abs(want).max(), 1e-30)
    assert np.abs(got - want).max() <= 1e-5 * scale, (what, np.abs(got - want).max(), scale)


@pytest.mark.parametrize("B,K,C,kind,seed", dd.CASES)
def test_restatement_reproduces_the_reference(golden, B, K, C, kind, seed):
    g = golden("ddbh.npz")
    c = dd.ddbh_case(B, K, C, kind, seed)
    tag, sc = c["tag"], dd.scalars(K)
    for mode in dd.MODES:
        assert float(g[f"{tag}_{mode}_gap"]) >= 100.0 * float(g[f"{tag}_{mode}_err"])         # the fixture's own condition
        v = c["u"] if mode == "intra" else c["v"]
        r = dd.bp_loss(c["u"], v, c["lab"], sc)
        want = float(g[f"{tag}_{mode}_loss"])
        assert abs(r["loss"] - want) <= 1e-5 * abs(want), (tag, mode, r["loss"], want)
        if mode == "intra":
            _close(r["du"] + r["dv"], g[f"{tag}_{mode}_gu"], (tag, mode, "gu"))
        else:
            _close(r["du"], g[f"{tag}_{mode}_gu"], (tag, mode, "gu"))
            _close(r["dv"], g[f"{tag}_{mode}_gv"], (tag, mode, "gv"))
    loss, gi, gt = dd.step_loss(c["u"], c["v"], c["lab"], sc)
    want = float(g[f"{tag}_step_loss"])
    assert abs(loss - want) <= 1e-5 * abs(want), (tag, "step", loss, want)
    _close(gi, g[f"{tag}_step_gi"], (tag, "step gi"))
    _close(gt, g[f"{tag}_step_gt"], (tag, "step gt"))
    if kind == "zero":
        assert all(float(g[f"{tag}_{m}_loss"]) == 0.0 for m in dd.MODES)
    if kind.startswith("mix"):
        act = dd.bp_loss(c["u"], c["v"], c["lab"], sc)["active"]
        assert act.any() and not act.all()


def test_registry_arguments_and_query_rows(monkeypatch):
    import main
    import query
    from code_rules import CODE_RULES, SOFT_RULES, sign_code, soft_output
    assert main.trainers["DDBH"].__name__ == "DDBHTrainer"
    with pytest.raises(NotImplementedError):
        main.trainers["DPSIH"]
    monkeypatch.setattr(sys, "argv", ["main.py", "--method", "DDBH", "--dataset", "synthetic", "--output-dim", "64"])
    from train.DDBH.get_args import get_args
    a = get_args(argparse.Namespace(method="DDBH", dataset="synthetic", output_dim=64, is_train=True))
    assert a.save_dir.endswith("DDBH/synthetic/64")
    query.check_method("DDBH")
    assert CODE_RULES["DDBH"] is sign_code and SOFT_RULES["DDBH"] is soft_output
    from train.DDBH.loss import BPLoss
    bp = BPLoss(64)
    assert bp.scalars() == dd.scalars(64)
    assert (bp.y_p, bp.right, bp.left, bp.lowerBound, bp.upperBound, bp.percent) == (0.5, 64 / 6, 64 / 12, 0, 16.0, 0.9)


def _operands():
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    arr = (C.c_void_p * 4)(p.value, p.value, p.value, p.value)                    # a host array of (never read) operand addresses
    return buf, p, arr


def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    """The two entry points that take a workspace, with valid shapes, non-null operands (host addresses the call never reads) and
    need - 1 bytes; the backward entry points take no workspace (they write their outputs only)."""
    import cmh_native as N
    lib = N.lib()
    buf, p, arr = _operands()
    B, K, Cn = 5, 16, 7
    need = lib.cmh_ddbh_workspace_bytes(B)
    assert need >= 4 * B * 2 * 8
    sc = dd.scalars(K)
    cases = {
        "ddbh_bp_loss": lambda n: lib.cmh_ddbh_bp_loss(arr, arr, 3, p, B, K, Cn, *sc, p, p, p, p, n, None),
        "ddbh_quant_loss": lambda n: lib.cmh_ddbh_quant_loss(arr, 2, p, B, K, Cn, p, p, p, n, None),
    }
    for name, call in cases.items():
        assert call(need - 1) == INVALID, (name, lib.cmh_last_error())
        assert name.encode() in lib.cmh_last_error() and b"workspace too small" in lib.cmh_last_error(), lib.cmh_last_error()


def test_workspace_query_and_shape_refusals():
    import cmh_native as N
    lib = N.lib()
    buf, p, arr = _operands()
    assert lib.cmh_ddbh_workspace_bytes(0) == 0 and lib.cmh_ddbh_workspace_bytes(-7) == 0
    assert lib.cmh_ddbh_workspace_bytes(4096) > lib.cmh_ddbh_workspace_bytes(128) > 0
    sc = dd.scalars(16)
    big = 1 << 20
    calls = {
        "ddbh_bp_loss": lambda B, K, Cn, a=arr: lib.cmh_ddbh_bp_loss(a, arr, 1, p, B, K, Cn, *sc, p, p, p, p, big, None),
        "ddbh_bp_loss_backward": lambda B, K, Cn, a=arr: lib.cmh_ddbh_bp_loss_backward(a, arr, 1, p, B, K, Cn, *sc, p, p, p, arr, arr, None),
        "ddbh_quant_loss": lambda B, K, Cn, a=arr: lib.cmh_ddbh_quant_loss(a, 1, p, B, K, Cn, p, p, p, big, None),
        "ddbh_quant_loss_backward": lambda B, K, Cn, a=arr: lib.cmh_ddbh_quant_loss_backward(a, 1, p, B, K, p, arr, None),
    }
    for name, call in calls.items():
        for dims in ((8193, 16, 4), (0, 16, 4), (8, 0, 4), (8, 1025, 4)) + (((8, 16, 0),) if name != "ddbh_quant_loss_backward" else ()):
            assert call(*dims) == INVALID, (name, dims)
            assert name.encode() in lib.cmh_last_error(), (name, lib.cmh_last_error())
        assert call(8193, 16, 4) == INVALID and b"8192" in lib.cmh_last_error()                 # the limit is in the message
        assert call(8, 16, 4, None) == INVALID and name.encode() in lib.cmh_last_error()        # null operand table
        holes = (C.c_void_p * 4)(None, None, None, None)
        assert call(8, 16, 4, holes) == INVALID and b"null pointer" in lib.cmh_last_error()
    assert lib.cmh_ddbh_bp_loss(arr, arr, 5, p, 8, 16, 4, *sc, p, p, p, p, big, None) == INVALID         # more calls than a launch takes
    bad = (0.5, 16 / 6, 16 / 12, 0, 4.0, 1.5)                                                            # percent beyond 1
    assert lib.cmh_ddbh_bp_loss(arr, arr, 1, p, 8, 16, 4, *bad, p, p, p, p, big, None) == INVALID and b"percent" in lib.cmh_last_error()
