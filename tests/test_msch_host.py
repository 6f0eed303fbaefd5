"""MSCH without a GPU: the float64 restatement of tests/mschutil.py against the REFERENCE's own losses, counts and autograd gradients
(tests/golden/make_golden21.py) and against torch autograd in float64, the registry rows and flags, the header, and the host-side
refusals of the new entry points (nothing is launched)."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import mschutil as ms
from conftest import ROOT

INVALID = -1                                                                      # CMH_ERR_INVALID (include/cmh.h)
SHORT = {"all": "all", "semi-hard": "semi"}


def _close(got, want, what, tol=1e-6):
    scale = max(np.abs(want).max(), 1e-30)
    assert np.abs(got - want).max() <= tol * scale, (what, np.abs(got - want).max(), scale)


@pytest.mark.parametrize("B,K,C,seed,norms", ms.CASES)
def test_restatement_reproduces_the_reference(golden, B, K, C, seed, norms):
    g = golden("msch.npz")
    c = ms.msch_case(B, K, C, seed)
    tag = c["tag"]
    for rule in ms.RULES:
        for mode in ms.MODES:
            for nz in norms:
                key = f"{tag}_{SHORT[rule]}_{mode}_n{int(nz)}"
                assert float(g[f"{key}_gap"]) >= 100.0 * float(g[f"{key}_err"])               # the fixture's own condition
                r = ms.msc_loss(c["u"], c["u"] if mode == "intra" else c["v"], c["lab"], ms.MARGIN, rule, nz)
                want = float(g[f"{key}_loss"])
                assert r["count"] == int(g[f"{key}_count"]), (key, r["count"], int(g[f"{key}_count"]))
                assert abs(r["loss"] - want) <= 1e-6 * max(1.0, abs(want)), (key, r["loss"], want)
                if mode == "intra":
                    _close(r["du"] + r["dv"], g[f"{key}_gu"], (key, "gu"))
                else:
                    _close(r["du"], g[f"{key}_gu"], (key, "gu"))
                    _close(r["dv"], g[f"{key}_gv"], (key, "gv"))
    loss, gi, gt = ms.step_loss(c["u"], c["v"], c["lab"])
    want = float(g[f"{tag}_step_loss"])
    assert abs(loss - want) <= 1e-6 * abs(want), (tag, "step", loss, want)
    _close(gi, g[f"{tag}_step_gi"], (tag, "step gi"))
    _close(gt, g[f"{tag}_step_gt"], (tag, "step gt"))
    assert int(g[f"{tag}_semi_cross_n0_count"]) < int(g[f"{tag}_all_cross_n0_count"])         # the two rules differ on every case


def _torch_loss(u, v, y, margin, rule, normalize):
    """the definition as float64 torch ops over the [B, B, B] mask (small B only)"""
    a, b = (torch.nn.functional.normalize(x, p=2, dim=1) for x in (u, v)) if normalize else (u, v)
    s = -(a @ b.t())
    sim = (y @ y.t()) > 0
    same, diff = sim & ~torch.eye(len(y), dtype=torch.bool), ~sim
    tm = s[:, None, :] - s[:, :, None]                                            # [a, p, n]
    act = same[:, :, None] & diff[:, None, :] & (tm <= margin)
    if rule == "semi-hard":
        act &= tm > 0
    return torch.relu(-tm + margin)[act].mean(), int(act.sum())


@pytest.mark.parametrize("rule", ms.RULES)
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_gradient_is_autograds_in_float64(rule, normalize):
    c = ms.msch_case(33, 16, 5, 94)
    y = torch.from_numpy(c["lab"]).double()
    for mode in ms.MODES:
        u = torch.from_numpy(c["u"]).double().requires_grad_()
        v = u if mode == "intra" else torch.from_numpy(c["v"]).double().requires_grad_()
        loss, count = _torch_loss(u, v, y, ms.MARGIN, rule, normalize)
        loss.backward()
        r = ms.msc_loss(c["u"], c["u"] if mode == "intra" else c["v"], c["lab"], ms.MARGIN, rule, normalize)
        assert r["count"] == count and abs(r["loss"] - float(loss.detach())) <= 1e-12
        if mode == "intra":
            _close(r["du"] + r["dv"], u.grad.numpy(), (rule, mode), 1e-12)
        else:
            _close(r["du"], u.grad.numpy(), (rule, mode, "u"), 1e-12)
            _close(r["dv"], v.grad.numpy(), (rule, mode, "v"), 1e-12)


def test_restatement_decides_on_given_similarities_in_their_arithmetic():
    """s= a float32 matrix: the differences are float32 differences, as the reference forms them; ties at m and at 0 are exact"""
    c = ms.tie_case()
    s32 = (-(c["u"] @ c["v"].T)).astype(np.float32)
    a = ms.msc_loss(c["u"], c["v"], c["lab"], c["margin"], "all", s=s32)
    h = ms.msc_loss(c["u"], c["v"], c["lab"], c["margin"], "semi-hard", s=s32)
    assert a["gap"] == 0.0 and h["gap"] == 0.0
    assert a["count"] > h["count"] > 0
    assert np.array_equal(a["coef"], ms.msc_loss(c["u"], c["v"], c["lab"], c["margin"], "all")["coef"])        # integers either way


def test_registry_flags_and_query_rows(monkeypatch):
    import main
    import query
    from code_rules import CODE_RULES, SOFT_RULES, sign_code, soft_output
    assert main.trainers["MSCH"].__name__ == "MSCHTrainer"
    with pytest.raises(NotImplementedError):
        main.trainers["DPSIH"]
    assert set(CODE_RULES) == set(SOFT_RULES) == set(query.MODELS) and "MSCH" in CODE_RULES
    assert CODE_RULES["MSCH"] is sign_code and SOFT_RULES["MSCH"] is soft_output and query.MODELS["MSCH"] == ("model.MSCH", "MMSCH")
    query.check_method("MSCH")
    from train.MSCH.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", "--method", "MSCH", "--dataset", "synthetic", "--output-dim", "64"])
    a = get_args(argparse.Namespace(method="MSCH", dataset="synthetic", output_dim=64, is_train=True))
    assert a.save_dir.endswith("MSCH/synthetic/64")
    assert (a.msc_margin, a.msc_scale, a.msc_mining, a.msc_symmetric) == (0.25, 100.0, "all", False)
    monkeypatch.setattr(sys, "argv", ["main.py", "--msc-margin", "0.5", "--msc-scale", "10", "--msc-mining", "semi-hard", "--msc-symmetric", "true"])
    a = get_args(argparse.Namespace(method="MSCH", dataset="synthetic", output_dim=64, is_train=True))
    assert (a.msc_margin, a.msc_scale, a.msc_mining, a.msc_symmetric) == (0.5, 10.0, "semi-hard", True)
    monkeypatch.setattr(sys, "argv", ["main.py", "--msc-mining", "hard"])
    with pytest.raises(SystemExit):
        get_args(argparse.Namespace(method="MSCH", dataset="synthetic", output_dim=64, is_train=True))
    from train.MSCH.loss import MSCLoss
    m = MSCLoss()
    assert (m.margin, m.mining, m.normalize) == (0.25, "all", False)
    with pytest.raises(ValueError):
        MSCLoss(mining="hard")


def test_header_declares_the_entry_points():
    import cmh_native as N
    src = open(os.path.join(ROOT, "include", "cmh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("cmh_msc_triplet_workspace_bytes", "cmh_msc_triplet_loss", "cmh_msc_triplet_loss_backward"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in N.SIGNATURES
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", src) and N.ABI_VERSION == 6
    assert "train/DPSIH/Loss.py:78-137" in src


def _operands():
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    arr = (C.c_void_p * 4)(p.value, p.value, p.value, p.value)                    # a host array of (never read) operand addresses
    return buf, p, arr


def test_workspace_query_and_refusals_without_a_launch():
    import cmh_native as N
    lib = N.lib()
    buf, p, arr = _operands()
    ws = lib.cmh_msc_triplet_workspace_bytes
    assert ws(0) == 0 and ws(-3) == 0 and ws(1025) == 0
    assert ws(1024) > ws(128) > ws(1) > 0
    big = 1 << 20
    fwd = lambda B=8, K=16, Cn=4, mining=0, a=arr, lab=p, n=big, calls=1, nz=0, unit=None: lib.cmh_msc_triplet_loss(
        a, arr, calls, lab, B, K, Cn, 0.25, mining, nz, p, p, p, p, unit, unit, p, n, None)
    bwd = lambda B=8, K=16, a=arr, coef=p, calls=1, nz=0, unit=None: lib.cmh_msc_triplet_loss_backward(
        a, arr, calls, B, K, nz, coef, p, unit, unit, p, arr, arr, None)
    for name, call in (("msc_triplet_loss", fwd), ("msc_triplet_loss_backward", bwd)):
        for kw, word in ((dict(B=1025), b"1024"), (dict(B=0), b"B=0"), (dict(K=129), b"128"), (dict(K=0), b"K=0"), (dict(calls=5), b"calls=5"),
                         (dict(a=None), b"null pointer"), (dict(a=(C.c_void_p * 4)(None, None, None, None)), b"null pointer"),
                         (dict(nz=1), b"null pointer")):
            assert call(**kw) == INVALID, (name, kw)
            msg = lib.cmh_last_error()
            assert msg.startswith(name.encode() + b":") and word in msg, (name, kw, msg)
    assert fwd(lab=None) == INVALID and b"null pointer" in lib.cmh_last_error()
    assert bwd(coef=None) == INVALID and b"null pointer" in lib.cmh_last_error()
    assert fwd(Cn=0) == INVALID and b"C=0" in lib.cmh_last_error()
    assert fwd(mining=2) == INVALID and b"mining=2" in lib.cmh_last_error()
    assert fwd(mining=-1) == INVALID
    need = ws(8)
    assert fwd(n=need - 1) == INVALID and b"msc_triplet_loss: workspace too small" in lib.cmh_last_error()
    holes = (C.c_void_p * 4)(None, None, None, None)                              # gradient buffers missing
    assert lib.cmh_msc_triplet_loss_backward(arr, arr, 1, 8, 16, 0, p, p, None, None, p, holes, holes, None) == INVALID
    assert b"null gradient pointer" in lib.cmh_last_error()


def test_cpu_tensors_are_refused():
    import cmh_native as N
    with pytest.raises(N.NativeError):
        N.msc_triplet_loss([(torch.zeros(4, 8), torch.zeros(4, 8))], torch.zeros(4, 2), 0.25)
    with pytest.raises(N.NativeError, match="mining"):
        N.msc_triplet_loss([(torch.zeros(4, 8), torch.zeros(4, 8))], torch.zeros(4, 2), 0.25, mining="hard")
