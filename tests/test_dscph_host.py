"""DScPH without a GPU: the float64 restatement of tests/dscphutil.py against the REFERENCE's own CPF loss, quantisation terms (through
its HouseHolder rotation) and autograd gradients (tests/golden/make_golden22.py) and against torch autograd in float64, the registry
rows and flags, the header, and the host-side refusals of the new entry points (nothing is launched)."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dscphutil as ds
from conftest import ROOT

INVALID = -1                                                                      # CMH_ERR_INVALID (include/cmh.h)
TAGS = [f"B{B}_K{K}_C{Cn}" for B, K, Cn, _ in ds.CASES] + list(ds.SPECIALS)


def _close(got, want, what, tol=1e-5):
    scale = max(np.abs(want).max(), 1e-30)
    assert np.abs(got - want).max() <= tol * scale, (what, np.abs(got - want).max(), scale)


def _case(tag):
    return {c["tag"]: c for c in ds.all_cases()}[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(golden, tag):
    g = golden("dscph.npz")
    c = _case(tag)
    assert float(g[f"{tag}_gap"]) >= 100.0 * float(g[f"{tag}_err"])                           # the fixture's own condition
    assert float(g[f"{tag}_rot_dev"]) == 0.0                                                  # the identity HouseHolder is X -> -X exactly
    r = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"])
    assert abs(r["gap"] - float(g[f"{tag}_gap"])) <= 1e-12
    assert abs(r["cpf"] - float(g[f"{tag}_cpf"])) <= 1e-6, (tag, r["cpf"], float(g[f"{tag}_cpf"]))
    assert abs(r["step"] - float(g[f"{tag}_step"])) <= 1e-6, (tag, r["step"], float(g[f"{tag}_step"]))
    # the q terms THROUGH the reference's rot against the folded form (no rotation): float rounding
    assert abs(r["q"][0] - float(g[f"{tag}_q_img"])) <= 1e-6 and abs(r["q"][1] - float(g[f"{tag}_q_txt"])) <= 1e-6
    for j, side in enumerate(("gi", "gt")):
        _close(r["g_cpf"][j], g[f"{tag}_cpf_{side}"], (tag, "cpf", side))
        _close(r["g_step"][j], ds.step_grad(g, tag, side), (tag, "step", side))
        # The q gradient against its OWN maximum.  In unit space it is nearly parallel to the row (sigma (1 - sigma) (1 - 2 sigma) ~
        # -z / 8), so the normaliser's projection leaves about a seventh of it and float32 autograd carries up to 4e-5 of the result:
        # this golden is the reference's rot and bit_var_loss run in float64 (make_golden22.py), stored as float32
        _close(r["g_step"][j] - r["g_cpf"][j], g[f"{tag}_q_{side}"], (tag, "q", side), 1e-6)
    _close(r["g_cpf"][2], g[f"{tag}_cpf_gw"], (tag, "gw"))
    above = np.array([int((r["above"] & (c["lab"] == 0)).sum()), int((r["above"] & (c["lab"] == 1)).sum())])
    assert np.array_equal(above, g[f"{tag}_above"])


def test_the_goldens_hold_the_cases_the_loss_can_go_wrong_on(golden):
    g = golden("dscph.npz")
    assert g["none_above_above"].tolist() == [0, 0]
    c = _case("all_neg_above")
    assert int(g["all_neg_above_above"][0]) == 2 * int((c["lab"] == 0).sum()) > 0             # every negative, both modalities
    assert not _case("zero_labels")["lab"].any() and _case("row_ones")["lab"][2].all()
    z = _case("zero_cos")
    r = ds.cpf_step(z["hi"], z["ht"], z["W"], z["lab"])
    assert r["cos"][0, 0, 0] == 0.0 and z["lab"][0, 0] == 1.0 and r["pos"][0, 0, 0]           # c == 0 on a positive: tp's gradient passes
    assert max(int(g[f"{t}_above"][0]) for t in TAGS) >= 40 and max(int(g[f"{t}_above"][1]) for t in TAGS) >= 40


def _torch_step(hi, ht, W, Y, s, qw):
    """the definition as float64 torch ops (the exponentials detached, clamp(min=0) as the reference writes it)"""
    F = torch.nn.functional
    total = 0.0
    for h in (hi, ht):
        c = F.linear(F.normalize(h), F.normalize(W))
        tp = (c.clamp(min=0.0) * Y * 2).sum() + s["b"]
        lp = ((1.0 - c) * torch.exp((1.0 - c) * s["sp"]).detach() * Y).sum()
        ln = (torch.where(c > s["tau"], (c - s["psi"]) * torch.exp((c - s["mu"]) * s["sn"]).detach(), torch.zeros_like(c)) * (1 - Y)).sum()
        sg = torch.sigmoid(F.normalize(h))
        total = total + (1.0 - tp / (tp + lp + ln)) + qw * (sg * (1 - sg)).mean()
    return total


@pytest.mark.parametrize("tag", ["B33_K64_C24", "all_neg_above", "zero_cos", "zero_labels"])
def test_restatement_gradient_is_autograds_in_float64(tag):
    c = _case(tag)
    hi, ht, W = (torch.from_numpy(c[k]).double().requires_grad_() for k in ("hi", "ht", "W"))
    total = _torch_step(hi, ht, W, torch.from_numpy(c["lab"]).double(), ds.SCALARS, 0.5)
    total.backward()
    r = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"], quant_weight=0.5)
    assert abs(r["step"] - float(total.detach())) <= 1e-12
    for got, want in zip(r["g_step"], (hi.grad, ht.grad, W.grad)):
        _close(got, want.numpy(), tag, 1e-12)


def test_restatement_decides_on_given_cosines_in_their_arithmetic():
    """cos= a float32 array: `c > tau` is a float32 comparison against float32(tau), as torch compares a float32 tensor with a number,
    and the masks follow the GIVEN values, not the restatement's own cosines"""
    c = _case("B5_K16_C3")
    base = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"])
    given = base["cos"].astype(np.float32)
    given[0, 0, 0] = np.float32(0.9)                                               # equal to float32(tau): not above
    given[1, 0, 0] = np.nextafter(np.float32(0.9), np.float32(1))                  # one ulp more: above
    given[0, 1, 1] = np.float32(-0.0)                                              # -0.0 >= 0: the gradient of tp passes
    given[1, 1, 1] = -np.float32(1e-30)
    r = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"], cos=given)
    assert not r["above"][0, 0, 0] and r["above"][1, 0, 0] and r["pos"][0, 1, 1] and not r["pos"][1, 1, 1]
    assert np.array_equal(r["cos"], base["cos"])                                   # the values stay the float64 ones
    # tau = 0.5 is a float32 number: equality is not above in either arithmetic
    half = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"], scalars=dict(tau=0.5), cos=np.full_like(given, 0.5))
    assert not half["above"].any() and half["pos"].all()


def test_registry_flags_and_query_rows(monkeypatch):
    import main
    import query
    from code_rules import CODE_RULES, SOFT_RULES, sign_code, soft_output
    assert main.trainers["CPFH"].__name__ == "DScPHTrainer"
    for name in ("DPBE", "DDWSH", "DScPH", "DPSIH", "DGHDGH"):                 # (the reference's name stays a refusal: tests/test_host.py)
        with pytest.raises(NotImplementedError):
            main.trainers[name]
    assert set(CODE_RULES) == set(SOFT_RULES) == set(query.MODELS) and "CPFH" in CODE_RULES
    assert CODE_RULES["CPFH"] is sign_code and SOFT_RULES["CPFH"] is soft_output and query.MODELS["CPFH"] == ("model.DScPH", "MDScPH")
    query.check_method("CPFH")
    from train.DScPH.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", "--method", "CPFH", "--dataset", "synthetic", "--output-dim", "64"])
    a = get_args(argparse.Namespace(method="CPFH", dataset="synthetic", output_dim=64, is_train=True))
    assert a.save_dir.endswith("CPFH/synthetic/64")
    assert (a.cpf_tau, a.cpf_psi, a.cpf_sp, a.cpf_sn, a.cpf_mu, a.cpf_b, a.quant_weight) == (0.9, 0.7, 1.3, 1.3, 1.0, 2.0, 1.0)
    monkeypatch.setattr(sys, "argv", ["main.py", "--cpf-tau", "0.8", "--cpf-psi", "0.5", "--cpf-sp", "2", "--cpf-sn", "3", "--cpf-mu", "0.9",
                                      "--cpf-b", "1", "--quant-weight", "0.25", "--hypseed", "7", "--alpha", "0.3"])
    a = get_args(argparse.Namespace(method="CPFH", dataset="synthetic", output_dim=64, is_train=True))
    assert (a.cpf_tau, a.cpf_psi, a.cpf_sp, a.cpf_sn, a.cpf_mu, a.cpf_b, a.quant_weight) == (0.8, 0.5, 2.0, 3.0, 0.9, 1.0, 0.25)
    from train.DScPH.loss import CPFLoss
    torch.manual_seed(0)
    m = CPFLoss(16, 5)
    assert m.weight.shape == (5, 16) and [n for n, _ in m.named_parameters()] == ["weight"]
    assert m.scalars == ds.SCALARS and m.quant_weight == 1.0
    bound = (6.0 / (16 + 5)) ** 0.5                                                # xavier_uniform_
    w = m.weight.detach()
    assert float(w.abs().max()) <= bound and float(w.std()) > 0.3 * bound


def test_header_declares_the_entry_points():
    import cmh_native as N
    src = open(os.path.join(ROOT, "include", "cmh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("cmh_cpf_workspace_bytes", "cmh_cpf_tape_bytes", "cmh_cpf_loss", "cmh_cpf_loss_backward"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in N.SIGNATURES
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", src) and N.ABI_VERSION == 6
    assert "train/DScPH/CPF_loss.py:24-54" in src
    kernel = open(os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "csrc", "cpf.hip")).read()
    for const, value in (("kCpfRows", N.CPF_ROWS), ("kCpfChunk", N.CPF_CHUNK), ("kCpfSlice", N.CPF_SLICE), ("kCpfMaxB", N.CPF_MAX_B),
                         ("kCpfMaxK", N.CPF_MAX_K), ("kCpfMaxC", N.CPF_MAX_C)):                # the binding's copies are the kernel's
        assert re.search(r"\b%s = %d\b" % (const, value), kernel), const


def test_workspace_query_and_refusals_without_a_launch():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_version() == 6                                                  # entry points were added, nothing else changed
    buf = (C.c_uint8 * 1024)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)                                # a 256-byte aligned host address the calls never read
    ws, tape = lib.cmh_cpf_workspace_bytes, lib.cmh_cpf_tape_bytes
    for q in (ws, tape):
        assert q(0, 16, 4) == 0 and q(1025, 16, 4) == 0 and q(8, 0, 4) == 0 and q(8, 129, 4) == 0 and q(8, 16, 0) == 0 and q(8, 16, 1025) == 0
        assert q(1024, 128, 1024) > q(128, 64, 24) > q(1, 1, 1) > 0
    assert tape(8, 16, 4) == 4 * (16 + 2 * 8 * 16 + 4 * 16 + 2 * 8 + 4) and ws(8, 16, 4) > tape(8, 16, 4)
    big = 1 << 30
    fwd = lambda B=8, K=16, Cn=4, hi=p, lab=p, w=p, out=p, n=big, wsp=p: lib.cmh_cpf_loss(
        hi, p, lab, w, B, K, Cn, 0.9, 0.7, 1.3, 1.3, 1.0, 2.0, 1.0, out, out, out, None, wsp, n, None)
    bwd = lambda B=8, K=16, Cn=4, lab=p, tp=p, d=p: lib.cmh_cpf_loss_backward(lab, p, tp, B, K, Cn, 0.9, 1.3, 1.3, 1.0, 1.0, p, d, p, p, None)
    for name, call in (("cpf_loss", fwd), ("cpf_loss_backward", bwd)):
        for kw, word in ((dict(B=1025), b"1024"), (dict(B=0), b"B=0"), (dict(K=129), b"128"), (dict(K=0), b"K=0"), (dict(Cn=0), b"C=0"),
                         (dict(Cn=1025), b"C=1025"), (dict(lab=None), b"null pointer")):
            assert call(**kw) == INVALID, (name, kw)
            msg = lib.cmh_last_error()
            assert msg.startswith(name.encode() + b":") and word in msg, (name, kw, msg)
    for kw in (dict(hi=None), dict(w=None), dict(out=None)):
        assert fwd(**kw) == INVALID and b"cpf_loss: null pointer" in lib.cmh_last_error()
    for kw in (dict(tp=None), dict(d=None)):
        assert bwd(**kw) == INVALID and b"cpf_loss_backward: null pointer" in lib.cmh_last_error()
    assert fwd(wsp=None) == INVALID and b"cpf_loss: null workspace" in lib.cmh_last_error()
    assert fwd(n=ws(8, 16, 4) - 1) == INVALID and b"cpf_loss: workspace too small" in lib.cmh_last_error()
    assert fwd(wsp=C.c_void_p(p.value + 8)) == INVALID and b"not 256-byte aligned" in lib.cmh_last_error()


def test_cpu_tensors_are_refused():
    import cmh_native as N
    z = torch.zeros
    with pytest.raises(N.NativeError, match="GPU only"):
        N.cpf_loss(z(4, 8), z(4, 8), z(4, 2), z(2, 8))
