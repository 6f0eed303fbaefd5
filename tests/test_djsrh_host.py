"""DJSRH without a GPU: the float64 restatement of tests/djsrhutil.py against torch autograd and its own edge properties, the registry,
query and rule rows, the trainer's flags and one-rank refusal, and the host-side refusals of the cmh_djsrh_* entry points (nothing is
launched)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

import djsrhutil as dj
from conftest import ROOT

NEW = ["cmh_djsrh_workspace_bytes", "cmh_djsrh_target", "cmh_djsrh_loss", "cmh_djsrh_loss_backward"]
INVALID = -1                                                                      # CMH_ERR_INVALID (include/cmh.h)


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("B,K,D", dj.HOST_SHAPES)
def test_hand_derived_gradient_equals_autograd_in_float64(B, K, D):
    import torch
    import torch.nn.functional as F
    c = dj.case(B, K, D)
    beta, eta, mu, l1, l2 = dj.SCALARS
    S = dj.target(c["fi"], c["ft"], beta, eta, mu)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    fi, ft = F.normalize(t(c["fi"])), F.normalize(t(c["ft"]))
    st = beta * (2 * fi @ fi.T - 1) + (1 - beta) * (2 * ft @ ft.T - 1)
    S_t = mu * ((1 - eta) * st + (eta / B) * st @ st.T)
    assert np.abs(S_t.numpy() - S).max() <= 1e-12
    hi, ht = t(c["hi"]).requires_grad_(), t(c["ht"]).requires_grad_()
    bi, bt = F.normalize(hi), F.normalize(ht)
    terms = [((bi @ bi.T - S_t) ** 2).mean(), ((bi @ bt.T - S_t) ** 2).mean(), ((bt @ bt.T - S_t) ** 2).mean()]
    total = l1 * terms[0] + terms[1] + l2 * terms[2]
    (0.25 * total).backward()
    r = dj.loss(c["hi"], c["ht"], S, l1, l2, dloss=0.25)
    assert abs(r["loss"] - float(total.detach())) <= 1e-12
    assert np.abs(r["terms"] - np.array([float(v.detach()) for v in terms])).max() <= 1e-12
    print(f"\n({B}, {K}, {D}): max |gi - autograd| {np.abs(r['gi'] - hi.grad.numpy()).max():.2e}, gt {np.abs(r['gt'] - ht.grad.numpy()).max():.2e}")
    assert np.abs(r["gi"] - hi.grad.numpy()).max() <= 1e-12 and np.abs(r["gt"] - ht.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("B,K,D", dj.HOST_SHAPES)
def test_target_is_symmetric(B, K, D):
    c = dj.case(B, K, D)
    S = dj.target(c["fi"], c["ft"], *dj.SCALARS[:3])
    assert S.shape == (B, B) and np.abs(S - S.T).max() <= 1e-14


def test_one_row_terms_are_one_minus_mu_squared():
    """B = 1: St = [[1]], S = mu ((1 - eta) + eta) = mu, b b^T = 1: the II and TT residuals are 1 - mu"""
    c = dj.case(1, 16, 64)
    for mu in (1.5, 1.0, 0.25):
        S = dj.target(c["fi"], c["ft"], 0.9, 0.4, mu)
        r = dj.loss(c["hi"], c["ht"], S, 0.1, 0.1)
        assert abs(S[0, 0] - mu) <= 1e-15
        assert abs(r["terms"][0] - (1.0 - mu) ** 2) <= 1e-15 and abs(r["terms"][2] - (1.0 - mu) ** 2) <= 1e-15


def test_zero_feature_row_gives_minus_one():
    c = dj.case(7, 16, 40)
    c["fi"][3] = 0.0
    c["ft"][3] = 0.0
    st = dj.s_tilde(c["fi"], c["ft"], 0.9)
    assert (st[3] == -1.0).all() and (st[:, 3] == -1.0).all() and st[3, 3] == -1.0
    assert np.isfinite(dj.target(c["fi"], c["ft"], *dj.SCALARS[:3])).all()


# ---------------------------------------------------------------------------------------------------- registration
def test_registry_query_and_rule_rows():
    import main
    import query
    from code_rules import CODE_RULES, SOFT_RULES, code_rule, sign_code, soft_output, soft_rule
    assert main.trainers["DJSRH"].__name__ == "DJSRHTrainer"
    assert main._REGISTRY["DJSRH"] == ("train.DJSRH.hash_train", "DJSRHTrainer")
    query.check_method("DJSRH")
    assert query.MODELS["DJSRH"] == ("model.DJSRH", "MDJSRH")
    assert CODE_RULES["DJSRH"] is sign_code and SOFT_RULES["DJSRH"] is soft_output
    assert code_rule("DJSRH") is sign_code and soft_rule("DJSRH") is soft_output
    assert set(CODE_RULES) == set(SOFT_RULES) == set(query.MODELS)
    from model.DJSRH import MDJSRH
    from model.modelbase import Baseclip
    assert issubclass(MDJSRH, Baseclip)


def _args(monkeypatch, *cli):
    from train.DJSRH.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", *cli])
    return get_args(argparse.Namespace(method="DJSRH", dataset="synthetic", output_dim=64, is_train=True))


def test_flag_defaults_and_save_dir(monkeypatch):
    from train.DJSRH.loss import JointSemanticsLoss
    a = _args(monkeypatch)
    assert (a.djsrh_beta, a.djsrh_eta, a.djsrh_mu, a.djsrh_lambda1, a.djsrh_lambda2, a.init_heads) == (0.9, 0.4, 1.5, 0.1, 0.1, "random")
    assert JointSemanticsLoss().scalars() == (0.9, 0.4, 1.5, 0.1, 0.1) == dj.SCALARS
    assert a.batch_size == 300                                                     # the default batch the kernels are sized around
    assert a.save_dir.endswith(os.path.join("DJSRH", "synthetic", "64"))
    b = _args(monkeypatch, "--djsrh-beta", "0.5", "--djsrh-eta", "0.25", "--djsrh-mu", "1.25", "--djsrh-lambda1", "0.2", "--djsrh-lambda2", "0.3",
              "--init-heads", "cca")
    assert (b.djsrh_beta, b.djsrh_eta, b.djsrh_mu, b.djsrh_lambda1, b.djsrh_lambda2, b.init_heads) == (0.5, 0.25, 1.25, 0.2, 0.3, "cca")
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--init-heads", "labels")


def test_more_than_one_rank_is_refused_by_name_before_any_data(monkeypatch, tmp_path):
    import dist_utils as du
    import main
    monkeypatch.setattr(du, "world_size", lambda: 2)
    monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path / "run"), "--data-dir", str(tmp_path / "missing")])
    with pytest.raises(NotImplementedError, match="DJSRH: the target cache is built on one rank"):
        main.trainers["DJSRH"](argparse.Namespace(method="DJSRH", dataset="flickr", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


def test_trainer_refuses_bad_scalars_by_name(monkeypatch, tmp_path):
    import main
    for bad in (("--djsrh-beta", "1.5"), ("--djsrh-eta", "-0.1"), ("--djsrh-mu", "0"), ("--djsrh-lambda1", "-1")):
        monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path / "run"), *bad])
        with pytest.raises(ValueError, match="DJSRH: --djsrh-"):
            main.trainers["DJSRH"](argparse.Namespace(method="DJSRH", dataset="synthetic", output_dim=16, is_train=True), 0)
    assert not (tmp_path / "run").exists()


# ---------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_in_binding_and_header():
    import cmh_native as N
    raw = open(os.path.join(ROOT, "include", "cmh.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(cmh_djsrh_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW)
    for name in NEW:
        assert name in N.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert len(N.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name             # one ctypes row per parameter
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", header) and N.ABI_VERSION == 6
    assert N.lib().cmh_version() == 6                                                    # entry points were added, nothing else changed


def test_workspace_query():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_djsrh_workspace_bytes(0, 64, 512) == 0
    for dims in ((-1, 64, 512), (1025, 64, 512), (300, 0, 512), (300, 129, 512), (300, 64, 0), (300, 64, 4097)):
        assert lib.cmh_djsrh_workspace_bytes(*dims) == 0, dims
    small, default, largest = (lib.cmh_djsrh_workspace_bytes(*d) for d in ((1, 1, 1), (300, 64, 512), (1024, 128, 4096)))
    assert 0 < small < default < largest and default >= 300 * 300 * 4 + 2 * 300 * 4 and default % 256 == 0


def test_host_side_refusals_before_any_launch():
    """Null pointers, sizes out of range, a workspace that is null, one byte short or misaligned: CMH_ERR_INVALID with a message that
    names the call, and nothing launched (the operands are host addresses the call never reads)."""
    import cmh_native as N
    lib = N.lib()
    one, ws, big = 256, 4096, 1 << 40

    def refused(rc, *words):
        msg = lib.cmh_last_error()
        assert rc == INVALID, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def holes(count):
        for hole in range(count):
            ptrs = [one] * count
            ptrs[hole] = None
            yield ptrs

    target = lambda B, D, p=(one, one, one), w=ws, n=big: lib.cmh_djsrh_target(p[0], p[1], B, D, 0.9, 0.4, 1.5, p[2], w, n, None)
    loss = lambda B, K, p=(one,) * 5, w=ws, n=big: lib.cmh_djsrh_loss(p[0], p[1], p[2], B, K, 0.1, 0.1, p[3], p[4], None, w, n, None)
    back = lambda B, K, p=(one,) * 6, w=ws, n=big: lib.cmh_djsrh_loss_backward(p[0], p[1], p[2], B, K, 0.1, 0.1, p[3], p[4], p[5], w, n, None)
    for B, D in ((0, 64), (1025, 64), (-3, 64), (8, 0), (8, 4097)):
        refused(target(B, D), b"djsrh_target", b"1024", b"4096")
    for name, call in ((b"djsrh_loss", loss), (b"djsrh_loss_backward", back)):
        for B, K in ((0, 16), (1025, 16), (8, 0), (8, 129)):
            refused(call(B, K), name, b"1024", b"128")
    for p in holes(3):
        refused(target(8, 64, p), b"djsrh_target: null pointer")
    for p in holes(5):
        refused(loss(8, 16, p), b"djsrh_loss: null pointer")
    for p in holes(6):
        refused(back(8, 16, p), b"djsrh_loss_backward: null pointer")
    need = lib.cmh_djsrh_workspace_bytes(300, 64, 512)
    for name, call in ((b"djsrh_target", lambda **kw: target(300, 512, **kw)), (b"djsrh_loss", lambda **kw: loss(300, 64, **kw)),
                       (b"djsrh_loss_backward", lambda **kw: back(300, 64, **kw))):
        refused(call(w=None), name, b"null workspace")
        refused(call(n=need - 1), name, b"workspace too small")
        refused(call(w=ws + 4), name, b"aligned")


def test_cpu_tensors_and_shapes_are_refused():
    import torch
    import cmh_native as N
    with pytest.raises(N.NativeError):
        N.djsrh_target(torch.zeros(4, 8), torch.zeros(4, 8), 0.9, 0.4, 1.5)
    with pytest.raises(N.NativeError):
        N.djsrh_loss(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 4), 0.1, 0.1)
