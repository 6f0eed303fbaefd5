"""DDWSH without a GPU: the float64 restatement of tests/ddwshutil.py against the REFERENCE's own margin loss, counts, autograd gradients
and sampling distributions (tests/golden/make_golden23.py) and against torch autograd in float64, the committed uniforms of the sampler
tests, the registry rows and flags, the header, and the host-side refusals of the new entry points (nothing is launched)."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import ddwshutil as dw
from conftest import ROOT

INVALID = -1                                                                      # CMH_ERR_INVALID (include/cmh.h)
GOLDEN_TAGS = [f"B{B}_K{K}_C{Cn}" for B, K, Cn, _, _ in dw.CASES]
TAGS = GOLDEN_TAGS + [c["tag"] for c in dw.special_cases()]
ENTRIES = ("cmh_dws_workspace_bytes", "cmh_dws_distances", "cmh_dws_mine", "cmh_dws_margin_loss", "cmh_dws_margin_loss_backward")


def _close(got, want, what, tol=1e-5):
    scale = max(np.abs(want).max(), 1e-30)
    assert np.abs(got - want).max() <= tol * scale, (what, np.abs(got - want).max(), scale)


def _case(tag):
    return {c["tag"]: c for c in dw.all_cases()}[tag]


def _q(w):
    tot = w.sum(1, keepdims=True)
    return w / np.where(tot > 0, tot, 1.0)


@pytest.mark.parametrize("mode", dw.MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_on_its_triplets(golden, tag, mode):
    g = golden("ddwsh.npz")
    c = _case(tag)
    key = f"{tag}_{mode}"
    trip = g[f"{key}_trip"]
    if (trip >= 0).any():
        assert float(g[f"{key}_gap"]) >= 100.0 * float(g[f"{key}_err"])                       # the fixture's own condition
    y = c["x"] if mode == "intra" else c["y"]
    r = dw.margin_loss(c["x"], y, c["lab"], c["beta"], trip)
    assert r["count"] == int(g[f"{key}_count"])
    assert abs(r["loss"] - float(g[f"{key}_loss"])) <= 1e-6, (key, r["loss"], float(g[f"{key}_loss"]))
    if mode == "intra":
        _close(r["dx"] + r["dy"], g[f"{key}_gx"], (key, "gx"))
    else:
        _close(r["dx"], g[f"{key}_gx"], (key, "gx"))
        _close(r["dy"], g[f"{key}_gy"], (key, "gy"))
    _close(r["dbeta"], g[f"{key}_gbeta"], (key, "gbeta"))
    # the reference's triplets are triplets of the definition: valid anchors exactly, a positive other than the anchor, a negative
    pos, valid = dw.positives(c["lab"])
    assert np.array_equal(trip[:, 0] >= 0, valid) and np.array_equal(trip[:, 1] >= 0, valid)
    for i in np.flatnonzero(valid):
        assert pos[i, trip[i, 0]] and trip[i, 0] != i and not pos[i, trip[i, 1]]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_weights_are_the_references_q(golden, tag):
    """per case the deviation the GPU test doubles for the kernel (tests/ddwshutil.py::Q_DEV holds the measured values)"""
    g = golden("ddwsh.npz")
    c = _case(tag)
    B, K = c["x"].shape
    bound = dw.Q_DEV.get(tag, dict(intra=1e-5, cross=1e-5, emb=1e-5))
    for mode, y, space, key in (("intra", c["x"], "distances", f"{tag}_intra_q"), ("cross", c["y"], "distances", f"{tag}_cross_q"),
                                ("emb", c["x"], "embeddings", f"{tag}_emb_q")):
        M, dim = dw.mining_matrix(dw.distances(c["x"], y), K, space=space)
        assert dim == (B if space == "distances" else K)
        w = dw.sphere_weights(M, c["lab"], dim)
        ref = g[key].astype(np.float64)
        dev = float(np.abs(_q(w) - ref).max())
        print(f"{tag} {mode}: max |q - reference q| {dev:.3e} (committed {bound[mode]:.3e})")
        assert dev <= bound[mode], (tag, mode, dev)
        assert np.array_equal(ref.sum(1) > 0, dw.positives(c["lab"])[1])                      # a q row for every valid anchor, no other
        # every negative the reference drew has positive weight
        trip = g[f"{tag}_{'emb' if mode == 'emb' else mode}_trip"]
        for i in np.flatnonzero(trip[:, 1] >= 0):
            assert w[i, trip[i, 1]] > 0 and ref[i, trip[i, 1]] > 0


def test_the_goldens_hold_the_cases_the_sampler_can_go_wrong_on(golden):
    g = golden("ddwsh.npz")
    lonely, shares, none = (c for c in dw.special_cases())
    assert not dw.positives(lonely["lab"])[1][0] and dw.positives(lonely["lab"])[0][0].sum() == 1      # no other positive
    assert not dw.positives(shares["lab"])[1][0] and dw.positives(shares["lab"])[0][0].all()           # shares a label with every item
    assert dw.positives(lonely["lab"])[1][1:].all() and dw.positives(shares["lab"])[1][1:].all()
    assert not dw.positives(none["lab"])[1].any()
    for mode in dw.MODES:
        assert (g[f"{lonely['tag']}_{mode}_trip"][0] == -1).all() and (g[f"{shares['tag']}_{mode}_trip"][0] == -1).all()
        assert (g[f"{none['tag']}_{mode}_trip"] == -1).all() and int(g[f"{none['tag']}_{mode}_count"]) == 0
        assert float(g[f"{none['tag']}_{mode}_loss"]) == 0.0
    # most anchors of the larger cases have at least 2 other positives and at least 4 eligible negatives
    for B, K, Cn, seed, p in dw.CASES[1:]:
        pos, valid = dw.positives(dw.ddwsh_case(B, K, Cn, seed, p)["lab"])
        rich = ((pos.sum(1) - 1 >= 2) & ((~pos).sum(1) >= 4)).sum()
        assert 2 * rich > B, (B, rich)


def test_step_sum_and_gradients(golden):
    g = golden("ddwsh.npz")
    for tag in TAGS[:-1]:
        c = _case(tag)
        loss, gi, gt, gb = dw.step_loss(c["x"], c["y"], c["lab"], c["beta"], g[f"{tag}_step_trips"])
        assert abs(loss - float(g[f"{tag}_step_loss"])) <= 2e-6
        _close(gi, g[f"{tag}_step_gi"], (tag, "gi"))
        _close(gt, g[f"{tag}_step_gt"], (tag, "gt"))
        _close(gb, g[f"{tag}_step_gbeta"], (tag, "gbeta"))


@pytest.mark.parametrize("tag", ["B12_K16_C4", "B33_K16_C5"])
def test_restatement_gradient_is_autograds_in_float64(golden, tag):
    c = _case(tag)
    trip = golden("ddwsh.npz")[f"{tag}_cross_trip"]
    F = torch.nn.functional
    x, y, beta = (torch.from_numpy(np.asarray(c[k], np.float64)).requires_grad_() for k in ("x", "y", "beta"))
    lab = torch.from_numpy(c["lab"]).double()
    d = F.normalize(x)[:, None, :] - F.normalize(y)[None, :, :]
    D = (d * d).sum(2).sqrt().clamp(min=1e-8)
    a = torch.from_numpy(np.flatnonzero(trip[:, 0] >= 0))
    bi = (lab[a] * beta).sum(1) / lab[a].sum(1)
    pos, neg = F.relu(D[a, torch.from_numpy(trip[a, 0]).long()] - bi + dw.MARGIN), F.relu(bi - D[a, torch.from_numpy(trip[a, 1]).long()] + dw.MARGIN)
    total = (pos + neg).sum() / ((pos > 0) | (neg > 0)).sum()
    total.backward()
    r = dw.margin_loss(c["x"], c["y"], c["lab"], c["beta"], trip)
    assert abs(r["loss"] - float(total.detach())) <= 1e-12
    for got, want in zip((r["dx"], r["dy"], r["dbeta"]), (x.grad, y.grad, beta.grad)):
        _close(got, want.numpy(), tag, 1e-10)


def test_inverse_cdf_pick_and_its_edges():
    w = np.array([0.0, 0.25, 0.0, 0.5, 0.0, 0.25, 0.0])
    assert dw.pick_negative(w, 0.0)[0] == 1                                        # u = 0: the first item of positive weight
    assert dw.pick_negative(w, np.nextafter(np.float32(1), np.float32(0)))[0] == 5  # the last item of positive weight
    assert dw.pick_negative(w, 0.25)[0] == 3 and dw.pick_negative(w, 0.2499)[0] == 1      # searchsorted(side="right")
    assert dw.pick_negative(w, 0.25)[1] == 0.0 and dw.pick_negative(w, 0.5)[1] == 0.25
    one = np.zeros(9)
    one[4] = 3e-300
    assert all(dw.pick_negative(one, u)[0] == 4 for u in (0.0, 0.3, 0.999999))
    pos = np.array([True, False, True, True, False, True])
    assert [dw.pick_positive(pos, 2, u) for u in (0.0, 0.34, 0.67, 0.999999)] == [0, 3, 5, 5]


@pytest.mark.parametrize("space", dw.SPACES)
def test_committed_uniforms_stay_inside_the_skip_cap(space):
    """The GPU test compares a negative pick only where u total lies at least 1e-9 total from every cdf boundary and caps what that
    leaves out at 1 % of the anchors per case: on the restatement's weights the committed uniforms leave out none or nearly none"""
    for B, K, Cn, seed, p in dw.CASES:
        c = dw.ddwsh_case(B, K, Cn, seed, p)
        uni = dw.case_uniforms(3, B, seed)
        for q, (a, b) in enumerate(((c["x"], c["x"]), (c["y"], c["y"]), (c["x"], c["y"]))):
            M, dim = dw.mining_matrix(dw.distances(a, b), K, space=space)
            trip, margin = dw.mine(dw.sphere_weights(M, c["lab"], dim), c["lab"], uni[q])
            valid = dw.positives(c["lab"])[1]
            assert np.array_equal(trip[:, 0] >= 0, valid)
            assert (margin[valid] < 1e-9).sum() <= 0.01 * B, (B, space, q)


def test_registry_flags_and_query_rows(monkeypatch):
    import main
    import query
    from code_rules import CODE_RULES, SOFT_RULES, sign_code, soft_output
    assert main.trainers["DWSH"].__name__ == "DDWSHTrainer"
    for name in ("DPBE", "DDWSH", "DScPH", "DPSIH", "DGHDGH"):                 # (the reference's name stays a refusal: tests/test_host.py)
        with pytest.raises(NotImplementedError):
            main.trainers[name]
    assert set(CODE_RULES) == set(SOFT_RULES) == set(query.MODELS) and "DWSH" in CODE_RULES
    assert CODE_RULES["DWSH"] is sign_code and SOFT_RULES["DWSH"] is soft_output and query.MODELS["DWSH"] == ("model.DDWSH", "MDDWSH")
    query.check_method("DWSH")
    from train.DDWSH.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", "--method", "DWSH", "--dataset", "synthetic", "--output-dim", "64"])
    a = get_args(argparse.Namespace(method="DWSH", dataset="synthetic", output_dim=64, is_train=True))
    assert a.save_dir.endswith("DWSH/synthetic/64")
    assert (a.dws_margin, a.dws_beta, a.dws_cutoff, a.dws_space, a.dws_seed) == (0.2, 1.2, 0.5, "distances", 0)
    monkeypatch.setattr(sys, "argv", ["main.py", "--dws-margin", "0.3", "--dws-beta", "1.0", "--dws-cutoff", "0.4", "--dws-space", "embeddings",
                                      "--dws-seed", "7", "--similarity-function", "cosine"])
    a = get_args(argparse.Namespace(method="DWSH", dataset="synthetic", output_dim=64, is_train=True))
    assert (a.dws_margin, a.dws_beta, a.dws_cutoff, a.dws_space, a.dws_seed) == (0.3, 1.0, 0.4, "embeddings", 7)
    from train.DDWSH.loss import MarginLoss
    m = MarginLoss(5, beta=1.1, seed=3)
    assert [n for n, _ in m.named_parameters()] == ["beta"] and m.beta.shape == (5,) and bool((m.beta == 1.1).all())
    assert (m.margin, m.cutoff, m.space, m.seed) == (0.2, 0.5, "distances", 3)
    with pytest.raises(ValueError, match="space"):
        MarginLoss(5, space="cosine")
    a, b = (MarginLoss(5, seed=3).uniforms(3, 9, "cpu") for _ in range(2))        # one generator per module, seeded from the flag
    assert torch.equal(a, b) and a.shape == (3, 9, 2) and float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert not torch.equal(a, MarginLoss(5, seed=4).uniforms(3, 9, "cpu")) and not torch.equal(m.uniforms(3, 9, "cpu"), m.uniforms(3, 9, "cpu"))


def test_header_declares_the_entry_points():
    import cmh_native as N
    src = open(os.path.join(ROOT, "include", "cmh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in N.SIGNATURES
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", src) and N.ABI_VERSION == 6
    for cite in ("train/DDWSH/loss.py:17-20", "train/DDWSH/loss.py:22", "train/DDWSH/loss.py:28-49"):
        assert cite in src, cite
    kernel = open(os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "csrc", "dws.hip")).read()
    for const, value in (("kDwsMaxB", N.DWS_MAX_B), ("kDwsMaxK", N.DWS_MAX_K), ("kDwsMaxC", N.DWS_MAX_C), ("kDwsMaxPairs", N.DWS_MAX_PAIRS)):
        assert re.search(r"\b%s = %d\b" % (const, value), kernel), const              # the binding's copies are the kernel's
    assert "atomic" not in re.sub(r"//.*", "", kernel)


def test_workspace_query_and_refusals_without_a_launch():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_version() == 6                                                  # entry points were added, nothing else changed
    buf = (C.c_uint8 * 1024)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)                                # a 256-byte aligned host address the calls never read
    ws = lib.cmh_dws_workspace_bytes
    assert ws(0, 16, 4) == 0 and ws(1025, 16, 4) == 0 and ws(8, 0, 4) == 0 and ws(8, 129, 4) == 0 and ws(8, 16, 0) == 0 and ws(8, 16, 1025) == 0
    assert ws(1024, 128, 1024) > ws(128, 64, 24) > ws(1, 1, 1) > 0
    ptrs = (C.c_void_p * 3)(p, p, p)
    nulls = (C.c_void_p * 3)(None, None, None)
    big = 1 << 30
    dist = lambda n=1, B=8, K=16, u=ptrs, out=p: lib.cmh_dws_distances(u, ptrs, n, B, K, out, p, p, None)
    mine = lambda n=1, B=8, K=16, Cn=4, lab=p, uni=p, space=0, wsp=p, nb=big: lib.cmh_dws_mine(
        p, n, lab, B, K, Cn, 0.5, space, uni, p, None, wsp, nb, None)
    loss = lambda n=1, B=8, K=16, Cn=4, lab=p, uni=p, wsp=p, nb=big: lib.cmh_dws_margin_loss(p, uni, n, lab, p, B, Cn, 0.2, p, p, p, wsp, nb, None)
    bwd = lambda n=1, B=8, K=16, Cn=4, lab=p, u=ptrs, d=p: lib.cmh_dws_margin_loss_backward(
        u, ptrs, n, lab, B, K, Cn, p, p, p, p, p, p, p, ptrs, ptrs, d, None)
    for name, call, has_k, has_c in (("dws_distances", dist, True, False), ("dws_mine", mine, True, True), ("dws_margin_loss", loss, False, True),
                                     ("dws_margin_loss_backward", bwd, True, True)):
        cases = [(dict(B=1025), b"1024"), (dict(B=0), b"B=0"), (dict(n=0), b"pairs=0"), (dict(n=4), b"pairs=4")]
        cases += [(dict(K=129), b"K=129"), (dict(K=0), b"K=0")] if has_k else []
        cases += [(dict(Cn=0), b"C=0"), (dict(Cn=1025), b"C=1025"), (dict(lab=None), b"null pointer")] if has_c else []
        for kw, word in cases:
            assert call(**kw) == INVALID, (name, kw)
            msg = lib.cmh_last_error()
            assert msg.startswith(name.encode() + b":") and word in msg, (name, kw, msg)
    assert dist(u=None) == INVALID and b"dws_distances: null pointer" in lib.cmh_last_error()
    assert dist(out=None) == INVALID and b"dws_distances: null pointer" in lib.cmh_last_error()
    assert dist(u=nulls) == INVALID and b"dws_distances: null pointer in pair 0" in lib.cmh_last_error()
    assert mine(uni=None) == INVALID and b"dws_mine: null pointer" in lib.cmh_last_error()
    assert mine(space=2) == INVALID and b"dws_mine: space=2" in lib.cmh_last_error()
    assert loss(uni=None) == INVALID and b"dws_margin_loss: null pointer" in lib.cmh_last_error()
    assert bwd(d=None) == INVALID and b"dws_margin_loss_backward: null pointer" in lib.cmh_last_error()
    assert bwd(u=nulls) == INVALID and b"dws_margin_loss_backward: null pointer in pair 0" in lib.cmh_last_error()
    for name, call in (("dws_mine", mine), ("dws_margin_loss", loss)):
        assert call(wsp=None) == INVALID and name.encode() + b": null workspace" in lib.cmh_last_error()
        assert call(nb=ws(8, 16, 4) - 1) == INVALID and name.encode() + b": workspace too small" in lib.cmh_last_error()
        assert call(wsp=C.c_void_p(p.value + 8)) == INVALID and b"not 256-byte aligned" in lib.cmh_last_error()


def test_cpu_tensors_and_bad_names_are_refused():
    import cmh_native as N
    z = torch.zeros
    with pytest.raises(N.NativeError, match="GPU only"):
        N.dws_distances([(z(4, 8), z(4, 8))])
    with pytest.raises(N.NativeError, match="GPU only"):
        N.dws_mine(z(1, 4, 4), z(4, 2), 8, z(1, 4, 2))
    with pytest.raises(N.NativeError, match="GPU only"):
        N.dws_margin_loss([(z(4, 8), z(4, 8))], z(4, 2), z(2), z(1, 4, 2, dtype=torch.int32))
    with pytest.raises(N.NativeError, match="space 'cosine'"):
        N.dws_mine(z(1, 4, 4), z(4, 2), 8, z(1, 4, 2), space="cosine")
