"""DDBH on the GPU (csrc/ddbh.hip through train/DDBH): the base-point loss, the quantisation term and the trainer's five-term sum against
the REFERENCE's own values and autograd gradients (tests/golden/make_golden20.py), against the float64 restatement of tests/ddbhutil.py
at the kernel's edges (codes in {-1, +1}: exact integer inner products, real ties at the tail cut), the trainer end to end, a three-step
training trajectory against the reference's, and the query front end.  Tolerances are those tests/test_gpu_qmi.py holds the sister loss to."""
import numpy as np
import pytest
import torch

import ddbhutil as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _loss_close(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), (what, got)
    else:
        assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (what, got, want)


def _grad_close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    print(f"{what}: max |diff| {np.abs(got.cpu().numpy() - ref).max():.3e} of max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=str(what))


def _run(K, u, v, lab, scale=2.0, bp=None):
    """BPLoss(K)(u, v, lab) with (scale * loss).backward(), twice -> loss, u.grad, v.grad (None when v is u); asserts that the no_grad
    value is the differentiable one bit for bit and that the second run's gradients have the first's bits"""
    from train.DDBH.loss import BPLoss
    bp = BPLoss(K) if bp is None else bp
    intra = v is u
    out = []
    for _ in range(2):
        a = tt(u).requires_grad_()
        b = a if intra else tt(v).requires_grad_()
        with torch.no_grad():
            plain = bp(a, b, tt(lab))
        loss = bp(a, b, tt(lab))
        assert plain.dim() == 0 and (torch.equal(plain, loss.detach()) or (torch.isnan(plain) and torch.isnan(loss.detach())))
        (scale * loss).backward()
        out.append((float(loss.detach()), a.grad, None if intra else b.grad))
    assert torch.equal(out[0][1], out[1][1]) and (intra or torch.equal(out[0][2], out[1][2]))
    return out[0]


def _against_restatement(K, c, what, sc=None):
    sc = dd.scalars(K) if sc is None else sc
    intra = c["v"] is c["u"]
    r = dd.bp_loss(c["u"], c["v"], c["lab"], sc)
    loss, gu, gv = _run(K, c["u"], c["v"], c["lab"])
    _loss_close(loss, r["loss"], what)
    if intra:
        _grad_close(gu, 2.0 * (r["du"] + r["dv"]), (what, "gu"))
    else:
        _grad_close(gu, 2.0 * r["du"], (what, "gu"))
        _grad_close(gv, 2.0 * r["dv"], (what, "gv"))
    return loss


@pytest.mark.parametrize("B,K,C,kind,seed", dd.CASES)
def test_bp_loss_and_step_match_reference(golden, B, K, C, kind, seed):
    from types import SimpleNamespace
    from train.DDBH.hash_train import DDBHTrainer
    from train.DDBH.loss import BPLoss
    g = golden("ddbh.npz")
    c = dd.ddbh_case(B, K, C, kind, seed)
    tag = c["tag"]
    for mode in dd.MODES:
        loss, gu, gv = _run(K, c["u"], c["u"] if mode == "intra" else c["v"], c["lab"])
        _loss_close(loss, float(g[f"{tag}_{mode}_loss"]), (tag, mode))
        _grad_close(gu, 2.0 * g[f"{tag}_{mode}_gu"], (tag, mode, "gu"))
        if mode == "cross":
            _grad_close(gv, 2.0 * g[f"{tag}_{mode}_gv"], (tag, mode, "gv"))
    me = SimpleNamespace(bp=BPLoss(K))
    hi, ht = tt(c["u"]).requires_grad_(), tt(c["v"]).requires_grad_()
    with torch.no_grad():
        plain = DDBHTrainer.compute_loss(me, hi, ht, tt(c["lab"]))
    loss = DDBHTrainer.compute_loss(me, hi, ht, tt(c["lab"]))
    assert torch.equal(plain, loss.detach())
    _loss_close(float(loss.detach()), float(g[f"{tag}_step_loss"]), (tag, "step"))
    (2.0 * loss).backward()
    _grad_close(hi.grad, 2.0 * g[f"{tag}_step_gi"], (tag, "step gi"))
    _grad_close(ht.grad, 2.0 * g[f"{tag}_step_gt"], (tag, "step gt"))


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_edges_batch_sizes(B):
    c = dd.edge_case(B, 16, 5, 3)
    _against_restatement(16, c, f"B{B} cross")
    _against_restatement(16, dict(c, v=c["u"]), f"B{B} intra")


@pytest.mark.parametrize("K,C", [(16, 1), (20, 65), (128, 5), (18, 7)])
def test_edges_code_and_label_widths(K, C):
    """K = 18 is no multiple of four (the scalar inner-product loop); C = 1: every labelled row is similar to every other"""
    c = dd.edge_case(67, K, C, 4, p=0.5 if C == 1 else 0.08 if C == 65 else 0.3)
    assert _against_restatement(K, c, f"K{K} C{C}") > 0.0


@pytest.mark.parametrize("sizes", [[1, 11], [1, 9], [9, 11], [10, 10], [9, 9, 2], [2, 1], [300, 11, 10, 9, 1]])
def test_edges_tail_lengths(sizes):
    """n_s = 1; n_d and n_s = 9, 10, 11 (tails of 1, 1, 2); [2, 1]: two rows and one, the smallest batch with every row active"""
    B = sum(sizes)
    u, v = (dd.recipe.sign_codes(B, 16, 6, f"ddbh_tail_{w}_{B}") for w in "uv")
    c = dict(u=u, v=v, lab=dd.group_labels(sizes))
    assert dd.bp_loss(u, v, c["lab"], dd.scalars(16))["active"].all()
    _against_restatement(16, c, f"groups {sizes}")


def test_edges_tied_tail_and_empty_kept_set():
    c = dd.tied_tail_case()
    assert (np.sort(c["u"][0] @ c["v"][4:].T)[-6:] == 12.0).all()                 # the tail of 3 is one tied value, with more ties beyond
    _against_restatement(16, c, "tied tail")
    c = dd.tied_tail_case(empty_kept=True)
    r = dd.bp_loss(c["u"], c["v"], c["lab"], dd.scalars(16))
    assert r["bp"][0] == 2.0 and np.isnan(r["loss"]) and np.isfinite(r["du"]).all()
    assert np.isnan(_against_restatement(16, c, "empty kept set"))                 # NaN from both; the gradients are finite and agree


def test_saturated_codes_stay_finite():
    c = dd.saturated_case()
    K, sc = 128, dd.scalars(128)
    r = dd.bp_loss(c["u"], c["v"], c["lab"], sc)
    _, ac, _, g = dd.coefficients(r["bpds"][0], sc)
    assert ac * 128.0 + g < -90.0                                                  # row 0's hard dissimilar entries: f = -110
    loss = _against_restatement(K, c, "saturated")
    assert np.isfinite(loss) and loss > 10.0


def test_quantization_loss_and_gradient():
    from train.DDBH.loss import quantization_loss
    c = dd.ddbh_case(37, 64, 24, "p0.1", 91)
    h = c["u"].copy()
    h[0, :3] = (0.0, 1.0, -1.0)                                                    # sign(0) = 0; saturated entries cost nothing
    want, grad = dd.quant_loss(h, c["lab"])
    x = tt(h).requires_grad_()
    with torch.no_grad():
        plain = quantization_loss(x, tt(c["lab"]))
    loss = quantization_loss(x, tt(c["lab"]))
    assert torch.equal(plain, loss.detach())
    _loss_close(float(loss.detach()), want, "quant")
    (2.0 * loss).backward()
    _grad_close(x.grad, 2.0 * grad, "quant grad")


def test_refusals_name_their_entry():
    import cmh_native as N
    from train.DDBH.loss import BPLoss, quantization_loss
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(N.NativeError, match=r"ddbh_bp_loss.*8192"):
        BPLoss(16)(z(8193, 16), z(8193, 16), z(8193, 2))
    for B, K, C in ((4, 0, 2), (4, 16, 0), (4, 1025, 2)):
        with pytest.raises(N.NativeError, match="ddbh_bp_loss"):
            BPLoss(16)(z(4, K), z(4, K), z(4, C))
        with pytest.raises(N.NativeError, match="ddbh_quant_loss"):
            quantization_loss(z(4, K), z(4, C))
    with pytest.raises(N.NativeError, match="ddbh_bp_loss"):
        BPLoss(16)(z(4, 16), z(5, 16), z(4, 2))                                    # operands of different shapes
    lib, sc = N.lib(), dd.scalars(16)
    arr = N._ptr_array([z(4, 16)])
    assert lib.cmh_ddbh_bp_loss(arr, None, 1, None, 4, 16, 2, *sc, None, None, None, None, 0, None) == -1
    assert b"ddbh_bp_loss: null pointer" in lib.cmh_last_error()
    assert lib.cmh_ddbh_bp_loss_backward(arr, arr, 1, None, 4, 16, 2, *sc, None, None, None, None, None, None) == -1
    assert b"ddbh_bp_loss_backward: null pointer" in lib.cmh_last_error()
    assert lib.cmh_ddbh_quant_loss(None, 1, None, 4, 16, 2, None, None, None, 0, None) == -1 and b"ddbh_quant_loss" in lib.cmh_last_error()
    assert lib.cmh_ddbh_quant_loss_backward(arr, 1, None, 4, 16, None, None, None) == -1 and b"ddbh_quant_loss_backward" in lib.cmh_last_error()


def test_ddbh_trainer_end_to_end(tmp_path, monkeypatch):
    """Registry -> DDBHTrainer -> model -> native loss and valid on the synthetic dataset, then two optimisation steps on the tiny CLIP."""
    import argparse
    import sys
    import recipe
    import main
    import dataset.synthetic as ds
    from train.DDBH.loss import quantization_loss
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path), "--batch-size", "16", "--num-workers", "0",
                                      "--resolution", "64", "--max-words", "16", "--query-num", "24", "--train-num", "32",
                                      "--synthetic-size", "120", "--epochs", "0"])
    tr = main.trainers["DDBH"](argparse.Namespace(method="DDBH", dataset="synthetic", output_dim=16, is_train=True), 0)
    assert type(tr).__name__ == "DDBHTrainer" and type(tr.model).__name__ == "MDDBH"
    tr.change_state(mode="valid")
    assert len(tr.valid(0)) == 4
    image, text, label, index = next(iter(tr.train_loader))
    with torch.no_grad():
        hi, ht = tr.model(image.to(DEV), text.to(DEV))
        lab = label.to(DEV).float()
        total = tr.compute_loss(hi, ht, lab)
        parts = (tr.bp(hi, hi, lab) + tr.bp(ht, ht, lab) + tr.bp(hi, ht, lab)) + 0.1 * (quantization_loss(hi, lab) + quantization_loss(ht, lab))
    assert torch.isfinite(total).item() and torch.equal(total, parts)
    tr.change_state(mode="train")
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = 4
    before = [[p.detach().clone() for p in grp["params"]] for grp in tr.optimizer.param_groups]
    for image, text, label, index in list(tr.train_loader)[:2]:
        assert torch.isfinite(tr._step(image, text, label)).item()
    assert len(before) == 3
    for grp, old in zip(tr.optimizer.param_groups, before):
        assert any(not torch.equal(p.detach(), o) for p, o in zip(grp["params"], old))
    assert all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_ddbh_training_trajectory_matches_reference(golden):
    """Three steps of the DDBH loop (tape forward -> LinearHash heads -> five-term loss -> backward through heads and towers -> fused
    BertAdam) on the tiny CLIP: the loss of every step and the final parameters against the REFERENCE's own run on the CPU
    (tests/golden/make_golden20.py; the heads in eval mode on both sides: no dropout draw)."""
    from types import SimpleNamespace
    import dchmtutil as du
    from model.base.optimization import BertAdam
    from model.modelbase import LinearHash
    from test_gpu_clip import _clip
    from train.DDBH.hash_train import DDBHTrainer
    from train.DDBH.loss import BPLoss
    g = golden("ddbh_traj.npz")
    assert float(g["gap_over_err"]) >= 100.0
    clip = _clip(du.CFG, du.SEED, "f32")
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    ih, th = ih.to(DEV), th.to(DEV)
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    me = SimpleNamespace(bp=BPLoss(dd.TRAJ_K))
    losses = []
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        loss = DDBHTrainer.compute_loss(me, ih(clip.encode_image(img.to(DEV))), th(clip.encode_text(txt.to(DEV))), lab.to(DEV).float())
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"DDBH trajectory: losses {losses} (reference {g['losses'].tolist()})")
    np.testing.assert_allclose(np.array(losses), g["losses"], rtol=1e-4)
    named = dict(clip.named_parameters())
    named.update({"image_hash." + n: p for n, p in ih.named_parameters()})
    named.update({"text_hash." + n: p for n, p in th.named_parameters()})
    worst = 0.0
    for key in g.files:
        if not key.startswith("p_"):
            continue
        ref = g[key]
        err = np.abs(du.cut(named[key[2:]].detach().cpu().numpy()) - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err < 1e-4, (key, err)
    print(f"DDBH trajectory: worst parameter error {worst:.2e} of max")


def test_query_encoder_gives_the_trainers_codes(tmp_path):
    """A state_dict saved from the tiny DDBH model, loaded by QueryEncoder("DDBH", ...): the codes get_code's rule writes for the same
    captions and pictures, and with soft=True the outputs whose sign they are."""
    import cmh_native as N
    import recipe
    from dataset.base import shared_tokenizer
    from dataset.gpu_transform import RaggedImages, preprocess
    from model.DDBH import MDDBH
    from query import QueryEncoder
    from test_gpu_query import BITS, CAPTIONS, MERGES, RES, WORDS, _images
    clip_file = str(tmp_path / "clip.pt")
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(dict(recipe.CLIP_TINY, vocab_size=49408), 7).items()}, clip_file)
    torch.manual_seed(11)
    model = MDDBH(outputDim=BITS, clipPath=clip_file, saveDir=str(tmp_path / "log")).to(DEV)
    ck = str(tmp_path / "DDBH.pth")
    torch.save(model.state_dict(), ck)
    model.float()
    model.clip.set_gemm_dtype("f32")
    model.eval()
    enc = QueryEncoder("DDBH", ck, clip_file, BITS, max_words=WORDS, resolution=RES, bpe_path=MERGES)
    tokens = shared_tokenizer(MERGES).encode_captions(CAPTIONS, WORDS).to(DEV)
    pixels = preprocess(RaggedImages.from_arrays(_images()).to(DEV), RES, train=False)
    with torch.no_grad():
        want_t, want_i = N.sign_codes(model.encode_text(tokens)), N.sign_codes(model.encode_image(pixels))
    got_t, got_i = enc.encode_text(CAPTIONS), enc.encode_image(_images())
    assert tuple(got_t.shape) == (len(CAPTIONS), BITS) and torch.equal(got_t, want_t) and torch.equal(got_i, want_i)
    soft_t, soft_i = enc.encode_text(CAPTIONS, soft=True), enc.encode_image(_images(), soft=True)
    assert torch.equal(torch.sign(soft_t), got_t) and torch.equal(torch.sign(soft_i), got_i) and soft_t.abs().max() < 1.0
    assert len({tuple(r) for r in got_t.tolist()}) > 1
