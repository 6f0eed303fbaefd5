"""MSCH on the GPU (csrc/msc.hip through train/MSCH): the all-triplets margin loss against the REFERENCE's own values, counts and
autograd gradients (tests/golden/make_golden21.py); at the kernel's edges against the float64 restatement of tests/mschutil.py DECIDING ON
THE KERNEL'S OWN similarities (larger batches always hold a triplet on a threshold), with counts and coefficients compared as integers and
the similarities themselves held to float64 within 1e-6; exact integer ties; bit-equality; the trainer end to end, a three-step training
trajectory against the reference's, and the query front end.  Tolerances are those of tests/test_gpu_ddbh.py.

Inputs of the edge tests: codes in {-1, +1} without normalisation (every similarity is an exact integer) or tanh codes WITH normalisation
(|s| <= 1, so a K-term float32 chain stays within K 2^-24 < 1e-5 in the worst case and near 1e-7 in fact): the two ways the 1e-6 bound on
s is a statement about the kernel and not about the magnitude of un-normalised products."""
import numpy as np
import pytest
import torch

import mschutil as ms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHORT = {"all": "all", "semi-hard": "semi"}
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _loss_close(got, want, what):
    print(f"{what}: loss {got!r} want {want!r}")
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (what, got, want)


def _grad_close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    print(f"{what}: max |diff| {np.abs(got.cpu().numpy() - ref).max():.3e} of max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=str(what))


def _run(u, v, lab, margin=ms.MARGIN, rule="all", normalize=False, scale=2.0):
    """MSCLoss(u, v, lab) with (scale * loss).backward(), twice -> loss, u.grad, v.grad (None when v is u); asserts that the no_grad value
    is the differentiable one bit for bit and that the second run's loss and gradients have the first's bits"""
    from train.MSCH.loss import MSCLoss
    fn = MSCLoss(margin, rule, normalize)
    intra = v is u
    out = []
    for _ in range(2):
        a = tt(u).requires_grad_()
        b = a if intra else tt(v).requires_grad_()
        with torch.no_grad():
            plain = fn(a, b, tt(lab))
        loss = fn(a, b, tt(lab))
        assert plain.dim() == 0 and torch.equal(plain, loss.detach())
        (scale * loss).backward()
        out.append((loss.detach().clone(), a.grad, None if intra else b.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and (intra or torch.equal(out[0][2], out[1][2]))
    return float(out[0][0]), out[0][1], out[0][2]


def _native(u, v, lab, margin, rule, normalize):
    """one forward through the wrapper -> loss, count, sim [B, B], coef [B, B] as numpy"""
    import cmh_native as N
    a = tt(u)
    b = a if v is u else tt(v)
    loss, count, sim, saved = N.msc_triplet_loss([(a, b)], tt(lab), margin, rule, normalize)
    return float(loss[0]), int(count[0]), sim[0].cpu().numpy(), saved[1][0].cpu().numpy()


def _against_restatement(c, what, rule="all", normalize=False, margin=ms.MARGIN):
    """the kernel against the restatement deciding on the kernel's own s: count and coef exactly, s within 1e-6 of float64, loss and
    gradients at the usual tolerances -> the restatement's result"""
    u, v, lab = c["u"], c["v"], c["lab"]
    loss, count, sim, coef = _native(u, v, lab, margin, rule, normalize)
    exact = ms.msc_loss(u, v, lab, margin, rule, normalize)
    print(f"{what}: max |s - float64 s| {np.abs(sim - exact['s']).max():.3e}; count {count} (float64 decides {exact['count']})")
    assert np.abs(sim - exact["s"]).max() <= 1e-6, what
    r = ms.msc_loss(u, v, lab, margin, rule, normalize, s=sim)
    assert count == r["count"], (what, count, r["count"])
    assert coef.dtype == np.int32 and np.array_equal(coef, r["coef"]), (what, int(np.abs(coef - r["coef"]).max()))
    _loss_close(loss, r["loss"], what)
    got, gu, gv = _run(u, v, lab, margin, rule, normalize)
    assert got == loss
    if v is u:
        _grad_close(gu, 2.0 * (r["du"] + r["dv"]), (what, "gu"))
    else:
        _grad_close(gu, 2.0 * r["du"], (what, "gu"))
        _grad_close(gv, 2.0 * r["dv"], (what, "gv"))
    return r


@pytest.mark.parametrize("B,K,C,seed,norms", ms.CASES)
def test_loss_count_and_step_match_reference(golden, B, K, C, seed, norms):
    from types import SimpleNamespace
    from train.MSCH.hash_train import MSCHTrainer
    from train.MSCH.loss import MSCLoss
    g = golden("msch.npz")
    c = ms.msch_case(B, K, C, seed)
    tag = c["tag"]
    for rule in ms.RULES:
        for mode in ms.MODES:
            for nz in norms:
                key = f"{tag}_{SHORT[rule]}_{mode}_n{int(nz)}"
                v = c["u"] if mode == "intra" else c["v"]
                assert _native(c["u"], v, c["lab"], ms.MARGIN, rule, nz)[1] == int(g[f"{key}_count"]), key
                loss, gu, gv = _run(c["u"], v, c["lab"], ms.MARGIN, rule, nz)
                _loss_close(loss, float(g[f"{key}_loss"]), key)
                _grad_close(gu, 2.0 * g[f"{key}_gu"], (key, "gu"))
                if mode == "cross":
                    _grad_close(gv, 2.0 * g[f"{key}_gv"], (key, "gv"))
    me = SimpleNamespace(msc=MSCLoss(), args=SimpleNamespace(msc_symmetric=False, msc_scale=ms.SCALE))
    hi, ht = tt(c["u"]).requires_grad_(), tt(c["v"]).requires_grad_()
    with torch.no_grad():
        plain = MSCHTrainer.compute_loss(me, hi, ht, tt(c["lab"]))
    loss = MSCHTrainer.compute_loss(me, hi, ht, tt(c["lab"]))
    assert torch.equal(plain, loss.detach())
    _loss_close(float(loss.detach()), float(g[f"{tag}_step_loss"]), (tag, "step"))
    (2.0 * loss).backward()
    _grad_close(hi.grad, 2.0 * g[f"{tag}_step_gi"], (tag, "step gi"))
    _grad_close(ht.grad, 2.0 * g[f"{tag}_step_gt"], (tag, "step gt"))


def test_symmetric_step_adds_the_fourth_pair():
    from types import SimpleNamespace
    from train.MSCH.hash_train import MSCHTrainer
    from train.MSCH.loss import MSCLoss
    c = ms.edge_case(33, 16, 5, 2, signs=True)
    me = SimpleNamespace(msc=MSCLoss(), args=SimpleNamespace(msc_symmetric=True, msc_scale=10.0))
    hi, ht = tt(c["u"]).requires_grad_(), tt(c["v"]).requires_grad_()
    loss = MSCHTrainer.compute_loss(me, hi, ht, tt(c["lab"]))
    want, gi, gt = ms.step_loss(c["u"], c["v"], c["lab"], scale=10.0, symmetric=True)           # integer similarities: one decision
    assert want > ms.step_loss(c["u"], c["v"], c["lab"], scale=10.0)[0]
    _loss_close(float(loss.detach()), want, "symmetric step")
    loss.backward()
    _grad_close(hi.grad, gi, "symmetric gi")
    _grad_close(ht.grad, gt, "symmetric gt")


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1024])
def test_edges_batch_sizes(B):
    """the ballot rounds of 256 columns and their 64-bit words; B = 1024 is the limit (262 144 pairs at most per anchor)"""
    p = 0.3 if B < 255 else 0.1
    c = ms.edge_case(B, 16, 5, 3, p=p)
    r = _against_restatement(c, f"B{B} cross all normalised", "all", True)
    assert B < 63 or r["count"] > 0
    c = ms.edge_case(B, 16, 5, 3, p=p, signs=True)
    _against_restatement(dict(c, v=c["u"]), f"B{B} intra semi-hard signs", "semi-hard", False, margin=2.0)


@pytest.mark.parametrize("K", [1, 4, 65, 128])
@pytest.mark.parametrize("rule", ms.RULES)
def test_edges_code_widths(K, rule):
    """K = 65: the backward's second column per lane holds one; K = 128 is the limit; K = 1: every unit row is +-1"""
    c = ms.edge_case(67, K, 5, 4)
    assert _against_restatement(c, f"K{K} cross normalised", rule, True)["count"] > 0 or K == 1
    c = ms.edge_case(67, K, 5, 4, signs=True)
    assert _against_restatement(dict(c, v=c["u"]), f"K{K} intra signs", rule, False, margin=1.0 if K < 4 else 2.0)["count"] > 0 or K == 1


@pytest.mark.parametrize("C", [1, 33, 65, 80])
def test_edges_label_widths(C):
    """C = 1: a labelled row is similar to every other labelled row and the rows without labels are everyone's negatives - and their own"""
    c = ms.edge_case(67, 16, C, 5, p=0.5 if C == 1 else 0.04)
    assert _against_restatement(c, f"C{C} cross", "all", True)["count"] > 0
    assert _against_restatement(dict(c, v=c["u"]), f"C{C} intra", "semi-hard", True)["count"] > 0


def _assert_zero(u, v, lab, rule="all"):
    loss, count, sim, coef = _native(u, v, lab, ms.MARGIN, rule, False)
    assert (loss, count) == (0.0, 0) and not coef.any()
    got, gu, gv = _run(u, v, lab, ms.MARGIN, rule, False)
    assert got == 0.0 and not gu.any() and (gv is None or not gv.any())


def test_edges_no_negatives_no_positives_one_anchor_and_no_active_triplet():
    c = ms.edge_case(37, 16, 5, 6, signs=True)
    shared = np.ones((37, 1), np.float32)                                          # every row shares a label: no negatives
    _assert_zero(c["u"], c["v"], shared)
    _assert_zero(c["u"], c["u"], shared)
    # single-label rows, all distinct: no positives on the intra-modal call, and none on the cross-modal call either - the reference
    # clears the diagonal of every square mask (train/DPSIH/Loss.py:107-108), so an image's own caption is not its positive
    distinct = np.eye(37, dtype=np.float32)
    _assert_zero(c["u"], c["u"], distinct)
    _assert_zero(c["u"], c["v"], distinct)
    assert ms.msc_loss(c["u"], c["v"], distinct)["count"] == 0
    # one anchor alone has active triplets.  (Eligible ones cannot be one anchor's alone: its positive has it as a positive and its
    # negative as a negative.)  Rows 0 and 1 share a class and the other rows carry no label: they are negatives of both and have no
    # positive.  v_1 = -u_0 puts anchor 0's positive at s = +K, beyond every negative; v_0 = u_1 puts anchor 1's at s = -K, where no
    # negative is within the margin
    lab = np.zeros((37, 1), np.float32)
    lab[:2] = 1.0
    u, v = c["u"].copy(), c["v"].copy()
    v[1], v[0] = -u[0], u[1]
    assert ((u[1] @ v[2:].T) < 16).all()
    r = ms.msc_loss(u, v, lab)
    per_anchor = np.abs(r["coef"]).sum(1)
    assert r["count"] == 35 and per_anchor[0] == 70 and not per_anchor[1:].any()
    _against_restatement(dict(u=u, v=v, lab=lab), "one anchor")
    # semi-hard without an active triplet: u = (+1 .. +1); columns 0-2 lie at s = 0 and columns 3-5 at s = -16, one class each.  Anchors
    # 0-2 see tm = -16 (not > 0), anchors 3-5 see tm = +16 (not <= m = 4); `all` takes the first kind
    u, v = np.ones((6, 16), np.float32), np.ones((6, 16), np.float32)
    v[:3, :8] = -1.0
    lab = ms.group_labels([3, 3])
    _assert_zero(u, v, lab, "semi-hard")
    assert ms.msc_loss(u, v, lab, rule="semi-hard")["count"] == 0
    assert _native(u, v, lab, ms.MARGIN, "all", False)[1] == 18 == ms.msc_loss(u, v, lab)["count"]


def test_exact_ties_at_the_margin_and_at_zero():
    """+-1 codes, no normalisation, margin 4: every tm is an integer.  Triplets at tm == m are counted under both rules and add nothing
    to a coefficient (relu'(0) = 0); triplets at tm == 0 are counted under `all` and not under semi-hard.  All compared as integers."""
    c = ms.tie_case()
    u, v, lab, m = c["u"], c["v"], c["lab"], c["margin"]
    s = -(u.astype(np.int64) @ v.astype(np.int64).T)
    same = (lab @ lab.T > 0) & ~np.eye(len(lab), dtype=bool)
    diff = ~(lab @ lab.T > 0)
    tm = s[:, None, :] - s[:, :, None]                                             # [a, p, n]
    elig = same[:, :, None] & diff[:, None, :]
    at_m, at_0 = int((elig & (tm == 4)).sum()), int((elig & (tm == 0)).sum())
    assert at_m >= 4 and at_0 >= 4
    want_all, want_semi = int((elig & (tm <= 4)).sum()), int((elig & (tm <= 4) & (tm > 0)).sum())
    strict_all, strict_semi = elig & (tm < 4), elig & (tm < 4) & (tm > 0)
    for rule, want, strict in (("all", want_all, strict_all), ("semi-hard", want_semi, strict_semi)):
        loss, count, sim, coef = _native(u, v, lab, m, rule, False)
        assert np.array_equal(sim, s.astype(np.float32))
        assert count == want, (rule, count, want)
        want_coef = np.where(same, strict.sum(2), 0) - np.where(diff, strict.sum(1), 0)
        assert np.array_equal(coef, want_coef), rule
        assert count > int(strict.sum())                                           # the tm == m triplets are in the count alone
        _loss_close(loss, float(np.where(strict, 4 - tm, 0).sum()) / want, ("ties", rule))
    assert want_all - want_semi == int((elig & (tm <= 0)).sum()) >= at_0
    _against_restatement(c, "ties", "semi-hard", False, margin=m)


def test_four_pairs_in_one_call_are_four_single_calls_bit_for_bit():
    import cmh_native as N
    c = ms.edge_case(130, 24, 7, 8)
    for normalize in (False, True):
        hi, ht, lab = tt(c["u"]), tt(c["v"]), tt(c["lab"])
        pairs = [(hi, hi), (ht, ht), (hi, ht), (ht, hi)]
        loss, count, sim, saved = N.msc_triplet_loss(pairs, lab, ms.MARGIN, "all", normalize)
        dl = torch.tensor([1.0, 2.0, 0.5, 3.0], device=DEV)
        grads = N.msc_triplet_loss_backward(saved, dl)
        again = N.msc_triplet_loss(pairs, lab, ms.MARGIN, "all", normalize)
        assert torch.equal(loss, again[0]) and torch.equal(count, again[1]) and torch.equal(sim, again[2]) and torch.equal(saved[1], again[3][1])
        for q, pr in enumerate(pairs):
            l1, c1, s1, saved1 = N.msc_triplet_loss([pr], lab, ms.MARGIN, "all", normalize)
            assert torch.equal(l1[0], loss[q]) and torch.equal(c1[0], count[q]) and torch.equal(s1[0], sim[q]) and torch.equal(saved1[1][0], saved[1][q])
            (du, dv), = N.msc_triplet_loss_backward(saved1, dl[q:q + 1])
            assert torch.equal(du, grads[q][0]) and ((dv is None and grads[q][1] is None) or torch.equal(dv, grads[q][1]))
        assert grads[0][1] is None and grads[2][1] is not None and int(count.min()) > 0


def test_refusals_name_their_entry():
    import cmh_native as N
    from train.MSCH.loss import MSCLoss
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(N.NativeError, match=r"msc_triplet_loss.*1024"):
        MSCLoss()(z(1025, 16), z(1025, 16), z(1025, 2))
    with pytest.raises(N.NativeError, match=r"msc_triplet_loss.*128"):
        MSCLoss()(z(4, 129), z(4, 129), z(4, 2))
    with pytest.raises(N.NativeError, match="msc_triplet_loss"):
        MSCLoss()(z(4, 16), z(5, 16), z(4, 2))                                     # operands of different shapes
    with pytest.raises(N.NativeError, match="msc_triplet_loss"):
        MSCLoss()(z(4, 16), z(4, 16), z(4, 0))
    lib = N.lib()
    arr = N._ptr_array([z(4, 16)])
    assert lib.cmh_msc_triplet_loss(arr, arr, 1, None, 4, 16, 2, 0.25, 0, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"msc_triplet_loss: null pointer" in lib.cmh_last_error()


def _trainer(tmp_path, monkeypatch, *extra):
    import argparse
    import sys
    import recipe
    import main
    import dataset.synthetic as ds
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510)
    monkeypatch.setattr(ds, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16", "--num-workers", "0",
                                      "--resolution", "64", "--max-words", "16", "--query-num", "24", "--train-num", "32",
                                      "--synthetic-size", "120", *extra])
    torch.manual_seed(3)
    return main.trainers["MSCH"](argparse.Namespace(method="MSCH", dataset="synthetic", output_dim=16, is_train=True), 0), ck


def test_one_epoch_checkpoint_loads_as_dsph_and_serves_queries(tmp_path, monkeypatch):
    """Registry -> MSCHTrainer -> one epoch on the synthetic set with the tiny towers; the checkpoint has DSPH's keys and serves the
    trainer's codes through QueryEncoder as MSCH and as DSPH"""
    import cmh_native as N
    from query import QueryEncoder
    tr, ck = _trainer(tmp_path, monkeypatch, "--epochs", "1")
    assert type(tr).__name__ == "MSCHTrainer" and type(tr.model).__name__ == "MMSCH" and tr.global_step == 2
    model_file = tmp_path / "run" / "MSCH" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists()
    state = torch.load(model_file, map_location="cpu")
    from model.DSPH import MDSPH
    dsph = MDSPH(outputDim=16, clipPath=str(ck), saveDir=str(tmp_path / "log"))
    assert set(state) == set(dsph.state_dict())
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    encs = [QueryEncoder(method, str(model_file), str(ck), 16, max_words=16, resolution=64) for method in ("MSCH", "DSPH")]
    for batch in tr.query_loader:
        image, text, index = batch[0].to(DEV), batch[1], batch[-1]
        with torch.no_grad():
            got_i = [enc.rule(enc.model.encode_image(image)) for enc in encs]
        got_t = [enc.encode_tokens(text) for enc in encs]
        assert torch.equal(got_i[0], got_i[1]) and torch.equal(got_t[0], got_t[1])     # one checkpoint under both names: equal codes
        # ... and they are the codes the trainer's model writes for the same batch through the method's rule
        with torch.no_grad():
            want_i, want_t = N.sign_codes(tr.model.encode_image(image)), N.sign_codes(tr.model.encode_text(text.to(DEV)))
        assert torch.equal(got_i[0], want_i) and torch.equal(got_t[0], want_t)
        off_i, off_t = got_i[0] != q_img[index.to(DEV)], got_t[0] != q_txt[index.to(DEV)]
        print(f"against get_code's pipelined loop: {int(off_i.sum())} image and {int(off_t.sum())} text entries of {off_t.numel()} differ")
    # the step's sum is the sum of its three single calls
    image, text, label, index = next(iter(tr.train_loader))
    with torch.no_grad():
        hi, ht = tr.model(image.to(DEV), text.to(DEV))
        lab = label.to(DEV).float()
        total = tr.compute_loss(hi, ht, lab)
        parts = (tr.msc(hi, hi, lab) + tr.msc(ht, ht, lab) + tr.msc(hi, ht, lab)) * 100.0
    assert torch.isfinite(total).item() and abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))


def test_two_steps_change_every_parameter_group_and_stay_finite(tmp_path, monkeypatch):
    tr, _ = _trainer(tmp_path, monkeypatch, "--epochs", "0", "--msc-symmetric", "true", "--msc-mining", "semi-hard")
    assert tr.msc.mining == "semi-hard" and tr.args.msc_symmetric is True
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


def test_msch_training_trajectory_matches_reference(golden):
    """Three steps of the MSCH loop (tape forward -> LinearHash heads -> three-pair loss x 100 -> backward through heads and towers -> fused
    BertAdam) on the tiny CLIP: the loss of every step and the final parameters against the REFERENCE's own run on the CPU
    (tests/golden/make_golden21.py; the heads in eval mode on both sides: no dropout draw)."""
    from types import SimpleNamespace
    import ddbhutil as dd
    import dchmtutil as du
    from model.base.optimization import BertAdam
    from model.modelbase import LinearHash
    from test_gpu_clip import _clip
    from train.MSCH.hash_train import MSCHTrainer
    from train.MSCH.loss import MSCLoss
    g = golden("msch_traj.npz")
    assert float(g["gap_over_err"]) >= 100.0
    clip = _clip(du.CFG, du.SEED, "f32")
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    ih, th = ih.to(DEV), th.to(DEV)
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    me = SimpleNamespace(msc=MSCLoss(), args=SimpleNamespace(msc_symmetric=False, msc_scale=ms.SCALE))
    losses = []
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        loss = MSCHTrainer.compute_loss(me, ih(clip.encode_image(img.to(DEV))), th(clip.encode_text(txt.to(DEV))), lab.to(DEV).float())
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"MSCH trajectory: losses {losses} (reference {g['losses'].tolist()})")
    np.testing.assert_allclose(np.array(losses), g["losses"], rtol=1e-4)
    named = dict(clip.named_parameters())
    named.update({"image_hash." + n: p for n, p in ih.named_parameters()})
    named.update({"text_hash." + n: p for n, p in th.named_parameters()})
    worst = 0.0
    for key in g.files:
        if not key.startswith("p_"):
            continue
        ref = g[key]
        err = np.abs(ms.cut(named[key[2:]].detach().cpu().numpy()) - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err < 1e-4, (key, err)
    print(f"MSCH trajectory: worst parameter error {worst:.2e} of max")
