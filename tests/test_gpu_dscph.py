"""DScPH on the GPU (csrc/cpf.hip through train/DScPH): the proxy-fusion loss, the two quantisation terms and the three gradients
against the REFERENCE's own values and autograd gradients (tests/golden/make_golden22.py); at the kernel's edges against the float64
restatement of tests/dscphutil.py DECIDING ON THE KERNEL'S OWN cosines (larger shapes always hold a cosine near a threshold), with the
cosines themselves held to float64 within their worst-case float32 bound; bit-equality; refusals; the trainer end to end, a three-step
training trajectory against the reference's, and the query front end.  Tolerances are those of tests/test_gpu_djsrh.py /
tests/test_gpu_ddbh.py: rtol 2e-4, atol 2e-5 of the reference's maximum.

How the masks are compared exactly.  The kernel writes no mask: it decides on the `cos` it writes, and the restatement is handed that
array.  The number of negatives above tau per modality is read back as an integer (psi = -2^20 and sn = 0 turn ln into 2^20 times that
count plus less than one), and every coefficient of a wrongly decided element would move a gradient row by about its maximum."""
import numpy as np
import pytest
import torch

import dscphutil as ds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, CHUNK, SLICE = 16, 64, 256                  # asserted below to be csrc/cpf.hip's kCpfRows, kCpfChunk, kCpfSlice
TAGS = [f"B{B}_K{K}_C{Cn}" for B, K, Cn, _ in ds.CASES] + list(ds.SPECIALS)
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _close(got, ref, what):
    got, ref = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    print(f"{what}: max |diff| {np.abs(got - ref).max():.3e} of max |ref| {top:.3e}")
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-5 * top, err_msg=str(what))


def _module(c, scalars=None, qw=1.0):
    from train.DScPH.loss import CPFLoss
    fn = CPFLoss(c["W"].shape[1], c["W"].shape[0], quant_weight=qw, **dict(ds.SCALARS, **(scalars or {}))).to(DEV)
    fn.weight.data.copy_(tt(c["W"]))
    return fn


def _run(c, scalars=None, qw=1.0, scale=1.0, lab=None):
    """CPFLoss on the case with (scale * loss).backward(), twice -> loss, terms [4], (d hi, d ht, d W); asserts that the no_grad value is
    the differentiable one bit for bit, that the second run has the first's bits and that no input was written"""
    fn = _module(c, scalars, qw)
    y = tt(c["lab"] if lab is None else lab)
    out = []
    for _ in range(2):
        a, b = tt(c["hi"]).requires_grad_(), tt(c["ht"]).requires_grad_()
        fn.weight.grad = None
        with torch.no_grad():
            plain, plain_terms = fn.step_terms(a, b, y)
        loss, terms = fn.step_terms(a, b, y)
        assert plain.dim() == 0 and torch.equal(plain, loss.detach()) and torch.equal(plain_terms, terms) and not terms.requires_grad
        (scale * loss).backward()
        out.append((loss.detach().clone(), terms.clone(), a.grad, b.grad, fn.weight.grad.clone()))
        assert torch.equal(a.detach(), tt(c["hi"])) and torch.equal(b.detach(), tt(c["ht"])) and torch.equal(fn.weight.detach(), tt(c["W"]))
        assert torch.equal(y, tt(c["lab"] if lab is None else lab))
    assert all(torch.equal(x, z) for x, z in zip(out[0], out[1]))
    return float(out[0][0]), out[0][1].cpu().numpy().astype(np.float64), out[0][2:]


def _native(c, scalars=None, qw=1.0):
    """one forward through the wrapper with a tape -> loss, terms, cos [2, B, C] (numpy), the six f64 sums of the tape"""
    import cmh_native as N
    loss, terms, cos, saved = N.cpf_loss(tt(c["hi"]), tt(c["ht"]), tt(c["lab"]), tt(c["W"]), scalars, qw, keep=True)
    sums = saved[2][:12].view(torch.float64).cpu().numpy()
    return float(loss[0]), terms.cpu().numpy().astype(np.float64), cos.cpu().numpy(), sums


def _against_restatement(c, what, grads=True):
    """the kernel against the restatement deciding on the kernel's own cos -> the restatement's result"""
    loss, terms, cos, sums = _native(c)
    B, K = c["hi"].shape
    exact = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"])
    bound = (K + 6) * 2.0 ** -24                 # K rounded partial sums of magnitude <= 1 and three roundings per unit element
    print(f"{what}: max |cos - float64 cos| {np.abs(cos - exact['cos']).max():.3e} (bound {bound:.3e})")
    assert cos.dtype == np.float32 and np.abs(cos - exact["cos"]).max() <= bound, what
    r = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"], cos=cos)
    # the negatives above tau, as integers: ln = sum (c + 2^20) over them
    counted = _native(c, dict(psi=-2.0 ** 20, sn=0.0))[3]
    for m in range(2):
        want = int((r["above"][m] & (c["lab"] == 0)).sum())
        assert int(round(counted[3 * m + 2] / 2.0 ** 20)) == want, (what, m, counted[3 * m + 2] / 2.0 ** 20, want)
    _close(terms, np.concatenate([r["L"], r["q"]]), (what, "terms"))
    _close(np.array([loss]), np.array([r["step"]]), (what, "loss"))
    if grads:
        got, got_terms, g = _run(c, scale=2.0)
        assert got == loss and np.array_equal(got_terms, terms)
        for name, mine, ref in zip(("d hi", "d ht", "d W"), g, r["g_step"]):
            _close(mine, 2.0 * ref, (what, name))
    return r


def test_the_tests_constants_are_the_kernels():
    import cmh_native as N
    assert (ROWS, CHUNK, SLICE) == (N.CPF_ROWS, N.CPF_CHUNK, N.CPF_SLICE)          # (tests/test_dscph_host.py ties those to csrc/cpf.hip)


@pytest.mark.parametrize("tag", TAGS)
def test_loss_terms_and_gradients_match_reference(golden, tag):
    g = golden("dscph.npz")
    c = {x["tag"]: x for x in ds.all_cases()}[tag]
    # the CPF part alone (quant_weight 0), then the whole step
    loss, terms, grads = _run(c, qw=0.0, scale=2.0)
    _close(np.array([loss]), np.array([float(g[f"{tag}_cpf"])]), (tag, "cpf"))
    _close(np.array([terms[0] + terms[1]]), np.array([float(g[f"{tag}_cpf"])]), (tag, "L_img + L_txt"))
    _close(terms[2:], np.array([float(g[f"{tag}_q_img"]), float(g[f"{tag}_q_txt"])]), (tag, "q"))
    for name, mine, key in zip(("gi", "gt", "gw"), grads, ("cpf_gi", "cpf_gt", "cpf_gw")):
        _close(mine, 2.0 * g[f"{tag}_{key}"].astype(np.float64), (tag, "cpf", name))
    loss, terms, grads = _run(c, scale=2.0)
    _close(np.array([loss]), np.array([float(g[f"{tag}_step"])]), (tag, "step"))
    _close(grads[0], 2.0 * ds.step_grad(g, tag, "gi"), (tag, "step gi"))
    _close(grads[1], 2.0 * ds.step_grad(g, tag, "gt"), (tag, "step gt"))
    _close(grads[2], 2.0 * g[f"{tag}_cpf_gw"].astype(np.float64), (tag, "step gw"))
    # the q terms' gradient against ITS OWN maximum (about 1e-3 of the CPF gradient): with no label and no cosine above tau = 2 the CPF
    # coefficients are exactly zero (lp = ln = 0), and the q terms see neither labels nor proxies
    loss, terms, grads = _run(c, dict(tau=2.0), lab=np.zeros_like(c["lab"]))
    assert terms[0] == 0.0 and terms[1] == 0.0 and not grads[2].any()
    _close(grads[0], g[f"{tag}_q_gi"].astype(np.float64), (tag, "q gi"))
    _close(grads[1], g[f"{tag}_q_gt"].astype(np.float64), (tag, "q gt"))


@pytest.mark.parametrize("B", [1, 2, ROWS - 1, ROWS, ROWS + 1, SLICE - 1, SLICE, SLICE + 1, 1024])
def test_edges_batch_sizes(B):
    """the row blocks of 16 (forward and backward), the d_proxies slices of 256 batch rows, and the limit"""
    r = _against_restatement(ds.edge_case(B, 24, 7, 3), f"B{B}")
    assert B < ROWS or (r["above"].any() and not r["above"].all())


@pytest.mark.parametrize("K", [1, 31, 32, 33, 63, 64, 65, 127, 128])
def test_edges_code_widths(K):
    """the staging rounds of 32 columns, the second column per lane of the normaliser's finish (K = 65), and the limit"""
    _against_restatement(ds.edge_case(37, K, 9, 4), f"K{K}")


@pytest.mark.parametrize("B,C", [(19, 1), (19, CHUNK - 1), (19, CHUNK), (19, CHUNK + 1), (5, SLICE - 1), (5, SLICE), (5, SLICE + 1), (5, 1024)])
def test_edges_class_counts(B, C):
    """the staged proxy tiles of 64 classes (forward), the d_hi / d_ht slices of 256 classes, the 16-class blocks of d_proxies, the limit"""
    _against_restatement(ds.edge_case(B, 16, C, 5, p=0.05), f"B{B} C{C}")


def test_zero_row_forward_only():
    """an all-zero h row: unit row 0 (x / 1e-12), cosines 0 on that row, sigma = 0.5; the gradient is g / 1e-12 in the reference too and
    is not pinned"""
    c = ds.edge_case(9, 16, 5, 6)
    c["hi"][3] = 0.0
    c["lab"][3, 1] = 1.0
    r = _against_restatement(c, "zero row", grads=False)
    assert not r["cos"][0, 3].any() and r["pos"][0, 3].all()
    fn = _module(c)
    with torch.no_grad():
        assert torch.isfinite(fn(tt(c["hi"]), tt(c["ht"]), tt(c["lab"]))).item()


def test_forward_only_bit_equality_and_dloss_scaling():
    import cmh_native as N
    c = ds.edge_case(130, 65, 21, 8)
    hi, ht, lab, W = tt(c["hi"]), tt(c["ht"]), tt(c["lab"]), tt(c["W"])
    before = [x.clone() for x in (hi, ht, lab, W)]
    loss, terms, cos, saved = N.cpf_loss(hi, ht, lab, W, keep=True)
    plain = N.cpf_loss(hi, ht, lab, W)                                            # no tape: the unit rows live in the workspace
    assert plain[3] is None and torch.equal(plain[0], loss) and torch.equal(plain[1], terms) and torch.equal(plain[2], cos)
    view = torch.full((2, 130, 21), float("nan"), device=DEV)
    assert N.cpf_loss(hi, ht, lab, W, cos=view)[2] is view and torch.equal(view, cos)
    one = torch.ones(1, device=DEV)
    g1 = N.cpf_loss_backward(saved, one)
    g1b = N.cpf_loss_backward(saved, one)
    again = N.cpf_loss(hi, ht, lab, W, keep=True)
    g1c = N.cpf_loss_backward(again[3], one)
    bits = lambda tape: torch.cat([tape[:12], tape[16:]]).view(torch.int32)       # (floats 12 .. 15 pad the six f64 sums and are not written)
    assert torch.equal(again[0], loss) and torch.equal(bits(again[3][2]), bits(saved[2]))
    for a, b, d in zip(g1, g1b, g1c):
        assert torch.equal(a, b) and torch.equal(a, d)                             # d_proxies included: fixed order, no atomics
    g4 = N.cpf_loss_backward(saved, 4.0 * one)                                     # a power of two scales every rounding with it
    for a, b in zip(g1, g4):
        assert torch.equal(4.0 * a, b) and bool(a.any())
    g3 = N.cpf_loss_backward(saved, 3.0 * one)
    for a, b in zip(g1, g3):
        _close(b, 3.0 * a.cpu().numpy().astype(np.float64), "dloss 3")
    assert all(torch.equal(x, y) for x, y in zip((hi, ht, lab, W), before))


def test_refusals_name_their_entry():
    import cmh_native as N
    from train.DScPH.loss import CPFLoss
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(N.NativeError, match=r"cpf_loss.*128"):
        CPFLoss(129, 2).to(DEV)(z(4, 129), z(4, 129), z(4, 2))
    with pytest.raises(N.NativeError, match=r"cpf_loss.*1024"):
        CPFLoss(16, 2).to(DEV)(z(1025, 16), z(1025, 16), z(1025, 2))
    with pytest.raises(N.NativeError, match="cpf_loss"):
        CPFLoss(16, 2).to(DEV)(z(0, 16), z(0, 16), z(0, 2))
    with pytest.raises(N.NativeError, match="cpf_loss"):
        N.cpf_loss(z(4, 16), z(4, 16), z(4, 0), z(0, 16))
    with pytest.raises(N.NativeError, match="cpf_loss"):
        CPFLoss(16, 2).to(DEV)(z(4, 16), z(5, 16), z(4, 2))                        # operands of different shapes
    lib = N.lib()
    hi, lab, W, out, cos = z(4, 16), z(4, 2), z(2, 16), torch.full((8,), 7.0, device=DEV), z(2, 4, 2)
    ws = N.workspace(lib.cmh_cpf_workspace_bytes(4, 16, 2), hi.device, "loss")
    call = lambda B=4, K=16, Cn=2, a=hi, n=ws.numel(), w=ws: lib.cmh_cpf_loss(
        N.ptr(a), N.ptr(hi), N.ptr(lab), N.ptr(W), B, K, Cn, 0.9, 0.7, 1.3, 1.3, 1.0, 2.0, 1.0, N.ptr(out), N.ptr(out[4:]), N.ptr(cos), None,
        N.ptr(w), n, None)
    for kw, word in ((dict(K=129), b"K=129"), (dict(B=0), b"B=0"), (dict(B=1025), b"B=1025"), (dict(Cn=0), b"C=0"),
                     (dict(n=lib.cmh_cpf_workspace_bytes(4, 16, 2) - 1), b"workspace too small"), (dict(a=None), b"null pointer"),
                     (dict(w=None), b"null workspace")):
        assert call(**kw) == -1, kw
        msg = lib.cmh_last_error()
        assert msg.startswith(b"cpf_loss:") and word in msg, (kw, msg)
    assert lib.cmh_cpf_loss_backward(N.ptr(lab), N.ptr(cos), None, 4, 16, 2, 0.9, 1.3, 1.3, 1.0, 1.0, N.ptr(out), N.ptr(hi), N.ptr(hi), N.ptr(W),
                                     None) == -1 and b"cpf_loss_backward: null pointer" in lib.cmh_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                # nothing was launched


def _trainer(tmp_path, monkeypatch, *extra):
    import argparse
    import sys
    import recipe
    import main
    import dataset.synthetic as dsy
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(dsy, "SOT", 510)
    monkeypatch.setattr(dsy, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16", "--num-workers", "0",
                                      "--resolution", "64", "--max-words", "16", "--query-num", "24", "--train-num", "32",
                                      "--synthetic-size", "120", *extra])
    torch.manual_seed(3)
    return main.trainers["CPFH"](argparse.Namespace(method="CPFH", dataset="synthetic", output_dim=16, is_train=True), 0), ck


def test_one_epoch_checkpoint_loads_as_dsph_and_serves_queries(tmp_path, monkeypatch):
    """Registry -> DScPHTrainer -> one epoch on the synthetic set with the tiny towers; the checkpoint has DSPH's keys (no proxies) and
    serves the trainer's codes through QueryEncoder as CPFH and as DSPH.

    What "the trainer's codes" are.  A model is built with the towers' GEMM weights in float16 until `.float()` (the reference's
    convert_weights), and QueryEncoder - like every trainer's `--pretrained` - loads the state BEFORE `.float()`: a loaded checkpoint
    holds those weights rounded to float16, while the trainer that wrote it went on from float32 values.  With the in-memory float32
    weights one text output of the first query batch lies at +0.0150 where the loaded model gives -0.0191 (largest output difference
    4.0e-2 on these random tiny towers; measured, each model repeatable bit for bit), so one code entry of 256 differs.  The test
    therefore states the rounding exactly - every loaded tensor equals the trainer's, through float16 where the loader stores float16 -
    and then asks the trainer's OWN model object, holding those rounded weights, for the very codes QueryEncoder gives."""
    import cmh_native as N
    from query import QueryEncoder
    tr, ck = _trainer(tmp_path, monkeypatch, "--epochs", "1")
    assert type(tr).__name__ == "DScPHTrainer" and type(tr.model).__name__ == "MDScPH" and tr.global_step == 2
    assert len(tr.optimizer.param_groups) == 4 and tr.optimizer.param_groups[3]["params"][0] is tr.cpf.weight
    assert tr.cpf.weight.shape == (tr.args.nclass, 16) and tr.cpf.weight.is_cuda
    model_file = tmp_path / "run" / "CPFH" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists()
    state = torch.load(model_file, map_location="cpu")
    from model.DSPH import MDSPH
    dsph = MDSPH(outputDim=16, clipPath=str(ck), saveDir=str(tmp_path / "log"))
    assert set(state) == set(dsph.state_dict())
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters()) and bool(torch.isfinite(tr.cpf.weight).all())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    encs = [QueryEncoder(method, str(model_file), str(ck), 16, max_words=16, resolution=64) for method in ("CPFH", "DSPH")]
    half = {k for k, v in dsph.state_dict().items() if v.dtype == torch.float16}
    own = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    assert half and all(k.startswith("clip.") for k in half)
    for k, v in encs[0].model.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, (own[k].half().float() if k in half else own[k]).to(v.device)), k
    off_grid = sum(int((own[k] != own[k].half().float()).sum()) for k in half)
    image, text = next(iter(tr.query_loader))[:2]
    with torch.no_grad():
        before = N.sign_codes(tr.model.encode_text(text.to(DEV)))
    print(f"{off_grid} tower weights of the trainer lie off the float16 grid; with them {int((before != encs[0].encode_tokens(text)).sum())} "
          f"text code entries of {before.numel()} differ from the loaded checkpoint's")
    with torch.no_grad():
        for k, p in tr.model.named_parameters():
            if k in half:
                p.copy_(p.half().float())
    for batch in tr.query_loader:
        image, text = batch[0].to(DEV), batch[1]
        with torch.no_grad():
            got_i = [enc.rule(enc.model.encode_image(image)) for enc in encs]
        got_t = [enc.encode_tokens(text) for enc in encs]
        assert torch.equal(got_i[0], got_i[1]) and torch.equal(got_t[0], got_t[1])     # one checkpoint under both names: equal codes
        with torch.no_grad():
            want_i, want_t = N.sign_codes(tr.model.encode_image(image)), N.sign_codes(tr.model.encode_text(text.to(DEV)))
        assert torch.equal(got_i[0], want_i) and torch.equal(got_t[0], want_t)
    # the step's sum is its four terms
    image, text, label, index = next(iter(tr.train_loader))
    with torch.no_grad():
        hi, ht = tr.model(image.to(DEV), text.to(DEV))
        total, part = tr.compute_loss(hi, ht, label.to(DEV).float())
        terms = tr.cpf.terms(hi, ht, label.to(DEV).float())
    assert torch.isfinite(total).item() and float(part) == float(terms[0] + terms[1])
    assert abs(float(total) - float(terms.double().sum())) <= 1e-6 * abs(float(total))


def test_two_steps_move_every_group_the_proxies_included(tmp_path, monkeypatch):
    tr, _ = _trainer(tmp_path, monkeypatch, "--epochs", "0", "--cpf-tau", "0.5", "--quant-weight", "0.5")
    assert tr.cpf.scalars["tau"] == 0.5 and tr.cpf.quant_weight == 0.5
    tr.change_state(mode="train")
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = 4
    before = [[p.detach().clone() for p in grp["params"]] for grp in tr.optimizer.param_groups]
    for image, text, label, index in list(tr.train_loader)[:2]:
        assert torch.isfinite(tr._step(image, text, label)).item()
    assert len(before) == 4
    for grp, old in zip(tr.optimizer.param_groups, before):
        assert any(not torch.equal(p.detach(), o) for p, o in zip(grp["params"], old))
    assert not torch.equal(tr.cpf.weight.detach(), before[3][0])                   # the proxies moved
    assert all(torch.isfinite(p).all() for p in tr.model.parameters()) and bool(torch.isfinite(tr.cpf.weight).all())


def test_dscph_training_trajectory_matches_reference(golden):
    """Three steps of the DScPH loop (tape forward -> LinearHash heads -> CPF + the two q terms -> backward through heads and towers ->
    fused BertAdam over FOUR groups) on the tiny CLIP: the CPF loss and the sum of every step, the final parameters and the final
    proxies against the REFERENCE's own run on the CPU (tests/golden/make_golden22.py; the heads in eval mode on both sides)."""
    from types import SimpleNamespace
    import ddbhutil as dd
    import dchmtutil as du
    import mschutil as ms
    from model.base.optimization import BertAdam
    from model.modelbase import LinearHash
    from test_gpu_clip import _clip
    from train.DScPH.hash_train import DScPHTrainer
    from train.DScPH.loss import CPFLoss
    g = golden("dscph_traj.npz")
    assert float(g["gap_over_err"]) >= 100.0
    clip = _clip(du.CFG, du.SEED, "f32")
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    ih, th = ih.to(DEV), th.to(DEV)
    cpf = CPFLoss(dd.TRAJ_K, du.C).to(DEV)
    cpf.weight.data.copy_(tt(ds.traj_proxies()))
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}, {"params": cpf.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    me = SimpleNamespace(cpf=cpf)
    losses, totals = [], []
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        total, part = DScPHTrainer.compute_loss(me, ih(clip.encode_image(img.to(DEV))), th(clip.encode_text(txt.to(DEV))), lab.to(DEV).float())
        losses.append(float(part.detach()))
        totals.append(float(total.detach()))
        opt.zero_grad()
        total.backward()
        opt.step()
    print(f"DScPH trajectory: losses {losses} (reference {g['losses'].tolist()}), sums {totals} (reference {g['totals'].tolist()})")
    np.testing.assert_allclose(np.array(losses), g["losses"], rtol=1e-4)
    np.testing.assert_allclose(np.array(totals), g["totals"], rtol=1e-4)
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
    err = np.abs(cpf.weight.detach().cpu().numpy() - g["proxies"]).max() / np.abs(g["proxies"]).max()
    print(f"DScPH trajectory: worst parameter error {worst:.2e} of max, proxies {err:.2e}")
    assert err < 1e-4 and np.abs(g["proxies"] - ds.traj_proxies()).max() > 1e-4       # ... and the reference's proxies moved
