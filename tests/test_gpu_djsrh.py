"""DJSRH on the GPU (csrc/djsrh.hip through train/DJSRH): the joint-semantics target, the reconstruction loss and its backward against
the float64 restatement of tests/djsrhutil.py at one row, ragged K and D, both sides of the 64-row wave and the 32-row tile edge and
the default batch; the scalar edges; bit-equal repeats; a short SGD trajectory through the autograd function; the trainer end to end
on the tiny synthetic CLIP state.  Tolerances are those tests/test_gpu_ddbh.py holds the sister loss to."""
import numpy as np
import pytest
import torch

import djsrhutil as dj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
_REF = {}


def _loss_close(got, want, what):
    print(f"{what}: got {got!r}, want {want!r}")
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (what, got, want)


def _mat_close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    print(f"{what}: max |diff| {np.abs(got.cpu().numpy() - ref).max():.3e} of max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=str(what))


def _reference(B, K, D, scalars=dj.SCALARS, zero_row=None):
    """the case and its float64 target, loss and gradients (at dloss = 2), computed once per (shape, scalars) and never written to"""
    key = (B, K, D, scalars, zero_row)
    if key not in _REF:
        c = dj.case(B, K, D)
        if zero_row is not None:
            c["fi"][zero_row] = 0.0
            c["ft"][zero_row] = 0.0
        beta, eta, mu, l1, l2 = scalars
        S = dj.target(c["fi"], c["ft"], beta, eta, mu)
        _REF[key] = dict(c, S=S, **dj.loss(c["hi"], c["ht"], S.astype(np.float32), l1, l2, dloss=2.0))
    return _REF[key]


def _run(r, scalars=dj.SCALARS, scale=2.0):
    """target, then loss with (scale * loss).backward() -> S, loss, terms, d_hi, d_ht; the no_grad value is the differentiable one"""
    from train.DJSRH.loss import JointSemanticsLoss
    jsl = JointSemanticsLoss(*scalars)
    S = jsl.target(tt(r["fi"]), tt(r["ft"]))
    hi, ht = tt(r["hi"]).requires_grad_(), tt(r["ht"]).requires_grad_()
    with torch.no_grad():
        plain, plain_terms = jsl.terms(hi, ht, S)
    loss, terms = jsl.terms(hi, ht, S)
    assert loss.dim() == 0 and torch.equal(plain, loss.detach()) and torch.equal(plain_terms, terms) and not terms.requires_grad
    (scale * loss).backward()
    return S, loss.detach(), terms, hi.grad, ht.grad


def _check(r, scalars, what):
    l1, l2 = scalars[3:]
    S, loss, terms, gi, gt = _run(r, scalars)
    _mat_close(S, r["S"], (what, "S"))
    assert torch.equal(S, S.T)                                                    # symmetric bit for bit
    # the loss against the restatement on the SAME f32 target the kernel read (r's loss is on the float64 target rounded once)
    want = dj.loss(r["hi"], r["ht"], S.cpu().numpy(), l1, l2, dloss=2.0)
    _loss_close(float(loss), want["loss"], (what, "loss"))
    for k, name in enumerate(("II", "IT", "TT")):
        _loss_close(float(terms[k]), want["terms"][k], (what, name))
        _loss_close(float(terms[k]), r["terms"][k], (what, name, "float64 target"))
    _loss_close(float(loss), r["loss"], (what, "loss", "float64 target"))
    _mat_close(gi, r["gi"], (what, "d_hi"))
    _mat_close(gt, r["gt"], (what, "d_ht"))


@pytest.mark.parametrize("B,K,D", dj.GPU_SHAPES)
def test_target_loss_and_gradients_match_the_restatement(B, K, D):
    _check(_reference(B, K, D), dj.SCALARS, (B, K, D))


@pytest.mark.parametrize("name,scalars", [("beta0", (0.0, 0.4, 1.5, 0.1, 0.1)), ("beta1", (1.0, 0.4, 1.5, 0.1, 0.1)),
                                          ("eta0", (0.9, 0.0, 1.5, 0.1, 0.1))])
def test_scalar_edges(name, scalars):
    """beta = 0 / 1: one modality alone makes the target; eta = 0: no second-order term (S = mu St)"""
    _check(_reference(65, 64, 100, scalars), scalars, name)


def test_one_zero_feature_row_forward():
    from train.DJSRH.loss import JointSemanticsLoss
    r = _reference(65, 64, 100, zero_row=33)
    S = JointSemanticsLoss().target(tt(r["fi"]), tt(r["ft"]))
    assert bool(torch.isfinite(S).all()) and torch.equal(S, S.T)
    _mat_close(S, r["S"], "zero row S")
    only = JointSemanticsLoss(eta=0.0, mu=1.0).target(tt(r["fi"]), tt(r["ft"]))   # St itself
    assert bool((only[33] == -1.0).all()) and bool((only[:, 33] == -1.0).all())
    loss, terms = JointSemanticsLoss().terms(tt(r["hi"]), tt(r["ht"]), S)
    _loss_close(float(loss), r["loss"], "zero row loss")


def test_two_calls_are_bit_equal_and_dloss_scales_exactly():
    r = _reference(300, 64, 512)
    a, b = _run(r), _run(r)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    q = _run(r, scale=0.25)
    one = _run(r, scale=1.0)
    assert torch.equal(q[3], 0.25 * one[3]) and torch.equal(q[4], 0.25 * one[4])  # a power of two: the same bits, scaled
    assert float(one[3].abs().max()) > 0.0


def test_no_gradient_reaches_the_target_or_the_features():
    from train.DJSRH.loss import JointSemanticsLoss
    r = _reference(65, 64, 100)
    jsl = JointSemanticsLoss()
    fi, ft = tt(r["fi"]).requires_grad_(), tt(r["ft"]).requires_grad_()
    S = jsl.target(fi, ft)
    assert not S.requires_grad
    S = S.clone().requires_grad_()
    hi, ht = tt(r["hi"]).requires_grad_(), tt(r["ht"]).requires_grad_()
    jsl(hi, ht, S).backward()
    assert S.grad is None and fi.grad is None and ft.grad is None and hi.grad is not None and ht.grad is not None


def test_sgd_trajectory_through_the_autograd_function():
    """Five plain-SGD steps (lr 0.5) on leaf tensors, losses against the restatement's float64 trajectory on the same f32 target"""
    from train.DJSRH.loss import JointSemanticsLoss
    r = _reference(65, 24, 40)
    jsl = JointSemanticsLoss()
    S = jsl.target(tt(r["fi"]), tt(r["ft"]))
    want = dj.sgd_losses(r["hi"], r["ht"], S.cpu().numpy(), 0.1, 0.1, steps=5, lr=0.5)
    hi, ht = tt(r["hi"]).requires_grad_(), tt(r["ht"]).requires_grad_()
    got = []
    for _ in range(5):
        loss = jsl(hi, ht, S)
        got.append(float(loss.detach()))
        hi.grad = ht.grad = None
        loss.backward()
        with torch.no_grad():
            hi -= 0.5 * hi.grad
            ht -= 0.5 * ht.grad
    print(f"losses {got} (float64 {want.tolist()})")
    np.testing.assert_allclose(np.array(got), want, rtol=1e-4)
    assert want[-1] < want[0]


def test_refusals_name_their_entry():
    import cmh_native as N
    from train.DJSRH.loss import JointSemanticsLoss
    z = lambda *s: torch.zeros(*s, device=DEV)
    jsl = JointSemanticsLoss()
    with pytest.raises(N.NativeError, match=r"djsrh_target.*1024"):
        jsl.target(z(1025, 8), z(1025, 8))
    with pytest.raises(N.NativeError, match=r"djsrh_target.*4096"):
        jsl.target(z(4, 4097), z(4, 4097))
    with pytest.raises(N.NativeError, match=r"djsrh_loss.*128"):
        jsl(z(4, 129), z(4, 129), z(4, 4))
    with pytest.raises(N.NativeError, match="djsrh_loss"):
        jsl(z(4, 16), z(5, 16), z(4, 4))                                           # operands of different shapes
    with pytest.raises(N.NativeError, match="djsrh_loss"):
        jsl(z(4, 16), z(4, 16), z(4, 5))


# ---------------------------------------------------------------------------------------------------- the trainer
def _trainer(tmp_path, monkeypatch, *extra):
    import argparse
    import sys
    import recipe
    import main
    import dataset.synthetic as ds
    ck = tmp_path / "clip.pt"
    if not ck.exists():
        torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510)
    monkeypatch.setattr(ds, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16", "--num-workers", "0",
                                      "--resolution", "64", "--max-words", "16", "--query-num", "24", "--train-num", "32",
                                      "--synthetic-size", "120", *extra])
    torch.manual_seed(3)
    return main.trainers["DJSRH"](argparse.Namespace(method="DJSRH", dataset="synthetic", output_dim=16, is_train=True), 0), ck


def test_target_cache_rows_are_the_stock_features(tmp_path, monkeypatch):
    """--epochs 0: the cache alone.  One row per train item; the rows a batch's `index` names are the towers' features of that batch
    (f32 rounding apart: the batch was composed differently when the cache was filled)."""
    tr, _ = _trainer(tmp_path, monkeypatch, "--epochs", "0")
    assert type(tr).__name__ == "DJSRHTrainer" and type(tr.model).__name__ == "MDJSRH"
    n = len(tr.train_loader.dataset)
    assert n == 32 and tuple(tr.cache_i.shape) == tuple(tr.cache_t.shape) == (n, tr.model.embedDim) and tr.cache_i.dtype == torch.float32
    tr.change_state(mode="valid")
    seen = 0
    for image, text, label, index in tr.train_loader:
        with torch.no_grad():
            fi, ft = tr.model.clip.encode_image(image.to(DEV)).float(), tr.model.clip.encode_text(text.to(DEV)).float()
        for got, want in ((tr.cache_i[index.to(DEV)], fi), (tr.cache_t[index.to(DEV)], ft)):
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
        seen += index.numel()
    assert seen == n and float(tr.cache_i.std(0).mean()) > 0.0


def test_one_epoch_checkpoint_loads_as_dsph_and_serves_queries(tmp_path, monkeypatch):
    from query import QueryEncoder
    tr, ck = _trainer(tmp_path, monkeypatch, "--epochs", "1")
    model_file = tmp_path / "run" / "DJSRH" / "synthetic" / "16" / "model-0.pth"
    assert model_file.exists() and tr.global_step == 2
    state = torch.load(model_file, map_location="cpu")
    assert {"image_hash.fc.weight", "image_hash.fc.bias", "text_hash.fc.weight", "text_hash.fc.bias"} <= set(state)
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for method in ("DJSRH", "DSPH"):
        enc = QueryEncoder(method, str(model_file), str(ck), 16, max_words=16, resolution=64)
        for batch in tr.query_loader:
            image, text, index = batch[0].to(DEV), batch[1], batch[-1]
            with torch.no_grad():
                got_i = enc.rule(enc.model.encode_image(image))
            assert torch.equal(got_i, q_img[index.to(DEV)]) and torch.equal(enc.encode_tokens(text), q_txt[index.to(DEV)])


def test_init_heads_cca_gives_the_itq_fit_on_the_cached_features(tmp_path, monkeypatch):
    """--init-heads cca --epochs 0: the heads are what `--method ITQ --projection cca` fits on the same features, so are the codes"""
    import cmh_native as N
    from utils.itq import fit_hash_heads
    tr, _ = _trainer(tmp_path, monkeypatch, "--epochs", "0", "--init-heads", "cca")
    fit = fit_hash_heads(tr.cache_i, tr.cache_t, 16, "cca", "itq", seed=tr.args.seed)
    for side, head in (("i", tr.model.image_hash), ("t", tr.model.text_hash)):
        assert torch.equal(head.fc.weight.detach(), fit[f"W_{side}"]) and torch.equal(head.fc.bias.detach(), fit[f"b_{side}"])
    tr.change_state(mode="valid")
    with torch.no_grad():
        for feats, head, side in ((tr.cache_i, tr.model.image_hash, "i"), (tr.cache_t, tr.model.text_hash, "t")):
            want = N.sign_codes(N.linear_act(feats, fit[f"W_{side}"], fit[f"b_{side}"], N.ACT_TANH, None, 0.0))
            assert torch.equal(N.sign_codes(head(feats)), want) and len({tuple(row) for row in want.tolist()}) > 1
