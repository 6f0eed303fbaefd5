"""encode_image / encode_text on the GPU (C ABI cmh_vit_encode / cmh_text_encode, through the
reference-shaped CLIP module) vs the goldens produced by the reference and vs the oracle."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _clip(cfg, seed, mode, fp16_roundtrip=False):
    from model.base.model import CLIP
    m = CLIP(cfg["embed_dim"], cfg["image_resolution"], cfg["vision_layers"], cfg["vision_width"],
             cfg["vision_patch_size"], cfg["context_length"], cfg["vocab_size"], cfg["transformer_width"],
             cfg["transformer_heads"], cfg["transformer_layers"])
    sd = {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, seed, fp16_roundtrip).items()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).float().set_gemm_dtype(mode)


def test_tiny_f32_matches_reference_goldens_with_taps(golden):
    g = golden("clip_tiny.npz")
    cfg, seed = recipe.CLIP_TINY, int(g["seed"])
    m = _clip(cfg, seed, "f32")
    B, T, d = 3, 5, cfg["vision_width"]
    taps = [torch.empty(B * T, d, device=DEV) for _ in range(1 + cfg["vision_layers"])]
    img = m.encode_image(torch.from_numpy(recipe.images(B, cfg["image_resolution"], seed)).to(DEV), taps=taps)
    tol = dict(rtol=1e-4, atol=1e-4)          # north_star: floats within 1e-4
    np.testing.assert_allclose(taps[0].cpu().numpy().reshape(B, T, d), g["v_ln_pre"], **tol)
    for i in range(cfg["vision_layers"]):
        np.testing.assert_allclose(taps[1 + i].cpu().numpy().reshape(B, T, d), g[f"v_block{i}"], **tol)
    np.testing.assert_allclose(img.detach().cpu().numpy(), g["img_feat"], **tol)
    for L, s in ((16, seed), (9, seed + 1)):
        tw = cfg["transformer_width"]
        taps = [None] + [torch.empty(B * L, tw, device=DEV) for _ in range(cfg["transformer_layers"])]
        txt = m.encode_text(torch.from_numpy(recipe.captions(B, L, cfg["vocab_size"], s)).to(DEV), taps=taps)
        for i in range(cfg["transformer_layers"]):
            np.testing.assert_allclose(taps[1 + i].cpu().numpy().reshape(B, L, tw), g[f"t_block{i}_L{L}"], **tol)
        np.testing.assert_allclose(txt.detach().cpu().numpy(), g[f"txt_feat_L{L}"], **tol)


def test_vitb32_f32_matches_reference_goldens(golden):
    g = golden("clip_vitb32.npz")
    cfg, seed = recipe.CLIP_VITB32, int(g["seed"])
    m = _clip(cfg, seed, "f32")
    rows = g["v_rows"]
    taps = [torch.empty(2 * 50, 768, device=DEV) for _ in range(13)]
    img = m.encode_image(torch.from_numpy(recipe.images(2, 224, seed)).to(DEV), taps=taps)
    # north_star's tolerance (1e-4) at full size, with the measured error behind it: on MI355X the largest |difference| to the
    # reference's own outputs is 1.0e-5 at any tap (values up to 4.9; 8.8e-6 after block 11, 3.8e-6 / 7.5e-6 on the image / text
    # features), so |d| <= 2e-5 + 1e-4 |ref| holds with a margin of four (round 2 allowed 2e-4 + 1e-3 |ref| here)
    tol = dict(rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(taps[0].cpu().numpy().reshape(2, 50, 768)[:, rows], g["v_ln_pre_rows"], **tol)
    for i in (0, 5, 11):
        np.testing.assert_allclose(taps[1 + i].cpu().numpy().reshape(2, 50, 768)[:, rows], g[f"v_block{i}_rows"], **tol)
    np.testing.assert_allclose(img.detach().cpu().numpy(), g["img_feat"], **tol)
    txt = m.encode_text(torch.from_numpy(recipe.captions(2, 77, cfg["vocab_size"], seed)).to(DEV))
    np.testing.assert_allclose(txt.detach().cpu().numpy(), g["txt_feat_L77"], **tol)
    txt = m.encode_text(torch.from_numpy(recipe.captions(2, 32, cfg["vocab_size"], seed + 1)).to(DEV))
    np.testing.assert_allclose(txt.detach().cpu().numpy(), g["txt_feat_L32"], **tol)


def test_vitb32_bf16_close_to_f32_and_flip_rate(golden):
    """bf16 mode (bf16 MFMA operands, fp16 residual stream) against the f32 parity mode: features within bf16 noise of the
    reference's own rows, and the sign-flip rate of 64-bit codes on 64 samples per tower.  "Bit-exact sign()" holds away from 0
    only; measured on MI355X with these seeded random-init weights: 0.15 % (image) / 0.27 % (text) of the bits on the 256-pair
    bench batch (bench.py `flip_rate_vs_f32`), hence the 1 % gate."""
    g = golden("clip_vitb32.npz")
    cfg, seed = recipe.CLIP_VITB32, int(g["seed"])
    m = _clip(cfg, seed, "bf16")
    B = 64
    images = torch.from_numpy(recipe.images(B, 224, seed)).to(DEV)
    texts = torch.from_numpy(recipe.captions(B, 77, cfg["vocab_size"], seed)).to(DEV)
    with torch.no_grad():
        img, txt = m.encode_image(images).cpu().numpy(), m.encode_text(texts).cpu().numpy()
        m.set_gemm_dtype("f32")
        img32, txt32 = m.encode_image(images).cpu().numpy(), m.encode_text(texts).cpu().numpy()
    np.testing.assert_allclose(img32[:2], g["img_feat"], rtol=1e-3, atol=1e-4)          # the f32 mode IS the reference (its golden rows)
    np.testing.assert_allclose(txt32[:2], g["txt_feat_L77"], rtol=1e-3, atol=1e-4)
    w, b = recipe.head_linear(512, 64, seed, "flip")
    for name, a, r in (("image", img, img32), ("text", txt, txt32)):
        cos = (a * r).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(r, axis=-1)
        assert cos.min() > 0.9995, cos.min()
        assert np.abs(a - r).max() < 0.05 * np.abs(r).max()
        flips = float(np.mean(np.sign(a @ w.T + b) != np.sign(r @ w.T + b)))
        print(f"bf16 {name}: cosine min {cos.min():.6f}; sign flip rate of 64-bit codes on {B} samples: {flips:.4f}")
        assert flips < 0.01, flips


def test_eot_is_first_argmax_and_batch_independence():
    """Pooled row = first argmax of the ids (model/base/model.py:370); rows of a batch do not interact."""
    cfg, seed = recipe.CLIP_TINY, 7
    m = _clip(cfg, seed, "f32")
    t = recipe.captions(4, 16, cfg["vocab_size"], 3)
    t[1, 5] = cfg["vocab_size"] - 1                      # an earlier EOT id: argmax must pick position 5
    full = m.encode_text(torch.from_numpy(t).to(DEV)).detach().cpu().numpy()
    one = m.encode_text(torch.from_numpy(t[1:2]).to(DEV)).detach().cpu().numpy()
    np.testing.assert_allclose(full[1:2], one, rtol=1e-5, atol=1e-6)
    from oracle import clip_oracle as co
    ref = co.encode_text(recipe.clip_state_dict(cfg, seed), t)
    np.testing.assert_allclose(full, ref, rtol=1e-4, atol=1e-4)


def test_large_batch_matches_small_batches():
    """M-tail handling of the GEMM tiles: B=37 (M=185, 592) equals per-sample encodes."""
    cfg, seed = recipe.CLIP_TINY, 7
    m = _clip(cfg, seed, "f32")
    img = torch.from_numpy(recipe.images(37, cfg["image_resolution"], 9)).to(DEV)
    full = m.encode_image(img).detach().cpu().numpy()
    part = torch.cat([m.encode_image(img[i:i + 5]).detach() for i in range(0, 37, 5)]).cpu().numpy()
    np.testing.assert_allclose(full, part, rtol=1e-5, atol=1e-6)


def test_backward_is_native_or_fails_loudly():
    """encode_* under grad mode run the tape-keeping forward and a real backward (tests/test_gpu_backward.py pins the values);
    a frozen model stays inference-only and refuses to differentiate."""
    cfg, seed = recipe.CLIP_TINY, 7
    m = _clip(cfg, seed, "f32")
    txt = torch.from_numpy(recipe.captions(2, 16, cfg["vocab_size"], 3)).to(DEV)
    out = m.encode_text(txt)
    assert out.requires_grad
    out.sum().backward()
    assert m.text_projection.grad is not None and torch.isfinite(m.text_projection.grad).all()
    assert m.visual.proj.grad is None
    m.assume_frozen = True
    with pytest.raises(NotImplementedError):
        m.encode_text(txt).sum().backward()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_packed_text_encode_is_bit_identical(mode):
    """cmh_text_encode_packed (no padding rows) == cmh_text_encode, bit for bit, ViT-B/32-sized text tower, ragged captions
    (one full-length, one of 3 tokens)."""
    cfg = recipe.CLIP_VITB32
    torch.manual_seed(9)
    from model.base.model import CLIP
    m = CLIP(**cfg).to(DEV).float().set_gemm_dtype(mode)
    m.assume_frozen = True
    txt = recipe.captions(12, 77, cfg["vocab_size"], 5)
    txt[1] = 0
    txt[1, 0], txt[1, 1], txt[1, 2] = cfg["vocab_size"] - 2, 17, cfg["vocab_size"] - 1      # shortest possible caption
    t = torch.from_numpy(txt).to(DEV)
    with torch.no_grad():
        m.pack_text = False
        dense = m.encode_text(t)
        m.pack_text = True
        packed = m.encode_text(t)
    rows, total = m.last_text_rows
    assert rows == int((txt.argmax(1) + 1).sum()) and total == 12 * 77 and rows < total
    assert torch.equal(dense, packed)


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8"])
def test_pooled_rows_through_the_last_block_are_bit_identical(mode):
    """cmh_set_pooled_tail: only the class-token / EOT rows are carried through the last block's out_proj, ln_2 and MLP
    (csrc/encoders.hip: block_forward on a lane with `pooled` rows) - the features must equal the full-size path bit for bit, both towers, packed
    and dense captions."""
    import cmh_native as N
    cfg = recipe.CLIP_VITB32
    torch.manual_seed(11)
    from model.base.model import CLIP
    m = CLIP(**cfg).to(DEV).float().set_gemm_dtype("bf16" if mode == "fp8" else mode)
    m.assume_frozen = True
    img = torch.from_numpy(recipe.images(6, cfg["image_resolution"], 3)).to(DEV)
    t = torch.from_numpy(recipe.captions(9, 77, cfg["vocab_size"], 4)).to(DEV)
    if mode == "fp8":
        m.calibrate_fp8(img, t)
        m.set_gemm_dtype("fp8")
    try:
        with torch.no_grad():
            outs = {}
            for on in (False, True):
                N.set_pooled_tail(on)
                for pack in (False, True):
                    m.pack_text = pack
                    outs[on, pack] = (m.encode_image(img).clone(), m.encode_text(t).clone())
    finally:
        N.set_pooled_tail(True)
    for pack in (False, True):
        assert torch.equal(outs[False, pack][0], outs[True, pack][0])
        assert torch.equal(outs[False, pack][1], outs[True, pack][1])
    assert torch.isfinite(outs[True, True][0]).all() and outs[True, True][0].abs().sum() > 0
