"""The fused conv1 stem (csrc/conv1_stem.hip, cmh_set_conv1_fused): one implicit-GEMM launch whose loader waves round the image into the
bf16 patch tile, against the two-launch stem (patchify_kernel + GEMM) on the same inputs.  Another schedule of the same arithmetic - the
same rounding per image value, the same MFMA chain over K per output element - so every comparison is bit equality.

Shapes: the smallest at which the kernel can go wrong - one partial 160-row tile with one and with three column tiles, two full tiles
plus a partial one with the seam of a two-tensor batch inside a tile, and patch 16 (four 16-float runs per K-step instead of two of
32).  The images carry bf16 rounding ties and near-ties, so a rounding other than f32_to_bf16's round-to-nearest-even cannot pass."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TEXT = dict(context_length=16, vocab_size=512, transformer_width=128, transformer_heads=2, transformer_layers=1)
CASES = {   # name: (patch, resolution, width, batch or (batch_a, batch_b))
    "p32_one_partial_tile_one_column_tile": (32, 64, 256, 3),
    "p32_one_partial_tile_three_column_tiles": (32, 224, 768, 3),
    "p32_split_batch_seam_inside_a_tile": (32, 224, 768, (3, 4)),
    "p16_four_runs_per_kstep": (16, 64, 256, 5),
}


def _model(patch, resolution, width, mode="bf16", layers=1):
    from model.base.model import CLIP
    torch.manual_seed(1000 * patch + width)
    m = CLIP(embed_dim=64, image_resolution=resolution, vision_layers=layers, vision_width=width, vision_patch_size=patch, **TEXT)
    m = m.to(DEV).float().set_gemm_dtype(mode)
    m.assume_frozen = True
    return m


def _ties(n):
    """bf16 keeps 7 mantissa bits: 1 + k / 256 with odd k lies exactly between two neighbours (round to even: down for k = 1, up for
    k = 3), one f32 ulp to either side of it is a near-tie; the same around other exponents and signs, a value that rounds up into the
    next binade, an f32 denormal, and the largest finite values (the last rounds to infinity only if the rounding adds instead of
    truncating - kept out: an infinity would turn the outputs into NaN)."""
    ulp = 2.0 ** -23
    base = [1 + 1 / 256, 1 + 3 / 256, 1 + 1 / 256 + ulp, 1 + 1 / 256 - ulp, 1 + 3 / 256 + ulp, 1 + 3 / 256 - ulp, 1 + 255 / 256, 1 + 255 / 256 + ulp,
            1 + 127 / 256, 1 + 129 / 256]
    vals = [s * v * e for v in base for e in (1.0, 2.0 ** -6, 2.0 ** 5) for s in (1.0, -1.0)] + [1e-40, -1e-40, 0.0, -0.0]
    return torch.tensor((vals * (n // len(vals) + 1))[:n], dtype=torch.float32)


def _images(batch, resolution, seed):
    """N(0, 1) scaled so that the patch dot products stay O(1), with ties placed at scattered positions of every image"""
    x = torch.from_numpy(recipe.images(batch, resolution, seed)) * 0.5
    flat = x.view(batch, -1)
    g = torch.Generator().manual_seed(seed)
    n = 257
    for b in range(batch):
        pos = torch.randperm(flat.shape[1], generator=g)[:n]
        flat[b, pos] = _ties(n)
    flat[:, 0] = 1 + 1 / 256          # ... and at the corners of the first and the last patch
    flat[:, -1] = -(1 + 3 / 256)
    return x.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _both(N, fn):
    """fn() with the fused stem off, then on -> (off, on, launches of the fused kernel in the `on` run)"""
    try:
        N.set_conv1_fused(0)
        N.prof_gemm_begin(256)
        try:
            off = fn()
        finally:
            N.prof_gemm_end()
        assert "conv1_stem_kernel" not in N.prof_gemm_by_kernel()
        N.set_conv1_fused(1)
        N.prof_gemm_begin(256)
        try:
            on = fn()
        finally:
            N.prof_gemm_end()
        ran = N.prof_gemm_by_kernel().get("conv1_stem_kernel", (0.0, 0.0, 0))
    finally:
        N.set_conv1_fused(-1)
    return off, on, ran


@pytest.mark.parametrize("name", list(CASES))
def test_fused_stem_has_the_two_launch_stem_s_bits(name):
    import cmh_native as N
    patch, R, width, batch = CASES[name]
    m = _model(patch, R, width)
    split = isinstance(batch, tuple)
    B = sum(batch) if split else batch
    img = _images(B, R, 5)
    parts = (img[:batch[0]].contiguous(), img[batch[0]:].contiguous()) if split else (img,)
    txt = torch.from_numpy(recipe.captions(B, TEXT["context_length"], TEXT["vocab_size"], 3)).to(DEV)

    def run():
        with torch.no_grad():
            po, _ = m.patch_embed(*parts)
            if split:
                feat = m.encode_pair2(parts[0], txt[:batch[0]], parts[1], txt[batch[0]:])[0]
            else:
                feat = m.encode_image(img)
            return po.clone(), feat.clone()

    (po0, f0), (po1, f1), (ms, flops, launches) = _both(N, run)
    g2, K = (R // patch) ** 2, 3 * patch * patch
    print(f"{name}: M = {B * g2}, N = {width}, K = {K}; fused launches {launches}, {flops:.0f} FLOPs")
    assert launches == 2 and flops == 2 * 2.0 * B * g2 * width * K      # patch_embed's and the encode's, real rows
    assert torch.isfinite(po0).all() and po0.abs().max() > 0.1
    assert torch.equal(_bits(po0), _bits(po1))
    assert torch.equal(_bits(f0), _bits(f1)) and torch.isfinite(f0).all()
    # ... and against the definition, bf16(unfold(image)) . bf16(W)^T in f64: the products of bf16 values are exact in f32, so the
    # error is that of K f32 additions in whatever order - at most K 2^-24 sum |a| |w| per element
    w = m.visual.conv1.weight.detach().reshape(width, K).bfloat16().double()
    pm = torch.nn.functional.unfold(img.bfloat16().double(), patch, stride=patch).transpose(1, 2).reshape(B * g2, K)
    err, bound = (po1.double() - pm @ w.T).abs(), K * 2.0 ** -24 * (pm.abs() @ w.abs().T)
    print(f"{name}: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_a_stage_with_a_nan_is_rounded_by_f32_to_bf16_itself():
    """The loader converts a stage with v_cvt_pk_bf16_f32 unless the stage holds a NaN (conv1_stem.hip: C1_ROUND); then f32_to_bf16
    rounds it.  One image with NaNs of two payloads and an inf - inf false alarm: the same bits in patch_out, NaNs included."""
    import cmh_native as N
    patch, R, width, B = 32, 64, 256, 3
    m = _model(patch, R, width)
    img = _images(B, R, 9)
    flat = img.view(B, -1)
    nans = np.array([0x7FC00001, 0xFFC00123, 0x7F800001], dtype=np.uint32).view(np.float32)      # quiet, negative quiet, signalling
    flat[1, 100:103] = torch.from_numpy(nans).to(DEV)
    flat[2, 5000], flat[2, 5001] = float("inf"), float("-inf")

    def run():
        with torch.no_grad():
            return m.patch_embed(img)[0].clone()

    po0, po1, (_, _, launches) = _both(N, run)
    assert launches == 1
    assert torch.isnan(po0).any() and torch.isfinite(po0[:4]).all()
    assert torch.equal(_bits(po0), _bits(po1))


@pytest.mark.parametrize("what", ["f32_mode", "patch_14"])
def test_shapes_the_fused_stem_is_not_built_for_keep_the_two_launches(what):
    import cmh_native as N
    patch, R, width, mode = (32, 64, 256, "f32") if what == "f32_mode" else (14, 56, 256, "bf16")
    m = _model(patch, R, width, mode)
    img = _images(3, R, 7)

    def run():
        with torch.no_grad():
            return m.patch_embed(img)[0].clone(), m.encode_image(img).clone()

    (po0, f0), (po1, f1), (_, _, launches) = _both(N, run)
    assert launches == 0
    assert torch.equal(_bits(po0), _bits(po1)) and torch.equal(_bits(f0), _bits(f1)) and torch.isfinite(f0).all()


def test_training_forward_still_writes_the_patch_matrix():
    """The tape keeps the patch matrix for conv1's weight gradient: the training forward never takes the fused stem, whatever the
    switch says.  keep_patches (the flag the training forward passes) must leave bf16(unfold(image)); and a real backward through
    encode_image gives the same conv1 gradient with the switch on and off."""
    import cmh_native as N
    patch, R, width, B = 32, 64, 256, 3
    m = _model(patch, R, width)
    img = _images(B, R, 11)
    K, g2 = 3 * patch * patch, (R // patch) ** 2
    want = torch.nn.functional.unfold(img.bfloat16().float(), patch, stride=patch).transpose(1, 2).reshape(B * g2, K).bfloat16()

    def kept():
        with torch.no_grad():
            po, pm = m.patch_embed(img, keep_patches=True)
            return po.clone(), pm.clone()

    (po0, pm0), (po1, pm1), (_, _, launches) = _both(N, kept)
    assert launches == 0
    assert torch.equal(pm0.view(torch.int16), want.view(torch.int16)) and torch.equal(pm1.view(torch.int16), want.view(torch.int16))
    assert torch.equal(_bits(po0), _bits(po1))

    m.assume_frozen = False

    def train():
        m.zero_grad(set_to_none=True)
        f = m.encode_image(img)
        assert f.requires_grad
        f.square().sum().backward()
        return f.detach().clone(), m.visual.conv1.weight.grad.clone()

    (f0, g0), (f1, g1), (_, _, launches) = _both(N, train)
    assert launches == 0
    assert torch.equal(_bits(f0), _bits(f1)) and torch.equal(_bits(g0), _bits(g1))
    assert torch.isfinite(g0).all() and g0.abs().max() > 0
