"""Host-side checks of the K-padded conv1 (patch 14: K = 3 * 14^2 = 588, padded to 768), nothing launched: the workspace and tape
size queries cover the padded patch matrix and the padded weight, patch 16 and 32 size exactly as before the padded path existed,
a patch-14 call with null pointers fails on its arguments, and one with valid pointers gets as far as the workspace / tape size check
(before the padded path it was refused for the patch size there).  The fp8 mode's native refusal of the padded conv1."""
import ctypes as C

import pytest

import cmh_native as N

# (gemm_dtype, resolution, patch, width, layers, embed_dim, batch) -> (cmh_vit_workspace_bytes, cmh_vit_train_bytes), as returned
# before the padded path existed (fp8: the training query is not used)
UNCHANGED = {
    (N.F32, 224, 32, 768, 12, 512, 256): (354683136, 8694429184),
    (N.F32, 224, 16, 768, 12, 512, 64): (348783360, 8450796544),
    (N.F32, 64, 32, 128, 2, 64, 3): (187904, 56125440),
    (N.F32, 224, 16, 128, 2, 64, 6): (6642176, 92721920),
    (N.BF16, 224, 32, 768, 12, 512, 256): (197003520, 4460934656),
    (N.BF16, 224, 16, 768, 12, 512, 64): (193757952, 4337527808),
    (N.BF16, 64, 32, 128, 2, 64, 3): (98048, 54334208),
    (N.BF16, 224, 16, 128, 2, 64, 6): (3623936, 75438080),
    (N.FP8, 224, 32, 768, 12, 512, 256): (197003520, None),
    (N.FP8, 224, 16, 768, 12, 512, 64): (193757952, None),
}
# the same queries for patch 14 before, when they sized an unpadded K of 588 that the encoders then refused
P14_UNPADDED = {
    (N.F32, 224, 14, 1024, 24, 768, 8): (75825664, 3541352192),
    (N.F32, 336, 14, 1024, 24, 768, 2): (42549760, 2035647232),
    (N.F32, 56, 14, 128, 2, 64, 3): (245504, 54895872),
    (N.BF16, 224, 14, 1024, 24, 768, 8): (42123776, 1816989440),
    (N.BF16, 336, 14, 1024, 24, 768, 2): (23638528, 1056250624),
    (N.BF16, 56, 14, 128, 2, 64, 3): (136192, 53805568),
}
PK, PKP = 588, 768


def _struct(dt, res, p, d, layers, E):
    s = N.VitWeights()
    s.gemm_dtype, s.resolution, s.patch, s.width, s.layers, s.embed_dim = dt, res, p, d, layers, E
    return s


def _sizes(key):
    dt, res, p, d, layers, E, B = key
    s = _struct(dt, res, p, d, layers, E)
    lib = N.lib()
    return lib.cmh_vit_workspace_bytes(C.byref(s), B), (lib.cmh_vit_train_bytes(C.byref(s), B) if dt != N.FP8 else None)


@pytest.mark.parametrize("key", sorted(UNCHANGED))
def test_patch16_and_32_sizes_are_unchanged(key):
    assert _sizes(key) == UNCHANGED[key]


@pytest.mark.parametrize("key", sorted(P14_UNPADDED))
def test_patch14_sizes_cover_the_padded_patch_matrix_and_weight(key):
    dt, res, p, d, layers, E, B = key
    e = 4 if dt == N.F32 else 2
    g2 = (res // p) ** 2
    T, M = g2 + 1, B * (g2 + 1)
    ws, tape = _sizes(key)
    ws0, tape0 = P14_UNPADDED[key]
    # encoder workspace: x, h, qkv (patch_out f32 aliases it), mlp (the patch matrix aliases it), then the padded weight [d, 768]
    lower = M * d * 4 + M * d * e + max(M * 3 * d * e, B * g2 * d * 4) + max(M * 4 * d * e, B * g2 * PKP * e) + d * PKP * e
    assert ws >= lower and ws - ws0 >= d * PKP * e, (ws, lower, ws0)
    # training tape: the patch matrix kept for conv1's weight gradient grows by the pad columns; the padded weight (GEMM dtype) and
    # its f32 gradient before the compaction are new
    assert tape - tape0 >= B * g2 * (PKP - PK) * e + d * PKP * e + d * PKP * 4, (tape, tape0)
    assert T * B == M


def test_patch14_null_pointers_are_argument_errors():
    lib = N.lib()
    s = _struct(N.BF16, 224, 14, 1024, 24, 768)
    assert lib.cmh_vit_encode(C.byref(s), None, 8, None, None, 0, None, None) == -1
    msg = lib.cmh_last_error().decode()
    assert "null pointer" in msg and "K-step" not in msg, msg
    feat = (C.c_float * 8)()
    assert lib.cmh_vit_encode(C.byref(s), None, 8, feat, None, 0, None, None) == -1
    msg = lib.cmh_last_error().decode()
    assert "null pointer" in msg and "K-step" not in msg, msg
    assert lib.cmh_vit_forward_train(C.byref(s), None, 8, feat, None, 0, None) == -1
    msg = lib.cmh_last_error().decode()
    assert "bad arguments" in msg and "K-step" not in msg, msg


def _dummy_call_args(dt, d=1024, layers=24, E=768, res=224):
    """a patch-14 struct whose pointers are valid host addresses (nothing is dereferenced before the size checks return)"""
    s = _struct(dt, res, 14, d, layers, E)
    keep = [(C.c_float * 16)() for _ in range(8)]
    blocks = (N.BlockWeights * layers)()
    for name, buf in zip(("conv1_w", "class_embedding", "positional_embedding", "ln_pre_w", "ln_pre_b", "ln_post_w", "ln_post_b",
                          "proj_t"), keep):
        setattr(s, name, C.addressof(buf))
    s.blocks = blocks
    return s, (keep, blocks), (C.c_float * 16)(), (C.c_float * 16)(), (C.c_uint8 * 4096)()


@pytest.mark.parametrize("dt", [N.F32, N.BF16])
def test_patch14_calls_reach_the_workspace_check(dt):
    """the padded path is taken: the encode and the training forward fail only on the (deliberately) small scratch"""
    lib = N.lib()
    s, _keep, image, feat, ws = _dummy_call_args(dt)
    assert lib.cmh_vit_encode(C.byref(s), image, 8, feat, ws, 1024, None, None) == -2, lib.cmh_last_error().decode()
    assert "workspace" in lib.cmh_last_error().decode()
    assert lib.cmh_vit_forward_train(C.byref(s), image, 8, feat, ws, 1024, None) == -2, lib.cmh_last_error().decode()
    assert "tape too small" in lib.cmh_last_error().decode()


def test_patch14_fp8_mode_is_refused_natively():
    """the library refuses the fp8 mode for a patch size that needs the padded conv1 before it looks at the workspace (the Python check in
    CLIP.set_gemm_dtype comes first in the product)"""
    lib = N.lib()
    s, _keep, image, feat, ws = _dummy_call_args(N.FP8)
    assert lib.cmh_vit_encode(C.byref(s), image, 8, feat, ws, 1024, None, None) == -1
    msg = lib.cmh_last_error().decode()
    assert "fp8 mode: patch 14" in msg and "not built for fp8" in msg, msg
