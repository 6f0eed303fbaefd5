"""Attention at image-token counts past 128 (ViT-B/16: T = 197, ViT-L/14: 257, ViT-L/14@336px: 577) against an fp64 statement of the
op on the same rounded operands.  The backward runs on the tiled kernel of csrc/attention_bwd.hip (T > 128); the bf16 forward there
runs on the f32-accumulating VALU kernel.

Bounds: f32 rtol 1e-4 / atol 1e-5.  bf16, per Q / K / V slice: 1e-2 of the slice's max and an error 2-norm <= 4e-3 of the slice's
2-norm.  The tiled kernel computes S, P, dP and dS in f32 from the bf16 operands and rounds only its outputs (2^-9 relative), so the
argument of test_gpu_backward.test_attention_backward_at_tower_shapes carries over with room to spare."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG_T = [129, 197, 257, 577]


def _inputs(B, T, d, kpm, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * d, generator=g)
    dout = torch.randn(B * T, d, generator=g)
    mask = None
    if kpm:
        vis = torch.randint(1, T + 1, (B,), generator=g)
        vis[0] = 1
        if B > 1:
            vis[1] = T
        mask = torch.arange(T)[None, :] >= vis[:, None]              # trailing pads; key 0 always visible
    return qkv, dout, mask


def _probs(qd, B, T, d, causal, md):
    H = d // 64
    q, k, v = qd.double().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)                     # [B, H, T, 64] each
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64, device=DEV).triu(1)
    if md is not None:
        s = s.masked_fill(md[:, None, None, :], float("-inf"))
    return q, k, v, torch.softmax(s, -1)


def _check_slices(got, ref, d, what):
    worst = [0.0, 0.0]
    for i in range(ref.shape[1] // d):
        r, e = ref[:, i * d:(i + 1) * d], got[:, i * d:(i + 1) * d] - ref[:, i * d:(i + 1) * d]
        emax, enorm = float(e.abs().max() / r.abs().max()), float(e.norm() / r.norm())
        worst = [max(worst[0], emax), max(worst[1], enorm)]
        assert emax <= 1e-2 and enorm <= 4e-3, (what, i, emax, enorm)
    print(f"{what}: worst {worst[0]:.2e} of a slice's max, {worst[1]:.2e} of its 2-norm")


@pytest.mark.parametrize("T", LONG_T)
@pytest.mark.parametrize("variant", ["plain", "causal", "kpm"])
def test_attention_forward_bf16_long(T, variant):
    import cmh_native as N
    B, d = 3, 128
    causal, kpm = variant == "causal", variant == "kpm"
    qkv, _, mask = _inputs(B, T, d, kpm, 11 * T + len(variant))
    qd = qkv.to(torch.bfloat16).to(DEV)
    md = None if mask is None else mask.to(DEV)
    o = N.attention(qd, B, T, causal, md)
    _, _, v, p = _probs(qd, B, T, d, causal, md)
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B * T, d)
    _check_slices(o.double(), ref, d, f"attention forward bf16 T={T} {variant}")


def _backward_case(B, T, d, causal, kpm, mode):
    import backward_ops as Bo
    import cmh_native as N
    qkv, dout, mask = _inputs(B, T, d, kpm, B + T + d + 7 * causal + kpm)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    qd, dd = qkv.to(dt).to(DEV), dout.to(dt).to(DEV)
    md = None if mask is None else mask.to(DEV)
    o_gpu = N.attention(qd, B, T, causal, md)
    dqkv = Bo.attention_backward(qd, o_gpu, dd, B, T, causal, md)
    assert torch.equal(dqkv, Bo.attention_backward(qd, o_gpu, dd, B, T, causal, md)), "the backward is not deterministic"
    H = d // 64
    q, k, v, p = _probs(qd, B, T, d, causal, md)
    do = dd.double().view(B, T, H, 64).permute(0, 2, 1, 3)
    o = p @ v                    # the tiled kernel forms D = rowsum(P o dP) from its own P and dP (= rowsum(dO o PV)), not from o_gpu
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)) / 8.0
    ref = torch.stack((ds @ k, ds.transpose(-1, -2) @ q, dv)).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * d)
    got = dqkv.double()
    assert torch.isfinite(got).all()
    if mode == "f32":
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    else:
        _check_slices(got, ref, d, f"attention backward bf16 B={B} T={T} d={d} causal={causal} kpm={kpm}")


@pytest.mark.parametrize("T", LONG_T)
@pytest.mark.parametrize("variant", ["plain", "causal", "kpm"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attention_backward_long(T, variant, mode):
    _backward_case(3, T, 128, variant == "causal", variant == "kpm", mode)


@pytest.mark.parametrize("B,T,d", [(256, 197, 768), (32, 257, 1024)])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attention_backward_long_tower_shapes(B, T, d, mode):
    """ViT-B/16 at batch 256 (12 heads x 197 tokens) and ViT-L/14 at batch 32 (16 heads x 257 tokens)."""
    _backward_case(B, T, d, False, False, mode)


def test_attention_backward_refuses_beyond_built_length():
    import backward_ops as Bo
    import cmh_native as N
    B, T, d = 1, 4097, 64
    qkv = torch.zeros(B * T, 3 * d, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(B * T, d, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(N.NativeError, match="not built"):
        Bo.attention_backward(qkv, o, o, B, T, False)
