"""ViT-B/16 geometry (224 px, patch 16: 197 image tokens) through CLIP.encode_image / encode_text under autograd, against
oracle/clip_autograd.py in float64 on the GPU (torch's own ops, nothing of libcmh), for L = sum(img_feat * Gi) + sum(txt_feat * Gt).
Past 128 tokens the attention backward runs on the tiled kernel of csrc/attention_bwd.hip; before it, training refused T > 128.

Bars: those of test_gpu_train_real_size.py.  f32 mode: features within 1e-4, every gradient within 1e-4 of its largest element and
its norm within 1e-4 relative.  bf16 mode: every gradient's cosine >= 0.9995 and norm within 1 %."""
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 13
CFG_TINY = dict(recipe.CLIP_TINY, image_resolution=224, vision_patch_size=16)          # width 128, 2 layers, 2 heads, T = 197
CFG_B16 = dict(recipe.CLIP_VITB32, vision_patch_size=16)                                # 12 layers, widths 768 / 512, T = 197
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_after_module():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _get(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _inputs(cfg, B):
    def make():
        image = recipe.images(B, cfg["image_resolution"], SEED)
        text = recipe.captions(B, cfg["context_length"], cfg["vocab_size"], SEED)
        g = torch.Generator().manual_seed(2000 + B)
        gi, gt = torch.randn(B, cfg["embed_dim"], generator=g), torch.randn(B, cfg["embed_dim"], generator=g)
        return tuple(torch.as_tensor(a).to(DEV) for a in (image, text, gi, gt))
    return _get(("inputs", id(cfg), B), make)


def _state_dict(cfg):
    return _get(("sd", id(cfg)), lambda: recipe.clip_state_dict(cfg, SEED))


def _reference(cfg, B):
    def make():
        from oracle import clip_autograd as ca
        out = ca.towers(_state_dict(cfg), *_inputs(cfg, B), device=DEV)
        torch.cuda.empty_cache()
        return out
    return _get(("ref", id(cfg), B), make)


def _model(cfg):
    def make():
        from model.base.model import CLIP
        m = CLIP(cfg["embed_dim"], cfg["image_resolution"], cfg["vision_layers"], cfg["vision_width"], cfg["vision_patch_size"],
                 cfg["context_length"], cfg["vocab_size"], cfg["transformer_width"], cfg["transformer_heads"], cfg["transformer_layers"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict(cfg).items()}, strict=True)
        return m.to(DEV).float()
    return _get(("model", id(cfg)), make)


def _train(cfg, B, mode):
    m = _model(cfg).set_gemm_dtype(mode)
    m.zero_grad(set_to_none=True)
    image, text, gi, gt = _inputs(cfg, B)
    fi, ft = m.encode_image(image), m.encode_text(text)
    ((fi * gi).sum() + (ft * gt).sum()).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return fi.detach(), ft.detach(), grads


def _compare(got, ref, cfg):
    assert got.keys() == ref.keys(), set(got) ^ set(ref)
    assert len(ref) == 8 + 5 + 12 * (cfg["vision_layers"] + cfg["transformer_layers"])
    out = {}
    for n, r in ref.items():
        g = got[n].double()
        cos = float(g.flatten() @ r.flatten() / (g.norm() * r.norm() + 1e-300))
        out[n] = (float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300), float(g.norm() / r.norm()), cos)
    return out


def _check_f32(cfg, B):
    rfi, rft, ref = _reference(cfg, B)
    fi, ft, got = _train(cfg, B, "f32")
    df = max(float((fi.double() - rfi).abs().max()), float((ft.double() - rft).abs().max()))
    st = _compare(got, ref, cfg)
    worst = max(st, key=lambda n: st[n][0])
    print(f"\nf32 B={B} patch {cfg['vision_patch_size']}: features max|d| {df:.2e}; worst err/max {st[worst][0]:.2e} ({worst}); "
          f"worst |norm ratio - 1| {max(abs(v[1] - 1) for v in st.values()):.2e}")
    assert df <= 1e-4, df
    bad = {n: v for n, v in st.items() if not (v[0] <= 1e-4 and abs(v[1] - 1) <= 1e-4)}
    assert not bad, bad


def _check_bf16(cfg, B):
    _, _, ref = _reference(cfg, B)
    _, _, got = _train(cfg, B, "bf16")
    st = _compare(got, ref, cfg)
    worst = min(st, key=lambda n: st[n][2])
    print(f"\nbf16 B={B} patch {cfg['vision_patch_size']}: worst cosine {st[worst][2]:.6f} ({worst}); worst |norm ratio - 1| "
          f"{max(abs(v[1] - 1) for v in st.values()):.2e}")
    bad = {n: v for n, v in st.items() if not (v[2] >= 0.9995 and abs(v[1] - 1) <= 0.01)}
    assert not bad, bad


def test_tiny_b16_f32_mode_gradients_match_fp64_autograd():
    _check_f32(CFG_TINY, 6)


def test_tiny_b16_bf16_mode_gradients_track_fp64_autograd():
    _check_bf16(CFG_TINY, 6)


def test_b16_f32_mode_gradients_match_fp64_autograd():
    _check_f32(CFG_B16, 64)


def test_b16_bf16_mode_gradients_track_fp64_autograd():
    _check_bf16(CFG_B16, 64)


def test_tiny_b16_pair_paths_are_bit_identical_to_one_tower_calls():
    """cmh_clip_encode_pair / _pair2 at 197 image tokens against 16 caption tokens: the towers have different row counts per sample"""
    m = _model(CFG_TINY).set_gemm_dtype("bf16")
    image, text, _, _ = _inputs(CFG_TINY, 6)
    with torch.no_grad():
        fi, ft = m.encode_image(image), m.encode_text(text)
        pi, pt = m.encode_pair(image, text)
        qi, qt = m.encode_pair2(image[:4], text[:4], image[4:], text[4:])
    assert torch.equal(pi, fi) and torch.equal(pt, ft)
    assert torch.equal(qi, fi) and torch.equal(qt, ft)


def test_tiny_b16_fp8_mode_is_refused():
    m = _model(CFG_TINY)
    with pytest.raises(Exception, match="at most 128 image tokens"):
        m.set_gemm_dtype("fp8")
    assert m._gemm_dtype != __import__("cmh_native").FP8


def test_tiny_b16_mith_is_refused():
    from model.MITH import build_model
    with pytest.raises(NotImplementedError, match="at most 80 tokens"):
        build_model({k: torch.from_numpy(v) for k, v in _state_dict(CFG_TINY).items()})
