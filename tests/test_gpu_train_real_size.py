"""The training towers' gradients at the size the product trains at: ViT-B/32 (12 blocks, widths 768 / 512, 12 / 8 heads, 50 image
tokens, 77-token captions) through CLIP.encode_image / encode_text under autograd (model/base/train_ops.py -> cmh_*_forward_train /
cmh_*_backward_part), against oracle/clip_autograd.py run in float64 on the GPU with torch's own ops (nothing of libcmh), for
L = sum(img_feat * Gi) + sum(txt_feat * Gt).  Every parameter gradient of both towers (301 tensors) is checked.

The batch: recipe images; captions on the real vocabulary (EOT = 49407) with one full 77-token caption (row 0), one that is
SOT EOT only (row 1: 2 packed rows) and the rest ragged.  B = 137 is a ragged last batch (the train loader keeps it, train/base.py):
6 850 image rows, a K tail of 2 in every weight gradient.  At this size the bf16 training path takes forms the width-256 tests never
reach: the one-launch block wgrad with no K split on the image tower (216 tiles) and a split of 2 on the text tower (96 tiles), the
16-bit residual-gradient stream over 12 blocks (24 roundings), the batched final reductions over 12 800 / ~10 000 rows."""
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = recipe.CLIP_VITB32
SEED = 11
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_after_module():
    """the fp64 references, inputs and model are shared by the tests of this file and released after its last one"""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _inputs(B):
    key = ("inputs", B)
    if key not in _CACHE:
        image = recipe.images(B, CFG["image_resolution"], SEED)
        text = recipe.captions(B, CFG["context_length"], CFG["vocab_size"], SEED)
        text[1] = 0
        text[1, :2] = recipe.SOT, recipe.EOT
        assert text[0, -1] == recipe.EOT and (text == recipe.EOT).sum() == B and text.max() == recipe.EOT
        g = torch.Generator().manual_seed(1000 + B)
        gi, gt = torch.randn(B, CFG["embed_dim"], generator=g), torch.randn(B, CFG["embed_dim"], generator=g)
        _CACHE[key] = tuple(torch.as_tensor(a).to(DEV) for a in (image, text, gi, gt))
    return _CACHE[key]


def _state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = recipe.clip_state_dict(CFG, SEED)
    return _CACHE["sd"]


def _reference(B):
    """fp64 autograd of the reference's towers on the GPU (oracle/clip_autograd.py): (img_feat, txt_feat, {name: grad}), float64"""
    key = ("ref", B)
    if key not in _CACHE:
        from oracle import clip_autograd as ca
        image, text, gi, gt = _inputs(B)
        _CACHE[key] = ca.towers(_state_dict(), image, text, gi, gt, device=DEV)
        torch.cuda.empty_cache()
    return _CACHE[key]


def _model():
    if "model" not in _CACHE:
        from model.base.model import CLIP
        m = CLIP(CFG["embed_dim"], CFG["image_resolution"], CFG["vision_layers"], CFG["vision_width"], CFG["vision_patch_size"],
                 CFG["context_length"], CFG["vocab_size"], CFG["transformer_width"], CFG["transformer_heads"], CFG["transformer_layers"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict().items()}, strict=True)
        _CACHE["model"] = m.to(DEV).float()
    return _CACHE["model"]


def _train(B, mode):
    """one forward + backward of both towers -> (img_feat, txt_feat, {name: f32 gradient})"""
    m = _model().set_gemm_dtype(mode)
    m.zero_grad(set_to_none=True)
    image, text, gi, gt = _inputs(B)
    fi, ft = m.encode_image(image), m.encode_text(text)
    ((fi * gi).sum() + (ft * gt).sum()).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return fi.detach(), ft.detach(), grads


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def _compare(got, ref):
    """{name: (max|got - ref| / max|ref|, |got| / |ref|, cosine)}; every gradient of the reference, no other"""
    assert got.keys() == ref.keys(), set(got) ^ set(ref)
    assert len(ref) == 8 + 5 + 12 * 12 * 2
    out = {}
    for n, r in ref.items():
        g = got[n].double()
        out[n] = (float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300), float(g.norm() / r.norm()), _cos(g, r))
    return out


def _worst(stats, i, largest=True, k=3):
    order = sorted(stats.items(), key=lambda kv: kv[1][i], reverse=largest)
    return ", ".join(f"{n} {v[i]:.6g}" for n, v in order[:k])


def _peak():
    return f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB"


@pytest.mark.parametrize("B", [64, 137])
def test_f32_mode_gradients_match_fp64_autograd(B):
    """The f32 mode (the reference's arithmetic) at real size: features within 1e-4 of the fp64 statement; every gradient within
    1e-4 of its largest element, its norm within 1e-4 relative (the tiny configuration measured 2e-6 of max)."""
    rfi, rft, ref = _reference(B)
    fi, ft, got = _train(B, "f32")
    df = max(float((fi.double() - rfi).abs().max()), float((ft.double() - rft).abs().max()))
    st = _compare(got, ref)
    print(f"\nf32 B={B}: features max|d| {df:.2e}; worst err/max: {_worst(st, 0)}; worst |norm ratio - 1| "
          f"{max(abs(v[1] - 1) for v in st.values()):.2e}; {_peak()}")
    assert df <= 1e-4, df
    bad = {n: v for n, v in st.items() if not (v[0] <= 1e-4 and abs(v[1] - 1) <= 1e-4)}
    assert not bad, bad


@pytest.mark.parametrize("B", [256, 137])
def test_bf16_mode_gradients_track_fp64_autograd(B):
    """The default training path (bf16 GEMM operands, fp16 residual stream, MFMA attention backward, one-launch block wgrad, 16-bit
    gradient stream) against fp64: every gradient's cosine >= 0.9995 and norm within 1 %.  Measured on MI355X: worst cosine 0.99992
    (token_embedding / positional_embedding, the text tower's first blocks), worst norm ratio 1 +- 2.4e-3, no growth with depth
    beyond ~3e-5 of cosine from block 11 to block 0; with the f32 stream (cmh_set_grad_stream16(0)) 0.99995, in the f32 mode 1 - 1e-10:
    the bf16 operands, not the stream, set the distance, and the bars stand 6x / 4x above it."""
    _, _, ref = _reference(B)
    _, _, got = _train(B, "bf16")
    st = _compare(got, ref)
    print(f"\nbf16 B={B}: worst cosine: {_worst(st, 2, largest=False)}; worst |norm ratio - 1|: "
          f"{max(abs(v[1] - 1) for v in st.values()):.2e} ({max(st, key=lambda n: abs(st[n][1] - 1))}); {_peak()}")
    bad = {n: v for n, v in st.items() if not (v[2] >= 0.9995 and abs(v[1] - 1) <= 0.01)}
    assert not bad, bad


def _moved(a, b, image_tower):
    return sum(int(not torch.equal(a[n], b[n])) for n in a if n.startswith("visual.") == image_tower)


@pytest.mark.parametrize("B", [256, 137])
def test_one_launch_block_wgrad_matches_four_launches(B, monkeypatch):
    """The block's four weight gradients as ONE multi-problem launch (CMH_WGRAD_MULTI=1, the default) against four launches (=0), on
    the same f32 gradient stream: the same products summed in another split of the rows, <= 2e-4 of max per tensor (the bound of
    test_block_wgrads_in_one_launch_match_the_four_launches).  At this width the image tower's launch has no K split (S = 1) and the
    text tower's S = 2 (partial planes + the bias gradients' final jobs over 2 slices); the path must have been taken on both."""
    import cmh_native as Nn
    Nn.set_grad_stream16(0)
    try:
        monkeypatch.setenv("CMH_WGRAD_MULTI", "1")
        one = _train(B, "bf16")[2]
        monkeypatch.setenv("CMH_WGRAD_MULTI", "0")
        four = _train(B, "bf16")[2]
    finally:
        Nn.set_grad_stream16(-1)
    worst = (0.0, "")
    for n, a in four.items():
        err = float((a - one[n]).abs().max()) / (float(a.abs().max()) + 1e-30)
        worst = max(worst, (err, n))
        assert err <= 2e-4, (n, err)
    print(f"\none-launch vs four-launch wgrads B={B}: worst {worst[0]:.2e} of max ({worst[1]})")
    assert _moved(four, one, True) > 0 and _moved(four, one, False) > 0


@pytest.mark.parametrize("B", [256, 137])
def test_16bit_gradient_stream_tracks_the_f32_stream_at_real_size(B):
    """The 16-bit residual-gradient stream (default) against the f32 stream (cmh_set_grad_stream16(0)) over 12 blocks per tower:
    cosine > 0.9995, norms within 1 % (the bounds of the 6-layer test), and against the fp64 statement the 16-bit stream loses less
    than 2e-3 of cosine for any tensor."""
    import cmh_native as Nn
    _, _, ref = _reference(B)
    try:
        Nn.set_grad_stream16(1)
        s16 = _train(B, "bf16")[2]
        Nn.set_grad_stream16(0)
        s32 = _train(B, "bf16")[2]
    finally:
        Nn.set_grad_stream16(-1)
    worst, gap, moved = (1.0, ""), (0.0, ""), 0
    for n, a in s32.items():
        b = s16[n]
        moved += int(not torch.equal(a, b))
        c = _cos(a, b)
        worst = min(worst, (c, n))
        assert c > 0.9995, (n, c)
        assert abs(float(b.norm() / a.norm()) - 1.0) < 0.01, (n, float(a.norm()), float(b.norm()))
        gap = max(gap, (_cos(ref[n], a) - _cos(ref[n], b), n))
    print(f"\n16-bit vs f32 stream B={B}: worst cosine {worst[0]:.6f} ({worst[1]}); largest loss of cosine against fp64 "
          f"{gap[0]:.2e} ({gap[1]})")
    assert moved > 0
    assert gap[0] < 2e-3, gap


@pytest.mark.parametrize("B", [256, 137])
def test_backward_in_parts_equals_one_call_at_real_size(B):
    """model/base/train_ops.py PARTS: the towers' backward as 2 calls gives the same gradients as 1, bit for bit; token_embedding
    (the atomic scatter) to its summation order, as in test_tower_backward_in_parts_equals_one_call."""
    from model.base import train_ops as T
    old = T.PARTS
    try:
        T.PARTS = 1
        one = _train(B, "bf16")[2]
        T.PARTS = 2
        two = _train(B, "bf16")[2]
    finally:
        T.PARTS = old
    assert one.keys() == two.keys()
    for n in one:
        if n == "token_embedding.weight":
            torch.testing.assert_close(one[n], two[n], rtol=1e-4, atol=1e-5 * float(one[n].abs().max()))
        else:
            assert torch.equal(one[n], two[n]), n


@pytest.mark.parametrize("B", [256, 137])
def test_pooled_tail_matches_the_full_path_at_real_size(B):
    """The last block's row-wise tail on the pooled rows only (cmh_set_pooled_tail, default on) against the full-size path: identical
    features either way.  On the f32 gradient stream the two differ by the weight gradients' summation order only: every gradient
    within the bf16 bound of test_pooled_tail_of_the_training_towers_matches_the_full_path (4e-3 of max; measured 1.4e-6).
    On the default 16-bit stream they do NOT differ by summation order alone: the full-size last block is a one-launch block and so
    carries its residual gradient as bf16 (two roundings), the pooled one keeps it in f32 (csrc/encoders_bwd.hip block_backward),
    and those roundings, fed through 11 more blocks of bf16 operands, move single elements by up to 1.3 % of a tensor's max while
    both paths stay equally far from fp64 (measured 1.2-1.6 % each for the tensors that move most).  There the bounds are those of
    the 16-bit stream itself: cosine > 0.9995 between the two, and against fp64 neither is more than 2e-3 of cosine worse."""
    import cmh_native as Nn
    _, _, ref = _reference(B)
    res = {}
    try:
        for s16 in (0, 1):
            Nn.set_grad_stream16(s16)
            for on in (False, True):
                Nn.set_pooled_tail(on)
                res[s16, on] = _train(B, "bf16")
    finally:
        Nn.set_pooled_tail(True)
        Nn.set_grad_stream16(-1)
    for s16 in (0, 1):
        assert torch.equal(res[s16, False][0], res[s16, True][0]) and torch.equal(res[s16, False][1], res[s16, True][1])
    worst, cmin, gap = (0.0, ""), (1.0, ""), (0.0, "")
    for n, a in res[0, False][2].items():
        err = float((res[0, True][2][n] - a).abs().max()) / max(float(a.abs().max()), 1e-6)
        worst = max(worst, (err, n))
        assert err < 4e-3, (n, err)
        on, off = res[1, True][2][n], res[1, False][2][n]
        cmin = min(cmin, (_cos(on, off), n))
        assert cmin[0] > 0.9995, cmin
        gap = max(gap, (abs(_cos(ref[n], on) - _cos(ref[n], off)), n))
    print(f"\npooled tail on vs off B={B}: f32 stream worst {worst[0]:.2e} of max ({worst[1]}); 16-bit stream worst cosine "
          f"{cmin[0]:.6f} ({cmin[1]}), largest difference of cosine against fp64 {gap[0]:.2e} ({gap[1]})")
    assert gap[0] < 2e-3, gap
