"""Both towers' attentions as one launch (csrc/attention.hip: attention_mfma_pair_kernel<NA, NB>, launch_attention_pair; include/cmh.h:
cmh_attention_pair) and the five-key-tile body behind its text side (65 <= T <= 80).

Each side of a pair launch runs the single kernels' body, and the five-tile form feeds the MFMAs what the six-tile form feeds them
at T <= 80 (its sixth tile is all masked: scores -1e30, exp2 = 0, V rows zero), so every output has cmh_attention's bits: the tests
ask for torch.equal, never for a tolerance, except where the five-tile form is set against the fp64 statement of the op - there
with the bounds tests/test_gpu_attention_edges.py uses for bf16."""
import numpy as np
import pytest
import torch

import attnutil as au
import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLICE_MAX, SLICE_NORM = 1e-2, 4e-3          # as tests/test_gpu_attention_edges.py (bf16)

# (B, T, d, causal) of side 0 and of side 1
ROWS = [((3, 50, 192, 0), (5, 77, 128, 1)),
        ((3, 50, 192, 0), (5, 65, 128, 1)),
        ((3, 50, 192, 0), (5, 80, 128, 1)),
        ((2, 33, 128, 0), (3, 64, 64, 1)),
        ((2, 49, 128, 0), (3, 17, 128, 1))]
SIDE1_VARIANTS = ("none", "tail", "holes", "tile")          # attnutil.CAUSAL_OK: these keep key 0 visible
PATTERN = 0x7FC1                                            # a bf16 NaN no kernel produces


def _qkv(side, seed):
    B, T, d, _ = side
    return au.random_inputs(B, T, d, seed)[0].to(torch.bfloat16).to(DEV)


def _mask(side, variant):
    B, T, _, _ = side
    m = au.key_mask(variant, B, T)
    return None if m is None else m.to(DEV)


def _guarded(side):
    B, T, d, _ = side
    return torch.full((B * T + au.GUARD_ROWS, d), PATTERN, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _pair(s0, q0, m0, s1, q1, m1):
    """-> (o0, o1) [B T, d] of the pair launch, written into guarded buffers whose guard rows are checked here"""
    import cmh_native as N
    g0, g1 = _guarded(s0), _guarded(s1)
    n0, n1 = s0[0] * s0[1], s1[0] * s1[1]
    got = N.attention_pair(q0, s0[0], s0[1], s0[3], q1, s1[0], s1[1], s1[3], m0, m1, out=(g0, g1))
    assert got is not None, ("the launcher declined a pair it has a kernel for", s0, s1)
    torch.cuda.synchronize()
    for name, g, n in (("o0", g0, n0), ("o1", g1, n1)):
        bits = g.view(torch.int16)
        assert bool((bits[n:] == PATTERN).all()), f"{s0} | {s1}: {name} was written behind row B T"
        assert not bool((bits[:n] == PATTERN).any()), f"{s0} | {s1}: an element of {name} was never written"
    return g0[:n0], g1[:n1]


@pytest.fixture(scope="module")
def singles():
    """cmh_attention's outputs, computed once per (side, seed, variant) and shared"""
    import cmh_native as N
    cache = {}

    def get(side, seed, variant):
        key = (side, seed, variant)
        if key not in cache:
            B, T, _, causal = side
            cache[key] = N.attention(_qkv(side, seed), B, T, causal, _mask(side, variant))
        return cache[key]
    return get


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_pair_launch_has_the_two_single_launches_bits(row, singles):
    s0, s1 = ROWS[row]
    seed0, seed1 = 100 + row, 200 + row
    q0, q1 = _qkv(s0, seed0), _qkv(s1, seed1)
    for variant in SIDE1_VARIANTS:
        if variant == "tile" and s1[1] <= 16:
            continue
        o0, o1 = _pair(s0, q0, None, s1, q1, _mask(s1, variant))
        assert torch.equal(o0, singles(s0, seed0, "none")), (row, variant, "side 0")
        assert torch.equal(o1, singles(s1, seed1, variant)), (row, variant, "side 1")


def test_pair_launch_with_the_sides_swapped(singles):
    s1, s0 = ROWS[0]                                       # the five-tile problem as side 0
    seed0, seed1 = 200, 100                                # (the seeds of row 0: the single launches are shared with the test above)
    q0, q1 = _qkv(s0, seed0), _qkv(s1, seed1)
    for variant in SIDE1_VARIANTS:
        o0, o1 = _pair(s0, q0, _mask(s0, variant), s1, q1, None)
        assert torch.equal(o0, singles(s0, seed0, variant)), variant
        assert torch.equal(o1, singles(s1, seed1, "none")), variant


@pytest.mark.parametrize("what,s0,s1,dtype", [
    ("T = 81", (3, 50, 192, 0), (5, 81, 128, 1), torch.bfloat16),
    ("T = 129", (3, 50, 192, 0), (2, 129, 128, 1), torch.bfloat16),
    ("T = 81 as side 0", (5, 81, 128, 1), (3, 50, 192, 0), torch.bfloat16),
    ("f32", (3, 50, 192, 0), (5, 77, 128, 1), torch.float32)])
def test_the_launcher_declines_what_it_has_no_kernel_for(what, s0, s1, dtype):
    """the "launch singly" code and no launch: both outputs keep their prefill"""
    import cmh_native as N
    q0, q1 = (au.random_inputs(s[0], s[1], s[2], 7)[0].to(dtype).to(DEV) for s in (s0, s1))
    idt, pattern = (torch.int16, PATTERN) if dtype == torch.bfloat16 else (torch.int32, 0x7FC0BEEF)
    outs = tuple(torch.full((s[0] * s[1], s[2]), pattern, dtype=idt, device=DEV).view(dtype) for s in (s0, s1))
    assert N.attention_pair(q0, s0[0], s0[1], s0[3], q1, s1[0], s1[1], s1[3], out=outs) is None, what
    torch.cuda.synchronize()
    assert all(bool((o.view(idt) == pattern).all()) for o in outs), what + ": declined, but something was written"


@pytest.mark.parametrize("T", [65, 77, 80])
def test_five_tile_form_against_fp64_and_the_visible_set(T):
    """attention_mfma_body<5> as side 1 of a pair launch (side 0: the image shape), over shape x causal x mask variant of
    attnutil.cases(T): random operands against the fp64 statement on the same rounded operands, then Q = 0 with the V that spells
    the key index - the set of visible keys read off the output exactly, for every (batch, head, query)"""
    s0 = (3, 50, 192, 0)
    q0 = _qkv(s0, 5)
    worst = [0.0, 0.0]
    for B, d, causal, variant in au.cases(T):
        s1 = (B, T, d, causal)
        what = f"T={T} B={B} d={d} causal={causal} {variant}"
        mask = au.key_mask(variant, B, T)
        md = None if mask is None else mask.to(DEV)
        vis = au.visible(B, T, causal, mask, DEV)
        q1 = au.random_inputs(B, T, d, 1000 * T + 100 * B + d + 7 * causal + au.VARIANTS.index(variant))[0].to(torch.bfloat16).to(DEV)
        _, o = _pair(s0, q0, None, s1, q1, md)
        assert bool(torch.isfinite(o).all()), what
        ref, _ = au.reference_forward(q1, B, T, vis)
        torch.testing.assert_close(o.double(), ref, rtol=1e-2, atol=1e-2, msg=lambda m: f"{what}: {m}")
        emax, enorm = au.slice_errors(o.double(), ref, d)
        worst = [max(worst[0], emax), max(worst[1], enorm)]
        print(f"five-tile {what}: {emax:.2e} of max, {enorm:.2e} of 2-norm")
        assert emax <= SLICE_MAX and enorm <= SLICE_NORM, (what, emax, enorm)
        qd = au.decode_inputs(B, T, d, 3).to(torch.bfloat16).to(DEV)
        _, od = _pair(s0, q0, None, s1, qd, md)
        au.decode_check(od, B, T, au.visible(B, T, causal, mask), what)
    print(f"five-tile T={T}: worst {worst[0]:.2e} of max, {worst[1]:.2e} of 2-norm")


# ---- packed rows: seq_off through the five-tile side, by way of encode_pair -------------------------------------------------------
def _pair_cfg(L):
    # attnutil.pack_cfg()'s text tower at context length L beside an image tower whose attention pairs with it: 37 tokens (four key
    # tiles; the tiny tower's 5 tokens would take the two-tile form, and (5, 2) is not a pair the launcher has), width 256 like
    # the text tower's (lock-step needs the two residual streams to be of one kind)
    return dict(au.pack_cfg(), context_length=L, image_resolution=192, vision_width=256)


@pytest.mark.parametrize("L,mode", [(77, "bf16"), (80, "bf16"), (77, "fp8")])
def test_encode_pair_on_packed_captions_equals_the_single_towers(L, mode):
    """encode_pair (pair launch: image four tiles, text five tiles on seq_off - a 3-token caption, a full-length one) against
    encode_image + encode_text (attention_mfma_kernel<4> and <6>), bit for bit; fp8: the e4m3 output of both sides"""
    from test_gpu_clip import _clip
    cfg = _pair_cfg(L)
    text_np = au.pack_captions(L, cfg["vocab_size"])
    assert int(text_np.argmax(1).min()) == 2 and not bool((text_np[2] == 0).any())
    m = _clip(cfg, 7, "bf16")
    m.assume_frozen = True
    img = torch.from_numpy(recipe.images(au.PACK_B, cfg["image_resolution"], 5)).to(DEV)
    txt = torch.from_numpy(text_np).to(DEV)
    if mode == "fp8":
        m.calibrate_fp8(img, txt)
        m.set_gemm_dtype("fp8")
    with torch.no_grad():
        for pack in (True, False):
            m.pack_text = pack
            ref = (m.encode_image(img).clone(), m.encode_text(txt).clone())
            got = tuple(t.clone() for t in m.encode_pair(img, txt))
            for r, g in zip(ref, got):
                assert bool(torch.isfinite(r).all()) and float(r.abs().sum()) > 0
                assert torch.equal(r, g), (L, mode, pack)
