"""Every attention kernel form at its tile edges, under key-padding masks of every shape, and on packed rows.

csrc/attention.hip and csrc/attention_bwd.hip compile fifteen forms and pick one by T and dtype (tests/attnutil.py restates the choice;
tests/test_attention_cases_host.py checks the tables).  Per length of attnutil.EDGE_T and per mode, over shape x causal x mask variant:
  (a) random operands against the fp64 statement of the op on the same rounded operands, with the bounds the suite already uses
      (forward: test_gpu_kernels.test_attention; slices and backward: test_gpu_attention_long / test_attention_backward_at_tower_shapes),
      finite outputs, equal bits from a second call, exact zeros in dK / dV for keys that no query sees;
  (b) Q = 0 and a V that spells the key index: the set of visible keys is read off the output exactly, for every (batch, head, query) -
      random data at rtol 1e-2 does not notice one dropped key in a hundred;
  (c) a query with ONE visible key returns that key's V row bit for bit (p = 1, l = 1: nothing rounds in any form);
  (d) rows behind B T keep their bits, in both directions;
  (e) packed rows (seq_off) through every form, by way of a small text tower with context_length 160."""
import numpy as np
import pytest
import torch

import attnutil as au
import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLICE_MAX, SLICE_NORM = 1e-2, 4e-3          # of a slice's max / 2-norm (bf16), as test_gpu_attention_long._check_slices


def _dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _seed(T, B, d, causal, variant):
    return 1000 * T + 100 * B + d + 7 * causal + au.VARIANTS.index(variant)


@pytest.mark.parametrize("T", au.EDGE_T)
@pytest.mark.parametrize("mode", au.MODES)
def test_random_operands_against_fp64(T, mode):
    """(a) and (c).  The reference's O in D = rowsum(dO o O) is what the form reads: the GPU forward's o for the whole-sequence VALU
    backward (f32 at T <= 128, bf16 at 97..128), the exact P V (as D = rowsum(P o dP), the kernels' own expression) for the bf16 MFMA
    backward and the tiled one.  A slice whose reference is exactly zero (every query of the case has one visible key: dS = 0) must be
    exactly zero.
    bf16 bounds per slice: 1e-2 of the slice's max and 4e-3 of its 2-norm, unchanged from the long-sequence tests.  The MFMA forward
    rounds P to bf16 for the P V product and then the output - two independent roundings of at most 2^-8, about 2^-9 in the mean - and
    stays near 2^-9 of the 2-norm; nobody had measured that below T = 129.  Worst over all cases of a form on MI355X, as share of the
    slice's max / of its 2-norm:
      forward   attention_mfma_kernel<2> 3.8e-3 / 2.1e-3   <4> 3.9e-3 / 2.1e-3   <6> 3.6e-3 / 2.2e-3   <8> 3.4e-3 / 2.2e-3
                attention_kernel<bf16_t> (T = 129, 160) 3.6e-3 / 1.7e-3          attention_kernel<float> 8.1e-7 / 3.2e-7
      backward  attention_bwd_mfma_kernel<1> 5.1e-3 / 2.6e-3   <2> 4.9e-3 / 2.5e-3   <3> 4.6e-3 / 2.5e-3   <4> 4.6e-3 / 2.5e-3
                <5> 6.0e-3 / 2.5e-3   <6> 5.2e-3 / 2.4e-3   attention_bwd_kernel<bf16_t> 3.7e-3 / 1.8e-3
                attention_bwd_tiled_kernel<bf16_t> 3.7e-3 / 1.8e-3   attention_bwd_kernel<float> 6.1e-6 / 1.1e-6
                attention_bwd_tiled_kernel<float> 9.5e-7 / 3.7e-7
    The test prints its own figures (pytest -s)."""
    import backward_ops as Bo
    import cmh_native as N
    dt = _dtype(mode)
    worst = {"fwd": [0.0, 0.0], "bwd": [0.0, 0.0]}
    for B, d, causal, variant in au.cases(T):
        what = f"T={T} {mode} B={B} d={d} causal={causal} {variant}"
        qkv, dout = au.random_inputs(B, T, d, _seed(T, B, d, causal, variant))
        qd, dd = qkv.to(dt).to(DEV), dout.to(dt).to(DEV)
        mask = au.key_mask(variant, B, T)
        md = None if mask is None else mask.to(DEV)
        vis = au.visible(B, T, causal, mask, DEV)
        o = N.attention(qd, B, T, causal, md)
        dqkv = Bo.attention_backward(qd, o, dd, B, T, causal, md)
        assert torch.equal(o, N.attention(qd, B, T, causal, md)), what + ": the forward is not deterministic"
        assert torch.equal(dqkv, Bo.attention_backward(qd, o, dd, B, T, causal, md)), what + ": the backward is not deterministic"
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(dqkv).all()), what
        ref_o, p = au.reference_forward(qd, B, T, vis)
        ref_g = au.reference_backward(qd, dd, p, B, T, o_for_d=o if au.backward_reads_o(T, mode) else None)
        got_o, got_g = o.double(), dqkv.double()
        if mode == "f32":
            torch.testing.assert_close(got_o, ref_o, rtol=1e-5, atol=1e-5, msg=lambda m: f"{what} forward: {m}")
            torch.testing.assert_close(got_g, ref_g, rtol=1e-4, atol=1e-5, msg=lambda m: f"{what} backward: {m}")
        else:
            torch.testing.assert_close(got_o, ref_o, rtol=1e-2, atol=1e-2, msg=lambda m: f"{what} forward: {m}")
        for name, got, ref in (("fwd", got_o, ref_o), ("bwd", got_g, ref_g)):
            emax, enorm = au.slice_errors(got, ref, d, skip_below=1e-6 if mode == "f32" else 0.0)      # f32: reported, bounded above
            worst[name] = [max(worst[name][0], emax), max(worst[name][1], enorm)]
            if mode == "bf16":
                assert emax <= SLICE_MAX and enorm <= SLICE_NORM, (what, name, emax, enorm)
        # keys that no query sees (masked by key_padding_mask; under `lead`, batch row 2: all but the last): P = 0 exactly in every form
        unseen = ~vis.any(1)                                                     # [B, key]
        if bool(unseen.any()):
            assert float(dqkv.view(B, T, 3, d)[:, :, 1:][unseen].abs().max()) == 0.0, what + ": dK / dV of an unseen key"
        # (c) one visible key: the output row is that key's V row, bit for bit
        one = vis.sum(-1) == 1                                                   # [B, query]
        if variant == "lead" and B > 2:
            assert bool(one[2].all())
        if bool(one.any()):
            key = vis.float().argmax(-1)                                         # [B, query]
            v = qd.view(B, T, 3, d)[:, :, 2]
            want = torch.gather(v, 1, key[:, :, None].expand(B, T, d))
            assert torch.equal(o.view(B, T, d)[one], want[one]), what + ": a query with one visible key does not return that key's V"
    print(f"edges T={T} {mode}: forward {au.forward_form(T, mode)} worst {worst['fwd'][0]:.2e} of max, {worst['fwd'][1]:.2e} of 2-norm; "
          f"backward {au.backward_form(T, mode)} worst {worst['bwd'][0]:.2e} of max, {worst['bwd'][1]:.2e} of 2-norm")


@pytest.mark.parametrize("T", au.EDGE_T)
@pytest.mark.parametrize("mode", au.MODES)
def test_visible_set_decode(T, mode):
    """(b): the decoded set of visible keys equals the expected one for every (batch, head, query), exactly"""
    import cmh_native as N
    resid = 0.0
    for B, d, causal, variant in au.cases(T):
        mask = au.key_mask(variant, B, T)
        qd = au.decode_inputs(B, T, d, _seed(T, B, d, causal, variant)).to(_dtype(mode)).to(DEV)
        o = N.attention(qd, B, T, causal, None if mask is None else mask.to(DEV))
        resid = max(resid, au.decode_check(o, B, T, au.visible(B, T, causal, mask), f"T={T} {mode} B={B} d={d} causal={causal} {variant}"))
    print(f"decode T={T} {mode} {au.forward_form(T, mode)}: largest distance to an integer {resid:.3f} (threshold 0.5)")


@pytest.mark.parametrize("T", au.GUARD_T)
@pytest.mark.parametrize("mode", au.MODES)
def test_rows_behind_the_batch_keep_their_bits(T, mode):
    """(d): o and dqkv are 64 rows longer than B T and prefilled with a NaN pattern no kernel produces; the launches overwrite every
    element below row B T and nothing behind it"""
    import cmh_native as N
    B, d = au.MAIN_SHAPE
    dt, code = _dtype(mode), N.BF16 if mode == "bf16" else N.F32
    idt, pattern = (torch.int16, 0x7FC1) if mode == "bf16" else (torch.int32, 0x7FC0BEEF)
    dev = torch.device(DEV)
    for causal, variant in ((0, "none"), (1, "tail"), (0, "lead")):
        what = f"T={T} {mode} causal={causal} {variant}"
        qkv, dout = au.random_inputs(B, T, d, _seed(T, B, d, causal, variant))
        qd, dd = qkv.to(dt).to(DEV), dout.to(dt).to(DEV)
        mask = au.key_mask(variant, B, T)
        kpm = None if mask is None else mask.to(torch.uint8).to(DEV)
        o = torch.full((B * T + au.GUARD_ROWS, d), pattern, dtype=idt, device=DEV).view(dt)
        dqkv = torch.full((B * T + au.GUARD_ROWS, 3 * d), pattern, dtype=idt, device=DEV).view(dt)
        N.check(N.lib().cmh_attention(code, N.ptr(qd), N.ptr(o), B, T, d, causal, N.ptr(kpm), N.stream_ptr(dev)), "cmh_attention")
        N.check(N.lib().cmh_attention_backward(code, N.ptr(qd), N.ptr(o), N.ptr(dd), N.ptr(dqkv), B, T, d, causal, N.ptr(kpm),
                                               N.stream_ptr(dev)), "cmh_attention_backward")
        torch.cuda.synchronize()
        for name, t in (("o", o), ("dqkv", dqkv)):
            bits = t.view(idt)
            assert bool((bits[B * T:] == pattern).all()), f"{what}: {name} was written behind row B T"
            assert not bool((bits[:B * T] == pattern).any()), f"{what}: an element of {name} was never written"


# ---- (e) packed rows ---------------------------------------------------------------------------------------------------------------
def _captions(L):
    cfg = au.pack_cfg()
    text_np = au.pack_captions(L, cfg["vocab_size"])
    last = np.array([np.flatnonzero(r != 0).max() for r in text_np])
    keep = torch.from_numpy(np.arange(L)[None, :] <= np.maximum(last, text_np.argmax(1))[:, None]).to(DEV)
    assert int(text_np.argmax(1).min()) == 2 and not bool((text_np[2] == 0).any()) and 0 < int((~keep).sum()) < au.PACK_B * L
    return cfg, text_np, keep


def _mith_clip(cfg, mode, seed=7):
    from model.MITH import build_model
    return build_model({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, seed).items()}).to(DEV).float().set_gemm_dtype(mode)


@pytest.mark.parametrize("L", au.PACK_L)
@pytest.mark.parametrize("mode", au.MODES)
def test_packed_pooled_text_encode_keeps_the_bits(L, mode):
    """cmh_text_encode_packed == cmh_text_encode bit for bit (the invariant of test_gpu_clip.test_packed_text_encode_is_bit_identical)
    with the causal attention on seq_off in the form this L selects; f32: the dense result against the oracle"""
    from test_gpu_clip import _clip
    cfg, text_np, _ = _captions(L)
    m = _clip(cfg, 7, mode)
    m.assume_frozen = True
    t = torch.from_numpy(text_np).to(DEV)
    with torch.no_grad():
        m.pack_text = False
        dense = m.encode_text(t)
        m.pack_text = True
        packed = m.encode_text(t)
    rows, total = m.last_text_rows
    assert rows == int((text_np.argmax(1) + 1).sum()) and total == au.PACK_B * L and rows < total
    assert bool(torch.isfinite(dense).all()) and torch.equal(dense, packed)
    if mode == "f32":
        from oracle import clip_oracle as co
        np.testing.assert_allclose(dense.cpu().numpy(), co.encode_text(recipe.clip_state_dict(cfg, 7), text_np), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("L", au.PACK_L)
@pytest.mark.parametrize("mode", au.MODES)
def test_packed_token_encode_keeps_the_bits(L, mode):
    """causal + key-padding mask + seq_off together (test_gpu_mith.test_token_packing_keeps_the_bits_of_every_position_somebody_reads
    without its HashingModel part): kept positions carry the dense call's bits, skipped ones are zeros, the EOT rows are equal"""
    import mith_ops as M
    from test_gpu_mith import tt
    cfg, text_np, keep = _captions(L)
    clip = _mith_clip(cfg, mode)
    text, kpm = tt(text_np), tt(text_np == 0)
    with torch.no_grad():
        dense, rows_d = M.text_encode_tokens(clip, text, kpm)
        packed, rows_p = M.text_encode_tokens(clip, text, kpm, padded_unused=True)
    assert torch.equal(rows_d, rows_p) and bool(torch.isfinite(dense[keep]).all())
    assert torch.equal(packed[keep], dense[keep])
    assert float(packed[~keep].abs().max()) == 0.0
    flat = lambda tok: tok.reshape(au.PACK_B * L, -1)[rows_d.long()]
    assert torch.equal(flat(packed), flat(dense))


@pytest.mark.parametrize("L", au.PACK_TRAIN_L)
@pytest.mark.parametrize("mode", au.MODES)
def test_packed_training_matches_the_dense_tape(L, mode):
    """test_gpu_mith.test_token_packing_under_training_matches_the_dense_tape with its own bounds, at lengths whose backward runs
    attention_bwd_mfma_kernel<3> / <5>, the whole-sequence VALU kernel and the tiled kernel on seq_off"""
    from test_gpu_mith import tt
    cfg, text_np, keep = _captions(L)
    text, kpm = tt(text_np), tt(text_np == 0)
    gen = torch.Generator().manual_seed(5)
    G = torch.randn(L, au.PACK_B, 512, generator=gen).to(DEV) * keep.T[:, :, None]          # no weight on the padded positions
    Ge = torch.randn(au.PACK_B, 512, generator=gen).to(DEV)
    res = {}
    for packed in (False, True):
        clip = _mith_clip(cfg, mode)
        clip.padded_tokens_unused = packed
        seq_t, _, _, eos = clip.encode_text(text, kpm)
        ((seq_t * G).sum() + (eos * Ge).sum()).backward()
        res[packed] = (seq_t.detach().clone(), eos.detach().clone(), {n: p.grad.detach().clone() for n, p in clip.named_parameters() if p.grad is not None})
    assert torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][0][keep.T], res[False][0][keep.T]) and float(res[True][0][~keep.T].abs().max()) == 0.0
    assert res[True][2].keys() == res[False][2].keys() and len(res[True][2]) > 20
    tol = 2e-5 if mode == "f32" else 4e-3
    for name, ref in res[False][2].items():
        got = res[True][2][name]
        assert bool(torch.isfinite(got).all()), name
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
        assert err < tol, (name, err)
