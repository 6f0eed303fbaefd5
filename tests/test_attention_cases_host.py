"""The case tables of tests/attnutil.py, checked on the CPU: every kernel form of csrc/attention.hip / csrc/attention_bwd.hip is
selected at both of its edges, no case holds a query without a visible key (so the GPU tests may assert finiteness on every row),
and the visible-set decode check notices each of four deliberate defects of the fp64 reference."""
import pytest
import torch

import attnutil as au

# (form, mode, first length that selects it, last one; None = open-ended): launch_attention_varlen / launch_attention_backward
FORM_RANGES = [("attention_mfma_kernel<2>", "bf16", 1, 32), ("attention_mfma_kernel<4>", "bf16", 33, 64),
               ("attention_mfma_kernel<6>", "bf16", 65, 96), ("attention_mfma_kernel<8>", "bf16", 97, 128),
               ("attention_kernel<bf16_t>", "bf16", 129, None), ("attention_kernel<float>", "f32", 1, None)] + [
               (f"attention_bwd_mfma_kernel<{n}>", "bf16", 16 * n - 15, 16 * n) for n in range(1, 7)] + [
               ("attention_bwd_kernel<bf16_t>", "bf16", 97, 128), ("attention_bwd_kernel<float>", "f32", 1, 128),
               ("attention_bwd_tiled_kernel<float>", "f32", 129, None), ("attention_bwd_tiled_kernel<bf16_t>", "bf16", 129, None)]


def test_every_form_is_selected_at_both_of_its_edges():
    """the fifteen rows of the form table (the tiled backward is one row, two instantiations): each is selected by at least two of the
    lengths, one at its upper edge and one just past the previous form's edge"""
    assert sorted(f for f, *_ in FORM_RANGES) == sorted(au.FORWARD_FORMS + au.BACKWARD_FORMS) and len(FORM_RANGES) == 16
    for form, mode, lo, hi in FORM_RANGES:
        select = au.backward_form if "bwd" in form else au.forward_form
        hits = [T for T in au.EDGE_T if select(T, mode) == form]
        assert len(hits) >= 2 and hits[0] == lo and (hi is None or hits[-1] == hi), (form, hits)
        assert hi is None or hi + 1 in au.EDGE_T, form
        assert all(lo <= T and (hi is None or T <= hi) for T in hits), (form, hits)
    for T in au.EDGE_T:
        for mode in au.MODES:
            assert au.forward_form(T, mode) in au.FORWARD_FORMS and au.backward_form(T, mode) in au.BACKWARD_FORMS
    assert {T for T in au.EDGE_T if au.backward_reads_o(T, "bf16")} == {97, 112, 127, 128}
    assert {T for T in au.EDGE_T if au.backward_reads_o(T, "f32")} == {T for T in au.EDGE_T if T <= 128}
    assert set(au.EXTRA_T) | set(au.GUARD_T) <= set(au.EDGE_T)


def test_mask_variants_are_what_the_table_says():
    m = au.key_mask("tail", 5, 33)
    assert [int((~r).sum()) for r in m] == [1, 33, 17, 1, 33] and bool((~m[2][:17]).all())
    m = au.key_mask("holes", 3, 17)
    assert m[1].nonzero().flatten().tolist() == [1, 4, 7, 10, 13, 16] and torch.equal(m[0], m[2])
    m = au.key_mask("tile", 3, 97)
    assert [r.nonzero().flatten()[[0, -1]].tolist() for r in m] == [[16, 31], [32, 63], [16, 95]]
    m = au.key_mask("tile", 3, 17)
    assert m[0].nonzero().flatten().tolist() == [16] and not bool(m[1].any()) and m[2].nonzero().flatten().tolist() == [16]
    m = au.key_mask("lead", 3, 33)
    assert [int(r.sum()) for r in m] == [16, 32, 32] and not bool(m[:, 32].any())
    m = au.key_mask("lead", 3, 2)
    assert m.tolist() == [[True, False]] * 3
    assert au.key_mask("none", 3, 9) is None
    assert au.variants(16, 0) == ["none", "tail", "holes", "lead"] and au.variants(1, 0) == ["none", "tail", "holes"]
    assert au.variants(17, 1) == ["none", "tail", "holes", "tile"]


@pytest.mark.parametrize("T", au.EDGE_T)
def test_every_query_has_a_visible_key(T):
    """for every (shape, causal, variant) at this length: at least one visible key per query row, a finite fp64 forward and backward,
    `lead` never together with causal, and key 0 visible in every variant that is: zero rows need excluding on the GPU"""
    cases = au.cases(T)
    assert len(cases) >= 6 and {(B, d) for B, d, _, _ in cases} == set(au.shapes(T))
    for B, d, causal, variant in cases:
        what = (T, B, d, causal, variant)
        assert not (causal and variant == "lead"), what
        mask = au.key_mask(variant, B, T)
        if causal and mask is not None:
            assert not bool(mask[:, 0].any()), what
        vis = au.visible(B, T, causal, mask)
        assert int(vis.sum(-1).min()) >= 1, what
        if variant == "lead" and B > 2:
            assert int(vis[2].sum(-1).max()) == 1 and bool(vis[2, :, T - 1].all()), what
        qkv, dout = au.random_inputs(B, T, d, T + B)
        o, p = au.reference_forward(qkv, B, T, vis)
        dqkv = au.reference_backward(qkv, dout, p, B, T)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(dqkv).all()), what
        assert o.shape == (B * T, d) and dqkv.shape == (B * T, 3 * d)


def test_reference_backward_is_autograd():
    """the closed-form fp64 backward is the derivative of the fp64 forward (torch autograd), with D from the exact O and from a given o"""
    B, T, d = 2, 19, 128
    qkv, dout = au.random_inputs(B, T, d, 3)
    vis = au.visible(B, T, 1, au.key_mask("holes", B, T))
    x = qkv.double().requires_grad_(True)
    o, p = au.reference_forward(x, B, T, vis)
    o.backward(dout.double())
    torch.testing.assert_close(au.reference_backward(qkv, dout, p.detach(), B, T), x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(au.reference_backward(qkv, dout, p.detach(), B, T, o_for_d=o.detach()), x.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T", au.EDGE_T)
def test_decode_reads_the_visible_set_off_the_clean_reference(T):
    for B, d, causal, variant in au.cases(T):
        vis = au.visible(B, T, causal, au.key_mask(variant, B, T))
        for rounded in (False, True):                      # the bf16 mode's operands and a bf16 output
            qkv = au.decode_inputs(B, T, d, T)
            o, _ = au.reference_forward(qkv.bfloat16() if rounded else qkv, B, T, vis)
            resid = au.decode_check(o.bfloat16() if rounded else o, B, T, vis, (T, B, d, causal, variant))
            assert resid < 0.03


# (defect, causal, variant): every defect where it changes the visible set; short_sequence and drop_one_key at every kind of mask
BITE = [("drop_one_key", 0, "none"), ("drop_one_key", 1, "tail"), ("drop_one_key", 0, "tile"),("drop_one_key", 1, "holes"),
        ("causal_off_by_one", 1, "none"), ("causal_off_by_one", 1, "tile"),
        ("next_rows_mask", 0, "tail"), ("next_rows_mask", 1, "tail"), ("next_rows_mask", 0, "tile"), ("next_rows_mask", 1, "tile"),
        ("short_sequence", 0, "none"), ("short_sequence", 1, "none"), ("short_sequence", 0, "tile"), ("short_sequence", 0, "lead")]


@pytest.mark.parametrize("T", [17, 33, 97, 128, 129, 160])
@pytest.mark.parametrize("defect,causal,variant", BITE)
def test_decode_fails_on_a_seeded_defect(defect, causal, variant, T):
    """one dropped key for one query, key < query for the causal bound, batch row b under row b + 1's mask, Tn = T - 1: each must fail
    the decode assertion that the clean reference (test above) passes - also after rounding the output to bf16"""
    for B, d in au.shapes(T):
        mask = au.key_mask(variant, B, T)
        vis = au.visible(B, T, causal, mask)
        bad = au.DEFECTS[defect](B, T, causal, mask)
        assert not torch.equal(bad, vis)
        o, _ = au.reference_forward(au.decode_inputs(B, T, d, T), B, T, bad)
        for out in (o, o.bfloat16()):
            with pytest.raises(AssertionError):
                au.decode_check(out, B, T, vis, defect)
