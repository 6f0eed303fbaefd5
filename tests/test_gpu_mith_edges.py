"""The MITH head and loss kernels (csrc/mith.hip) and the DMsH-LN multi-similarity loss (csrc/msl.hip msl_*) at their compile-time
limits, lane / slice / quarter / chunk edges and decision edges, through the wrappers the trainer uses (mith_ops, mith_train_ops.*Fn,
MultiSimilarityLoss), against the float64 references of tests/mithedgeutil.py (anchored to the reference project's recorded values,
checked for settled decisions and for sensitivity to each edge by tests/test_mith_edges_host.py).

Bound, the one of tests/test_gpu_loss_edges.py: |loss - ref| <= 1e-5 max(1, |ref|); every tensor max |got - ref| <= 1e-4 max |ref| (per
row where the table says so); where the reference is exactly zero the kernel's output is exactly zero.  The upstream gradient is 1.7
or 0.3, never 1.  Every case runs twice on fresh tensors: forward tensors and gradients must be equal bit for bit, the multi-similarity
loss too; the losses that finish through f64 atomics (Bayesian, InfoNCE, sq_diff) agree within the bound.

Which kernel form each case reaches:
  LTA (B, Ltot, l0, L, K, D, top_k, mask): lta_kernel / lta_bwd_kernel, grid (B, ceil(D / 256))
    (3, 80, 0, 80, 128, 260, 8, yes)  kLtaMaxL and kLtaMaxK; the second column block holds 4 columns; sample 1 fully masked (exact zeros),
                                      one token masked in sample 2
    (2, 50, 1, 49, 16, 512, 8, no)    row0 = b Ltot + 1: the CLS row is skipped; the memset branch of cmh_mith_lta_backward (the entry is
                                      also called on a NaN-filled dtokens: row 0 must come back as exact zeros)
    (5, 7, 0, 7, 4, 65, 1, yes)       one quad of concepts, top_k = 1, D below one block; tokens without a positive
    (2, 9, 2, 6, 12, 64, 3, yes)      by hand: the third largest value twice and three times (4 and 5 kept), the largest twice (3 kept), two
                                      positives, none, two concepts without a survivor, a masked token, l0 + L < Ltot
  BitwiseHashing (B, K, D): bitwise_hash_kernel (a wave per (b, k), float4 trips of 256), bithash_dx_kernel, bithash_dw_kernel (K, ceil(D / 64))
    (3, 5, 260)     15 rows: the last workgroup holds three; the second float4 trip is one lane; dw's fifth column block holds 4 columns
    (1, 1, 4)       the smallest shape: one lane, three empty sample quarters
    (5, 16, 512)    sample quarters of 2 / 2 / 1 / 0
    (261, 4, 68)    66 samples per wave: the second db lane trip, the 4-way unroll's remainder of 2; the second column block holds 4 columns
  L2 normalize (R, D): l2norm_rows_kernel / l2norm_bwd_kernel, a wave per row   (5, 65) one row in the last workgroup, one column past a
                  wave;  (3, 7) fewer columns than lanes;  (4, 128) row 1 zero, row 2 = 1e-20 x row 3: the eps-clamped rows, per row
  mith_mix n = 257 (exact zeros of both kinds, both signs, one element in the second block); add_positional (3, 5, 7); gelu n = 257 (0, +-6);
  sq_diff_sum n = 1, n = 262 144 + 257 (the grid-stride trip of 257), a == b (value 0, zero gradients), da only, db only
  Bayesian loss (Mb, B, K, C): forward bayes_mfma_kernel (K, C <= 128) else bayes_kernel; backward bayes_bwd_mfma_kernel (K % 16 == 0 and
  C <= 128) else bayes_bwd_kernel, then bayes_bwd_reduce_kernel
    (1023, 17, 16, 5)    MFMA both ways; forward in ONE slice; the second batch tile holds one row
    (1025, 17, 16, 5)    forward in sixteen slices of 65, the last holding 50
    (5, 3, 16, 1)        backward slices 5 .. 15 are empty
    (10257, 17, 16, 5)   642 rows per slice: the second LDS chunk of bayes_bwd_mfma_kernel holds two
    (33, 5, 5, 1)        forward MFMA with K % 4 != 0 (a partly filled operand quad); backward VALU
    (300, 37, 24, 21)    backward VALU: K below a wave, quarters of 5 / 5 / 5 / 4 rows with the unroll's remainder
    (70, 9, 128, 130)    both VALU kernels (C > 128): the second K half full, C in three lane trips (the last two classes)
    Mb = 65 537          the backward is refused by the library (4097 rows per slice), nothing is launched
  InfoNCE (R, G, D): D % 64 == 0: nce_scores / nce_lse / nce_weights / nce_grad<false, true>; else row_ce / row_lse / info_nce_bwd
    (130, 65, 64)    tiles: a fifth 16-tile and a second 64-block of one row and column; row quarters 17 / 17 / 17 / 14
    (10, 5, 64)      tiles: the fourth quarter is empty
    (130, 65, 100)   rows: the second lane trip holds one candidate
    (12, 1, 65)      rows: groups of one: loss 0 and zero gradients, exactly
  Multi-similarity loss (B, K, Kl), feat2 None (msl_bwd_cols accumulates) and feat2 given: msl_rows, msl_sum, msl_bwd_rows, msl_bwd_cols
    (257, 65, 33)     the second j trip holds one entry; B % 4 = 1: the unrolled sums take their remainder
    (300, 257, 5)     the second k trip holds one column
    (7, 1024, 1023)   the limits of K and Kl; a skipped row
    (65, 16, 3)       both mining cuts well populated; the negative term weighs in the gradient
    (5, 16, 3)        row 0 of the features zero: the eps-clamped row (its gradient is ~1e12: compared per row)

Measured on MI355X, worst over a family's cases (loss: |got - ref| / max(1, |ref|); tensors: max |got - ref| / max |ref|, per row for L2
normalize and the (5, 16, 3) multi-similarity case), next to the worst e32 of the family printed by tests/test_mith_edges_host.py:
  LTA             merge 1.9e-07 (e32 1.8e-07)   dtokens 1.4e-07 (1.6e-07)
  BitwiseHashing  y 2.2e-07 (4.5e-07)   dx 8.9e-07 (8.9e-07)   dw 9.3e-07 (9.3e-07)   db 9.1e-07 (9.1e-07)      the three at (1, 1, 4): one product, the
                  rounding of tanh' alone
  L2 normalize    y 1.1e-07 (7.4e-08)   dx 1.8e-07 (1.4e-07)
  elementwise     mith_mix B exact, H 3.1e-08   add_positional y 3.7e-08 dx 6.8e-08   gelu y 3.2e-08 (1.1e-07) dx 9.1e-08 (1.7e-07)
  sq_diff_sum     sum 1.3e-08 (2.6e-08)   da, db 1.1e-07 (one rounding of a - b)
  Bayesian loss   loss 5.7e-08 (1.3e-07)   dbatch 2.0e-07 (7.9e-07)      the largest single ratio: loss at (70, 9, 128, 130), 5 x its e32 of 1.1e-08
  InfoNCE         loss 5.9e-08 (7.8e-08)   da 4.4e-07 (3.4e-07)   db 3.8e-07 (4.0e-07)
  MSL             loss 5.6e-08 (8.3e-08)   dfeats 2.3e-07 (7.7e-07)   dfeat2 2.2e-07 (6.0e-07)
No case is above 5 x its e32 (64 x would need explaining); the slowest case takes 1.2 s (the first launch of the module), the others
under 0.1 s.
Out of scope: the CMH_BAYES_MFMA=0 switch (read once per process; the VALU forms are reached by shape above), the bf16 GEMM modes of
HashingModel, twdh_* and the forward small-linear kernels."""
import pytest
import torch

import mithedgeutil as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(what, losses=(), tensors=(), rows=False):
    """losses: (name, got, ref); tensors: (name, got, ref).  Prints every figure, then asserts the bounds and the exact zeros."""
    measure = U.per_row if rows else U.of_max
    le = [(n, U.loss_err(g, r)) for n, g, r in losses]
    te = [(n, measure(g, r)) for n, g, r in tensors]
    print(f"measured {what}: " + " ".join(f"{n} {e:.1e}" for n, e in le + te))
    for n, g, r in tensors:
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), (what, n)
        assert not bool(g.detach().cpu()[r == 0].any()), (what, n, "exact zeros")
    for n, e in le:
        assert e <= U.LOSS_BOUND, (what, n, e)
    for n, e in te:
        assert e <= U.TENSOR_BOUND, (what, n, e)


def _twice(run, loss_bits):
    """run() -> (losses, tensors) on fresh tensors, twice: tensors bit for bit, losses bit for bit or within the bound"""
    first, again = run(), run()
    for a, b in zip(first[1], again[1]):
        assert torch.equal(a, b)
    for a, b in zip(first[0], again[0]):
        assert a == b if loss_bits else U.loss_err(a, b) <= U.LOSS_BOUND, (a, b)
    return first


def _on(t):
    return t.detach().clone().to(DEV).requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("case", U.LTA_CASES)
def test_lta_edges(case):
    import cmh_native as N
    import mith_ops as M
    from mith_train_ops import LtaFn
    B, Ltot, l0, L, K, D, top_k, with_kpm = case
    c = U.lta_case(*case)
    leaf = c["tokens"].double().requires_grad_(True)
    ref = U.lta_forward(leaf, c["sim"], c["kpm"], l0, L, top_k)
    ref.backward(U.UPSTREAM["lta"] * c["dmerge"].double())
    sim, dmerge = c["sim"].to(DEV), U.UPSTREAM["lta"] * c["dmerge"].to(DEV)
    kpm = None if c["kpm"] is None else c["kpm"].to(DEV)

    def run():
        tokens = _on(c["tokens"])
        out = LtaFn.apply(tokens, sim, kpm, l0, L, top_k)
        out.backward(dmerge)
        assert torch.equal(M.lta(tokens.detach(), sim, kpm, l0, L, top_k), out.detach())
        return [], [out.detach(), tokens.grad]
    _, (out, dtok) = _twice(run, loss_bits=True)
    _check(f"lta {case}", tensors=[("merge", out, ref.detach()), ("dtokens", dtok, leaf.grad)])
    if L != Ltot:                                                    # the entry itself on a NaN-filled gradient: the rows outside the slice are zeroed
        filled = torch.full((B, Ltot, D), float("nan"), device=DEV)
        kpm8 = None if kpm is None else kpm.to(torch.uint8).contiguous()
        N.check(N.lib().cmh_mith_lta_backward(N.ptr(sim), N.ptr(kpm8), N.ptr(dmerge.contiguous()), N.ptr(filled), B, Ltot, l0, L, K, D, top_k,
                                              N.stream_ptr(sim.device)), "cmh_mith_lta_backward")
        assert torch.equal(filled, dtok) and not bool(filled[:, :l0].any()) and not bool(filled[:, l0 + L:].any())


@pytest.mark.parametrize("case", U.BITHASH_CASES)
def test_bitwise_hashing_edges(case):
    from mith_train_ops import BitHashFn
    c = U.bithash_case(*case)
    leaves64 = [c[k].double().requires_grad_(True) for k in ("x", "w", "b")]
    yref = U.bithash(*leaves64)
    yref.backward(U.UPSTREAM["bithash"] * c["dy"].double())
    dy = U.UPSTREAM["bithash"] * c["dy"].to(DEV)

    def run():
        leaves = [_on(c[k]) for k in ("x", "w", "b")]
        y = BitHashFn.apply(*leaves)
        y.backward(dy)
        return [], [y.detach()] + [l.grad for l in leaves]
    _, got = _twice(run, loss_bits=True)
    _check(f"bithash {case}", tensors=list(zip(("y", "dx", "dw", "db"), got, [yref.detach()] + [l.grad for l in leaves64])))


@pytest.mark.parametrize("case", U.L2NORM_CASES)
def test_l2_normalize_edges(case):
    from mith_train_ops import L2NormFn
    c = U.l2norm_case(*case)
    x64, dy64 = c["x"].double(), U.UPSTREAM["l2norm"] * c["dy"].double()
    dy = U.UPSTREAM["l2norm"] * c["dy"].to(DEV)

    def run():
        x = _on(c["x"])
        y = L2NormFn.apply(x)
        y.backward(dy)
        return [], [y.detach(), x.grad]
    _, (y, dx) = _twice(run, loss_bits=True)
    _check(f"l2norm {case}", tensors=[("y", y, U.l2norm(x64)), ("dx", dx, U.l2norm_dx(x64, dy64))], rows=True)


def test_elementwise_edges():
    import mith_ops as M
    from mith_train_ops import AddPosFn, GeluFn
    c = U.mix_case()
    _, Bref, Hi, Ht = U.mith_mix(*(c[k].double() for k in ("ic", "it", "tc", "tt")), U.MIX_LAMBDA)
    run = lambda: ([], list(M.mith_mix(*(c[k].to(DEV) for k in ("ic", "it", "tc", "tt")), U.MIX_LAMBDA)))
    _, (Bc, Hi_, Ht_) = _twice(run, loss_bits=True)
    assert torch.equal(Bc.cpu().double(), Bref)                      # signs and exact zeros (0 == -0)
    _check("mith_mix", tensors=[("H_i", Hi_, Hi), ("H_t", Ht_, Ht)])

    g = U.gen(21, 3, 5, 7)
    x, pe, dy = (torch.randn(*s, generator=g) for s in ((3, 5, 7), (9, 7), (3, 5, 7)))

    def run_pos():
        leaf = _on(x)
        y = AddPosFn.apply(leaf, pe.to(DEV))
        y.backward(U.UPSTREAM["addpos"] * dy.to(DEV))
        return [], [y.detach(), leaf.grad]
    _, (y, dx) = _twice(run_pos, loss_bits=True)
    _check("add_positional (3, 5, 7)", tensors=[("y", y, U.add_positional(x.double(), pe.double())), ("dx", dx, U.UPSTREAM["addpos"] * dy.double())])

    c = U.gelu_case()
    x64 = c["x"].double().requires_grad_(True)
    yref = torch.nn.functional.gelu(x64)
    yref.backward(U.UPSTREAM["gelu"] * c["dy"].double())

    def run_gelu():
        leaf = _on(c["x"])
        y = GeluFn.apply(leaf)
        y.backward(U.UPSTREAM["gelu"] * c["dy"].to(DEV))
        return [], [y.detach(), leaf.grad]
    _, (y, dx) = _twice(run_gelu, loss_bits=True)
    _check("gelu 257", tensors=[("y", y, yref.detach()), ("dx", dx, x64.grad)])


@pytest.mark.parametrize("n", U.SQDIFF_SIZES)
@pytest.mark.parametrize("wrt", ["both", "a", "b", "equal"])
def test_sq_diff_sum_edges(n, wrt):
    from mith_train_ops import SqDiffSumFn
    c = U.sqdiff_case(n)
    a0, b0 = c["a"], (c["a"] if wrt == "equal" else c["b"])
    up = U.UPSTREAM["sqdiff"]
    ref = ((a0.double() - b0.double()) ** 2).sum()
    da = 2 * up * (a0.double() - b0.double())

    def run():
        a, b = _on(a0), _on(b0)
        if wrt == "a":
            b = b.detach()
        if wrt == "b":
            a = a.detach()
        loss = SqDiffSumFn.apply(a, b)
        (up * loss).backward()
        assert (a.grad is None) == (wrt == "b") and (b.grad is None) == (wrt == "a")
        return [float(loss.detach())], [t.grad for t in (a, b) if t.grad is not None]
    losses, grads = _twice(run, loss_bits=False)
    want = {"both": [da, -da], "equal": [da, -da], "a": [da], "b": [-da]}[wrt]
    names = {"both": ["da", "db"], "equal": ["da", "db"], "a": ["da"], "b": ["db"]}[wrt]
    if wrt == "equal":
        assert losses[0] == 0.0
    _check(f"sq_diff {n} {wrt}", [("sum", losses[0], float(ref))], list(zip(names, grads, want)))


# ------------------------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("case", U.BAYES_CASES)
def test_bayesian_loss_edges(case):
    from mith_train_ops import BayesianLossFn
    c = U.bayes_case(*case)
    up = U.UPSTREAM["bayes"]
    (ref,), (gref,) = U.evaluate(lambda batch: U.bayes_loss(batch, c["bank"], c["bank_label"], c["label"]), [c["batch"]], upstream=up)
    bank, bl, lab = (c[k].to(DEV) for k in ("bank", "bank_label", "label"))

    def run():
        x = _on(c["batch"])
        loss = BayesianLossFn.apply(bank, x, bl, lab)
        (up * loss).backward()
        return [float(loss.detach())], [x.grad]
    losses, grads = _twice(run, loss_bits=False)
    _check(f"bayes {case}", [("loss", losses[0], ref)], [("dbatch", grads[0], gref)])


def test_bayesian_backward_refuses_a_bank_past_its_slices():
    from mith_train_ops import BayesianLossFn
    Mb, B, K, C = U.BAYES_TOO_LARGE, 3, 16, 1
    x = torch.zeros(B, K, device=DEV, requires_grad=True)
    loss = BayesianLossFn.apply(torch.zeros(Mb, K, device=DEV), x, torch.ones(Mb, C, device=DEV), torch.ones(B, C, device=DEV))
    with pytest.raises(RuntimeError, match=f"bank of {Mb} rows is too large"):
        loss.backward()
    assert x.grad is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", U.NCE_CASES)
def test_info_nce_edges(case):
    from mith_train_ops import InfoNceFn
    R, G, D = case
    c = U.nce_case(*case)
    up = U.UPSTREAM["nce"]
    (ref,), grefs = U.evaluate(lambda a, b: U.info_nce(a, b, G), [c["a"], c["b"]], upstream=up)

    def run():
        a, b = _on(c["a"]), _on(c["b"])
        loss = InfoNceFn.apply(a, b, G, U.NCE_TEMPERATURE)
        (up * loss).backward()
        return [float(loss.detach())], [a.grad, b.grad]
    losses, grads = _twice(run, loss_bits=False)
    if G == 1:
        assert losses[0] == 0.0
    _check(f"nce {case}", [("loss", losses[0], ref)], list(zip(("da", "db"), grads, grefs)))


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("case", U.MSL_CASES)
def test_multi_similarity_loss_edges(case, cross):
    from train.DMsH_LN.MSLOSS import MultiSimilarityLoss
    c, fn, tensors, names = U.msl_problem(case, cross)
    up = U.UPSTREAM["msl"]
    (ref,), grefs = U.evaluate(fn, tensors, upstream=up)
    code, msl = c["code"].to(DEV), MultiSimilarityLoss()

    def run():
        leaves = [_on(t) for t in tensors]
        loss = msl(leaves[0], code, feat2=leaves[1] if cross else None)
        (up * loss).backward()
        with torch.no_grad():
            assert float(msl(leaves[0], code, feat2=leaves[1] if cross else None)) == float(loss.detach())
        return [float(loss.detach())], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=True)
    _check(f"msl {case[:3]} {'cross' if cross else 'self'}", [("loss", losses[0], ref)], list(zip(names, grads, grefs)),
           rows=case[:3] == U.MSL_ZERO_ROW)
