"""The loss and head kernels (csrc/losses.hip, heads_bwd.hip, heads2.hip, qmi.hip, msl.hip spl_*) at wave, slice and tile edges,
through the wrappers the trainers use, against the float64 references of tests/lossutil.py (anchored to the reference project's
goldens and checked for settled threshold decisions by tests/test_loss_edges_host.py).

Bound, the same for every family (the project's existing one for these kernels, test_hyp_loss_backward / test_gpu_msl, stated "of
max"): |loss - ref| <= 1e-5 max(1, |ref|); every gradient (and forward) tensor max |got - ref| <= 1e-4 max |ref|.  A wrong index at
these sizes moves a gradient by about 1/B of its maximum (>= 1e-3 at B = 1025), so the bound catches it; the float32 evaluation of
the same formula on the CPU (e32 below) sits two orders under it.  The upstream gradient is 1.7 or 2.0, never 1.  Every case runs
twice on fresh tensors: the gradients must be equal bit for bit (fixed summation order); the losses that finish through f64 atomics
(HyP, DCHMT, DNPH) are compared within the bound instead, QMI and SPL bit for bit.

Which kernel form each case reaches:
  HyP (B, K, C), thr .05, alpha .8
    (65, 65, 5)      hyp_rows / hyp_proxy <KV=2>, one column in slice 2; the second ballot window holds one row; proxy quarters
                     17/17/17/14; dsph_pair_kernel<2> 3 x 3 tiles, the last holding one row
    (63, 130, 24)    <KV=4>, two columns in slice 3; one partial window; 32-row pair tiles with a partial last tile
    (129, 192, 70)   <KV=4>, empty fourth slice; C > 64; the third window holds one row        (and alpha = 0: pair kernels skipped)
    (130, 257, 24)   <KV=8>, one column in slice 5
    (3, 512, 6)      <KV=8> full; hyp_proxy_kernel waves with empty row ranges (labels by hand: row 0 empty, rows 1, 2 disjoint)
    (1024, 16, 24)   the last batch of dsph_pair_kernel<2> (32 x 32 tiles); 16 full ballot windows
    (1025, 64, 24)   the first of dsph_pair_kernel<4> (17 x 17 tiles, the last holding one row); 17 windows, the last holding one row
  DCHMT (B, D, C, similarity, type): dchmt_pair_kernel (B^2 threads), dchmt_rows_kernel (8 slices)
    (65, 65, 70, cosine, l1)      B^2 no multiple of 256; C > 64 in the lane-strided label dot; slice tail
    (33, 100, 24, cosine, l2)     sim_threshold .13 (.1 is on the lattice of D = 100)
    (17, 512, 5, euclidean, l2)   all 8 slices full
    (130, 257, 24, euclidean, l1) one column in slice 5
  DNPH (B, K, C, noise): dnph_row_kernel (4 of the 2B rows per workgroup), dnph_rows_bwd / dnph_proxy_bwd (8 slices), ce_argmax_bwd
    (33, 65, 65, yes)   66 rows: the last workgroup holds two; C and K one past a wave
    (129, 512, 24, no)  full slices
    (7, 257, 130, yes)  slice tail; C spans three lane trips
    (8, 64, 4096, no)   the documented C limit (16 KB of dynamic LDS)
  QMI (B, K, C): qmi_rows_kernel<false / true>
    (257, 65, 33)    the second 256-trip holds one row (masked tail, the j < B clamp, LDS slices added to twice); second label word one bit
    (300, 257, 24)   44 rows in the second trip
    (65, 1024, 512)  maximal K (4 x 1024 LDS slices) and 16 label words
  SPL (B, K, C, delta), each with a is b and a != b: spl_rows, spl_bwd_rows, spl_bwd_cols (accumulating when a is b)
    (257, 65, 24, .5)       the second trip holds one row; odd B: the two-way unrolled sums take their remainder
    (300, 513, 80, 1.0)     the third column-per-thread slot holds one column
    (65, 1024, 1024, .25)   the limits of K and C
  LinearHash (M, N, K) x act x mask: la_dz, la_dx, la_dw
    (67, 5, 260)     the second grid.y block holds 4 columns; 8-row unroll remainder 3; db's second lane trip
    (9, 64, 513)     the third grid.y block holds one column; remainder 1.  The forward refuses K % 4 != 0, so no trainer reaches
                     this shape: the backward entry is called directly, with the float64 y rounded to float32
  BatchNorm (B, d): batchnorm_train / running / bwd   (65, 7) lane stride past 64 rows, last 4-column workgroup holds 3;
                     (3, 130) fewer rows than lanes, last workgroup holds 2;  (256, 513) four full lane trips, last workgroup holds 1

Measured on MI355X, worst over a family's cases (loss: |got - ref| / max(1, |ref|); tensors: max |got - ref| / max |ref|), next to the
worst e32 of the family printed by tests/test_loss_edges_host.py:
  HyP        loss 6.1e-08 (e32 1.3e-07)   dx 2.2e-06 (3.2e-07)   dy 2.5e-06 (3.4e-07)   dproxies 1.1e-06 (5.2e-07)      worst at (1024, 16, 24):
             about 7 x e32 - 24 proxy and up to ~600 pair terms per row in one serial fma chain against torch's blocked sums
  DCHMT      loss 3.5e-08 (5.9e-08)       dimg 3.3e-07 (2.8e-07)   dtxt 3.7e-07 (2.7e-07)
  DNPH       loss 5.9e-08 (2.2e-08)       dhash 1.8e-06 (3.5e-07, at C = 4096: one chain over the classes)   dpre 6.7e-08 (9.2e-08)
             dproxies 1.9e-06 (4.7e-07, at 2B = 258 rows in one chain)   the three forward outputs <= 8.7e-08
  QMI        loss 3.8e-08 (5.5e-08)       dimg 1.6e-07 (5.2e-07)   dtxt 1.9e-07 (6.6e-07)
  SPL        loss 9.1e-08 (1.9e-07)       da 2.2e-06 (2.9e-06, a is b)   db 5.3e-07 (8.9e-07)
  LinearHash y 1.9e-07 (1.1e-06)          dx 2.8e-07 (3.5e-07)   dW 1.1e-07 (4.3e-07)   db 2.3e-07 (7.3e-07)
  BatchNorm  y 1.5e-07 (2.8e-07)          running statistics 6.8e-08 (9.3e-08)   dx 1.5e-07 (1.7e-07)   dw 1.1e-07 (2.0e-07)   db 8.4e-08 (1.6e-07)
No case is above 8 x e32 (64 x would need explaining); every case takes under a second.
Elsewhere: the DMsH-LN multi-similarity loss and csrc/mith.hip (tests/test_gpu_mith_edges.py).  Out of scope: twdh_* (elementwise),
the forward small-linear kernels (test_linear_act_many_rows_has_the_one_row_kernels_bits)."""
import pytest
import torch

import lossutil as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_BOUND, TENSOR_BOUND = 1e-5, 1e-4


def _loss_err(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


def _of_max(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _check(what, losses, tensors):
    """losses: (name, got, ref); tensors: (name, got, ref).  Prints every figure, then asserts the bounds."""
    le = [(n, _loss_err(g, r)) for n, g, r in losses]
    te = [(n, _of_max(g, r)) for n, g, r in tensors]
    print(f"measured {what}: " + " ".join(f"{n} {e:.1e}" for n, e in le + te))
    for n, g, r in tensors:
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), (what, n)
    for n, e in le:
        assert e <= LOSS_BOUND, (what, n, e)
    for n, e in te:
        assert e <= TENSOR_BOUND, (what, n, e)


def _twice(run, loss_bits):
    """run() -> (losses, gradients) on fresh tensors, twice: gradients bit for bit, losses bit for bit or within the bound"""
    first, again = run(), run()
    for a, b in zip(first[1], again[1]):
        assert torch.equal(a, b)
    for a, b in zip(first[0], again[0]):
        assert a == b if loss_bits else _loss_err(a, b) <= LOSS_BOUND, (a, b)
    return first


def _on(t):
    return t.to(DEV).requires_grad_(True)


@pytest.mark.parametrize("case", L.HYP_CASES)
def test_hyp_loss_edges(case):
    from backward_ops import HypLoss
    c, fn, tensors, names = L.problem("hyp", case)
    (ref,), rgrads = L.evaluate(fn, tensors, upstream=L.UPSTREAM["hyp"])
    lab = c["lab"].to(DEV)

    def run():
        leaves = [_on(t) for t in tensors]
        loss = HypLoss.apply(leaves[0], leaves[1], lab, leaves[2], c["thr"], c["alpha"])
        (loss * L.UPSTREAM["hyp"]).backward()
        return [float(loss.detach())], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=False)
    _check(f"hyp {case}", [("loss", losses[0], ref)], list(zip(names, grads, rgrads)))


@pytest.mark.parametrize("case", L.DCHMT_CASES)
def test_dchmt_loss_edges(case):
    from backward_ops import DchmtLoss
    c, fn, tensors, names = L.problem("dchmt", case)
    (ref,), rgrads = L.evaluate(fn, tensors, upstream=L.UPSTREAM["dchmt"])
    lab = c["lab"].to(DEV)

    def run():
        leaves = [_on(t) for t in tensors]
        loss = DchmtLoss.apply(leaves[0], leaves[1], lab, *c["cfg"])
        (loss * L.UPSTREAM["dchmt"]).backward()
        return [float(loss.detach())], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=False)
    _check(f"dchmt {case}", [("loss", losses[0], ref)], list(zip(names, grads, rgrads)))


@pytest.mark.parametrize("case", L.DNPH_CASES)
def test_dnph_loss_edges(case):
    import cmh_native as N
    from backward_ops import DnphLoss
    c, fn, tensors, names = L.problem("dnph", case)
    rvals, rgrads = L.evaluate(fn, tensors, upstream=L.UPSTREAM["dnph"])
    lab = c["lab"].to(DEV)
    ni, nt = (None if c[k] is None else c[k].to(DEV) for k in ("noise_i", "noise_t"))

    def run():
        leaves = [_on(t) for t in tensors]
        loss = DnphLoss.apply(leaves[0], leaves[1], leaves[2], leaves[3], lab, leaves[4], ni, nt, 1.0, 0.1)
        (loss * L.UPSTREAM["dnph"]).backward()
        three = N.dnph_loss(*(l.detach() for l in leaves[:4]), lab, leaves[4].detach(), ni, nt, 1.0, 0.1)
        return [float(loss.detach())] + [float(v) for v in three], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=False)
    _check(f"dnph {case}", [("loss", losses[0], rvals[0]), ("total", losses[1], rvals[0]), ("loss1", losses[2], rvals[1]),
                            ("noise", losses[3], rvals[2])], list(zip(names, grads, rgrads)))


@pytest.mark.parametrize("case", L.QMI_CASES)
def test_qmi_loss_edges(case):
    from train.DNpH_TMM.loss import qmi_loss
    c, fn, tensors, names = L.problem("qmi", case)
    (ref,), rgrads = L.evaluate(fn, tensors, upstream=L.UPSTREAM["qmi"])
    lab = c["lab"].to(DEV)

    def run():
        leaves = [_on(t) for t in tensors]
        loss = qmi_loss(images=leaves[0], texts=leaves[1], targets=lab)
        (L.UPSTREAM["qmi"] * loss).backward()
        with torch.no_grad():
            assert float(qmi_loss(images=leaves[0], texts=leaves[1], targets=lab)) == float(loss.detach())
        return [float(loss.detach())], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=True)
    _check(f"qmi {case}", [("loss", losses[0], ref)], list(zip(names, grads, rgrads)))


@pytest.mark.parametrize("variant", ["same", "cross"])
@pytest.mark.parametrize("case", L.SPL_CASES)
def test_spl_loss_edges(case, variant):
    from train.DHaPH.MSLoss import MSLoss
    c, fn, tensors, names = L.problem("spl", case, variant)
    (ref,), rgrads = L.evaluate(fn, tensors, upstream=L.UPSTREAM["spl"])
    lab = c["lab"].to(DEV)
    crit, epoch = MSLoss(temperature=L.SPL_TEMPERATURE, totalepoch=12, self_paced=True), int(case[3] * 4)
    assert crit.delta(epoch) == case[3]

    def run():
        leaves = [_on(t) for t in tensors]
        loss = crit(leaves[0], leaves[-1], lab, epoch)              # one leaf: the same tensor in both roles
        (L.UPSTREAM["spl"] * loss).backward()
        return [float(loss.detach())], [l.grad for l in leaves]
    losses, grads = _twice(run, loss_bits=True)
    _check(f"spl {case} {variant}", [("loss", losses[0], ref)], list(zip(names, grads, rgrads)))


@pytest.mark.parametrize("M,N,K", L.LINEAR_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("use_mask", [False, True])
def test_linear_act_edges(M, N, K, act, use_mask):
    import cmh_native as Nn
    from backward_ops import LinearAct
    c = L.linear_case(M, N, K, act, use_mask)
    leaves64 = [c[k].double().requires_grad_(True) for k in ("x", "w", "b")]
    yref = L.linear_act(*leaves64, act, c["mask"], L.LINEAR_DROP)
    yref.backward(c["dy"].double())
    mask = None if c["mask"] is None else c["mask"].to(DEV)
    dy = c["dy"].to(DEV)

    def run():
        leaves = [_on(c[k]) for k in ("x", "w", "b")]
        if K % 4 == 0:
            out = LinearAct.apply(leaves[0], leaves[1], leaves[2], act, mask, L.LINEAR_DROP)
            out.backward(dy)
            return [], [out.detach()] + [l.grad for l in leaves]
        with pytest.raises(Nn.NativeError, match="multiple of 4"):
            LinearAct.apply(leaves[0], leaves[1], leaves[2], act, mask, L.LINEAR_DROP)
        x, w = leaves[0].detach(), leaves[1].detach()
        y = yref.detach().float().to(DEV)
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(N, dtype=torch.float32, device=DEV)
        ws = Nn.workspace(M * N * 4 + 256, x.device, "bwd")
        Nn.check(Nn.lib().cmh_linear_act_backward(Nn.ptr(x), Nn.ptr(w), Nn.ptr(y), Nn.ptr(dy), Nn.ptr(mask), 1.0 / (1.0 - L.LINEAR_DROP), act,
                                                  Nn.ptr(dx), Nn.ptr(dw), Nn.ptr(db), M, N, K, Nn.ptr(ws), ws.numel(), Nn.stream_ptr(x.device)),
                 "cmh_linear_act_backward")
        return [], [y, dx, dw, db]
    _, got = _twice(run, loss_bits=True)
    _check(f"linear {(M, N, K)} act {act} mask {use_mask}", [], list(zip(("y", "dx", "dW", "db"), got, [yref.detach()] + [l.grad for l in leaves64])))


@pytest.mark.parametrize("B,d", L.BATCHNORM_SHAPES)
def test_batchnorm_edges(B, d):
    import cmh_native as Nn
    from backward_ops import BatchNorm1dTrain
    c = L.batchnorm_case(B, d)
    leaves64 = [c[k].double().requires_grad_(True) for k in ("x", "w", "b")]
    yref = L.batchnorm_train(*leaves64, L.BATCHNORM_EPS)
    yref.backward(c["dy"].double())
    rref = L.batchnorm_running(c["x"].double(), c["rm"].double(), c["rv"].double(), L.BATCHNORM_MOMENTUM)
    dy = c["dy"].to(DEV)

    def run():
        leaves = [_on(c[k]) for k in ("x", "w", "b")]
        out = BatchNorm1dTrain.apply(leaves[0], leaves[1], leaves[2], L.BATCHNORM_EPS)
        out.backward(dy)
        rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
        x = leaves[0].detach()
        Nn.check(Nn.lib().cmh_batchnorm1d_update_running(Nn.ptr(x), L.BATCHNORM_MOMENTUM, Nn.ptr(rm), Nn.ptr(rv), B, d, Nn.stream_ptr(x.device)),
                 "cmh_batchnorm1d_update_running")
        return [], [out.detach(), rm, rv] + [l.grad for l in leaves]
    _, got = _twice(run, loss_bits=True)
    _check(f"batchnorm {(B, d)}", [], list(zip(("y", "running_mean", "running_var", "dx", "dw", "db"), got,
                                               [yref.detach(), rref[0], rref[1]] + [l.grad for l in leaves64])))


def test_one_past_the_limit_is_refused_by_the_library():
    """K = 513 for the HyP, DCHMT and DNPH backward, K = 1025 for QMI and SPL, C = 513 for QMI: the library's error, not a launch"""
    from backward_ops import DchmtLoss, DnphLoss, HypLoss
    from train.DHaPH.MSLoss import MSLoss
    from train.DNpH_TMM.loss import qmi_loss
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    B, C = 5, 6
    lab = torch.zeros(B, C)
    lab[torch.arange(B), torch.arange(B)] = 1
    lab[1, :3] = 1
    lab = lab.to(DEV)
    x, y, prox = r(B, 513).requires_grad_(), r(B, 513).requires_grad_(), r(C, 513).requires_grad_()
    with pytest.raises(RuntimeError, match="dsph_hyp_loss_backward: bad shape"):
        HypLoss.apply(x, y, lab, prox, 0.05, 0.8).backward()
    with pytest.raises(RuntimeError, match="dchmt_loss_backward: bad shape"):
        DchmtLoss.apply(x, y, lab, 256, "cosine", "l2", 0.5, 0.1).backward()
    with pytest.raises(RuntimeError, match="dnph_loss_backward: bad shape"):
        DnphLoss.apply(x, y, r(B, C).requires_grad_(), r(B, C).requires_grad_(), lab, prox, None, None, 1.0, 0.1).backward()
    big, big2 = r(B, 1025).requires_grad_(), r(B, 1025).requires_grad_()
    with pytest.raises(RuntimeError, match=r"qmi_loss: B=5 K=1025"):
        qmi_loss(images=big, texts=big2, targets=lab)
    with pytest.raises(RuntimeError, match=r"qmi_loss: B=5 K=8 \(<= 1024\) C=513"):
        qmi_loss(images=r(B, 8).requires_grad_(), texts=r(B, 8), targets=torch.ones(B, 513, device=DEV))
    with pytest.raises(RuntimeError, match="spl_loss: bad shape B=5 K=1025"):
        MSLoss()(big, big2, lab, 1)
    assert x.grad is None and big.grad is None
    torch.cuda.synchronize()
