"""The fused BertAdam step (csrc/optim.hip: adam_sumsq_kernel, adam_coef_kernel, adam_update_kernel) against oracle/adam_oracle.py BIT FOR
BIT, tensor by tensor, through cmh_native.bert_adam_step with hand-built entries (adamutil.Slot: sizes, offsets and per-tensor scalars).

The only part of a step whose value depends on a summation order is the clip coefficient c = min(1, max_norm / (||g|| + 1e-6)).  So for a
clipped tensor the kernel's c is RECOVERED: it is the float32 near the oracle's for which the gradient the kernel left is fl(g * c) on
every element (adamutil.recover_coef), and then p, m, v and g must equal the oracle's step with that c in every bit.  An unclipped tensor
must equal the oracle outright, and its gradient must keep its bits.

How far the kernel's c may lie from the oracle's (adamutil.COEF_ULPS = 16): adam_sumsq_kernel adds a chunk's squares in f32 - 16 float4
trips per thread, 6 shuffle levels, 2 LDS adds, about 26 roundings in sequence, <= 26 * 2^-24 relative on the sum of squares and half that
on the norm (~13 * 2^-24, under 2 ulps of a float32 in [1, 2)); the partials are then added in f64; one more rounding each for the cast
of the norm, the + 1e-6 and the divide.  16 ulps is that bound with a margin of four.  LARGEST DISTANCE SEEN ON THE MI355X, over every
clipped tensor of every test in this file: 2 ulps (one tensor of the back-to-back calls; 0 or 1 everywhere else).

Three mutations of csrc/optim.hip were tried on a scratch copy (never committed); every test says which of them it catches:
  M1  adam_coef_kernel's loop over the chunk partials stops at 256 (`i < nch` -> `i < min(nch, 256)`);
  M2  adam_update_kernel's tail loop starts one element late (`tail + threadIdx.x` -> `tail + 1 + threadIdx.x`);
  M3  the `p_bf16` store of the tail loop is dropped (caught in test_gpu_adam_bf16.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import adamutil as au

pytestmark = pytest.mark.gpu
DEV = au.DEV
SIZES = (49153, 1, 16384, 3, 32769, 4, 16385, 5, 16380, 255, 32768, 256, 16383, 257, 16387, 1023, 1025)   # small ones between large ones
LRS = (1e-3, 1e-5, 3e-2)
WORKSPACE = -2                     # CMH_ERR_WORKSPACE (include/cmh.h)


@pytest.fixture(scope="module")
def N():
    import cmh_native
    return cmh_native


def test_the_size_list_is_the_one_the_kernels_have_edges_at():
    assert sorted(SIZES) == [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 16380, 16383, 16384, 16385, 16387, 32768, 32769, 49153]


def test_sizes_and_scalars_mixed_in_one_call(N):
    """Every size of the list in ONE call (first_chunk bookkeeping: 1- to 4-chunk tensors with single-element ones between them), each
    tensor with its own lr, weight_decay in {0, 0.2} and max_grad_norm in {1, 0, -1}; of the max_grad_norm = 1 tensors, gradients of norm
    ~3 sqrt(n) clip and gradients of norm ~0.3 do not.  Two steps, so m and v are non-zero on the second.
    Catches M2 (n % 4 != 0: the element at the head of the tail keeps its old p / m / v)."""
    slots = []
    for i, n in enumerate(SIZES):
        mx = (1.0, 0, -1, 1.0)[i % 4]
        clips = i % 8 < 4                      # of the max_grad_norm = 1 tensors, every other one clips
        slots.append(au.Slot(n, lr=LRS[i % 3], wd=(0.0, 0.2)[(i // 2) % 2], mx=mx, seed=i,
                             gscale=3.0 if clips else 0.3 / np.sqrt(n)))
    worst = au.run_steps(N, slots, steps=2, what="mixed")
    clipped = [sl.n for sl in slots if sl.mx > 0 and all(c < 1 for c in sl.coefs)]
    kept = [sl.n for sl in slots if sl.mx > 0 and all(c == 1 for c in sl.coefs)]
    assert len(clipped) >= 3 and len(kept) >= 3, (clipped, kept)
    print(f"mixed call: clipped {clipped}, inside their norm {kept}, recovered coefficient at most {worst} ulp from the oracle's")
    assert worst <= au.COEF_ULPS


OFFSETS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("n", [1000, 16385])
def test_one_stream_misaligned_and_all_four(N, n):
    """p, g, m, v each alone one element off a 16-byte boundary, and all four: adam_update_kernel must leave the float4 path when ANY of
    the four is misaligned, adam_sumsq_kernel when g is; the slack before and after every view keeps its bits.  One call holds the five
    layouts and an aligned tensor; clipped (gradient norm ~3 sqrt(n)), with weight decay.  Catches M2 (every element is tail here: the
    first of each chunk is skipped)."""
    slots = [au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, off=off, seed=10 + i, gscale=3.0) for i, off in enumerate(OFFSETS)]
    slots.append(au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, seed=20, gscale=3.0))
    slots.append(au.Slot(n, lr=1e-3, wd=0.0, mx=-1, off=(0, 1, 0, 0), seed=21))        # misaligned g without clipping
    worst = au.run_steps(N, slots, steps=2, what="offsets")
    assert all(c < 1 for sl in slots if sl.mx > 0 for c in sl.coefs)
    print(f"n={n}: recovered coefficient at most {worst} ulp from the oracle's")


@pytest.mark.parametrize("n", [256 * 16384, 256 * 16384 + 1, 257 * 16384 + 5])
def test_more_than_256_chunks(N, n):
    """adam_coef_kernel's `for (i = threadIdx.x; i < nch; i += 256)` takes a second trip only above 256 chunks.  Gradient 1e-4 everywhere
    and 0.5 in the last 16389 elements (for the largest size all of it in chunk indices >= 256; for 256 * 16384 + 1 one element of it): with every partial summed the
    norm is ~64 and the tensor clips; without the second trip it is <= 1 and it would not.  A mirrored tensor has the energy in its first
    chunk.  One step: the second would walk the same paths.  (n = 256 * 16384 has exactly 256 chunks: the last size at which one trip is
    enough.)  Catches M1 at the two larger sizes."""
    g = np.full(n, 1e-4, np.float32)
    g[n - 16389:] = 0.5
    tail, head = au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, seed=30), au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, seed=31)
    if n >= 257 * 16384:
        assert np.sqrt((g[:256 * 16384].astype(np.float64) ** 2).sum()) + 1e-6 < 1 < np.sqrt((g.astype(np.float64) ** 2).sum())
    slots = [tail, head]
    worst = au.run_steps(N, slots, steps=1, what=">256 chunks", grads=[[g, g[::-1]]])
    assert all(sl.coefs[0] < 1 for sl in slots)
    print(f"n={n}: coefficients {[float(sl.coefs[0]) for sl in slots]}, at most {worst} ulp from the oracle's")


def _with_norm(n, target, seed):
    """a float32 gradient whose f64 norm is `target` up to the rounding of its elements"""
    g = np.random.default_rng(seed).standard_normal(n)
    for _ in range(3):
        g = (g * (target / np.sqrt((g.astype(np.float32).astype(np.float64) ** 2).sum()))).astype(np.float32).astype(np.float64)
    return g.astype(np.float32)


def test_clip_threshold(N):
    """Gradients whose norm sits within an ulp or two of the point where max_norm / (norm + 1e-6) crosses 1, on both sides, at 1 itself, and
    one well inside.  Whichever side the kernel's own summation falls on, the rule holds - coefficient < 1 iff the gradient's bits moved -
    and the step equals the oracle's with that coefficient (Slot.verify; a gradient left alone although the oracle clips it is accepted
    only within COEF_ULPS of 1)."""
    n, cross = 1000, 1.0 - 1e-6
    targets = [cross + k * 2.0 ** -24 for k in (-2, -1, 0, 1, 2)] + [1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 0.5, 1.0 + 1e-3]
    grads = [_with_norm(n, t, 40 + i) for i, t in enumerate(targets)]
    slots = [au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, seed=40 + i) for i in range(len(targets))]
    au.run_steps(N, slots, steps=1, what="threshold", grads=[grads])
    sides = [bool(sl.coefs[0] < 1) for sl in slots]
    print("clip threshold: norm - (1 - 1e-6) in 2^-24 units -> clipped: " +
          ", ".join(f"{(t - cross) * 2 ** 24:+.1f}: {s}" for t, s in zip(targets, sides)))
    assert sides[-2] is False and sides[-1] is True            # well inside / well outside
    assert sides[7] is True                                    # norm 1 + 2^-23: the sum + 1e-6 is far above 1 in any summation order


def test_degenerate_scalars(N):
    """lr = 0 (step 0 of a warm-up) leaves p as it is while m and v advance; gradient entries that are exactly 0 (all of them, with
    e > 0: 0 / (0 + e)) stay finite; weight_decay = 0 skips the decay term.  Each is also held to the oracle bit for bit."""
    n = 1027
    g_holes = np.random.default_rng(50).standard_normal(n).astype(np.float32)
    g_holes[::3] = 0
    frozen = au.Slot(n, lr=0.0, wd=0.2, mx=1.0, seed=51, gscale=3.0)
    zeros = au.Slot(n, lr=1e-2, wd=0.0, mx=1.0, seed=52)
    holes = au.Slot(n, lr=1e-2, wd=0.2, mx=-1, seed=53)
    nodecay, decay = au.Slot(n, lr=1e-2, wd=0.0, mx=-1, seed=54), au.Slot(n, lr=1e-2, wd=0.2, mx=-1, seed=54)
    slots = [frozen, zeros, holes, nodecay, decay]
    p0 = [sl.view["p"].clone() for sl in slots]
    for s in range(2):
        gs = [None, np.zeros(n, np.float32), g_holes, None, None]
        au.run_steps(N, slots, steps=1, what="degenerate", grads=[gs])
        assert torch.equal(frozen.view["p"].view(torch.int32), p0[0].view(torch.int32))
        assert frozen.view["m"].abs().sum() > 0 and frozen.view["v"].abs().sum() > 0
        assert torch.equal(zeros.view["p"].view(torch.int32), p0[1].view(torch.int32))          # update 0 / (0 + e) = 0, no decay
        assert all(bool(torch.isfinite(sl.view[k]).all()) for sl in slots for k in au.STREAMS)
    assert not torch.equal(nodecay.view["p"], decay.view["p"])
    # same seed, same gradients: the two differ by the decay term alone, and m and v not at all
    assert torch.equal(nodecay.view["m"], decay.view["m"]) and torch.equal(nodecay.view["v"], decay.view["v"])


def test_e_zero_and_other_betas(N):
    """(b1, b2, e) are per launch: e = 0 with non-zero gradients, b1 = 0 (no momentum), b2 = 0.999 - bit for bit like the defaults"""
    for b1, b2, e in ((0.9, 0.999, 0.0), (0.0, 0.98, 1e-6), (0.5, 0.0, 1e-8)):
        slots = [au.Slot(n, lr=1e-3, wd=0.2, mx=1.0, seed=60 + i, gscale=2.0) for i, n in enumerate((7, 1025, 16385))]
        au.run_steps(N, slots, steps=2, b1=b1, b2=b2, e=e, what=f"b1={b1} b2={b2} e={e}")


def test_refusals_leave_every_tensor_untouched(N):
    """An empty tensor, b1 = 1, and a workspace one byte short (through the raw call: CMH_ERR_WORKSPACE) are refused before anything is
    launched: every tensor of the call keeps its bits."""
    slots = [au.Slot(n, seed=70 + i, gscale=3.0).gradient() for i, n in enumerate((5, 16385))]
    before = [sl.host() for sl in slots]

    def untouched():
        torch.cuda.synchronize()
        for sl, bf in zip(slots, before):
            now = sl.host()
            for k in au.STREAMS:
                au.same_bits(now[k], bf[k], f"refused call wrote {k} of n={sl.n}")
    entries = [sl.entry() for sl in slots]
    empty = torch.empty(0, device=DEV)
    with pytest.raises(N.NativeError):
        N.bert_adam_step(entries + [(empty, empty, empty, empty, 1e-3, 0.2, 1.0)], au.B1, au.B2, au.EPS)
    untouched()
    with pytest.raises(N.NativeError):
        N.bert_adam_step(entries, 1.0, au.B2, au.EPS)
    untouched()
    with pytest.raises(N.NativeError):
        N.bert_adam_step(entries, au.B1, 1.0, au.EPS)
    untouched()
    arr = (N.AdamTensor * len(slots))()
    for i, (p, g, m, v, lr, wd, mx) in enumerate(entries):
        arr[i] = N.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, wd, mx, None)
    need = N.lib().cmh_bert_adam_workspace_bytes(len(slots), sum(sl.n for sl in slots))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = N.lib().cmh_bert_adam_step(arr, len(slots), au.B1, au.B2, au.EPS, N.ptr(ws), need - 1, N.stream_ptr(DEV))
    assert rc == WORKSPACE and b"workspace" in N.lib().cmh_last_error()
    with pytest.raises(N.NativeError):
        N.check(rc, "cmh_bert_adam_step")
    untouched()
    # ... and the same call with the byte it lacked runs
    assert N.lib().cmh_bert_adam_step(arr, len(slots), au.B1, au.B2, au.EPS, N.ptr(ws), need, N.stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    for sl, bf in zip(slots, before):
        sl.verify(bf, sl.host(), what="raw call")


def test_back_to_back_calls_with_lists_of_different_sizes(N):
    """Five calls without a synchronisation between them, on disjoint sets of 3, 40, 1, 400 and 2 tensors: both pinned staging tables
    (used in turn, regrown by 5/4) are outgrown while the uploads of earlier calls may still be pending, and the device workspace
    regrows under queued launches.  One synchronisation, then every tensor against the oracle."""
    sizes = (1, 7, 64, 255, 1025, 3, 16385, 130)
    groups, k = [], 0
    for count in (3, 40, 1, 400, 2):
        groups.append([au.Slot(sizes[(k + j) % len(sizes)] if count != 1 else 32769, lr=LRS[j % 3], wd=(0.0, 0.2)[j % 2],
                               mx=(1.0, -1)[(j // 2) % 2], seed=1000 + k + j, gscale=(3.0, 0.01)[(j // 4) % 2]).gradient()
                       for j in range(count)])
        k += count
    before = [[sl.host() for sl in grp] for grp in groups]
    torch.cuda.synchronize()
    for grp in groups:
        N.bert_adam_step([sl.entry() for sl in grp], au.B1, au.B2, au.EPS)
    torch.cuda.synchronize()
    for gi, (grp, bfs) in enumerate(zip(groups, before)):
        for sl, bf in zip(grp, bfs):
            sl.verify(bf, sl.host(), what=f"call {gi}")
    print(f"back to back: recovered coefficient at most {max(d for grp in groups for sl in grp for d in sl.dist)} ulp from the oracle's")


def test_side_stream(N):
    """The same step inside torch.cuda.stream(side): cmh_native.workspace keys every scratch buffer by (device, current stream, tag), so
    the "adam" workspace of the side stream is its own buffer, and the step there equals the oracle's like anywhere else."""
    side = torch.cuda.Stream(device=DEV)
    slots = [au.Slot(n, lr=1e-3, wd=0.2, mx=(1.0, -1)[i % 2], seed=80 + i, gscale=3.0) for i, n in enumerate((5, 1000, 16385, 32769))]
    au.run_steps(N, slots[:2], steps=1, what="default stream")         # the default stream's workspace exists (and is smaller)
    for s in range(2):
        for sl in slots:
            sl.gradient()
        before = [sl.host() for sl in slots]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            N.bert_adam_step([sl.entry() for sl in slots], au.B1, au.B2, au.EPS)
        side.synchronize()
        for sl, bf in zip(slots, before):
            sl.verify(bf, sl.host(), what="side stream")
    keys = [k for k in N._ws_cache if k[2] == "adam"]
    assert {k[1] for k in keys} >= {int(side.cuda_stream), int(torch.cuda.current_stream(DEV).cuda_stream)}
    assert N._ws_cache[(str(DEV), int(side.cuda_stream), "adam")] is not N._ws_cache[(str(DEV), int(torch.cuda.current_stream(DEV).cuda_stream), "adam")]


def test_the_optimizer_class_reaches_the_same_bits(N):
    """BertAdam.step (model/base/optimization.py) on parameters of the edge sizes, two groups with their own lr: what the class hands
    to the kernel - scheduled lr as a python double, weight decay, max_grad_norm - gives the oracle's step bit for bit, unclipped
    (gradients far inside max_grad_norm = 1, so no coefficient has to be recovered)."""
    import oracle.adam_oracle as ao
    from model.base.optimization import BertAdam
    rng = np.random.default_rng(90)
    ns = (3, 16385, 1023, 32768)
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)) for n in ns]
    kw = dict(au.CONFIGS["trainer"])
    opt = BertAdam([{"params": ps[:2], "lr": au.GROUP0_LR}, {"params": ps[2:]}], **kw)
    ref = [(p.detach().cpu().numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32), None) for p, n in zip(ps, ns)]   # p, m, v, g
    for s in range(3):
        for i, p in enumerate(ps):
            g = rng.standard_normal(p.numel()).astype(np.float32) * np.float32(0.1 / np.sqrt(p.numel()))
            p.grad = torch.from_numpy(g).to(DEV)
            lr = au.GROUP0_LR if i < 2 else kw["lr"]
            rp, rg, rm, rv = ao.step(ref[i][0], g, ref[i][1], ref[i][2], s, lr, kw["b1"], kw["b2"], kw["e"], kw["weight_decay"],
                                     kw["max_grad_norm"], kw["t_total"], kw["warmup"], kw["schedule"])
            ref[i] = (rp, rm, rv, rg)
        opt.step()
        for i, p in enumerate(ps):
            got = (p.detach(), opt.state[p]["next_m"], opt.state[p]["next_v"], p.grad)
            for name, a, r in zip("pmvg", got, ref[i]):
                au.same_bits(a.cpu().numpy(), r, f"step {s} {name}{i}")
