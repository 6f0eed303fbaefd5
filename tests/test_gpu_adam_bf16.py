"""The bf16 copies of the weights that the encoder GEMMs read, bit for bit against torch's round-to-nearest-even cast (made on the CPU:
c10's round_to_nearest_even, pure integer arithmetic).

Two writers make them: cmh_cast_f32_to_bf16 (csrc/norm_embed.hip; software f32_to_bf16 of csrc/cmh_common.h throughout) when a copy is
created, and adam_update_kernel (csrc/optim.hip) on every training step - pack_bf16x2 (the hardware v_cvt_pk_bf16_f32) on its float4
path, f32_to_bf16 on its tail and on its scalar path.  A weight whose size is no multiple of 4 mixes the two, so they must round alike:
adamutil.CRAFTED_BITS holds ties to even and to odd, values one off a tie, +-0, the largest finite value (rounds to inf) and the
largest that stays finite, the smallest normal, denormals (with ties among them) and +-inf, and adamutil.crafted_vector puts each of
them on every position mod 4 of a float4 body and, by rotation, into the tail.  No NaN.

Mutation M3 of test_gpu_adam_edges.py's list (the `p_bf16` store dropped from adam_update_kernel's tail loop) is caught by
test_step_rewrites_the_copy_of_a_crafted_parameter (every layout with a tail or a scalar path) and by
test_copy_follows_the_parameter_through_bertadam_steps; M2 (the tail loop starting one element late) by the former, which also holds p,
m and v to the oracle and finds the skipped element's copy still poisoned."""
import numpy as np
import pytest
import torch

import adamutil as au

pytestmark = pytest.mark.gpu
DEV = au.DEV
INVALID = -1                       # CMH_ERR_INVALID (include/cmh.h)
GRID_CAP = 4096 * 256 * 4          # elements one trip of cast_bf16_kernel's stride loop covers at the grid cap of 4096 blocks


@pytest.fixture(scope="module")
def N():
    import cmh_native
    return cmh_native


def test_crafted_vector_covers_every_position():
    """host-side check of the generator: over 4 periods every crafted value stands on every position mod 4, and over the rotations in
    each of the last 3 elements"""
    K = len(au.CRAFTED_BITS)
    n = 4 * (2 * K + 1) + 3
    x = au.crafted_vector(n).view(np.uint32)
    for b in au.CRAFTED_BITS:
        at = np.flatnonzero(x[:n - 3] == b)
        assert {int(i) % 4 for i in at} == {0, 1, 2, 3}, hex(b)
    tails = [set() for _ in range(3)]
    for rot in au.crafted_rotations(n):
        t = au.crafted_vector(n, rot).view(np.uint32)[n - 3:]
        for k in range(3):
            tails[k].add(int(t[k]))
    assert all(set(au.CRAFTED_BITS) <= tk for tk in tails)
    assert not np.isnan(au.crafted_vector(n)).any()


def test_the_reference_cast_rounds_to_nearest_even():
    """what the tests below compare with, spelled out on the patterns whose answer is known by hand"""
    src = np.array([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x7f7fffff, 0x7f7f7fff, 0x7f7f8000, 0x007fffff, 0x00008000, 0x00008001,
                    0x00018000, 0x80000000, 0xff800000], np.uint32)
    want = [0x3f80, 0x3f82, 0x3f80, 0x3f81, 0x7f80, 0x7f7f, 0x7f80, 0x0080, 0x0000, 0x0001, 0x0002, 0x8000, 0xff80]
    got = au.rne_bf16_bits(torch.from_numpy(src.view(np.float32))).numpy().view(np.uint16)
    assert [int(v) for v in got] == want


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
def test_cast_bf16_small(N, n):
    """every crafted value through the float4 body and, by rotation, through the tail loop of cast_bf16_kernel"""
    for rot in au.crafted_rotations(n):
        x = torch.from_numpy(au.crafted_vector(n, rot)).to(DEV)
        got = N.cast_bf16(x)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        assert torch.equal(au.bf16_bits(got), au.rne_bf16_bits(x)), (n, rot)
        assert torch.equal(got.view(torch.int16), x.to(torch.bfloat16).view(torch.int16)), (n, rot)


def test_cast_bf16_second_trip_of_the_stride_loop(N):
    """n just above 4096 * 256 * 4 and no multiple of 4: the grid is capped at 4096 blocks, so the stride loop takes a second trip and the
    tail starts behind it"""
    n = GRID_CAP + 7
    x = torch.from_numpy(au.crafted_vector(n, rot=5)).to(DEV)
    got = N.cast_bf16(x)
    want = au.rne_bf16_bits(x)
    assert torch.equal(au.bf16_bits(got), want)
    assert torch.equal(au.bf16_bits(got)[GRID_CAP - 8:], want[GRID_CAP - 8:])        # (the second trip and the tail, named)


def test_cast_bf16_empty_and_misaligned(N):
    e = N.cast_bf16(torch.empty(0, device=DEV))
    assert e.dtype == torch.bfloat16 and e.numel() == 0
    assert N.cast_bf16(torch.empty(0, 7, device=DEV)).shape == (0, 7)
    src = torch.from_numpy(au.crafted_vector(64 + 1)).to(DEV)
    dst = torch.full((64 + 4,), 3.0, dtype=torch.bfloat16, device=DEV)
    before = au.bf16_bits(dst)
    lib, st = N.lib(), N.stream_ptr(DEV)
    assert lib.cmh_cast_f32_to_bf16(N.ptr(src[1:]), N.ptr(dst), 64, st) == INVALID           # source 4 bytes off
    assert lib.cmh_cast_f32_to_bf16(N.ptr(src), N.ptr(dst[1:]), 64, st) == INVALID           # destination 2 bytes off
    assert lib.cmh_cast_f32_to_bf16(N.ptr(src), N.ptr(dst[2:]), 64, st) == INVALID           # ... 4 bytes off
    assert lib.cmh_cast_f32_to_bf16(N.ptr(src), N.ptr(dst), -1, st) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(au.bf16_bits(dst), before)
    with pytest.raises(N.NativeError):
        N.check(lib.cmh_cast_f32_to_bf16(N.ptr(src[1:]), N.ptr(dst), 64, st), "cmh_cast_f32_to_bf16")
    assert lib.cmh_cast_f32_to_bf16(N.ptr(src), N.ptr(dst[4:]), 64, st) == 0                 # 8 bytes off is what the kernel needs
    torch.cuda.synchronize()
    assert torch.equal(au.bf16_bits(dst[4:]), au.rne_bf16_bits(src[:64])) and torch.equal(au.bf16_bits(dst[:4]), before[:4])


def _attach(N, slot, poison=True):
    """a bf16 copy on the slot's parameter view, made by the library's cast as model/base/model.py::_gemm_w makes it, living in a buffer
    with slack on both sides; `poison` then overwrites it, so that whatever the step does not write shows"""
    p = slot.view["p"]
    cbase = torch.full((slot.n + 16,), au.GUARD, dtype=torch.bfloat16, device=DEV)
    copy = cbase[8:8 + slot.n]
    copy.copy_(N.cast_bf16(p.clone()))                      # (the clone: the cast wants a 16-byte aligned source)
    assert torch.equal(au.bf16_bits(copy), au.rne_bf16_bits(p))
    if poison:
        copy.fill_(-3.0)
    p._cmh_bf16 = copy
    return cbase, copy


K2 = 2 * len(au.CRAFTED_BITS) + 1
LAYOUTS = {"aligned, n % 4 == 0": (4 * K2 + 4, (0, 0, 0, 0)), "aligned, n % 4 == 3 (tail)": (4 * K2 + 3, (0, 0, 0, 0)),
           "p misaligned (scalar path)": (4 * K2 + 4, (1, 0, 0, 0)), "two chunks and a tail": (16384 + 4 * K2 + 3, (0, 0, 0, 0))}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_step_rewrites_the_copy_of_a_crafted_parameter(N, layout):
    """lr = 0, weight_decay = 0 and finite gradients: p keeps its bits (crafted values, inf and denormals among them), and the step must
    leave copy == rne(p) although the copy held other values before - through pack_bf16x2 on the float4 path, f32_to_bf16 on the tail and
    on the scalar path.  One call holds one tensor per rotation, so every crafted value passes through the tail.  The slack around the copy
    keeps its bits."""
    n, off = LAYOUTS[layout]
    rots = list(au.crafted_rotations(n)) if n < 16384 else [0, 1, 2]
    slots = [au.Slot(n, lr=0.0, wd=0.0, mx=(1.0, -1)[r % 2], off=off, seed=200 + r, gscale=2.0, p=au.crafted_vector(n, r)) for r in rots]
    held = [_attach(N, sl) for sl in slots]
    p0 = [sl.view["p"].clone() for sl in slots]
    for s in range(2):
        au.run_steps(N, slots, steps=1, what=layout)
        for sl, (cbase, copy), before in zip(slots, held, p0):
            # (p + -(0 * update) is p in every bit but one: -0 + +0 = +0 under a negative update, in the reference as here - Slot.verify
            # has held p to the oracle's bits already)
            now, was = sl.view["p"].view(torch.int32), before.view(torch.int32)
            assert bool(((now == was) | ((was == -2 ** 31) & (now == 0))).all()), "lr = 0 moved p"
            got, want = au.bf16_bits(copy), au.rne_bf16_bits(sl.view["p"])
            bad = (got != want).nonzero().flatten()
            assert bad.numel() == 0, (f"{layout}: {bad.numel()} of {sl.n} copy elements differ from rne(p), e.g. at {bad[:6].tolist()}: p bits "
                                      f"{[hex(int(v) & 0xffffffff) for v in sl.view['p'].view(torch.int32).cpu()[bad[:6]]]}, copy "
                                      f"{[hex(int(v) & 0xffff) for v in got[bad[:6]]]}, rne {[hex(int(v) & 0xffff) for v in want[bad[:6]]]}")
            assert bool((cbase[:8] == au.GUARD).all()) and bool((cbase[8 + sl.n:] == au.GUARD).all()), "the step wrote around the copy"
            copy.fill_(-3.0)


@pytest.mark.parametrize("n", [1000, 16385, 32769])
def test_copy_follows_the_parameter_through_bertadam_steps(N, n):
    """Ordinary values, lr > 0, two BertAdam.step calls; the copy is attached the way the model attaches it (mith_ops.weight_bf16).  After
    each step the SAME copy tensor holds rne(new p), `_cmh_bf16_version` names the parameter's new version, and weight_bf16 hands that
    tensor back without another cast."""
    import mith_ops
    from model.base.optimization import BertAdam
    rng = np.random.default_rng(n)
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)),
          torch.nn.Parameter(torch.from_numpy(rng.standard_normal((n // 7, 7)).astype(np.float32) * 1e-3).to(DEV)),
          torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n + 1).astype(np.float32)).to(DEV))]       # this one never gets a copy
    copies = [mith_ops.weight_bf16(p) for p in ps[:2]]
    assert all(p._cmh_bf16 is c and c.dtype == torch.bfloat16 for p, c in zip(ps, copies))
    assert torch.equal(au.bf16_bits(copies[0]).reshape(-1), au.rne_bf16_bits(ps[0]))
    opt = BertAdam(ps, lr=1e-2, b1=0.9, b2=0.98, e=1e-6, weight_decay=0.2, max_grad_norm=1.0)
    for s in range(2):
        for p in ps:
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV)
        old = [p.detach().clone() for p in ps]
        opt.step()
        for p, c, o in zip(ps, copies, old):
            assert not torch.equal(p.detach(), o)
            assert p._cmh_bf16 is c and p._cmh_bf16_version == (p.data_ptr(), p._version)
            assert torch.equal(au.bf16_bits(c).reshape(-1), au.rne_bf16_bits(p).reshape(-1)), f"step {s}: copy != rne(p), n={p.numel()}"
            assert mith_ops.weight_bf16(p) is c
        assert not hasattr(ps[2], "_cmh_bf16") and not hasattr(ps[2], "_cmh_bf16_version")
    with torch.no_grad():
        ps[0].mul_(2.0)                                     # any other writer bumps the version: the copy is stale and is rebuilt
    fresh = mith_ops.weight_bf16(ps[0])
    assert fresh is not copies[0] and torch.equal(au.bf16_bits(fresh).reshape(-1), au.rne_bf16_bits(ps[0]).reshape(-1))


@pytest.mark.parametrize("kind", ["numel", "dtype", "strided"])
def test_a_copy_of_the_wrong_size_or_type_is_left_alone_and_rebuilt(N, kind):
    """Something else hung on `_cmh_bf16` - a bf16 tensor of another size, an fp16 tensor of the right size, a strided bf16 view - is not
    written by the step, is not stamped current, and mith_ops.weight_bf16 replaces it by a real copy of the new parameter."""
    import mith_ops
    from model.base.optimization import BertAdam
    n = 1003
    rng = np.random.default_rng(7)
    p = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV))
    wrong = {"numel": lambda: torch.full((n + 1,), 5.0, dtype=torch.bfloat16, device=DEV),
             "dtype": lambda: torch.full((n,), 5.0, dtype=torch.float16, device=DEV),
             "strided": lambda: torch.full((2 * n,), 5.0, dtype=torch.bfloat16, device=DEV)[::2]}[kind]()
    keep = wrong.clone()
    p._cmh_bf16, p._cmh_bf16_version = wrong, (p.data_ptr(), p._version)
    p.grad = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
    p0 = p.detach().clone()
    BertAdam([p], lr=1e-2, weight_decay=0.2).step()
    torch.cuda.synchronize()
    assert not torch.equal(p.detach(), p0)
    assert torch.equal(wrong.view(torch.int16), keep.view(torch.int16)), "the step wrote a tensor that is no copy of this parameter"
    assert p._cmh_bf16_version != (p.data_ptr(), p._version), "a copy the step did not write was stamped current"
    rebuilt = mith_ops.weight_bf16(p)
    assert rebuilt is not wrong and rebuilt.dtype == torch.bfloat16 and rebuilt.numel() == n and p._cmh_bf16 is rebuilt
    assert torch.equal(au.bf16_bits(rebuilt).reshape(-1), au.rne_bf16_bits(p).reshape(-1))
    assert p._cmh_bf16_version == (p.data_ptr(), p._version)
