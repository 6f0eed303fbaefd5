"""The 160-row 12-wave GEMM (csrc/gemm_lc.hip: gemm_lc3_kernel, cmh_set_gemm_lc(9)) and the per-launch route that picks between it and
the wide kernel (cmh_set_gemm_lc(8), the default; which launch takes which form: tests/test_gemm_route.py).  Another schedule of the wide kernel's arithmetic - the
same MFMA chain over K per output element, the same epilogue order, the same residual-first rule - so every comparison is torch.equal
against the wide kernel (cmh_set_gemm_lc(0))."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _problem(M, Nn, K, kind, g):
    p = {"x": torch.randn(M, K, generator=g).bfloat16().to(DEV), "w": (torch.randn(Nn, K, generator=g) * K ** -0.5).bfloat16().to(DEV),
         "bias": torch.randn(Nn, generator=g).to(DEV)}
    if kind == 1:
        p["residual"] = torch.randn(M, Nn, generator=g).half().to(DEV)
    return p


def _plain(N, p, kind):
    return N.linear_gemm(p["x"], p["w"], bias=p["bias"], residual=p.get("residual"), quickgelu=kind == 2, out_bf16=kind != 1, out_f16=kind == 1)


# kind 0 bias -> bf16, 1 bias + fp16 residual -> fp16 (K <= 1024: the residual first, else behind the bias), 2 bias + QuickGELU -> bf16
BLOCK = [(2304, 768, 0), (768, 768, 1), (3072, 768, 2), (768, 3072, 1)]          # image tower: qkv, out_proj, c_fc, c_proj
TEXT = [(1536, 512, 0), (512, 512, 1), (2048, 512, 2), (512, 2048, 1)]           # text tower
PLAIN = ([(12800, n, k, kind) for n, k, kind in BLOCK] + [(10499, n, k, kind) for n, k, kind in TEXT]
         + [(12544, n, k, kind) for n, k, kind in BLOCK] + [(137 * 50, n, k, kind) for n, k, kind in BLOCK]
         + [(2049, 256, 512, 0), (300, 256, 1088, 1), (5000, 1024, 576, 2), (130, 512, 1024, 1)])


def _epi(N, kind):
    return N.EPI_BIAS | ({0: N.EPI_OUT_BF16, 1: N.EPI_RESIDUAL | N.EPI_RES_F16 | N.EPI_OUT_F16, 2: N.EPI_QUICKGELU | N.EPI_OUT_BF16}[kind])


def test_the_route_cases_reach_every_form():
    # (so that the mode-8 comparisons below compare the 160-row form with the wide kernel, not only the wide kernel with itself)
    import cmh_native as N
    try:
        N.set_gemm_lc(8)
        plain = {N.gemm_route((M, Nn, K), None, _epi(N, kind)) for M, Nn, K, kind in PLAIN}
        grouped = {N.gemm_route(a, b, _epi(N, kind)) for a, b, kind in GROUPED}
    finally:
        N.set_gemm_lc(-1)
    assert plain == {0, 3} and grouped == {0, 3}


@pytest.mark.parametrize("mode", [9, 8])
@pytest.mark.parametrize("case", range(len(PLAIN)))
def test_lc3_plain_launch_gives_the_wide_kernels_bits(case, mode):
    import cmh_native as N
    M, Nn, K, kind = PLAIN[case]
    g = torch.Generator().manual_seed(1000 + case)
    p = _problem(M, Nn, K, kind, g)
    try:
        N.set_gemm_rows(0)
        N.set_gemm_lc(0)
        ref = _plain(N, p, kind)
        N.set_gemm_lc(mode)
        if mode == 9:
            assert N.gemm_route((M, Nn, K), None, _epi(N, kind)) == 3
        got = _plain(N, p, kind)
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    assert torch.equal(ref, got)


GROUPED = [((12800, n, k), (10499, nt, kt), kind) for (n, k, kind), (nt, kt, _) in zip(BLOCK, TEXT)] + [
    ((12544, 2304, 768), (6850, 1536, 512), 0),
    ((2049, 512, 1024), (2500, 256, 1024), 1),
]


@pytest.mark.parametrize("mode", [9, 8])
@pytest.mark.parametrize("case", range(len(GROUPED)))
def test_lc3_grouped_launch_gives_the_wide_kernels_bits(case, mode):
    import cmh_native as N
    (Ma, Na, Ka), (Mb, Nb, Kb), kind = GROUPED[case]
    g = torch.Generator().manual_seed(1100 + case)
    probs = [_problem(Ma, Na, Ka, kind, g), _problem(Mb, Nb, Kb, kind, g)]
    md = torch.tensor([Mb - 37], dtype=torch.int32, device=DEV)      # a device-side row count smaller than M (packed captions)
    out = "f16" if kind == 1 else "bf16"
    try:
        N.set_gemm_lc(0)
        ref = [_plain(N, p, kind) for p in probs]
        N.set_gemm_lc(mode)
        if mode == 9:
            assert N.gemm_route((Ma, Na, Ka), (Mb, Nb, Kb), _epi(N, kind)) == 3
        got = N.linear_gemm_grouped(probs, quickgelu=kind == 2, out=out)
        got_md = N.linear_gemm_grouped(probs, quickgelu=kind == 2, out=out, m_dev=(None, md))
    finally:
        N.set_gemm_lc(-1)
    for r, o in zip(ref, got):
        assert torch.equal(r, o)
    assert torch.equal(got_md[0], ref[0]) and torch.equal(got_md[1][:Mb - 37], ref[1][:Mb - 37])


# ---- the edges of the tile deal the loader / consumer kernels share (csrc/cmh_common.h: deal_share / deal_count / deal_tile; gemm_lc.hip:
# LcSchedule), under every form that deals with it: the 8-wave kernel (mode 1), the 12-wave forms on 128 rows (4) and 160 rows (9), the
# e4m3 form (7).  Small shapes, each against the wide kernel's bits.
FORM = {1: 1, 4: 2, 9: 3}                  # mode -> gemm_route's answer
FAMILY = {1: 3, 4: 4, 9: 5, 7: 6}          # mode -> cmh_gemm_plan's family (GEMM_LC, GEMM_LC2, GEMM_LC3, GEMM_LC2Q)
# (M, N, K, kind):
#  161 x 256: two tiles on a grid of 8 - six workgroups return at once, the second tile is a one-row tail
#  4641 x 2304: 30 x 9 = 270 tiles of 160 rows (37 x 9 of 128) on 256 workgroups - total % 8 != 0, some workgroups take two tiles and
#  park stores, the last m-tile is partial
#  kind 1 at K = 512 / 1088: the residual first / behind the bias
EDGE_PLAIN = [(161, 256, 512, 0), (4641, 2304, 512, 0), (161, 256, 512, 1), (161, 256, 1088, 1)]
# grouped, residual-free (the two K take different residual forms).  The longer K runs first.  First case: every XCD that has a tile of
# the second problem has one of the first, each workgroup runs one and then the other.  Second case: the first problem is one tile
# of 160 rows (two of 128) against four of the second, so the workgroups of the next XCDs start in the second problem (n_first == 0)
EDGE_GROUPED = [((161, 256, 512), (130, 512, 1024)), ((161, 512, 512), (130, 256, 1024))]


def _reached(N, mode, a, b, epi, dt=None):
    if mode in FORM:
        assert N.gemm_route(a, b, epi) == FORM[mode]
    plan = N.gemm_plan(a, b, epi, dt)[1]      # (the e4m3 form is not one of gemm_route's answers: the plan's family says it)
    assert [p["family"] for p in plan] == [FAMILY[mode]]


@pytest.mark.parametrize("mode", [1, 4, 9])
@pytest.mark.parametrize("case", range(len(EDGE_PLAIN)))
def test_deal_edges_plain_launch_gives_the_wide_kernels_bits(case, mode):
    import cmh_native as N
    M, Nn, K, kind = EDGE_PLAIN[case]
    g = torch.Generator().manual_seed(1200 + case)
    p = _problem(M, Nn, K, kind, g)
    try:
        if M <= 2048:
            N.set_gemm_rows(0)
        N.set_gemm_lc(0)
        ref = _plain(N, p, kind)
        N.set_gemm_lc(mode)
        _reached(N, mode, (M, Nn, K), None, _epi(N, kind))
        got = _plain(N, p, kind)
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    assert torch.equal(ref, got)


@pytest.mark.parametrize("case", [0, 1])
def test_deal_edges_plain_e4m3_launch_gives_the_wide_kernels_bits(case):
    import cmh_native as N
    M, Nn, K, _ = EDGE_PLAIN[case]
    g = torch.Generator().manual_seed(1300 + case)
    e4m3 = lambda shape, sc: (torch.randn(*shape, generator=g) * sc).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    x, w = e4m3((M, K), 1.0), e4m3((Nn, K), 8 * K ** -0.5)
    cs, b = (torch.rand(Nn, generator=g) * 0.1 + 0.05).to(DEV), torch.randn(Nn, generator=g).to(DEV)
    try:
        if M <= 2048:
            N.set_gemm_rows(0)
        N.set_gemm_lc(0)
        ref = N.linear_gemm_fp8(x, w, cs, 0.37, bias=b, out="bf16")
        N.set_gemm_lc(7)
        _reached(N, 7, (M, Nn, K), None, N.EPI_BIAS | N.EPI_OUT_BF16, N.FP8)
        got = N.linear_gemm_fp8(x, w, cs, 0.37, bias=b, out="bf16")
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    assert torch.equal(ref, got)


@pytest.mark.parametrize("mode", [1, 4, 9])
@pytest.mark.parametrize("case", range(len(EDGE_GROUPED)))
def test_deal_edges_grouped_launch_gives_the_wide_kernels_bits(case, mode):
    import cmh_native as N
    (Ma, Na, Ka), (Mb, Nb, Kb) = EDGE_GROUPED[case]
    g = torch.Generator().manual_seed(1400 + case)
    probs = [_problem(Ma, Na, Ka, 0, g), _problem(Mb, Nb, Kb, 0, g)]
    md = torch.tensor([Mb - 37], dtype=torch.int32, device=DEV)      # once more with a device-side row count on the second problem
    try:
        N.set_gemm_rows(0)
        N.set_gemm_lc(0)
        ref = [_plain(N, p, 0) for p in probs]
        N.set_gemm_lc(mode)
        _reached(N, mode, (Ma, Na, Ka), (Mb, Nb, Kb), _epi(N, 0))
        got = N.linear_gemm_grouped(probs, out="bf16")
        got_md = N.linear_gemm_grouped(probs, out="bf16", m_dev=(None, md))
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    for r, o in zip(ref, got):
        assert torch.equal(r, o)
    assert torch.equal(got_md[0], ref[0]) and torch.equal(got_md[1][:Mb - 37], ref[1][:Mb - 37])


def test_lc3_never_writes_rows_past_the_device_side_count():
    import ctypes as C
    import cmh_native as N
    g = torch.Generator().manual_seed(17)
    M, Nn, K = 3000, 512, 512
    probs = [_problem(M, Nn, K, 0, g), _problem(M, Nn, K, 0, g)]
    md = torch.tensor([1234], dtype=torch.int32, device=DEV)
    outs = [torch.full((M, Nn), -7.0, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    structs = [N.GemmProblem(N.ptr(p["x"]), N.ptr(p["w"]), N.ptr(p["bias"]), N.ptr(None), N.ptr(o), M, Nn, K, N.ptr(m), N.ptr(None), 1.0, 1.0)
               for p, o, m in zip(probs, outs, (None, md))]
    try:
        N.set_gemm_lc(9)
        N.check(N.lib().cmh_linear_gemm_grouped(N.BF16, C.byref(structs[0]), C.byref(structs[1]), N.EPI_BIAS | N.EPI_OUT_BF16,
                                                N.stream_ptr(torch.device(DEV))), "cmh_linear_gemm_grouped")
        torch.cuda.synchronize()
    finally:
        N.set_gemm_lc(-1)
    assert bool((outs[1][1234:] == -7.0).all()) and not bool((outs[1][:1234] == -7.0).all()) and not bool((outs[0] == -7.0).any())
