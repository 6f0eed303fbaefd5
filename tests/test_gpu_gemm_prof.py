"""The measurement hook of the GEMM launch path (csrc/gemm.hip: prof_open / prof_close; include/cmh.h: cmh_prof_gemm_*): one session over
one launch of each kind, at the smallest shapes that reach it.  The hook counts a launch per plan (include/cmh.h: cmh_gemm_plan),
algorithmic FLOPs on real rows, and files each launch under one of three names: the wide kernel and every loader / consumer form under
"gemm_wide_kernel", the few-row kernel under "gemm_rows_kernel", the 128 x 128 kernel under "fallback".  Outputs do not depend on it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE, ROWS, FALLBACK, LC, LC2, LC3, LC2Q = range(7)
NAME = {WIDE: "gemm_wide_kernel", LC: "gemm_wide_kernel", LC2: "gemm_wide_kernel", LC3: "gemm_wide_kernel", LC2Q: "gemm_wide_kernel",
        ROWS: "gemm_rows_kernel", FALLBACK: "fallback"}
REAL_ROWS = 2063      # the device-side row count of the grouped launch's second problem (M = 2100 is its upper bound)


def _launches(N):
    """[(name, switches, family expected or None, dt, epi, a, b, real FLOPs, call)]; a / b as cmh_gemm_plan takes them"""
    g = torch.Generator().manual_seed(77)

    def bf16(M, K):
        return (torch.randn(M, K, generator=g) * K ** -0.5).bfloat16().to(DEV)

    def fp8(M, K):
        return N.fp8_quantize((torch.randn(M, K, generator=g) * K ** -0.5).to(DEV), 1.0 / 64)

    def bias(n):
        return torch.randn(n, generator=g).to(DEV)
    out = []

    def plain(name, switches, family, M, Nn, K, with_bias=False):
        x, w, b = bf16(M, K), bf16(Nn, K), bias(Nn) if with_bias else None
        epi = (N.EPI_BIAS | N.EPI_OUT_BF16) if with_bias else 0
        out.append((name, switches, family, N.BF16, epi, (M, Nn, K), None, 2.0 * M * Nn * K,
                    lambda: [N.linear_gemm(x, w, bias=b, out_bf16=with_bias)]))

    def plain_fp8(name, family, M, Nn, K):
        x, w, cs, b = fp8(M, K), fp8(Nn, K), torch.rand(Nn, generator=g).to(DEV) + 0.5, bias(Nn)
        out.append((name, {}, family, N.FP8, N.EPI_BIAS | N.EPI_OUT_BF16, (M, Nn, K), None, 2.0 * M * Nn * K,
                    lambda: [N.linear_gemm_fp8(x, w, cs, 0.25, bias=b, out="bf16")]))

    plain("rows", {}, ROWS, 64, 256, 64)
    plain("wide", {}, WIDE, 2049, 256, 256)
    plain("lc3", {"lc": 9}, LC3, 2049, 256, 512, with_bias=True)
    plain("fallback", {"rows": 0}, FALLBACK, 130, 128, 64)      # (the few-row kernel would take 130 rows: switched off for this one)
    plain_fp8("fp8 wide", WIDE, 2049, 256, 512)
    plain_fp8("fp8 rows", ROWS, 64, 256, 128)
    pa = {"x": bf16(2049, 512), "w": bf16(256, 512), "bias": bias(256)}
    pb = {"x": bf16(2100, 512), "w": bf16(512, 512), "bias": bias(512)}
    md = torch.tensor([REAL_ROWS], dtype=torch.int32, device=DEV)
    out.append(("grouped", {}, None, N.BF16, N.EPI_BIAS | N.EPI_OUT_BF16, (2049, 256, 512), (2100, 512, 512, 1, 0),
                2.0 * 2049 * 256 * 512 + 2.0 * REAL_ROWS * 512 * 512,
                lambda: N.linear_gemm_grouped([pa, pb], out="bf16", m_dev=(None, md))))
    return out


def _run(N, launches):
    """every launch under its switches -> (outputs, the plan's launches of each)"""
    outs, plans = [], []
    try:
        for name, sw, family, dt, epi, a, b, _, call in launches:
            N.set_gemm_lc(sw.get("lc", -1))
            N.set_gemm_rows(sw.get("rows", -1))
            plan = N.gemm_plan(a, b, epi, dt)[1]
            if family is not None:
                assert [p["family"] for p in plan] == [family], name
            plans.append(plan)
            outs.append(call())
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    torch.cuda.synchronize()
    return outs, plans


def test_one_session_over_every_kind_of_launch():
    import cmh_native as N
    launches = _launches(N)
    ref, _ = _run(N, launches)
    N.prof_gemm_begin(32)
    try:
        got, plans = _run(N, launches)
    finally:
        ms, flops, n = N.prof_gemm_end()
    by = N.prof_gemm_by_kernel()
    print("session:", ms, "ms", flops, "FLOPs", n, "launches;", by, "; plans:", plans)
    assert n == sum(len(p) for p in plans)
    assert flops == sum(l[7] for l in launches)                      # doubles of integers: exact
    want = {k: 0 for k in by}
    for plan in plans:
        for p in plan:
            want[NAME[p["family"]]] += 1
    assert {k: v[2] for k, v in by.items()} == want and all(want.values())
    assert sum(v[1] for v in by.values()) == flops
    for k, (k_ms, _, k_n) in by.items():
        assert k_ms > 0, k
    assert ms > 0
    # in the grouped launch the rows behind the device-side count are not written: compare what is
    for (name, *_), r, o in zip(launches, ref, got):
        for i, (a, b) in enumerate(zip(r, o)):
            rows = REAL_ROWS if (name == "grouped" and i == 1) else a.shape[0]
            assert torch.equal(a[:rows], b[:rows]), name
    # a second session starts from zero
    N.prof_gemm_begin(8)
    ms2, flops2, n2 = N.prof_gemm_end()
    assert (ms2, flops2, n2) == (0.0, 0.0, 0)
    assert all(v == (0.0, 0.0, 0) for v in N.prof_gemm_by_kernel().values())
