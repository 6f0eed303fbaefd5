"""The 160-row 12-wave GEMM's form for bias + QuickGELU launches (csrc/gemm_lc.hip: gemm_lc3g_kernel - three of a tile's ten output
pieces are parked as f32 pre-activations and activated, packed and stored under the next tile's first K-steps).  Another schedule of
the same arithmetic, so every comparison is torch.equal against the wide kernel (cmh_set_gemm_lc(0)) with the 160-row form forced
(cmh_set_gemm_lc(9)); every case runs twice.  CMH_LC3_DGE=0 sends the same launches to gemm_lc3_kernel: compared with the default.

The shapes (all bias + QuickGELU, bf16 output):
  (a) 2100 x 5120 x 512: 14 x 20 = 280 tiles on 256 workgroups - some take two tiles (the first parks, the second finishes in its
      epilogue) and some one; the last row tile has 20 rows; eight K-steps is the kernel's minimum
  (b) the same with a device row count of 2000 under the host's 2100.  Only the grouped call takes a device row count
      (include/cmh.h: CmhGemmProblem.m_dev), so (b) is the launch of (c) with that count on its first problem
  (c) grouped with 2060 x 2048 x 512: a tile parked in the first problem is stored after the switch to the second (other `out`, N, M)
  (d) 2049 x 256 x 768: 13 tiles, one per workgroup at most - nothing is ever parked"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = (2100, 5120, 512)
B2 = (2060, 2048, 512)
D = (2049, 256, 768)


def _problem(shape, g):
    M, Nn, K = shape
    return {"x": torch.randn(M, K, generator=g).bfloat16().to(DEV), "w": (torch.randn(Nn, K, generator=g) * K ** -0.5).bfloat16().to(DEV),
            "bias": torch.randn(Nn, generator=g).to(DEV)}


def _plain(N, p):
    return N.linear_gemm(p["x"], p["w"], bias=p["bias"], quickgelu=True, out_bf16=True)


@pytest.fixture(scope="module")
def data():
    """the operands and the wide kernel's outputs, computed once"""
    import cmh_native as N
    g = torch.Generator().manual_seed(3100)
    ps = {"a": _problem(A, g), "b2": _problem(B2, g), "d": _problem(D, g)}
    try:
        N.set_gemm_rows(0)
        N.set_gemm_lc(0)
        ref = {k: _plain(N, p) for k, p in ps.items()}
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)
    torch.cuda.synchronize()
    return ps, ref


def _forced(fn):
    """fn() under the forced 160-row form, and the library's switches put back"""
    import cmh_native as N
    try:
        N.set_gemm_rows(0)
        N.set_gemm_lc(9)
        return fn(N)
    finally:
        N.set_gemm_lc(-1)
        N.set_gemm_rows(-1)


def _epi(N):
    return N.EPI_BIAS | N.EPI_QUICKGELU | N.EPI_OUT_BF16


@pytest.mark.parametrize("case", ["a", "d"])
def test_plain_launch_gives_the_wide_kernels_bits_twice(data, case):
    ps, ref = data
    shape = {"a": A, "d": D}[case]

    def run(N):
        assert N.gemm_route(shape, None, _epi(N)) == 3
        return [_plain(N, ps[case]) for _ in range(2)]
    for got in _forced(run):
        assert torch.equal(got, ref[case])


@pytest.mark.parametrize("rows", [None, 2000])
def test_grouped_launch_gives_the_wide_kernels_bits_twice(data, rows):
    ps, ref = data
    md = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=DEV)
    n0 = A[0] if rows is None else rows

    def run(N):
        assert N.gemm_route(A, B2, _epi(N)) == 3
        return [N.linear_gemm_grouped([ps["a"], ps["b2"]], quickgelu=True, out="bf16", m_dev=(md, None)) for _ in range(2)]
    for got in _forced(run):
        assert torch.equal(got[0][:n0], ref["a"][:n0])
        assert torch.equal(got[1], ref["b2"])


def test_the_switch_selects_the_plain_form_and_both_agree(data):
    ps, ref = data
    old = os.environ.get("CMH_LC3_DGE")

    def run(N):
        out = {}
        for sw in ("0", None):
            if sw is None:
                os.environ.pop("CMH_LC3_DGE", None)
            else:
                os.environ["CMH_LC3_DGE"] = sw
            out[sw] = [_plain(N, ps["a"]), _plain(N, ps["d"])] + N.linear_gemm_grouped([ps["a"], ps["b2"]], quickgelu=True, out="bf16")
        return out
    try:
        got = _forced(run)
    finally:
        if old is None:
            os.environ.pop("CMH_LC3_DGE", None)
        else:
            os.environ["CMH_LC3_DGE"] = old
    for x, y in zip(got["0"], got[None]):
        assert torch.equal(x, y)
    for x, r in zip(got[None], [ref["a"], ref["d"], ref["a"], ref["b2"]]):
        assert torch.equal(x, r)
