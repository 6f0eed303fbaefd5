"""The per-launch GEMM route (csrc/gemm_lc.hip: gemm_lc_form; include/cmh.h: cmh_gemm_route) on configs[1]'s block launches: which
kernel the default mode gives each plain and grouped launch, and the rules the per-shape table (profiles/r06_a_lc_per_shape.txt)
added to the cost model.  Host-only: nothing is launched, so no GPU is needed (the model assumes 256 CUs without one, as on MI355X)."""
import pytest

import cmh_native as N

R, B, G = N.EPI_RESIDUAL, N.EPI_BIAS, N.EPI_QUICKGELU
EPI = {0: B | N.EPI_OUT_BF16, 1: B | R | N.EPI_RES_F16 | N.EPI_OUT_F16, 2: B | G | N.EPI_OUT_BF16}
BLOCK = {   # name: (image, text, kind)  kind 0 bias, 1 fp16 residual stream, 2 QuickGELU
    "qkv": ((12800, 2304, 768), (10499, 1536, 512), 0),
    "out": ((12800, 768, 768), (10499, 512, 512), 1),
    "fc1": ((12800, 3072, 768), (10499, 2048, 512), 2),
    "fc2": ((12800, 768, 3072), (10499, 512, 2048), 1),
}
WIDE, LC2, LC3 = 0, 2, 3
# what the default route gives each launch (v_ image plain, t_ text plain, g_ the pair path's grouped launch)
EXPECTED = {"v_qkv": LC3, "t_qkv": WIDE, "g_qkv": LC3, "v_out": WIDE, "t_out": WIDE, "g_out": WIDE,
            "v_fc1": LC3, "t_fc1": WIDE, "g_fc1": LC3, "v_fc2": WIDE, "t_fc2": WIDE, "g_fc2": WIDE}


def _routes():
    out = {}
    for name, (im, tx, kind) in BLOCK.items():
        out["v_" + name] = N.gemm_route(im, None, EPI[kind])
        out["t_" + name] = N.gemm_route(tx, None, EPI[kind])
        out["g_" + name] = N.gemm_route(im, tx, EPI[kind])
    return out


@pytest.fixture
def mode():
    def set_(m):
        N.set_gemm_lc(m)
    yield set_
    N.set_gemm_lc(-1)


def test_default_route_of_the_block_launches(mode):
    mode(8)
    assert _routes() == EXPECTED


def test_forced_modes(mode):
    for m, form in ((0, WIDE), (4, LC2), (9, LC3)):
        mode(m)
        assert set(_routes().values()) == {form}, m


def test_route_rules(mode):
    mode(8)
    for M in (2049, 6850, 10499, 12544, 12800, 25600):
        for Nn, K in ((512, 512), (768, 768), (768, 3072), (512, 2048), (1024, 1088), (2304, 768)):
            assert N.gemm_route((M, Nn, K), None, EPI[1]) == WIDE               # no residual launch on a 12-wave form
            assert N.gemm_route((M, Nn, K), None, EPI[0]) in (WIDE, LC3)        # the 128-row form is an opt-in (mode 4)
            assert N.gemm_route((M, Nn, K), (M // 2, Nn, K), EPI[2]) in (WIDE, LC3)
    assert N.gemm_route((12800, 2304, 768), None, N.EPI_BIAS, dt=N.F32) == WIDE   # f32 operands: the wide kernel only
    assert N.gemm_route((12800, 2304, 256), None, N.EPI_BIAS | N.EPI_OUT_BF16) == WIDE  # 4 K-steps: too short for a 12-wave form


def test_removed_modes_are_refused():
    for m in (5, 6, 10):
        with pytest.raises(N.NativeError):
            N.set_gemm_lc(m)
    N.set_gemm_lc(-1)
