"""Static checks of the loader / consumer GEMM kernels' gfx950 assembly (tools/lc_hazards.py): no scratch, no scalar load and no
compiler-emitted LDS instruction inside a K-step, and no register of a hand-counted ds_read touched before the s_waitcnt that covers
it - for every instantiation of gemm_lc2_kernel / gemm_lc3_kernel the launchers can select.  CPU only (assembles with hipcc)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lc_hazards as H  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm():
    assert os.path.exists(HIPCC) or shutil.which("hipcc"), "hipcc is needed to assemble gemm_lc.hip"
    return H.assemble()


def test_every_12_wave_instantiation_is_hazard_free(asm):
    fns = H.functions(asm)
    names = sorted(fns)
    # 2 (plain / grouped) x 4 (no residual bf16 / fp16 out, residual first, residual behind the bias) per form
    assert sum("gemm_lc2_kernel" in n for n in names) == 8 and sum("gemm_lc3_kernel" in n for n in names) == 8, names
    findings = {n: H.check_function(fns[n]) for n in names}
    assert all(not f for f in findings.values()), {n: f[:3] for n, f in findings.items() if f}


def test_every_12_wave_k_loop_has_its_mfmas():
    # (the checker's loop depth is the K loop: a body without MFMAs at depth 2 would make every check above vacuous)
    fns = H.functions(H.assemble())
    for name, body in fns.items():
        depth, mfma = 0, 0
        for raw in body:
            if raw.startswith(".LBB") or raw.startswith("; %bb."):
                depth = 2 if "Depth=2" in raw else 0
            elif raw.lstrip().startswith(";") and "Depth=2" in raw:
                depth = 2
            if depth == 2 and raw.strip().startswith("v_mfma"):
                mfma += 1
        assert mfma >= 32, (name, mfma)


def test_the_checker_sees_a_read_used_before_its_wait():
    body = [
        "\tds_read_b128 v[10:13], v2 offset:0",
        "\tds_read_b128 v[14:17], v2 offset:2048",
        "\ts_waitcnt lgkmcnt(1)",
        "\tv_mov_b32_e32 v40, v12",          # covered: the older read has landed
        "\tv_mov_b32_e32 v41, v15",          # NOT covered: one read may still fly
        "\ts_waitcnt lgkmcnt(0)",
        "\tv_mov_b32_e32 v42, v16",
    ]
    f = H.check_function(body)
    assert [k for k, _, _ in f] == ["use-before-wait"] and f[0][1] == 4


def test_the_checker_sees_scratch_and_scalar_loads_in_the_k_loop():
    body = [
        ".LBB0_3:                               ; =>This Inner Loop Header: Depth=2",
        "\tscratch_store_dwordx4 off, v[10:13], off",
        "\ts_load_dword s4, s[0:1], 0x10",
        "\tds_write_b32 v1, v2",
        ".LBB0_4:                               ;   in Loop: Header=BB0_1 Depth=1",
        "\tscratch_load_dwordx4 v[10:13], off, off",
    ]
    assert sorted(k for k, _, _ in H.check_function(body)) == ["lds", "scratch", "smem"]
