"""Register, scratch and hazard budget of gemm_lc3g_kernel (csrc/gemm_lc.hip: the 160-row 12-wave GEMM's form for bias + QuickGELU
launches), read from the compiler's own kernel-resource-usage remarks and from the gfx950 assembly.  The form only pays at three
waves per SIMD - at most 168 registers - without scratch anywhere: its straight-line K-steps, which carry the parked pieces, are not
inside the K loop that tools/lc_hazards.py searches for scratch, so the whole kernel's scratch size has to be zero.
CPU only (compiles csrc/gemm_lc.hip's device code with hipcc)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of csrc/Makefile
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=on"]
KERNEL = r"_ZN3cmh16gemm_lc3g_kernel"
INSTANCES = 4                                              # grouped or not x bf16 or fp16 output


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """({mangled name: {field: int}}, {mangled name: [assembly lines]}) of the gemm_lc3g_kernel instantiations"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile gemm_lc.hip"
    asm = tmp_path_factory.mktemp("lc3g_budget") / "gemm_lc.s"
    p = subprocess.run([hipcc] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                                          os.path.join(CSRC, "gemm_lc.hip"), "-o", str(asm)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stdout[-2000:]
    usage, cur = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = usage.setdefault(m.group(1), {}) if re.match(KERNEL, m.group(1)) else None
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lc_hazards
    finally:
        sys.path.pop(0)
    return usage, lc_hazards.functions(asm.read_text(), KERNEL), lc_hazards


def test_every_instance_runs_three_waves_per_simd_without_scratch(build):
    usage = build[0]
    assert len(usage) == INSTANCES, sorted(usage)
    for n, u in sorted(usage.items()):
        print(n, u)
        assert u["VGPRs"] + u["AGPRs"] <= 168 and u["ScratchSize"] == 0 and u["Occupancy"] == 3, (n, u)


def test_the_hazard_checks_pass(build):
    _, fns, lc_hazards = build
    assert len(fns) == INSTANCES, sorted(fns)
    for n, body in sorted(fns.items()):
        assert lc_hazards.check_function(body) == [], n


def test_a_carrying_k_step_holds_what_it_should(build):
    """Between the kernel's first and last MFMA lie the three straight-line K-steps and the K loop: 4 x 40 MFMAs, per parked piece 8
    v_exp_f32, 8 v_rcp_f32, 4 packs, 2 lane-pair exchanges and one 16-byte store - and no packed-f32 VALU, no scratch access, no LDS access but the fragment reads."""
    _, fns, _ = build
    for n, body in sorted(fns.items()):
        ops = [line.split(";")[0].split()[0] for line in body if line.split(";")[0].strip() and not line.split(";")[0].strip().endswith(":")
               and not line.lstrip().startswith(".")]
        mf = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
        assert len(mf) == 160, (n, len(mf))
        span = ops[mf[0]:mf[-1] + 1]
        count = {k: sum(op.startswith(k) for op in span) for k in
                 ("v_exp_f32", "v_rcp_f32", "v_cvt_pk_", "v_permlane16_swap", "global_store_dwordx4", "v_pk_", "scratch_", "ds_")}
        print(n, count)
        assert count["v_exp_f32"] == 24 and count["v_rcp_f32"] == 24 and count["v_cvt_pk_"] == 12, (n, count)
        assert count["v_permlane16_swap"] == 6 and count["global_store_dwordx4"] == 3, (n, count)
        assert count["v_pk_"] == 0 and count["scratch_"] == 0, (n, count)
        assert count["ds_"] == sum(op == "ds_read_b128" for op in span), (n, count)
