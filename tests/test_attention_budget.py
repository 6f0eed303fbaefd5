"""Register, scratch and LDS budgets of the bf16 MFMA attention kernels (csrc/attention.hip), read from the compiler's own
kernel-resource-usage remarks for gfx950.  The pair launch (attention_mfma_pair_kernel<NA, NB>, both towers' attentions as one grid)
only pays if every wave of it - image side and text side - runs at three waves per SIMD without scratch, and twelve blocks share a
CU's 160 KB of LDS only at 13 312 bytes per block or less; the single forms keep the occupancies they have had.
CPU only (compiles csrc/attention.hip's device code with hipcc)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of csrc/Makefile
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=on"]

PAIR_FORMS = ((5, 4), (4, 4), (4, 2))                    # (leading side's key tiles, trailing side's): launch_attention_pair's table
SINGLE_WAVES = {2: 4, 4: 3, 6: 2, 8: 2}                  # attention_mfma_kernel<NKT>: waves per SIMD
LDS_MAX = 13312


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel (demangled enough: name<template arguments>): {field: int}}"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile attention.hip"
    obj = tmp_path_factory.mktemp("attn_budget") / "attention.o"
    p = subprocess.run([hipcc] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                          os.path.join(CSRC, "attention.hip"), "-o", str(obj)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stdout[-2000:]
    out, cur = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = out.setdefault(_short(m.group(1)), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    return out


def _short(mangled):
    """_ZN3cmh26attention_mfma_pair_kernelILi5ELi4EEEv... -> attention_mfma_pair_kernel<5,4>"""
    m = re.match(r"_ZN3cmh\d+(attention_mfma(?:_pair)?_kernel)I((?:Li\d+E)+)E", mangled)
    if not m:
        return mangled
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"Li(\d+)E", m.group(2))))


def test_every_pair_form_runs_three_waves_per_simd_without_scratch(usage):
    names = sorted(n for n in usage if n.startswith("attention_mfma_pair_kernel<"))
    assert names == sorted("attention_mfma_pair_kernel<%d,%d>" % f for f in PAIR_FORMS), names
    for n in names:
        u = usage[n]
        print(n, u)
        assert u["Occupancy"] == 3 and u["ScratchSize"] == 0 and u["LDS Size"] <= LDS_MAX, (n, u)
        assert u["VGPRs"] + u["AGPRs"] <= 170, (n, u)          # 512 registers per SIMD lane, three waves


def test_the_single_forms_keep_their_budgets(usage):
    for nkt, waves in SINGLE_WAVES.items():
        n = "attention_mfma_kernel<%d>" % nkt
        assert n in usage, sorted(usage)
        u = usage[n]
        print(n, u)
        assert u["Occupancy"] == waves and u["ScratchSize"] == 0, (n, u)
