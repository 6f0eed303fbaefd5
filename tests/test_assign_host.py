"""CPU checks around DNPH's noise assignment on the GPU: the --noise-assign flag, the ABI's two entry points and their host-side
refusals (nothing is launched), and the untouched host path."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from heads2util import DNPH_CASES, dnph_case


def _args(monkeypatch, *cli):
    from train.DNPH_TOMM.get_args import get_args
    monkeypatch.setattr(sys, "argv", ["main.py", *cli])
    return get_args(argparse.Namespace(method="DNPH", dataset="synthetic", output_dim=16, is_train=True))


def test_noise_assign_flag(monkeypatch):
    assert _args(monkeypatch).noise_assign == "gpu"
    assert _args(monkeypatch, "--noise-assign", "host").noise_assign == "host"
    assert _args(monkeypatch, "--noise-assign", "gpu").noise_assign == "gpu"
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--noise-assign", "cpu")


def test_header_and_binding_carry_both_entry_points():
    import cmh_native as N
    src = open(os.path.join(ROOT, "include", "cmh.h")).read()
    assert "train/DNPH_TOMM/b_reg.py:5-40" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("cmh_assign_rows_workspace_bytes", "cmh_assign_rows"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in N.SIGNATURES
    assert len(N.SIGNATURES["cmh_assign_rows"][1]) == 10 and len(N.SIGNATURES["cmh_assign_rows_workspace_bytes"][1]) == 2
    assert re.search(r"#define\s+CMH_VERSION\s+6\b", src) and N.ABI_VERSION == 6


def test_host_side_refusals_and_workspace_size():
    import cmh_native as N
    lib = N.lib()
    size = lib.cmh_assign_rows_workspace_bytes
    assert size(2, 256) >= 2 * 256 * 256 * 8 + 2 * 256 * 4 and size(2, 256) % 256 == 0
    assert size(1, 1) > 0 and size(3, 1024) >= 3 * 1024 * 1024 * 8
    assert size(2, 0) == 0 and size(2, 1025) == 0 and size(0, 16) == 0
    one = 1                                                                      # any non-null address: nothing is launched
    for P, B, K, ws in ((2, 1025, 16, 1 << 30), (2, 0, 16, 1 << 30), (0, 16, 16, 1 << 30), (2, 16, 0, 1 << 30)):
        assert lib.cmh_assign_rows(one, one, P, B, K, one, None, one, ws, None) == -1 and len(lib.cmh_last_error()) > 0
    assert lib.cmh_assign_rows(None, one, 2, 16, 8, one, None, one, 1 << 30, None) == -1 and b"null" in lib.cmh_last_error()
    assert lib.cmh_assign_rows(one, one, 2, 16, 8, one, None, one, size(2, 16) - 1, None) < 0 and b"workspace" in lib.cmh_last_error()


def test_assign_noise_refuses_an_unknown_path():
    import torch
    from train.DNPH_TOMM.b_reg import assign_noise
    with pytest.raises(ValueError):
        assign_noise(torch.zeros(2, 4), torch.zeros(2, 4), np.ones((2, 4), dtype=np.int64), "auto")


def test_gene_noise_is_unchanged(golden):
    from train.DNPH_TOMM import b_reg
    from train.DNPH_TOMM.b_reg import assign_noise, gene_noise, rand_unit_rect   # noqa: F401  (all three importable)
    g = golden("dnph.npz")
    c = dnph_case(*DNPH_CASES[0])
    s_vec = g[f"{c['tag']}_s_vec"].astype(np.int64)
    got = gene_noise(c["hi"], s_vec)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, g[f"{c['tag']}_noise_i"].astype(np.float64))
    np.random.seed(3)
    r = rand_unit_rect(5, 7)
    np.random.seed(3)
    want = np.random.randint(0, 2, size=(5, 7))
    want[want == 0] = -1
    assert r.shape == (5, 7) and np.array_equal(r, want)
    assert b_reg.assign_noise.__defaults__ == ("gpu",)
