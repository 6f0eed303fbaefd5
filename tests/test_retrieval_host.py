"""CPU checks of the retrieval layer: host-side argument validation of cmh_hamming_hist / cmh_hamming_topk (nothing is launched),
the workspace query, the reductions from counts / hit flags to curves on hand-made arrays, and retrieve.py's command line."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT


def test_argument_validation_of_the_retrieval_entry_points():
    import cmh_native as N
    lib = N.lib()
    k_max = int(re.search(r"#define\s+CMH_TOPK_MAX\s+(\d+)", open(os.path.join(ROOT, "include", "cmh.h")).read()).group(1))
    assert k_max >= 5000
    p = 256                      # a non-null address that is never dereferenced: every call below is refused before any launch
    hist = lambda *, qs=p, labels=(None, None), Q=4, n=100, bits=64, classes=24, counts=p, ws=p, wsb=1 << 30: lib.cmh_hamming_hist(
        qs, p, labels[0], p, p, labels[1], Q, n, bits, classes, counts, ws, wsb, None)
    topk = lambda *, qs=p, labels=(None, None), Q=4, n=100, bits=64, classes=24, k=10, idx=p, rel=None, ws=p, wsb=1 << 30: lib.cmh_hamming_topk(
        qs, p, labels[0], p, p, labels[1], Q, n, bits, classes, k, idx, p, rel, None, ws, wsb, None)
    calls = [
        lambda: lib.cmh_hamming_hist(*([None] * 6), 4, 100, 64, 24, None, None, 0, None),
        lambda: lib.cmh_hamming_topk(*([None] * 6), 4, 100, 64, 24, 10, None, None, None, None, None, 0, None),
        lambda: hist(qs=None), lambda: hist(counts=None), lambda: topk(idx=None),
        lambda: hist(labels=(p, None)), lambda: topk(labels=(None, p)), lambda: topk(rel=p),
        lambda: topk(k=0), lambda: topk(k=-3), lambda: topk(k=k_max + 1, n=k_max), lambda: topk(k=101),
        lambda: hist(bits=2049), lambda: topk(bits=2049), lambda: hist(bits=0),
        lambda: hist(labels=(p, p), classes=2049), lambda: topk(labels=(p, p), classes=0),
        lambda: hist(Q=0), lambda: topk(Q=65536), lambda: hist(n=0), lambda: topk(n=1 << 19, k=10),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc == -1, (i, rc)
        assert len(lib.cmh_last_error()) > 0
    assert topk(k=0) == -1 and b"k=0" in lib.cmh_last_error()
    assert hist(bits=2049) == -1 and b"bits=2049" in lib.cmh_last_error()
    # a workspace that is missing or too small is refused too (status -2), before any launch
    assert hist(ws=None, wsb=0) == -2 and topk(ws=p, wsb=16) == -2 and b"workspace" in lib.cmh_last_error()


def test_retrieval_workspace_bytes():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_retrieval_workspace_bytes(0, 0, 64) == 0
    assert lib.cmh_retrieval_workspace_bytes(0, 1000, 64) == 0 and lib.cmh_retrieval_workspace_bytes(10, 0, 64) == 0
    assert lib.cmh_retrieval_workspace_bytes(10, 1000, 0) == 0 and lib.cmh_retrieval_workspace_bytes(10, 1000, 4096) == 0
    small = lib.cmh_retrieval_workspace_bytes(64, 1000, 64)
    assert small >= 2 * 129 * 64 * 4                    # at least one column image and the offsets of one query tile
    for Q, n, bits in ((5000, 190834, 128), (65535, 524287, 128), (65535, 524287, 2048), (1, 1, 16)):
        assert 0 < lib.cmh_retrieval_workspace_bytes(Q, n, bits) <= (300 << 20), (Q, n, bits)      # batches of query tiles bound it


def test_bindings_refuse_cpu_tensors_and_bad_operands():
    import cmh_native as N
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(N.NativeError):
        N.hamming_hist((z(4, 2), z(4, 2)), (z(9, 2), z(9, 2)), 64)
    with pytest.raises(N.NativeError):
        N.hamming_topk((z(4, 2), z(4, 2)), (z(9, 2), z(9, 2)), 64, 3)


def test_curves_from_hand_made_counts():
    from utils.retrieval import curves_from_counts
    # 3 queries, 4 radii; [h, 0] = others, [h, 1] = relevant
    counts = torch.tensor([
        [[0, 0], [1, 1], [0, 2], [3, 1]],      # empty ball at h = 0; 4 relevant items
        [[2, 0], [0, 0], [1, 0], [5, 0]],      # no relevant item: left out of numerator and denominator
        [[0, 1], [0, 0], [4, 0], [0, 3]],      # 4 relevant items
    ], dtype=torch.int32)
    p, r = curves_from_counts(counts)
    assert p.dtype == torch.float64 and r.dtype == torch.float64
    p0, r0 = [0.0, 1 / 2, 3 / 4, 4 / 8], [0.0, 1 / 4, 3 / 4, 1.0]
    p2, r2 = [1.0, 1.0, 1 / 5, 4 / 8], [1 / 4, 1 / 4, 1 / 4, 1.0]
    assert p.tolist() == [(a + b) / 2 for a, b in zip(p0, p2)]
    assert r.tolist() == [(a + b) / 2 for a, b in zip(r0, r2)]
    # nobody has a relevant item: all zeros, no division by zero
    p, r = curves_from_counts(counts[1:2])
    assert p.tolist() == [0.0] * 4 and r.tolist() == [0.0] * 4
    # counts add over query shards: the curve of the whole set is the one of the concatenation
    both = curves_from_counts(torch.cat([counts[:1], counts[2:]]))
    assert both[0].tolist() == curves_from_counts(counts)[0].tolist()


def test_topn_from_hand_made_hit_flags():
    from utils.retrieval import topn_from_rel
    rel = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 1, 0, 0, 0]], dtype=torch.uint8)
    relevant = torch.tensor([6, 0, 1])
    p, r = topn_from_rel(rel, relevant, (1, 2, 5))
    assert p.tolist() == [(1 / 1 + 0 / 1) / 2, (1 / 2 + 1 / 2) / 2, (3 / 5 + 1 / 5) / 2]
    assert r.tolist() == [(1 / 6 + 0 / 1) / 2, (1 / 6 + 1 / 1) / 2, (3 / 6 + 1 / 1) / 2]
    p, r = topn_from_rel(rel[1:2], relevant[1:2], (1, 5))
    assert p.tolist() == [0.0, 0.0] and r.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        topn_from_rel(rel, relevant, (1, 6))
    with pytest.raises(ValueError):
        topn_from_rel(rel, relevant, (0,))


def test_eval_curves_flag_is_off_by_default(monkeypatch):
    import argsbase
    monkeypatch.setattr(sys, "argv", ["main.py"])
    assert argsbase.get_baseargs().parse_known_args([])[0].eval_curves is False
    assert argsbase.get_baseargs().parse_known_args(["--eval-curves", "true"])[0].eval_curves is True


def test_retrieve_cli_help_runs_without_a_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--help"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--codes" in out.stdout and "--direction" in out.stdout and "--queries" in out.stdout and "i2t" in out.stdout
    import retrieve
    assert retrieve.query_slice(":", 7) == (0, 7) and retrieve.query_slice("2:5", 7) == (2, 5) and retrieve.query_slice("3:", 7) == (3, 7)
    with pytest.raises(SystemExit):
        retrieve.query_slice("5:9", 7)
