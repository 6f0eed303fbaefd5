"""CPU checks of the mAP by counting: the ABI of cmh_map_count_workspace_bytes / cmh_hamming_ap_partial / cmh_ap_finish (declared,
exported, bound; nothing is launched), their refusals, the float64 restatement of tests/mapcountutil.py on a hand-made ranking, and
the flags of the command line and the trainers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

NEW = ("cmh_map_count_workspace_bytes", "cmh_hamming_ap_partial", "cmh_ap_finish")


def test_new_symbols_are_declared_exported_and_bound():
    import cmh_native as N
    lib = N.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmh.h")).read(), flags=re.S)
    exported = set(re.findall(r" T (cmh_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)))
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in exported and name in N.SIGNATURES and getattr(lib, name).argtypes == N.SIGNATURES[name][1]
    assert lib.cmh_version() == N.ABI_VERSION == 6                    # entry points were added, nothing else changed


def test_map_count_workspace_bytes():
    import cmh_native as N
    ws = N.lib().cmh_map_count_workspace_bytes
    assert ws(0, 1000, 64) == 0 and ws(65536, 1000, 64) == 0 and ws(10, 0, 64) == 0 and ws(10, N.TOPK_MAX + 1, 64) == 0
    assert ws(10, 1000, 0) == 0 and ws(10, 1000, 2049) == 0
    # two bases per (chunk, bin, lane), two columns of totals: more than the search's one image and one column
    assert ws(64, 1000, 64) > N.lib().cmh_retrieval_workspace_bytes(64, 1000, 64) >= 2 * 129 * 64 * 4
    for Q, n, bits in ((5000, 190834, 128), (65535, 524287, 128), (65535, 524287, 2048), (1, 1, 16)):
        assert 0 < ws(Q, n, bits) <= (300 << 20), (Q, n, bits)        # batches of query tiles bound it


def test_refusals_of_the_map_count_entry_points():
    import cmh_native as N
    lib = N.lib()
    p = 256                      # a non-null address that is never dereferenced: every call below is refused before any launch

    def part(*, qs=p, ql=p, rl=p, Q=4, n=100, bits=64, classes=24, topk=0, ap_sum=p, ws=p, wsb=1 << 30):
        return lib.cmh_hamming_ap_partial(qs, p, ql, p, p, rl, Q, n, bits, classes, topk, None, None, None, ap_sum, ws, wsb, None)

    def fin(*, s=p, counts=p, Q=4, bits=64, ap=p, mp=p):
        return lib.cmh_ap_finish(s, counts, Q, bits, 0, ap, mp, None)

    refused = [
        (lambda: part(qs=None), b"null"), (lambda: part(ap_sum=None), b"null"),
        (lambda: part(ql=None), b"labels"), (lambda: part(rl=None), b"labels"),
        (lambda: part(Q=0), b"Q=0"), (lambda: part(Q=65536), b"Q=65536"), (lambda: part(n=0), b"N=0"),
        (lambda: part(n=1 << 19), b"exceeds"), (lambda: part(bits=0), b"bits=0"), (lambda: part(bits=2049), b"bits=2049"),
        (lambda: part(classes=0), b"classes=0"), (lambda: part(classes=2049), b"classes=2049"),
        (lambda: part(ws=None, wsb=0), b"workspace"), (lambda: part(wsb=16), b"workspace"),
        (lambda: fin(s=None), b"null"), (lambda: fin(counts=None), b"null"), (lambda: fin(ap=None), b"null"),
        (lambda: fin(mp=None), b"null"), (lambda: fin(Q=0), b"Q=0"), (lambda: fin(bits=0), b"bits=0"), (lambda: fin(bits=2049), b"bits=2049"),
    ]
    for i, (call, word) in enumerate(refused):
        assert call() == -1, i
        assert word in lib.cmh_last_error(), (i, lib.cmh_last_error())


def test_bindings_refuse_cpu_tensors_and_missing_labels():
    import cmh_native as N
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(N.NativeError):
        N.hamming_ap_partial((z(4, 2), z(4, 2)), (z(9, 2), z(9, 2)), 64, z(4, 1), z(9, 1))
    with pytest.raises(N.NativeError, match="labels"):
        N.hamming_ap_partial((z(4, 2), z(4, 2)), (z(9, 2), z(9, 2)), 64, None, None)
    with pytest.raises(N.NativeError):
        N.ap_finish(torch.zeros(4, dtype=torch.float64), z(4, 129, 2), 64)


def test_restatement_on_a_hand_made_ranking():
    import mapcountutil as mu
    # one 4-bit query, five items: h = 0, 4, 4, 8, 0 -> stable order 0, 4, 1, 2, 3; relevant: items 1, 3, 4 -> ranks 2, 3, 5
    qB = np.array([[1, 1, 1, 1]], np.float32)
    rB = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [-1, -1, 1, 1], [-1, -1, -1, -1], [1, 1, 1, 1]], np.float32)
    qL = np.array([[1, 0]], np.float32)
    rL = np.array([[0, 1], [1, 0], [0, 0], [1, 1], [1, 0]], np.float32)
    assert mu.half_units(qB, rB).tolist() == [[0, 4, 4, 8, 0]]
    ref = mu.restated_ap(qB, rB, qL, rL, (None, 1, 2, 7))
    assert ref[None][0][0] == (1 / 2 + 2 / 3 + 3 / 5) / 3 and ref[7] == ref[None]
    assert ref[1][0][0] == 1 / 2 and ref[2][0][0] == (1 / 2 + 2 / 3) / 2
    none = mu.restated_ap(qB, rB, np.zeros_like(qL), rL, (None,))
    assert none[None][0][0] == 0.0 and none[None][1] == 0.0
    for shape in ((1, 1, 16, False, 4), (2, 70, 16, True, 4), (65, 3, 64, True, 80), (130, 1000, 64, True, 100)):
        mu.check_label_mix(*mu.case(*shape)[2:])


def test_flags_of_the_trainers_and_the_command_line(monkeypatch):
    import argsbase
    monkeypatch.setattr(sys, "argv", ["main.py"])
    assert argsbase.get_baseargs().parse_known_args([])[0].map_tie_order == "reference"
    assert argsbase.get_baseargs().parse_known_args(["--map-tie-order", "stable"])[0].map_tie_order == "stable"
    with pytest.raises(SystemExit):
        argsbase.get_baseargs().parse_known_args(["--map-tie-order", "other"])
    import retrieve
    assert retrieve.parse(["--codes", "x.mat"]).map is False and retrieve.parse(["--codes", "x.mat", "--map", "--k", "5"]).k == 5
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--help"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "--map" in out.stdout
