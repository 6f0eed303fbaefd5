"""CPU checks of the graded-relevance layer: utils.retrieval.graded_from_grades (pure host arithmetic) against hand-made values and
against the NumPy restatement of tests/gradedutil.py, host-side argument validation of cmh_hamming_topk_graded /
cmh_label_overlap_hist (nothing is launched), the --eval-graded flag and retrieve.py --graded.

Tolerance of the comparisons with the restatement: both sides are float64 sums of at most max(topn) <= 1000 positive terms in
different orders (the restatement sorts the database's grades for IDCG, the product walks the histogram), so they differ by at most
n * eps ~ 1e-13 relative; asserted: 1e-12."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradedutil as G
from conftest import PKG

RTOL = 1e-12


def _close(got, want):
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), want, rtol=RTOL, atol=0)


def test_graded_from_hand_made_grades():
    from utils.retrieval import graded_from_grades
    grade = torch.tensor([[2, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=torch.uint8)
    # database grades of the three queries: (2, 0, 1, 1, 0), all zero (left out of the means), (0, 1, 0, 0, 0)
    counts = torch.tensor([[2, 2, 1], [5, 0, 0], [4, 1, 0]], dtype=torch.int32)
    ndcg, acg, wap = graded_from_grades(grade, counts, (1, 3))
    l3 = math.log2(3.0)
    q0 = {"ndcg": (3.0 / 3.0, (3.0 + 1.0 / 2.0) / (3.0 + 1.0 / l3 + 1.0 / 2.0)), "acg": (2.0, 1.0), "wap": (2.0, (2.0 + 1.0) / 2.0)}
    q2 = {"ndcg": (0.0, (1.0 / l3) / 1.0), "acg": (0.0, 1.0 / 3.0), "wap": (0.0, 1.0 / 2.0)}
    for got, key in ((ndcg, "ndcg"), (acg, "acg"), (wap, "wap")):
        _close(got, [(a + b) / 2 for a, b in zip(q0[key], q2[key])])
    # nobody has a relevant item: zeros, no division by zero
    for got in graded_from_grades(grade[1:2], counts[1:2], (1, 2, 3)):
        assert got.dtype == torch.float64 and got.tolist() == [0.0, 0.0, 0.0]
    # the restatement agrees on the same rows
    allg = np.array([[2, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 1, 0, 0, 0]])
    np.testing.assert_array_equal(G.histogram(allg, 2), counts.numpy())
    for got, want in zip((ndcg, acg, wap), G.metrics(grade.numpy(), allg, (1, 3))):
        _close(got, want)
    with pytest.raises(ValueError):
        graded_from_grades(grade, counts, (1, 4))
    with pytest.raises(ValueError):
        graded_from_grades(grade, counts, (0,))
    with pytest.raises(ValueError):
        graded_from_grades(grade, counts, ())


def _random_case(seed, Q, N, bits, C, density):
    rng = np.random.default_rng(seed)
    qB = np.where(rng.random((Q, bits)) < 0.5, -1.0, 1.0).astype(np.float32)
    rB = np.where(rng.random((N, bits)) < 0.5, -1.0, 1.0).astype(np.float32)
    qL = (rng.random((Q, C)) < density).astype(np.float32)
    rL = (rng.random((N, C)) < density).astype(np.float32)
    return qB, rB, qL, rL


@pytest.mark.parametrize("Q,N,bits,C,density,topn", [(37, 3000, 64, 24, 0.15, (1, 100, 1000)), (20, 5000, 128, 80, 0.3, (1, 50, 1000)),
                                                      (11, 1500, 16, 255, 0.02, (1, 7, 1000, 1500))])
def test_graded_from_grades_matches_the_numpy_restatement(Q, N, bits, C, density, topn):
    from utils.retrieval import graded_from_grades
    qB, rB, qL, rL = _random_case(Q * 7 + C, Q, N, bits, C, density)
    qL[0] = 0                                      # no relevant item: left out of numerator and denominator
    qL[1] = 0; qL[1, 3] = 1; rL[:, 3] = 0; rL[5, 3] = 1; rL[77, 3] = 1
    qL[2] = 1; rL[9] = 1; rL[10] = 1               # grades up to C (and query 1 has four relevant items: IDCG runs out of non-zero grades)
    k = max(topn)
    allg = G.grades(qL, rL)
    assert allg[0].max() == 0 and (allg[1] > 0).sum() == 4 and allg.max() == C and (allg.max(1) > 0).sum() >= 3
    grade = np.take_along_axis(allg, G.ranking(qB, rB, k), 1)
    counts = G.histogram(allg, C)
    got = graded_from_grades(torch.from_numpy(grade.astype(np.uint8)), torch.from_numpy(counts.astype(np.int32)), topn)
    want = G.metrics(grade, allg, topn)
    for a, b in zip(got, want):
        assert a.shape == (len(topn),)
        _close(a, b)
    ndcg = got[0].numpy()
    assert (ndcg >= 0).all() and (ndcg <= 1 + 1e-12).all()
    if k == N:                                     # the whole database ranked: DCG of a permutation of the ideal order
        assert ndcg[-1] < 1
    # the set of queries without relevant items alone gives zeros
    for z in graded_from_grades(torch.from_numpy(grade[:1].astype(np.uint8)), torch.from_numpy(counts[:1].astype(np.int32)), topn):
        assert z.tolist() == [0.0] * len(topn)


def test_eval_graded_flag_is_off_by_default(monkeypatch):
    import argsbase
    monkeypatch.setattr(sys, "argv", ["main.py"])
    args = argsbase.get_baseargs().parse_known_args([])[0]
    assert args.eval_graded is False and args.eval_curves is False
    args = argsbase.get_baseargs().parse_known_args(["--eval-graded", "true"])[0]
    assert args.eval_graded is True and args.eval_curves is False
    assert argsbase.BASE_FLAGS[-1][0] == "--eval-graded"


def test_retrieve_cli_help_lists_graded_without_a_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--help"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--graded" in out.stdout and "--codes" in out.stdout
    import retrieve
    assert retrieve.parse(["--codes", "x.mat"]).graded is False and retrieve.parse(["--codes", "x.mat", "--graded"]).graded is True


def test_argument_validation_of_the_graded_entry_points():
    import cmh_native as N
    lib = N.lib()
    p = 256                      # a non-null address that is never dereferenced: every call below is refused before any launch
    topk = lambda *, qs=p, labels=(p, p), Q=4, n=100, bits=64, classes=24, k=10, idx=p, grade=p, ws=p, wsb=1 << 30: \
        lib.cmh_hamming_topk_graded(qs, p, labels[0], p, p, labels[1], Q, n, bits, classes, k, idx, p, None, grade, None, ws, wsb, None)
    hist = lambda *, ql=p, rl=p, Q=4, n=100, classes=24, out=p, ws=p, wsb=1 << 30: \
        lib.cmh_label_overlap_hist(ql, rl, Q, n, classes, out, ws, wsb, None)
    calls = [
        lambda: lib.cmh_hamming_topk_graded(*([None] * 6), 4, 100, 64, 24, 10, None, None, None, None, None, None, 0, None),
        lambda: lib.cmh_label_overlap_hist(None, None, 4, 100, 24, None, None, 0, None),
        lambda: topk(qs=None), lambda: topk(idx=None), lambda: topk(grade=None),
        lambda: topk(labels=(None, None)), lambda: topk(labels=(p, None)), lambda: topk(labels=(None, p)),
        lambda: topk(k=0), lambda: topk(k=101), lambda: topk(bits=2049), lambda: topk(classes=0), lambda: topk(classes=256),
        lambda: topk(Q=0), lambda: topk(Q=65536), lambda: topk(n=1 << 19),
        lambda: hist(ql=None), lambda: hist(rl=None), lambda: hist(out=None),
        lambda: hist(classes=0), lambda: hist(classes=256), lambda: hist(classes=2048),
        lambda: hist(Q=0), lambda: hist(Q=65536), lambda: hist(n=0), lambda: hist(n=1 << 19),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc == -1, (i, rc)
        assert len(lib.cmh_last_error()) > 0
    assert topk(classes=256) == -1 and b"classes=256" in lib.cmh_last_error() and b"255" in lib.cmh_last_error()
    assert hist(classes=256) == -1 and b"classes=256" in lib.cmh_last_error() and b"255" in lib.cmh_last_error()
    assert topk(grade=None) == -1 and b"null" in lib.cmh_last_error()
    # a workspace that is missing or too small is refused too (status -2), before any launch
    assert topk(ws=None, wsb=0) == -2 and b"workspace" in lib.cmh_last_error()
    assert hist(ws=None, wsb=0) == -2 and hist(ws=p, wsb=16) == -2 and b"workspace" in lib.cmh_last_error()


def test_label_overlap_workspace_bytes():
    import cmh_native as N
    lib = N.lib()
    f = lib.cmh_label_overlap_workspace_bytes
    assert f(0, 1000, 24) == 0 and f(10, 0, 24) == 0 and f(10, 1000, 0) == 0 and f(10, 1000, 256) == 0 and f(65536, 1000, 24) == 0
    assert f(64, 1000, 24) >= 25 * 64 * 4                    # at least one column image of one query tile
    for Q, n, C in ((5000, 190834, 21), (5000, 15015, 24), (65535, 524287, 255), (1, 524287, 255), (1, 1, 1)):
        assert 0 < f(Q, n, C) <= (80 << 20), (Q, n, C)


def test_graded_bindings_refuse_cpu_tensors_and_bad_operands():
    import cmh_native as N
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    planes = ((z(4, 2), z(4, 2)), (z(9, 2), z(9, 2)))
    with pytest.raises(N.NativeError):
        N.hamming_topk_graded(*planes, 64, 3, z(4, 1), z(9, 1))
    with pytest.raises(N.NativeError):
        N.hamming_topk_graded(*planes, 64, 3, None, None)
    with pytest.raises(N.NativeError):
        N.label_overlap_hist(z(4, 1), z(9, 1), 24)
    with pytest.raises(N.NativeError):
        N.label_overlap_hist(None, z(9, 1), 24)
