"""Graded relevance on the GPU: cmh_hamming_topk_graded / cmh_label_overlap_hist, utils/retrieval.py's graded_* functions, the
trainer's --eval-graded and retrieve.py --graded, against tests/golden/retrieval.npz, the plain search, and the NumPy restatement
of tests/gradedutil.py (grades = qL @ rL.T, np.argsort(stable), the definitions as float64 loops, IDCG from the sorted grades).
Everything integer is compared exactly; the metrics within relative 1e-12 (both sides are float64 sums of at most 1000 positive terms
in different orders: n * eps ~ 1e-13)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradedutil as G
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _packed(qB, rB, qL, rL):
    import cmh_native as N
    return N.pack_codes(_t(qB)), N.pack_codes(_t(rB)), N.pack_labels(_t(qL)), N.pack_labels(_t(rL))


def _case_names():
    return [str(n) for n in np.load(os.path.join(GOLDEN, "retrieval.npz"))["cases"]]


def _check_search(qB, rB, qL, rL, k, want_idx=None):
    """graded search == plain search on idx / dist, grade == (qL @ rL.T) gathered at idx, grade > 0 == rel; also with counts."""
    import cmh_native as N
    bits, C = rB.shape[1], rL.shape[1]
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    idx, dist, rel, counts = N.hamming_topk(qp, rp, bits, k, ql, rl, want_counts=True)
    gi, gd, grade, gcounts = N.hamming_topk_graded(qp, rp, bits, k, ql, rl, want_counts=True, classes=C)
    assert gi.dtype == torch.int32 and gd.dtype == torch.float32 and grade.dtype == torch.uint8 and grade.shape == (qB.shape[0], k)
    assert torch.equal(gi, idx) and torch.equal(gd, dist) and torch.equal(gcounts, counts)
    if want_idx is not None:
        np.testing.assert_array_equal(gi.cpu().numpy(), want_idx)
    allg = G.grades(qL, rL)
    np.testing.assert_array_equal(grade.cpu().numpy().astype(np.int64), np.take_along_axis(allg, idx.cpu().numpy().astype(np.int64), 1))
    assert torch.equal((grade > 0).to(torch.uint8), rel)
    three = N.hamming_topk_graded(qp, rp, bits, k, ql, rl, classes=C)
    assert len(three) == 3 and torch.equal(three[0], idx) and torch.equal(three[1], dist) and torch.equal(three[2], grade)
    return idx, grade, allg


def _check_hist(qL, rL, allg=None):
    import cmh_native as N
    C = rL.shape[1]
    allg = G.grades(qL, rL) if allg is None else allg
    hist = N.label_overlap_hist(N.pack_labels(_t(qL)), N.pack_labels(_t(rL)), C)
    assert hist.dtype == torch.int32 and hist.shape == (qL.shape[0], C + 1)
    h = hist.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(h, G.histogram(allg, C))
    assert (h.sum(1) == rL.shape[0]).all()
    return hist


@pytest.mark.parametrize("name", _case_names())
def test_graded_search_and_label_histogram_on_the_reference_goldens(golden, name):
    import cmh_native as N
    g = golden("retrieval.npz")
    qB, rB, qL, rL = (g[f"{name}_{key}"].astype(np.float32) for key in ("qB", "rB", "qL", "rL"))
    k = int(g[f"{name}_k"])
    _, grade, allg = _check_search(qB, rB, qL, rL, k, want_idx=g[f"{name}_idx"])
    np.testing.assert_array_equal((grade > 0).cpu().numpy().astype(np.uint8), g[f"{name}_rel"])
    hist = _check_hist(qL, rL, allg)
    relevant = g[f"{name}_counts"].astype(np.int64)[:, :, 1].sum(1)
    np.testing.assert_array_equal(rB.shape[0] - hist[:, 0].cpu().numpy().astype(np.int64), relevant)
    if rL.shape[1] <= 32 * 7:      # without `classes` the binding takes what the packed words hold
        qp, rp, ql, rl = _packed(qB, rB, qL, rL)
        assert torch.equal(N.hamming_topk_graded(qp, rp, rB.shape[1], k, ql, rl)[2], grade)


@functools.lru_cache(maxsize=None)
def _random(Q, n, bits, C, zeros, identical, density=0.2):
    rng = np.random.default_rng(Q * 1000 + n + bits + C)
    vals = np.array([-1.0, 1.0, 0.0] if zeros else [-1.0, 1.0], np.float32)
    qB = vals[rng.integers(0, len(vals), (Q, bits))]
    rB = vals[rng.integers(0, len(vals), (n, bits))]
    if identical:
        rB[:] = rB[0]                                     # one tie group: the order is index order
    qL = (rng.random((Q, C)) < density).astype(np.float32)
    rL = (rng.random((n, C)) < density).astype(np.float32)
    qL[0] = 0                                             # a query without relevant items
    qL[-1] = 1; rL[n // 2] = 1                            # the largest grade there is: C
    return qB, rB, qL, rL


# bits 16 / 64 / 128 (columns in LDS), 200 / 512 (columns in the workspace); classes 24 (one word), 40 (staged), 80 (three words), 255;
# codes with zeros; Q not a multiple of 64 and more than one query tile; k = 1 and k = N; a database of identical codes
@pytest.mark.parametrize("Q,n,bits,C,k,zeros,identical", [
    (70, 300, 16, 24, 1, False, False), (65, 257, 64, 40, 257, True, False), (9, 1000, 128, 80, 100, True, False),
    (5, 600, 200, 255, 50, False, False), (4, 500, 512, 24, 77, True, False), (3, 333, 512, 80, 333, False, False),
    (7, 400, 64, 24, 400, False, True), (130, 129, 128, 255, 129, False, False)])
def test_graded_search_on_random_cases(Q, n, bits, C, k, zeros, identical):
    qB, rB, qL, rL = _random(Q, n, bits, C, zeros, identical)
    idx, grade, allg = _check_search(qB, rB, qL, rL, k)
    np.testing.assert_array_equal(idx.cpu().numpy(), G.ranking(qB, rB, k))
    assert int(grade[0].max()) == 0 and int(grade.max()) > 0
    if k == n:
        assert int(grade.max()) == C                      # the item that shares every label with the last query
    if identical:
        np.testing.assert_array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (Q, 1)))


# N > 65 532: several chunks and the reduce, more items than a 16-bit counter holds; one chunk with a tail only; every label path
@pytest.mark.parametrize("Q,n,C", [(70, 70000, 24), (3, 37, 21), (65, 3001, 40), (9, 2999, 80), (5, 1003, 255), (130, 517, 1)])
def test_label_histogram_on_random_cases(Q, n, C):
    import cmh_native as N
    qB, rB, qL, rL = _random(Q, n, 16, C, False, False, density=0.5 if C == 1 else 0.2)
    hist = _check_hist(qL, rL)
    assert int(hist[0, 0]) == n and int(hist[-1, C]) >= 1
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    relevant = N.hamming_hist(qp, rp, 16, ql, rl)[:, :, 1].sum(1)
    assert torch.equal(n - hist[:, 0], relevant.to(hist.dtype))
    assert torch.equal(N.label_overlap_hist(ql, rl, C), hist)      # written once: the same on a second call


def test_graded_entry_points_refuse_more_than_255_classes():
    import cmh_native as N
    qB, rB, qL, rL = _random(3, 50, 16, 256, False, False)
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    with pytest.raises(N.NativeError, match="255"):
        N.hamming_topk_graded(qp, rp, 16, 5, ql, rl, classes=256)
    with pytest.raises(N.NativeError, match="255"):
        N.label_overlap_hist(ql, rl, 256)
    assert N.hamming_topk(qp, rp, 16, 5, ql, rl)[2].shape == (3, 5)      # the plain search takes them as before


@pytest.mark.parametrize("Q,n,bits,C,topn", [(20, 1200, 64, 24, (1, 100, 1000)), (9, 700, 128, 80, (1, 50, 700)), (6, 500, 16, 255, (1, 500))])
def test_graded_metrics_match_the_numpy_restatement(Q, n, bits, C, topn):
    from utils.retrieval import graded_metrics, graded_topk, grade_histogram
    qB, rB, qL, rL = _random(Q, n, bits, C, False, False)
    c = [torch.from_numpy(a) for a in (qB, rB, qL, rL)]      # CPU inputs, as calc_utils takes them
    ndcg, acg, wap, grade = graded_metrics(*c, topn=topn)
    allg = G.grades(qL, rL)
    assert allg[0].max() == 0 and (allg.max(1) > 0).any()    # one query is left out of the means, and not all of them
    k = max(topn)
    ranked = np.take_along_axis(allg, G.ranking(qB, rB, k), 1)
    assert grade.is_cuda and grade.dtype == torch.uint8
    np.testing.assert_array_equal(grade.cpu().numpy().astype(np.int64), ranked)
    for got, want in zip((ndcg, acg, wap), G.metrics(ranked, allg, topn)):
        assert got.dtype == torch.float64 and not got.is_cuda and got.shape == (len(topn),)
        np.testing.assert_allclose(got.numpy(), want, rtol=RTOL, atol=0)
    counts = grade_histogram(c[2], c[3])
    assert counts.is_cuda and counts.dtype == torch.int32
    np.testing.assert_array_equal(counts.cpu().numpy().astype(np.int64), G.histogram(allg, C))
    again = graded_metrics(*c, topn=topn, grade_counts=counts)
    assert all(torch.equal(a, b) for a, b in zip(again, (ndcg, acg, wap, grade)))
    idx, dist, g3 = graded_topk(c[0], c[1], k, c[2], c[3])
    assert torch.equal(g3, grade) and idx.dtype == torch.int32 and dist.dtype == torch.float32
    with pytest.raises(ValueError):
        graded_metrics(*c, topn=(0, 5))


def _state(seed=7):
    import recipe
    return {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, seed).items()}


def test_trainer_eval_graded_codeindex_and_cli(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set, then test() from its checkpoint without and with --eval-graded: the .mat of the second
    holds the six usual keys unchanged plus exactly the graded keys, whose values are graded_metrics' recomputed from the file's codes
    and labels; the log holds the graded(i2t) line with that value; CodeIndex.search(graded=True) and retrieve.py --graded (a fresh
    process) give the grades of graded_topk."""
    import argparse
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    from utils.retrieval import DEFAULT_TOPN, CodeIndex, graded_metrics, graded_topk, grade_histogram
    ck = tmp_path / "clip.pt"
    torch.save(_state(), ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    common = ["main.py", "-clip-path", str(ck), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
              "--max-words", "16", "--query-num", "24", "--train-num", "32", "--synthetic-size", "120", "--gemm-dtype", "f32"]
    monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / "run"), "--epochs", "1"])
    main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    model = tmp_path / "run" / "DSPH" / "synthetic" / "16" / "model-0.pth"
    assert model.exists()
    runs = {}
    for tag, extra in (("plain", []), ("graded", ["--eval-graded", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()      # (read now: later trainers' lines reach this file too)
        runs[tag] = (path, {k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, graded = runs["plain"][1], runs["graded"][1]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], graded[k])
    dirs = ("i2t", "t2i", "i2i", "t2t")
    assert set(graded) - set(plain) == {"graded_topn", "grade_counts"} | {f"{a}_{d}" for d in dirs for a in ("ndcg", "acg", "wap")}
    topn = tuple(n for n in DEFAULT_TOPN if n <= 96)
    np.testing.assert_array_equal(graded["graded_topn"].ravel(), topn)
    L = [torch.from_numpy(plain[k]).float() for k in ("q_l", "r_l")]
    np.testing.assert_array_equal(graded["grade_counts"], grade_histogram(*L).cpu().numpy())
    np.testing.assert_array_equal(graded["grade_counts"], G.histogram(G.grades(plain["q_l"], plain["r_l"]), plain["q_l"].shape[1]))
    sides = {"i2t": ("q_img", "r_txt"), "t2i": ("q_txt", "r_img"), "i2i": ("q_img", "r_img"), "t2t": ("q_txt", "r_txt")}
    for d, (qk, rk) in sides.items():
        ndcg, acg, wap, _ = graded_metrics(torch.from_numpy(plain[qk]).float(), torch.from_numpy(plain[rk]).float(), *L, topn=topn)
        for key, want in (("ndcg", ndcg), ("acg", acg), ("wap", wap)):
            np.testing.assert_array_equal(graded[f"{key}_{d}"].ravel(), want.numpy())
        if d == "i2t":
            shown = (ndcg, acg, wap)
    n = topn[-1]                                           # 96 database items: neither 100 nor 1000 fits, the line shows the largest cut-off
    log = runs["graded"][2]
    assert f"graded(i2t): NDCG@{n}: {float(shown[0][-1]):.6f}, ACG@{n}: {float(shown[1][-1]):.6f}, WAP@{n}: {float(shown[2][-1]):.6f}" in log
    assert all(f"graded({d}): NDCG@{n}: " in log for d in dirs) and "curves(" not in log
    assert "MAP(i->t)" in runs["plain"][2] and "graded(" not in runs["plain"][2]
    # the values in the file against the restatement
    allg = G.grades(plain["q_l"], plain["r_l"])
    ranked = np.take_along_axis(allg, G.ranking(plain["q_img"], plain["r_txt"], n), 1)
    for key, want in zip(("ndcg", "acg", "wap"), G.metrics(ranked, allg, topn)):
        np.testing.assert_allclose(graded[f"{key}_i2t"].ravel(), want, rtol=RTOL, atol=0)
    # CodeIndex on the file, and the CLI in a fresh process
    path = runs["graded"][0]
    c = [torch.from_numpy(plain[k]).float() for k in ("q_img", "r_txt", "q_l", "r_l")]
    index = CodeIndex.from_mat(str(path), side="r_txt")
    got = index.search(c[0], 10, c[2], graded=True)
    want = graded_topk(c[0], c[1], 10, c[2], c[3])
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want)) and got[2].dtype == torch.uint8
    assert torch.equal((want[2] > 0).to(torch.uint8), index.search(c[0], 10, c[2])[2])
    import cmh_native as N
    with pytest.raises(N.NativeError):
        index.search(c[0], 10, graded=True)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(path), "--direction", "i2t", "--k", "10",
                          "--queries", "3:9", "--graded"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 6
    idx, dist, grade = (t.cpu().numpy() for t in want)
    assert grade.max() > 1                                 # a count, not a flag
    for row, line in zip(range(3, 9), lines):
        head, *cols = line.split()
        assert int(head) == row and len(cols) == 10
        assert [int(cc.split(":")[0]) for cc in cols] == idx[row].tolist()
        assert [float(cc.split(":")[1]) for cc in cols] == dist[row].tolist()
        assert [int(cc.split(":")[2]) for cc in cols] == grade[row].tolist()
