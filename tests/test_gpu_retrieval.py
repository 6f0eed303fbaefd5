"""Top-k Hamming search and distance histograms by relevance on the GPU (cmh_hamming_topk / cmh_hamming_hist, utils/retrieval.py,
retrieve.py) against tests/golden/retrieval.npz (the reference's calc_hammingDist / calc_neighbor + torch.sort(stable=True)), against
the project's own stable ranking, and as properties at NUS-WIDE size.  Integers and half-integers: every comparison is exact unless
it says otherwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(g, name):
    return (g[f"{name}_qB"].astype(np.float32), g[f"{name}_rB"].astype(np.float32), g[f"{name}_qL"].astype(np.float32),
            g[f"{name}_rL"].astype(np.float32), int(g[f"{name}_k"]))


def _packed(qB, rB, qL=None, rL=None):
    import cmh_native as N
    return (N.pack_codes(_t(qB)), N.pack_codes(_t(rB)), None if qL is None else N.pack_labels(_t(qL)),
            None if rL is None else N.pack_labels(_t(rL)))


def _case_names():
    return [str(n) for n in np.load(os.path.join(os.path.dirname(__file__), "golden", "retrieval.npz"))["cases"]]


@pytest.mark.parametrize("name", _case_names())
def test_topk_and_histograms_match_the_reference_goldens(golden, name):
    import cmh_native as N
    g = golden("retrieval.npz")
    qB, rB, qL, rL, k = _case(g, name)
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    idx, dist, rel, counts = N.hamming_topk(qp, rp, rB.shape[1], k, ql, rl, want_counts=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), g[f"{name}_idx"])
    np.testing.assert_array_equal(dist.cpu().numpy(), g[f"{name}_dist"])
    np.testing.assert_array_equal(rel.cpu().numpy(), g[f"{name}_rel"])
    want = g[f"{name}_counts"].astype(np.int64)
    np.testing.assert_array_equal(counts.cpu().numpy().astype(np.int64), want)
    hist = N.hamming_hist(qp, rp, rB.shape[1], ql, rl).cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(hist, want)
    assert (hist.sum((1, 2)) == rB.shape[0]).all()
    # without labels: the same neighbours, no hit flags, every item in column 0
    idx2, dist2, rel2 = N.hamming_topk(qp, rp, rB.shape[1], k)
    assert rel2 is None and torch.equal(idx2, idx) and torch.equal(dist2, dist)
    plain = N.hamming_hist(qp, rp, rB.shape[1]).cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(plain[:, :, 0], want.sum(2))
    assert (plain[:, :, 1] == 0).all()


def _ap_at_k(rel_row, relevant, k):
    """The reference's AP (utils/calc_utils.py:32-36) in float64 from the hit flags of a ranking's first columns: the mean of
    r / position_r over the first total = min(k, relevant) relevant items.  The reference looks for them in the WHOLE ranking, also
    behind column k, so k columns decide the value only if they hold `total` hits: None otherwise."""
    total = min(k, int(relevant))
    pos = np.nonzero(rel_row)[0][:total].astype(np.float64) + 1.0
    if len(pos) < total:
        return None
    return float(np.mean(np.arange(1, total + 1, dtype=np.float64) / pos)) if total else 0.0


@pytest.mark.parametrize("Q,N,K,C,k,zeros", [(5, 7, 16, 4, 7, False), (9, 200, 64, 8, 50, False), (6, 1000, 128, 12, 1000, True),
                                              (4, 4097, 512, 24, 1000, False), (3, 5000, 2048, 24, 5000, True),
                                              (3, 30000, 64, 24, 5000, False)])
def test_topk_is_the_prefix_of_the_stable_ranking(Q, N, K, C, k, zeros):
    """Against cmh_hamming_map(tie_order=CMH_TIE_STABLE) for the queries it ranks, and its per-query AP (topk=k) recomputed from the
    hit flags within 2e-6 (the per-query AP bound of tests/test_gpu_map.py): from the k columns wherever they decide it (see
    _ap_at_k), and for every ranked query from the hit flags of a search with k = N; dist against calc_hammingDist gathered at idx,
    bit for bit."""
    import cmh_native as Nn
    rng = np.random.default_rng(Q * 1000 + N + K)
    vals = np.array([-1.0, 1.0, 0.0] if zeros else [-1.0, 1.0], np.float32)
    qB = vals[rng.integers(0, len(vals), (Q, K))]
    rB = vals[rng.integers(0, len(vals), (N, K))]
    qL = (rng.random((Q, C)) < 0.2).astype(np.float32)
    rL = (rng.random((N, C)) < 0.2).astype(np.float32)
    qL[0] = 0                                             # no relevant item: the ranking kernel skips it, the search answers it
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    idx, dist, rel, counts = Nn.hamming_topk(qp, rp, K, k, ql, rl, want_counts=True)
    _, ap, perm = Nn.hamming_map(qp, ql, rp, rl, K, C, topk=k, tie_order=Nn.TIE_STABLE, want_perm=True)
    relevant = counts[:, :, 1].sum(1).cpu().numpy()
    np.testing.assert_array_equal(relevant, (qL @ rL.T > 0).sum(1))
    ranked = torch.from_numpy(relevant > 0).to(DEV)
    assert not bool(ranked[0]) and bool(ranked.any()) and bool((perm[~ranked] == -1).all())
    assert torch.equal(idx[ranked], perm[ranked][:, :k])
    full = Nn.hamming_dist(qp, rp, K)
    assert torch.equal(dist, full.gather(1, idx.long()))
    for i in np.nonzero(relevant == 0)[0]:
        np.testing.assert_array_equal(idx[i].cpu().numpy(), np.argsort(oracle.hamming_row(qB[i], rB), kind="stable")[:k])
        assert int(rel[i].sum()) == 0
    rel_np, ap_np = rel.cpu().numpy(), ap.cpu().numpy()
    idx_all, _, rel_all = Nn.hamming_topk(qp, rp, K, N, ql, rl)
    assert torch.equal(idx_all[ranked], perm[ranked]) and torch.equal(idx_all[:, :k], idx) and torch.equal(rel_all[:, :k], rel)
    rel_all = rel_all.cpu().numpy()
    decided = 0
    for i in np.nonzero(relevant > 0)[0]:
        assert abs(_ap_at_k(rel_all[i], relevant[i], k) - float(ap_np[i])) < 2e-6, (i, relevant[i])
        mine = _ap_at_k(rel_np[i], relevant[i], k)
        if mine is not None:
            decided += 1
            assert abs(mine - float(ap_np[i])) < 2e-6, (i, relevant[i])
    assert decided > 0 or k < N
    sim = (qL @ rL.T > 0)
    np.testing.assert_array_equal(rel_np, np.take_along_axis(sim, idx.cpu().numpy().astype(np.int64), 1).astype(np.uint8))


def test_entry_points_match_calc_utils_distances(golden):
    """utils.retrieval.hamming_topk with CPU inputs (as calc_utils takes them): dist == calc_hammingDist(qB, rB).gather(1, idx)."""
    from utils.calc_utils import calc_hammingDist
    from utils.retrieval import hamming_topk
    g = golden("retrieval.npz")
    qB, rB, qL, rL, k = _case(g, "b128_zeros_c40")
    idx, dist, rel = hamming_topk(torch.from_numpy(qB), torch.from_numpy(rB), k, torch.from_numpy(qL), torch.from_numpy(rL))
    assert idx.is_cuda and idx.dtype == torch.int32 and rel.dtype == torch.uint8
    assert torch.equal(dist, calc_hammingDist(torch.from_numpy(qB), torch.from_numpy(rB)).gather(1, idx.long()))
    assert bool((dist % 1 == 0.5).any())
    two = hamming_topk(torch.from_numpy(qB), torch.from_numpy(rB), k)
    assert len(two) == 2 and torch.equal(two[0], idx)
    np.testing.assert_array_equal(rel.cpu().numpy(), g["b128_zeros_c40_rel"])


def test_properties_at_nuswide_size():
    """Q = 5000, N = 190 834, 128 bit, 21 classes, k = 1000: rows sorted by (dist, idx); the last distance is the radius where the
    query's cumulative counts first reach k; below that radius every item is returned; 8 rows equal the stable ranking's prefix."""
    import cmh_native as Nn
    rng = np.random.default_rng(11)
    Q, N, K, C, k = 5000, 190834, 128, 21, 1000
    rL = (rng.random((N, C)) < 0.15).astype(np.float32)
    qL = (rng.random((Q, C)) < 0.15).astype(np.float32)
    rB = np.where(rng.random((N, K)) < 0.5, -1.0, 1.0).astype(np.float32)
    qB = np.where(rng.random((Q, K)) < 0.5, -1.0, 1.0).astype(np.float32)
    qL[qL.sum(1) == 0, 0] = 1
    rL[:8, 0] = 1
    qL[:8, 0] = 1
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    idx, dist, rel, counts = Nn.hamming_topk(qp, rp, K, k, ql, rl, want_counts=True)
    assert torch.equal(counts, Nn.hamming_hist(qp, rp, K, ql, rl))
    tot = counts.long().sum(2)
    assert bool((tot.sum(1) == N).all())
    h = (dist * 2).long()
    assert torch.equal(h.float() * 0.5, dist)
    key = h * (1 << 19) + idx.long()
    assert bool((key[:, 1:] > key[:, :-1]).all())          # sorted by (dist, idx), no item twice
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    cum = tot.cumsum(1)
    hstar = (cum < k).sum(1)                               # the first radius where the cumulative count reaches k
    assert torch.equal(h[:, -1], hstar)
    got = torch.zeros_like(tot).scatter_add_(1, h, torch.ones_like(h))
    bins = torch.arange(tot.shape[1], device=DEV)[None, :]
    below = bins < hstar[:, None]
    assert torch.equal(got[below], tot[below])
    at = got.gather(1, hstar[:, None])[:, 0]
    assert torch.equal(at, k - (cum.gather(1, hstar[:, None])[:, 0] - tot.gather(1, hstar[:, None])[:, 0]))
    assert int(got[bins > hstar[:, None]].sum()) == 0
    relr = torch.zeros_like(tot).scatter_add_(1, h, rel.long())
    assert torch.equal(relr[below], counts[:, :, 1].long()[below])
    # 8 rows against the stable ranking
    sub = ((qp[0][:8].contiguous(), qp[1][:8].contiguous()), ql[:8].contiguous())
    _, _, perm = Nn.hamming_map(sub[0], sub[1], rp, rl, K, C, tie_order=Nn.TIE_STABLE, want_perm=True)
    assert torch.equal(idx[:8], perm[:, :k])


def _curves_f64(counts, rel, relevant, topn):
    """A float64 restatement of the conventions: queries without relevant items left out, empty ball -> 0."""
    keep = [i for i in range(counts.shape[0]) if relevant[i] > 0]
    H = counts.shape[1]
    P, R = np.zeros((len(keep), H)), np.zeros((len(keep), H))
    TP, TR = np.zeros((len(keep), len(topn))), np.zeros((len(keep), len(topn)))
    for a, i in enumerate(keep):
        hits = ball = 0
        for h in range(H):
            hits += int(counts[i, h, 1])
            ball += int(counts[i, h, 0]) + int(counts[i, h, 1])
            P[a, h] = hits / ball if ball else 0.0
            R[a, h] = hits / int(relevant[i])
        for b, n in enumerate(topn):
            s = int(rel[i, :n].sum())
            TP[a, b] = s / n
            TR[a, b] = s / int(relevant[i])
    return P.mean(0), R.mean(0), TP.mean(0), TR.mean(0)


@pytest.mark.parametrize("name,topn", [("b64_4097", (1, 50, 100)), ("b128_zeros_c40", (1, 10, 77)), ("b16_1000", (1, 25, 50))])
def test_curves_match_a_float64_restatement_of_the_golden_counts(golden, name, topn):
    from utils.retrieval import pr_curve, topn_precision
    g = golden("retrieval.npz")
    qB, rB, qL, rL, k = _case(g, name)
    c = [torch.from_numpy(a) for a in (qB, rB, qL, rL)]
    p, r, counts = pr_curve(*c)
    tp, tr, rel = topn_precision(*c, topn=topn)
    np.testing.assert_array_equal(counts.cpu().numpy().astype(np.int64), g[f"{name}_counts"].astype(np.int64))
    np.testing.assert_array_equal(rel.cpu().numpy(), g[f"{name}_rel"][:, :max(topn)])
    gc = g[f"{name}_counts"].astype(np.int64)
    P, R, TP, TR = _curves_f64(gc, g[f"{name}_rel"], gc[:, :, 1].sum(1), topn)
    for got, want in ((p, P), (r, R), (tp, TP), (tr, TR)):
        assert got.dtype == torch.float64
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-6)
    assert gc[1, :, 1].sum() == 0                           # query 1 has no relevant item and is left out of the means


def test_two_calls_agree_also_on_another_stream(golden):
    import cmh_native as N
    g = golden("retrieval.npz")
    qB, rB, qL, rL, k = _case(g, "b64_4097")
    qp, rp, ql, rl = _packed(qB, rB, qL, rL)
    a = N.hamming_topk(qp, rp, 64, k, ql, rl, want_counts=True)
    b = N.hamming_topk(qp, rp, 64, k, ql, rl, want_counts=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = N.hamming_topk(qp, rp, 64, k, ql, rl, want_counts=True)
        d = N.hamming_hist(qp, rp, 64, ql, rl)
    s.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(d, a[3])


def _state(seed=7):
    import recipe
    return {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, seed).items()}


def test_trainer_eval_curves_codeindex_and_cli(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set, then test() from its checkpoint: without --eval-curves the .mat holds exactly the six
    keys it always held, with it the curve arrays as well; CodeIndex.from_mat reads that file back and searches like hamming_topk;
    retrieve.py (a fresh process) prints the same neighbours."""
    import argparse
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    from utils.retrieval import DEFAULT_TOPN, CodeIndex, hamming_topk, pr_curve, topn_precision
    ck = tmp_path / "clip.pt"
    torch.save(_state(), ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    common = ["main.py", "-clip-path", str(ck), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
              "--max-words", "16", "--query-num", "24", "--train-num", "32", "--synthetic-size", "120", "--gemm-dtype", "f32"]
    monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / "run"), "--epochs", "1"])
    main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    model = tmp_path / "run" / "DSPH" / "synthetic" / "16" / "model-0.pth"
    assert model.exists()
    keys = {}
    for tag, extra in (("plain", []), ("curves", ["--eval-curves", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()      # (read now: later trainers' lines reach this file too)
        keys[tag] = (path, {k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, curves = keys["plain"][1], keys["curves"][1]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], curves[k])
    new = set(curves) - set(plain)
    assert new == {"curve_topn"} | {f"{a}_{d}" for d in ("i2t", "t2i", "i2i", "t2t")
                                    for a in ("pr_precision", "pr_recall", "pr_counts", "topn_precision", "topn_recall")}
    topn = tuple(n for n in DEFAULT_TOPN if n <= 96)
    np.testing.assert_array_equal(curves["curve_topn"].ravel(), topn)
    c = [torch.from_numpy(plain[k]).float() for k in ("q_img", "r_txt", "q_l", "r_l")]
    p, r, counts = pr_curve(*c)
    tp, _, _ = topn_precision(*c, topn=topn)
    np.testing.assert_array_equal(curves["pr_precision_i2t"].ravel(), p.numpy())
    np.testing.assert_array_equal(curves["pr_recall_i2t"].ravel(), r.numpy())
    np.testing.assert_array_equal(curves["pr_counts_i2t"], counts.cpu().numpy())
    np.testing.assert_array_equal(curves["topn_precision_i2t"].ravel(), tp.numpy())
    assert "curves(i2t): P@H<=2:" in keys["curves"][2] and "curves(t2t): P@H<=2:" in keys["curves"][2]
    assert "MAP(i->t)" in keys["plain"][2] and "curves(" not in keys["plain"][2]
    want_p = float(p[4])
    assert f"curves(i2t): P@H<=2: {want_p:.6f}" in keys["curves"][2]
    # CodeIndex on the file, and the CLI in a fresh process
    path = keys["plain"][0]
    index = CodeIndex.from_mat(str(path), side="r_txt")
    assert index.size == 96 and index.bits == 16
    got = index.search(c[0], 10, c[2])
    want = hamming_topk(c[0], c[1], 10, c[2], c[3])
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(index.search(c[0], 10)[0], want[0])
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(path), "--direction", "i2t", "--k", "10",
                          "--queries", "3:9"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 6
    idx, dist, rel = (t.cpu().numpy() for t in want)
    for row, line in zip(range(3, 9), lines):
        head, *cols = line.split()
        assert int(head) == row and len(cols) == 10
        assert [int(cc.split(":")[0]) for cc in cols] == idx[row].tolist()
        assert [float(cc.split(":")[1]) for cc in cols] == dist[row].tolist()
        assert [int(cc.split(":")[2]) for cc in cols] == rel[row].tolist()
