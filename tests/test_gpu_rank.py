"""The ranks of given targets on the GPU (cmh_hamming_rank, utils/retrieval.py::target_counts / recall_at_k, CodeIndex.rank_of /
recall, retrieve.py --recall, the trainers' --eval-recall) against the NumPy restatement of tests/rankutil.py (half-distances as
K - q.r, the three counts as sums over a row) and against the code there was: the target's column in hamming_topk(k = N) and the
bins of hamming_hist.  Every count is compared exactly; the float64 metrics within relative 1e-12 (both sides are means of at most a
few hundred terms in different orders: n * eps ~ 1e-14)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rankutil as U
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12
KS = (1, 5, 10)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _native(qB, rB, t=None, bound=None, ht_rows=None):
    """ONE cmh_hamming_rank: targets t [Q, G] (rows of rB, -1 = padding; the bound is the target's row unless given)."""
    import cmh_native as N
    qp, rp = N.pack_codes(_t(qB)), N.pack_codes(_t(rB))
    rows = _t(np.maximum(t if ht_rows is None else ht_rows, 0).reshape(-1))
    tp = tuple(x.index_select(0, rows) for x in rp)
    b = _t((t if bound is None else bound).astype(np.int32))
    out = N.hamming_rank(qp, rp, rB.shape[1], tp, b)
    assert out.dtype == torch.int32 and tuple(out.shape) == b.shape + (3,) and out.is_contiguous()
    return out.cpu().numpy().astype(np.int64)


# (Q, N, bits, zeros, G): Q around the 64-query tile; N = 1, 2, around a tile, 257 (two chunks, walk tails of 4 and 13 items at 16
# bit), 7 and 19 (no group at all / one group of 16 and a tail of 3), 65 533 (a second chunk under the search's plan); every register
# form (1..4 words, 33 bit = a cut last word), the staged form (160 bit) and the longest code; G = 1 (its own form), 5 and 8.
CASES = [(1, 1, 16, False, 1), (63, 2, 32, True, 5), (64, 63, 33, True, 8), (65, 64, 64, False, 1), (130, 65, 96, True, 5),
         (64, 257, 128, False, 8), (65, 257, 160, True, 1), (63, 65, 2048, True, 5), (130, 65533, 64, False, 8), (1, 65533, 16, True, 1),
         (5, 19, 16, True, 5), (3, 7, 64, False, 8), (130, 257, 16, True, 1), (65, 65, 160, False, 8), (2, 257, 33, False, 5)]


@pytest.mark.parametrize("Q,n,bits,zeros,G", CASES)
def test_counts_equal_the_restatement(Q, n, bits, zeros, G):
    qB, rB = U.codes(Q, n, bits, zeros, 1000 + Q + n + bits)
    h = U.half_units(qB, rB)
    t = U.targets(Q, n, G, 3)
    assert (t == 0).any() and (Q == 1 or (t == n - 1).any()) and (G == 1 or all((t[:, g] < 0).any() or Q < G for g in range(G)))
    want = U.counts(h, t)
    got = _native(qB, rB, t)
    np.testing.assert_array_equal(got, want)
    assert (got[t < 0] == 0).all() and (got[t >= 0][:, 2] >= 1).all()
    if zeros and n > 2 and Q >= 5:
        assert (np.take_along_axis(h, np.maximum(t, 0), 1)[t >= 0] % 2).any()          # odd half-distances among the targets


def test_bounds_passed_directly():
    """bound = 0 (nothing before), bound = N (every tie before), any value between, -1: the bound is a count, not the target."""
    Q, n, bits, G = 65, 300, 16, 8
    qB, rB = U.codes(Q, n, bits, True, 8)
    h = U.half_units(qB, rB)
    rows = np.random.default_rng(4).integers(0, n, (Q, G))
    ht = np.take_along_axis(h, rows, 1)
    for bound in (np.zeros((Q, G), np.int64), np.full((Q, G), n, np.int64), np.random.default_rng(5).integers(-1, n + 1, (Q, G))):
        got = _native(qB, rB, bound=bound, ht_rows=rows)
        np.testing.assert_array_equal(got, U.counts_bound(h, ht, bound))
    assert (got[bound < 0] == 0).all()
    zero, full = _native(qB, rB, bound=np.zeros((Q, G), np.int64), ht_rows=rows), _native(qB, rB, bound=np.full((Q, G), n), ht_rows=rows)
    assert (zero[..., 1] == 0).all() and (full[..., 1] == full[..., 2]).all() and (full[..., 2] > 1).any()


def test_duplicated_codes_tie_in_the_hundreds():
    qB, rB = U.duplicated(65, 3000, 16, 6, 21)
    t = U.targets(65, 3000, 5, 9)
    got = _native(qB, rB, t)
    np.testing.assert_array_equal(got, U.counts(U.half_units(qB, rB), t))
    assert got[t >= 0][:, 2].min() > 100 and (got[..., 1] > 100).any()


@pytest.mark.parametrize("Q,n,bits,zeros", [(130, 5000, 64, False), (65, 1031, 160, True), (9, 300, 16, True)])
def test_counts_agree_with_topk_and_hist(Q, n, bits, zeros):
    """The code that exists: less + ties_before is the target's column in hamming_topk(k = N); less and ties are a prefix sum and an
    entry of hamming_hist's bins."""
    import cmh_native as N
    qB, rB = U.codes(Q, n, bits, zeros, 77)
    t = U.targets(Q, n, 8, 13)
    got = _native(qB, rB, t)
    qp, rp = N.pack_codes(_t(qB)), N.pack_codes(_t(rB))
    idx, dist, _, counts = N.hamming_topk(qp, rp, bits, n, want_counts=True)
    col = torch.empty_like(idx)
    col.scatter_(1, idx.long(), torch.arange(n, dtype=torch.int32, device=DEV)[None, :].expand(Q, n))      # col[q, j] = column of item j
    tt = _t(np.maximum(t, 0))
    valid = t >= 0
    np.testing.assert_array_equal((got[..., 0] + got[..., 1])[valid], col.gather(1, tt).cpu().numpy()[valid])
    bins = counts.long().sum(2)                                                     # [Q, 2K+1]
    below = torch.cat([torch.zeros(Q, 1, dtype=torch.int64, device=DEV), bins.cumsum(1)], 1)
    ht = (2 * dist.gather(1, col.gather(1, tt).long())).long()                      # the target's half-distance, from the search's own list
    np.testing.assert_array_equal(got[..., 0][valid], below.gather(1, ht).cpu().numpy()[valid])
    np.testing.assert_array_equal(got[..., 2][valid], bins.gather(1, ht).cpu().numpy()[valid])


@pytest.mark.parametrize("step", [1, 64, 100])
def test_shards_add_up(step):
    from utils.retrieval import target_counts
    qB, rB = U.codes(9, 257, 16, True, 31)
    t = U.targets(9, 257, 5, 17)
    t[2, 3], t[3, 1], t[4, 2] = step - 1, step, 256 - 256 % step                    # last of a shard, first of the next, first of the last
    whole = target_counts(_t(qB), _t(rB), _t(t))
    assert whole.dtype == torch.int64 and whole.is_cuda and tuple(whole.shape) == (9, 5, 3)
    np.testing.assert_array_equal(whole.cpu().numpy(), U.counts(U.half_units(qB, rB), t))
    assert torch.equal(target_counts(_t(qB), _t(rB), _t(t), shard_items=step), whole)


def test_more_queries_than_one_call_takes():
    from utils.retrieval import target_counts
    import cmh_native as N
    Q = N.QUERIES_MAX + 65
    qB, rB = U.codes(Q, 5, 16, False, 41)
    t = np.random.default_rng(2).integers(0, 5, Q)
    got = target_counts(_t(qB), _t(rB), _t(t)).cpu().numpy()
    h = U.half_units(qB, rB)
    ht = h[np.arange(Q), t][:, None]
    before = (h == ht) & (np.arange(5)[None, :] < t[:, None])
    np.testing.assert_array_equal(got[:, 0], np.stack([(h < ht).sum(1), before.sum(1), (h == ht).sum(1)], 1))


def test_more_targets_than_one_call_takes(monkeypatch):
    import cmh_native as N
    from utils.retrieval import target_counts
    qB, rB = U.codes(65, 300, 33, True, 43)
    t = U.targets(65, 300, 11, 19)
    calls = []
    real = N.hamming_rank
    monkeypatch.setattr(N, "hamming_rank", lambda *a: calls.append(tuple(a[4].shape)) or real(*a))
    got = target_counts(_t(qB), _t(rB), _t(t))
    np.testing.assert_array_equal(got.cpu().numpy(), U.counts(U.half_units(qB, rB), t))
    assert calls == [(65, 8), (65, 3)]
    calls.clear()
    target_counts(_t(qB), _t(rB), _t(t[:, :8]))
    target_counts(_t(qB), _t(rB), _t(t[:, 0]))
    assert calls == [(65, 8), (65, 1)]                                              # within the limits: exactly one native call each


def test_two_calls_and_two_streams_give_equal_bytes():
    from utils.retrieval import target_counts
    qB, rB = U.codes(130, 70001, 64, True, 51)
    t = U.targets(130, 70001, 8, 23)
    ops = (_t(qB), _t(rB), _t(t))
    a = target_counts(*ops)
    b = target_counts(*ops)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = target_counts(*ops)
        d = target_counts(*ops, shard_items=30000)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert bytes(a.cpu().numpy().tobytes()) == bytes(c.cpu().numpy().tobytes())
    np.testing.assert_array_equal(a.cpu().numpy(), U.counts(U.half_units(qB, rB), t))


def _close(got, want, ties):
    np.testing.assert_allclose(got["recall"].numpy(), want["recall"], rtol=RTOL, atol=0)
    np.testing.assert_allclose([got["median_rank"], got["mean_rank"]], [want["median_rank"], want["mean_rank"]], rtol=RTOL, atol=0)
    np.testing.assert_array_equal(got["best_rank"].numpy(), want["best_rank"])
    if ties == "expected":
        assert "mrr" not in got
    else:
        np.testing.assert_allclose(got["mrr"], want["mrr"], rtol=RTOL, atol=0)


def test_recall_at_k_and_codeindex_recall(tmp_path):
    """Identity pairing and five captions per image with padding, under the four conventions; an index grown by add() and one
    reloaded by load() give the counts of the whole one."""
    import cmh_native as N
    from utils.retrieval import CodeIndex, recall_at_k
    rB = U.duplicated(1, 400, 16, 40, 61)[1]
    qB = rB[:70].copy()                                                             # item q is a copy of query q, and so are some 10 others
    h = U.half_units(qB, rB)
    five = U.targets(70, 400, 5, 29)
    whole = CodeIndex(_t(rB))
    grown = CodeIndex(_t(rB[:150]), shard_items=128).add(_t(rB[150:]))
    grown.save(tmp_path / "grown.npz")
    loaded = CodeIndex.load(tmp_path / "grown.npz", shard_items=333)
    for t, given in ((np.arange(70), None), (five, five)):
        c = U.counts(h, t)
        arg = None if given is None else _t(given)
        for index in (whole, grown, loaded):
            np.testing.assert_array_equal(index.rank_of(_t(qB), _t(t)).cpu().numpy(), c)
        seen = set()
        for ties in U.TIES:
            want = U.metrics(c, KS, ties)
            got = recall_at_k(_t(qB), _t(rB), arg, KS, ties)
            _close(got, want, ties)
            np.testing.assert_array_equal(got["counts"].cpu().numpy(), c)
            _close(grown.recall(_t(qB), arg, KS, ties), want, ties)
            _close(recall_at_k(_t(qB), _t(rB), arg, KS, ties, shard_items=77), want, ties)
            seen.add(tuple(want["recall"]))
        assert len(seen) == (4 if given is None else len(seen))                     # identity: four conventions, four answers
    with pytest.raises(N.NativeError):
        whole.rank_of(_t(qB), _t(np.full(70, 400)))
    with pytest.raises(N.NativeError):
        whole.rank_of(_t(qB[:, :8]), _t(np.arange(70)))
    with pytest.raises(N.NativeError):
        CodeIndex(_t(rB[:10])).recall(_t(qB))                                       # identity pairing with fewer items than queries


def test_retrieve_recall_cli(tmp_path):
    """retrieve.py --recall in fresh processes: the paired query sides of a .mat (identity, sliced by --queries), and a saved index
    with --targets."""
    import scipy.io as scio
    from utils.retrieval import CodeIndex
    img, txt = U.duplicated(40, 40, 16, 12, 71)
    _, rB = U.duplicated(1, 300, 16, 12, 71)
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": img, "q_txt": txt, "r_img": rB, "r_txt": rB[::-1].copy()})
    CodeIndex(_t(rB)).save(tmp_path / "db.npz")
    t = U.targets(40, 300, 3, 5)
    (tmp_path / "targets.txt").write_text("".join(" ".join(str(x) for x in row if x >= 0) + "\n" for row in t))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(mat), "--recall"]

    def line(want, ks, ties):
        cols = [f"R@{k}: {v:.6f}" for k, v in zip(ks, want["recall"])] + [f"MedR: {want['median_rank']:g}", f"MeanR: {want['mean_rank']:.6f}"]
        return " ".join(cols + ([] if ties == "expected" else [f"MRR: {want['mrr']:.6f}"]))

    runs = [(["--direction", "t2i", "--queries", "3:33"], U.counts(U.half_units(txt, img), np.arange(40))[3:33], KS, "index"),
            (["--index", str(tmp_path / "db.npz"), "--targets", str(tmp_path / "targets.txt"), "--ks", "1,20", "--ties", "expected"],
             U.counts(U.half_units(img, rB), t), (1, 20), "expected")]
    for extra, c, ks, ties in runs:
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines() == [line(U.metrics(c, ks, ties), ks, ties)]


def _state(seed=7):
    import recipe
    return {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, seed).items()}


def test_trainer_eval_recall(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set (the configuration of the other end-to-end tests), then test() from its checkpoint
    without and with --eval-recall: the second .mat holds the six usual keys unchanged plus the recall keys, whose counts are
    target_counts' on the stored codes and the restatement's; the log holds the recall lines."""
    import argparse
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    from utils.retrieval import recall_from_counts, target_counts
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
    for tag, extra in (("plain", []), ("recall", ["--eval-recall", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()
        runs[tag] = ({k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, rec = runs["plain"][0], runs["recall"][0]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], rec[k])
    new = set(rec) - set(plain)
    assert {"recall_ks", "recall_counts_i2t", "recall_counts_t2i"} <= new and all(k.startswith("recall_") for k in new)
    np.testing.assert_array_equal(rec["recall_ks"].ravel(), KS)
    log = runs["recall"][1]
    for name, (qk, rk) in {"i2t": ("q_img", "q_txt"), "t2i": ("q_txt", "q_img")}.items():
        counts = target_counts(torch.from_numpy(plain[qk]).float(), torch.from_numpy(plain[rk]).float(), torch.arange(24))
        assert rec[f"recall_counts_{name}"].shape == (24, 1, 3)
        np.testing.assert_array_equal(rec[f"recall_counts_{name}"], counts.cpu().numpy())
        np.testing.assert_array_equal(rec[f"recall_counts_{name}"], U.counts(U.half_units(plain[qk], plain[rk]), np.arange(24)))
        shown = []
        for ties in ("index", "expected"):
            want = U.metrics(rec[f"recall_counts_{name}"].astype(np.int64), KS, ties)
            np.testing.assert_allclose(rec[f"recall_{ties}_{name}"].ravel(), want["recall"], rtol=RTOL, atol=0)
            np.testing.assert_allclose(rec[f"recall_medr_{ties}_{name}"].ravel()[0], want["median_rank"], rtol=RTOL, atol=0)
            m = recall_from_counts(counts, KS, ties)
            shown.append(f"{ties}: " + ", ".join([f"R@{k}: {float(v):.6f}" for k, v in zip(KS, m["recall"])] + [f"MedR: {m['median_rank']:g}"]))
        assert f"recall({name}): " + "; ".join(shown) in log
    assert "MAP(i->t)" in runs["plain"][1] and "recall(" not in runs["plain"][1]
