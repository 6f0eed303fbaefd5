"""Retrieval past the entry points' limits (N <= 524 287, Q <= 65 535): cmh_topk_merge against NumPy's stable argsort, the sharded
search / histograms of utils/retrieval.py against the unsharded ones bit for bit, a database one shard cannot hold against NumPy,
query blocks, CodeIndex.add / save / load and retrieve.py --index.  Integers and half-integers: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the merge kernel ----------------------------------------------------------------------------------------------------------
# Rows of min(ka, k) + min(kb, k) entries.  Up to 256: four rows per workgroup; up to 16 384: one row staged in LDS, above 48 KiB
# (12 288 entries) with the raised LDS limit; longer: searched in global memory in slices of 4096 entries, the last one ragged.
MERGE_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (3, 5, 9, 7), (3, 9, 5, 14), (65, 64, 65, 100), (2, 257, 1, 257), (5, 300, 1000, 1000),
                (4, 1000, 300, 50), (2, 5000, 5000, 10000),       # 10 000 entries: 40 000 B of LDS, still staged
                (2, 7000, 7000, 14000),                           # 14 000 entries: 56 000 B of LDS, staged above the 48 KiB default
                (2, 9000, 9000, 18000), (2, 9000, 8500, 9001)]    # 18 000 and 17 500 entries: global memory, five slices each
PATTERNS = ["random33", "equal", "b_below_a", "interleaved"]


def _half_units(pattern, rng, Q, ka, kb):
    if pattern == "random33":                                     # 16-bit codes: 33 values, heavy ties
        return rng.integers(0, 33, (Q, ka)), rng.integers(0, 33, (Q, kb))
    if pattern == "equal":                                        # the output is a, then b
        return np.full((Q, ka), 7), np.full((Q, kb), 7)
    if pattern == "b_below_a":                                    # every b strictly below every a
        return rng.integers(20, 30, (Q, ka)), rng.integers(0, 10, (Q, kb))
    ha = 2 * np.arange(ka)[None, :] + np.zeros((Q, 1), np.int64)  # strictly interleaved: no two entries at one distance
    hb = 2 * np.arange(kb)[None, :] + 1 + np.zeros((Q, 1), np.int64)
    return ha, hb


def _sorted_list(rng, h, universe):
    """Rows of distinct indices below `universe`, ordered by (h, idx) as hamming_topk orders them; a random tag per entry."""
    Q, k = h.shape
    idx = np.stack([rng.permutation(universe)[:k] for _ in range(Q)])
    order = np.lexsort((idx, h), axis=1)
    h, idx = np.take_along_axis(h, order, 1), np.take_along_axis(idx, order, 1)
    return idx.astype(np.int32), (0.5 * h).astype(np.float32), rng.integers(0, 256, (Q, k)).astype(np.uint8)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Q,ka,kb,k", MERGE_SHAPES)
def test_topk_merge_is_the_stable_argsort_of_the_union(Q, ka, kb, k, pattern):
    import cmh_native as N
    rng = np.random.default_rng(Q * 7919 + ka * 31 + kb + PATTERNS.index(pattern))
    ha, hb = _half_units(pattern, rng, Q, ka, kb)
    b_base = ka + 11
    a_idx, a_dist, a_tag = _sorted_list(rng, ha, b_base)          # every index of a below b_base <= every index of b
    b_idx, b_dist, b_tag = _sorted_list(rng, hb, kb + 5)
    dist = np.concatenate([a_dist, b_dist], 1)
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    want = [np.take_along_axis(x, order, 1) for x in (np.concatenate([a_idx, b_idx + b_base], 1), dist, np.concatenate([a_tag, b_tag], 1))]
    a, b = tuple(_t(x) for x in (a_idx, a_dist, a_tag)), tuple(_t(x) for x in (b_idx, b_dist, b_tag))
    got = N.topk_merge(a, b, b_base, k)
    again = N.topk_merge(a, b, b_base, k)
    plain = N.topk_merge(a[:2] + (None,), b[:2] + (None,), b_base, k)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.uint8 and plain[2] is None
    for j in range(3):
        np.testing.assert_array_equal(got[j].cpu().numpy(), want[j])
        assert torch.equal(got[j], again[j])
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    if pattern == "equal":
        np.testing.assert_array_equal(got[0].cpu().numpy(), np.concatenate([a_idx, b_idx + b_base], 1)[:, :k])
    # into buffers the caller owns (the fold over shards writes two of them in turn)
    out = (torch.full((Q, k), -7, dtype=torch.int32, device=DEV), torch.full((Q, k), -7.0, device=DEV),
           torch.full((Q, k), 9, dtype=torch.uint8, device=DEV))
    ret = N.topk_merge(a, b, b_base, k, out=out)
    assert all(r.data_ptr() == o.data_ptr() and torch.equal(o, g) for r, o, g in zip(ret, out, got))
    pool = torch.zeros(Q * (ka + k), dtype=torch.int32, device=DEV)     # an out that begins on the last element of an input
    with pytest.raises(N.NativeError):
        N.topk_merge((pool[:Q * ka].view(Q, ka),) + a[1:], b, b_base, k, out=(pool[Q * ka - 1:Q * ka - 1 + Q * k].view(Q, k),) + out[1:])
    with pytest.raises(N.NativeError):
        N.topk_merge(a, b, b_base, ka + kb + 1)
    with pytest.raises(N.NativeError):
        N.topk_merge(a, b[:2] + (None,), b_base, k)


# ---- 2. sharded = whole -----------------------------------------------------------------------------------------------------------
def _database(Q, n, K, C, zeros, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([-1.0, 1.0, 0.0] if zeros else [-1.0, 1.0], np.float32)
    qB, rB = vals[rng.integers(0, len(vals), (Q, K))], vals[rng.integers(0, len(vals), (n, K))]
    qL, rL = (rng.random((Q, C)) < 0.25).astype(np.float32), (rng.random((n, C)) < 0.25).astype(np.float32)
    qL[1] = 0                                                     # a query without any relevant item
    return tuple(torch.from_numpy(x) for x in (qB, rB, qL, rL))


_WHOLE = {}


def _whole(key, c, ks):
    """The unsharded results (shard_items=None: one native call each), computed once per database and shared."""
    if key not in _WHOLE:
        import utils.retrieval as R
        w = {"counts": R.pr_curve(*c)[2], "ghist": R.grade_histogram(c[2], c[3])}
        for k in ks:
            topn = sorted({1, k})
            w[k] = {"topk": R.hamming_topk(*c[:2], k, *c[2:]), "plain": R.hamming_topk(*c[:2], k), "graded": R.graded_topk(*c[:2], k, *c[2:]),
                    "topn": R.topn_precision(*c, topn=topn), "metrics": R.graded_metrics(*c, topn=topn)}
        _WHOLE[key] = w
    return _WHOLE[key]


def _assert_sharded_equals_whole(key, c, ks, s):
    import utils.retrieval as R
    w = _whole(key, c, ks)
    assert torch.equal(R.pr_curve(*c, shard_items=s)[2], w["counts"])
    assert torch.equal(R.grade_histogram(c[2], c[3], shard_items=s), w["ghist"])
    assert w["counts"].dtype == torch.int32 and bool((w["counts"].long().sum((1, 2)) == c[1].shape[0]).all())
    for k in ks:
        topn = sorted({1, k})
        got = {"topk": R.hamming_topk(*c[:2], k, *c[2:], shard_items=s), "plain": R.hamming_topk(*c[:2], k, shard_items=s),
               "graded": R.graded_topk(*c[:2], k, *c[2:], shard_items=s), "topn": R.topn_precision(*c, topn=topn, shard_items=s),
               "metrics": R.graded_metrics(*c, topn=topn, shard_items=s)}
        assert len(got["topk"]) == 3 and len(got["plain"]) == 2 and len(got["graded"]) == 3
        for name, g in got.items():
            for x, y in zip(g, w[k][name]):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (name, k, s)
        assert got["topn"][0].dtype == torch.float64 and got["metrics"][0].dtype == torch.float64
        assert got["topk"][0].shape == (c[0].shape[0], k) and got["topk"][0].is_contiguous()


@pytest.mark.parametrize("shard_items", [1000, 999, 333, 256, 7])
def test_sharded_search_and_histograms_equal_the_whole(shard_items):
    """Q = 9, N = 1000, 16-bit codes with zeros, 6 classes: one shard (no merge), a last shard of one item, four shards, shards of
    the chunk granularity, 143 shards narrower than k."""
    c = _database(9, 1000, 16, 6, True, 5)
    _assert_sharded_equals_whole("b16", c, (1, 50, 1000), shard_items)


@pytest.mark.parametrize("K", [64, 512])
def test_sharded_equals_whole_at_wider_codes(K):
    """64 bit (two words in registers) and 512 bit (the columns in global memory), N = 700 as shards of 300 + 300 + 100."""
    c = _database(9, 700, K, 6, False, K)
    _assert_sharded_equals_whole(f"b{K}", c, (1, 50, 700), 300)


def test_fold_writes_two_buffer_sets_in_turn_and_makes_the_second_at_the_third_shard():
    import cmh_native as N
    import utils.retrieval as R
    qB, rB, _, _ = _database(3, 40, 16, 6, True, 11)
    qp, rp = R._codes(qB, DEV), R._codes(rB, DEV)
    k, shards, flat = 12, R._cuts(40, 10), [None, None]
    per = [N.hamming_topk(qp, R._rows(rp, sc, 40), 16, 10) for sc in shards]
    run, seen = per[0], []
    for s, (sc, b) in enumerate(zip(shards[1:], per[1:])):
        run = R._fold(run, b, sc, k, flat, s)
        seen.append((run[0].data_ptr(), flat[1] is None))
    assert [x[1] for x in seen] == [True, False, False] and seen[0][0] == seen[2][0] != seen[1][0]
    assert flat[0][0].numel() == 3 * k and flat[0][2] is None
    assert all(torch.equal(x, y) for x, y in zip(run[:2], N.hamming_topk(qp, rp, 16, k)))


# ---- 3. past the entry point's limit ----------------------------------------------------------------------------------------------
def test_search_of_a_database_one_shard_cannot_hold():
    """N = 524 288 + 37 (two shards at the default shard_items), 16-bit codes without zeros, 4 classes, k = 300, against NumPy in
    integer arithmetic."""
    import utils.retrieval as R
    rng = np.random.default_rng(3)
    Q, n, K, C, k = 3, 524288 + 37, 16, 4, 300
    qB, rB = rng.choice([-1, 1], (Q, K)).astype(np.int32), rng.choice([-1, 1], (n, K)).astype(np.int32)
    qL, rL = (rng.random((Q, C)) < 0.4).astype(np.int32), (rng.random((n, C)) < 0.4).astype(np.int32)
    qL[0] = [1, 0, 0, 1]
    rB[n - 1], rB[n - 30] = qB[0], qB[1]                          # the second shard holds the nearest item of two queries
    h = K - qB @ rB.T
    order = np.stack([np.argsort(h[i], kind="stable")[:k] for i in range(Q)])
    c = [torch.from_numpy(x.astype(np.float32)) for x in (qB, rB, qL, rL)]
    idx, dist, rel = R.hamming_topk(c[0], c[1], k, c[2], c[3])
    np.testing.assert_array_equal(idx.cpu().numpy(), order)
    np.testing.assert_array_equal(dist.cpu().numpy(), (0.5 * np.take_along_axis(h, order, 1)).astype(np.float32))
    np.testing.assert_array_equal(rel.cpu().numpy(), np.take_along_axis(qL @ rL.T > 0, order, 1).astype(np.uint8))
    assert bool((idx[:2] >= 524287).any(1).all()) and int(dist[0, 0]) == 0
    counts = R.pr_curve(*c)[2]
    assert counts.dtype == torch.int32 and counts.shape == (Q, 2 * K + 1, 2)
    np.testing.assert_array_equal(counts.long().sum((1, 2)).cpu().numpy(), [n] * Q)
    np.testing.assert_array_equal(counts[:, :, 1].long().sum(1).cpu().numpy(), (qL @ rL.T > 0).sum(1))


# ---- 4. query blocks --------------------------------------------------------------------------------------------------------------
def test_more_queries_than_one_call_takes():
    import cmh_native as N
    import utils.retrieval as R
    rng = np.random.default_rng(4)
    Q, n, K, k = 65536 + 5, 8, 16, 8
    qB, rB = _t(rng.choice([-1.0, 0.0, 1.0], (Q, K)).astype(np.float32)), _t(rng.choice([-1.0, 1.0], (n, K)).astype(np.float32))
    qL, rL = _t((rng.random((Q, 3)) < 0.4).astype(np.float32)), _t((rng.random((n, 3)) < 0.4).astype(np.float32))
    got = R.hamming_topk(qB, rB, k, qL, rL)
    rp, rl = N.pack_codes(rB), N.pack_labels(rL)
    blocks = [N.hamming_topk(N.pack_codes(qB[a:b]), rp, K, k, N.pack_labels(qL[a:b]), rl) for a, b in ((0, 65535), (65535, Q))]
    for j in range(3):
        assert got[j].shape == (Q, k) and torch.equal(got[j], torch.cat([blocks[0][j], blocks[1][j]]))
    counts = R.pr_curve(qB, rB, qL, rL)[2]
    assert counts.shape == (Q, 2 * K + 1, 2) and bool((counts.long().sum((1, 2)) == n).all())
    assert torch.equal(counts[65535:], N.hamming_hist(N.pack_codes(qB[65535:]), rp, K, N.pack_labels(qL[65535:]), rl))


# ---- 5. CodeIndex: growth and persistence -----------------------------------------------------------------------------------------
def test_code_index_grows_by_add_and_round_trips_through_a_file(tmp_path):
    import cmh_native as N
    from utils.retrieval import CodeIndex
    qB, rB, qL, rL = _database(9, 1000, 16, 6, True, 5)
    whole = CodeIndex(rB, rL)
    grown = CodeIndex(rB[:1], rL[:1], shard_items=256)
    assert grown.add(rB[1:301], rL[1:301]) is grown
    grown.add(rB[301:], rL[301:])
    bare = CodeIndex(rB[:1], shard_items=256).add(rB[1:301]).add(rB[301:])
    assert grown.size == bare.size == 1000 and grown.bits == 16 and grown.classes == 6 and bare.classes is None and bare.labels is None
    assert all(torch.equal(a, b) for a, b in zip(grown.planes, whole.planes)) and torch.equal(grown.labels, whole.labels)
    grown.save(tmp_path / "grown.npz")
    bare.save(tmp_path / "bare.npz")
    loaded, loaded_bare = CodeIndex.load(tmp_path / "grown.npz", shard_items=333), CodeIndex.load(tmp_path / "bare.npz")
    assert (loaded.size, loaded.bits, loaded.classes, loaded_bare.classes) == (1000, 16, 6, None)
    for k in (1, 300, 1000):
        want, want_g, want_p = whole.search(qB, k, qL), whole.search(qB, k, qL, graded=True), whole.search(qB, k)
        assert len(want) == 3 and len(want_g) == 3 and len(want_p) == 2
        for index in (grown, loaded):
            assert all(torch.equal(a, b) for a, b in zip(index.search(qB, k, qL), want))
            assert all(torch.equal(a, b) for a, b in zip(index.search(qB, k, qL, graded=True), want_g))
            assert all(torch.equal(a, b) for a, b in zip(index.search(qB, k), want_p))
        for index in (bare, loaded_bare):
            assert all(torch.equal(a, b) for a, b in zip(index.search(qB, k), want_p))
    # many small adds: one buffer per plane that doubles, not one shard per add
    small = CodeIndex(rB[:1], shard_items=256)
    caps = set()
    for i in range(1, 40):
        small.add(rB[i:i + 1])
        caps.add(small._sign.shape[0])
    assert small.size == 40 and len(caps) <= 7 and torch.equal(small.planes[0], whole.planes[0][:40])
    for bad in (lambda: grown.add(rB[:3, :8], rL[:3]), lambda: grown.add(rB[:3], rL[:3, :5]), lambda: grown.add(rB[:3]),
                lambda: bare.add(rB[:3], rL[:3]), lambda: grown.add(rB[:3], rL[:2]), lambda: bare.search(qB, 5, qL),
                lambda: grown.search(qB, 1001)):
        with pytest.raises(N.NativeError):
            bad()
    assert grown.size == 1000 and bare.size == 1000


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------
def test_retrieve_cli_searches_a_saved_index(tmp_path):
    import scipy.io as scio
    from utils.retrieval import CodeIndex
    qB, rB, qL, rL = (x.numpy() for x in _database(6, 90, 16, 6, True, 8))
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB[::-1].copy(), "r_img": rB, "r_txt": rB[::-1].copy(), "q_l": qL, "r_l": rL[::-1].copy()})
    index = CodeIndex.from_mat(str(mat), side="r_txt")
    half = CodeIndex(torch.from_numpy(rB[::-1][:40].copy()), torch.from_numpy(rL[::-1][:40].copy()), shard_items=32)
    half.add(torch.from_numpy(rB[::-1][40:].copy()), torch.from_numpy(rL[::-1][40:].copy())).save(tmp_path / "db.npz")
    assert torch.equal(half.planes[0], index.planes[0])
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for extra in ([], ["--index", str(tmp_path / "db.npz")]):
        out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(mat), "--direction", "i2t", "--k", "12",
                              "--queries", "1:5"] + extra, capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        assert ("r_txt" in out.stderr and "is not searched" in out.stderr) == bool(extra)      # --direction's database half is unused
        outs.append(out.stdout)
    assert outs[0] == outs[1] and len(outs[0].strip().splitlines()) == 4
    idx = index.search(torch.from_numpy(qB), 12, torch.from_numpy(qL))[0].cpu().numpy()
    first = outs[1].splitlines()[0].split()
    assert int(first[0]) == 1 and [int(c.split(":")[0]) for c in first[1:]] == idx[1].tolist() and first[1].count(":") == 2
