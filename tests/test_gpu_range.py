"""The radius search on the GPU (cmh_hamming_range, utils/retrieval.py::hamming_range, CodeIndex.range_search / duplicates,
retrieve.py --radius) against the NumPy restatement of tests/rangeutil.py, against hamming_topk, sharded against whole, past one
call's limits, and at the edges.  Integers and half-integers: every comparison is exact.

Random codes concentrate at K / 2, so the random-code radii are 0.375 K, 0.4375 K, 0.5 K and K; for the small radii 0, 0.5, 1 and 2
neighbours are planted (rangeutil.plant) at row 0, row N - 1 and on both sides of a chunk edge and of a shard edge.  Every test
asserts that its inputs hold an empty ball, a singleton and a ball whose items lie in more than one chunk, where its shape allows
them (a database of one chunk has no second chunk; the note sits at the test)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rangeutil as U
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_RADII = (0, 0.5, 1, 2)


def _radii(K):
    return SMALL_RADII + (0.375 * K, 0.4375 * K, 0.5 * K, K)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pack(qB, rB, qL=None, rL=None):
    import utils.retrieval as R
    return (R._codes(torch.from_numpy(qB), DEV), R._codes(torch.from_numpy(rB), DEV),
            None if qL is None else R._labels(torch.from_numpy(qL), DEV), None if rL is None else R._labels(torch.from_numpy(rL), DEV))


def _one_call(qp, rp, bits, hr, ql=None, rl=None):
    """hist -> offsets -> ONE cmh_hamming_range over the whole database: (offsets, idx, dist, rel or None)."""
    import cmh_native as N
    counts = N.hamming_hist(qp, rp, bits, ql, rl)
    off = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=DEV)
    off[1:] = counts[:, :hr + 1].sum((1, 2)).cumsum(0)
    T = int(off[-1])
    out = (torch.empty(T, dtype=torch.int32, device=DEV), torch.empty(T, dtype=torch.float32, device=DEV),
           None if ql is None else torch.empty(T, dtype=torch.uint8, device=DEV))
    if T:
        N.hamming_range(qp, rp, bits, hr, ql, rl, row_off=off[:-1].contiguous(), out=out)
    return (off,) + out


def _same(got, want, note=None):
    """A CSR result on the GPU (three tensors without labels, four with; a fourth that is None counts as absent) equals the
    restatement's arrays, dtypes included."""
    if len(got) == 4 and got[3] is None:
        got = got[:3]
    assert len(got) == (3 if want[3] is None else 4), note
    for g, w, dt in zip(got, want, (torch.int64, torch.int32, torch.float32, torch.uint8)):
        assert g.dtype == dt and g.is_cuda and g.dim() == 1, note
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=str(note))


def _holds(off, idx, chunk, empty=1, single=1, spans=1):
    e, s, m = U.ball_facts(np.asarray(off), np.asarray(idx), chunk)
    return e >= empty and s >= single and m >= spans


_CASES = {}


def _case(K, Q, n, C, zeros, edges=None, planted=True, seed=None):
    """Inputs, their packed planes and the integer half-units, built once per shape and shared."""
    key = (K, Q, n, C, zeros, edges, planted, seed)
    if key not in _CASES:
        qB, rB, qL, rL = U.database(Q, n, K, C or 6, zeros, K + Q if seed is None else seed)
        chunk = U.chunk_items(Q, n, K, _cus())
        if planted:
            U.plant(qB, rB, edges or (chunk, 2 * chunk))
        if C is None:
            qL = rL = None
        _CASES[key] = dict(qB=qB, rB=rB, qL=qL, rL=rL, chunk=chunk, h=U.half_units(qB, rB), packed=_pack(qB, rB, qL, rL))
    return _CASES[key]


def _facts(seen, off, idx, chunk):
    e, s, m = U.ball_facts(off, idx, chunk)
    seen["empty"] += e
    seen["single"] += s
    seen["spans"] += m


# ---- 1. against NumPy, one native call --------------------------------------------------------------------------------------------
# bits: 16 (one word), 24 (a partial word, with zeros), 64, 96 (three words), 128 (four), 160 (columns in global memory);
# Q around the 64-query tile; N around the 256-item floor of a chunk and at five chunks; labels: none, one word, three words, two words
# (the any-width path).
RICH = [(16, 63, 257, None, True), (24, 64, 1031, 24, True), (64, 65, 1031, 80, False), (96, 130, 257, 40, True),
        (128, 65, 1031, 24, False), (160, 64, 1031, 40, True), (160, 130, 257, None, False), (64, 130, 1031, 40, True)]


@pytest.mark.parametrize("K,Q,n,C,zeros", RICH)
def test_lists_equal_the_restatement(K, Q, n, C, zeros):
    import utils.retrieval as R
    c = _case(K, Q, n, C, zeros)
    qp, rp, ql, rl = c["packed"]
    seen = dict(empty=0, single=0, spans=0)
    for radius in _radii(K):
        hr = U.half_radius(radius, K)
        want = U.range_lists(c["h"], hr, c["qL"], c["rL"])
        _same(_one_call(qp, rp, K, hr, ql, rl), want, (K, Q, n, radius))
        labels = () if C is None else (torch.from_numpy(c["qL"]), torch.from_numpy(c["rL"]))
        got = R.hamming_range(torch.from_numpy(c["qB"]), torch.from_numpy(c["rB"]), radius, *labels)
        assert len(got) == (3 if C is None else 4)
        _same(got, want, (K, Q, n, radius, "function"))
        _facts(seen, want[0], want[1], c["chunk"])
    assert min(seen.values()) > 0, seen
    whole = U.range_lists(c["h"], 2 * K)[0]
    np.testing.assert_array_equal(np.diff(whole), [n] * Q)             # radius K: the whole database for every query


def test_lists_at_the_smallest_shapes():
    """One query, one item, a database just below / at the one-chunk floor: no second chunk there, so the multi-chunk ball of this
    test's inputs is the (16 bit, 63 x 257) case's that runs with them."""
    seen = dict(empty=0, single=0, spans=0)
    for K, Q, n, C, zeros in [(16, 1, 1, None, True), (16, 1, 255, 24, True), (64, 3, 256, 80, False), (128, 1, 1, 40, False),
                              (160, 1, 1, 24, True), (24, 63, 255, None, True), (96, 1, 257, None, False), (16, 63, 257, None, True)]:
        c = _case(K, Q, n, C, zeros)
        qp, rp, ql, rl = c["packed"]
        for radius in _radii(K):
            hr = U.half_radius(radius, K)
            want = U.range_lists(c["h"], hr, c["qL"], c["rL"])
            _same(_one_call(qp, rp, K, hr, ql, rl), want, (K, Q, n, radius))
            _facts(seen, want[0], want[1], c["chunk"])
    assert min(seen.values()) > 0, seen


# ---- 2. against the search --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Q,n,C,zeros", [RICH[0], RICH[2], RICH[5]])
def test_a_list_is_the_head_of_the_search_row(K, Q, n, C, zeros):
    """For every query the list equals row q of hamming_topk(k = the largest ball) cut at ball(q)."""
    import utils.retrieval as R
    c = _case(K, Q, n, C, zeros)
    t = [None if c[x] is None else torch.from_numpy(c[x]) for x in ("qB", "rB", "qL", "rL")]
    labels = () if C is None else tuple(t[2:])
    seen = dict(empty=0, single=0, spans=0)
    for radius in (0, 0.5, 2, 0.4375 * K, 0.5 * K, K):
        got = R.hamming_range(t[0], t[1], radius, *labels)
        ball = got[0][1:] - got[0][:-1]
        kmax = int(ball.max())
        assert kmax >= 1
        rows = R.hamming_topk(t[0], t[1], kmax, *labels)
        head = torch.arange(kmax, device=DEV)[None, :] < ball[:, None]
        assert len(rows) == len(got) - 1
        for lst, row in zip(got[1:], rows):
            assert torch.equal(lst, row[head]), (K, radius)
        _facts(seen, got[0].cpu().numpy(), got[1].cpu().numpy(), c["chunk"])
    assert min(seen.values()) > 0, seen


# ---- 3. guarded outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Q,n,C,zeros", [RICH[1], RICH[3], RICH[6]])
def test_nothing_outside_the_rows_is_written_and_every_word_inside_is(K, Q, n, C, zeros):
    """out buffers of T + 64 entries filled with a sentinel, row_off shifted by 32: the 32 entries before and behind the rows are
    untouched, no sentinel is left inside, two calls give equal bits."""
    import cmh_native as N
    c = _case(K, Q, n, C, zeros)
    qp, rp, ql, rl = c["packed"]
    seen = dict(empty=0, single=0, spans=0)
    for radius in (0, 1, 0.4375 * K, K):
        hr = U.half_radius(radius, K)
        want = U.range_lists(c["h"], hr, c["qL"], c["rL"])
        T = int(want[0][-1])
        row_off = _t(want[0][:-1] + 32)

        def filled():
            out = (torch.full((T + 64,), -7, dtype=torch.int32, device=DEV), torch.full((T + 64,), -7.0, device=DEV),
                   None if C is None else torch.full((T + 64,), 9, dtype=torch.uint8, device=DEV))
            ret = N.hamming_range(qp, rp, K, hr, ql, rl, row_off=row_off, out=out)
            assert all((r is None and o is None) or r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))
            return out

        a, b = filled(), filled()
        for x, y, w, guard in zip(a, b, want[1:], (-7, -7.0, 9)):
            if x is None:
                continue
            assert torch.equal(x, y)
            x = x.cpu().numpy()
            assert (x[:32] == guard).all() and (x[T + 32:] == guard).all(), (K, radius)
            np.testing.assert_array_equal(x[32:T + 32], w)
            assert not (x[32:T + 32] == guard).any()                  # (no index or distance is negative, no flag is 9)
        _facts(seen, want[0], want[1], c["chunk"])
    assert min(seen.values()) > 0, seen


# ---- 4. sharded equals whole ------------------------------------------------------------------------------------------------------
_WHOLE = {}


def _whole(key, c, radius, labels):
    import utils.retrieval as R
    k = (key, radius, labels)
    if k not in _WHOLE:
        t = [torch.from_numpy(c[x]) for x in ("qB", "rB", "qL", "rL")]
        _WHOLE[k] = R.hamming_range(t[0], t[1], radius, *(t[2:] if labels else ()))
    return _WHOLE[k]


def _assert_sharded_equals_whole(key, c, radii, s, K):
    import utils.retrieval as R
    t = [torch.from_numpy(c[x]) for x in ("qB", "rB", "qL", "rL")]
    seen = dict(empty=0, single=0, spans=0)
    for radius in radii:
        for labels in (True, False):
            whole = _whole(key, c, radius, labels)
            got = R.hamming_range(t[0], t[1], radius, *(t[2:] if labels else ()), shard_items=s)
            assert len(got) == len(whole) == (4 if labels else 3)
            for x, y in zip(got, whole):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (key, radius, s, labels)
        whole = _whole(key, c, radius, True)
        _same(whole, U.range_lists(c["h"], U.half_radius(radius, K), c["qL"], c["rL"]), (key, radius))
        _facts(seen, whole[0].cpu().numpy(), whole[1].cpu().numpy(), c["chunk"])
    assert min(seen.values()) > 0, seen


@pytest.mark.parametrize("shard_items", [1000, 999, 333, 256, 7])
def test_sharded_lists_equal_the_whole(shard_items):
    """Q = 9, N = 1000, 16-bit codes with zeros, 6 classes (random codes alone: radius 4 has one empty ball, singletons and balls of
    up to 6 items, 20 in all; radius 6 holds 789, radius 16 the database): one shard, a last shard of one item, four shards, shards
    of the chunk granularity, 143 shards."""
    c = _case(16, 9, 1000, 6, True, planted=False, seed=5)
    assert [int(U.range_lists(c["h"], 2 * r)[0][-1]) for r in (4, 5, 6, 16)] == [20, 179, 789, 9000]
    _assert_sharded_equals_whole("b16", c, (4, 6, 16), shard_items, 16)


@pytest.mark.parametrize("K", [64, 512])
def test_sharded_equals_whole_at_wider_codes(K):
    """64 bit (two words in registers) and 512 bit (the columns in global memory), N = 700 as shards of 300 + 300 + 100, neighbours
    planted on both sides of a chunk edge and of the shard edge at row 300."""
    chunk = U.chunk_items(9, 700, K, _cus())
    c = _case(K, 9, 700, 6, False, edges=(chunk, 300), seed=K)
    _assert_sharded_equals_whole(f"b{K}", c, (0, 0.5, 2, 0.4375 * K, K), 300, K)


# ---- 5. past one call's limit -----------------------------------------------------------------------------------------------------
def test_lists_over_a_database_one_shard_cannot_hold():
    """N = 524 288 + 37 (two shards at the default shard_items), 16-bit codes, Q = 3, radius 1, against NumPy.  Every database row
    but the planted ones begins (+1, +1); query 0 does too (its ball: ~480 items over both shards and many chunks), queries 1 and 2
    begin (-1, -1) and so lie at distance >= 2 from every unplanted row: query 1 has one planted copy in the second shard (a
    singleton), query 2 none (an empty ball)."""
    import utils.retrieval as R
    rng = np.random.default_rng(3)
    Q, n, K, C = 3, 524288 + 37, 16, 4
    qB, rB = rng.choice([-1, 1], (Q, K)).astype(np.int32), rng.choice([-1, 1], (n, K)).astype(np.int32)
    qL, rL = (rng.random((Q, C)) < 0.4).astype(np.int32), (rng.random((n, C)) < 0.4).astype(np.int32)
    rB[:, :2] = 1
    qB[0, :2], qB[1, :2], qB[2, :2] = 1, -1, -1
    qB[2, 2:] = -qB[1, 2:]
    rB[n - 1], rB[n - 30], rB[n - 7] = qB[0], qB[1], qB[0]            # the second shard holds the nearest items of two queries
    rB[n - 7, 5] *= -1
    h = K - qB @ rB.T
    want = U.range_lists(h, 2, qL, rL)
    sizes = np.diff(want[0])
    assert sizes[0] > 100 and sizes[1] == 1 and sizes[2] == 0
    assert _holds(want[0], want[1], U.chunk_items(Q, 524287, K, _cus()))
    c = [torch.from_numpy(x.astype(np.float32)) for x in (qB, rB, qL, rL)]
    got = R.hamming_range(c[0], c[1], 1, c[2], c[3])
    _same(got, want)
    assert int((got[1] >= 524287).sum()) >= 3 and int(got[1][got[0][1]]) == n - 30
    _same(R.hamming_range(c[0], c[1], 1), U.range_lists(h, 2))


# ---- 6. query blocks --------------------------------------------------------------------------------------------------------------
def test_more_queries_than_one_call_takes():
    """Q = 65 536 + 5, N = 8 (one chunk: no ball can span two), radius K / 2: the two blocks' results concatenated, offsets rebased."""
    import cmh_native as N
    import utils.retrieval as R
    rng = np.random.default_rng(4)
    Q, n, K = 65536 + 5, 8, 16
    qB, rB = rng.choice([-1.0, 0.0, 1.0], (Q, K)).astype(np.float32), rng.choice([-1.0, 1.0], (n, K)).astype(np.float32)
    qL, rL = (rng.random((Q, 3)) < 0.4).astype(np.float32), (rng.random((n, 3)) < 0.4).astype(np.float32)
    got = R.hamming_range(_t(qB), _t(rB), K / 2, _t(qL), _t(rL))
    rp, rl = N.pack_codes(_t(rB)), N.pack_labels(_t(rL))
    blocks = [_one_call(N.pack_codes(_t(qB[a:b])), rp, K, K, N.pack_labels(_t(qL[a:b])), rl) for a, b in ((0, 65535), (65535, Q))]
    assert got[0].shape == (Q + 1,) and got[0].dtype == torch.int64
    assert torch.equal(got[0], torch.cat([blocks[0][0], blocks[1][0][1:] + blocks[0][0][-1]]))
    for j in (1, 2, 3):
        assert torch.equal(got[j], torch.cat([blocks[0][j], blocks[1][j]]))
    sizes = (U.half_units(qB, rB) <= K).sum(1)
    np.testing.assert_array_equal(np.diff(got[0].cpu().numpy()), sizes)
    assert (sizes == 0).any() and (sizes == 1).any() and (sizes[65535:] > 0).any()


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------------
def test_empty_result_whole_database_size_guard_and_one_sided_labels(monkeypatch):
    import cmh_native as N
    import utils.retrieval as R
    c = _case(16, 63, 257, 6, True)
    t = [torch.from_numpy(c[x]) for x in ("qB", "rB", "qL", "rL")]
    K, Q, n = 16, 63, 257
    # radius >= K: the whole database for every query, in (distance, index) order
    want = U.range_lists(c["h"], 2 * K, c["qL"], c["rL"])
    for radius in (K, K + 5, math.inf):
        got = R.hamming_range(*t[:2], radius, *t[2:])
        _same(got, want, radius)
        np.testing.assert_array_equal(np.diff(got[0].cpu().numpy()), [n] * Q)
    # the size guard: T - 1 is refused (the message names T), T passes
    want = U.range_lists(c["h"], 12, c["qL"], c["rL"])
    T = int(want[0][-1])
    assert _holds(want[0], want[1], c["chunk"], empty=0, single=0) and T > Q
    _same(R.hamming_range(*t[:2], 6, *t[2:], max_hits=T), want)
    fills = []
    real = N.hamming_range
    monkeypatch.setattr(N, "hamming_range", lambda *a, **k: fills.append(1) or real(*a, **k))
    with pytest.raises(N.NativeError, match=f"T={T}"):
        R.hamming_range(*t[:2], 6, *t[2:], max_hits=T - 1)
    assert not fills                                                  # refused before the outputs exist: nothing was filled
    with pytest.raises(N.NativeError):
        R.hamming_range(*t[:2], 6, t[2])                              # labels on one side only
    with pytest.raises(N.NativeError):
        R.hamming_range(*t[:2], 6, retrieval_L=t[3])
    # every ball empty: T = 0, empty tensors of the right dtypes, offsets all zero, no fill pass
    far_q, far_r = torch.ones(5, K), -torch.ones(300, K)
    for labels in ((), (torch.ones(5, 3), torch.ones(300, 3))):
        got = R.hamming_range(far_q, far_r, 2, *labels)
        assert len(got) == 3 + bool(labels) and not fills
        assert got[0].dtype == torch.int64 and got[0].shape == (6,) and not bool(got[0].any())
        assert [(x.dtype, tuple(x.shape), x.is_cuda) for x in got[1:]] == \
            [(torch.int32, (0,), True), (torch.float32, (0,), True), (torch.uint8, (0,), True)][:len(got) - 1]
    # (this test's inputs: empty balls above, a singleton and a multi-chunk ball at radius 0 of the planted case)
    small = U.range_lists(c["h"], 0)
    assert _holds(small[0], small[1], c["chunk"])
    _same(R.hamming_range(*t[:2], 0), small)
    assert len(fills) == 1


# ---- 8. CodeIndex -----------------------------------------------------------------------------------------------------------------
def test_code_index_range_search_and_duplicates(tmp_path):
    import cmh_native as N
    import utils.retrieval as R
    from utils.retrieval import CodeIndex
    c = _case(64, 65, 1031, 80, False)
    qB, rB, qL, rL = (torch.from_numpy(c[x]) for x in ("qB", "rB", "qL", "rL"))
    whole = CodeIndex(rB, rL)
    grown = CodeIndex(rB[:300], rL[:300], shard_items=256).add(rB[300:], rL[300:])
    grown.save(tmp_path / "grown.npz")
    loaded = CodeIndex.load(tmp_path / "grown.npz", shard_items=333)
    bare = CodeIndex(rB, shard_items=400)
    seen = dict(empty=0, single=0, spans=0)
    for radius in (0, 0.5, 2, 28):
        want, plain = R.hamming_range(qB, rB, radius, qL, rL), R.hamming_range(qB, rB, radius)
        _same(want, U.range_lists(c["h"], U.half_radius(radius, 64), c["qL"], c["rL"]))
        for index in (whole, grown, loaded):
            got = index.range_search(qB, radius, qL)
            assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
            got = index.range_search(qB, radius)
            assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, plain))
        assert all(torch.equal(a, b) for a, b in zip(bare.range_search(qB, radius), plain))
        _facts(seen, want[0].cpu().numpy(), want[1].cpu().numpy(), c["chunk"])
    assert min(seen.values()) > 0, seen
    with pytest.raises(N.NativeError):
        bare.range_search(qB, 1, qL)                                  # query labels, an index without
    with pytest.raises(N.NativeError):
        whole.range_search(qB[:, :32], 1)
    with pytest.raises(N.NativeError):
        whole.range_search(qB, 28, max_hits=3)

    # duplicates: two planted triples, a near-duplicate of one of them, a code with a zero (not within radius 0 of itself)
    rng = np.random.default_rng(21)
    n, K = 600, 64
    codes = rng.choice([-1.0, 1.0], (n, K)).astype(np.float32)
    labels = (rng.random((n, 6)) < 0.3).astype(np.float32)
    codes[300] = codes[599] = codes[5]
    codes[11] = codes[400] = codes[10]
    codes[20] = codes[5]
    codes[20, 7] *= -1
    codes[50, 3] = 0
    h = U.half_units(codes, codes)
    index = CodeIndex(torch.from_numpy(codes), torch.from_numpy(labels), shard_items=256)
    lists = {}
    for radius in (0, 1):
        off, idx, dist, rel = (x.cpu().numpy() for x in index.duplicates(radius))
        w_off, w_idx, w_dist, w_rel = U.range_lists(h, 2 * radius, labels, labels)
        item = np.repeat(np.arange(n), np.diff(w_off))
        keep = w_idx != item
        np.testing.assert_array_equal(idx, w_idx[keep])
        np.testing.assert_array_equal(dist, w_dist[keep])
        np.testing.assert_array_equal(rel, w_rel[keep])
        np.testing.assert_array_equal(np.diff(off), np.bincount(item[keep], minlength=n))
        assert off.dtype == np.int64 and off[0] == 0 and off[-1] == idx.size
        lists[radius] = [idx[off[i]:off[i + 1]].tolist() for i in range(n)]
    triples = {5: [300, 599], 300: [5, 599], 599: [5, 300], 10: [11, 400], 11: [10, 400], 400: [10, 11]}
    assert all(lists[0][i] == triples.get(i, []) for i in range(n))   # the other two members; nothing for singletons
    assert all(set(lists[0][i]) <= set(lists[1][i]) for i in range(n))
    assert lists[1][5] == [300, 599, 20] and lists[1][20] == [5, 300, 599] and lists[1][50] == [] and lists[0][50] == []
    assert len(CodeIndex(torch.from_numpy(codes)).duplicates(0)) == 3


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------
def test_retrieve_cli_prints_the_balls(tmp_path):
    import scipy.io as scio
    from utils.retrieval import CodeIndex
    c = _case(16, 9, 300, 6, True)
    qB, rB, qL, rL = c["qB"], c["rB"], c["qL"], c["rL"]
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB[::-1].copy(), "r_img": rB[::-1].copy(), "r_txt": rB, "q_l": qL, "r_l": rL})
    CodeIndex(torch.from_numpy(rB[:100]), torch.from_numpy(rL[:100]), shard_items=128).add(
        torch.from_numpy(rB[100:]), torch.from_numpy(rL[100:])).save(tmp_path / "db.npz")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(mat), "--direction", "i2t"]
    want = U.range_lists(c["h"], 4, qL, rL)
    assert _holds(want[0], want[1], c["chunk"])
    lines = []
    for q in range(7):
        a, b = want[0][q], want[0][q + 1]
        lines.append(" ".join([str(q)] + [f"{want[1][j]}:{want[2][j]:g}:{want[3][j]}" for j in range(a, b)]))
    for extra in ([], ["--index", str(tmp_path / "db.npz")]):
        out = subprocess.run(base + ["--radius", "2", "--queries", "0:7", "--max-hits", "100000"] + extra, capture_output=True, text=True,
                             timeout=600, env=env, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.splitlines() == lines
    out = subprocess.run(base + ["--radius", "2", "--k", "3"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode != 0 and "--radius" in out.stderr and out.stdout == ""
