"""cmh_hamming_topk_few (csrc/retrieval_few.hip: lanes own items, any database size in one call) against two references that do
not run it: NumPy's stable argsort over rankutil.half_units, and N.hamming_topk (lanes own queries) on the same planes; past one
call of that, the tiles route over shards.  Integers and half-integers: every comparison is torch.equal.  Then the routing of
utils/retrieval.py::_search."""
import numpy as np
import pytest
import torch

import rankutil

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(B):
    import cmh_native as N
    return N.pack_codes(_t(B))


def _numpy_topk(qB, rB, k):
    h = rankutil.half_units(qB, rB)
    order = np.argsort(h, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), (0.5 * np.take_along_axis(h, order, 1)).astype(np.float32)


def _check(qB, rB, ks, tiles=True):
    """few == NumPy (and == the tiles kernel) for every k of ks on one pair of code matrices."""
    import cmh_native as N
    qp, rp = _planes(qB), _planes(rB)
    bits = qB.shape[1]
    for k in ks:
        idx, dist = N.hamming_topk_few(qp, rp, bits, k)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (qB.shape[0], k)
        want_idx, want_dist = _numpy_topk(qB, rB, k)
        assert torch.equal(idx, _t(want_idx)), (qB.shape, rB.shape, k)
        assert torch.equal(dist, _t(want_dist)), (qB.shape, rB.shape, k)
        if tiles:
            t_idx, t_dist, _ = N.hamming_topk(qp, rp, bits, k)
            assert torch.equal(idx, t_idx) and torch.equal(dist, t_dist)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_edges_of_the_item_walk(n):
    """One item, one short of a wave, a wave, one more, one past a 256-item set of slabs, 17 chunks with a ragged last one; 1, 2, 5
    queries and a full group of four workgroups per chunk; k = 1, 7 and the whole page."""
    for Q in (1, 2, 5, 64):
        qB, rB = rankutil.codes(Q, n, 64, 0.1, 1000 + 7 * n + Q)
        _check(qB, rB, sorted({1, min(7, n), min(n, 4096)}))


@pytest.mark.parametrize("bits", [16, 32, 33, 64, 96, 128])
def test_code_widths_and_the_cut_of_the_last_word(bits):
    """1..4 words per plane, and 33 bits: one bit in the second word.  The database planes then get set bits behind `bits`
    (pack_codes writes zeros there): a query cut to `bits` bits must not count them."""
    import cmh_native as N
    qB, rB = rankutil.codes(5, 4099, bits, 0.1, 2000 + bits)
    _check(qB, rB, [1, 7, 4096])
    if bits % 32:
        qp, (rs, rn) = _planes(qB), _planes(rB)
        high = torch.tensor(-(1 << (bits % 32)), dtype=torch.int32, device=DEV)        # the bits at and above `bits` of the last word
        rs, rn = rs.clone(), rn.clone()
        rs[:, -1] |= high
        rn[:, -1] |= high
        idx, dist = N.hamming_topk_few(qp, (rs, rn), bits, 100)
        want_idx, want_dist = _numpy_topk(qB, rB, 100)
        assert torch.equal(idx, _t(want_idx)) and torch.equal(dist, _t(want_dist))


def test_ternary_codes_zero_query_and_zero_item():
    """A zero bit counts half a unit: an all-zero query is at bits / 2 from everything (the answer is 0..k-1), an all-zero item at
    bits / 2 from every query."""
    qB, rB = rankutil.codes(5, 4099, 64, 0.1, 31)
    qB[2] = 0.0
    rB[0] = 0.0
    rB[300] = 0.0
    rB[4098] = 0.0
    _check(qB, rB, [1, 7, 4096])
    import cmh_native as N
    idx, dist = N.hamming_topk_few(_planes(qB[2:3]), _planes(rB), 64, 50)
    assert idx[0].tolist() == list(range(50)) and dist[0].tolist() == [32.0] * 50


def test_ties_across_chunks():
    """16-bit codes on 4099 items: tie groups of hundreds, so the cut inside the group at h* falls across chunk boundaries; a
    database of identical codes: indices 0..k-1 at one distance; the query's own code at items 0, 255, 256 and 4098 (bin 0)."""
    import cmh_native as N
    qB, rB = rankutil.codes(5, 4099, 16, 0, 41)
    for j in (0, 255, 256, 4098):
        rB[j] = qB[0]
    _check(qB, rB, [1, 4, 5, 300, 1000, 4096])
    idx, dist = N.hamming_topk_few(_planes(qB[:1]), _planes(rB), 16, 4)
    assert idx[0].tolist() == [0, 255, 256, 4098] and dist[0].tolist() == [0.0] * 4
    same = np.repeat(rB[7:8], 4099, 0)
    for k in (1, 257, 4096):
        idx, dist = N.hamming_topk_few(_planes(qB), _planes(same), 16, k)
        h = rankutil.half_units(qB, same[:1])[:, 0]
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device=DEV).expand(5, k))
        assert torch.equal(dist, _t((0.5 * h).astype(np.float32))[:, None].expand(5, k))


def test_many_chunks():
    qB, rB = rankutil.codes(3, 70001, 64, 0.1, 51)
    _check(qB, rB, [1000])


def test_past_one_tiles_call():
    """1 200 000 items: three shards and two merges on the tiles route, one call here.  Codes drawn on the GPU."""
    import cmh_native as N
    from utils import retrieval as R
    g = torch.Generator(device=DEV).manual_seed(61)
    n, bits = 1_200_000, 64
    rB = (torch.randint(0, 3, (n, bits), device=DEV, generator=g) - 1).float()
    qB = (torch.randint(0, 3, (3, bits), device=DEV, generator=g) - 1).float()
    qp, rp = N.pack_codes(qB), N.pack_codes(rB)
    idx, dist = N.hamming_topk_few(qp, rp, bits, 100)
    want = R._search("test", qp, rp, bits, 100, None, None, shard_items=524287)
    assert torch.equal(idx, want[0]) and torch.equal(dist, want[1])


def test_two_calls_give_equal_bytes_on_any_stream():
    import cmh_native as N
    qB, rB = rankutil.codes(5, 70001, 32, 0.1, 71)
    qp, rp = _planes(qB), _planes(rB)
    a = N.hamming_topk_few(qp, rp, 32, 1000)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = N.hamming_topk_few(qp, rp, 32, 1000)
    s.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals():
    import cmh_native as N
    assert N.FEW_Q_MAX == 64 and N.FEW_K_MAX == 4096
    qB, rB = rankutil.codes(65, 5000, 32, 0, 81)
    qp, rp = _planes(qB), _planes(rB)
    few = lambda q, r, bits, k: N.hamming_topk_few(q, r, bits, k)
    with pytest.raises(N.NativeError, match="Q=65"):
        few(qp, rp, 32, 10)
    q1 = tuple(x[:1] for x in qp)
    with pytest.raises(N.NativeError, match="k=4097"):
        few(q1, rp, 32, 4097)
    with pytest.raises(N.NativeError, match="exceeds N"):
        few(q1, tuple(x[:9] for x in rp), 32, 10)
    q5, r5 = (torch.zeros(1, 5, dtype=torch.int32, device=DEV),) * 2, (torch.zeros(50, 5, dtype=torch.int32, device=DEV),) * 2
    with pytest.raises(N.NativeError, match="bits=129"):
        few(q5, r5, 129, 10)
    for k in (0, -3, 2 ** 40):                                     # refused on the host, before Q x k entries are allocated
        with pytest.raises(N.NativeError, match="k="):
            few(q1, rp, 32, k)
    few(q1, rp, 32, 4096)                                          # the limits themselves are legal
    few(tuple(x[:64] for x in qp), rp, 32, 1)


def test_routing_of_the_search(monkeypatch):
    """With QUERIES_FEW as committed: one query against a CodeIndex gives the tiles kernel's row, with and without labels (the hit
    flags from the gathered label words equal the select pass's); the same call with a shard size still goes through shards."""
    import cmh_native as N
    from utils import retrieval as R
    rng = np.random.default_rng(91)
    qB, rB = rankutil.codes(3, 4099, 32, 0.1, 91)
    qL, rL = (rng.random((3, 40)) < 0.1).astype(np.float32), (rng.random((4099, 40)) < 0.1).astype(np.float32)      # two label words
    qL[:, 0] = 1.0
    q, r, ql, rl = (torch.from_numpy(x) for x in (qB, rB, qL, rL))
    index = R.CodeIndex(r, rl)
    want = N.hamming_topk(_planes(qB[:1]), _planes(rB), 32, 10, N.pack_labels(_t(qL[:1])), N.pack_labels(_t(rL)))
    calls = {"few": 0, "merge": 0}
    real_few, real_merge = N.hamming_topk_few, N.topk_merge
    monkeypatch.setattr(N, "hamming_topk_few", lambda *a, **k: calls.__setitem__("few", calls["few"] + 1) or real_few(*a, **k))
    monkeypatch.setattr(N, "topk_merge", lambda *a, **k: calls.__setitem__("merge", calls["merge"] + 1) or real_merge(*a, **k))
    got = index.search(q[:1], 10, ql[:1])
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
    plain = index.search(q[:1], 10)
    assert len(plain) == 2 and torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])
    assert calls["few"] == (2 if R.QUERIES_FEW >= 1 else 0) and calls["merge"] == 0
    sharded = R.CodeIndex(r, rl, shard_items=1000)
    got = sharded.search(q[:1], 10, ql[:1])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert calls["merge"] >= 1 and calls["few"] == (2 if R.QUERIES_FEW >= 1 else 0)


def test_bad_labels_are_refused_on_the_few_route(monkeypatch):
    """The native call takes no labels; the route checks them before it gathers the results' label words, as the tiles route's
    binding does: labels on one side only, other word counts on the two sides (20 classes against 40 would broadcast), a label
    matrix shorter than the database (the gather would read behind it)."""
    import cmh_native as N
    from utils import retrieval as R
    monkeypatch.setattr(R, "QUERIES_FEW", 64)                      # the route itself, whatever the committed constant
    qB, rB = rankutil.codes(2, 500, 32, 0, 101)
    qp, rp = _planes(qB), _planes(rB)
    lab = lambda rows, classes: N.pack_labels(torch.ones(rows, classes, device=DEV))
    assert R._few_route(2, 10, 32, None, False, False)
    for ql, rl in ((lab(2, 20), lab(500, 40)), (lab(2, 40), lab(500, 20)), (lab(2, 40), lab(499, 40)), (lab(3, 40), lab(500, 40)),
                   (lab(2, 40), None), (None, lab(500, 40)), (lab(2, 40).long(), lab(500, 40).long())):
        with pytest.raises(N.NativeError):
            R._search("test", qp, rp, 32, 10, ql, rl)
    with pytest.raises(N.NativeError):
        R.CodeIndex(torch.from_numpy(rB), torch.ones(500, 40)).search(torch.from_numpy(qB), 10, torch.ones(2, 20))
    idx, dist, rel, _ = R._search("test", qp, rp, 32, 10, lab(2, 40), lab(500, 40))
    assert rel.dtype == torch.uint8 and bool(rel.all())
