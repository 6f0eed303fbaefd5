"""The k nearest through the substring tables on the GPU (csrc/retrieval_mih.hip: cmh_mih_knn_count / _fill;
utils/retrieval.py::SubstringTables.topk, CodeIndex.search_tables; retrieve.py --tables) against the scan (hamming_topk on the same
tensors) and NumPy brute force.  Everything is an integer, an index, a whole-bit distance or a flag: every comparison is exact."""
import numpy as np
import pytest
import torch

import mihknnutil as K
import mihutil as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BITS = (16, 24, 32, 64, 96, 128)                                   # W = 1 .. 4; 24: a short last substring
SIZES = (1, 255, 256, 257, 2049, 5000)
QUERIES = (1, 3, 65)                                               # 65: past hamming_topk's few-query route


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


def _ks(n):
    return sorted({min(k, n) for k in (1, 2, 7, 300)})


_made = {}


def _case(bits, n):
    """-> (database {0, 1}, rB, rL on the GPU, its SubstringTables), made once per shape: half uniform, half clustered; from 2 049
    items on one code occurs 300 times (ties at r* beyond k, across a round of 256 candidates)."""
    from utils.retrieval import SubstringTables
    import cmh_native as Nv
    if (bits, n) not in _made:
        db = K.draw(n, bits, seed=bits * 7 + n, copies=300 if n >= 2049 else 0)
        rB = _t(U.codes(db))
        _made[bits, n] = (db, rB, _t(U.labels(n, bits + n)), SubstringTables.build(Nv.pack_codes(rB), bits))
    return _made[bits, n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_topk_equals_the_scan(bits, n):
    from utils.retrieval import hamming_topk
    db, rB, rL, tables = _case(bits, n)
    tabled = scanned = 0
    for Q in QUERIES:
        q = K.queries(db, Q, seed=Q)
        qB, qL = _t(U.codes(q)), _t(U.labels(Q, 100 + Q))
        for k in _ks(n):
            want = hamming_topk(qB, rB, k, qL, rL)
            got = tables.topk(qB, k, qL, rL, max_ball=n)           # every ball within the tables' reach goes through them
            assert len(got) == 3
            _same(got, want)
            if k == 7 or n == 1:
                _same(tables.topk(qB, k), want[:2])                # no labels, the default max_ball
            radius = tables_radius(tables, qB, k)
            tabled += int((radius >= 0).sum())
            scanned += int((radius < 0).sum())
    assert tabled > 0 and (scanned > 0 or n == 1 or bits <= 24)     # both routes took part


def tables_radius(tables, qB, k, r_cap=None):
    import cmh_native as Nv
    qs = Nv.pack_codes(qB)[0].contiguous()
    return Nv.mih_knn_count(qs, tables.sign, tables.bits, k, tables.max_radius if r_cap is None else r_cap, tables.order, tables.starts)[0]


@pytest.mark.parametrize("bits,n", [(16, 5000), (24, 2049), (32, 257), (64, 5000), (96, 2049), (128, 5000), (64, 1), (128, 256)])
def test_count_pass_equals_brute_force_and_the_fill_is_the_ball(bits, n):
    """radius, n_ball, n_less for every query and k of the case against NumPy; the fill's list, as a set, is ball(r*): each item
    once, each distance right; a second call, on another stream, gives equal bytes."""
    import cmh_native as Nv
    db, rB, _, tables = _case(bits, n)
    dw = U.pack(db)
    m = U.subs(bits)
    side = torch.cuda.Stream()
    for Q in QUERIES:
        q = K.queries(db, Q, seed=Q)
        qw = U.pack(q)
        qs = Nv.pack_codes(_t(U.codes(q)))[0].contiguous()
        d = np.stack([K.distances(row, dw, bits)[1] for row in qw])
        for k in _ks(n):
            for r_cap in sorted({0, 1, m, 3 * m - 1}):
                got = Nv.mih_knn_count(qs, tables.sign, bits, k, r_cap, tables.order, tables.starts)
                assert all(t.dtype == torch.int32 and t.shape == (Q,) for t in got)
                want = np.array([K.brute(row, k, r_cap) for row in d]).T
                for g, w in zip(got, want):
                    np.testing.assert_array_equal(g.cpu().numpy(), w)
                radius, n_ball, _ = got
                sizes = torch.where(radius >= 0, n_ball, torch.zeros_like(n_ball)).long()
                off = torch.zeros(Q + 1, dtype=torch.int64, device=DEV)
                torch.cumsum(sizes, 0, out=off[1:])
                T = int(off[-1])
                if T == 0:
                    continue
                idx, dist = Nv.mih_knn_fill(qs, tables.sign, bits, radius, tables.order, tables.starts, off, T)
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    again = Nv.mih_knn_fill(qs, tables.sign, bits, radius, tables.order, tables.starts, off, T)
                    recount = Nv.mih_knn_count(qs, tables.sign, bits, k, r_cap, tables.order, tables.starts)
                side.synchronize()
                _same(again, (idx, dist))
                _same(recount, got)
                idx, dist, off_h, rad = idx.cpu().numpy(), dist.cpu().numpy(), off.cpu().numpy(), radius.cpu().numpy()
                for i in range(Q):
                    own, own_d = idx[off_h[i]:off_h[i + 1]], dist[off_h[i]:off_h[i + 1]]
                    ball = np.nonzero(d[i] <= rad[i])[0]           # (radius -1: empty)
                    assert np.array_equal(np.sort(own), ball) and np.array_equal(own_d, d[i][own])


def test_fill_writes_nothing_outside_the_lists():
    """A radius below 0 or above 3 m - 1 is not walked; nothing lands at or behind min(offsets[q + 1], capacity)."""
    import cmh_native as Nv
    db, rB, _, tables = _case(64, 5000)
    qs = Nv.pack_codes(_t(U.codes(K.queries(db, 65, seed=5))))[0].contiguous()
    radius, n_ball, _ = Nv.mih_knn_count(qs, tables.sign, 64, 7, 11, tables.order, tables.starts)
    keep = torch.nonzero(radius >= 0).squeeze(1)[:5]               # five queries whose ball holds 7 items within 11 bits
    assert keep.numel() == 5
    qs, radius, n_ball = qs[keep].contiguous(), radius[keep].contiguous(), n_ball[keep]
    walk = radius.clone()
    walk[1], walk[3] = -1, 12                                      # not walked: their slots stay as they were
    off = torch.zeros(6, dtype=torch.int64, device=DEV)
    torch.cumsum(n_ball.long(), 0, out=off[1:])
    T = int(off[-1])
    cap = int(off[4]) + 1                                          # the last list is cut after one entry
    full = Nv.mih_knn_fill(qs, tables.sign, 64, radius, tables.order, tables.starts, off, T)
    lib, ptr = Nv.lib(), Nv.ptr
    idx = torch.full((T,), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((T,), -7, dtype=torch.int32, device=DEV)
    Nv.check(lib.cmh_mih_knn_fill(ptr(qs), 5, ptr(tables.sign), 5000, 64, ptr(walk), ptr(tables.order), ptr(tables.starts), ptr(off),
                                  cap, ptr(idx), ptr(dist), Nv.stream_ptr(qs.device)), "cmh_mih_knn_fill")
    o = off.cpu().tolist()
    for i in range(5):
        lo, hi = o[i], o[i + 1]
        if i in (1, 3):
            assert bool((idx[lo:hi] == -7).all()) and bool((dist[lo:hi] == -7).all())
        else:
            end = min(hi, cap)
            assert torch.equal(idx[lo:end], full[0][lo:end]) and torch.equal(dist[lo:end], full[1][lo:end])
            assert bool((idx[end:hi] == -7).all()) and bool((dist[end:hi] == -7).all())


def test_ties_at_the_stopping_radius_cross_a_round():
    """One code 700 times and more among 5 000 items: for the query equal to it ball(0) >= 700 > k, more than two rounds of 256
    candidates; the k entries are the k smallest indices among the copies."""
    from utils.retrieval import SubstringTables, hamming_topk
    import cmh_native as Nv
    rng = np.random.default_rng(70)
    db = K.draw(5000, 64, seed=71)
    code = db[0].copy()
    copies = np.sort(rng.choice(5000, size=700, replace=False))
    db[copies] = code
    copies = np.nonzero((db == code).all(1))[0]
    rB = _t(U.codes(db))
    tables = SubstringTables.build(Nv.pack_codes(rB), 64)
    qB = _t(U.codes(np.stack([code, K.flipped(rng, code[None], [1])[0], K.flipped(rng, code[None], [3])[0]])))
    assert copies.size >= 700
    for k in (1, 256, 257, 300, 699, 700, 701, 702):
        got = tables.topk(qB, k, max_ball=5000)
        _same(got, hamming_topk(qB, rB, k))
        assert got[0][0, :min(k, copies.size)].cpu().tolist() == copies[:k].tolist()
    assert tables_radius(tables, qB, 300).cpu().tolist() == [0, 1, 3]


def test_a_database_of_equal_codes():
    from utils.retrieval import SubstringTables, hamming_topk
    import cmh_native as Nv
    code = np.random.default_rng(80).integers(0, 2, size=(1, 96)).astype(np.uint8)
    rB = _t(U.codes(np.repeat(code, 1000, axis=0)))
    tables = SubstringTables.build(Nv.pack_codes(rB), 96)
    qB = _t(U.codes(np.concatenate([code, K.flipped(np.random.default_rng(81), np.repeat(code, 2, axis=0), [2, 17])])))
    qs = Nv.pack_codes(qB)[0].contiguous()
    for k in (1, 300, 1000):
        radius, n_ball, n_less = Nv.mih_knn_count(qs, tables.sign, 96, k, 17, tables.order, tables.starts)
        assert radius.cpu().tolist() == [0, 2, 17] and n_ball.cpu().tolist() == [1000] * 3 and n_less.cpu().tolist() == [0] * 3
        got = tables.topk(qB, k, max_ball=1000)
        _same(got, hamming_topk(qB, rB, k))
        assert got[0][0].cpu().tolist() == list(range(k))


def test_far_queries_and_small_caps_take_the_scan():
    """Nearest item beyond r_cap, k above |ball(r_cap)|, r_cap = 0 and 1 stated: radius -1, the scan's rows, the same bytes."""
    from utils.retrieval import hamming_topk
    db, rB, rL, tables = _case(64, 5000)
    rng = np.random.default_rng(90)
    far = rng.integers(0, 2, size=(4, 64)).astype(np.uint8)         # uniform: nothing within 11 bits of them
    q = np.concatenate([far[:2], K.queries(db, 5, seed=9), far[2:]])
    qB, qL = _t(U.codes(q)), _t(U.labels(9, 91))
    d = np.stack([K.distances(row, U.pack(db), 64)[1] for row in U.pack(q)])
    assert (d[[0, 1, 7, 8]].min(1) > 11).all()
    for k in (1, 7, 4000):                                         # 4000: above every ball within 11 bits
        want = hamming_topk(qB, rB, k, qL, rL)
        for caps in ({}, {"r_cap": 0}, {"r_cap": 1}, {"r_cap": 11, "max_ball": 5000}):
            _same(tables.topk(qB, k, qL, rL, **caps), want)
        radius = tables_radius(tables, qB, k).cpu().numpy()
        np.testing.assert_array_equal(radius, [K.brute(row, k, 11)[0] for row in d])
        assert (radius[[0, 1, 7, 8]] == -1).all() and ((radius[2:7] >= 0).all() if k == 1 else k == 7 or (radius == -1).all())
    for r_cap in (0, 1):
        got = tables_radius(tables, qB, 1, r_cap=r_cap).cpu().numpy()
        np.testing.assert_array_equal(got, [K.brute(row, 1, r_cap)[0] for row in d])
        assert got[2] == 0 and got[5] == -1                        # its own row; a row with 3 bits flipped


def test_max_ball_and_max_hits_do_not_change_a_byte(monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import hamming_topk
    db, rB, rL, tables = _case(32, 2049)
    q = K.queries(db, 65, seed=3)
    qB, qL = _t(U.codes(q)), _t(U.labels(65, 4))
    fills = []
    fill = Nv.mih_knn_fill
    monkeypatch.setattr(Nv, "mih_knn_fill", lambda *a: fills.append(int(a[-1])) or fill(*a))
    for k in (2, 300):
        want = hamming_topk(qB, rB, k, qL, rL)
        del fills[:]
        _same(tables.topk(qB, k, qL, rL, max_ball=0), want)        # every query on the scan route
        assert not fills
        _same(tables.topk(qB, k, qL, rL, max_ball=2049), want)     # every query the tables reach on theirs
        assert len(fills) == 1
        radius, n_ball, _ = Nv.mih_knn_count(Nv.pack_codes(qB)[0].contiguous(), tables.sign, 32, k, 5, tables.order, tables.starts)
        balls = n_ball[radius >= 0]
        total, widest = int(balls.sum()), int(balls.max())
        assert total == fills[0] and total > 3 * widest
        del fills[:]
        _same(tables.topk(qB, k, qL, rL, max_ball=2049, max_hits=widest), want)      # several groups, each within the budget
        assert len(fills) >= 3 and max(fills) <= widest and sum(fills) == total
        del fills[:]
        _same(tables.topk(qB, k, qL, rL, max_ball=2049, max_hits=widest - 1), want)  # the widest ball no longer fits: the scan
        assert sum(fills) < total


def test_query_blocks(monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import hamming_topk
    db, rB, rL, tables = _case(64, 2049)
    q = K.queries(db, 65, seed=6)
    qB, qL = _t(U.codes(q)), _t(U.labels(65, 7))
    want = hamming_topk(qB, rB, 7, qL, rL)
    monkeypatch.setattr(Nv, "QUERIES_MAX", 23)                     # three blocks of queries
    _same(tables.topk(qB, 7, qL, rL, max_ball=2049), want)


def test_search_tables_follows_add():
    from utils.retrieval import CodeIndex
    db, rB, rL, _ = _case(64, 2049)
    q = K.queries(db, 9, seed=8)
    qB, qL = _t(U.codes(q)), _t(U.labels(9, 10))
    index = CodeIndex(rB[:1200], rL[:1200])
    _same(index.search_tables(qB, 7, qL), index.search(qB, 7, qL))
    first = index.substrings()
    index.add(rB[1200:], rL[1200:])
    assert index.substrings() is not first and index.substrings().n == 2049
    for k in (1, 7, 300):
        _same(index.search_tables(qB, k, qL), index.search(qB, k, qL))
        _same(index.search_tables(qB, k), index.search(qB, k))
        _same(index.search_tables(qB, k, qL, max_ball=2049, r_cap=4, max_hits=5000), index.search(qB, k, qL))
    sharded = CodeIndex(rB, rL, shard_items=700)
    _same(sharded.search_tables(qB, 300, qL, max_ball=0), index.search(qB, 300, qL))


def test_refusals_name_the_limit_before_a_launch(monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import CodeIndex
    db, rB, rL, tables = _case(128, 256)
    qB = rB[:3]
    launched = []
    for name in ("mih_build", "mih_knn_count", "mih_knn_fill"):
        monkeypatch.setattr(Nv, name, lambda *a, _n=name, **k: launched.append(_n))
    zero = rB[:50].clone()
    zero[3, 5] = 0
    with pytest.raises(Nv.NativeError, match=r"0 entry.*range_search"):
        CodeIndex(zero).search_tables(qB, 3)
    wide = torch.cat([rB[:50], rB[:50, :1]], dim=1)
    with pytest.raises(Nv.NativeError, match=r"search_tables: 129-bit codes exceed BUCKET_BITS_MAX = 128"):
        CodeIndex(wide).search_tables(wide[:2], 3)
    index = CodeIndex(rB[:50])
    for args, kwargs, text in (((qB, 0), {}, r"k=0 outside \[1, N=50\]"), ((qB, 51), {}, r"k=51 outside \[1, N=50\]"),
                               ((qB[:, :64], 3), {}, r"64-bit queries for an index of 128 bits"),
                               ((qB, 3, torch.ones(3, 5)), {}, r"query labels given, but the index has none"),
                               ((qB, 3), {"r_cap": 24}, r"r_cap=24 .*\[0, 23\]"), ((qB, 3), {"max_ball": -1}, r"max_ball=-1")):
        with pytest.raises(Nv.NativeError, match=text):
            index.search_tables(*args, **kwargs)
    with pytest.raises(TypeError, match=r"unknown option 'radius'"):
        index.search_tables(qB, 3, radius=4)
    assert not launched
    zq = qB.clone()
    zq[0, 0] = 0
    with pytest.raises(Nv.NativeError, match=r"a query with a 0 entry"):
        tables.topk(zq, 3)
    assert not launched


def test_retrieve_cli_tables_prints_the_plain_lines(tmp_path, capsys):
    import scipy.io as scio
    import retrieve
    from utils.retrieval import CodeIndex
    db, q = U.case(64)
    rB, qB = U.codes(db[:3000]), U.codes(q)
    rL, qL = U.labels(3000, 1), U.labels(11, 2)
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB[::-1].copy(), "r_img": rB[::-1].copy(), "r_txt": rB, "q_l": qL, "r_l": rL})
    CodeIndex(_t(rB), _t(rL)).save(tmp_path / "db.npz")
    for extra in ([], ["--index", str(tmp_path / "db.npz")]):
        base = ["--codes", str(mat), "--direction", "i2t", "--queries", "0:11", "--k", "12"] + extra
        assert retrieve.main(base) == 0
        want = capsys.readouterr().out
        assert retrieve.main(base + ["--tables"]) == 0
        got = capsys.readouterr().out
        assert got == want and len(got.splitlines()) == 11 and got.count(":") == 11 * 12 * 2
