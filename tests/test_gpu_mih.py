"""Multi-index hashing on the GPU (csrc/retrieval_mih.hip: cmh_mih_build, cmh_mih_count / _fill; utils/retrieval.py::SubstringTables,
CodeIndex.substrings / lookup_far / near_duplicates; retrieve.py --near) against the scan (hamming_range / range_search /
duplicates) and, below 3 bits, the bucket table.  Everything is an integer, an index or a whole-bit distance: every comparison is
exact."""
import numpy as np
import pytest
import torch

import mihutil as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


_cases = {}


def _case(bits):
    """-> (rB, rL, qB, qL on the GPU, the case's SubstringTables), made once per code length."""
    from utils.retrieval import SubstringTables
    import cmh_native as Nv
    if bits not in _cases:
        db, q = U.case(bits)
        rB, qB = _t(U.codes(db)), _t(U.codes(q))
        _cases[bits] = (rB, _t(U.labels(db.shape[0], bits + 1)), qB, _t(U.labels(q.shape[0], bits + 2)),
                        SubstringTables.build(Nv.pack_codes(rB), bits))
    return _cases[bits]


_wanted = {}


def _want(bits, r):
    """hamming_range's tuple with labels for a case and radius, computed once."""
    from utils.retrieval import hamming_range
    if (bits, r) not in _wanted:
        rB, rL, qB, qL, _ = _case(bits)
        _wanted[bits, r] = hamming_range(qB, rB, r, qL, rL)
    return _wanted[bits, r]


@pytest.mark.parametrize("bits,r", U.POINTS)
def test_lookup_equals_the_scan(bits, r):
    from utils.retrieval import CodeIndex
    rB, rL, qB, qL, tables = _case(bits)
    want = _want(bits, r)
    got = tables.lookup(qB, r, qL, rL)
    assert len(got) == 4 and int(got[0][-1]) > 0
    _same(got, want)
    _same(tables.lookup(qB, r), want[:3])
    _same(tables.lookup(qB, r, qL, rL), got)                       # a second call: equal bytes
    ref = U.brute(U.pack(U.case(bits)[1]), U.pack(U.case(bits)[0]), bits, r)      # ... and the scan is the brute force
    np.testing.assert_array_equal(got[0].cpu().numpy(), np.concatenate([[0], np.cumsum([i.size for i, _ in ref])]))
    np.testing.assert_array_equal(got[1].cpu().numpy(), np.concatenate([i for i, _ in ref]))
    np.testing.assert_array_equal(got[2].cpu().numpy(), np.concatenate([d for _, d in ref]).astype(np.float32))
    if r <= 2:
        _same(CodeIndex(rB, rL).lookup(qB, r, qL), got)


@pytest.mark.parametrize("bits,r", [(24, 3), (64, 4), (64, 11), (128, 16)])
def test_the_walk_gives_equal_bytes_and_every_item_once(bits, r):
    """The kernels' own output, before the sort: two calls agree byte for byte, and a query's list holds no item twice."""
    import cmh_native as Nv
    _, _, qB, _, tables = _case(bits)
    qs = Nv.pack_codes(qB)[0].contiguous()
    hits = Nv.mih_count(qs, tables.sign, bits, r, tables.order, tables.starts)
    assert hits.dtype == torch.int32 and torch.equal(hits.long(), _want(bits, r)[0].diff())
    off = torch.zeros(hits.numel() + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(hits, 0, out=off[1:])
    T = int(off[-1])
    first = Nv.mih_fill(qs, tables.sign, bits, r, tables.order, tables.starts, off, T)
    again = Nv.mih_fill(qs, tables.sign, bits, r, tables.order, tables.starts, off, T)
    _same(first, again)
    assert torch.equal(hits, Nv.mih_count(qs, tables.sign, bits, r, tables.order, tables.starts))
    query = torch.repeat_interleave(torch.arange(hits.numel(), device=DEV), hits.long())
    assert torch.unique(query * tables.n + first[0].long()).numel() == T


def _garbage_planes(bits, seed):
    """The case's planes with random bits ORed in behind `bits` of the sign plane (they must not matter)."""
    import cmh_native as Nv
    db = U.case(bits)[0]
    sign, nz = Nv.pack_codes(_t(U.codes(db)))
    words = U.pack(db, garbage_seed=seed)
    assert bits % 32 == 0 or (words != U.pack(db)).any()
    return (_t(words.view(np.int32)), nz), words


@pytest.mark.parametrize("bits", [24, 64])
def test_table_invariants(bits):
    from utils.retrieval import SubstringTables
    planes, words = _garbage_planes(bits, seed=9)
    tables = SubstringTables.build(planes, bits)
    n, m = words.shape[0], U.subs(bits)
    assert (tables.n, tables.m, tables.bits, tables.max_radius) == (n, m, bits, 3 * m - 1)
    assert tables.order.dtype == torch.int32 and tuple(tables.order.shape) == (m, n)
    assert tables.starts.dtype == torch.int32 and tuple(tables.starts.shape) == (m, 65537)
    order, starts = tables.order.cpu().numpy(), tables.starts.cpu().numpy()
    for j in range(m):
        s = U.sub_width(bits, j)
        key = ((words[:, j // 2] >> np.uint32(16 * (j % 2))) & np.uint32((1 << s) - 1)).astype(np.int64)
        np.testing.assert_array_equal(np.sort(order[j]), np.arange(n))                       # a permutation
        np.testing.assert_array_equal(order[j], np.lexsort((np.arange(n), key)))             # by (key, index)
        assert starts[j, 0] == 0 and starts[j, -1] == n and (np.diff(starts[j]) >= 0).all()
        np.testing.assert_array_equal(starts[j], np.searchsorted(key[order[j]], np.arange(65537), side="left"))
        assert (starts[j, 1 << s:] == n).all()                                               # keys >= 2^s: empty
    again = SubstringTables.build(planes, bits)
    assert torch.equal(again.order, tables.order) and torch.equal(again.starts, tables.starts)
    if bits == 24:                                                 # the lookup cuts the garbage too
        _, _, qB, _, clean = _case(bits)
        for r in U.CASE[bits][4]:
            _same(tables.lookup(qB, r), clean.lookup(qB, r))


def _random_codes(rng, n, bits):
    return (rng.integers(0, 2, size=(n, bits)) * 2 - 1).astype(np.float32)


def _flipped(rng, rows, flips):
    out = rows.copy()
    for i in range(out.shape[0]):
        out[i, rng.choice(out.shape[1], size=flips[i % len(flips)], replace=False)] *= -1
    return out


@pytest.mark.parametrize("n", [1, 65])
def test_tiny_databases(n):
    """n = 1, and n = 65: a lane past a wave (all 65 items share substring 0: one bucket of 65)."""
    from utils.retrieval import CodeIndex, hamming_range
    rng = np.random.default_rng(n)
    rB = _random_codes(rng, n, 64)
    rB[:, :16] = rB[0, :16]
    qB = np.concatenate([_flipped(rng, rB[:min(n, 5)], [0, 1, 4, 5, 11]), _random_codes(rng, 2, 64)])
    index = CodeIndex(_t(rB))
    for r in (0, 4, 11):
        _same(index.lookup_far(_t(qB), r), hamming_range(_t(qB), _t(rB), r))
    assert int(index.lookup_far(_t(qB), 11)[0][-1]) >= min(n, 5)


def test_one_bucket_of_three_thousand():
    """3 000 copies of one code and 37 others: a bucket of 3 000 items in every table; the query equal to the code gets them all at
    distance 0, each once (through substring 0)."""
    from utils.retrieval import CodeIndex, hamming_range
    rng = np.random.default_rng(30)
    code = _random_codes(rng, 1, 64)
    rB = np.concatenate([np.repeat(code, 3000, axis=0), _random_codes(rng, 37, 64)])[rng.permutation(3037)]
    qB = np.concatenate([code, _flipped(rng, np.repeat(code, 4, axis=0), [1, 3, 8, 12])])
    index = CodeIndex(_t(rB))
    copies = np.nonzero((rB == code).all(1))[0]
    for r in (0, 3, 4, 8, 11):
        got = index.lookup_far(_t(qB), r)
        _same(got, hamming_range(_t(qB), _t(rB), r))
        assert int(got[0][1]) == 3000 and got[1][:3000].cpu().tolist() == copies.tolist() and not got[2][:3000].any()
    assert index.lookup_far(_t(qB), 11)[0].diff().cpu().tolist() == [3000, 3000, 3000, 3000, 0]


@pytest.mark.parametrize("r", [4, 8])
def test_constant_first_substring(r):
    """Substring 0 is the same in every item, the others are random: every item is a candidate of table 0."""
    from utils.retrieval import CodeIndex, hamming_range
    rng = np.random.default_rng(40)
    rB = _random_codes(rng, 2500, 64)
    rB[:, :16] = rB[0, :16]
    qB = np.concatenate([_flipped(rng, rB[:9], [0, 1, 3, 4, 5, 7, 8, 9, 2]), _random_codes(rng, 2, 64)])
    qB[1, 0] *= -1                                                 # ... and of its neighbours' buckets
    index = CodeIndex(_t(rB))
    assert int(index.substrings().starts[0].diff().max()) == 2500
    got = index.lookup_far(_t(qB), r)
    _same(got, hamming_range(_t(qB), _t(rB), r))
    assert int(got[0][-1]) >= 5


@pytest.mark.parametrize("Q", [1, 130])
def test_query_counts(Q):
    from utils.retrieval import hamming_range
    rB, rL, _, _, tables = _case(32)
    rng = np.random.default_rng(Q)
    qB = _flipped(rng, U.codes(U.case(32)[0][:Q]), [0, 2, 1, 6, 3])
    qL = _t(U.labels(Q, 77))
    for r in (2, 5):
        _same(tables.lookup(_t(qB), r, qL, rL), hamming_range(_t(qB), rB, r, qL, rL))


def test_no_hit_at_all():
    from utils.retrieval import hamming_range
    rB, rL, _, _, tables = _case(64)
    qB = _t(_random_codes(np.random.default_rng(50), 7, 64))
    qL = _t(U.labels(7, 51))
    got = tables.lookup(qB, 3, qL, rL)
    _same(got, hamming_range(qB, rB, 3, qL, rL))
    assert torch.equal(got[0], torch.zeros(8, dtype=torch.int64, device=DEV))
    assert [t.dtype for t in got[1:]] == [torch.int32, torch.float32, torch.uint8] and all(t.shape == (0,) for t in got[1:])
    assert len(tables.lookup(qB, 3)) == 3


def test_max_hits_one_below_is_refused_before_the_fill(monkeypatch):
    import cmh_native as Nv
    rB, _, qB, _, tables = _case(64)
    T = int(_want(64, 4)[0][-1])
    _same(tables.lookup(qB, 4, max_hits=T), _want(64, 4)[:3])
    filled = []
    monkeypatch.setattr(Nv, "mih_fill", lambda *a, **k: filled.append(a))
    with pytest.raises(Nv.NativeError, match=rf"T={T} hits exceed max_hits={T - 1}"):
        tables.lookup(qB, 4, max_hits=T - 1)
    assert not filled


def test_lookup_far_equals_range_search_and_the_tables_follow_add():
    from utils.retrieval import CodeIndex
    rB, rL, qB, qL, _ = _case(40)
    index = CodeIndex(rB[:1700], rL[:1700])
    first = index.substrings()
    assert index.substrings() is first                             # kept between calls
    for r in U.CASE[40][4]:
        _same(index.lookup_far(qB, r, qL), index.range_search(qB, r, qL))
        _same(index.lookup_far(qB, r), index.range_search(qB, r))
    index.add(rB[1700:], rL[1700:])
    assert index.substrings() is not first and index.substrings().n == rB.shape[0]
    for r in U.CASE[40][4]:
        _same(index.lookup_far(qB, r, qL), _want(40, r))
        _same(index.lookup_far(qB, r, qL), index.range_search(qB, r, qL))


@pytest.mark.parametrize("bits", [32, 64])
def test_near_duplicates_equal_duplicates(bits, monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import CodeIndex
    rB, rL, _, _, _ = _case(bits)
    for labels in (rL, None):
        index = CodeIndex(rB, labels)
        for r in (0, 3, 5):
            want = index.duplicates(r)
            assert len(want) == (3 if labels is None else 4) and int(want[0][-1]) > 0
            _same(index.near_duplicates(r), want)
    monkeypatch.setattr(Nv, "QUERIES_MAX", 7001)                   # the index against itself in three blocks of queries
    want = index.duplicates(3)
    _same(index.near_duplicates(3), want)
    T = int(want[0][-1]) + index.size                              # max_hits bounds the lists before the own entries leave
    _same(index.near_duplicates(3, max_hits=T), want)
    with pytest.raises(Nv.NativeError, match=rf"hits exceed max_hits={T - 1}"):
        index.near_duplicates(3, max_hits=T - 1)


def test_refusals_name_the_limit_before_a_launch(monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import CodeIndex, SubstringTables
    rB, _, qB, _, _ = _case(128)
    launched = []
    for name in ("mih_build", "mih_count", "mih_fill"):
        monkeypatch.setattr(Nv, name, lambda *a, _n=name, **k: launched.append(_n))
    zero = rB[:50].clone()
    zero[3, 5] = 0
    with pytest.raises(Nv.NativeError, match=r"0 entry.*range_search"):
        CodeIndex(zero).substrings()
    with pytest.raises(Nv.NativeError, match=r"0 entry.*range_search"):
        CodeIndex(zero).lookup_far(qB, 4)
    with pytest.raises(Nv.NativeError, match=r"0 entry.*range_search"):
        CodeIndex(zero).near_duplicates(4)
    wide = torch.cat([rB[:50], rB[:50, :1]], dim=1)
    with pytest.raises(Nv.NativeError, match=r"lookup_far: .*129-bit codes .*BUCKET_BITS_MAX = 128.*range_search"):
        CodeIndex(wide).lookup_far(wide[:2], 4)
    with pytest.raises(Nv.NativeError, match=r"129-bit codes exceed BUCKET_BITS_MAX = 128 \(range_search"):
        SubstringTables.build(Nv.pack_codes(wide), 129)
    index = CodeIndex(rB[:50])
    with pytest.raises(Nv.NativeError, match=r"lookup_far: .*radius=24 .*\[0, 23\].*range_search takes any radius"):
        index.lookup_far(qB, 24)
    with pytest.raises(Nv.NativeError, match=r"near_duplicates: .*radius=24 .*\[0, 23\]"):
        index.near_duplicates(24)
    with pytest.raises(Nv.NativeError, match=r"radius=0.5 .*whole number"):
        index.lookup_far(qB, 0.5)
    with pytest.raises(Nv.NativeError, match=r"64-bit queries for an index of 128 bits"):
        index.lookup_far(qB[:, :64], 4)
    with pytest.raises(Nv.NativeError, match=r"query labels given, but the index has none"):
        index.lookup_far(qB, 4, torch.ones(11, 5))
    assert not launched
    monkeypatch.undo()
    index.substrings()
    for name in ("mih_count", "mih_fill"):
        monkeypatch.setattr(Nv, name, lambda *a, _n=name, **k: launched.append(_n))
    zq = qB.clone()
    zq[0, 0] = 0
    with pytest.raises(Nv.NativeError, match=r"a query with a 0 entry"):
        index.lookup_far(zq, 4)
    assert not launched


def test_retrieve_cli_near_prints_radius_lines(tmp_path, capsys):
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
        base = ["--codes", str(mat), "--direction", "i2t", "--queries", "0:11"] + extra
        assert retrieve.main(base + ["--radius", "4"]) == 0
        want = capsys.readouterr().out
        assert retrieve.main(base + ["--near", "4"]) == 0
        got = capsys.readouterr().out
        assert got == want and len(got.splitlines()) == 11 and got.count(":") > 20
    with pytest.raises(SystemExit, match=r"--near: .*radius=12 .*\[0, 11\]"):
        retrieve.main(["--codes", str(mat), "--near", "12"])
