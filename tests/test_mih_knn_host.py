"""CPU checks of the k-nearest search through the substring tables: the growth rule itself (utils.retrieval.knn_steps walked in NumPy
by tests/mihknnutil.py against brute force, for every query and every k), that the entry points are declared and bound, the
argument checks of cmh_mih_knn_count / _fill (nothing is launched, so no GPU is needed), the Python layer's refusals and the
--tables flag of retrieve.py."""
import os

import numpy as np
import pytest

import mihknnutil as K
import mihutil as U

NEW = ("cmh_mih_knn_count", "cmh_mih_knn_fill")
BITS = (1, 5, 16, 24, 64)


def _databases(bits):
    """Small databases (N <= 300) and their queries as packed words: a random one, one that is a few codes repeated many times."""
    rng = np.random.default_rng(bits)
    out = []
    for n, distinct in ((300, None), (257, 5), (1, None)):
        db = rng.integers(0, 2, size=(n, bits)).astype(np.uint8)
        if distinct is not None:
            db = K.flipped(rng, db[:distinct], [0, 1])[rng.integers(0, distinct, size=n)]
        q = np.concatenate([K.flipped(rng, db[:min(n, 6)], [0, 1, 2, 3, 5, 9]), rng.integers(0, 2, size=(2, bits)).astype(np.uint8)])
        out.append((U.pack(q), U.pack(db)))
    return out


@pytest.mark.parametrize("bits", BITS)
def test_steps_probe_exactly_the_substring_radii(bits):
    from utils.retrieval import knn_steps, substring_radii
    m = U.subs(bits)
    steps = knn_steps(bits, 3 * m - 1)
    assert steps == [(s % m, s // m) for s in range(3 * m)] and len(set(steps)) == 3 * m
    for r in range(3 * m):
        assert knn_steps(bits, r) == steps[:r + 1]
        levels = [[t for j, t in steps[:r + 1] if j == sub] for sub in range(m)]
        assert all(ls == list(range(len(ls))) for ls in levels)                    # every level up to the radius, each once, ascending
        assert [len(ls) - 1 for ls in levels] == substring_radii(bits, r) == U.radii(bits, r)


@pytest.mark.parametrize("bits", BITS)
def test_rule_emits_each_item_of_the_ball_once_and_stops_where_brute_force_does(bits):
    from utils.retrieval import knn_steps
    m = U.subs(bits)
    seen_stop = seen_cap = 0
    for r_cap in sorted({0, m - 1, 3 * m - 1}):
        steps = knn_steps(bits, r_cap)
        for qw, dw in _databases(bits):
            n = dw.shape[0]
            for q in qw:
                dj, d = K.distances(q, dw, bits)
                reached = K.walk(dj, d, steps, r_cap)
                for r in range(r_cap + 1):                                         # after step r: ball(r) is there, nothing twice
                    sofar = np.concatenate(reached[:r + 1])
                    assert np.unique(sofar).size == sofar.size
                    assert np.array_equal(np.sort(sofar[d[sofar] <= r]), np.nonzero(d <= r)[0])
                for k in range(1, n + 1):
                    got, want = K.stop(d, reached, k, r_cap), K.brute(d, k, r_cap)
                    assert got == want, (bits, r_cap, n, k, got, want)
                    if got[0] >= 0:                                                # what the fill pass emits: ball(r*), each item once
                        emitted = np.concatenate(reached[:got[0] + 1])
                        emitted = emitted[d[emitted] <= got[0]]
                        assert emitted.size == got[1] >= k > got[2] and np.unique(emitted).size == emitted.size
                        seen_stop += 1
                    else:
                        assert got[1] == got[2] < k
                        seen_cap += 1
    assert seen_stop > 0 and (seen_cap > 0 or bits == 1)


def test_the_uniqueness_test_matters():
    """Without the first-reach test an item is counted through every substring that reaches it."""
    from utils.retrieval import knn_steps
    bits, twice = 64, 0
    steps = knn_steps(bits, 11)
    for qw, dw in _databases(bits):
        for q in qw:
            dj, d = K.distances(q, dw, bits)
            loose = np.concatenate([np.nonzero((dj[j] == t) & (d <= 11))[0] for j, t in steps])
            twice += loose.size - np.unique(loose).size
    assert twice > 0


def test_knn_steps_refuses_by_name():
    import cmh_native as N
    from utils.retrieval import knn_steps
    assert knn_steps(64, 0) == [(0, 0)] and knn_steps(16, 2) == [(0, 0), (0, 1), (0, 2)]
    assert knn_steps(24, 5) == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    for bits, r_cap, text in ((64, 12, r"knn_steps: .*r_cap=12 .*\[0, 11\]"), (16, 3, r"r_cap=3 .*\[0, 2\]"), (64, -1, r"r_cap=-1 "),
                              (64, 1.5, r"r_cap=1.5 .*whole number"), (129, 1, r"129-bit codes"), (0, 0, r"0-bit codes")):
        with pytest.raises(N.NativeError, match=text):
            knn_steps(bits, r_cap)


def test_entry_points_are_declared_and_bound():
    import cmh_native as N
    from conftest import ROOT
    assert set(NEW) <= set(N.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in NEW:
        assert f"int {name}(" in header and hasattr(N.lib(), name)
    assert callable(N.mih_knn_count) and callable(N.mih_knn_fill)
    assert N.ABI_VERSION == 6 and N.lib().cmh_version() == 6


def test_argument_checks_run_before_any_launch():
    """Null operands, Q, N, bits, k, r_cap outside their limits, misaligned offsets and rows, capacity 0: each comes back -1 with a
    message that names the limit.  Non-null pointers are needed to reach the size checks: a host buffer serves, nothing reads it."""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    buf = (C.c_int64 * 8)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    count = lambda q=p, Q=4, db=p, n=10, bits=64, k=3, r_cap=4, order=p, starts=p, radius=p, ball=p, less=p: \
        lib.cmh_mih_knn_count(q, Q, db, n, bits, k, r_cap, order, starts, radius, ball, less, None)
    fill = lambda q=p, Q=4, db=p, n=10, bits=64, radius=p, order=p, starts=p, off=p, cap=5, idx=p, dist=p: \
        lib.cmh_mih_knn_fill(q, Q, db, n, bits, radius, order, starts, off, cap, idx, dist, None)
    cases = []
    for name, call in (("mih_knn_count", count), ("mih_knn_fill", fill)):
        cases += [
            (lambda call=call: call(q=None), name.encode() + b": null"), (lambda call=call: call(db=None), b"null"),
            (lambda call=call: call(order=None), b"null"), (lambda call=call: call(starts=None), b"null"),
            (lambda call=call: call(radius=None), b"null"),
            (lambda call=call: call(Q=0), b"Q=0 outside [1, 65535]"), (lambda call=call: call(Q=65536), b"Q=65536 outside [1, 65535]"),
            (lambda call=call: call(n=0), b"N=0 outside [1, 2^31 - 1]"), (lambda call=call: call(n=2 ** 31), b"outside [1, 2^31 - 1]"),
            (lambda call=call: call(bits=0), b"bits=0 outside [1, 128]"), (lambda call=call: call(bits=129), b"bits=129 outside [1, 128]"),
            (lambda call=call: call(db=odd), b"aligned to 8 bytes"), (lambda call=call: call(db=odd, bits=128), b"aligned to 16 bytes"),
        ]
    cases += [(lambda: count(ball=None), b"null"), (lambda: count(less=None), b"null"),
              (lambda: count(k=0), b"k=0 outside [1, N=10]"), (lambda: count(k=11), b"k=11 outside [1, N=10]"),
              (lambda: count(r_cap=12), b"r_cap=12 outside [0, 11]"), (lambda: count(r_cap=-1), b"r_cap=-1 below 0"),
              (lambda: count(bits=16, r_cap=3), b"r_cap=3 outside [0, 2]"), (lambda: count(bits=24, r_cap=6), b"r_cap=6 outside [0, 5]"),
              (lambda: count(bits=128, r_cap=24), b"r_cap=24 outside [0, 23]"),
              (lambda: fill(off=None), b"null"), (lambda: fill(idx=None), b"null"), (lambda: fill(dist=None), b"null"),
              (lambda: fill(cap=0), b"capacity=0 below 1"), (lambda: fill(off=odd), b"offsets holds 64-bit integers: aligned to 8 bytes")]
    for i, (call, text) in enumerate(cases):
        rc = call()
        assert rc == -1, (i, rc, lib.cmh_last_error())
        assert text in lib.cmh_last_error(), (i, lib.cmh_last_error())


def test_python_layer_refuses_by_name_before_anything_is_packed():
    """SubstringTables over CPU tensors: every refusal below comes before the first tensor is moved or packed."""
    import torch
    import cmh_native as N
    from utils.retrieval import MAX_HITS_TOPK, SubstringTables, _check_topk
    n, bits = 40, 64
    tables = SubstringTables(torch.zeros(4, n, dtype=torch.int32), torch.zeros(4, 65537, dtype=torch.int32),
                             torch.zeros(n, 2, dtype=torch.int32), bits, n)
    q = torch.ones(3, bits)
    for kwargs, text in ((dict(k=0), r"topk: k=0 outside \[1, N=40\]"), (dict(k=41), r"k=41 outside \[1, N=40\]"),
                         (dict(k=2.5), r"k=2.5 outside"), (dict(k=True), r"k=True outside"),
                         (dict(k=3, r_cap=12), r"r_cap=12 .*\[0, 11\]"), (dict(k=3, r_cap=-1), r"r_cap=-1 "),
                         (dict(k=3, r_cap=0.5), r"r_cap=0.5 .*whole number"), (dict(k=3, max_ball=-1), r"max_ball=-1.*below 0"),
                         (dict(k=3, max_hits=-5), r"max_hits=-5: below 0"),
                         (dict(k=3, query_labels=torch.ones(3, 5)), r"labels on one side only"),
                         (dict(k=3, retrieval_L=torch.ones(n, 5)), r"labels on one side only"),
                         (dict(k=3, query_labels=torch.ones(3, 5), retrieval_L=torch.ones(n + 1, 5)), r"labels of 41 items for tables of 40")):
        with pytest.raises(N.NativeError, match=text):
            tables.topk(q, **kwargs)
    with pytest.raises(N.NativeError, match=r"32-bit queries for an index of 64 bits"):
        tables.topk(q[:, :32], 3)
    assert _check_topk("t", bits, n, bits, 3, None, None, None) == (11, n // 64, MAX_HITS_TOPK) and MAX_HITS_TOPK == 2 ** 28
    with pytest.raises(N.NativeError, match=r"129-bit codes exceed BUCKET_BITS_MAX = 128"):
        _check_topk("t", 129, n, 129, 3, None, None, None)
    sign = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.mih_knn_count(sign, sign, 64, 2, 4, torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 65537, dtype=torch.int32))
    with pytest.raises(N.NativeError, match="GPU only"):
        N.mih_knn_fill(sign, sign, 64, torch.zeros(4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.int32),
                       torch.zeros(4, 65537, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), 1)


def test_retrieve_tables_flag(capsys):
    import retrieve
    args = retrieve.parse(["--codes", "x.mat", "--k", "5", "--tables"])
    assert args.tables and args.k == 5
    assert not retrieve.parse(["--codes", "x.mat", "--k", "5"]).tables
    assert retrieve.parse(["--codes", "x.mat", "--tables", "--index", "db.npz", "--direction", "t2i", "--queries", "0:5"]).tables
    asked = ["--text", "a dog", "--index", "db.npz", "--method", "DSPH", "--pretrained", "m.pth", "-clip-path", "c.pt", "--output-dim", "64"]
    assert retrieve.parse(asked + ["--tables", "--k", "3"]).tables
    refused = [(["--graded"], "--graded"), (["--radius", "1"], "--radius"), (["--lookup", "1"], "--lookup"), (["--near", "4"], "--near"),
               (["--map"], "--map"), (["--recall"], "--recall"), (["--stats"], "--stats"), (["--bucket-stats"], "--bucket-stats")]
    refused += [(["--index", "db.npz", flag, "1"], flag) for flag in retrieve.FILTERS]
    for extra, flag in refused:
        with pytest.raises(SystemExit) as e:
            retrieve.parse(["--codes", "x.mat", "--tables"] + extra)
        assert e.value.code == 2 and f"--tables and {flag} exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        retrieve.parse(asked + ["--tables", "--soft"])
    assert e.value.code == 2 and "--tables and --soft exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                           # the existing flags keep their messages
        retrieve.parse(["--codes", "x.mat", "--near", "4", "--k", "5"])
    assert e.value.code == 2 and "--near and --k exclude each other" in capsys.readouterr().err
