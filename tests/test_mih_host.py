"""CPU checks of multi-index hashing on 16-bit substrings: the rule itself (tests/mihutil.py's NumPy restatement against brute force
on every case and radius, that the cases are populated, and that each part of the rule matters), utils.retrieval.substring_radii,
the argument checks of the four entry points of csrc/retrieval_mih.hip (nothing is launched, so no GPU is needed) and the --near
flag of retrieve.py."""
import os

import numpy as np
import pytest

import mihutil as U

NEW = ("cmh_mih_build_workspace_bytes", "cmh_mih_build", "cmh_mih_count", "cmh_mih_fill")


def _packed(bits, garbage_seed=None):
    db, q = U.case(bits)
    return U.pack(q, garbage_seed), U.pack(db, None if garbage_seed is None else garbage_seed + 1)


def test_substring_radii_against_a_hand_table():
    import cmh_native as N
    from utils.retrieval import substring_radii
    table = {(64, 4): [1, 0, 0, 0], (24, 0): [0, -1], (128, 23): [2] * 8, (16, 0): [0], (16, 2): [2], (24, 1): [0, 0], (24, 3): [1, 1],
             (24, 5): [2, 2], (32, 2): [1, 0], (40, 2): [0, 0, 0], (40, 3): [1, 0, 0], (40, 8): [2, 2, 2], (64, 0): [0, -1, -1, -1],
             (64, 3): [0, 0, 0, 0], (64, 7): [1, 1, 1, 1], (64, 8): [2, 1, 1, 1], (64, 11): [2, 2, 2, 2], (128, 7): [0] * 8,
             (128, 8): [1] + [0] * 7, (128, 15): [1] * 8, (128, 16): [2] + [1] * 7, (1, 2): [2], (17, 5): [2, 2], (113, 9): [1, 1] + [0] * 6}
    for (bits, r), want in table.items():
        got = substring_radii(bits, r)
        assert got == want and got == U.radii(bits, r), (bits, r, got)
        assert sum(a + 1 for a in got) == r + 1                    # the pigeonhole count: every probed substring beaten costs a_j + 1 bits
    for bits, r in U.POINTS:
        assert substring_radii(bits, r) == U.radii(bits, r)
    for bits, r, text in ((16, 3, r"radius=3 .*\[0, 2\].*range_search takes any radius"), (32, 6, r"radius=6 .*\[0, 5\]"),
                          (64, 12, r"radius=12 .*\[0, 11\]"), (128, 24, r"radius=24 .*\[0, 23\].*range_search takes any radius"),
                          (64, -1, r"radius=-1 "), (64, 2.5, r"radius=2.5 .*whole number"), (64, True, r"radius=True"),
                          (129, 1, r"129-bit codes .*BUCKET_BITS_MAX = 128.*range_search"), (0, 0, r"0-bit codes")):
        with pytest.raises(N.NativeError, match=text):
            substring_radii(bits, r)


@pytest.mark.parametrize("bits,r", U.POINTS)
def test_rule_equals_brute_force_and_emits_nothing_twice(bits, r):
    qw, dw = _packed(bits)
    want = U.brute(qw, dw, bits, r)
    got = U.rule(qw, dw, bits, r)
    for idx, _ in got:
        assert np.unique(idx).size == idx.size
    assert U.same(U.ordered(got), want)


@pytest.mark.parametrize("bits,r", U.POINTS)
def test_cases_are_populated(bits, r):
    """Every (case, radius) has a query with an empty list, one with at least two hits at distance exactly r, and hits at all."""
    qw, dw = _packed(bits)
    lists = U.brute(qw, dw, bits, r)
    assert qw.shape[0] == 11 and dw.shape[0] == U.CASE[bits][1]
    assert any(idx.size == 0 for idx, _ in lists)
    assert any(int((d == r).sum()) >= 2 for _, d in lists)
    assert sum(idx.size for idx, _ in lists) > 0
    if (bits, r) == (64, 0):
        assert sum(int((d == r).sum()) >= 2 for _, d in lists) == 1 and sum(idx.size for idx, _ in lists) == 5


def test_cases_cover_the_rule():
    """The radii sit on every change of (a, b); substrings go unprobed; a short last substring occurs probed and unprobed."""
    seen = {(bits, r): U.radii(bits, r) for bits, r in U.POINTS}
    assert {tuple(seen[64, r]) for r in (3, 4, 7, 8, 11)} == {(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 1, 1), (2, 1, 1, 1), (2, 2, 2, 2)}
    assert seen[128, 7] == [0] * 8 and seen[128, 8][:2] == [1, 0] and seen[128, 16][:2] == [2, 1] and seen[128, 23] == [2] * 8
    assert any(-1 in a for a in seen.values())
    assert [U.sub_width(24, j) for j in range(2)] == [16, 8] and [U.sub_width(40, j) for j in range(3)] == [16, 16, 8]
    assert seen[24, 0][-1] == -1 and seen[24, 3][-1] == 1 and seen[40, 2][-1] == 0 and seen[40, 8][-1] == 2


def test_each_part_of_the_rule_matters():
    """Dropping the exactly-once rule emits items twice; a_j = a - 1 everywhere misses items; ignoring the width of the short last
    substring (taking 16 bits of the word, whatever lies behind `bits`) changes the lists."""
    twice = misses = 0
    for bits, r in U.POINTS:
        qw, dw = _packed(bits)
        want = U.brute(qw, dw, bits, r)
        loose = U.rule(qw, dw, bits, r, once=False)
        twice += sum(idx.size - np.unique(idx).size for idx, _ in loose)
        a = r // U.subs(bits)
        low = U.rule(qw, dw, bits, r, sub_radii=[a - 1] * U.subs(bits))
        misses += sum(w[0].size - g[0].size for w, g in zip(want, low))
    assert twice > 0 and misses > 0
    changed = 0
    for bits in (24, 40):
        qw, dw = _packed(bits, garbage_seed=3)
        for r in U.CASE[bits][4]:
            want = U.brute(qw, dw, bits, r)
            assert U.same(want, U.brute(*_packed(bits), bits, r))                  # bits behind `bits` do not matter ...
            assert U.same(U.ordered(U.rule(qw, dw, bits, r)), want)
            changed += not U.same(U.ordered(U.rule(qw, dw, bits, r, cut_width=False)), want)      # ... unless the width is ignored
    assert changed > 0


def test_entry_points_are_declared_and_bound():
    import cmh_native as N
    from conftest import ROOT
    assert set(NEW) <= set(N.SIGNATURES)
    assert (N.MIH_SUB_BITS, N.MIH_SUB_RADIUS_MAX, N.BUCKET_BITS_MAX, N.BUCKET_RADIUS_MAX) == (16, 2, 128, 2)
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for macro, value in (("CMH_MIH_SUB_BITS", N.MIH_SUB_BITS), ("CMH_MIH_SUB_RADIUS_MAX", N.MIH_SUB_RADIUS_MAX)):
        assert f"#define {macro} {value}" in header
    assert N.ABI_VERSION == 6 and N.lib().cmh_version() == 6
    assert [N.mih_substrings(b) for b in (1, 16, 17, 24, 64, 113, 128)] == [1, 1, 2, 2, 4, 8, 8]


def test_build_workspace_size():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_mih_build_workspace_bytes(20000, 64) == lib.cmh_code_sort_workspace_bytes(20000, 64)      # the sort's own
    big = lib.cmh_mih_build_workspace_bytes(2 ** 31 - 1, 128)
    assert 2 * 4 * (2 ** 31 - 1) < big < 2 ** 36 and big % 256 == 0
    for n, bits in ((0, 64), (2 ** 31, 64), (10, 0), (10, 129), (-1, 64)):
        assert lib.cmh_mih_build_workspace_bytes(n, bits) == 0


def test_argument_checks_run_before_any_launch():
    """Null pointers, bits outside [1, 128], radius outside [0, 3 m - 1], Q outside [1, 65 535], N < 1, a workspace that is too small:
    each comes back with its error code and a message that names the limit.  Non-null pointers are needed to reach the size checks:
    a host buffer serves, nothing dereferences it."""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    buf = (C.c_int64 * 8)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    build = lambda sign=p, n=10, bits=64, order=p, starts=p, ws=p, wsb=1 << 20: lib.cmh_mih_build(sign, n, bits, order, starts, ws, wsb, None)
    count = lambda q=p, Q=4, db=p, n=10, bits=64, radius=4, order=p, starts=p, hits=p: \
        lib.cmh_mih_count(q, Q, db, n, bits, radius, order, starts, hits, None)
    fill = lambda q=p, Q=4, db=p, n=10, bits=64, radius=4, order=p, starts=p, off=p, cap=5, idx=p, dist=p: \
        lib.cmh_mih_fill(q, Q, db, n, bits, radius, order, starts, off, cap, idx, dist, None)
    cases = [
        (lambda: build(sign=None), -1, b"mih_build: null"), (lambda: build(order=None), -1, b"null"), (lambda: build(starts=None), -1, b"null"),
        (lambda: build(n=0), -1, b"N=0 outside [1, 2^31 - 1]"), (lambda: build(n=2 ** 31), -1, b"outside [1, 2^31 - 1]"),
        (lambda: build(bits=0), -1, b"bits=0 outside [1, 128]"), (lambda: build(bits=129), -1, b"bits=129 outside [1, 128]"),
        (lambda: build(ws=None), -2, b"workspace"), (lambda: build(wsb=16), -2, b"mih_build: workspace 16 <"),
    ]
    for name, call in (("mih_count", count), ("mih_fill", fill)):
        cases += [
            (lambda call=call: call(q=None), -1, name.encode() + b": null"), (lambda call=call: call(db=None), -1, b"null"),
            (lambda call=call: call(order=None), -1, b"null"), (lambda call=call: call(starts=None), -1, b"null"),
            (lambda call=call: call(Q=0), -1, b"Q=0 outside [1, 65535]"), (lambda call=call: call(Q=65536), -1, b"Q=65536 outside [1, 65535]"),
            (lambda call=call: call(n=0), -1, b"N=0 outside [1, 2^31 - 1]"),
            (lambda call=call: call(bits=0), -1, b"bits=0 outside [1, 128]"), (lambda call=call: call(bits=129), -1, b"bits=129 outside [1, 128]"),
            (lambda call=call: call(radius=-1), -1, b"radius=-1 outside [0, 11]"), (lambda call=call: call(radius=12), -1, b"radius=12 outside [0, 11]"),
            (lambda call=call: call(bits=16, radius=3), -1, b"radius=3 outside [0, 2]"),
            (lambda call=call: call(bits=24, radius=6), -1, b"radius=6 outside [0, 5]"),
            (lambda call=call: call(bits=128, radius=24), -1, b"radius=24 outside [0, 23]"),
            (lambda call=call: call(db=odd), -1, b"aligned to 8 bytes"),
        ]
    cases += [(lambda: count(hits=None), -1, b"null"), (lambda: fill(off=None), -1, b"null"), (lambda: fill(idx=None), -1, b"null"),
              (lambda: fill(dist=None), -1, b"null"), (lambda: fill(cap=0), -1, b"capacity=0 below 1"),
              (lambda: fill(off=odd), -1, b"aligned to 8 bytes")]
    for k, (call, code, text) in enumerate(cases):
        rc = call()
        assert rc == code, (k, rc, lib.cmh_last_error())
        assert text in lib.cmh_last_error(), (k, lib.cmh_last_error())


def test_python_layer_refuses_cpu_tensors_and_limits_by_name():
    import torch
    import cmh_native as N
    sign = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.mih_build(sign, 64)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.mih_count(sign, sign, 64, 4, torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 65537, dtype=torch.int32))


def test_retrieve_near_flag(capsys):
    import retrieve
    args = retrieve.parse(["--codes", "x.mat", "--near", "4"])
    assert args.near == 4 and args.lookup is None and args.radius is None
    assert retrieve.parse(["--codes", "x.mat"]).near is None
    assert retrieve.parse(["--codes", "x.mat", "--near", "0", "--index", "db.npz", "--direction", "t2i", "--queries", "0:5"]).near == 0
    refused = [(["--radius", "1"], "--radius"), (["--lookup", "1"], "--lookup"), (["--map"], "--map"), (["--recall"], "--recall"),
               (["--stats"], "--stats"), (["--bucket-stats"], "--bucket-stats"), (["--k", "5"], "--k"), (["--graded"], "--graded")]
    refused += [(["--index", "db.npz", flag, "1"], flag) for flag in retrieve.FILTERS]
    for extra, flag in refused:
        with pytest.raises(SystemExit) as e:
            retrieve.parse(["--codes", "x.mat", "--near", "4"] + extra)
        assert e.value.code == 2 and f"--near and {flag} exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        retrieve.parse(["--codes", "x.mat", "--near", "-1"])
    assert e.value.code == 2 and "--near -1: a whole number of bits >= 0" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                           # the existing flags keep their messages
        retrieve.parse(["--codes", "x.mat", "--lookup", "1", "--radius", "1"])
    assert e.value.code == 2 and "--lookup and --radius exclude each other" in capsys.readouterr().err
