"""CPU checks around the radius search: the radius -> half-units rule, the NumPy restatement against a brute-force double loop, the
ABI's two entry points and their host-side refusals, and retrieve.py's argument exclusivity.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rangeutil as U
from conftest import ROOT


def test_radius_to_half_units():
    """hr = min(2K, floor(2 * radius)); radius < 0 or NaN is a NativeError."""
    import cmh_native as N
    import utils.retrieval as R
    K = 16
    for radius, hr in ((0, 0), (0.5, 1), (0.49, 0), (2, 4), (K, 2 * K), (K + 3, 2 * K), (1e30, 2 * K), (math.inf, 2 * K), (0.999, 1),
                       (K - 0.5, 2 * K - 1), (K - 0.25, 2 * K - 1)):
        assert R.radius_half_units(radius, K) == hr == U.half_radius(radius, K), radius
    for bad in (-1, -0.001, -math.inf, math.nan):
        with pytest.raises(N.NativeError):
            R.radius_half_units(bad, K)
        with pytest.raises(ValueError):
            U.half_radius(bad, K)


@pytest.mark.parametrize("zeros", [False, True])
def test_restatement_equals_a_double_loop(zeros):
    qB, rB, qL, rL = U.database(5, 23, 8, 3, zeros, 17)
    U.plant(qB, rB, [11])
    h = U.half_units(qB, rB)
    assert h.min() >= 0 and h.max() <= 16
    facts = set()
    for hr in (0, 1, 2, 4, 7, 8, 16):
        want = U.range_lists_brute(qB, rB, hr, qL, rL)
        got = U.range_lists(h, hr, qL, rL)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)
        plain = U.range_lists(h, hr)
        assert plain[3] is None and all(np.array_equal(a, b) for a, b in zip(plain[:3], got[:3]))
        sizes = np.diff(got[0])
        facts |= {"empty"} if (sizes == 0).any() else set()
        facts |= {"single"} if (sizes == 1).any() else set()
        for q in range(5):                                            # (distance, index) ascending inside every list
            d, i = got[2][got[0][q]:got[0][q + 1]], got[1][got[0][q]:got[0][q + 1]]
            assert all((d[x], i[x]) < (d[x + 1], i[x + 1]) for x in range(len(d) - 1))
    assert facts == {"empty", "single"}
    assert np.diff(U.range_lists(h, 16)[0]).tolist() == [23] * 5       # radius K: the whole database
    np.testing.assert_array_equal(U.range_lists(h, 0)[1][:3], [0, 10, 11])   # the three planted copies of query 0, by index


def test_workspace_query_answers_without_a_gpu():
    import cmh_native as N
    lib = N.lib()
    for Q, n, bits in ((1, 1, 1), (9, 1000, 16), (130, 1031, 64), (65, 1031, 128), (64, 1031, 160), (65535, 524287, 2048), (5000, 190834, 128)):
        assert lib.cmh_range_workspace_bytes(Q, n, bits) > 0, (Q, n, bits)
        # the images of the histogram pass and one word per (bin, lane) and per lane more: what the search's own passes take
        assert lib.cmh_range_workspace_bytes(Q, n, bits) == lib.cmh_retrieval_workspace_bytes(Q, n, bits)
    for Q, n, bits in ((0, 10, 16), (65536, 10, 16), (10, 0, 16), (10, 524288, 16), (10, 10, 0), (10, 10, 2049), (-1, 10, 16)):
        assert lib.cmh_range_workspace_bytes(Q, n, bits) == 0, (Q, n, bits)


def test_abi_carries_both_names():
    import cmh_native as N
    lib = N.lib()
    names = {"cmh_range_workspace_bytes", "cmh_hamming_range"}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmh.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(cmh_[a-z0-9_]+)\s*\(", header))
    assert names <= set(N.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert names <= set(re.findall(r" T (cmh_[a-z0-9_]+)", out))
    assert lib.cmh_version() == N.ABI_VERSION == 6                    # entry points were added, nothing else changed
    assert len(N.SIGNATURES["cmh_hamming_range"][1]) == 22


def test_native_refusals_come_before_any_launch():
    """Null operands, labels on one side only, rel without labels, a radius outside [0, 2 * bits], sizes outside the limits and a
    short workspace return -1 with a message: nothing is launched, so this runs without a GPU.  (Non-null pointers are host
    addresses the call never reads.)"""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40

    def call(qs=p, qn=p, ql=None, rs=p, rn=p, rl=None, Q=4, n=10, bits=16, classes=0, hr=4, row_off=p, base=0, idx=p, dist=p, rel=None,
             ws=p, ws_bytes=big):
        return lib.cmh_hamming_range(qs, qn, ql, rs, rn, rl, Q, n, bits, classes, hr, None, None, row_off, base, idx, dist, rel, None,
                                     ws, ws_bytes, None)

    bad = [dict(qs=None), dict(qn=None), dict(rs=None), dict(rn=None), dict(row_off=None), dict(idx=None), dict(dist=None),
           dict(ql=p, classes=6), dict(rl=p, classes=6), dict(rel=p), dict(hr=-1), dict(hr=33), dict(Q=0), dict(Q=65536), dict(n=0),
           dict(n=524288), dict(bits=0), dict(bits=2049), dict(ql=p, rl=p, classes=0), dict(ql=p, rl=p, classes=2049), dict(ws=None),
           dict(ws_bytes=lib.cmh_range_workspace_bytes(4, 10, 16) - 1), dict(base=-1), dict(base=2 ** 31 - 10)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert len(lib.cmh_last_error()) > 0


def test_binding_and_functions_refuse_bad_arguments_on_the_host():
    import torch
    import cmh_native as N
    import utils.retrieval as R
    planes = (torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(N.NativeError):                                # CPU tensors: no fallback
        N.hamming_range(planes, planes, 16, 4, row_off=torch.zeros(2, dtype=torch.int64),
                        out=(torch.zeros(4, dtype=torch.int32), torch.zeros(4), None))
    codes, lab = torch.ones(2, 16), torch.ones(2, 3)
    with pytest.raises(N.NativeError):
        R.hamming_range(codes, codes, 1, query_L=lab)                 # labels on one side only
    with pytest.raises(N.NativeError):
        R.hamming_range(codes, codes, -1)
    with pytest.raises(N.NativeError):
        R.hamming_range(codes, codes, float("nan"))


def test_retrieve_argument_exclusivity():
    import retrieve
    a = retrieve.parse(["--codes", "x.mat", "--radius", "1.5", "--max-hits", "100", "--index", "db.npz", "--queries", "0:3"])
    assert a.radius == 1.5 and a.max_hits == 100 and a.k is None and not a.map and not a.graded
    a = retrieve.parse(["--codes", "x.mat", "--k", "3"])
    assert a.radius is None and a.max_hits is None and a.k == 3
    for extra in (["--k", "3"], ["--map"], ["--graded"]):
        with pytest.raises(SystemExit) as e:
            retrieve.parse(["--codes", "x.mat", "--radius", "1"] + extra)
        assert e.value.code != 0
    for argv in (["--codes", "x.mat", "--radius", "-1"], ["--codes", "x.mat", "--radius", "nan"], ["--codes", "x.mat", "--max-hits", "5"]):
        with pytest.raises(SystemExit) as e:
            retrieve.parse(argv)
        assert e.value.code != 0
