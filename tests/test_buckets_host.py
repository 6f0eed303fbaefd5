"""CPU checks of the bucket table's host side: the statistics of an occupancy table (utils/code_stats.py::bucket_stats_from_sizes)
against direct NumPy arithmetic, the argument checks of the six entry points of csrc/retrieval_buckets.hip (nothing is launched, so
no GPU is needed), and the new flags of retrieve.py and the trainer."""
import math

import numpy as np
import pytest

NEW = ("cmh_code_sort_workspace_bytes", "cmh_code_sort", "cmh_code_bucket_count", "cmh_code_bucket_fill", "cmh_bucket_probe_count",
       "cmh_bucket_probe_fill")

# hand-made occupancy tables: bucket sizes, one entry per bucket
TABLES = {"singletons": [1] * 9, "one bucket": [7], "mixed": [1, 1, 1, 2, 2, 5, 5, 5, 40, 3]}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_bucket_stats_from_sizes_against_numpy(name):
    from utils.code_stats import bucket_stats_from_sizes
    per_bucket = np.array(TABLES[name], dtype=np.int64)
    n = int(per_bucket.sum())
    sizes, size_counts = np.unique(per_bucket, return_counts=True)
    st = bucket_stats_from_sizes(n, sizes, size_counts, bits=6)
    assert st["n"] == n and st["distinct"] == per_bucket.size and st["singletons"] == int((per_bucket == 1).sum())
    assert st["largest"] == int(per_bucket.max())
    want = sum(int(b) * (int(b) - 1) // 2 for b in per_bucket)
    assert type(st["collisions"]) is int and st["collisions"] == want
    assert st["collision_probability"] == float((per_bucket.astype(np.float64) ** 2).sum()) / (n * n)
    share = per_bucket / n
    assert math.isclose(st["bucket_entropy_bits"], float(-(share * np.log2(share)).sum()), rel_tol=0, abs_tol=1e-12)
    assert isinstance(st["bucket_entropy_bits"], float)
    assert st["used_share"] == per_bucket.size / min(n, 64) and st["bits"] == 6
    np.testing.assert_array_equal(st["occupancy"], np.stack([sizes, size_counts], axis=1))
    assert "used_share" not in bucket_stats_from_sizes(n, sizes, size_counts)
    if name == "singletons":
        assert st["collisions"] == 0 and st["collision_probability"] == 1 / 9 and st["used_share"] == 1.0
    if name == "one bucket":
        assert st["collisions"] == 21 and st["collision_probability"] == 1.0 and st["bucket_entropy_bits"] == 0.0


def test_bucket_stats_keep_exact_integers_past_float64_and_refuse_a_bad_table():
    import torch
    from utils.code_stats import bucket_stats_from_sizes
    n = 2 ** 31 - 1
    st = bucket_stats_from_sizes(n, torch.tensor([n]), torch.tensor([1]))
    assert st["collisions"] == n * (n - 1) // 2 and st["collisions"] > 2 ** 53      # no float64 in between
    for sizes, counts in (([1, 2], [1, 1]), ([0, 4], [1, 1]), ([2, 2], [1, 1]), ([], [])):
        with pytest.raises(ValueError, match="bucket_stats_from_sizes"):
            bucket_stats_from_sizes(4, sizes, counts)


def test_entry_points_are_declared_and_bound():
    import cmh_native as N
    assert set(NEW) <= set(N.SIGNATURES)
    assert (N.BUCKET_BITS_MAX, N.BUCKET_RADIUS_MAX, N.SORT_TILE) == (128, 2, 2048)
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "cmh.h")).read()
    for macro, value in (("CMH_BUCKET_BITS_MAX", N.BUCKET_BITS_MAX), ("CMH_BUCKET_RADIUS_MAX", N.BUCKET_RADIUS_MAX), ("CMH_SORT_TILE", N.SORT_TILE)):
        assert f"#define {macro} {value}" in header
    assert N.ABI_VERSION == 6


def test_sort_workspace_size():
    import cmh_native as N
    lib = N.lib()
    big = lib.cmh_code_sort_workspace_bytes(2 ** 31 - 1, 128)
    assert 2 * 4 * (2 ** 31 - 1) < big < 2 ** 36 and big % 256 == 0      # two index buffers and the counters; finite
    small = lib.cmh_code_sort_workspace_bytes(1, 1)
    assert 0 < small < 8192 and small % 256 == 0
    assert lib.cmh_code_sort_workspace_bytes(2 ** 31 - 1, 2048) == big     # the code length adds passes, not memory
    for n, bits in ((0, 64), (2 ** 31, 64), (10, 0), (10, 2049), (-1, 64)):
        assert lib.cmh_code_sort_workspace_bytes(n, bits) == 0


def test_argument_checks_run_before_any_launch():
    """Null pointers, bits = 0, bits = 129 (probes), radius = 3, Q = 65 536, N = 0: each comes back with its error code and a message
    that names the limit.  Non-null pointers are needed to reach the size checks: a host buffer serves, nothing dereferences it."""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    sort = lambda sign=p, n=10, bits=64, order=p, ws=p, wsb=1 << 20: lib.cmh_code_sort(sign, n, bits, order, ws, wsb, None)
    count = lambda sign=p, order=p, n=10, bits=64, head=p, nb=p, ws=p, wsb=1 << 20: \
        lib.cmh_code_bucket_count(sign, order, n, bits, head, nb, ws, wsb, None)
    fill = lambda sign=p, order=p, head=p, n=10, bits=64, U=3, starts=p, codes=p: \
        lib.cmh_code_bucket_fill(sign, order, head, n, bits, U, starts, codes, None)
    pcount = lambda q=p, Q=4, codes=p, starts=p, U=3, bits=64, radius=2, nb=p, ni=p: \
        lib.cmh_bucket_probe_count(q, Q, codes, starts, U, bits, radius, nb, ni, None)
    pfill = lambda q=p, Q=4, codes=p, starts=p, U=3, bits=64, radius=2, off=p, cap=5, hb=p, hd=p: \
        lib.cmh_bucket_probe_fill(q, Q, codes, starts, U, bits, radius, off, cap, hb, hd, None)
    odd = C.c_void_p(p.value + 4)
    cases = [
        (lambda: sort(sign=None), -1, b"null"), (lambda: sort(order=None), -1, b"null"),
        (lambda: sort(n=0), -1, b"N=0 outside [1, 2^31 - 1]"), (lambda: sort(n=2 ** 31), -1, b"outside [1, 2^31 - 1]"),
        (lambda: sort(bits=0), -1, b"bits=0 outside [1, 2048]"), (lambda: sort(bits=2049), -1, b"bits=2049 outside [1, 2048]"),
        (lambda: sort(ws=None), -2, b"workspace"), (lambda: sort(wsb=16), -2, b"workspace 16 <"),
        (lambda: count(head=None), -1, b"null"), (lambda: count(nb=None), -1, b"null"), (lambda: count(n=0), -1, b"N=0 outside"),
        (lambda: count(bits=0), -1, b"bits=0 outside"), (lambda: count(nb=odd), -1, b"aligned to 8 bytes"),
        (lambda: count(wsb=16), -2, b"workspace 16 <"),
        (lambda: fill(starts=None), -1, b"null"), (lambda: fill(n=0), -1, b"N=0 outside"), (lambda: fill(bits=0), -1, b"bits=0 outside"),
        (lambda: fill(U=0), -1, b"U=0 outside [1, N=10]"), (lambda: fill(U=11), -1, b"U=11 outside [1, N=10]"),
        (lambda: pcount(q=None), -1, b"null"), (lambda: pcount(ni=None), -1, b"null"),
        (lambda: pcount(Q=0), -1, b"Q=0 outside [1, 65535]"), (lambda: pcount(Q=65536), -1, b"Q=65536 outside [1, 65535]"),
        (lambda: pcount(bits=0), -1, b"bits=0 outside [1, 128]"), (lambda: pcount(bits=129), -1, b"bits=129 outside [1, 128]"),
        (lambda: pcount(radius=3), -1, b"radius=3 outside [0, 2]"), (lambda: pcount(radius=-1), -1, b"radius=-1 outside [0, 2]"),
        (lambda: pcount(U=0), -1, b"U=0 outside"), (lambda: pcount(ni=odd), -1, b"aligned to 8 bytes"),
        (lambda: pfill(hb=None), -1, b"null"), (lambda: pfill(off=None), -1, b"null"),
        (lambda: pfill(Q=65536), -1, b"Q=65536 outside [1, 65535]"), (lambda: pfill(bits=129), -1, b"bits=129 outside [1, 128]"),
        (lambda: pfill(bits=0), -1, b"bits=0 outside [1, 128]"), (lambda: pfill(radius=3), -1, b"radius=3 outside [0, 2]"),
        (lambda: pfill(cap=0), -1, b"capacity=0 below 1"), (lambda: pfill(off=odd), -1, b"aligned to 8 bytes"),
    ]
    for k, (call, code, text) in enumerate(cases):
        rc = call()
        assert rc == code, (k, rc)
        assert text in lib.cmh_last_error(), (k, lib.cmh_last_error())


def test_python_layer_refuses_cpu_tensors_and_limits_by_name():
    import torch
    import cmh_native as N
    sign = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.code_sort(sign, 64)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.bucket_probe_count(sign, sign, torch.zeros(5, dtype=torch.int32), 64, 0)


def test_retrieve_flags(capsys):
    import retrieve
    args = retrieve.parse(["--codes", "x.mat", "--lookup", "2"])
    assert args.lookup == 2 and not args.bucket_stats and args.radius is None
    assert retrieve.parse(["--codes", "x.mat"]).lookup is None
    args = retrieve.parse(["--codes", "x.mat", "--bucket-stats"])
    assert args.bucket_stats and not args.stats
    assert retrieve.parse(["--index", "db.npz", "--bucket-stats", "--stats-out", "o.npz"]).stats_out == "o.npz"
    assert retrieve.parse(["--codes", "x.mat", "--lookup", "0", "--index", "db.npz", "--direction", "t2i", "--queries", "0:5"]).lookup == 0
    refused = [(["--radius", "1"], "--lookup and --radius exclude each other"), (["--map"], "--lookup and --map exclude each other"),
               (["--recall"], "--lookup and --recall exclude each other"), (["--soft"], "--lookup and --soft exclude each other"),
               (["--k", "5"], "--lookup and --k exclude each other"), (["--graded"], "--lookup and --graded exclude each other")]
    refused += [(["--index", "db.npz", flag, "1"], f"--lookup and {flag} exclude each other") for flag in retrieve.FILTERS]
    for extra, message in refused:
        with pytest.raises(SystemExit) as e:
            retrieve.parse(["--codes", "x.mat", "--lookup", "1"] + extra)
        assert e.value.code == 2 and message in capsys.readouterr().err
    for argv, message in ((["--codes", "x.mat", "--lookup", "3"], "--lookup 3: 0, 1 or 2 bits"),
                          (["--codes", "x.mat", "--lookup", "-1"], "--lookup -1: 0, 1 or 2 bits"),
                          (["--bucket-stats"], "--bucket-stats: --codes FILE or --index FILE is required"),
                          (["--codes", "x.mat", "--bucket-stats", "--map"], "--bucket-stats and --map exclude each other"),
                          (["--codes", "x.mat", "--bucket-stats", "--radius", "1"], "--bucket-stats and --radius exclude each other"),
                          (["--codes", "x.mat", "--stats-out", "o.npz"], "--stats-out goes with --stats")):
        with pytest.raises(SystemExit) as e:
            retrieve.parse(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err


def test_eval_buckets_flag():
    import argsbase
    assert "--eval-buckets" in [f[0] for f in argsbase.BASE_FLAGS]
    parser = argsbase.get_baseargs()
    assert parser.parse_args([]).eval_buckets is False
    assert parser.parse_args(["--eval-buckets", "true"]).eval_buckets is True
