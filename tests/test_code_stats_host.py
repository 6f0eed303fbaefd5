"""Host side of the code diagnostics, without a GPU: stats_from_counts against the NumPy restatement of statsutil.py (which works
from float codes), the decisions that are exact in Python integers, the refusals of cmh_code_gram (they run before any HIP call),
the trainer flag and retrieve.py --stats' parsing."""
import os
import re

import numpy as np
import pytest

import statsutil
from conftest import ROOT

TOL = 1e-12      # the project's bar for the graded metrics


def _counts(A):
    g, s, ab, _, _ = statsutil.gram(A, A)
    return g, s, ab


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any(), what
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= TOL, f"{what}: {err:.3e}"


@pytest.mark.parametrize("classes", [None, 1, 5])
@pytest.mark.parametrize("zeros", [0.0, 0.1])
@pytest.mark.parametrize("K", [1, 16, 33])
def test_stats_from_counts_against_the_restatement(K, zeros, classes):
    from utils.code_stats import stats_from_counts
    n = 257
    A, B = statsutil.codes(n, K, 10 * K + 1, zeros), statsutil.codes(n, K, 10 * K + 2, zeros)
    B[:, : K // 2] = A[:, : K // 2]                                 # half of the other modality's bits agree
    B[::5] = -B[::5]
    L = None if classes is None else statsutil.labels(n, classes, K)
    want = statsutil.stats(A, paired=B, L=L)
    assert len(want["dead_bits"]) == 0 and float(want["live_variance"].min()) >= 0.01      # the restatement's own conditioning
    g, s, ab = _counts(A)
    gxy, _, _, s2, ab2 = statsutil.gram(A, B)
    cls = None
    if L is not None:
        glc, cnt = statsutil.gram(L, A)[:2]
        cls = (cnt, glc, statsutil.gram(L, np.abs(A))[0])
    got = stats_from_counts(n, g, s, ab, pair=(gxy, s2, ab2), classes=cls)
    for key in ("bit_mean", "bit_bias", "balance", "bit_entropy", "corr", "mean_abs_corr", "max_abs_corr", "bit_agreement",
                "mean_agreement", "pair_distance", "cross_corr"):
        _close(got[key], want[key], key)
    assert got["dead_bits"] == [] and got["duplicate_bits"] == want["duplicate_bits"]
    assert np.array_equal(got["pair_dot"], want["pair_dot"])
    if got["max_corr_pair"] is not None:
        i, j = got["max_corr_pair"]
        assert i < j and abs(got["corr"][i, j]) == got["max_abs_corr"]
    else:
        assert K == 1
    if L is not None:
        for key in ("class_bit_mean", "bit_class_mi", "best_class_mi"):
            _close(got[key], want[key], key)
        assert all(got["bit_class_mi"][got["best_class"][k], k] == got["best_class_mi"][k] for k in range(K))
    assert np.array_equal(got["gram"], g) and np.array_equal(got["sum"], s) and np.array_equal(got["abs"], ab)


def test_dead_copied_negated_and_almost_copied_bits():
    from utils.code_stats import stats_from_counts
    n = 257
    A = statsutil.codes(n, 8, 3)
    A[:, 2] = 1.0                                                   # constant: dead
    A[:, 5] = A[:, 0]                                               # a copy
    A[:, 6] = -A[:, 1]                                              # a negation
    A[:, 7] = A[:, 3]
    A[100, 7] = -A[100, 7]                                          # a copy but for one item
    got = stats_from_counts(n, *_counts(A))
    assert got["dead_bits"] == [2]
    assert not got["corr"][2].any() and not got["corr"][:, 2].any()
    assert got["duplicate_bits"] == [(0, 5), (1, 6)]
    assert got["corr"][0, 5] == 1.0 and got["corr"][1, 6] == -1.0 and 0.9 < got["corr"][3, 7] < 1.0
    assert all(got["corr"][i, i] == 1.0 for i in range(8) if i != 2)
    want = statsutil.stats(A)
    assert want["dead_bits"] == [2] and want["duplicate_bits"] == [(0, 5), (1, 6)]
    _close(got["corr"], want["corr"], "corr")


def test_exact_decisions_where_int64_products_overflow():
    """n = 2^31 - 1 items without zeros: bit 1 copies bit 0; bit 2 copies it but for ONE item that went from +1 to -1.  D and V are
    near 2^62 and the compared products near 2^124: int64 arithmetic would wrap."""
    from utils.code_stats import stats_from_counts
    n, s0 = 2 ** 31 - 1, 12345
    s = [s0, s0, s0 - 2, n]
    gram = [[n, n, n - 2, s0], [n, n, n - 2, s0], [n - 2, n - 2, n, s0 - 2], [s0, s0, s0 - 2, n]]      # bit 3: all +1
    got = stats_from_counts(n, gram, s, [n] * 4)
    assert got["dead_bits"] == [3] and got["duplicate_bits"] == [(0, 1)]
    D, V0, V2 = n * (n - 2) - s0 * (s0 - 2), n * n - s0 * s0, n * n - (s0 - 2) ** 2
    assert D * D != V0 * V2 and min(D, V0, V2) > 2 ** 61 and D * D > 2 ** 123      # (the hand-made case is what it claims to be)
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    want = float(Decimal(D) / (Decimal(V0) * Decimal(V2)).sqrt())                  # 1 - 9.3e-10: one item in 2^31 differs
    assert got["corr"][0, 1] == 1.0 and want < 1.0 and abs(got["corr"][0, 2] - want) < 1e-15 and not got["corr"][3].any()
    assert got["max_corr_pair"] == (0, 1)


def test_an_empty_class_gives_zeros():
    from utils.code_stats import stats_from_counts
    n, K = 257, 16
    A, L = statsutil.codes(n, K, 5, 0.1), statsutil.labels(n, 3, 5)
    L[:, 1] = 0.0
    glc, cnt = statsutil.gram(L, A)[:2]
    got = stats_from_counts(n, *_counts(A), classes=(cnt, glc, statsutil.gram(L, np.abs(A))[0]))
    assert int(got["class_count"][1]) == 0
    for key in ("class_bit_mean", "bit_class_mi"):
        assert not np.isnan(got[key]).any() and not got[key][1].any(), key
    want = statsutil.stats(A, L=L)
    _close(got["bit_class_mi"], want["bit_class_mi"], "bit_class_mi")


def test_entry_points_in_binding_and_header():
    import cmh_native as N
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in ("cmh_code_gram", "cmh_code_gram_workspace_bytes"):
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    for name, value in (("CMH_GRAM_BITS_MAX", N.GRAM_BITS_MAX), ("CMH_GRAM_CHUNK_MAX", N.GRAM_CHUNK_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert N.ABI_VERSION == 6 and N.lib().cmh_version() == 6


def test_native_refusals_on_the_host():
    """Nothing is launched: the checks run before any HIP call.  Addresses are never read: 16 is any aligned non-null one."""
    import cmh_native as N
    lib = N.lib()
    p = 16
    size = lib.cmh_code_gram_workspace_bytes
    for n, ab, bb, ch in ((1, 1, 1, 0), (2 ** 31 - 1, 256, 256, 0), (1000, 64, 21, 64), (70000, 128, 128, N.GRAM_CHUNK_MAX)):
        assert size(n, ab, bb, ch) > 0
    for n, ab, bb, ch in ((0, 16, 16, 0), (2 ** 31, 16, 16, 0), (10, 0, 16, 0), (10, 257, 16, 0), (10, 16, 0, 0), (10, 16, 257, 0),
                          (10, 16, 16, 65), (10, 16, 16, -64), (10, 16, 16, N.GRAM_CHUNK_MAX + 64)):
        assert size(n, ab, bb, ch) == 0, (n, ab, bb, ch)

    def run(a_s=p, a_n=p, b_s=p, b_n=p, n=100, ab=16, bb=16, ch=0, gram=p, ws=p, ws_bytes=1 << 30):
        return lib.cmh_code_gram(a_s, a_n, b_s, b_n, n, ab, bb, ch, gram, p, p, p, p, ws, ws_bytes, None)

    for kw in (dict(a_s=None), dict(a_n=None), dict(b_s=None), dict(b_n=None), dict(gram=None)):
        assert run(**kw) == -1 and b"code_gram" in lib.cmh_last_error() and b"null" in lib.cmh_last_error(), kw
    for kw, what in ((dict(n=0), b"N=0"), (dict(n=2 ** 31), b"N="), (dict(ab=0), b"abits=0"), (dict(ab=257), b"abits=257"),
                     (dict(bb=0), b"bbits=0"), (dict(bb=257), b"bbits=257"), (dict(ch=65), b"chunk_items=65"),
                     (dict(ch=N.GRAM_CHUNK_MAX + 64), b"chunk_items=")):
        assert run(**kw) == -1 and what in lib.cmh_last_error(), kw
    # B rows of an even number of words are read as 8-byte pairs
    assert run(bb=64, b_s=12) == -1 and b"aligned to 8 bytes" in lib.cmh_last_error()
    assert run(bb=128, b_n=20) == -1 and b"aligned to 8 bytes" in lib.cmh_last_error()
    assert run(bb=96, b_n=20, ws_bytes=0) == -2                   # three words per row: read word by word, any alignment
    need = size(100, 16, 16, 0)
    assert run(ws_bytes=need - 1) == -2 and b"workspace" in lib.cmh_last_error()
    assert run(ws=None) == -2


def test_eval_codes_flag():
    import argsbase
    assert argsbase.BASE_FLAGS[-1][0] == "--eval-graded"
    assert "--eval-codes" in [f[0] for f in argsbase.BASE_FLAGS]
    parser = argsbase.get_baseargs()
    assert parser.parse_args([]).eval_codes is False
    assert parser.parse_args(["--eval-codes", "true"]).eval_codes is True


def test_retrieve_stats_parses_and_excludes():
    import retrieve
    args = retrieve.parse(["--codes", "x.mat", "--stats", "--stats-out", "s.npz"])
    assert args.stats and args.stats_out == "s.npz"
    assert retrieve.parse(["--index", "db.npz", "--stats"]).codes is None
    assert not retrieve.parse(["--codes", "x.mat"]).stats
    model = ["--method", "DSPH", "--pretrained", "m.pth", "-clip-path", "c.pt", "--output-dim", "16"]
    for argv in (["--codes", "x.mat", "--stats", "--map"], ["--codes", "x.mat", "--stats", "--radius", "2"],
                 ["--codes", "x.mat", "--stats", "--recall"], ["--index", "db.npz", "--stats", "--text", "a dog"] + model,
                 ["--index", "db.npz", "--stats", "--image", "a.jpg"] + model, ["--codes", "x.mat", "--stats-out", "s.npz"],
                 ["--stats"]):
        with pytest.raises(SystemExit):
            retrieve.parse(argv)
