"""Host side of the filtered search, without a GPU: the entry points in the header and the binding, the refusals of the native calls
(they run before any HIP call), ItemMask's plain-torch half (bool round trip, & | ~, count), the NumPy restatement of maskutil.py
against brute force, the refusals of utils/retrieval.py's mask= and of retrieve.py's filter options."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import maskutil
import rankutil
from conftest import PKG, ROOT

ENTRY_POINTS = ("cmh_hamming_topk_few_masked", "cmh_topk_few_masked_workspace_bytes", "cmh_soft_topk_masked",
                "cmh_soft_topk_masked_workspace_bytes", "cmh_mask_from_labels", "cmh_mask_from_ids")


def test_entry_points_in_binding_and_header():
    import cmh_native as N
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in ENTRY_POINTS:
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    for name, value in (("CMH_MASK_ANY", N.MASK_ANY), ("CMH_MASK_ALL", N.MASK_ALL), ("CMH_MASK_NONE", N.MASK_NONE)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert N.ABI_VERSION == 6 and N.lib().cmh_version() == 6


def test_native_refusals_on_the_host():
    """Nothing is launched: the checks run before any HIP call.  Addresses are never read: 16 is any aligned non-null one."""
    import cmh_native as N
    lib = N.lib()
    p = 16
    for Q, n, bits in ((1, 100, 16), (64, 2 ** 31 - 1, 128), (17, 4099, 96)):
        assert lib.cmh_topk_few_masked_workspace_bytes(Q, n, bits) == lib.cmh_topk_few_workspace_bytes(Q, n, bits) > 0
        assert lib.cmh_soft_topk_masked_workspace_bytes(Q, n, bits) == lib.cmh_soft_topk_workspace_bytes(Q, n, bits) > 0
    for Q, n, bits in ((0, 10, 16), (65, 10, 16), (1, 0, 16), (1, 2 ** 31, 16), (1, 10, 129)):
        assert lib.cmh_topk_few_masked_workspace_bytes(Q, n, bits) == 0 and lib.cmh_soft_topk_masked_workspace_bytes(Q, n, bits) == 0
    for call, name in ((lib.cmh_hamming_topk_few_masked, b"hamming_topk_few_masked"), (lib.cmh_soft_topk_masked, b"soft_topk_masked")):
        run = lambda allow=p, Q=1, n=100, bits=16, k=5, found=p, ws=1 << 30, q=p: call(q, p, p, p, allow, Q, n, bits, k, p, p, found, p, ws, None)
        assert run(allow=None) == -1 and name in lib.cmh_last_error() and b"allow" in lib.cmh_last_error()
        for off in (1, 4, 20):                                     # a mask word is 8 bytes
            assert run(allow=off) == -1 and b"aligned to 8 bytes" in lib.cmh_last_error()
        assert run(found=None) == -1
        assert run(q=None) == -1 and b"null" in lib.cmh_last_error()
        assert run(n=9, k=10) == -1 and b"exceeds N" in lib.cmh_last_error()      # k against N, not against the admitted count
        for kw, what in ((dict(Q=65), b"Q=65"), (dict(k=4097), b"k=4097"), (dict(k=0), b"k=0"), (dict(bits=129), b"bits=129"),
                         (dict(n=2 ** 31), b"N=")):
            assert run(**kw) == -1 and what in lib.cmh_last_error(), kw
        assert run(ws=8) == -2 and b"workspace" in lib.cmh_last_error()
    assert lib.cmh_mask_from_labels(None, p, 0, 10, 8, p, None) == -1 and lib.cmh_mask_from_labels(p, p, 0, 10, 8, None, None) == -1
    assert lib.cmh_mask_from_labels(p, p, 0, 10, 8, 12, None) == -1 and b"aligned" in lib.cmh_last_error()
    assert lib.cmh_mask_from_labels(p, p, 3, 10, 8, p, None) == -1 and b"mode=3" in lib.cmh_last_error()
    assert lib.cmh_mask_from_labels(p, p, 0, 0, 8, p, None) == -1 and lib.cmh_mask_from_labels(p, p, 0, 10, 0, p, None) == -1
    assert lib.cmh_mask_from_ids(None, 3, 10, 1, p, p, None) == -1 and lib.cmh_mask_from_ids(p, 3, 10, 1, None, p, None) == -1
    assert lib.cmh_mask_from_ids(p, 3, 10, 1, p, None, None) == -1
    assert lib.cmh_mask_from_ids(p, 3, 10, 2, p, p, None) == -1 and b"value=2" in lib.cmh_last_error()
    assert lib.cmh_mask_from_ids(p, 3, 10, 1, 12, p, None) == -1 and lib.cmh_mask_from_ids(p, -1, 10, 1, p, p, None) == -1
    assert lib.cmh_mask_from_ids(None, 0, 10, 1, p, p, None) == 0                 # an empty list: nothing to do, nothing launched


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 1000])
def test_item_mask_bool_round_trip_operators_and_count(n):
    from utils.retrieval import ItemMask
    rng = np.random.default_rng(n)
    a, b = rng.random(n) < 0.5, rng.random(n) < 0.3
    a[n - 1] = True                                                # the last item, and with n = 64 k bit 63: the sign bit of the word
    ma, mb = ItemMask.from_bool(torch.from_numpy(a)), ItemMask.from_bool(torch.from_numpy(b))
    assert ma.words.dtype == torch.int64 and tuple(ma.words.shape) == ((n + 63) // 64,) and ma.n == n
    assert np.array_equal(ma.words.numpy(), maskutil.pack(a)) and np.array_equal(mb.words.numpy(), maskutil.pack(b))
    assert np.array_equal(ma.to_bool().numpy(), a) and np.array_equal(maskutil.unpack(ma.words.numpy(), n), a)
    assert ma.count() == int(a.sum()) and mb.count() == int(b.sum())
    assert np.array_equal((ma & mb).words.numpy(), maskutil.pack(a & b))
    assert np.array_equal((ma | mb).words.numpy(), maskutil.pack(a | b))
    assert np.array_equal((~ma).words.numpy(), maskutil.pack(~a))                 # ... with the tail bits cleared
    assert (~ma).count() == n - int(a.sum()) and (~~ma).count() == ma.count()
    full = ItemMask.all(n)
    assert np.array_equal(full.words.numpy(), maskutil.pack(np.ones(n, bool))) and full.count() == n and (~full).count() == 0
    # garbage behind n is never counted as admitted by to_bool / count
    if n % 64:
        dirty = ItemMask(ma.words.clone(), n)
        dirty.words[-1] |= -1 << (n % 64)
        assert np.array_equal(dirty.to_bool().numpy(), a) and dirty.count() == int(a.sum())
    with pytest.raises(Exception, match="items"):
        ma & ItemMask.all(n + 1)
    with pytest.raises(Exception, match="int64"):
        ItemMask(torch.zeros((n + 63) // 64 + 1, dtype=torch.int64), n)


def test_numpy_restatement_against_brute_force():
    for seed, (Q, n, K, k) in enumerate(((3, 1, 16, 1), (2, 65, 16, 7), (3, 130, 48, 40), (2, 257, 96, 5))):
        qB, rB = rankutil.codes(Q, n, K, 0.1, 300 + seed)
        for name, admit in maskutil.masks(n, k, 400 + seed):
            got, want = maskutil.masked_topk(qB, rB, admit, k), maskutil.brute_topk(qB, rB, admit, k)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, n)
            assert got[2][0] == min(k, int(admit.sum()))
    lab = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 1], [0, 1, 0]], np.float32)
    assert maskutil.label_rule(lab, [0, 2], "any").tolist() == [True, False, True, False]
    assert maskutil.label_rule(lab, [0, 1], "all").tolist() == [False, False, True, False]
    assert maskutil.label_rule(lab, [1], "none").tolist() == [True, True, False, False]
    assert not maskutil.label_rule(lab, [], "any").any() and maskutil.label_rule(lab, [], "all").all() and maskutil.label_rule(lab, [], "none").all()


def test_python_refusals_name_the_limit():
    """Before anything touches a GPU: CPU tensors never get as far as the device lookup."""
    import cmh_native as N
    from utils import retrieval as R
    q, r = torch.ones(2, 16), torch.ones(100, 16)
    m = R.ItemMask.all(100)
    with pytest.raises(N.NativeError, match="bits=160 exceeds 128"):
        R.hamming_topk(torch.ones(2, 160), torch.ones(100, 160), 5, mask=m)
    with pytest.raises(N.NativeError, match="k=4097 exceeds 4096"):
        R.hamming_topk(torch.ones(2, 16), torch.ones(5000, 16), 4097, mask=R.ItemMask.all(5000))
    with pytest.raises(N.NativeError, match="covers 99 items, the database holds 100"):
        R.hamming_topk(q, r, 5, mask=R.ItemMask.all(99))
    with pytest.raises(N.NativeError, match="shard_items and mask="):
        R.hamming_topk(q, r, 5, shard_items=50, mask=m)
    with pytest.raises(N.NativeError, match=r"k=101 outside \[1, N=100\]"):
        R.hamming_topk(q, r, 101, mask=m)
    with pytest.raises(N.NativeError, match="ItemMask"):
        R.hamming_topk(q, r, 5, mask=torch.ones(100, dtype=torch.bool))
    for kw, what in ((dict(graded=True), "graded=True and mask="), (dict(want_counts=True), "want_counts and mask="),
                     (dict(shard_items=1000), "shard_items and mask=")):
        with pytest.raises(N.NativeError, match=what):
            R._check_mask("CodeIndex.search", m, 100, 16, 5, **kw)
    with pytest.raises(N.NativeError, match="bits=160 exceeds 128"):
        R.soft_topk(torch.ones(2, 160), torch.ones(100, 160), 5, mask=m)
    with pytest.raises(N.NativeError, match="covers 100 items, the database holds 50"):
        R.soft_topk(q, torch.ones(50, 16), 5, mask=m)
    with pytest.raises(N.NativeError, match="k=4097 exceeds 4096"):
        R.soft_topk(torch.ones(2, 16), torch.ones(5000, 16), 4097, mask=R.ItemMask.all(5000))
    # _few_route keeps its keyword set: the mask is no routing matter
    assert R._few_route(Q=1, k=1, bits=16, shard_items=None, graded=False, want_counts=False) is (R.QUERIES_FEW >= 1)


def _retrieve(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), *argv], capture_output=True, text=True, timeout=300, env=env)


def test_retrieve_filter_arguments():
    import retrieve
    model = ["--method", "DSPH", "--pretrained", "m.pth", "-clip-path", "c.pt", "--output-dim", "16"]
    args = retrieve.parse(["--text", "a dog", "--index", "db.npz", "--any-label", "3,7", "--all-labels", "1", "--no-label", "2",
                           "--exclude-ids", "seen.txt", "--only-ids", "mine.txt", "--soft", *model])
    assert (args.any_label, args.all_labels, args.no_label) == ([3, 7], [1], [2]) and args.filtered
    assert (args.exclude_ids, args.only_ids) == ("seen.txt", "mine.txt")
    args = retrieve.parse(["--codes", "f.mat", "--index", "db.npz", "--queries", "0:3", "--no-label", "0"])
    assert args.no_label == [0] and args.filtered and args.any_label is None
    assert retrieve.parse(["--codes", "f.mat"]).filtered is False
    out = _retrieve("--codes", "f.mat", "--any-label", "3")
    assert out.returncode == 2 and "--any-label filters a saved CodeIndex: --index FILE is required" in out.stderr
    for mode in (["--map"], ["--graded"], ["--radius", "2"], ["--recall", "--targets", "t.txt"]):
        out = _retrieve("--codes", "f.mat", "--index", "db.npz", "--exclude-ids", "seen.txt", *mode)
        assert out.returncode == 2 and f"--exclude-ids and {mode[0]} exclude each other" in out.stderr, mode
    for bad in ("3,x", "-1", ""):
        out = _retrieve("--codes", "f.mat", "--index", "db.npz", "--all-labels=" + bad)
        assert out.returncode == 2 and "--all-labels: comma-separated class numbers >= 0" in out.stderr, bad
    out = _retrieve("--help")
    assert out.returncode == 0 and all(f in out.stdout for f in retrieve.FILTERS)
