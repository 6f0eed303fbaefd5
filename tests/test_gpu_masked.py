"""The filtered search (cmh_hamming_topk_few_masked, cmh_soft_topk_masked, cmh_mask_from_labels, cmh_mask_from_ids; ItemMask and
mask= of utils/retrieval.py) against code that is not under test: the UNMASKED search on a database of the admitted rows alone,
keep = mask.to_bool().nonzero(), k' = min(k, len(keep)), indices mapped back through keep; and, for the Hamming distance, the NumPy
restatement of maskutil.py.  Integers and half-integers: every comparison is torch.equal, the pad columns are checked on their own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import maskutil
import rankutil
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
SHAPES = [(16, 1), (48, 16), (64, 17), (96, 64), (128, 1), (64, 64), (128, 17), (16, 64)]      # (bits, Q): W = 1..4, a partial last
                                                                                                # word, both sides of the 16-query group


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reference(search, q, r, mask, k):
    """The unmasked search on r[keep] -> (idx [Q, k'], dist [Q, k']) in database indices, k' = min(k, len(keep)); None when nothing
    is admitted."""
    keep = mask.to_bool().nonzero().flatten()
    if keep.numel() == 0:
        return None
    idx, dist = search(q, r[keep], min(k, keep.numel()))[:2]
    return keep[idx.long()].to(torch.int32), dist


def _check(got, want, k, pad_dist, what):
    idx, dist, found = got[0], got[1], got[-1]
    Q = idx.shape[0]
    assert tuple(idx.shape) == tuple(dist.shape) == (Q, k) and found.dtype == torch.int32 and tuple(found.shape) == (Q,), what
    w = 0 if want is None else want[0].shape[1]
    assert torch.equal(found, torch.full((Q,), w, dtype=torch.int32, device=DEV)), what
    if want is not None:
        assert torch.equal(idx[:, :w], want[0]) and torch.equal(dist[:, :w], want[1]), what
    assert bool((idx[:, w:] == -1).all()) and bool((dist[:, w:] == pad_dist).all()), what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_hamming_masks_at_the_edges_of_the_walk(n):
    """One item ... 17 chunks with a ragged last one (1000 items: four 256-item chunks; 257: a one-item chunk), ternary codes
    (half-unit distances), every mask of maskutil.masks under k = 1, 7 and 300 (cut to n): the sparse masks admit fewer than k."""
    import cmh_native as N
    from utils import retrieval as R
    for s, (bits, Q) in enumerate(SHAPES):
        qB, rB = rankutil.codes(Q, n, bits, 0.1, 5000 + 31 * n + s)
        q, r = _t(qB), _t(rB)
        qp, rp = N.pack_codes(q), N.pack_codes(r)
        h = rankutil.half_units(qB, rB)
        for k in sorted({1, min(7, n), min(300, n)}):
            plain = N.hamming_topk_few(qp, rp, bits, k)
            for name, admit in maskutil.masks(n, k, 6000 + n + s):
                what = (n, bits, Q, k, name)
                mask = R.ItemMask.from_bool(_t(admit))
                got = R.hamming_topk(q, r, k, mask=mask)
                assert len(got) == 4 and got[2] is None
                _check(got, _reference(R.hamming_topk, q, r, mask, k), k, INF, what)
                w_idx, w_dist, w_found = maskutil.masked_topk(qB, rB, admit, k, h)
                assert torch.equal(got[0], _t(w_idx)) and torch.equal(got[1], _t(w_dist)) and torch.equal(got[3], _t(w_found)), what
                if name == "all":                                  # the unmasked kernel's bytes, found = k; and with garbage behind n
                    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[3].tolist() == [k] * Q
                    if n % 64:
                        dirty = mask.words.clone()
                        dirty[-1] |= -1 << (n % 64)
                        again = N.hamming_topk_few_masked(qp, rp, dirty, bits, k)
                        assert all(torch.equal(a, b) for a, b in zip(again, (got[0], got[1], got[3]))), what


@pytest.mark.parametrize("n", [1, 65, 257, 1000, 4099])
def test_soft_masks(n):
    """The same masks through soft_topk(mask=): pads idx = -1, dist = +inf, wdist = 2^31 - 1; all ones = the unmasked call."""
    from utils import retrieval as R
    for s, (bits, Q) in enumerate([(16, 1), (64, 17), (128, 2), (96, 64)]):
        _, rB = rankutil.codes(1, n, bits, 0.1, 7000 + 13 * n + s)
        u = torch.from_numpy(np.random.default_rng(7100 + n + s).standard_normal((Q, bits)).astype(np.float32)).to(DEV)
        r = _t(rB)
        k = min(7, n) if s % 2 else min(300, n)
        plain = R.soft_topk(u, r, k)
        for name, admit in maskutil.masks(n, k, 7200 + n + s):
            what = (n, bits, Q, k, name)
            mask = R.ItemMask.from_bool(_t(admit))
            got = R.soft_topk(u, r, k, mask=mask)
            assert len(got) == 4 and got[2].dtype == torch.int32
            want = _reference(R.soft_topk, u, r, mask, k)
            _check(got, want, k, INF, what)
            w = 0 if want is None else want[0].shape[1]
            assert bool((got[2][:, w:] == 2 ** 31 - 1).all()), what
            if want is not None:
                keep = mask.to_bool().nonzero().flatten()
                assert torch.equal(got[2][:, :w], R.soft_topk(u, r[keep], w)[2]), what
            if name == "all":
                assert all(torch.equal(a, b) for a, b in zip(got[:3], plain)) and got[3].tolist() == [k] * Q


@pytest.mark.parametrize("Q", [65, 130])
def test_more_than_64_queries_go_in_blocks(Q):
    from utils import retrieval as R
    qB, rB = rankutil.codes(Q, 1000, 64, 0.1, 8000 + Q)
    q, r = _t(qB), _t(rB)
    rng = np.random.default_rng(8100 + Q)
    qL, rL = (rng.random((Q, 40)) < 0.2).astype(np.float32), (rng.random((1000, 40)) < 0.1).astype(np.float32)
    for share, k in ((0.5, 20), (0.01, 20)):
        admit = rng.random(1000) < share
        mask = R.ItemMask.from_bool(_t(admit))
        idx, dist, rel, found = R.hamming_topk(q, r, k, _t(qL), _t(rL), mask=mask)
        w_idx, w_dist, w_found = maskutil.masked_topk(qB, rB, admit, k)
        assert torch.equal(idx, _t(w_idx)) and torch.equal(dist, _t(w_dist)) and torch.equal(found, _t(w_found))
        _check((idx, dist, found), _reference(R.hamming_topk, q, r, mask, k), k, INF, (Q, share))
        hit = (qL @ rL.T > 0)                                      # calc_neighbor's test; pads are no hits
        want_rel = np.where(w_idx >= 0, np.take_along_axis(hit, np.maximum(w_idx, 0).astype(np.int64), 1), False).astype(np.uint8)
        assert rel.dtype == torch.uint8 and torch.equal(rel, _t(want_rel))
        u = torch.from_numpy(rng.standard_normal((Q, 64)).astype(np.float32)).to(DEV)
        got = R.soft_topk(u, r, k, mask=mask)
        _check(got, _reference(R.soft_topk, u, r, mask, k), k, INF, (Q, share, "soft"))


def test_two_calls_give_equal_bytes_on_any_stream():
    import cmh_native as N
    qB, rB = rankutil.codes(5, 70001, 32, 0.1, 71)
    qp, rp = N.pack_codes(_t(qB)), N.pack_codes(_t(rB))
    admit = np.random.default_rng(72).random(70001) < 0.005       # about 350 admitted: 1000 columns end in pads
    allow = _t(maskutil.pack(admit))
    a = N.hamming_topk_few_masked(qp, rp, allow, 32, 1000)
    b = N.hamming_topk_few_masked(qp, rp, allow, 32, 1000)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = N.hamming_topk_few_masked(qp, rp, allow, 32, 1000)
    s.synchronize()
    w = maskutil.masked_topk(qB, rB, admit, 1000)
    for x, y, z, want in zip(a, b, c, w):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, _t(want))
    assert 0 < int(a[2][0]) < 1000


@pytest.mark.parametrize("classes", [20, 40])
def test_mask_from_labels(classes):
    """One and two label words; one item, a full word, one more, 16 words with a ragged last one; the three modes; an empty class
    set: any admits nothing, all and none everything."""
    from utils import retrieval as R
    rng = np.random.default_rng(9000 + classes)
    for n in (1, 64, 65, 1000):
        lab = (rng.random((n, classes)) < 0.15).astype(np.float32)
        lab[0, classes - 1] = 1.0                                  # the last class: the top of the last word in use
        for wanted in ([], [0], [classes - 1], [1, 5, classes - 1], list(range(classes))):
            for mode, kw in (("any", "any_of"), ("all", "all_of"), ("none", "none_of")):
                m = R.ItemMask.from_labels(_t(lab), **{kw: wanted})
                want = maskutil.label_rule(lab, wanted, mode)
                assert m.n == n and np.array_equal(m.to_bool().cpu().numpy(), want), (n, wanted, mode)
                assert np.array_equal(m.words.cpu().numpy(), maskutil.pack(want)), (n, wanted, mode)       # tail bits zero
        both = R.ItemMask.from_labels(_t(lab), any_of=[0, 1], none_of=[2])
        want = maskutil.label_rule(lab, [0, 1], "any") & maskutil.label_rule(lab, [2], "none")
        assert np.array_equal(both.to_bool().cpu().numpy(), want)
        assert R.ItemMask.from_labels(_t(lab)).count() == n        # no condition admits everything
    import cmh_native as N
    with pytest.raises(N.NativeError, match="class outside"):
        R.ItemMask.from_labels(_t(lab), any_of=[classes])


def test_mask_from_ids():
    import cmh_native as N
    from utils import retrieval as R
    for n in (1, 64, 65, 1000):
        ids = np.random.default_rng(9100 + n).integers(0, n, 3 * n // 4 + 1)
        ids = np.concatenate([ids, ids[:5], [0, n - 1, n - 1]])    # duplicates, both ends
        want = np.zeros(n, bool)
        want[ids] = True
        allowed, denied = R.ItemMask.from_ids(n, torch.from_numpy(ids)), R.ItemMask.from_ids(n, ids.tolist(), keep=False)
        assert np.array_equal(allowed.words.cpu().numpy(), maskutil.pack(want))
        assert np.array_equal(denied.words.cpu().numpy(), maskutil.pack(~want))
    assert R.ItemMask.from_ids(100, []).count() == 0 and R.ItemMask.from_ids(100, [], keep=False).count() == 100
    for bad in (100, -1, 2 ** 32 + 5):                             # (the last would fold into range as an int32)
        with pytest.raises(N.NativeError, match="outside"):
            R.ItemMask.from_ids(100, [3, bad, 7])
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(N.NativeError, match="outside"):
        N.mask_from_ids(words, torch.tensor([3, 100, 99, -1, 64], dtype=torch.int32, device=DEV), 100, 1)
    want = np.zeros(100, bool)
    want[[3, 99, 64]] = True
    assert np.array_equal(words.cpu().numpy(), maskutil.pack(want))               # the other bits are right


def test_code_index_masks(tmp_path):
    """CodeIndex.search(mask=index.mask(any_of=[c])) returns only items that carry class c and equals the reference; ids and label
    conditions AND; a mask built before add() is refused; the routes that take no mask refuse it; retrieve.py --any-label."""
    import cmh_native as N
    from utils import retrieval as R
    rng = np.random.default_rng(9200)
    qB, rB = rankutil.codes(3, 1000, 32, 0.1, 9201)
    qL, rL = (rng.random((3, 40)) < 0.2).astype(np.float32), (rng.random((1000, 40)) < 0.1).astype(np.float32)
    q, r = _t(qB), _t(rB)
    index = R.CodeIndex(r, _t(rL))
    c = 37
    mask = index.mask(any_of=[c])
    carries = rL[:, c] > 0
    assert np.array_equal(mask.to_bool().cpu().numpy(), carries) and 12 < carries.sum() < 1000
    idx, dist, rel, found = index.search(q, 12, mask=mask)
    assert rel is None and found.tolist() == [12] * 3 and bool(_t(carries)[idx.long()].all())
    _check((idx, dist, found), _reference(R.hamming_topk, q, r, mask, 12), 12, INF, "any_of")
    with_rel = index.search(q, 12, _t(qL), mask=mask)
    hit = (qL @ rL.T > 0)
    assert torch.equal(with_rel[0], idx) and torch.equal(with_rel[2], _t(np.take_along_axis(hit, idx.cpu().numpy().astype(np.int64), 1).astype(np.uint8)))
    deny = idx[0, :4].tolist()
    narrower = index.mask(any_of=[c], none_of=[0], ids=list(range(500)), exclude_ids=deny)
    want = carries & ~(rL[:, 0] > 0) & (np.arange(1000) < 500)
    want[deny] = False
    assert np.array_equal(narrower.to_bool().cpu().numpy(), want)
    got = index.search(q, 12, mask=narrower)
    w = maskutil.masked_topk(qB, rB, want, 12)
    assert torch.equal(got[0], _t(w[0])) and torch.equal(got[1], _t(w[1])) and torch.equal(got[3], _t(w[2]))
    u = torch.from_numpy(rng.standard_normal((3, 32)).astype(np.float32)).to(DEV)
    _check(index.search_soft(u, 12, mask=narrower), _reference(R.soft_topk, u, r, narrower, 12), 12, INF, "soft index")
    with pytest.raises(N.NativeError, match="graded=True and mask="):
        index.search(q, 12, _t(qL), graded=True, mask=mask)
    with pytest.raises(N.NativeError, match="shard_items and mask="):
        R.CodeIndex(r, _t(rL), shard_items=300).search(q, 12, mask=mask)
    with pytest.raises(N.NativeError, match="without labels"):
        R.CodeIndex(r).mask(any_of=[c])
    assert R.CodeIndex(r).mask(exclude_ids=[5]).count() == 999
    index.save(str(tmp_path / "db.npz"))
    index.add(r[:7], _t(rL[:7]))
    with pytest.raises(N.NativeError, match="covers 1000 items, the database holds 1007"):
        index.search(q, 12, mask=mask)
    assert index.search(q, 12, mask=index.mask(any_of=[c]))[3].tolist() == [12] * 3
    # retrieve.py in a fresh process on the saved index: the same neighbours, rows cut at found
    import scipy.io as scio
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB, "q_l": qL})
    (tmp_path / "seen.txt").write_text("\n".join(str(i) for i in deny) + "\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(mat), "--index", str(tmp_path / "db.npz"), "--k", "12",
                          "--any-label", str(c), "--no-label", "0", "--exclude-ids", str(tmp_path / "seen.txt")],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    want = carries & ~(rL[:, 0] > 0)
    want[deny] = False
    w_idx, w_dist, w_found = maskutil.masked_topk(qB, rB, want, 12)
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 3
    for i, line in enumerate(lines):
        cols = line.split()
        assert int(cols[0]) == i and len(cols) == 1 + w_found[i]
        assert [int(x.split(":")[0]) for x in cols[1:]] == w_idx[i, :w_found[i]].tolist()
        assert [float(x.split(":")[1]) for x in cols[1:]] == w_dist[i, :w_found[i]].tolist()
        assert all(int(x.split(":")[2]) == int(hit[i, int(x.split(":")[0])]) for x in cols[1:])
    short = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(mat), "--index", str(tmp_path / "db.npz"), "--k", "12",
                            "--queries", "1:2", "--all-labels", f"{c},0,1"], capture_output=True, text=True, timeout=300, env=env)
    assert short.returncode == 0, short.stderr
    few = carries & (rL[:, 0] > 0) & (rL[:, 1] > 0)
    assert few.sum() < 12 and len(short.stdout.split()) == 1 + few.sum()          # a row shorter than --k prints only what it found
