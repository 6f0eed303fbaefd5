"""Every group-count edge of the database walk of csrc/retrieval.hip, for every register form and in every pass.

A database of N <= 256 items is one chunk (cut_chunks cuts none below 256), so N alone sets the number of groups, N // U, of the
walk that all pass kernels share: U = 16 items per group at 32 bit, 8 at 64, 4 at 96 and 128; 160 bit is the form with the columns
in the workspace, which takes the items one at a time (it gets the sizes of U = 4).  Per form
    N = 1, U-1, U, U+1, 2U, 2U+1, 3U, 3U+U-1, 4U+3
= no group; the odd last group alone; a pair; a pair and the odd last group; two pairs; with a tail of 1, of U-1 and of 3 items.
The label histogram walks groups of 16 (one label word) and 4 (three): it meets the same sizes at 32 and at 96 / 128 bit.
Label words: 1 (24 classes) and 3 (80) in registers, 2 (40 classes) staged, and none where the entry point allows it.  Q = 70: two
tiles, the second with 6 live lanes.  A tenth of the code entries is zero (odd half-units).  Query 0 has no zero entry and the
LAST database item is its copy, so that the ball of radius 0 is not empty and its one member sits where the walk ends.

Each entry point against the restatements of tests/mapcountutil.py, gradedutil.py and rangeutil.py.  Integers, indices, distances
and flags exactly; APs within test_gpu_map_count's bound against the float64 restatement (TOL_REF, derived there)."""
import functools

import numpy as np
import pytest
import torch

import gradedutil as G
import mapcountutil as mu
import rangeutil as U
from test_gpu_map_count import TOL_REF, _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 70
UNROLL = {32: 16, 64: 8, 96: 4, 128: 4, 160: 4}
CLASSES = (24, 80, 40)


def _sizes(u):
    return (1, u - 1, u, u + 1, 2 * u, 2 * u + 1, 3 * u, 3 * u + u - 1, 4 * u + 3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(bits, n, C):
    """Inputs and everything the restatements say about them, built once per shape."""
    rng = np.random.default_rng([bits, n, C, 5])
    qB, rB = mu.codes(rng, Q, bits, True), mu.codes(rng, n, bits, True)
    qB[0][qB[0] == 0] = 1.0
    rB[n - 1] = qB[0]
    qL, rL = mu.labels(rng, Q, n, C)
    h, rel, grades = mu.half_units(qB, rB), mu.relevance(qL, rL), G.grades(qL, rL)
    assert (h % 2 == 1).any() and h[0, n - 1] == 0 and 0 <= h.min() and h.max() <= 2 * bits
    counts = np.zeros((Q, 2 * bits + 1, 2), np.int64)
    np.add.at(counts, (np.arange(Q)[:, None], h, rel.astype(np.int64)), 1)
    return dict(qB=qB, rB=rB, qL=qL, rL=rL, h=h, rel=rel, grades=grades, counts=counts, order=np.argsort(h, axis=1, kind="stable"),
                ap=mu.restated_ap(qB, rB, qL, rL, (None, 1)))


def _eq(got, want, note):
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(note))


def _search(N, c, qp, rp, bits, n, ql, rl, note):
    for k in sorted({1, n}):
        idx, dist, rel = N.hamming_topk(qp, rp, bits, k, ql, rl)
        want = c["order"][:, :k]
        _eq(idx, want.astype(np.int32), (note, "topk idx", k))
        _eq(dist, (0.5 * np.take_along_axis(c["h"], want, 1)).astype(np.float32), (note, "topk dist", k))
        if ql is None:
            assert rel is None
        else:
            _eq(rel, np.take_along_axis(c["rel"], want, 1).astype(np.uint8), (note, "topk rel", k))


def _ranges(N, c, qp, rp, bits, ql, rl, counts, note):
    for hr in (0, bits, 2 * bits):
        off = torch.zeros(Q + 1, dtype=torch.int64, device=DEV)
        off[1:] = counts[:, :hr + 1].sum((1, 2)).cumsum(0)
        T = int(off[-1])
        want = U.range_lists(c["h"], hr, None if ql is None else c["qL"], None if ql is None else c["rL"])
        assert T == int(want[0][-1]) and T >= 1, (note, hr, T)
        out = (torch.full((T,), -7, dtype=torch.int32, device=DEV), torch.full((T,), -7.0, dtype=torch.float32, device=DEV),
               None if ql is None else torch.full((T,), 7, dtype=torch.uint8, device=DEV))
        N.hamming_range(qp, rp, bits, hr, ql, rl, row_off=off[:-1].contiguous(), out=out)
        _eq(off, want[0], (note, "range offsets", hr))
        _eq(out[0], want[1], (note, "range idx", hr))
        _eq(out[1], want[2], (note, "range dist", hr))
        if ql is not None:
            _eq(out[2], want[3], (note, "range rel", hr))


@pytest.mark.parametrize("C", CLASSES + (None,))
@pytest.mark.parametrize("bits", sorted(UNROLL))
def test_every_pass_at_every_group_count_edge(bits, C):
    import cmh_native as N
    for n in _sizes(UNROLL[bits]):
        note = f"bits={bits} N={n} C={C}"
        c = _case(bits, n, C or CLASSES[0])
        qp, rp = N.pack_codes(_t(c["qB"])), N.pack_codes(_t(c["rB"]))
        if C is None:                                                   # no labels: the histogram, the search and the radius search
            counts = N.hamming_hist(qp, rp, bits)
            _eq(counts[:, :, 0], c["counts"].sum(2).astype(np.int32), (note, "hist"))
            assert int(counts[:, :, 1].abs().sum()) == 0, note
            _search(N, c, qp, rp, bits, n, None, None, note)
            _ranges(N, c, qp, rp, bits, None, None, counts, note)
            continue
        ql, rl = N.pack_labels(_t(c["qL"])), N.pack_labels(_t(c["rL"]))
        counts = N.hamming_hist(qp, rp, bits, ql, rl)
        _eq(counts, c["counts"].astype(np.int32), (note, "hist"))
        _search(N, c, qp, rp, bits, n, ql, rl, note)
        for k in sorted({1, n}):
            idx, dist, grade = N.hamming_topk_graded(qp, rp, bits, k, ql, rl, classes=C)
            want = c["order"][:, :k]
            _eq(idx, want.astype(np.int32), (note, "graded idx", k))
            _eq(dist, (0.5 * np.take_along_axis(c["h"], want, 1)).astype(np.float32), (note, "graded dist", k))
            _eq(grade, np.take_along_axis(c["grades"], want, 1).astype(np.uint8), (note, "grade", k))
        _ranges(N, c, qp, rp, bits, ql, rl, counts, note)
        for k, (want_ap, want_map) in c["ap"].items():
            ap_sum, own = N.hamming_ap_partial(qp, rp, bits, ql, rl, topk=k, want_counts=True)
            assert torch.equal(own, counts), (note, "ap counts", k)
            mp, ap = N.ap_finish(ap_sum, counts, bits, topk=k)
            _check(f"{note} k={k}", mp, ap, want_ap, want_map, TOL_REF)
        _eq(N.label_overlap_hist(ql, rl, C), G.histogram(c["grades"], C).astype(np.int32), (note, "label histogram"))
