"""NumPy restatement of the ranks of given targets (utils/retrieval.py::target_counts / ranks_from_counts / recall_from_counts) and
the inputs its tests share.

    h[q, j]      = K - qB[q] . rB[j]                       integer half-units of calc_hammingDist, 0 <= h <= 2K
    less         = #{j : h[q, j] < h[q, t]}
    ties_before  = #{j < bound : h[q, j] = h[q, t]}        bound = t for the whole database
    ties         = #{j : h[q, j] = h[q, t]}                 the target included
    rank (0-based): index = less + ties_before (the position of t in np.argsort(h[q], kind="stable")), optimistic = less,
                    pessimistic = less + ties - 1, expected = less + (ties - 1) / 2
A target of -1 is padding: three zeros, rank -1 (NaN under "expected").  The counts are integers: comparisons with the GPU are
exact.  The metrics are written as loops over the queries, another route than the tensor arithmetic of recall_from_counts."""
import numpy as np

TIES = ("index", "optimistic", "pessimistic", "expected")


def half_units(qB, rB):
    """K - q . r on {-1, 0, +1} codes; the f32 product is exact (|q . r| <= K <= 2048 < 2^24) and runs on BLAS."""
    qB, rB = np.asarray(qB, np.float32), np.asarray(rB, np.float32)
    assert qB.shape[1] <= 2048 and set(np.unique(qB)) | set(np.unique(rB)) <= {-1.0, 0.0, 1.0}
    return qB.shape[1] - (qB @ rB.T).astype(np.int64)


def as2d(targets):
    t = np.asarray(targets).astype(np.int64)
    return t[:, None] if t.ndim == 1 else t


def counts(h, targets, lo=0, hi=None):
    """h int [Q, N], targets int [Q] or [Q, G] (indices into the N columns, -1 = padding) -> int64 [Q, G, 3] over the columns
    lo:hi of h (a shard): the target's distance comes from the whole row, "before" are the shard's columns below the target."""
    t = as2d(targets)
    hi = h.shape[1] if hi is None else hi
    out = np.zeros(t.shape + (3,), np.int64)
    for q in range(t.shape[0]):
        row = h[q, lo:hi]
        for g in range(t.shape[1]):
            if t[q, g] < 0:
                continue
            ht = h[q, t[q, g]]
            bound = min(max(t[q, g] - lo, 0), hi - lo)
            out[q, g] = ((row < ht).sum(), (row[:bound] == ht).sum(), (row == ht).sum())
    return out


def counts_bound(h, ht, bound):
    """The same three counts from given target distances ht [Q, G] and bounds [Q, G] (-1 = padding): what the native call takes."""
    out = np.zeros(ht.shape + (3,), np.int64)
    for q in range(ht.shape[0]):
        for g in range(ht.shape[1]):
            if bound[q, g] >= 0:
                out[q, g] = ((h[q] < ht[q, g]).sum(), (h[q, :bound[q, g]] == ht[q, g]).sum(), (h[q] == ht[q, g]).sum())
    return out


def ranks(c, ties):
    """c int [Q, G, 3] -> 0-based ranks [Q, G]: int64 with -1 for padding; float64 with NaN under "expected"."""
    less, before, tied = c[..., 0], c[..., 1], c[..., 2]
    pad = tied == 0
    if ties == "expected":
        return np.where(pad, np.nan, less + (tied - 1) / 2.0)
    r = {"index": less + before, "optimistic": less, "pessimistic": less + tied - 1}[ties]
    return np.where(pad, -1, r)


def metrics(c, ks, ties):
    """-> dict(recall [len(ks)], median_rank, mean_rank, mrr (None under "expected"), best_rank [Q]) by a loop over the queries."""
    r = ranks(c, ties)
    best, hits = [], []
    for q in range(c.shape[0]):
        valid = [g for g in range(c.shape[1]) if c[q, g, 2] > 0]
        if not valid:
            best.append(np.nan if ties == "expected" else -1)
            continue
        best.append(min(r[q, g] for g in valid) + 1)
        if ties == "expected":
            hits.append([max(min(max((k - c[q, g, 0]) / c[q, g, 2], 0.0), 1.0) for g in valid) for k in ks])
        else:
            hits.append([1.0 if best[-1] <= k else 0.0 for k in ks])
    have = np.array([b for b in best if b == b and b > 0], np.float64)
    out = {"best_rank": np.array(best, np.float64 if ties == "expected" else np.int64)}
    if have.size == 0:
        out.update(recall=np.zeros(len(ks)), median_rank=0.0, mean_rank=0.0, mrr=None if ties == "expected" else 0.0)
        return out
    out.update(recall=np.array(hits, np.float64).mean(0), median_rank=float(np.median(have)), mean_rank=float(have.mean()),
               mrr=None if ties == "expected" else float((1.0 / have).mean()))
    return out


def codes(Q, n, K, zeros, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([-1.0, 1.0, 0.0] if zeros else [-1.0, 1.0], np.float32)
    return vals[rng.integers(0, len(vals), (Q, K))], vals[rng.integers(0, len(vals), (n, K))]


def duplicated(Q, n, K, distinct, seed):
    """A database of `distinct` different codes repeated over n rows (ties in the hundreds), zero-free queries drawn from them."""
    rng = np.random.default_rng(seed)
    base = rng.choice([-1.0, 1.0], (distinct, K)).astype(np.float32)
    return base[rng.integers(0, distinct, Q)], base[rng.integers(0, distinct, n)]


def targets(Q, n, G, seed, pad=True):
    """Random targets [Q, G]; the first rows aim at index 0 and n - 1; with pad, -1 in every slot position (row q pads slot q % G
    and, every third row, one more), and row Q - 1 is all padding when Q > 2."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, n, (Q, G)).astype(np.int64)
    if pad and G > 1:
        for q in range(Q):
            t[q, q % G] = -1
            if q % 3 == 2:
                t[q, (q + 2) % G] = -1
        if Q > 2:
            t[Q - 1] = -1
    t[0, G - 1] = 0
    if Q > 1:
        t[1, 0] = n - 1
    return t
