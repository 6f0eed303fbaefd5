"""NumPy restatement of the filtered search (utils/retrieval.py: ItemMask, hamming_topk(mask=)) and the masks its tests share.

    an allow-mask is one bit per database item: bit j % 64 of 64-bit word j / 64 = item j is admitted
    masked top-k of query q = the first min(k, A) ADMITTED columns of np.argsort(h[q], kind="stable"), h = rankutil.half_units
                              (K - q . r, the integer half-units of calc_hammingDist), as DATABASE indices; A = admitted items;
                              the columns behind hold idx = -1, dist = +inf; found = min(k, A)
    label rules              any: (label & need) != 0, all: (label & need) == need, none: (label & need) == 0 on multi-hot rows
Everything is integers and half-integers: comparisons with the GPU are exact."""
import numpy as np

import rankutil


def words(n):
    return (n + 63) // 64


def pack(admit):
    """bool [n] -> int64 [ceil(n / 64)], tail bits zero; written as a loop over the items, not as shifts of a matrix."""
    admit = np.asarray(admit).astype(bool)
    out = np.zeros(words(admit.size), np.uint64)
    for j in np.flatnonzero(admit):
        out[j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return out.view(np.int64)


def unpack(w, n):
    w = np.asarray(w).view(np.uint64)
    return np.array([bool((int(w[j // 64]) >> (j % 64)) & 1) for j in range(n)], bool)


def masked_topk(qB, rB, admit, k, h=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k], found int32 [Q]): a stable argsort of the half-units over the admitted columns.
    h: rankutil.half_units(qB, rB) when the caller has it already (many masks over one pair of code matrices)."""
    admit = np.asarray(admit).astype(bool)
    keep = np.flatnonzero(admit)
    Q = qB.shape[0]
    idx = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), np.inf, np.float32)
    got = min(k, keep.size)
    if got:
        h = rankutil.half_units(qB, rB[keep]) if h is None else h[:, keep]
        order = np.argsort(h, axis=1, kind="stable")[:, :got]
        idx[:, :got] = keep[order]
        dist[:, :got] = 0.5 * np.take_along_axis(h, order, 1)
    return idx, dist, np.full(Q, got, np.int32)


def brute_topk(qB, rB, admit, k):
    """The same by sorting (distance, index) pairs of the admitted items in Python: the check of masked_topk itself."""
    Q, K = qB.shape
    idx = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), np.inf, np.float32)
    found = np.zeros(Q, np.int32)
    for q in range(Q):
        pairs = sorted((K - int(np.dot(qB[q], rB[j])), j) for j in range(rB.shape[0]) if admit[j])[:k]
        found[q] = len(pairs)
        for c, (h, j) in enumerate(pairs):
            idx[q, c], dist[q, c] = j, 0.5 * h
    return idx, dist, found


def label_rule(labels, classes, mode):
    """labels multi-hot [n, C], classes: a list of class indices -> bool [n]."""
    lab = np.asarray(labels) != 0
    hit = lab[:, list(classes)] if len(classes) else np.zeros((lab.shape[0], 0), bool)
    if mode == "any":
        return hit.any(1)
    if mode == "all":
        return hit.all(1)
    assert mode == "none"
    return ~hit.any(1)


def masks(n, k, seed):
    """The masks every shape is searched under -> a list of (name, bool [n]).  `k` fixes the two masks that admit exactly k and
    k - 1 items.  A 'chunk' is 256 items, the fewest the Hamming search gives a wave: one whole chunk of zero words where the
    database has more than one, else one zero word where it has more than one word."""
    rng = np.random.default_rng(seed)
    every = np.zeros(n, bool)
    every[::64] = True
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[n - 1] = True, True
    hole = np.ones(n, bool)
    if n > 512:
        hole[256:512] = False
    elif n > 256:
        hole[:256] = False
    elif n > 64:
        hole[:64] = False
    exact, short = np.zeros(n, bool), np.zeros(n, bool)
    exact[rng.permutation(n)[:k]] = True
    short[rng.permutation(n)[:k - 1]] = True
    return [("all", np.ones(n, bool)), ("hole", hole), ("first", first), ("last", last), ("every64", every),
            ("half", rng.random(n) < 0.5), ("sparse", rng.random(n) < 0.02), ("exactly_k", exact), ("k_minus_1", short),
            ("nothing", np.zeros(n, bool))]
