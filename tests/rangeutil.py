"""NumPy restatement of the radius search (utils/retrieval.py::hamming_range) and the inputs its tests share.

    h[q, j] = K - qB[q] . rB[j]            integer half-units of calc_hammingDist, 0 <= h <= 2K
    ball(q) = {j : h[q, j] <= hr},         hr = min(2K, floor(2 * radius))
    list(q) = np.flatnonzero(h[q] <= hr) reordered by np.argsort(h[q][sel], kind="stable"): (distance, database index) ascending
    dist    = 0.5 * h,   rel = (qL @ rL.T > 0)

Everything is integer or half-integer: comparisons with the GPU are exact."""
import math

import numpy as np


def half_radius(radius, K):
    """The radius rule, restated: hr = min(2K, floor(2 * radius)); negative or NaN has no hr."""
    r = float(radius)
    if math.isnan(r) or r < 0:
        raise ValueError(f"radius {radius}")
    return 2 * K if 2 * r >= 2 * K else int(math.floor(2 * r))


def half_units(qB, rB):
    qB, rB = np.asarray(qB).astype(np.int64), np.asarray(rB).astype(np.int64)
    return qB.shape[1] - qB @ rB.T


def range_lists(h, hr, qL=None, rL=None):
    """h int [Q, N] -> (offsets int64 [Q+1], idx int32 [T], dist f32 [T], rel uint8 [T] or None)."""
    Q = h.shape[0]
    hit = None if qL is None else (np.asarray(qL).astype(np.int64) @ np.asarray(rL).astype(np.int64).T > 0)
    offsets, idx, dist, rel = np.zeros(Q + 1, np.int64), [], [], []
    for q in range(Q):
        sel = np.flatnonzero(h[q] <= hr)
        sel = sel[np.argsort(h[q][sel], kind="stable")]
        offsets[q + 1] = offsets[q] + sel.size
        idx.append(sel.astype(np.int32))
        dist.append((0.5 * h[q][sel]).astype(np.float32))
        if hit is not None:
            rel.append(hit[q][sel].astype(np.uint8))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return offsets, cat(idx, np.int32), cat(dist, np.float32), (None if hit is None else cat(rel, np.uint8))


def range_lists_brute(qB, rB, hr, qL=None, rL=None):
    """The same lists by a double loop over (query, item) and Python's sort on (h, index): what range_lists is checked against."""
    qB, rB = np.asarray(qB), np.asarray(rB)
    K = qB.shape[1]
    offsets, idx, dist, rel = [0], [], [], []
    for q in range(qB.shape[0]):
        found = []
        for j in range(rB.shape[0]):
            hq = K - int(sum(int(a) * int(b) for a, b in zip(qB[q], rB[j])))
            if hq <= hr:
                found.append((hq, j))
        found.sort()
        offsets.append(offsets[-1] + len(found))
        for hq, j in found:
            idx.append(j)
            dist.append(0.5 * hq)
            if qL is not None:
                rel.append(1 if any(int(a) and int(b) for a, b in zip(qL[q], rL[j])) else 0)
    return (np.array(offsets, np.int64), np.array(idx, np.int32), np.array(dist, np.float32),
            None if qL is None else np.array(rel, np.uint8))


def database(Q, n, K, C, zeros, seed):
    """Random codes and labels (the recipe of the sharded-retrieval tests): values drawn with rng.integers, labels at density 0.25,
    query 1 without labels."""
    rng = np.random.default_rng(seed)
    vals = np.array([-1.0, 1.0, 0.0] if zeros else [-1.0, 1.0], np.float32)
    qB, rB = vals[rng.integers(0, len(vals), (Q, K))], vals[rng.integers(0, len(vals), (n, K))]
    qL, rL = (rng.random((Q, C)) < 0.25).astype(np.float32), (rng.random((n, C)) < 0.25).astype(np.float32)
    if Q > 1:
        qL[1] = 0
    return qB, rB, qL, rL


def chunk_items(Q, n, bits, cus=256):
    """Items per chunk of one native call (csrc/retrieval.hip::cut_chunks): where its workgroups' shares of the database meet."""
    tiles, glob = (Q + 63) // 64, bits > 128
    lds = 0 if glob else (2 * bits + 1) * 256
    per_cu = 8 if lds == 0 else min(160 * 1024 // lds, 8)
    s = cus * per_cu // tiles
    s = min(s, (n + 255) // 256, 32 if glob else 256)
    s = max(s, (n + 65531) // 65532, 1)
    return ((n + s - 1) // s + 3) & ~3


def plant(qB, rB, edges, seed=0):
    """Neighbours at small radii, written into rB (and zero-free codes into the planted queries of qB); -> the rows used.
    `edges` = rows e at which a chunk or a shard begins: copies go to e - 1 and e.
      query 0: three identical copies at rows 0, e0 - 1 and e0 (ties at h = 0 order by index; the ball spans the edge), a copy with
               one entry flipped (h = 2) at row N - 1
      query 1: one copy at row N - 2 or thereabouts: a singleton at radius 0
      query 2: a copy with one entry zeroed (odd h = 1) at row e1 - 1 and one with two entries flipped (h = 4) at row e1: empty at
               radius 0, a singleton at 0.5
    Queries a small input does not have, and rows it does not have, are left out."""
    rng = np.random.default_rng(1000 + seed)
    Q, K = qB.shape
    n = rB.shape[0]
    used = []

    def put(row, code):
        if 0 <= row < n and row not in used:
            rB[row] = code
            used.append(row)

    for q in range(min(Q, 3)):
        zero = qB[q] == 0
        qB[q][zero] = rng.choice([-1.0, 1.0], int(zero.sum()))
    edges = [e for e in edges if 0 < e < n] or [n // 2]
    e0, e1 = edges[0], edges[-1]

    def flipped(code, count):
        out = code.copy()
        out[rng.permutation(K)[:count]] *= -1
        return out

    put(0, qB[0])
    put(e0 - 1, qB[0])
    put(e0, qB[0])
    put(n - 1, flipped(qB[0], 1))
    if Q > 1:
        put(n - 2, qB[1])
    if Q > 2:
        zeroed = qB[2].copy()
        zeroed[int(rng.integers(0, K))] = 0
        put(e1 - 1 if e1 - 1 not in used else e1 - 2, zeroed)
        put(e1 if e1 not in used else e1 + 1, flipped(qB[2], 2))
    return used


def ball_facts(offsets, idx, chunk):
    """(empty balls, singletons, balls whose items lie in more than one chunk) of a CSR result."""
    sizes = np.diff(offsets)
    spans = sum(1 for q in range(len(sizes)) if sizes[q] > 1 and np.unique(idx[offsets[q]:offsets[q + 1]] // chunk).size > 1)
    return int((sizes == 0).sum()), int((sizes == 1).sum()), spans
