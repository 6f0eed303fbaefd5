"""NumPy restatement of the bucket table (csrc/retrieval_buckets.hip, utils/retrieval.py::BucketTable) and the case tables its tests
share.  No GPU code is imported here.

A row's key is its W = ceil(bits / 32) sign words with the bits at and behind `bits` cleared, taken as unsigned; keys compare with
word W - 1 most significant.  np.lexsort takes its LAST key as the primary one and is stable, so lexsort over the word columns in
ascending order IS the order the sort must produce, ties by item index included."""
import numpy as np

SORT_TILE = 2048          # cmh_native.SORT_TILE (the GPU test asserts they agree)


def word_masks(bits):
    W = (bits + 31) // 32
    m = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    if bits % 32:
        m[-1] = (1 << (bits % 32)) - 1
    return m


def keys(sign, bits):
    """sign: int32 / uint32 [N, W] as the plane holds it (garbage behind `bits` allowed) -> uint32 [N, W], masked."""
    return np.ascontiguousarray(sign).view(np.uint32).reshape(sign.shape) & word_masks(bits)[None, :]


def ref_order(words):
    return np.lexsort(tuple(words[:, w] for w in range(words.shape[1]))).astype(np.int32)


def ref_buckets(words):
    """-> (starts int32 [U + 1], codes uint32 [U, W]): np.unique sorts rows lexicographically by the first column, so the columns go
    in reversed (most significant word first) and come back."""
    uniq, counts = np.unique(words[:, ::-1], axis=0, return_counts=True)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return starts, np.ascontiguousarray(uniq[:, ::-1])


# ---- sort cases: (N, bits, draw).  N at the edges of one tile and of several, bits at the edges of a word; the draws:
#   random   independent fair bits (all distinct wherever 2^bits is far above N)
#   three    3 distinct codes over the whole N: stability decides the whole answer
#   equal    one code: every pass is skipped
#   topbit   equal but for bit 31 of the top word (bits % 32 == 0): a signed compare would reverse the order
#   lastbit  equal but for the last valid bit (the tail behind it holds garbage in every case with a tail)
#   ff       word 0 all ones in half of the items: the last bin of four passes
T = SORT_TILE
SORT_CASES = [
    (1, 1, "equal"), (1, 64, "random"), (2, 1, "random"), (2, 33, "lastbit"), (2, 128, "topbit"),
    (T - 1, 31, "random"), (T - 1, 64, "three"), (T, 32, "random"), (T, 32, "topbit"), (T, 96, "equal"),
    (T + 1, 33, "random"), (T + 1, 64, "ff"), (T + 1, 1, "random"),
    (3 * T + 17, 31, "lastbit"), (3 * T + 17, 64, "random"), (3 * T + 17, 128, "three"), (3 * T + 17, 96, "topbit"),
    (70001, 64, "random"), (70001, 128, "random"), (70001, 33, "three"), (70001, 32, "ff"), (70001, 96, "random"),
]


def draw_codes(N, bits, draw, seed):
    """-> f32 [N, bits] in {-1, +1}: the codes BEFORE the plane-level edits of `topbit` / `lastbit` (which the GPU test makes on the
    packed sign plane, so that they do not depend on how pack_codes lays bits out)."""
    rng = np.random.default_rng(seed)
    one = lambda: rng.integers(0, 2, size=(1, bits)) * 2 - 1
    if draw == "random":
        c = rng.integers(0, 2, size=(N, bits)) * 2 - 1
    elif draw == "three":
        base = np.concatenate([one(), one(), one()])
        base[1, 0], base[2, 0] = -base[0, 0], base[0, 0]          # at least two of them differ
        base[2, bits - 1] = -base[0, bits - 1] if bits > 1 else base[2, 0]
        c = base[rng.integers(0, 3, size=N)]
    elif draw in ("equal", "topbit", "lastbit"):
        c = np.repeat(one(), N, axis=0)
    elif draw == "ff":
        c = rng.integers(0, 2, size=(N, bits)) * 2 - 1
        c[rng.integers(0, 2, size=N) == 1, :32] = 1
    else:
        raise ValueError(draw)
    return c.astype(np.float32)


def edit_bit(N, bits, draw, seed):
    """-> (word, bit, flips bool [N]) of the plane-level edit of `topbit` / `lastbit`, or None: the bit is SET where flips, cleared
    elsewhere."""
    if draw not in ("topbit", "lastbit"):
        return None
    assert draw != "topbit" or bits % 32 == 0
    flips = np.random.default_rng(seed + 1).integers(0, 2, size=N) == 1
    if N >= 2:
        flips[0], flips[-1] = True, False                         # both values occur; item 0 carries the larger key
    return (bits - 1) // 32, (bits - 1) % 32, flips


# ---- lookup cases: name -> (n, bits, how the database is drawn)
LOOKUP_CASES = {"ties64": (4097, 64), "dense16": (1025, 16), "wide128": (257, 128)}
LOOKUP_CLASSES = 12


def lookup_case(name, Q, seed=11):
    """-> (rB f32 [n, bits], rL f32 [n, C], qB f32 [Q, bits], qL f32 [Q, C]).
    ties64: 4 097 items drawn from 300 distinct codes.  dense16: 1 025 items, each a centre code with at most two bits flipped - a
    16-bit code has 1 + 16 + 120 = 137 keys within radius 2, and the centre's ball hits every one of them (the most a ball can hold
    at this length).  wide128: 257 items from 40 codes.  The queries are database codes with 0, 1, 2, 3 entries flipped in turn."""
    n, bits = LOOKUP_CASES[name]
    rng = np.random.default_rng(seed + bits)
    if name == "dense16":
        rB = np.repeat(rng.integers(0, 2, size=(1, bits)) * 2 - 1, n, axis=0)
        near = [(a,) for a in range(bits)] + [(a, b) for a in range(bits) for b in range(a + 1, bits)]
        for i in range(1, n):                                     # item 0 stays the centre; items 1..136 are the other 136 keys
            for b in (near[i - 1] if i <= len(near) else rng.choice(bits, size=int(rng.integers(0, 3)), replace=False)):
                rB[i, b] = -rB[i, b]
    else:
        distinct = rng.integers(0, 2, size=(300 if name == "ties64" else 40, bits)) * 2 - 1
        rB = distinct[rng.integers(0, distinct.shape[0], size=n)]
    qB = rB[rng.integers(0, n, size=Q)].copy()
    for i in range(Q):
        for b in rng.choice(bits, size=(i + (0 if Q > 1 else 1)) % 4, replace=False):
            qB[i, b] = -qB[i, b]
    if name == "dense16":
        qB[0] = rB[0]                                             # the centre itself: its radius-2 ball is the whole database
    labels = lambda m: (rng.random((m, LOOKUP_CLASSES)) < 0.2).astype(np.float32)
    return rB.astype(np.float32), labels(n), qB.astype(np.float32), labels(Q)


def ref_lookup(qB, rB, radius, qL=None, rL=None):
    """Brute force over the unpacked codes -> (offsets int64 [Q+1], idx int32 [T], dist f32 [T], rel uint8 [T] or None): every item
    at distance (K - q.r) / 2 <= radius, by (distance, index)."""
    K = rB.shape[1]
    d = (K - qB.astype(np.int64) @ rB.astype(np.int64).T) // 2
    off, idx, dist, rel = [0], [], [], []
    for i in range(qB.shape[0]):
        j = np.nonzero(d[i] <= radius)[0]
        j = j[np.argsort(d[i, j], kind="stable")]
        idx.append(j)
        dist.append(d[i, j])
        if qL is not None:
            rel.append((rL[j] @ qL[i] > 0))
        off.append(off[-1] + j.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.array(off, dtype=np.int64), cat(idx, np.int32), cat(dist, np.float32), (cat(rel, np.uint8) if qL is not None else None)
