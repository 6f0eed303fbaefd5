"""NumPy restatement of multi-index hashing on 16-bit substrings (csrc/retrieval_mih.hip, utils/retrieval.py::SubstringTables) and
the cases its tests share.  No GPU code is imported here.

A code of `bits` entries in {-1, +1} is packed as pack_codes packs it: entry t is bit t % 32 of word t // 32, set for +1.  m =
ceil(bits / 16); substring j is bits [16 j, 16 j + s_j) of the packed words, s_j = 16 but for a shorter last one.  For a radius r,
a, b = divmod(r, m) and substring j is probed at radius a_j = a for j <= b, a - 1 behind (-1: not probed).  Item x reached through
substring j is emitted iff d(q, x) <= r and no probed j' < j has d_j'(q, x) <= a_j'."""
import numpy as np

SUB = 16
CLASSES = 5

# (bits, n, centres, p, radii): the radii sit on every change of (a, b); 24 and 40 bit have a short last substring (at 24 bit
# unprobed at radius 0, probed from radius 1 on); radii below m - 1 leave substrings unprobed
CASES = [
    (16, 300, 6, 0.04, (0, 1, 2)),
    (24, 1000, 8, 0.05, (0, 2, 3, 5)),
    (32, 5000, 16, 0.05, (0, 1, 2, 5)),
    (40, 3000, 10, 0.06, (2, 3, 8)),
    (64, 20000, 40, 0.06, (0, 3, 4, 7, 8, 11)),
    (128, 20000, 40, 0.06, (7, 8, 15, 16, 23)),
]
CASE = {c[0]: c for c in CASES}
POINTS = [(c[0], r) for c in CASES for r in c[4]]


def subs(bits):
    return (bits + SUB - 1) // SUB


def sub_width(bits, j):
    return min(SUB, bits - SUB * j)


def radii(bits, r):
    """The rule's substring radii, restated (utils.retrieval.substring_radii is checked against a hand table and against this)."""
    m = subs(bits)
    a, b = divmod(r, m)
    return [a if j <= b else a - 1 for j in range(m)]


def gen(n, bits, centres, p, seed):
    """-> (database uint8 [n, bits], queries uint8 [11, bits]) in {0, 1}: centres uniform, every item a random centre with each bit
    flipped with probability p; the queries are the first 6 centres with each bit flipped with probability p, 3 uniform random
    codes and the first 2 database items."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 2, size=(centres, bits))
    db = centre[rng.integers(0, centres, size=n)] ^ (rng.random((n, bits)) < p)
    near = centre[:6] ^ (rng.random((6, bits)) < p)
    far = rng.integers(0, 2, size=(3, bits))
    return db.astype(np.uint8), np.concatenate([near, far, db[:2]]).astype(np.uint8)


_made = {}


def case(bits):
    """-> (database, queries) of the case of that length, made once and shared (callers do not write into them)."""
    if bits not in _made:
        _, n, centres, p, _ = CASE[bits]
        _made[bits] = gen(n, bits, centres, p, seed=bits)
        for a in _made[bits]:
            a.setflags(write=False)
    return _made[bits]


def codes(b01):
    """{0, 1} -> f32 {-1, +1}: what the retrieval functions take."""
    return (b01.astype(np.float32) * 2 - 1)


def labels(n, seed):
    """5-class multi-hot f32 [n, 5]."""
    return (np.random.default_rng(seed).random((n, CLASSES)) < 0.3).astype(np.float32)


def pack(b01, garbage_seed=None):
    """{0, 1} [n, bits] -> uint32 [n, W] as pack_codes' sign plane; garbage_seed: random bits behind `bits` (they must not matter)."""
    n, bits = b01.shape
    W = (bits + 31) // 32
    padded = np.zeros((n, 32 * W), dtype=np.uint64)
    padded[:, :bits] = b01
    words = (padded.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    if garbage_seed is not None and bits % 32:
        junk = np.random.default_rng(garbage_seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        words[:, -1] |= junk & ~np.uint32((1 << (bits % 32)) - 1)
    return words


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(-1).astype(np.int64)


def sub_dists(qw, dw, bits, cut_width=True):
    """One query's packed words [W] against the database's [n, W] -> int64 [m, n]: the distance inside every substring.
    cut_width=False ignores the width of a short last substring (takes 16 bits of the word whatever lies behind `bits`)."""
    x = (dw ^ qw[None, :]).astype(np.uint32)
    out = []
    for j in range(subs(bits)):
        part = (x[:, j // 2] >> np.uint32(SUB * (j % 2))) & np.uint32(0xFFFF)
        if cut_width:
            part = part & np.uint32((1 << sub_width(bits, j)) - 1)
        out.append(_popcount(part.astype(np.uint32).reshape(-1, 1)))
    return np.stack(out)


def brute(qw, dw, bits, r):
    """-> per query (idx int64, dist int64) of the items within r, ordered by (distance, index)."""
    out = []
    for q in qw:
        d = sub_dists(q, dw, bits).sum(0)
        j = np.nonzero(d <= r)[0]
        j = j[np.argsort(d[j], kind="stable")]
        out.append((j, d[j]))
    return out


def rule(qw, dw, bits, r, once=True, sub_radii=None, cut_width=True):
    """The rule restated -> per query (idx, dist) in emission order (substring, then index): per probed substring the items with
    d_j <= a_j, minus those an earlier probed substring reaches (once=False drops that), cut at d <= r.  sub_radii overrides the
    rule's radii; cut_width as in sub_dists (the full distance then counts the bits behind `bits` too)."""
    a = radii(bits, r) if sub_radii is None else sub_radii
    out = []
    for q in qw:
        dj = sub_dists(q, dw, bits, cut_width)
        d = dj.sum(0)
        seen = np.zeros(dw.shape[0], dtype=bool)
        idx = []
        for j, aj in enumerate(a):
            if aj < 0:
                continue
            reach = dj[j] <= aj
            idx.append(np.nonzero(reach & (d <= r) & ~(seen if once else False))[0])
            seen |= reach
        idx = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
        out.append((idx, d[idx]))
    return out


def ordered(lists):
    """Emission order -> (distance, index) order."""
    out = []
    for idx, d in lists:
        by = np.lexsort((idx, d))
        out.append((idx[by], d[by]))
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
