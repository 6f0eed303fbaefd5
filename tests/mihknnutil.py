"""NumPy restatement of the k-nearest search through the substring tables (csrc/retrieval_mih.hip: cmh_mih_knn_count / _fill;
utils/retrieval.py::knn_steps, SubstringTables.topk) and the draws its tests share.  No GPU code is imported here.

Growth step s = t m + j probes substring j at exactly level t; an item reached through (j, t = d_j) counts iff d_j' m + j' >
t m + j for every j' != j; r* = the smallest r <= r_cap with |ball(r)| >= k, decided after step r."""
import numpy as np

import mihutil as U


def distances(qw, dw, bits):
    """One query's packed words against the database's -> (d_j int64 [m, n], d int64 [n])."""
    dj = U.sub_dists(qw, dw, bits)
    return dj, dj.sum(0)


def walk(dj, d, steps, r_cap):
    """The first-reach rule along `steps` (knn_steps' list) -> per step the items that count there (d <= r_cap), ascending."""
    m = dj.shape[0]
    out = []
    for j, t in steps:
        first = dj[j] == t
        for other in range(m):
            if other != j:
                first &= dj[other] * m + other > t * m + j
        out.append(np.nonzero(first & (d <= r_cap))[0])
    return out


def stop(d, reached, k, r_cap):
    """(r*, n_ball, n_less) as the count pass decides them: after step r the items at every distance <= r are complete."""
    at = np.zeros(r_cap + 1, dtype=np.int64)
    ball = 0
    for r in range(r_cap + 1):
        at += np.bincount(d[reached[r]], minlength=r_cap + 1)[:r_cap + 1]
        less, ball = ball, ball + int(at[r])
        if ball >= k:
            return r, ball, less
    return -1, ball, ball


def brute(d, k, r_cap):
    """(r*, n_ball, n_less) by counting whole balls."""
    for r in range(r_cap + 1):
        if int((d <= r).sum()) >= k:
            return r, int((d <= r).sum()), int((d < r).sum())
    return -1, int((d <= r_cap).sum()), int((d <= r_cap).sum())


def flipped(rng, rows, flips):
    """Rows of a {0, 1} array with flips[i % len(flips)] distinct bits of row i flipped (at most the row's length)."""
    out = rows.copy()
    for i in range(out.shape[0]):
        f = min(flips[i % len(flips)], out.shape[1])
        out[i, rng.choice(out.shape[1], size=f, replace=False)] ^= 1
    return out


def draw(n, bits, seed, copies=0):
    """-> database uint8 [n, bits] in {0, 1}: one half uniform, one half 8 centres with every bit flipped with probability 0.04,
    shuffled; the first `copies` rows (before the shuffle) are one and the same code."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 2, size=(8, bits))
    near = centre[rng.integers(0, 8, size=n)] ^ (rng.random((n, bits)) < 0.04)
    db = np.where((np.arange(n) % 2 == 0)[:, None], rng.integers(0, 2, size=(n, bits)), near)
    db[:copies] = centre[0]
    return db[rng.permutation(n)].astype(np.uint8)


def queries(db, Q, seed):
    """Q queries: database rows (spread over the database) with 0, 1, 2, 3 bits flipped in turn."""
    rng = np.random.default_rng(seed)
    rows = db[(np.arange(Q) * max(1, db.shape[0] // Q)) % db.shape[0]]
    return flipped(rng, rows, [0, 1, 2, 3])
