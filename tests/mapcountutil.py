"""mAP by counting (cmh_hamming_ap_partial / utils.retrieval.mean_average_precision): test inputs and the float64 restatement of the
reference's AP (utils/calc_utils.py:26-38) on a stable argsort: NumPy only, every term relrank / rank in float64."""
import functools

import numpy as np


def half_units(qB, rB):
    """h = K - q.r of calc_hammingDist (2 * distance), exact integers."""
    return rB.shape[1] - qB.astype(np.int64) @ rB.astype(np.int64).T


def relevance(qL, rL):
    return (qL.astype(np.int64) @ rL.astype(np.int64).T) > 0


def restated_ap(qB, rB, qL, rL, ks):
    """-> {k: (ap float64 [Q], map float64)} for every k of ks (None = N).  Ties by ascending database index."""
    h, rel = half_units(qB, rB), relevance(qL, rL)
    Q, N = h.shape
    out = {k: np.zeros(Q, np.float64) for k in ks}
    for q in range(Q):
        hits = rel[q][np.argsort(h[q], kind="stable")]
        pos = np.nonzero(hits)[0].astype(np.float64) + 1.0               # ranks of the relevant items, ascending
        for k in ks:
            total = min(N if k is None else k, len(pos))
            if total:
                out[k][q] = (np.arange(1, total + 1, dtype=np.float64) / pos[:total]).sum() / total
    return {k: (ap, float(ap.mean())) for k, ap in out.items()}


def codes(rng, n, bits, zeros):
    B = rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, bits))
    if zeros:
        B[rng.random((n, bits)) < 0.1] = 0.0                            # zero entries: odd half-units
    return B


def labels(rng, Q, N, C):
    """Multi-hot labels of density 0.3 (queries) and 0.2 (database) at C = 4, scaled by sqrt(4 / C) so that a pair shares a label
    about as often at any C.  Then made to hold what the tests assert: the last query has no label at all (no relevant item);
    database item 0 has a label, and the first ceil(Q / 2) queries (all but the last) share it (at least half the queries have a
    relevant item, also when N = 1).  Q = 1 cannot hold both: its one query keeps its relevant item."""
    s = (4.0 / C) ** 0.5
    qL = (rng.random((Q, C)) < 0.3 * s).astype(np.float32)
    rL = (rng.random((N, C)) < 0.2 * s).astype(np.float32)
    c0 = int(rng.integers(C))
    rL[0, c0] = 1.0
    qL[:(Q + 1) // 2, c0] = 1.0
    if Q > 1:
        qL[-1] = 0.0
    return qL, rL


@functools.lru_cache(maxsize=None)
def case(Q, N, bits, zeros, C, seed=0):
    """-> (qB, rB, qL, rL): built once per shape and shared by the tests that use it (nobody writes into them)."""
    rng = np.random.default_rng([Q, N, bits, int(zeros), C, seed])
    qL, rL = labels(rng, Q, N, C)
    out = codes(rng, Q, bits, zeros), codes(rng, N, bits, zeros), qL, rL
    for a in out:
        a.setflags(write=False)
    return out


def k_values(qL, rL):
    """None, 1, 5, 50, one above the largest number of relevant items of any query (k > R), ten times the database (k > N)."""
    N = rL.shape[0]
    return (None, 1, 5, 50, int(relevance(qL, rL).sum(1).max()) + 1, 10 * N)


@functools.lru_cache(maxsize=None)
def case_reference(Q, N, bits, zeros, C, seed=0):
    qB, rB, qL, rL = case(Q, N, bits, zeros, C, seed)
    return restated_ap(qB, rB, qL, rL, k_values(qL, rL))


def check_label_mix(qL, rL):
    """What every case must hold: at least half the queries have a relevant item, and (Q > 1) at least one has none."""
    has = relevance(qL, rL).any(1)
    assert 2 * int(has.sum()) >= len(has), (int(has.sum()), len(has))
    assert len(has) == 1 or not has.all()
