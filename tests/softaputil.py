"""mAP, R and rank sums of soft queries by counting (cmh_soft_ap / utils.retrieval.soft_mean_average_precision): the float64 NumPy
restatement and the inputs its tests share.

Per query: softutil.quantise -> softutil.wdist -> np.argsort(kind="stable") = ascending (wdist, database index); the relevant items'
positions p_1 < p_2 < ... < p_R (1-based) are their ranks, i is the relrank of the i-th;
  total = min(k, R),  AP = (1 / total) sum_{i <= total} i / p_i in float64 (0 when R = 0),  rank_sum = sum_i p_i over ALL i."""
import functools

import numpy as np

import mapcountutil as mu
import softutil


def restated(u, rB, qL, rL, ks, **broken):
    """-> ({k: ap float64 [Q]}, relevant int64 [Q], rank_sum int64 [Q]) of soft queries u f32 [Q, K]."""
    return restated_w(softutil.quantise(u)[0], rB, qL, rL, ks, **broken)


def restated_w(w, rB, qL, rL, ks, ties="stable", keep_all=False, use_k=True):
    """restated() from the integer weights w [Q, K].  The three switches BREAK a rule each (the host tests show that the
    restatement moves when they do): ties="reverse" puts equal distances in descending index order (a `>` where the order says
    `>=`), keep_all drops relrank <= total, use_k=False ignores k."""
    d, rel = softutil.wdist(w, rB), mu.relevance(qL, rL)
    Q, N = d.shape
    out = {k: np.zeros(Q, np.float64) for k in ks}
    rank_sum = np.zeros(Q, np.int64)
    for q in range(Q):
        order = np.argsort(d[q], kind="stable") if ties == "stable" else (N - 1 - np.argsort(d[q][::-1], kind="stable"))
        pos = np.nonzero(rel[q][order])[0].astype(np.int64) + 1
        rank_sum[q] = pos.sum()
        for k in ks:
            total = min(N if (k is None or not use_k) else k, len(pos))
            if total:
                used = pos if keep_all else pos[:total]
                out[k][q] = (np.arange(1, len(used) + 1, dtype=np.float64) / used.astype(np.float64)).sum() / total
    return out, rel.sum(1).astype(np.int64), rank_sum


def mean_f32(ap):
    """The f32 mean as cmh_map_mean forms it: a sequential f32 sum in query order, / Q."""
    acc = np.float32(0)
    for v in np.asarray(ap, np.float32):
        acc = np.float32(acc + v)
    return np.float32(acc / np.float32(len(ap)))


def labels(rng, Q, N, C):
    """mapcountutil.labels (the last query has no label: R = 0), and, for Q >= 3, the query before it carries EVERY class while every
    database item carries at least one: R = N."""
    qL, rL = mu.labels(rng, Q, N, C)
    rL[np.arange(N), rng.integers(C, size=N)] = 1.0
    if Q >= 3:
        qL[-2] = 1.0
    return qL, rL


def soft_queries(rng, Q, bits, style):
    """style "tanh": a tanh head's output; "coarse": entry 0 is 1 and the others lie in {0, +-1/15}: weights 15 and {0, +-1} (heavy
    ties: the quantiser always maps the largest entry to 15).  For Q >= 2 query 0 is all zeros (everything ties at 0)."""
    if style == "tanh":
        u = np.tanh(rng.normal(size=(Q, bits))).astype(np.float32)
    elif style == "coarse":
        u = (rng.integers(-1, 2, size=(Q, bits)).astype(np.float32) / np.float32(15)).astype(np.float32)
        u[:, 0] = 1.0
    else:
        raise ValueError(style)
    if Q >= 2:
        u[0] = 0.0
    return u


@functools.lru_cache(maxsize=None)
def case(Q, N, bits, zeros, C, style="tanh", seed=0):
    """-> (u, rB, qL, rL), built once per shape, read-only."""
    rng = np.random.default_rng([Q, N, bits, int(zeros), C, seed, len(style)])
    qL, rL = labels(rng, Q, N, C)
    out = soft_queries(rng, Q, bits, style), mu.codes(rng, N, bits, zeros), qL, rL
    for a in out:
        a.setflags(write=False)
    return out


def k_values(qL, rL):
    """None, 1, 50, N, one above the largest R of a query with R < N (k > R), each cut to [1, N]."""
    N = rL.shape[0]
    R = mu.relevance(qL, rL).sum(1)
    above = int(R[R < N].max()) + 1 if (R < N).any() else N
    return tuple(dict.fromkeys(k if k is None else max(1, min(N, k)) for k in (None, 1, 50, N, above)))


@functools.lru_cache(maxsize=None)
def case_reference(Q, N, bits, zeros, C, style="tanh", seed=0):
    u, rB, qL, rL = case(Q, N, bits, zeros, C, style, seed)
    return restated(u, rB, qL, rL, k_values(qL, rL))


def mixed_slabs(u, rB, qL, rL):
    """How many (query, 64-item slab, bin) hold both a relevant and a non-relevant item: what the second walk's two ballots differ on."""
    w, _, _ = softutil.quantise(u)
    d, rel = softutil.wdist(w, rB), mu.relevance(qL, rL)
    count = 0
    for q in range(d.shape[0]):
        for a in range(0, d.shape[1], 64):
            dd, rr = d[q, a:a + 64], rel[q, a:a + 64]
            hit, miss = set(dd[rr].tolist()), set(dd[~rr].tolist())
            count += len(hit & miss)
    return count


def check_mix(u, rB, qL, rL):
    """What a case with Q >= 3 and N >= 64 must hold: a query with R = 0, one with R = N, an all-zero query, and bins that hold
    relevant and non-relevant items within one slab (more than one class: with one, every labelled item is relevant to every labelled
    query)."""
    R = mu.relevance(qL, rL).sum(1)
    assert (R == 0).any() and (R == rL.shape[0]).any(), R
    assert not u[0].any()
    assert qL.shape[1] == 1 or mixed_slabs(u, rB, qL, rL) > 0
