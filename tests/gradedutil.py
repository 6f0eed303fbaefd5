"""A NumPy restatement of the graded-relevance metrics (NDCG@n, ACG@n, WAP@n), written for the tests: direct float64 loops over the
definitions in utils/retrieval.py's docstring, and the ideal DCG from the SORTED grades of the whole database, deliberately another
route than the histogram walk of utils.retrieval.graded_from_grades."""
import numpy as np


def hamming(qB, rB):
    """calc_hammingDist (utils/calc_utils.py:8-13) in float64: exact for codes in {-1, 0, +1}."""
    return 0.5 * (rB.shape[1] - qB.astype(np.float64) @ rB.astype(np.float64).T)


def grades(qL, rL):
    """The matrix calc_neighbor thresholds: shared labels of every (query, database item)."""
    return np.rint(qL.astype(np.float64) @ rL.astype(np.float64).T).astype(np.int64)


def ranking(qB, rB, k):
    """The first k columns of the ranking by (distance, database index)."""
    return np.argsort(hamming(qB, rB), axis=1, kind="stable")[:, :k]


def per_query(ranked, all_grades, n):
    """ranked: the grades of one query's ranking (at least n of them); all_grades: its grades against the whole database.
    -> (ndcg, acg, wap) at n; ndcg is None for a query without relevant items."""
    ranked = [int(v) for v in ranked[:n]]
    acg_sum, dcg, wap_sum, hits = 0.0, 0.0, 0.0, 0
    for i, g in enumerate(ranked, start=1):
        acg_sum += g
        dcg += (2.0 ** g - 1.0) / np.log2(i + 1.0)
        if g > 0:
            hits += 1
            wap_sum += acg_sum / i
    ideal = np.sort(np.asarray(all_grades, dtype=np.int64))[::-1][:n]
    idcg = 0.0
    for i, g in enumerate(ideal, start=1):
        idcg += (2.0 ** int(g) - 1.0) / np.log2(i + 1.0)
    return (dcg / idcg if idcg > 0 else None), acg_sum / n, (wap_sum / hits if hits else 0.0)


def metrics(ranked_grades, all_grades, topn):
    """ranked_grades [Q, k], all_grades [Q, N] -> (ndcg, acg, wap) float64 [len(topn)]: means over the queries that have at least
    one relevant database item; zeros when no query has one."""
    keep = [q for q in range(all_grades.shape[0]) if (all_grades[q] > 0).any()]
    out = np.zeros((3, len(topn)))
    if not keep:
        return out[0], out[1], out[2]
    for b, n in enumerate(topn):
        rows = [per_query(ranked_grades[q], all_grades[q], n) for q in keep]
        out[:, b] = np.mean(np.asarray(rows, dtype=np.float64), axis=0)
    return out[0], out[1], out[2]


def histogram(all_grades, classes):
    """grade_counts [Q, classes+1] of a grade matrix."""
    return np.stack([np.bincount(row, minlength=classes + 1) for row in all_grades])
