"""NumPy restatement of the soft-query search (csrc/retrieval_soft.hip, utils/retrieval.py::soft_topk) and the inputs its tests share.

Quantiser, per row u (np.float32, finite): s = max |u_i|; s == 0: w = 0; else w_i = rint((u_i / s) * 15), every operation in
np.float32 and rounded once (IEEE division, IEEE multiplication, round half to even).  wsum = sum |w_i|, scale = s.
Distance to an item r in {-1, 0, +1}^K: wdist = sum |w_i| - r . w, an integer in [0, 2 wsum].
Ranking: np.argsort(wdist, kind="stable")[:, :k]: ascending (wdist, database index).
dist = np.float32(wdist) * (scale / np.float32(30))."""
import numpy as np

LEVELS = 15


def quantise(u):
    """u f32 [Q, K] -> (w int64 [Q, K], wsum int64 [Q], scale f32 [Q])."""
    u = np.asarray(u, np.float32)
    assert np.isfinite(u).all()
    s = np.abs(u).max(axis=1)
    w = np.zeros(u.shape, np.int64)
    with np.errstate(all="ignore"):
        for q in range(u.shape[0]):
            if s[q] != 0:
                ratio = (u[q] / s[q]).astype(np.float32)
                w[q] = np.rint((ratio * np.float32(LEVELS)).astype(np.float32)).astype(np.int64)
    return w, np.abs(w).sum(axis=1), s.astype(np.float32)


def planes(w):
    """w int [Q, K] -> (q_sign int32 [Q, W], q_mag int32 [Q, 4, W]) as cmh_soft_query_planes lays them out: bit i % 32 of word
    i // 32; sign bit set where w_i > 0, plane b = bit b of |w_i|; zeros at and behind K."""
    Q, K = w.shape
    W = (K + 31) // 32
    sign, mag = np.zeros((Q, W), np.uint32), np.zeros((Q, 4, W), np.uint32)
    for i in range(K):
        bit = np.uint32(1 << (i % 32))
        sign[:, i // 32] |= np.where(w[:, i] > 0, bit, np.uint32(0))
        for b in range(4):
            mag[:, b, i // 32] |= np.where((np.abs(w[:, i]) >> b) & 1, bit, np.uint32(0))
    return sign.view(np.int32), mag.view(np.int32)


def wdist(w, rB):
    """w int64 [Q, K], rB codes [n, K] in {-1, 0, +1} -> int64 [Q, n]."""
    return np.abs(w).sum(axis=1)[:, None] - (np.asarray(rB).astype(np.int64) @ w.T).T


def topk(u, rB, k):
    """-> (idx int32 [Q, k], wdist int32 [Q, k], dist f32 [Q, k])."""
    w, _, scale = quantise(u)
    d = wdist(w, rB)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    wd = np.take_along_axis(d, order, 1)
    return order.astype(np.int32), wd.astype(np.int32), wd.astype(np.float32) * (scale / np.float32(30))[:, None]


def queries(Q, K, seed):
    """Random soft queries: tanh of normal draws, the shape of a tanh head's output."""
    return np.tanh(np.random.default_rng(seed).normal(size=(Q, K))).astype(np.float32)
