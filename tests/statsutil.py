"""NumPy restatement of the code diagnostics (utils/code_stats.py, cmh_code_gram) from FLOAT codes in {-1, 0, +1}: nothing here is
packed and nothing is derived from the integers the implementation uses - the correlation is the textbook one over centred columns,
the mutual information counts items one by one."""
import numpy as np


def codes(n, K, seed, zeros=0.0, pattern="random"):
    """f32 [n, K]: random signs, a share `zeros` of the entries 0; or a constant pattern."""
    if pattern in ("plus", "minus", "zero"):
        return np.full((n, K), {"plus": 1.0, "minus": -1.0, "zero": 0.0}[pattern], dtype=np.float32)
    rng = np.random.default_rng(seed)
    B = np.where(rng.random((n, K)) < 0.5, -1.0, 1.0).astype(np.float32)
    if zeros:
        B[rng.random((n, K)) < zeros] = 0.0
    return B


def labels(n, C, seed, p=0.3):
    rng = np.random.default_rng(seed + 77)
    return (rng.random((n, C)) < p).astype(np.float32)


def gram(A, B):
    """-> (gram, a_sum, a_abs, b_sum, b_abs) as int64, the outputs of cmh_code_gram."""
    a, b = np.rint(A).astype(np.int64), np.rint(B).astype(np.int64)
    return a.T @ b, a.sum(0), np.abs(a).sum(0), b.sum(0), np.abs(b).sum(0)


def entropy(A):
    """Per bit, in bits, over the symbols +1, -1, 0."""
    out = np.zeros(A.shape[1])
    for sym in (1.0, -1.0, 0.0):
        p = (A == sym).mean(0)
        out -= np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0)
    return out


def correlation(A, B=None):
    """Pearson's correlation of the columns of A with those of B (np.corrcoef's arithmetic over centred float64 columns), with
    the dead-bit rule: 0 where either column is constant.  -> (corr, variances of A's columns)."""
    X = A.astype(np.float64)
    Y = X if B is None else B.astype(np.float64)
    xc, yc = X - X.mean(0), Y - Y.mean(0)
    cov = xc.T @ yc / X.shape[0]
    vx, vy = (xc * xc).mean(0), (yc * yc).mean(0)
    dead_x, dead_y = (X == X[0]).all(0), (Y == Y[0]).all(0)
    den = np.sqrt(np.outer(vx, vy))
    corr = np.where(np.outer(~dead_x, ~dead_y), cov / np.where(den > 0, den, 1.0), 0.0)
    return corr, vx, dead_x


def class_tables(L, A):
    """-> (class_bit_mean [C, K], MI [C, K] in bits between the symbol of a bit and the membership of a class), by counting items."""
    n, C = L.shape
    K = A.shape[1]
    mean, mi = np.zeros((C, K)), np.zeros((C, K))
    for c in range(C):
        member = L[:, c] > 0
        if member.any():
            mean[c] = A[member].astype(np.float64).mean(0)
        for k in range(K):
            for sym in (1.0, -1.0, 0.0):
                for m in (True, False):
                    joint = int(((A[:, k] == sym) & (member == m)).sum())
                    ps, pm = int((A[:, k] == sym).sum()), int((member == m).sum())
                    if joint:
                        mi[c, k] += joint / n * np.log2(joint * n / (ps * pm))
    return mean, mi


def stats(A, paired=None, L=None):
    """The dict of utils.code_stats.stats_from_counts, restated."""
    n, K = A.shape
    corr, var, dead = correlation(A)
    live = [i for i in range(K) if not dead[i]]
    for i in live:
        corr[i, i] = 1.0
    off = [abs(corr[i, j]) for x, i in enumerate(live) for j in live[x + 1:]]
    mean = A.astype(np.float64).mean(0)
    dup = [(i, j) for x, i in enumerate(live) for j in live[x + 1:]
           if (A[:, i] == A[:, j]).all() or (A[:, i] == -A[:, j]).all()]
    out = {"bit_mean": mean, "bit_bias": np.abs(mean), "balance": float(np.abs(mean).mean()), "bit_entropy": entropy(A),
           "dead_bits": [i for i in range(K) if dead[i]], "corr": corr, "mean_abs_corr": float(np.mean(off)) if off else 0.0,
           "max_abs_corr": float(np.max(off)) if off else 0.0, "duplicate_bits": dup, "live_variance": var[live]}
    if paired is not None:
        dot = (A.astype(np.float64) * paired.astype(np.float64)).sum(0)
        out.update({"pair_dot": np.rint(dot).astype(np.int64), "bit_agreement": (1.0 + dot / n) / 2.0,
                    "mean_agreement": float(((1.0 + dot / n) / 2.0).mean()),
                    "pair_distance": float((0.5 * (K - (A.astype(np.float64) * paired).sum(1))).mean()),
                    "cross_corr": correlation(A, paired)[0]})
    if L is not None:
        cbm, mi = class_tables(L, A)
        out.update({"class_bit_mean": cbm, "bit_class_mi": mi, "best_class_mi": mi.max(0)})
    return out
