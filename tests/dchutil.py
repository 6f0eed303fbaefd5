"""NumPy fp64 restatement of the supervised training-free fit (csrc/dch.hip, utils/dch.py): discrete cross-modal hashing on frozen
features (DCH, Xu et al., TIP 2017; the cross-modal form of SDH, Shen et al., CVPR 2015) as DESIGN.md §7.11 states it - the PCAH
start, the ridge regressions of B on each modality, the label regression W, the bit-cyclic coordinate descent with "t == 0 keeps the
bit", the heads - with LAPACK (eigh, solve) where the product runs Jacobi and Cholesky, so the two share no arithmetic.  The
coordinate descent itself is the product's chain, term for term (acc = q_l, then acc -= b_k G[k][l] for k ascending, k != l; b_k G is
exact, so a subtraction is the kernel's fma), which is what lets the kernel test ask for the same smallest |t|.  Also the labelled
fixture generator, the retrieval score and the bounds the tests use."""
import numpy as np

import itqutil as IU

EPS = IU.EPS

# (N_fit, D, C, K, seed): generated with n = N_fit + HELD_OUT; the first N_fit rows are the fit set and the database, the last
# HELD_OUT rows the queries.  tests/test_dch_host.py asserts that every decision of these fits stands 1e-9 or more from zero.
FIXTURES = [(300, 24, 5, 8, 1), (517, 40, 7, 16, 2), (1000, 64, 10, 32, 3)]
HELD_OUT = 200
MARGIN_FLOOR = 1e-9


def make_labelled(n, d, c, seed):
    rng = np.random.default_rng(seed)
    spec = 1.0 / (1.0 + 0.15 * np.arange(d))
    rot = np.linalg.qr(rng.standard_normal((d, d)))[0]
    Y = (rng.random((n, c)) < 0.18).astype(np.float64)
    for i in np.where(Y.sum(1) == 0)[0]:
        Y[i, rng.integers(c)] = 1
    proto = 0.6 * rng.standard_normal((c, d)) * spec
    nuis = 2.0 * rng.standard_normal((6, d)) * spec
    latent = Y @ proto + nuis[rng.integers(6, size=n)] + rng.standard_normal((n, d)) * spec
    xi = (latent + 0.3 * rng.standard_normal((n, d)) * spec) @ rot.T + 8.0 * rng.standard_normal(d)
    xt = (0.8 * latent + 0.4 * rng.standard_normal((n, d)) * spec) @ rot.T + 8.0 * rng.standard_normal(d)
    return xi.astype(np.float32), xt.astype(np.float32), Y


def fixture(fix):
    """-> (fit features and labels, held-out features and labels) of a FIXTURES row."""
    n, d, c, _, seed = fix
    xi, xt, y = make_labelled(n + HELD_OUT, d, c, seed)
    return (xi[:n], xt[:n], y[:n]), (xi[n:], xt[n:], y[n:])


# ---- the coordinate descent -------------------------------------------------------------------------------------------------------
def dcc(q, g, b, rounds, keep_on_zero=True):
    """`rounds` Gauss-Seidel rounds over the bits of every item.  q [N, K] (the targets), g [K, K], b [N, K] of +-1 ->
    (the new b, flips per round [rounds] int64, the smallest |t| over all decisions).  t = q_l - sum_{k != l} b_k g[k][l], the sum
    taken as the chain the kernel runs; t > 0 sets +1, t < 0 sets -1, t == 0 keeps the bit (keep_on_zero = False: the rule the
    product does NOT use, t == 0 sets +1, for the test that tells the two apart)."""
    b = np.array(b, dtype=np.float64)
    n, k = b.shape
    flips = np.zeros(rounds, dtype=np.int64)
    least = np.inf
    for r in range(rounds):
        for l in range(k):
            acc = np.array(q[:, l], dtype=np.float64)
            for j in range(k):
                if j != l:
                    acc = acc - b[:, j] * g[j, l]
            if n:
                least = min(least, float(np.abs(acc).min()))
            new = np.where(acc > 0, 1.0, np.where(acc < 0, -1.0, b[:, l] if keep_on_zero else 1.0))
            flips[r] += int((new != b[:, l]).sum())
            b[:, l] = new
    return b, flips, least


# ---- the pieces of one iteration --------------------------------------------------------------------------------------------------
def label_regression(b, y, lam):
    """W [K, C] = (B^T B + lam I)^-1 B^T Y."""
    k = b.shape[1]
    return np.linalg.solve(b.T @ b + lam * np.eye(k), b.T @ y)


def objective(y, b, w, z_i, z_t, lam, mu):
    return float(((y - b @ w) ** 2).sum() + lam * (w ** 2).sum() + mu * (((b - z_i) ** 2).sum() + ((b - z_t) ** 2).sum()))


def targets(y, w, z_i, z_t, mu):
    """Q [N, K] = Y W^T + mu Z_i + mu Z_t, summed in that order."""
    return (y @ w.T + mu * z_i) + mu * z_t


def fit(fi, ft, y, bits, iters=10, rounds=3, lam=1.0, mu=0.01, reg=0.1):
    """The whole fit.  Besides the product's outputs: min_start (the smallest |x_i P0 + x_t P0| entry of the start), min_margin
    [iters], flips [iters, rounds], Z [2N, K] (both modalities' regressions of the final B) and codes = sign(Z)."""
    n, d = fi.shape
    y = np.asarray(y, dtype=np.float64)
    mu_i, mu_t, alpha, cov = IU.covariance(IU.moments(fi), IU.moments(ft), n)
    x, s = [], []
    for f, m, a in ((fi, mu_i, alpha[0]), (ft, mu_t, alpha[1])):
        xm = a * (np.asarray(f, dtype=np.float64) - m)
        x.append(xm)
        s.append(xm.T @ xm / n + (reg / d) * np.eye(d))               # S_mm + (reg / D) I

    def regress(b):
        p = [np.linalg.solve(s[m], x[m].T @ b / n) for m in range(2)]
        return p, [x[m] @ p[m] for m in range(2)]

    p0 = IU.eigh(cov)[1][:, :bits].copy()
    start = x[0] @ p0 + x[1] @ p0
    b = np.where(start >= 0, 1.0, -1.0)
    obj, flips, margins = [], [], []
    for _ in range(iters):
        p, z = regress(b)
        w = label_regression(b, y, lam)
        obj.append(objective(y, b, w, z[0], z[1], lam, mu))
        b, fl, least = dcc(targets(y, w, z[0], z[1], mu), w @ w.T, b, rounds)
        flips.append(fl)
        margins.append(least)
    p, z = regress(b)
    w = label_regression(b, y, lam)
    obj.append(objective(y, b, w, z[0], z[1], lam, mu))
    zz = np.concatenate(z)
    scale = 0.5 / np.sqrt((zz ** 2).mean())
    out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "B": b, "P_i": p[0], "P_t": p[1], "W": w, "Z": zz, "scale": scale,
           "codes": np.where(zz >= 0, 1.0, -1.0), "objective": np.array(obj), "flips": np.array(flips, dtype=np.int64).reshape(iters, rounds),
           "min_margin": np.array(margins), "min_start": float(np.abs(start).min())}
    for side, a, m, pm in (("i", alpha[0], mu_i, p[0]), ("t", alpha[1], mu_t, p[1])):
        head = scale * a * pm.T
        out[f"W_{side}"], out[f"b_{side}"] = head, -head @ m
    return out


# ---- retrieval score --------------------------------------------------------------------------------------------------------------
def head_codes(f, w, b):
    return np.where(np.asarray(f, dtype=np.float64) @ w.T + b >= 0, 1.0, -1.0)


def mean_average_precision(q_codes, q_labels, db_codes, db_labels):
    """mAP over the whole database, Hamming ranking (ties in database order); an item is relevant where it shares a label."""
    dist = 0.5 * (q_codes.shape[1] - q_codes @ db_codes.T)
    rel = (q_labels @ db_labels.T) > 0
    aps = []
    for i in range(q_codes.shape[0]):
        r = rel[i][np.argsort(dist[i], kind="stable")]
        if r.any():
            hits = np.cumsum(r)
            aps.append(float((hits[r] / (np.flatnonzero(r) + 1.0)).mean()))
    return float(np.mean(aps))


def held_out_map(heads, fit_set, queries):
    """(image -> text, text -> image) mAP of the held-out queries against the fit set's codes, all through the heads."""
    db_i, db_t = head_codes(fit_set[0], heads["W_i"], heads["b_i"]), head_codes(fit_set[1], heads["W_t"], heads["b_t"])
    q_i, q_t = head_codes(queries[0], heads["W_i"], heads["b_i"]), head_codes(queries[1], heads["W_t"], heads["b_t"])
    return mean_average_precision(q_i, queries[2], db_t, fit_set[2]), mean_average_precision(q_t, queries[2], db_i, fit_set[2])


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def order_bound(n_terms, abs_terms_sum):
    """The summation-order bound of a sum of n terms: 8 n eps sum|terms| (tests/test_gpu_itq.py's)."""
    return 8 * n_terms * EPS * abs_terms_sum


def random_codes(n, k, seed):
    return np.where(np.random.default_rng(seed).random((n, k)) < 0.5, 1.0, -1.0)


def dcc_case(n, k, seed, rounds=(1, 3)):
    """(Q, G, B0, {rounds: the restatement's (B, flips, smallest |t|)}) of a coordinate-descent problem: G = W W^T of a random
    W [K, 6] (symmetric bit for bit), Q the size of a label regression's targets.  Redrawn from seed + 1000 j until the
    restatement's smallest |t| is MARGIN_FLOOR or more for every number of rounds asked."""
    for j in range(50):
        rng = np.random.default_rng(seed + 1000 * j)
        w = rng.standard_normal((k, 6)) / np.sqrt(k)
        g = np.array([[float(np.dot(w[a], w[b])) if a <= b else 0.0 for b in range(k)] for a in range(k)])
        g = np.triu(g) + np.triu(g, 1).T
        q = rng.standard_normal((n, k))
        b0 = random_codes(n, k, seed + 7 + 1000 * j)
        refs = {r: dcc(q, g, b0, r) for r in rounds}
        if all(ref[2] >= MARGIN_FLOOR for ref in refs.values()):
            return q, g, b0, refs
    raise AssertionError(f"no robust draw for ({n}, {k}, {seed})")
