"""NumPy fp64 restatement of the training-free fit (csrc/itq.hip, utils/itq.py): moments, pooled covariance, projection, the ITQ
iteration, the heads - with the product's conventions (eigenvalues descending, each vector's largest entry positive, B = +1 where
Z >= 0, R <- (polar factor of B^T V)^T) but LAPACK where the product runs Jacobi, so the two share no arithmetic.  Also the fixture
generator and the error bounds the tests use."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

# (N, D, K, seed): the fixtures whose codes survive a perturbation of C by 1e-10 max|C| (tests/test_itq_host.py asserts it), so
# the GPU fit must reproduce the restatement's codes exactly
FIXTURES = [(300, 24, 8, 1), (517, 40, 16, 2), (1000, 64, 32, 3)]


def make_pair(n, d, seed, clusters=6):
    """Paired image / text features f32 [n, d]: clustered Gaussian data with a decaying spectrum behind a random rotation, the text
    side a noisier, damped view of the same latent, plus an offset per modality that is large against the spread."""
    rng = np.random.default_rng(seed)
    spec = 1.0 / (1.0 + 0.15 * np.arange(d))      # standard deviations: the eigenvalue gaps stay far above the perturbation
    rot = np.linalg.qr(rng.standard_normal((d, d)))[0]
    centers = 2.0 * rng.standard_normal((clusters, d)) * spec
    latent = centers[rng.integers(clusters, size=n)] + rng.standard_normal((n, d)) * spec
    xi = (latent + 0.3 * rng.standard_normal((n, d)) * spec) @ rot.T + 8.0 * rng.standard_normal(d)
    xt = (0.8 * latent + 0.4 * rng.standard_normal((n, d)) * spec) @ rot.T + 8.0 * rng.standard_normal(d)
    return xi.astype(np.float32), xt.astype(np.float32)


def moments(f):
    x = np.asarray(f, dtype=np.float64)
    return x.sum(0), x.T @ x


def moments_bound(f):
    """The summation-order bound 8 N eps sum|terms| of every entry of (sum, sq)."""
    x = np.abs(np.asarray(f, dtype=np.float64))
    n = x.shape[0]
    return 8 * n * EPS * x.sum(0), 8 * n * EPS * (x.T @ x)


def covariance(sums_i, sums_t, n):
    out = []
    cov = 0.0
    for s, q in (sums_i, sums_t):
        mu = s / n
        c = q / n - np.outer(mu, mu)
        tr = np.trace(c)
        alpha = 1.0 / np.sqrt(tr) if tr > 0 else 0.0
        out.append((mu, alpha))
        cov = cov + 0.5 * alpha * alpha * c
    return out[0][0], out[1][0], np.array([out[0][1], out[1][1]]), cov


def order_and_sign(evals, evecs):
    """Eigenvalues descending (ties by index), each vector's entry of largest magnitude (lowest row on a tie) positive."""
    order = np.argsort(-evals, kind="stable")
    evals, evecs = evals[order], evecs[:, order].copy()
    for j in range(evecs.shape[1]):
        i = int(np.argmax(np.abs(evecs[:, j])))
        if evecs[i, j] < 0:
            evecs[:, j] = -evecs[:, j]
    return evals, evecs


def eigh(cov):
    w, v = np.linalg.eigh((cov + cov.T) / 2)
    return order_and_sign(w[::-1].copy(), v[:, ::-1].copy())


def random_projection(d, k, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(d, k, generator=g, dtype=torch.float64).numpy()


def project(f, mu, alpha, p):
    return alpha * ((np.asarray(f, dtype=np.float64) - mu) @ p)


def polar_t(m):
    """(orthogonal polar factor of m)^T = UA UB^T for m = UB S UA^T."""
    u, _, vt = np.linalg.svd(m)
    return (u @ vt).T


def step(v, r):
    z = v @ r
    b = np.where(z >= 0, 1.0, -1.0)
    return z, b, b.T @ v, float(((b - z) ** 2).sum())


def rotate(v, r0, iters):
    r, obj = r0.copy(), []
    for _ in range(iters):
        _, _, m, o = step(v, r)
        obj.append(o)
        r = polar_t(m)
    z, b, _, o = step(v, r)
    obj.append(o)
    return r, np.array(obj), z, b


def fit(fi, ft, bits, projection="pca", rotation="itq", iters=50, seed=0, perturb=None):
    """Steps 1-5.  perturb = (relative size, seed): symmetric noise of that size times max|C| on C before the eigen-solver."""
    n, d = fi.shape
    mu_i, mu_t, alpha, cov = covariance(moments(fi), moments(ft), n)
    if perturb is not None:
        e = np.random.default_rng(perturb[1]).standard_normal((d, d))
        cov = cov + perturb[0] * np.abs(cov).max() * (e + e.T) / 2
    out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "C": cov}
    if projection == "pca":
        out["evals"], evecs = eigh(cov)
        p = evecs[:, :bits].copy()
    else:
        p = random_projection(d, bits, seed)
    v = np.concatenate([project(fi, mu_i, alpha[0], p), project(ft, mu_t, alpha[1], p)])
    r, obj, z, b = rotate(v, np.eye(bits), iters if rotation == "itq" else 0)
    s = 0.5 / np.sqrt((z ** 2).mean())
    heads = {}
    for side, a, mu in (("i", alpha[0], mu_i), ("t", alpha[1], mu_t)):
        w = s * a * (p @ r).T
        heads[f"W_{side}"], heads[f"b_{side}"] = w, -w @ mu
    out.update(P=p, V=v, R=r, objective=obj, Z=z, codes=b, scale=s, **heads)
    return out


# ---- the eigen-solver's and the polar factor's test matrices ----------------------------------------------------------------
def spd_matrix(d, seed, decay=0.9):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    a = (q * decay ** np.arange(d)) @ q.T
    return (a + a.T) / 2


def low_rank_covariance(n, d, seed):
    """Covariance of n < d + 1 points: rank n - 1."""
    x = np.random.default_rng(seed).standard_normal((n, d))
    x = x - x.mean(0)
    return x.T @ x / n


def repeated_eigenvalue_matrix(d, seed):
    """Eigenvalues 3 (three times), 1 (twice) and distinct ones below."""
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    lam = np.concatenate([[3.0, 3.0, 3.0, 1.0, 1.0], 0.5 * 0.8 ** np.arange(d - 5)])
    a = (q * lam) @ q.T
    return (a + a.T) / 2


def eigh_checks(c, evals, evecs):
    """-> (orthogonality defect, residual / |C|_F, eigenvalue error / |C|_F against LAPACK, the bound 64 D eps)."""
    d = c.shape[0]
    nf = np.linalg.norm(c)
    orth = np.abs(evecs.T @ evecs - np.eye(d)).max()
    resid = np.abs(c @ evecs - evecs * evals).max() / nf
    lam = np.abs(np.sort(evals)[::-1] - np.linalg.eigvalsh(c)[::-1]).max() / nf
    return orth, resid, lam, 64 * d * EPS


def conventions_hold(evals, evecs):
    if np.any(np.diff(evals) > 0):
        return False
    for j in range(evecs.shape[1]):
        a = np.abs(evecs[:, j])
        if evecs[int(np.argmax(a)), j] <= 0:
            return False
    return True
