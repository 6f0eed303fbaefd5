"""NumPy fp64 restatement of the CCA fit (csrc/itq.hip, utils/itq.py, projection="cca"): cross moments, normalised covariances,
whitening, the canonical directions, the rows, the rotation and the heads.  It follows the product's conventions (correlations
descending, each u_j's entry of largest magnitude positive, v_j following u_j) but uses LAPACK's eigh where the product runs Jacobi
and LAPACK's SVD of T where the product goes through the eigenvectors of T T^T, so the two share no arithmetic.  Also the gap
fixture, a fixture whose cross-covariance has rank 5 exactly, and the error bounds that tests/test_gpu_cca.py asserts.

Bounds (all from the restatement's own conditioning, none from the GPU's output).  Jacobi's backward error is 64 D eps |S|_F
(tests/test_gpu_itq.py), and its vectors are orthogonal within 64 D eps.
  whitening   H (S + r I) H - I with H = E diag((lambda + r)^-1/2) E^T.  A backward error dS gives H dS H, at most |dS| / r
              = 64 D eps (|S|_F / lambda_max) (lambda_max / r); the orthogonality defect enters once on each side of
              W (Lambda + r) W = I; the three chained products round at 8 D eps of terms that are at most sqrt(kappa) in size.  With
              kappa = (lambda_max + r) / r every part is below 64 D eps kappa times (|S|_F / lambda_max, 2, 1):
              whiten_bound = 64 D eps kappa (|S|_F / lambda_max + 3).
  directions  P_i^T (S_ii + r I) P_i - I = U_K^T (whitening residual) U_K + (U_K^T U_K - I): whiten_bound + 64 D eps.  On the text
              side V_K^T V_K - I = S^-1 U_K^T (T T^T) U_K S^-1 - I carries the third solve's backward error 64 D eps |G|_F over
              sigma_K^2: whiten_bound + 2 * 64 D eps |G|_F / sigma_K^2 (the residual and the product T T^T itself).
  correlation P_i^T S_it P_t - diag(sigma) = U_K^T T V_K - S: the same backward error over sigma_K, and the rounding of
              T = H_i S_it H_t, whose terms are at most sqrt(kappa_i kappa_t) in size:
              64 D eps (2 |G|_F / sigma_K + sqrt(kappa_i kappa_t)) + both whitening bounds.
  sigma       against the restatement from the same covariances: the whiteners differ by their bounds (relative, on a T of norm
              sigma_1 <= 1) and an eigenvalue of G moves by 64 D eps |G|_F, sigma_j by that over 2 sigma_j."""
import numpy as np

import itqutil as U

EPS = U.EPS
FLOOR = 1e-6                                  # utils.itq.CCA_FLOOR
GAP_SEEDS, GAP_BITS = (7, 8, 9, 10), (8, 12)


def gap_pair(n, d, seed, shared=12, private=10, pscale=4.0):
    """Paired features f32 [n, d] with `shared` latent directions that both modalities see and `private` directions of larger
    variance per modality that the other does not: pooled PCA spends its bits on the private ones."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, shared))
    rot = np.linalg.qr(rng.standard_normal((d, d)))[0]

    def side(k0):
        x = 0.05 * rng.standard_normal((n, d))
        x[:, :shared] += z / (1 + 0.1 * np.arange(shared))
        x[:, k0:k0 + private] += pscale * rng.standard_normal((n, private)) / (1 + 0.1 * np.arange(private))
        return (x @ rot.T + 8.0 * rng.standard_normal(d)).astype(np.float32)
    xi = side(shared)
    return xi, side(shared + private)


def rank5_pair():
    """f32 [64, 24] pairs whose cross-covariance has rank 5 exactly: integer features built on columns of a 64 x 64 Hadamard
    matrix (mutually orthogonal, mean zero), five of them shared and ten private to each side, so that every moment is an
    integer that f32 and f64 hold exactly and the private columns contribute exactly nothing to sum f_i f_t^T."""
    h = np.array([[1.0]])
    for _ in range(6):
        h = np.block([[h, h], [h, -h]])
    rng = np.random.default_rng(5)
    d = 24
    mix = [rng.integers(-3, 4, size=(5, d)).astype(np.float64) for _ in range(2)]
    own = [rng.integers(-2, 3, size=(10, d)).astype(np.float64) for _ in range(2)]
    xi = h[:, 1:6] @ mix[0] + h[:, 6:16] @ own[0]
    xt = h[:, 1:6] @ mix[1] + h[:, 16:26] @ own[1]
    return xi.astype(np.float32), xt.astype(np.float32)


def cross_moment(fi, ft):
    return np.asarray(fi, dtype=np.float64).T @ np.asarray(ft, dtype=np.float64)


def cross_bound(fi, ft):
    """The summation-order bound 8 N eps sum|terms| of every entry of the cross sum (itqutil.moments_bound's form)."""
    xi, xt = np.abs(np.asarray(fi, dtype=np.float64)), np.abs(np.asarray(ft, dtype=np.float64))
    return 8 * xi.shape[0] * EPS * (xi.T @ xt)


def covariances(fi, ft, perturb=None):
    """-> mu_i, mu_t, alpha [2], S_ii, S_tt, S_it.  perturb = (relative size, seed): symmetric noise of that size times max|S| on
    S_ii and S_tt, general noise of that relative size on S_it."""
    n, d = fi.shape
    (si, qi), (st, qt) = U.moments(fi), U.moments(ft)
    mu_i, mu_t = si / n, st / n
    ci, ct = qi / n - np.outer(mu_i, mu_i), qt / n - np.outer(mu_t, mu_t)
    alpha = np.array([1.0 / np.sqrt(np.trace(c)) if np.trace(c) > 0 else 0.0 for c in (ci, ct)])
    s_ii, s_tt = alpha[0] ** 2 * ci, alpha[1] ** 2 * ct
    s_it = alpha[0] * alpha[1] * (cross_moment(fi, ft) / n - np.outer(mu_i, mu_t))
    if perturb is not None:
        rng = np.random.default_rng(perturb[1])
        e1, e2, e3 = (rng.standard_normal((d, d)) for _ in range(3))
        s_ii = s_ii + perturb[0] * np.abs(s_ii).max() * (e1 + e1.T) / 2
        s_tt = s_tt + perturb[0] * np.abs(s_tt).max() * (e2 + e2.T) / 2
        s_it = s_it + perturb[0] * np.abs(s_it).max() * e3
    return mu_i, mu_t, alpha, s_ii, s_tt, s_it


def whitener(s, r):
    lam, e = U.eigh(s)
    return (e / np.sqrt(lam + r)) @ e.T, lam


def directions(s_ii, s_tt, s_it, bits, reg=0.1):
    """Steps 3-5 -> dict with H_i, H_t, T, sigma [D], U [D, D], Vfull [D, D], P_i, P_t [D, bits], lam_i, lam_t.  ValueError where
    sigma_bits <= 1e-6 sigma_1, with the number of directions above that level."""
    if not reg > 0:
        raise ValueError(f"reg = {reg!r}: the cca ridge must be positive")
    d = s_ii.shape[0]
    r = reg / d
    h_i, lam_i = whitener(s_ii, r)
    h_t, lam_t = whitener(s_tt, r)
    t = h_i @ s_it @ h_t
    u, sigma, vt = np.linalg.svd(t)
    v = vt.T.copy()
    for j in range(d):                          # each pair flipped together: u_j's largest entry positive
        if u[int(np.argmax(np.abs(u[:, j]))), j] < 0:
            u[:, j], v[:, j] = -u[:, j], -v[:, j]
    if not sigma[bits - 1] > FLOOR * sigma[0]:
        above = int((sigma > FLOOR * sigma[0]).sum()) if sigma[0] > 0 else 0
        raise ValueError(f"cca: {above} canonical directions stand above {FLOOR:g} of the largest correlation, {bits} bits were asked")
    return {"H_i": h_i, "H_t": h_t, "T": t, "sigma": sigma, "U": u, "Vfull": v, "P_i": h_i @ u[:, :bits], "P_t": h_t @ v[:, :bits],
            "lam_i": lam_i, "lam_t": lam_t, "r": r}


def fit(fi, ft, bits, rotation="itq", iters=50, reg=0.1, perturb=None):
    """Steps 1-8 with the cca projection; the keys of itqutil.fit with P_i, P_t in the place of P, and sigma."""
    mu_i, mu_t, alpha, s_ii, s_tt, s_it = covariances(fi, ft, perturb)
    dirs = directions(s_ii, s_tt, s_it, bits, reg)
    v = np.concatenate([U.project(fi, mu_i, alpha[0], dirs["P_i"]), U.project(ft, mu_t, alpha[1], dirs["P_t"])])
    r, obj, z, b = U.rotate(v, np.eye(bits), iters if rotation == "itq" else 0)
    s = 0.5 / np.sqrt((z ** 2).mean())
    out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "S_ii": s_ii, "S_tt": s_tt, "S_it": s_it, "reg": reg}
    for side, a, mu in (("i", alpha[0], mu_i), ("t", alpha[1], mu_t)):
        w = s * a * (dirs[f"P_{side}"] @ r).T
        out[f"W_{side}"], out[f"b_{side}"] = w, -w @ mu
    out.update(dirs)
    out.update(V=v, R=r, objective=obj, Z=z, codes=b, scale=s)
    return out


def pair_agreement(codes):
    """Mean share of equal bits between row n (image) and row N + n (text)."""
    n = codes.shape[0] // 2
    return float((codes[:n] == codes[n:]).mean())


# ---- the bounds of the module docstring -------------------------------------------------------------------------------------
def kappa(lam, r):
    return (lam.max() + r) / r


def whiten_bound(s, lam, r):
    return 64 * s.shape[0] * EPS * kappa(lam, r) * (np.linalg.norm(s) / lam.max() + 3)


def direction_bounds(ref, bits):
    """-> bounds on max|P_i^T (S_ii + r I) P_i - I|, the same for the text side, max|P_i^T S_it P_t - diag sigma| and
    max|sigma_gpu - sigma| over the kept directions, from a restatement fit or directions() dict (with S_ii, S_tt added)."""
    d, r = ref["T"].shape[0], ref["r"]
    wb_i, wb_t = whiten_bound(ref["S_ii"], ref["lam_i"], r), whiten_bound(ref["S_tt"], ref["lam_t"], r)
    g_fro = np.linalg.norm(ref["T"] @ ref["T"].T)
    sig_k = ref["sigma"][bits - 1]
    jac = 64 * d * EPS
    b_i = wb_i + jac
    b_t = wb_t + 2 * jac * g_fro / sig_k ** 2
    b_corr = jac * (2 * g_fro / sig_k + np.sqrt(kappa(ref["lam_i"], r) * kappa(ref["lam_t"], r))) + wb_i + wb_t
    b_sigma = wb_i + wb_t + jac * g_fro / (2 * sig_k)
    return b_i, b_t, b_corr, b_sigma
