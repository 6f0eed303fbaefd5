"""Training-free hash heads from paired features (no upstream counterpart): LSH, PCAH and ITQ fitted on the GPU by csrc/itq.hip.

    fit = fit_hash_heads(Fi, Ft, bits=64)                       # raw clip.encode_image / encode_text outputs, f32 [N, D]
    load_heads(model, fit)                                      # image_hash.fc / text_hash.fc <- W_m, b_m

The fit is code = sign(W_m f + b_m) per modality, which a LinearHash head computes (tanh keeps the sign).  Steps: the modalities'
means, scales alpha_m = 1 / sqrt(mean |f - mu_m|^2) and pooled covariance from running f64 sums; the projection P [D, K] (`pca`: the
K leading eigenvectors by cyclic Jacobi; `random`: Gaussian, drawn on the host from `seed`); V = [alpha_i (Fi - mu_i) P; alpha_t
(Ft - mu_t) P]; the rotation R (`none`: I; `itq`: `iters` iterations from R0); the heads W_m = s alpha_m (P R)^T, b_m = -W_m mu_m
with s = 0.5 / rms(V R).  pca + none is PCAH, random + none is LSH, pca + itq is ITQ.  Everything but casts, cat and slicing runs
in libcmh; nothing is read back before the fit is done.

`cca` (the cross-modal variant of the same paper) gives each modality its own projection: with S_mm = alpha_m^2 cov(f_m) (trace 1),
S_it = alpha_i alpha_t cov(f_i, f_t) and the ridge r = reg / D, the whiteners H_m = E_m diag((lambda + r)^-1/2) E_m^T, the whitened
cross-covariance T = H_i S_it H_t, its leading left vectors U_K from the eigenvectors of T T^T with sigma_j = sqrt(eigenvalue j)
(the canonical correlations), v_j = T^T u_j / sigma_j, and P_i = H_i U_K, P_t = H_t V_K.  Rows, rotation and heads follow as above
with P_m in the place of P.  One pair of correlations is read back (sigma_1, sigma_K) before any head is written: a fit that asks
for more bits than the pairing has correlated directions is refused."""
import torch

import cmh_native as N

PROJECTIONS, ROTATIONS = ("pca", "random", "cca"), ("itq", "none")
CCA_REG = 0.1             # the ridge, relative to the mean eigenvalue of a trace-1 covariance: a choice, not a measured optimum
CCA_FLOOR = 1e-6          # canonical directions at or below this share of sigma_1 are rounding, not correlation


class MomentStream:
    """Running f64 sums of both modalities, one batch per call (the trainer streams loader batches through it); with `cross` also
    the cross sum sum_n f_i f_t^T that the `cca` projection needs."""

    def __init__(self, cross=False):
        self.sums_i = self.sums_t = None
        self.cross = None
        self.want_cross = bool(cross)
        self.n = 0

    def add(self, Fi, Ft):
        if Fi.shape != Ft.shape:
            raise ValueError(f"paired features expected: image {tuple(Fi.shape)}, text {tuple(Ft.shape)}")
        self.sums_i = N.itq_moments(Fi, self.sums_i)
        self.sums_t = N.itq_moments(Ft, self.sums_t)
        if self.want_cross:
            self.cross = N.itq_cross_moments(Fi, Ft, self.cross)
        self.n += Fi.shape[0]
        return self

    def finish(self):
        """-> mu_i, mu_t, alpha [2], C"""
        return N.itq_covariance(self.sums_i, self.sums_t, self.n)

    def finish_cca(self):
        """-> mu_i, mu_t, alpha [2], S_ii, S_tt, S_it"""
        if self.cross is None:
            raise ValueError("MomentStream(cross=True) is needed for the cca projection: this stream kept no cross sum")
        return N.itq_cca_covariance(self.sums_i, self.sums_t, self.cross, self.n)


def random_projection(dim, bits, seed, device):
    """Gaussian [D, K] f64 from a CPU generator seeded with `seed`: the same on every machine."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(dim, bits, generator=g, dtype=torch.float64).to(device)


def whitener(S, ridge):
    """H = E diag((lambda + ridge)^-1/2) E^T of a symmetric S [D, D] f64 on the GPU (H H^T = (S + ridge I)^-1) -> H, the
    eigen-solve's sweeps, converged."""
    lam, E, sweeps, converged = N.itq_eigh(S)
    return N.itq_matmul(E, E, d=N.itq_inv_sqrt(lam, ridge), trans_b=True), sweeps, converged


def check_dims(what, dim, bits):
    """The D / bits bounds of every fit (the library's own, refused here before any launch)."""
    if not (1 <= dim <= N.ITQ_MAX_D and 1 <= bits <= min(dim, N.ITQ_MAX_K)):
        raise ValueError(f"{what}: D = {dim}, bits = {bits}: need 1 <= D <= {N.ITQ_MAX_D} and 1 <= bits <= min(D, {N.ITQ_MAX_K})")


def _check_names(projection, rotation, reg):
    if projection not in PROJECTIONS or rotation not in ROTATIONS:
        raise ValueError(f"projection {projection!r} / rotation {rotation!r}: one of {PROJECTIONS} and one of {ROTATIONS}")
    if projection == "cca" and not float(reg) > 0.0:
        raise ValueError(f"fit_hash_heads: reg = {reg!r}: the cca ridge must be positive")


def cca_directions(S_ii, S_tt, S_it, bits, reg=CCA_REG):
    """The CCA projections from the normalised covariances [D, D] f64 on the GPU -> dict with P_i, P_t [D, bits], correlations [D]
    (descending), the whiteners H_i, H_t, T = H_i S_it H_t, U (all D left vectors), and the sweeps / convergence of the three
    eigen-solves (S_ii, S_tt, T T^T).  ValueError where sigma_bits <= 1e-6 sigma_1."""
    dim = S_ii.shape[0]
    r = float(reg) / dim
    (H_i, sw_i, ok_i), (H_t, sw_t, ok_t) = whitener(S_ii, r), whitener(S_tt, r)
    T = N.itq_matmul(H_i, N.itq_matmul(S_it, H_t))
    g_evals, U, sw, ok = N.itq_eigh(N.itq_matmul(T, T, trans_b=True))
    sweeps, converged = (sw_i, sw_t, sw), (ok_i, ok_t, ok)
    inv_sigma, sigma = N.itq_inv_sqrt(g_evals, 0.0, want_root=True)
    first, last = (float(v) for v in sigma[[0, bits - 1]].cpu())             # the fit's one read before the heads
    if not last > CCA_FLOOR * first:
        above = int((sigma > CCA_FLOOR * first).sum()) if first > 0.0 else 0
        raise ValueError(f"cca: {above} canonical directions stand above {CCA_FLOOR:g} of the largest correlation, {bits} bits were asked")
    U_K = U[:, :bits].contiguous()
    V_K = N.itq_matmul(T, U_K, col_scale=inv_sigma[:bits].contiguous(), trans_a=True)
    return {"P_i": N.itq_matmul(H_i, U_K), "P_t": N.itq_matmul(H_t, V_K), "correlations": sigma, "H_i": H_i, "H_t": H_t, "T": T,
            "U": U, "eigh_sweeps": sweeps, "eigh_converged": all(converged), "eigh_converged_each": converged}


def fit_from_moments(Fi, Ft, moments, bits, projection="pca", rotation="itq", iters=50, R0=None, seed=0, reg=CCA_REG):
    """The fit behind fit_hash_heads, from features and their finished moments: (mu_i, mu_t, alpha, C), or for `cca`
    (mu_i, mu_t, alpha, S_ii, S_tt, S_it) from MomentStream(cross=True).finish_cca()."""
    _check_names(projection, rotation, reg)
    n, dim = Fi.shape
    bits = int(bits)
    check_dims("fit_hash_heads", dim, bits)
    dev = Fi.device
    if projection == "cca":
        if len(moments) != 6:
            raise ValueError("projection 'cca' needs the moments of MomentStream(cross=True).finish_cca()")
        mu_i, mu_t, alpha, S_ii, S_tt, S_it = moments
        out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "n": n, "reg": float(reg)}
        cca = cca_directions(S_ii, S_tt, S_it, bits, reg)
        P_i, P_t = cca["P_i"], cca["P_t"]
        out.update({key: cca[key] for key in ("P_i", "P_t", "correlations", "eigh_sweeps", "eigh_converged", "eigh_converged_each")})
    else:
        mu_i, mu_t, alpha, cov = moments
        out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "n": n}
        if projection == "pca":
            evals, evecs, sweeps, converged = N.itq_eigh(cov)
            P = evecs[:, :bits].contiguous()
            out.update(evals=evals, eigh_sweeps=sweeps, eigh_converged=converged)
        else:
            P = random_projection(dim, bits, seed, dev)
        P_i = P_t = P
        out.update(P=P)
    V = torch.empty(2 * n, bits, dtype=torch.float64, device=dev)
    N.itq_project(Fi, mu_i, alpha[0:1], P_i, out=V[:n])
    N.itq_project(Ft, mu_t, alpha[1:2], P_t, out=V[n:])
    if R0 is None:
        R0 = torch.eye(bits, dtype=torch.float64, device=dev)
    R, obj, zz = N.itq_rotate(V, R0, iters if rotation == "itq" else 0)
    W_i, b_i, W_t, b_t, s = N.itq_heads_pair(P_i, P_t, R, mu_i, mu_t, alpha, zz, 2 * n)      # P_i = P_t: cmh_itq_heads, bit for bit
    out.update(R=R, V=V, objective=obj, scale=s, W_i=W_i, b_i=b_i, W_t=W_t, b_t=b_t)
    return out


def fit_hash_heads(Fi, Ft, bits, projection="pca", rotation="itq", iters=50, R0=None, seed=0, reg=CCA_REG):
    """Image / text features f32 [N, D] on the GPU (the raw encode_image / encode_text outputs, not normalised) -> dict with the
    heads W_i, W_t f32 [bits, D] and b_i, b_t f32 [bits], and the fit's own record: P [D, bits], R [bits, bits], V [2N, bits],
    mu_i, mu_t, alpha [2], scale [1], objective [iters + 1] (|B - V R|^2 at the start of each iteration and for the R returned;
    one entry without ITQ), and with `pca` evals [D], eigh_sweeps, eigh_converged.  With `cca` the record has P_i, P_t in the place
    of P, correlations [D], reg, and eigh_sweeps / eigh_converged_each as triples (S_ii, S_tt, T T^T; eigh_converged: all three).
    All tensors stay on the device."""
    _check_names(projection, rotation, reg)         # before the moments are taken
    stream = MomentStream(cross=projection == "cca").add(Fi, Ft)
    moments = stream.finish_cca() if projection == "cca" else stream.finish()
    return fit_from_moments(Fi, Ft, moments, bits, projection, rotation, iters, R0, seed, reg)


def load_heads(model, fit):
    """Write a fit's heads into a Baseclip model's LinearHash heads."""
    with torch.no_grad():
        for side, head in (("i", model.image_hash), ("t", model.text_hash)):
            head.fc.weight.copy_(fit[f"W_{side}"])
            head.fc.bias.copy_(fit[f"b_{side}"])
