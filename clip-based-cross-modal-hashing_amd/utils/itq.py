"""Training-free hash heads from paired features (no upstream counterpart): LSH, PCAH and ITQ fitted on the GPU by csrc/itq.hip.

    fit = fit_hash_heads(Fi, Ft, bits=64)                       # raw clip.encode_image / encode_text outputs, f32 [N, D]
    load_heads(model, fit)                                      # image_hash.fc / text_hash.fc <- W_m, b_m

The fit is code = sign(W_m f + b_m) per modality, which a LinearHash head computes (tanh keeps the sign).  Steps: the modalities'
means, scales alpha_m = 1 / sqrt(mean |f - mu_m|^2) and pooled covariance from running f64 sums; the projection P [D, K] (`pca`: the
K leading eigenvectors by cyclic Jacobi; `random`: Gaussian, drawn on the host from `seed`); V = [alpha_i (Fi - mu_i) P; alpha_t
(Ft - mu_t) P]; the rotation R (`none`: I; `itq`: `iters` iterations from R0); the heads W_m = s alpha_m (P R)^T, b_m = -W_m mu_m
with s = 0.5 / rms(V R).  pca + none is PCAH, random + none is LSH, pca + itq is ITQ.  Everything but casts, cat and slicing runs
in libcmh; nothing is read back before the fit is done."""
import torch

import cmh_native as N

PROJECTIONS, ROTATIONS = ("pca", "random"), ("itq", "none")


class MomentStream:
    """Running f64 sums of both modalities, one batch per call (the trainer streams loader batches through it)."""

    def __init__(self):
        self.sums_i = self.sums_t = None
        self.n = 0

    def add(self, Fi, Ft):
        if Fi.shape != Ft.shape:
            raise ValueError(f"paired features expected: image {tuple(Fi.shape)}, text {tuple(Ft.shape)}")
        self.sums_i = N.itq_moments(Fi, self.sums_i)
        self.sums_t = N.itq_moments(Ft, self.sums_t)
        self.n += Fi.shape[0]
        return self

    def finish(self):
        """-> mu_i, mu_t, alpha [2], C"""
        return N.itq_covariance(self.sums_i, self.sums_t, self.n)


def random_projection(dim, bits, seed, device):
    """Gaussian [D, K] f64 from a CPU generator seeded with `seed`: the same on every machine."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(dim, bits, generator=g, dtype=torch.float64).to(device)


def fit_from_moments(Fi, Ft, moments, bits, projection="pca", rotation="itq", iters=50, R0=None, seed=0):
    """The fit behind fit_hash_heads, from features and their finished moments (mu_i, mu_t, alpha, C)."""
    if projection not in PROJECTIONS or rotation not in ROTATIONS:
        raise ValueError(f"projection {projection!r} / rotation {rotation!r}: one of {PROJECTIONS} and one of {ROTATIONS}")
    n, dim = Fi.shape
    bits = int(bits)
    if not (1 <= dim <= N.ITQ_MAX_D and 1 <= bits <= min(dim, N.ITQ_MAX_K)):
        raise ValueError(f"fit_hash_heads: D = {dim}, bits = {bits}: need 1 <= D <= {N.ITQ_MAX_D} and 1 <= bits <= min(D, {N.ITQ_MAX_K})")
    mu_i, mu_t, alpha, cov = moments
    dev = Fi.device
    out = {"mu_i": mu_i, "mu_t": mu_t, "alpha": alpha, "n": n}
    if projection == "pca":
        evals, evecs, sweeps, converged = N.itq_eigh(cov)
        P = evecs[:, :bits].contiguous()
        out.update(evals=evals, eigh_sweeps=sweeps, eigh_converged=converged)
    else:
        P = random_projection(dim, bits, seed, dev)
    V = torch.empty(2 * n, bits, dtype=torch.float64, device=dev)
    N.itq_project(Fi, mu_i, alpha[0:1], P, out=V[:n])
    N.itq_project(Ft, mu_t, alpha[1:2], P, out=V[n:])
    if R0 is None:
        R0 = torch.eye(bits, dtype=torch.float64, device=dev)
    R, obj, zz = N.itq_rotate(V, R0, iters if rotation == "itq" else 0)
    W_i, b_i, W_t, b_t, s = N.itq_heads(P, R, mu_i, mu_t, alpha, zz, 2 * n)
    out.update(P=P, R=R, V=V, objective=obj, scale=s, W_i=W_i, b_i=b_i, W_t=W_t, b_t=b_t)
    return out


def fit_hash_heads(Fi, Ft, bits, projection="pca", rotation="itq", iters=50, R0=None, seed=0):
    """Image / text features f32 [N, D] on the GPU (the raw encode_image / encode_text outputs, not normalised) -> dict with the
    heads W_i, W_t f32 [bits, D] and b_i, b_t f32 [bits], and the fit's own record: P [D, bits], R [bits, bits], V [2N, bits],
    mu_i, mu_t, alpha [2], scale [1], objective [iters + 1] (|B - V R|^2 at the start of each iteration and for the R returned;
    one entry without ITQ), and with `pca` evals [D], eigh_sweeps, eigh_converged.  All tensors stay on the device."""
    moments = MomentStream().add(Fi, Ft).finish()
    return fit_from_moments(Fi, Ft, moments, bits, projection, rotation, iters, R0, seed)


def load_heads(model, fit):
    """Write a fit's heads into a Baseclip model's LinearHash heads."""
    with torch.no_grad():
        for side, head in (("i", model.image_hash), ("t", model.text_hash)):
            head.fc.weight.copy_(fit[f"W_{side}"])
            head.fc.bias.copy_(fit[f"b_{side}"])
