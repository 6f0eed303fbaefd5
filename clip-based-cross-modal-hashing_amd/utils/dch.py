"""Supervised training-free hash heads (no upstream counterpart): discrete cross-modal hashing on frozen features (DCH, Xu et al.,
TIP 2017; the cross-modal form of SDH, Shen et al., CVPR 2015), fitted on the GPU by csrc/dch.hip with the pieces of csrc/itq.hip.

    fit = fit_supervised_heads(Fi, Ft, Y, bits=64)              # raw encode_image / encode_text outputs f32 [N, D], labels [N, C]
    utils.itq.load_heads(model, fit)                            # image_hash.fc / text_hash.fc <- W_m, b_m

The fit looks for B in {+-1}^{N x K} that predicts the labels linearly and is predicted linearly from each modality's features:

    objective = |Y - B W|^2 + lam |W|^2 + mu (|B - Z_i|^2 + |B - Z_t|^2),    Z_m = X_m P_m,   X_m = alpha_m (F_m - mu_m)

and ends, like ITQ, in one affine map per modality, code = sign(W_m f + b_m).  Steps (DESIGN.md §7.11 states them in full):

  1. moments   mu_m, alpha_m, the pooled C and S_mm = alpha_m^2 cov(f_m) (trace 1) from the running f64 sums; no cross moment
  2. once      A_m = (S_mm + (reg / D) I)^-1 = H_m H_m^T with the whitener H_m = E_m diag((lambda + reg / D)^-1/2) E_m^T
  3. start     P0 = the K leading eigenvectors of C, B = +1 where X_i P0 + X_t P0 >= 0 else -1
  4. `iters` times: T_m = F_m^T B and 1^T B; P_m = A_m alpha_m (T_m - mu_m bsum^T) / N; Z_m = X_m P_m; W = (B^T B + lam I)^-1 B^T Y;
     G = W W^T; the objective; Q = Y W^T + mu Z_i + mu Z_t; `rounds` Gauss-Seidel rounds of b_l <- sign(q_l - sum_{k != l} b_k G[k][l])
     over the bits of every item, a zero keeping the bit
  5. P_m, Z_m and W once more for the final B, the objective, and the heads W_m = s alpha_m P_m^T, b_m = -W_m mu_m, s = 0.5 / rms(Z)

Everything but casts, slicing and one transposed copy runs in libcmh, and nothing is read back inside the loop: the only host reads
are the eigen-solver's word per sweep."""
import torch

import cmh_native as N
from .itq import MomentStream, check_dims, whitener

# Choices made on the synthetic fixture of tests/dchutil.py, not optima measured on a real dataset.
DCH_ITERS = 10            # outer iterations: on the fixtures the flips per iteration fall by 10x to 100x within five
DCH_ROUNDS = 3            # Gauss-Seidel rounds over the bits per iteration
DCH_LAMBDA = 1.0          # ridge of the label regression W
DCH_MU = 0.01             # weight of the two feature terms: larger values pull B back to what the features alone predict
DCH_REG = 0.1             # ridge of the feature regressions, relative to the mean eigenvalue of a trace-1 covariance (as CCA_REG)


def supervised_moments(stream):
    """A MomentStream's sums -> mu_i, mu_t, alpha [2], C, S_ii, S_tt: what finish() returns, and each modality's own normalised
    covariance S_mm = alpha_m^2 cov(f_m).  No cross sum is needed."""
    mu_i, mu_t, alpha, cov = stream.finish()
    S_ii = N.dch_covariance(stream.sums_i[1], mu_i, alpha[0:1], stream.n)
    S_tt = N.dch_covariance(stream.sums_t[1], mu_t, alpha[1:2], stream.n)
    return mu_i, mu_t, alpha, cov, S_ii, S_tt


def _check(Fi, Ft, Y, bits, iters, rounds, lam, mu, reg):
    if Fi.dim() != 2 or Fi.shape != Ft.shape:
        raise ValueError(f"fit_supervised_heads: paired features expected: image {tuple(Fi.shape)}, text {tuple(Ft.shape)}")
    n, dim = Fi.shape
    if Y.dim() != 2 or Y.shape[0] != n:
        raise ValueError(f"fit_supervised_heads: labels {tuple(Y.shape)} for {n} pairs, expected [{n}, C]")
    check_dims("fit_supervised_heads", dim, bits)
    if not 1 <= Y.shape[1] <= N.DCH_MAX_C:
        raise ValueError(f"fit_supervised_heads: C = {Y.shape[1]} classes: need 1 <= C <= {N.DCH_MAX_C}")
    if n < 1 or iters < 0 or not 1 <= rounds <= N.DCH_MAX_ROUNDS:
        raise ValueError(f"fit_supervised_heads: N = {n}, iters = {iters}, rounds = {rounds}: need N >= 1, iters >= 0 and 1 <= rounds <= {N.DCH_MAX_ROUNDS}")
    if not (lam > 0.0 and mu >= 0.0 and reg > 0.0):
        raise ValueError(f"fit_supervised_heads: lam = {lam!r}, mu = {mu!r}, reg = {reg!r}: need lam > 0, mu >= 0 and reg > 0")


def fit_from_moments(Fi, Ft, Y, moments, bits, iters=DCH_ITERS, rounds=DCH_ROUNDS, lam=DCH_LAMBDA, mu=DCH_MU, reg=DCH_REG):
    """The fit behind fit_supervised_heads, from features, labels and supervised_moments(stream) of the same rows."""
    bits, iters, rounds, lam, mu, reg = int(bits), int(iters), int(rounds), float(lam), float(mu), float(reg)
    _check(Fi, Ft, Y, bits, iters, rounds, lam, mu, reg)
    Fi, Ft, Y = N.f32c(Fi), N.f32c(Ft), N.f32c(Y)
    n, dim = Fi.shape
    dev = Fi.device
    mu_i, mu_t, alpha, cov, S_ii, S_tt = moments
    sides = ((Fi, mu_i, alpha[0:1]), (Ft, mu_t, alpha[1:2]))
    # 2. the feature regressions' inverse, once
    A, sweeps, converged = [], [], []
    for S in (S_ii, S_tt):
        H, sw, ok = whitener(S, reg / dim)
        A.append(N.itq_matmul(H, H, trans_b=True))
        sweeps.append(sw)
        converged.append(ok)
    # 3. the start
    evals, evecs, sw, ok = N.itq_eigh(cov)
    sweeps.append(sw)
    converged.append(ok)
    P0 = evecs[:, :bits].contiguous()
    B = N.dch_start(*(N.itq_project(F, m, a, P0) for F, m, a in sides))
    record = torch.empty(iters + 1, 2, dtype=torch.float64, device=dev)          # (objective, |Z|^2) per iteration and for the result
    flips = torch.empty(iters, rounds, dtype=torch.int64, device=dev)
    margins = torch.empty(iters, dtype=torch.float64, device=dev)
    info = torch.zeros(iters + 1, dtype=torch.int32, device=dev)

    def regress(it):
        """P_m, Z_m and W of the current B."""
        P, Z = [], []
        for m, (F, mean, a) in enumerate(sides):
            T, bsum = N.dch_xtb(F, B, want_bsum=True)
            P.append(N.itq_matmul(A[m], N.dch_center(T, bsum, mean, a, n)))
            Z.append(N.itq_project(F, mean, a, P[m]))
        W, _ = N.dch_solve(N.dch_btb(B), N.dch_xtb(Y, B).t().contiguous(), lam, info=info[it:it + 1])
        return P, Z, W

    for it in range(iters):
        P, Z, W = regress(it)
        Qt, _ = N.dch_targets(Y, B, W, Z[0], Z[1], mu, lam, obj2=record[it])
        N.dch_dcc(Qt, N.itq_matmul(W, W, trans_b=True), B, rounds, flips=flips[it], min_margin=margins[it:it + 1])
    P, Z, W = regress(iters)
    N.dch_targets(Y, B, W, Z[0], Z[1], mu, lam, want_q=False, obj2=record[iters])
    eye = torch.eye(bits, dtype=torch.float64, device=dev)
    W_i, b_i, W_t, b_t, s = N.itq_heads_pair(P[0], P[1], eye, mu_i, mu_t, alpha, record[iters, 1:2].contiguous(), 2 * n)
    return {"W_i": W_i, "b_i": b_i, "W_t": W_t, "b_t": b_t, "scale": s, "B": B, "P_i": P[0], "P_t": P[1], "W": W, "mu_i": mu_i, "mu_t": mu_t,
            "alpha": alpha, "n": n, "evals": evals, "objective": record[:, 0].contiguous(), "flips": flips, "min_margin": margins,
            "solve_info": info, "eigh_sweeps": tuple(sweeps), "eigh_converged": all(converged), "eigh_converged_each": tuple(converged),
            "params": {"iters": iters, "rounds": rounds, "lam": lam, "mu": mu, "reg": reg}}


def fit_supervised_heads(Fi, Ft, Y, bits, iters=DCH_ITERS, rounds=DCH_ROUNDS, lam=DCH_LAMBDA, mu=DCH_MU, reg=DCH_REG):
    """Image / text features f32 [N, D] on the GPU (the raw encode_image / encode_text outputs, not normalised) and multi-hot labels
    [N, C] -> dict of device tensors: the heads W_i, W_t f32 [bits, D], b_i, b_t f32 [bits] and scale [1]; the fit's state B int8
    [N, bits], P_i, P_t [D, bits], W [bits, C] (the label regression), mu_i, mu_t, alpha [2]; and its diagnostics: objective
    [iters + 1] (at the start of each iteration, then for the result), flips int64 [iters, rounds], min_margin [iters] (the smallest
    |t| of each iteration's decisions: one at rounding level says the codes are not reproducible to the last bit), solve_info int32
    [iters + 1] (non-zero: that label regression met a pivot that was not positive), and the three eigen-solves' eigh_sweeps /
    eigh_converged_each (S_ii, S_tt, C; eigh_converged: all three)."""
    _check(Fi, Ft, Y, int(bits), int(iters), int(rounds), float(lam), float(mu), float(reg))
    return fit_from_moments(Fi, Ft, Y, supervised_moments(MomentStream().add(Fi, Ft)), bits, iters, rounds, lam, mu, reg)
