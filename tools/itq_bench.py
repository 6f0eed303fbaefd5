"""Times of the training-free fit (csrc/itq.hip, utils/itq.py) on the GPU against its NumPy fp64 restatement on the host
(tests/itqutil.py: BLAS and LAPACK on the CPU) in the same process, one JSON line per shape; medians of 5 timed regions after a
warm-up.  GPU regions are timed with device events (the eigen-solver's per-sweep host reads fall inside its region), host regions
with perf_counter.

    python tools/itq_bench.py [--shapes 10000x512x64,100000x512x64] [--iters 50]

Phases: moments (both modalities' running sums), covariance (means, scales, pooled C), eigh (all D eigenpairs), project (both
modalities), rotate (`iters` ITQ iterations and the final pass), heads.  The `cca` block of each line times the CCA projections the
same way (tests/ccautil.py is the host side): cross_moments, covariance (S_ii, S_tt, S_it), eigh_ii / eigh_tt / eigh_g (the three
eigen-solves; the host runs LAPACK's eigh twice and its SVD of T), products (the whiteners' spectra, H_i, H_t, T, T T^T, V_K, P_i,
P_t: eight dense products), project, rotate, heads, and `fit`: the whole cca + itq fit next to the whole pca + itq fit, each
timed as one region from the features to the heads.  The features are already on the device / in host memory; the upload is not
part of either side.  Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REGIONS = 5
SHAPES = "10000x512x64,100000x512x64"


def _gpu_ms(fn, regions=REGIONS):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        del out
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 3)


def _host_ms(fn, regions=REGIONS):
    fn()
    ts = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def shape_line(n, d, k, iters, dev):
    import numpy as np
    import torch
    import cmh_native as N
    import itqutil as U
    fi, ft = U.make_pair(n, d, 1)
    gi, gt = torch.from_numpy(fi).to(dev), torch.from_numpy(ft).to(dev)
    eye = torch.eye(k, dtype=torch.float64, device=dev)
    # the GPU's chain, each phase on the previous one's outputs
    si, st = N.itq_moments(gi), N.itq_moments(gt)
    mu_i, mu_t, alpha, cov = N.itq_covariance(si, st, n)
    evals, evecs, sweeps, converged = N.itq_eigh(cov)
    P = evecs[:, :k].contiguous()
    V = torch.empty(2 * n, k, dtype=torch.float64, device=dev)

    def project():
        N.itq_project(gi, mu_i, alpha[0:1], P, out=V[:n])
        return N.itq_project(gt, mu_t, alpha[1:2], P, out=V[n:])
    project()
    R, obj, zz = N.itq_rotate(V, eye, iters)
    gpu = {"moments": _gpu_ms(lambda: (N.itq_moments(gi), N.itq_moments(gt))),
           "covariance": _gpu_ms(lambda: N.itq_covariance(si, st, n)),
           "eigh": _gpu_ms(lambda: N.itq_eigh(cov)),
           "project": _gpu_ms(project),
           "rotate": _gpu_ms(lambda: N.itq_rotate(V, eye, iters)),
           "heads": _gpu_ms(lambda: N.itq_heads(P, R, mu_i, mu_t, alpha, zz, 2 * n))}
    # the host's chain
    hs_i, hs_t = U.moments(fi), U.moments(ft)
    h_mu_i, h_mu_t, h_alpha, h_cov = U.covariance(hs_i, hs_t, n)
    h_p = U.eigh(h_cov)[1][:, :k].copy()
    h_v = np.concatenate([U.project(fi, h_mu_i, h_alpha[0], h_p), U.project(ft, h_mu_t, h_alpha[1], h_p)])
    h_r, h_obj, h_z, _ = U.rotate(h_v, np.eye(k), iters)

    def host_heads():
        s = 0.5 / np.sqrt((h_z ** 2).mean())
        return [(s * a * (h_p @ h_r).T, -(s * a * (h_p @ h_r).T) @ mu) for a, mu in ((h_alpha[0], h_mu_i), (h_alpha[1], h_mu_t))]
    host = {"moments": _host_ms(lambda: (U.moments(fi), U.moments(ft))),
            "covariance": _host_ms(lambda: U.covariance(hs_i, hs_t, n)),
            "eigh": _host_ms(lambda: U.eigh(h_cov)),
            "project": _host_ms(lambda: (U.project(fi, h_mu_i, h_alpha[0], h_p), U.project(ft, h_mu_t, h_alpha[1], h_p))),
            "rotate": _host_ms(lambda: U.rotate(h_v, np.eye(k), iters)),
            "heads": _host_ms(host_heads)}
    gpu["total"], host["total"] = round(sum(gpu.values()), 3), round(sum(host.values()), 3)
    codes = np.where(N.itq_step(V, R)[0].cpu().numpy() >= 0, 1.0, -1.0)
    return {"tool": "itq_bench", "N": n, "D": d, "K": k, "iters": iters, "regions": REGIONS, "eigh_sweeps": sweeps,
            "eigh_converged": converged, "objective_first_last": [float(obj[0]), float(obj[-1])],
            "host_objective_first_last": [float(h_obj[0]), float(h_obj[-1])],
            "code_agreement_with_host": round(float((codes == np.where(h_z >= 0, 1.0, -1.0)).mean()), 6),
            "host_threads": os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"]),
            "gpu_ms": gpu, "host_ms": host, "cca": cca_block(n, d, k, iters, dev, fi, ft, gi, gt)}


def cca_block(n, d, k, iters, dev, fi, ft, gi, gt):
    """The CCA phases on the GPU and on the host, and both whole fits."""
    import numpy as np
    import torch
    import cmh_native as N
    import ccautil as CU
    import itqutil as U
    from utils.itq import fit_hash_heads
    eye = torch.eye(k, dtype=torch.float64, device=dev)
    r = 0.1 / d
    si, st, cross = N.itq_moments(gi), N.itq_moments(gt), N.itq_cross_moments(gi, gt)
    mu_i, mu_t, alpha, S_ii, S_tt, S_it = N.itq_cca_covariance(si, st, cross, n)
    (lam_i, E_i, sw_i, ok_i), (lam_t, E_t, sw_t, ok_t) = N.itq_eigh(S_ii), N.itq_eigh(S_tt)

    def whiteners():
        return (N.itq_matmul(E_i, E_i, d=N.itq_inv_sqrt(lam_i, r), trans_b=True), N.itq_matmul(E_t, E_t, d=N.itq_inv_sqrt(lam_t, r), trans_b=True))
    H_i, H_t = whiteners()

    def cross_products():
        T = N.itq_matmul(H_i, N.itq_matmul(S_it, H_t))
        return T, N.itq_matmul(T, T, trans_b=True)
    T, G = cross_products()
    g_evals, Uv, sw_g, ok_g = N.itq_eigh(G)
    U_K = Uv[:, :k].contiguous()

    def directions():
        inv_sigma = N.itq_inv_sqrt(g_evals, 0.0)
        V_K = N.itq_matmul(T, U_K, col_scale=inv_sigma[:k].contiguous(), trans_a=True)
        return N.itq_matmul(H_i, U_K), N.itq_matmul(H_t, V_K)
    P_i, P_t = directions()
    V = torch.empty(2 * n, k, dtype=torch.float64, device=dev)

    def project():
        N.itq_project(gi, mu_i, alpha[0:1], P_i, out=V[:n])
        return N.itq_project(gt, mu_t, alpha[1:2], P_t, out=V[n:])
    project()
    R, obj, zz = N.itq_rotate(V, eye, iters)
    gpu = {"cross_moments": _gpu_ms(lambda: N.itq_cross_moments(gi, gt)),
           "covariance": _gpu_ms(lambda: N.itq_cca_covariance(si, st, cross, n)),
           "eigh_ii": _gpu_ms(lambda: N.itq_eigh(S_ii)), "eigh_tt": _gpu_ms(lambda: N.itq_eigh(S_tt)), "eigh_g": _gpu_ms(lambda: N.itq_eigh(G)),
           "products": _gpu_ms(lambda: (whiteners(), cross_products(), directions())),
           "project": _gpu_ms(project),
           "rotate": _gpu_ms(lambda: N.itq_rotate(V, eye, iters)),
           "heads": _gpu_ms(lambda: N.itq_heads_pair(P_i, P_t, R, mu_i, mu_t, alpha, zz, 2 * n))}
    # the host's chain
    h_mu_i, h_mu_t, h_alpha, h_ii, h_tt, h_it = CU.covariances(fi, ft)
    (h_sum_i, h_sq_i), (h_sum_t, h_sq_t), h_cross = U.moments(fi), U.moments(ft), CU.cross_moment(fi, ft)

    def host_covariances():                     # from the finished sums, as the GPU phase
        mi, mt = h_sum_i / n, h_sum_t / n
        ci, ct = h_sq_i / n - np.outer(mi, mi), h_sq_t / n - np.outer(mt, mt)
        ai, at = 1.0 / np.sqrt(np.trace(ci)), 1.0 / np.sqrt(np.trace(ct))
        return ai * ai * ci, at * at * ct, ai * at * (h_cross / n - np.outer(mi, mt))
    (h_lam_i, h_e_i), (h_lam_t, h_e_t) = U.eigh(h_ii), U.eigh(h_tt)

    def host_whiteners():
        return (h_e_i / np.sqrt(h_lam_i + r)) @ h_e_i.T, (h_e_t / np.sqrt(h_lam_t + r)) @ h_e_t.T
    h_h_i, h_h_t = host_whiteners()

    def host_cross():
        t = h_h_i @ h_it @ h_h_t
        return t, t @ t.T
    h_t_mat = host_cross()[0]
    h_u, h_sigma, h_vt = np.linalg.svd(h_t_mat)
    for j in range(d):                          # the product's sign rule, so that the codes can be compared
        if h_u[int(np.argmax(np.abs(h_u[:, j]))), j] < 0:
            h_u[:, j] = -h_u[:, j]

    def host_directions():
        v = h_t_mat.T @ h_u[:, :k] / h_sigma[:k]
        return h_h_i @ h_u[:, :k], h_h_t @ v
    h_p_i, h_p_t = host_directions()
    h_v = np.concatenate([U.project(fi, h_mu_i, h_alpha[0], h_p_i), U.project(ft, h_mu_t, h_alpha[1], h_p_t)])
    h_r, h_obj, h_z, _ = U.rotate(h_v, np.eye(k), iters)

    def host_heads():
        s = 0.5 / np.sqrt((h_z ** 2).mean())
        return [(s * a * (p @ h_r).T, -(s * a * (p @ h_r).T) @ mu) for a, mu, p in ((h_alpha[0], h_mu_i, h_p_i), (h_alpha[1], h_mu_t, h_p_t))]
    host = {"cross_moments": _host_ms(lambda: CU.cross_moment(fi, ft)),
            "covariance": _host_ms(host_covariances),
            "eigh_ii": _host_ms(lambda: U.eigh(h_ii)), "eigh_tt": _host_ms(lambda: U.eigh(h_tt)), "eigh_g": _host_ms(lambda: np.linalg.svd(h_t_mat)),
            "products": _host_ms(lambda: (host_whiteners(), host_cross(), host_directions())),
            "project": _host_ms(lambda: (U.project(fi, h_mu_i, h_alpha[0], h_p_i), U.project(ft, h_mu_t, h_alpha[1], h_p_t))),
            "rotate": _host_ms(lambda: U.rotate(h_v, np.eye(k), iters)),
            "heads": _host_ms(host_heads)}
    fits = {"gpu_cca_itq": _gpu_ms(lambda: fit_hash_heads(gi, gt, k, "cca", "itq", iters)["W_i"]),
            "gpu_pca_itq": _gpu_ms(lambda: fit_hash_heads(gi, gt, k, "pca", "itq", iters)["W_i"]),
            "host_cca_itq": _host_ms(lambda: CU.fit(fi, ft, k, "itq", iters)), "host_pca_itq": _host_ms(lambda: U.fit(fi, ft, k, "pca", "itq", iters))}
    codes = np.where(N.itq_step(V, R)[0].cpu().numpy() >= 0, 1.0, -1.0)
    sigma = np.sqrt(np.maximum(g_evals.cpu().numpy(), 0))
    return {"gpu_ms": gpu, "host_ms": host, "fit_ms": fits, "eigh_sweeps": [sw_i, sw_t, sw_g], "eigh_converged": [ok_i, ok_t, ok_g],
            "sigma_first_kth": [float(sigma[0]), float(sigma[k - 1])], "host_sigma_first_kth": [float(h_sigma[0]), float(h_sigma[k - 1])],
            "objective_first_last": [float(obj[0]), float(obj[-1])], "host_objective_first_last": [float(h_obj[0]), float(h_obj[-1])],
            "code_agreement_with_host": round(float((codes == np.where(h_z >= 0, 1.0, -1.0)).mean()), 6)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated NxDxK")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("itq_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        n, d, k = (int(x) for x in shape.split("x"))
        print(json.dumps(shape_line(n, d, k, args.iters, dev)), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
