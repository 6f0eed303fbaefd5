"""Times of the supervised training-free fit (csrc/dch.hip, utils/dch.py) on the GPU against NumPy fp64 on the host (BLAS and LAPACK
on the CPU) in the same process, one JSON line per shape; medians of 5 timed regions after a warm-up.  GPU regions are timed with
device events (the eigen-solver's per-sweep host reads fall inside its region), host regions with perf_counter.

    python tools/dch_bench.py [--shapes 10000x512x64x24,10000x512x64x80,100000x512x64x24,100000x512x64x80] [--iters 10]

Phases: moments (both modalities' running sums, the pooled C and S_ii, S_tt), eigh_inverse (the eigen-solves of S_ii and S_tt and the
two A_m; the host inverts S_mm + r I through LAPACK's eigh as well), eigh_start (the third eigen-solve, of C, and the start B), then
the pieces of ONE iteration - xtb (F_i^T B, F_t^T B and 1^T B), regress (the two P_m = A_m U_m), project (Z_i, Z_t), label (B^T B,
B^T Y and the solve for W), targets (G = W W^T, Q and the objective), dcc (`rounds` rounds over the bits) - and heads; `fit` is the
whole fit with `iters` iterations as one region on each side.  The host side is tests/dchutil.py's arithmetic, except that its
coordinate descent takes t = q_l - (B G[:, l] - b_l G[l][l]) with one BLAS product per bit where the restatement runs the kernel's
chain term by term: the bench gives the host its fastest form, the tests the comparable one.  The features are already on the
device / in host memory.  Nothing is gated on these numbers."""
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
SHAPES = "10000x512x64x24,10000x512x64x80,100000x512x64x24,100000x512x64x80"
ROUNDS, LAM, MU, REG = 3, 1.0, 0.01, 0.1


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


def host_dcc(q, g, b, rounds):
    """The coordinate descent with one BLAS product per bit (not the kernel's chain order: rounding-level differences in t)."""
    import numpy as np
    b = b.copy()
    for _ in range(rounds):
        for l in range(b.shape[1]):
            t = q[:, l] - (b @ g[:, l] - b[:, l] * g[l, l])
            b[:, l] = np.where(t > 0, 1.0, np.where(t < 0, -1.0, b[:, l]))
    return b


def host_fit(fi, ft, y, k, iters):
    """tests/dchutil.py's fit with host_dcc in the place of the chain."""
    import numpy as np
    import itqutil as IU
    import dchutil as U
    n, d = fi.shape
    mu_i, mu_t, alpha, cov = IU.covariance(IU.moments(fi), IU.moments(ft), n)
    x = [alpha[0] * (fi.astype(np.float64) - mu_i), alpha[1] * (ft.astype(np.float64) - mu_t)]
    inv = []
    for xm in x:
        lam, e = np.linalg.eigh(xm.T @ xm / n)
        inv.append((e / (lam + REG / d)) @ e.T)
    p0 = IU.eigh(cov)[1][:, :k]
    b = np.where(x[0] @ p0 + x[1] @ p0 >= 0, 1.0, -1.0)
    for _ in range(iters):
        z = [xm @ (a @ (xm.T @ b / n)) for xm, a in zip(x, inv)]
        w = U.label_regression(b, y, LAM)
        U.objective(y, b, w, z[0], z[1], LAM, MU)
        b = host_dcc(U.targets(y, w, z[0], z[1], MU), w @ w.T, b, ROUNDS)
    p = [a @ (xm.T @ b / n) for xm, a in zip(x, inv)]
    return b, p


def shape_line(n, d, k, c, iters, dev):
    import numpy as np
    import torch
    import cmh_native as N
    import dchutil as U
    import itqutil as IU
    from utils.dch import fit_supervised_heads, supervised_moments
    from utils.itq import MomentStream, whitener
    fi, ft, y = U.make_labelled(n, d, c, 1)
    gi, gt, gy = torch.from_numpy(fi).to(dev), torch.from_numpy(ft).to(dev), torch.from_numpy(y).float().to(dev)
    r = REG / d
    # the GPU's chain, each phase on the previous one's outputs
    mu_i, mu_t, alpha, cov, S_ii, S_tt = supervised_moments(MomentStream().add(gi, gt))
    sides = ((gi, mu_i, alpha[0:1]), (gt, mu_t, alpha[1:2]))

    def inverses():
        out = []
        for S in (S_ii, S_tt):
            H, sw, ok = whitener(S, r)
            out.append((N.itq_matmul(H, H, trans_b=True), sw, ok))
        return out
    inv = inverses()
    A = [inv[0][0], inv[1][0]]

    def start():
        evals, evecs, sw, ok = N.itq_eigh(cov)
        P0 = evecs[:, :k].contiguous()
        return N.dch_start(*(N.itq_project(F, m, a, P0) for F, m, a in sides)), sw, ok
    B, sw_c, ok_c = start()

    def xtb():
        return [N.dch_xtb(F, B, want_bsum=True) for F, _, _ in sides]
    TB = xtb()

    def regress():
        return [N.itq_matmul(A[m], N.dch_center(TB[m][0], TB[m][1], sides[m][1], sides[m][2], n)) for m in range(2)]
    P = regress()

    def project():
        return [N.itq_project(sides[m][0], sides[m][1], sides[m][2], P[m]) for m in range(2)]
    Z = project()

    def label():
        return N.dch_solve(N.dch_btb(B), N.dch_xtb(gy, B).t().contiguous(), LAM)
    W, info = label()

    def targets():
        return N.itq_matmul(W, W, trans_b=True), N.dch_targets(gy, B, W, Z[0], Z[1], MU, LAM)
    G, (Qt, obj2) = targets()
    B_before = B.clone()

    def dcc():
        B.copy_(B_before)                       # every region starts from the same codes (the copy is inside the region: N K bytes)
        return N.dch_dcc(Qt, G, B, ROUNDS)
    eye = torch.eye(k, dtype=torch.float64, device=dev)
    gpu = {"moments": _gpu_ms(lambda: supervised_moments(MomentStream().add(gi, gt))),
           "eigh_inverse": _gpu_ms(inverses), "eigh_start": _gpu_ms(start), "xtb": _gpu_ms(xtb), "regress": _gpu_ms(regress),
           "project": _gpu_ms(project), "label": _gpu_ms(label), "targets": _gpu_ms(targets), "dcc": _gpu_ms(dcc),
           "heads": _gpu_ms(lambda: N.itq_heads_pair(P[0], P[1], eye, mu_i, mu_t, alpha, obj2[1:2].contiguous(), 2 * n))}
    flips, margin = dcc()
    # the host's chain
    h_mu_i, h_mu_t, h_alpha, h_cov = IU.covariance(IU.moments(fi), IU.moments(ft), n)
    x = [h_alpha[0] * (fi.astype(np.float64) - h_mu_i), h_alpha[1] * (ft.astype(np.float64) - h_mu_t)]
    f64 = [fi.astype(np.float64), ft.astype(np.float64)]
    h_s = [xm.T @ xm / n for xm in x]

    def host_moments():
        si, st = IU.moments(fi), IU.moments(ft)
        mi, mt, al, cv = IU.covariance(si, st, n)
        return cv, al[0] ** 2 * (si[1] / n - np.outer(mi, mi)), al[1] ** 2 * (st[1] / n - np.outer(mt, mt))

    def host_inverses():
        out = []
        for s in h_s:
            lam, e = np.linalg.eigh(s)
            out.append((e / (lam + r)) @ e.T)
        return out
    h_inv = host_inverses()

    def host_start():
        p0 = IU.eigh(h_cov)[1][:, :k]
        return np.where(x[0] @ p0 + x[1] @ p0 >= 0, 1.0, -1.0)
    h_b = host_start()
    means, scales = (h_mu_i, h_mu_t), h_alpha

    def host_xtb():
        return [(f.T @ h_b, h_b.sum(0)) for f in f64]
    h_tb = host_xtb()

    def host_regress():
        return [h_inv[m] @ (scales[m] * (h_tb[m][0] - np.outer(means[m], h_tb[m][1])) / n) for m in range(2)]
    h_p = host_regress()

    def host_project():
        return [scales[m] * ((f64[m] - means[m]) @ h_p[m]) for m in range(2)]
    h_z = host_project()
    h_w = U.label_regression(h_b, y, LAM)

    def host_targets():
        return h_w @ h_w.T, U.targets(y, h_w, h_z[0], h_z[1], MU), U.objective(y, h_b, h_w, h_z[0], h_z[1], LAM, MU)
    h_g, h_q, h_obj = host_targets()

    def host_heads():
        zz = np.concatenate(h_z)
        s = 0.5 / np.sqrt((zz ** 2).mean())
        return [(s * a * p.T, -(s * a * p.T) @ m) for a, m, p in ((scales[0], means[0], h_p[0]), (scales[1], means[1], h_p[1]))]
    host = {"moments": _host_ms(host_moments), "eigh_inverse": _host_ms(host_inverses), "eigh_start": _host_ms(host_start),
            "xtb": _host_ms(host_xtb), "regress": _host_ms(host_regress), "project": _host_ms(host_project),
            "label": _host_ms(lambda: U.label_regression(h_b, y, LAM)), "targets": _host_ms(host_targets),
            "dcc": _host_ms(lambda: host_dcc(h_q, h_g, h_b, ROUNDS)), "heads": _host_ms(host_heads)}
    once = ("moments", "eigh_inverse", "eigh_start", "heads")
    for side in (gpu, host):
        side["per_iteration"] = round(sum(v for key, v in side.items() if key not in once), 3)
    fits = {"gpu": _gpu_ms(lambda: fit_supervised_heads(gi, gt, gy, k, iters, ROUNDS, LAM, MU, REG)["W_i"]),
            "host": _host_ms(lambda: host_fit(fi, ft, y, k, iters), regions=3)}
    got = fit_supervised_heads(gi, gt, gy, k, iters, ROUNDS, LAM, MU, REG)
    h_fit_b, _ = host_fit(fi, ft, y, k, iters)
    return {"tool": "dch_bench", "N": n, "D": d, "K": k, "C": c, "iters": iters, "rounds": ROUNDS, "regions": REGIONS,
            "eigh_sweeps": [inv[0][1], inv[1][1], sw_c], "eigh_converged": [inv[0][2], inv[1][2], ok_c], "solve_info": int(info),
            "one_iteration_flips": flips.cpu().tolist(), "one_iteration_min_margin": float(margin),
            "start_agreement_with_host": round(float((B_before.cpu().numpy() == h_b).mean()), 6),
            "fit_objective_first_last": [float(got["objective"][0]), float(got["objective"][-1])],
            "fit_min_margin": float(got["min_margin"].min()), "fit_flips_per_iteration": got["flips"].sum(1).cpu().tolist(),
            "fit_code_agreement_with_host": round(float((got["B"].cpu().numpy() == h_fit_b).mean()), 6),
            "host_threads": os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"]),
            "gpu_ms": gpu, "host_ms": host, "fit_ms": fits}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated NxDxKxC")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dch_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        n, d, k, c = (int(x) for x in shape.split("x"))
        print(json.dumps(shape_line(n, d, k, c, args.iters, dev)), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
