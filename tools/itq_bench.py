"""Times of the training-free fit (csrc/itq.hip, utils/itq.py) on the GPU against its NumPy fp64 restatement on the host
(tests/itqutil.py: BLAS and LAPACK on the CPU) in the same process, one JSON line per shape; medians of 5 timed regions after a
warm-up.  GPU regions are timed with device events (the eigen-solver's per-sweep host reads fall inside its region), host regions
with perf_counter.

    python tools/itq_bench.py [--shapes 10000x512x64,100000x512x64] [--iters 50]

Phases: moments (both modalities' running sums), covariance (means, scales, pooled C), eigh (all D eigenpairs), project (both
modalities), rotate (`iters` ITQ iterations and the final pass), heads.  The features are already on the device / in host memory;
the upload is not part of either side.  Nothing is gated on these numbers."""
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
            "gpu_ms": gpu, "host_ms": host}


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
