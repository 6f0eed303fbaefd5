"""DNPH's noise assignment per training step, host path against GPU path (train/DNPH_TOMM/b_reg.py: assign_noise).

  micro  for B in {128, 256, 300, 512} and K in {64, 128}: the host path of one step (both modalities: D2H, numpy cost matrices,
         scipy, H2D) by wall clock around a device synchronise, and the GPU path (cmh_assign_rows, P = 2, alone and inside
         assign_noise with the noise upload) by stream events; the two alternate A/B/A/B in one process after a warm-up.
  step   the whole DNPHTOMMTrainer._step at ViT-B/32 size (bf16 GEMMs, batch 256, 77 tokens, --bits bit) with --noise-assign gpu and
         host, alternating in one process, wall clock around a synchronise.

Medians with the spread (min .. max).  Needs a GPU; prints one JSON object per part.  CMH_ASSIGN_CPT (1 | 2 | 4) picks the
solver's columns per thread for a mapping comparison and is echoed in the output."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np
import torch

import cmh_native as N
from train.DNPH_TOMM.b_reg import assign_noise, rand_unit_rect

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="micro,step")
ap.add_argument("--reps", type=int, default=7, help="timed repetitions of each setting (micro)")
ap.add_argument("--steps", type=int, default=9, help="timed steps of each setting (step)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--bits", type=int, default=128)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--skip-host", action="store_true", help="micro: GPU path only (mapping comparisons)")
a = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark measures a GPU; there is nothing to time without one"
dev = torch.device("cuda:0")


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def micro():
    rows = []
    for B in (128, 256, 300, 512):
        for K in (64, 128):
            rng = np.random.RandomState(B * 1000 + K)
            hi = torch.from_numpy(np.tanh(rng.randn(B, K)).astype(np.float32)).to(dev)
            ht = torch.from_numpy(np.tanh(rng.randn(B, K)).astype(np.float32)).to(dev)
            np.random.seed(B + K)
            s = rand_unit_rect(B, K)
            s_dev = torch.from_numpy(s.astype(np.float32)).to(dev)
            emb = torch.stack((hi, ht))
            host = lambda: assign_noise(hi, ht, s, "host")
            gpu = lambda: assign_noise(hi, ht, s, "gpu")
            kern = lambda: N.assign_rows(emb, s_dev)
            same = None if a.skip_host else all(torch.equal(x, y) for x, y in zip(gpu(), host()))
            for _ in range(a.warmup):
                gpu(), kern()
            t = {"host": [], "gpu": [], "kernels": []}
            for _ in range(a.reps):
                if not a.skip_host:
                    t["host"].append(wall(host))
                t["gpu"].append(events(gpu))
                t["kernels"].append(events(kern))
            row = {"B": B, "K": K, "same_rows": same, "gpu_assign_noise": spread(t["gpu"]), "gpu_kernels": spread(t["kernels"])}
            if not a.skip_host:
                row["host"] = spread(t["host"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def trainer(bits, batch):
    import main
    from bench import synthetic_batch
    from bench_configs import _vitb32_state
    from train.DNPH_TOMM.hash_train import DNPHTOMMTrainer
    tmp = "/tmp/cmh_dnph_assign_bench"
    os.makedirs(tmp, exist_ok=True)
    ck = os.path.join(tmp, "vitb32_random.pt")
    torch.save(_vitb32_state(11), ck)
    argv, run = sys.argv, DNPHTOMMTrainer.run
    sys.argv = ["main.py", "-clip-path", ck, "--save-dir", os.path.join(tmp, "run"), "--batch-size", str(batch), "--num-workers", "0",
                "--query-num", "64", "--train-num", "64", "--synthetic-size", "256", "--max-words", "77", "--gemm-dtype", "bf16",
                "--epochs", "1", "--save-mat", "false"]
    DNPHTOMMTrainer.run = lambda self: None
    try:
        torch.manual_seed(1)
        tr = main.trainers["DNPH"](argparse.Namespace(method="DNPH", dataset="synthetic", output_dim=bits, is_train=True), 0)
    finally:
        sys.argv, DNPHTOMMTrainer.run = argv, run
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = 100000
    tr.change_state(mode="train")
    return tr, synthetic_batch(batch, 77, tr.args.nclass, 7000, dev)


def step():
    tr, (image, text, label) = trainer(a.bits, a.batch)
    t = {"gpu": [], "host": []}

    def one(how):
        tr.args.noise_assign = how
        tr.global_step += 1
        return wall(lambda: tr._step(image, text, label))
    for _ in range(a.warmup):
        one("gpu"), one("host")
    for _ in range(a.steps):
        t["gpu"].append(one("gpu"))
        t["host"].append(one("host"))
    out = {"what": f"DNPHTOMMTrainer._step, ViT-B/32, bf16 GEMMs, batch {a.batch}, 77 tokens, {a.bits} bit; settings alternate",
           "noise_assign_gpu": spread(t["gpu"]), "noise_assign_host": spread(t["host"])}
    out["gpu_is_faster"] = out["noise_assign_gpu"]["median_ms"] < out["noise_assign_host"]["median_ms"]
    print(json.dumps(out), flush=True)
    return out


print(json.dumps({"device": torch.cuda.get_device_name(0), "CMH_ASSIGN_CPT": os.environ.get("CMH_ASSIGN_CPT", "1 (default)"),
                  "host_threads": torch.get_num_threads()}), flush=True)
for part in a.parts.split(","):
    {"micro": micro, "step": step}[part]()
