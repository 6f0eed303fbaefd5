"""DDBH's loss per training step: the native five-term loss (csrc/ddbh.hip through train/DDBH) against the same loss written with
torch ops on the GPU in the row loop with host reads that upstream uses (train/DDBH/loss.py:15-78: per row two sorts and four .item()).

  loss  for B x K x C in {128 x 64 x 24, 256 x 64 x 24, 1024 x 128 x 80}: forward + backward of
        bp(hi, hi) + bp(ht, ht) + bp(hi, ht) + 0.1 (q(hi) + q(ht)), wall clock around a device synchronise, the two alternating in one
        process after a warm-up; the two values and gradients are compared first.
  step  one DDBHTrainer._step next to one DNpHTMMTrainer._step (ViT-B/32, bf16 GEMMs, 77 tokens, 64 bits, batch 128 and 256): the same
        towers, heads and optimiser under another loss, so the difference is the loss.

Medians of --reps timed regions with the spread (min .. max).  Needs a GPU; prints one JSON object per row."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np
import torch
import torch.nn.functional as F

from train.DDBH.loss import BPLoss, quantization_losses

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="loss,step")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-torch", action="store_true", help="loss: the native path only")
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


def torch_bp(bp, u, v, y):
    """the base-point loss with torch ops, one row at a time with the host reads upstream makes (log(1 + e^-f) as softplus(-f))"""
    s = (y @ y.t()) > 0
    inner = u @ v.t()
    c = np.log(bp.y_p / (99 * (1 - bp.y_p))) / bp.right
    ac = -np.log(99 * bp.y_p / (1 - bp.y_p)) / bp.left                      # a c with a = -ln(99 y_p / (1 - y_p)) / (left c)
    l2 = np.log((1 - bp.y_p) / bp.y_p)
    pos = neg = 0
    count = 0
    for i in range(u.shape[0]):
        if s[i].sum() != 0 and (~s[i]).sum() != 0:
            count += 1
            S, D = inner[i][s[i]], inner[i][~s[i]]
            mean_s = S.mean().clamp(bp.lowerBound, bp.upperBound).item()
            d_max = D.sort().values[int(len(D) * bp.percent):].mean().item()
            P = mean_s - (bp.upperBound - mean_s) / bp.upperBound * abs(mean_s - d_max)
            mean_d = D.mean().clamp(bp.lowerBound, bp.upperBound).item()
            s_min = S.sort(descending=True).values[int(len(S) * bp.percent):].mean().item()
            Q = mean_d - mean_d / bp.upperBound * abs(mean_d - s_min)
            f = torch.cat((c * S[S > P] + (l2 - c * P), ac * S[S < P] + (l2 - ac * P)))
            pos = pos + (f + F.softplus(-f)).mean()
            f = torch.cat((c * D[D < Q] + (l2 - c * Q), ac * D[D > Q] + (l2 - ac * Q)))
            neg = neg + F.softplus(-f).mean()
    return (pos + neg) / count if count else inner.sum() * 0.0


def torch_step_loss(bp, hi, ht, y):
    s = ((y @ y.t()) > 0).float()
    q = lambda h: (s @ (h - h.sign()).pow(2)).mean()
    return (torch_bp(bp, hi, hi, y) + torch_bp(bp, ht, ht, y) + torch_bp(bp, hi, ht, y)) + 0.1 * (q(hi) + q(ht))


def native_step_loss(bp, hi, ht, y):
    b = bp.losses([(hi, hi), (ht, ht), (hi, ht)], y)
    q = quantization_losses([hi, ht], y)
    return (b[0] + b[1] + b[2]) + 0.1 * (q[0] + q[1])


def loss_part():
    for B, K, C in ((128, 64, 24), (256, 64, 24), (1024, 128, 80)):
        g = torch.Generator().manual_seed(B + K)
        hi = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
        ht = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
        y = (torch.rand(B, C, generator=g) < (0.1 if C < 50 else 0.03)).float().to(dev)
        bp = BPLoss(K)

        def run(fn):
            hi.grad = ht.grad = None
            loss = fn(bp, hi, ht, y)
            loss.backward()
            return loss.detach(), hi.grad.clone(), ht.grad.clone()
        row = {"B": B, "K": K, "C": C}
        nat = run(native_step_loss)
        if not a.skip_torch:
            ref = run(torch_step_loss)
            row["loss_native"], row["loss_torch"] = float(nat[0]), float(ref[0])
            row["grad_max_rel_diff"] = max(float((x - r).abs().max() / r.abs().max()) for x, r in zip(nat[1:], ref[1:]))
        for _ in range(a.warmup):
            run(native_step_loss)
        t = {"native": [], "torch": []}
        for _ in range(a.reps):
            t["native"].append(wall(lambda: run(native_step_loss)))
            if not a.skip_torch:
                t["torch"].append(wall(lambda: run(torch_step_loss)))
        row["native"] = spread(t["native"])
        if not a.skip_torch:
            row["torch_row_loop"] = spread(t["torch"])
            row["ratio"] = round(row["torch_row_loop"]["median_ms"] / row["native"]["median_ms"], 1)
        print(json.dumps(row), flush=True)


def trainer(method, cls_path, batch, tmp):
    import importlib
    import main
    from bench import synthetic_batch
    from bench_configs import _vitb32_state
    mod, name = cls_path
    cls = getattr(importlib.import_module(mod), name)
    ck = os.path.join(tmp, "vitb32_random.pt")
    if not os.path.exists(ck):
        torch.save(_vitb32_state(11), ck)
    argv, run = sys.argv, cls.run
    sys.argv = ["main.py", "-clip-path", ck, "--save-dir", os.path.join(tmp, "run"), "--batch-size", str(batch), "--num-workers", "0",
                "--query-num", "64", "--train-num", "64", "--synthetic-size", "256", "--max-words", "77", "--gemm-dtype", "bf16",
                "--epochs", "1", "--save-mat", "false"]
    cls.run = lambda self: None
    try:
        torch.manual_seed(1)
        tr = main.trainers[method](argparse.Namespace(method=method, dataset="synthetic", output_dim=64, is_train=True), 0)
    finally:
        sys.argv, cls.run = argv, run
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = 100000
    tr.change_state(mode="train")
    return tr, synthetic_batch(batch, 77, tr.args.nclass, 7000, dev)


def step_part():
    tmp = tempfile.mkdtemp(prefix="cmh_ddbh_bench_")
    for batch in (128, 256):
        t = {}
        for method, path in (("DDBH", ("train.DDBH.hash_train", "DDBHTrainer")), ("DNpH", ("train.DNpH_TMM.hash_train", "DNpHTMMTrainer"))):
            tr, (image, text, label) = trainer(method, path, batch, tmp)
            one = lambda: wall(lambda: tr._step(image, text, label))
            for _ in range(a.warmup):
                one()
            t[method] = [one() for _ in range(a.reps)]
            del tr
            torch.cuda.empty_cache()
        out = {"what": f"_step, ViT-B/32, bf16 GEMMs, batch {batch}, 77 tokens, 64 bit", "DDBH": spread(t["DDBH"]), "DNpH": spread(t["DNpH"])}
        out["ddbh_minus_dnph_ms"] = round(out["DDBH"]["median_ms"] - out["DNpH"]["median_ms"], 3)
        print(json.dumps(out), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
for part in a.parts.split(","):
    {"loss": loss_part, "step": step_part}[part]()
