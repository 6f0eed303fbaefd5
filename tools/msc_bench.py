"""MSCH's loss per training step: the native all-triplets margin loss (csrc/msc.hip through train/MSCH) against the reference's arithmetic
written with torch ops and autograd on the same GPU in the same process (train/DPSIH/Loss.py:99-137: the [B, B, B] mask, torch.where,
two gathers of three index vectors, the length read on the host).

  loss  for B x K x C in {128 x 64 x 24, 256 x 64 x 24, 512 x 64 x 80, 1024 x 128 x 80} and both mining rules: forward + backward of
        100 (L(hi, hi) + L(ht, ht) + L(hi, ht)) - one native call of three pairs (2 forward launches + 1 backward launch) against three
        torch calls - wall clock around a device synchronise, the two alternating in one process after a warm-up; values, counts and
        gradients are compared first.  The torch route at B = 1024 holds index vectors of some 1e8 entries: it is timed once.
  step  one MSCHTrainer._step next to one DSPHTrainer._step (ViT-B/32, bf16 GEMMs, 77 tokens, 64 bits, batch 256): the same towers, heads
        and optimiser under another loss, so the difference is the loss.

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
import torch
import torch.nn.functional as F

from train.MSCH.loss import MSCLoss

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="loss,step")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-torch", action="store_true", help="loss: the native path only")
ap.add_argument("--torch-once-from", type=int, default=1024, help="loss: batches from this size on time the torch route once, without a warm-up")
a = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark measures a GPU; there is nothing to time without one"
dev = torch.device("cuda:0")
SCALE, MARGIN, FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 100.0, 0.25, 2, 1


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_msc(u, v, y, rule):
    """one call of the loss with the torch ops the reference issues -> (loss, active count)"""
    sim = -torch.matmul(u, v.t())
    sames = y @ y.t() > 0
    diffs = ~sames
    sames.fill_diagonal_(False)
    ai, pi, ni = torch.where(sames.unsqueeze(2) * diffs.unsqueeze(1))
    tm = sim[ai, ni] - sim[ai, pi]
    keep = tm <= MARGIN
    if rule == "semi-hard":
        keep &= tm > 0
    ai, pi, ni = ai[keep], pi[keep], ni[keep]
    if len(ai) == 0:                                            # the host read the reference makes
        return sim.sum() * 0.0, 0
    return F.relu(sim[ai, pi] - sim[ai, ni] + MARGIN).mean(), len(ai)


def torch_step_loss(fn, hi, ht, y):
    parts = [torch_msc(hi, hi, y, fn.mining), torch_msc(ht, ht, y, fn.mining), torch_msc(hi, ht, y, fn.mining)]
    return (parts[0][0] + parts[1][0] + parts[2][0]) * SCALE, [n for _, n in parts]


def native_step_loss(fn, hi, ht, y):
    return fn.losses([(hi, hi), (ht, ht), (hi, ht)], y).sum() * SCALE, None


def loss_part():
    import cmh_native as N
    for B, K, C in ((128, 64, 24), (256, 64, 24), (512, 64, 80), (1024, 128, 80)):
        for rule in ("all", "semi-hard"):
            g = torch.Generator().manual_seed(B + K)
            hi = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
            ht = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
            y = (torch.rand(B, C, generator=g) < (0.1 if C < 50 else 0.03)).float().to(dev)
            fn = MSCLoss(MARGIN, rule)

            def run(step):
                hi.grad = ht.grad = None
                loss, counts = step(fn, hi, ht, y)
                loss.backward()
                return loss.detach(), hi.grad.clone(), ht.grad.clone(), counts
            once = B >= a.torch_once_from
            row = {"B": B, "K": K, "C": C, "mining": rule, "native_launches": {"forward": FORWARD_LAUNCHES, "backward": BACKWARD_LAUNCHES}}
            nat = run(native_step_loss)
            row["active"] = N.msc_triplet_loss([(hi.detach(), hi.detach()), (ht.detach(), ht.detach()), (hi.detach(), ht.detach())], y,
                                               MARGIN, rule)[1].tolist()
            t = {"native": [], "torch": []}
            if not a.skip_torch:
                box = {}
                ms_once = wall(lambda: box.update(ref=run(torch_step_loss)))
                ref = box.pop("ref")
                if once:
                    t["torch"].append(ms_once)
                row["loss_native"], row["loss_torch"], row["active_torch"] = float(nat[0]), float(ref[0]), ref[3]
                row["grad_max_rel_diff"] = max(float((x - r).abs().max() / r.abs().max().clamp_min(1e-30)) for x, r in zip(nat[1:3], ref[1:3]))
                del ref
                torch.cuda.empty_cache()
            for _ in range(a.warmup):
                run(native_step_loss)
            for _ in range(a.reps):
                t["native"].append(wall(lambda: run(native_step_loss)))
                if not a.skip_torch and not once:
                    t["torch"].append(wall(lambda: run(torch_step_loss)))
            row["native"] = spread(t["native"])
            if not a.skip_torch:
                row["torch_ops"] = spread(t["torch"])
                row["torch_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
                row["ratio"] = round(row["torch_ops"]["median_ms"] / row["native"]["median_ms"], 1)
                torch.cuda.reset_peak_memory_stats()
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
    tmp = tempfile.mkdtemp(prefix="cmh_msc_bench_")
    batch, t = 256, {}
    for method, path in (("MSCH", ("train.MSCH.hash_train", "MSCHTrainer")), ("DSPH", ("train.DSPH.hash_train", "DSPHTrainer"))):
        tr, (image, text, label) = trainer(method, path, batch, tmp)
        one = lambda: wall(lambda: tr._step(image, text, label))
        for _ in range(a.warmup):
            one()
        t[method] = [one() for _ in range(a.reps)]
        del tr
        torch.cuda.empty_cache()
    out = {"what": f"_step, ViT-B/32, bf16 GEMMs, batch {batch}, 77 tokens, 64 bit", "MSCH": spread(t["MSCH"]), "DSPH": spread(t["DSPH"])}
    out["msch_minus_dsph_ms"] = round(out["MSCH"]["median_ms"] - out["DSPH"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
for part in a.parts.split(","):
    {"loss": loss_part, "step": step_part}[part]()
