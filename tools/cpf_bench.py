"""DScPH's loss per training step: the native proxy-fusion loss with its two quantisation terms (csrc/cpf.hip through train/DScPH)
against the reference's arithmetic written with torch ops and autograd on the same GPU in the same process (train/DScPH/CPF_loss.py:
24-54 and train/DScPH/hash_train.py:64-70, the identity rotation written as the sign change it is).

  loss  for B x K x C in {128 x 64 x 24, 256 x 64 x 24, 512 x 64 x 80, 1024 x 128 x 80}: forward + backward of CPF + q_img + q_txt with
        gradients for hi, ht and the proxies - one native forward call (5 launches) and one backward launch against the torch ops - wall
        clock around a device synchronise over regions of --calls calls, the two alternating in one process after a warm-up; values
        and gradients are compared first.
  step  one DScPHTrainer._step next to one DSPHTrainer._step (ViT-B/32, bf16 GEMMs, 77 tokens, 64 bits, batch 256): the same towers,
        heads and BertAdam under another loss (DSPH adds an SGD step for its proxies, DScPH a fourth BertAdam group).

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

from train.DScPH.loss import CPFLoss

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="loss,step")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=50, help="loss: calls per timed region")
ap.add_argument("--skip-torch", action="store_true", help="loss: the native path only")
a = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark measures a GPU; there is nothing to time without one"
dev = torch.device("cuda:0")
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 5, 1


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def wall(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def torch_step_loss(fn, hi, ht, y):
    """the step's loss with the torch ops the reference issues"""
    s, w = fn.scalars, F.normalize(fn.weight)
    total = 0.0
    for h in (hi, ht):
        cosine = F.linear(F.normalize(h), w)
        tp = ((cosine.clamp(min=0.0) * y) * 2).sum() + s["b"]
        lossp = ((1.0 - cosine) * torch.exp((1.0 - cosine) * s["sp"]).detach() * y).sum()
        mask = cosine > s["tau"]
        above = cosine[mask]
        lossn = ((above - s["psi"]) * torch.exp((above - s["mu"]) * s["sn"]).detach() * (1 - y[mask])).sum()
        z = F.normalize(-h)                                       # rot(h^T)^T of the identity HouseHolder
        sg = 1 / (1 + torch.exp(-z))
        total = total + (1.0 - tp / (tp + lossp + lossn)) + torch.mean(sg * (1 - sg))
    return total


def native_step_loss(fn, hi, ht, y):
    return fn(hi, ht, y)


def loss_part():
    for B, K, C in ((128, 64, 24), (256, 64, 24), (512, 64, 80), (1024, 128, 80)):
        g = torch.Generator().manual_seed(B + K)
        fn = CPFLoss(K, C).to(dev)
        with torch.no_grad():
            w = F.normalize(fn.weight)
            cls = torch.randint(0, C, (B,), generator=g).to(dev)
            noise = lambda: (0.2 + 0.6 * torch.rand(B, 1, generator=g)).to(dev) * F.normalize(torch.randn(B, K, generator=g).to(dev))
            hi, ht = (w[cls] + noise()).requires_grad_(), (w[cls] + noise()).requires_grad_()
            y = (torch.rand(B, C, generator=g) < (0.1 if C < 50 else 0.03)).float().to(dev)
            y[torch.arange(B), cls] = (torch.rand(B, generator=g) < 0.5).float().to(dev)

        def run(step):
            hi.grad = ht.grad = fn.weight.grad = None
            loss = step(fn, hi, ht, y)
            loss.backward()
            return loss.detach(), hi.grad, ht.grad, fn.weight.grad
        row = {"B": B, "K": K, "C": C, "native_launches": {"forward": FORWARD_LAUNCHES, "backward": BACKWARD_LAUNCHES}}
        nat = [x.clone() for x in run(native_step_loss)]
        t = {"native": [], "torch": []}
        if not a.skip_torch:
            ref = [x.clone() for x in run(torch_step_loss)]
            row["loss_native"], row["loss_torch"] = float(nat[0]), float(ref[0])
            row["grad_max_rel_diff"] = max(float((x - r).abs().max() / r.abs().max().clamp_min(1e-30)) for x, r in zip(nat[1:], ref[1:]))
        for _ in range(a.warmup):
            wall(lambda: run(native_step_loss), a.calls)
            if not a.skip_torch:
                wall(lambda: run(torch_step_loss), a.calls)
        for _ in range(a.reps):
            t["native"].append(wall(lambda: run(native_step_loss), a.calls))
            if not a.skip_torch:
                t["torch"].append(wall(lambda: run(torch_step_loss), a.calls))
        row["native"] = spread(t["native"])
        if not a.skip_torch:
            row["torch_ops"] = spread(t["torch"])
            row["ratio"] = round(row["torch_ops"]["median_ms"] / row["native"]["median_ms"], 2)
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
    tmp = tempfile.mkdtemp(prefix="cmh_cpf_bench_")
    batch, t = 256, {}
    for method, path in (("CPFH", ("train.DScPH.hash_train", "DScPHTrainer")), ("DSPH", ("train.DSPH.hash_train", "DSPHTrainer"))):
        tr, (image, text, label) = trainer(method, path, batch, tmp)
        one = lambda: wall(lambda: tr._step(image, text, label))
        for _ in range(a.warmup):
            one()
        t[method] = [one() for _ in range(a.reps)]
        del tr
        torch.cuda.empty_cache()
    out = {"what": f"_step, ViT-B/32, bf16 GEMMs, batch {batch}, 77 tokens, 64 bit", "CPFH": spread(t["CPFH"]), "DSPH": spread(t["DSPH"])}
    out["cpfh_minus_dsph_ms"] = round(out["CPFH"]["median_ms"] - out["DSPH"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
for part in a.parts.split(","):
    {"loss": loss_part, "step": step_part}[part]()
