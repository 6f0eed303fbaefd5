"""DJSRH's label-free loss per training step: target + loss forward + backward on the native path (csrc/djsrh.hip through train/DJSRH)
against the same arithmetic written as torch ops on the GPU (F.normalize, matmul, autograd) in the same process.

  loss  for B x K x D in {128 x 64 x 512, 300 x 64 x 512, 256 x 128 x 768}: a timed region is --iters back-to-back calls of
        target -> loss -> backward, wall clock around a device synchronise, per call; the two alternate after a warm-up; values and
        gradients are compared first.
  step  one DJSRHTrainer._step next to one DSPHTrainer._step (ViT-B/32, bf16 GEMMs, 77 tokens, 64 bits, batch 256): the same towers,
        heads and optimiser under another loss, so the difference is the loss (and DSPH's SGD step on its proxies).

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

from train.DJSRH.loss import JointSemanticsLoss

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="loss,step")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=200, help="loss: calls per timed region")
a = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark measures a GPU; there is nothing to time without one"
dev = torch.device("cuda:0")


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def wall(fn, iters=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def torch_loss(jsl, fi, ft, hi, ht):
    with torch.no_grad():
        ni, nt = F.normalize(fi), F.normalize(ft)
        st = jsl.beta * (2 * ni @ ni.t() - 1) + (1 - jsl.beta) * (2 * nt @ nt.t() - 1)
        S = jsl.mu * ((1 - jsl.eta) * st + (jsl.eta / st.shape[0]) * st @ st.t())
    bi, bt = F.normalize(hi), F.normalize(ht)
    return (jsl.lambda1 * ((bi @ bi.t() - S) ** 2).mean() + ((bi @ bt.t() - S) ** 2).mean() + jsl.lambda2 * ((bt @ bt.t() - S) ** 2).mean())


def native_loss(jsl, fi, ft, hi, ht):
    return jsl(hi, ht, jsl.target(fi, ft))


def loss_part():
    jsl = JointSemanticsLoss()
    for B, K, D in ((128, 64, 512), (300, 64, 512), (256, 128, 768)):
        g = torch.Generator().manual_seed(B + K + D)
        fi, ft = (torch.randn(B, D, generator=g).to(dev) for _ in range(2))
        hi, ht = (torch.tanh(torch.randn(B, K, generator=g)).to(dev).requires_grad_() for _ in range(2))

        def run(fn):
            hi.grad = ht.grad = None
            loss = fn(jsl, fi, ft, hi, ht)
            loss.backward()
            return loss.detach(), hi.grad, ht.grad
        nat, ref = run(native_loss), run(torch_loss)
        row = {"B": B, "K": K, "D": D, "loss_native": float(nat[0]), "loss_torch": float(ref[0]),
               "grad_max_rel_diff": max(float((x - r).abs().max() / r.abs().max()) for x, r in zip(nat[1:], ref[1:]))}
        for _ in range(a.warmup):
            wall(lambda: run(native_loss), a.iters)
            wall(lambda: run(torch_loss), a.iters)
        t = {"native": [], "torch": []}
        for _ in range(a.reps):
            t["native"].append(wall(lambda: run(native_loss), a.iters))
            t["torch"].append(wall(lambda: run(torch_loss), a.iters))
        row["native"], row["torch_ops"] = spread(t["native"]), spread(t["torch"])
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
    tmp = tempfile.mkdtemp(prefix="cmh_djsrh_bench_")
    batch = 256
    t = {}
    for method, path in (("DJSRH", ("train.DJSRH.hash_train", "DJSRHTrainer")), ("DSPH", ("train.DSPH.hash_train", "DSPHTrainer"))):
        tr, (image, text, label) = trainer(method, path, batch, tmp)
        if method == "DJSRH":                                   # a target cache of `batch` rows, filled as collect_targets fills it
            with torch.no_grad():
                tr.cache_i, tr.cache_t = tr.model.clip.encode_image(image).float(), tr.model.clip.encode_text(text).float()
            last = torch.arange(batch, device=dev)
        else:
            last = label
        one = lambda: wall(lambda: tr._step(image, text, last))
        for _ in range(a.warmup):
            one()
        t[method] = [one() for _ in range(a.reps)]
        del tr
        torch.cuda.empty_cache()
    out = {"what": f"_step, ViT-B/32, bf16 GEMMs, batch {batch}, 77 tokens, 64 bit", "DJSRH": spread(t["DJSRH"]), "DSPH": spread(t["DSPH"])}
    out["djsrh_minus_dsph_ms"] = round(out["DJSRH"]["median_ms"] - out["DSPH"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
for part in a.parts.split(","):
    {"loss": loss_part, "step": step_part}[part]()
