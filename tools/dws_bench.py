"""DWSH's loss per training step: the native sampler and margin loss (csrc/dws.hip through train/DDWSH) against the reference's arithmetic
restated here with torch and numpy on the same GPU in the same process (train/DDWSH/loss.py:16-128: the labels copied to the host, the
Python loop over the B anchors, one [B] row of weights read back per anchor, two numpy draws per anchor).

  loss  for B x K x C in {128 x 64 x 24, 256 x 64 x 24, 512 x 64 x 80, 1024 x 128 x 80} and both mining spaces: forward + backward of
        L(hi) + L(ht) + L(hi, y=ht) - one native sampler call and one native loss call for the three pairs (8 forward launches, 7 in the
        `embeddings` space, + 2 backward) against three host loops - wall clock around a device synchronise, the two alternating in one
        process after a warm-up.  The draws differ (torch's generator here, numpy's there), so values are compared first on the
        baseline's OWN triplets, handed to the native loss.
  step  one DDWSHTrainer._step next to one DSPHTrainer._step (ViT-B/32, bf16 GEMMs, 77 tokens, 64 bits, batch 256): the same towers,
        heads and optimiser under another loss, so the difference is the loss.

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

from train.DDWSH.loss import MarginLoss

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="loss,step")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-host-loop", action="store_true", help="loss: the native path only")
ap.add_argument("--shapes", default="128x64x24,256x64x24,512x64x80,1024x128x80")
a = ap.parse_args()
assert torch.cuda.is_available(), "this benchmark measures a GPU; there is nothing to time without one"
dev = torch.device("cuda:0")
MARGIN, CUTOFF = 0.2, 0.5
LAUNCHES = {"distances": {"forward": 8, "backward": 2}, "embeddings": {"forward": 7, "backward": 2}}


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_loop_miner(batch, labels):
    """the miner as the reference runs it: the labels on the host, a Python loop over the anchors, the weights of one anchor computed on
    the GPU and read back, two numpy draws -> triplets int32 [B, 2] with (-1, -1) for a skipped anchor"""
    labels = labels.detach().cpu().numpy()
    bs, dim = batch.shape
    prod = batch @ batch.t()
    sq = prod.diag().unsqueeze(1).expand_as(prod)
    dist = (sq + sq.t() - 2 * prod).clamp(min=0).clamp(min=1e-4).sqrt().clamp(min=CUTOFF)
    trip = np.full((bs, 2), -1, np.int32)
    for i in range(bs):
        pos = (labels * labels[i]).sum(axis=1) > 0
        if pos.sum() <= 1 or pos.sum() == bs:
            continue
        d = dist[i]
        logw = (2.0 - float(dim)) * torch.log(d) - (float(dim - 3) / 2) * torch.log(torch.clamp(1.0 - 0.25 * d.pow(2), min=1e-8))
        same = np.where(pos)[0]
        logw[same] = 0
        w = torch.exp(logw - torch.max(logw))
        w[same] = 0
        q = (w / w.sum()).detach().cpu().numpy()                 # one device-to-host read per anchor
        pos[i] = False
        trip[i] = (np.random.choice(np.where(pos)[0]), np.random.choice(bs, p=q))
    return trip


def host_loop_loss(x, y, labels, beta, space):
    """one call of the reference's forward -> (loss, its triplets)"""
    xn = F.normalize(x)
    yn = xn if y is x else F.normalize(y)
    D = torch.cdist(xn, yn).clamp(min=1e-8)
    trip = host_loop_miner(D.detach() if space == "distances" else xn.detach(), labels)
    anc = np.flatnonzero(trip[:, 0] >= 0)
    if anc.size == 0:
        return D.sum() * 0.0, trip
    al = labels[anc]
    b = torch.einsum("nc,c->n", al, beta) / al.sum(dim=1)
    pos, neg = F.relu(D[anc, trip[anc, 0]] - b + MARGIN), F.relu(b - D[anc, trip[anc, 1]] + MARGIN)
    count = torch.sum((pos > 0.0) + (neg > 0.0))
    total = torch.sum(pos + neg)
    return (total if count == 0.0 else total / count), trip


def loss_part():
    for B, K, C in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        for space in ("distances", "embeddings"):
            g = torch.Generator().manual_seed(B + K)
            hi = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
            ht = torch.tanh(0.5 * torch.randn(B, K, generator=g)).to(dev).requires_grad_()
            y = (torch.rand(B, C, generator=g) < (0.1 if C < 50 else 0.03)).float().to(dev)
            fn = MarginLoss(C, MARGIN, 1.2, CUTOFF, space, seed=1).to(dev)
            np.random.seed(B)

            def native(trips=None):
                hi.grad = ht.grad = fn.beta.grad = None
                loss = fn(hi, ht, y, trips)
                loss.backward()
                return loss.detach(), hi.grad.clone(), ht.grad.clone(), fn.beta.grad.clone()

            def host():
                hi.grad = ht.grad = fn.beta.grad = None
                parts = [host_loop_loss(u, v, y, fn.beta, space) for u, v in ((hi, hi), (ht, ht), (hi, ht))]
                loss = parts[0][0] + parts[1][0] + parts[2][0]
                loss.backward()
                return (loss.detach(), hi.grad.clone(), ht.grad.clone(), fn.beta.grad.clone()), np.stack([p[1] for p in parts])
            row = {"B": B, "K": K, "C": C, "space": space, "native_launches": LAUNCHES[space]}
            t = {"native": [], "host_loop": []}
            if not a.skip_host_loop:
                ref, trips = host()
                nat = native(torch.from_numpy(trips).to(dev))
                row["triplets"] = int((trips[:, :, 0] >= 0).sum())
                row["loss_native_on_its_triplets"], row["loss_host_loop"] = float(nat[0]), float(ref[0])
                row["grad_max_rel_diff"] = max(float((x - r).abs().max() / r.abs().max().clamp_min(1e-30)) for x, r in zip(nat[1:], ref[1:]))
            for _ in range(a.warmup):
                native()
            for _ in range(a.reps):
                t["native"].append(wall(native))
                if not a.skip_host_loop:
                    t["host_loop"].append(wall(host))
            row["native"] = spread(t["native"])
            if not a.skip_host_loop:
                row["host_loop"] = spread(t["host_loop"])
                row["ratio"] = round(row["host_loop"]["median_ms"] / row["native"]["median_ms"], 1)
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
    tmp = tempfile.mkdtemp(prefix="cmh_dws_bench_")
    batch, t = 256, {}
    for method, path in (("DWSH", ("train.DDWSH.hash_train", "DDWSHTrainer")), ("DSPH", ("train.DSPH.hash_train", "DSPHTrainer"))):
        tr, (image, text, label) = trainer(method, path, batch, tmp)
        one = lambda: wall(lambda: tr._step(image, text, label))
        for _ in range(a.warmup):
            one()
        t[method] = [one() for _ in range(a.reps)]
        del tr
        torch.cuda.empty_cache()
    out = {"what": f"_step, ViT-B/32, bf16 GEMMs, batch {batch}, 77 tokens, 64 bit", "DWSH": spread(t["DWSH"]), "DSPH": spread(t["DSPH"])}
    out["dwsh_minus_dsph_ms"] = round(out["DWSH"]["median_ms"] - out["DSPH"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
for part in a.parts.split(","):
    {"loss": loss_part, "step": step_part}[part]()
