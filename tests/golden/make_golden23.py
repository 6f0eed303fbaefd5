#!/usr/bin/env python3
"""Twenty-third golden generator — DDWSH: the REFERENCE's MarginLoss with its DistanceWeightedMiner (train/DDWSH/loss.py:7-128) and its
autograd gradients on the CPU, the step's three-call sum (train/DDWSH/hash_train.py:68) with its gradients, and three steps of a
training loop body on the tiny CLIP with four BertAdam groups.

The reference's forward reads `self.beta_constant`, which nothing sets; the generator sets `crit.beta_constant = False` from outside,
which alters no reference text.  Under np.random.seed(s) the miner is repeatable: seeding again and calling `crit.miner(cdist, labels)`
stand-alone returns the triplets the loss just used, and `inverse_sphere_distances` is a module-level function, so the sampling
distribution of every anchor is recorded as data.

    ddwsh.npz       per case and mode (intra: no `y`; cross): the triplets the reference drew under np.random.seed(case seed), the q row
                    of every valid anchor, loss, count (from the reference's own tensors), x.grad (and y.grad), beta.grad, `gap` (the
                    smallest |D_ap - beta_i + m| and |beta_i - D_an + m| over the triplets, float64) and `err` (the largest
                    float32-against-float64 difference of those distances); intra only, the `embeddings` space: the miner called on
                    F.normalize(x) - triplets and q; per case the step's sum with its three gradients and its [3, B, 2] triplets
    ddwsh_traj.npz  the three losses, each step's triplets, the final parameters (cut as mschutil.cut does) and the final beta

A triplet on the wrong side of a relu threshold changes the count by one, so a case is accepted only when gap >= 100 err;
--search prints, per case, the first seed from the committed one on that passes (put it into tests/ddwshutil.py::CASES)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ddwshutil as dw  # noqa: E402
import mschutil as ms  # noqa: E402
import ddbhutil as dd  # noqa: E402
import dchmtutil as du  # noqa: E402
from make_golden import build_ref_clip, install_stubs, ref_import, save, t  # noqa: E402


def ref_crit(mod, beta):
    crit = mod.MarginLoss(SimpleNamespace(margin=dw.MARGIN, nclass=len(beta), beta=dw.BETA))
    crit.beta_constant = False                                     # the attribute the reference reads and never sets
    crit.beta.data = t(np.asarray(beta, np.float32)).clone()
    return crit


def ref_cdist(x, y):
    """the distances of the reference's forward (:17-20)"""
    with torch.no_grad():
        return torch.cdist(F.normalize(x), F.normalize(y)).clamp(min=1e-8)


def as_rows(B, anchors, positives, negatives):
    trip = np.full((B, 2), -1, np.int32)
    for a, p, n in zip(anchors, positives, negatives):
        trip[a] = (p, n)
    return trip


def ref_q(mod, batch, lab):
    """the q row of every valid anchor, by calling inverse_sphere_distances as the miner does (:96, :115); zero rows elsewhere"""
    B = batch.shape[0]
    dist = mod.pdist(batch).clamp(min=dw.CUTOFF)
    q = np.zeros((B, B), np.float32)
    for i in range(B):
        if ((lab * lab[i]).sum(1) > 0).sum() > 1:
            row = mod.inverse_sphere_distances(batch, dist[i], lab, lab[i])
            if row is not None:
                q[i] = row
    return q


def ref_count(crit, cdist, lab, trip):
    """pair_count (:45) from the reference's own tensors"""
    a = np.flatnonzero(trip[:, 0] >= 0)
    if a.size == 0:
        return 0
    with torch.no_grad():
        al = t(lab)[a]
        beta = torch.einsum("nc,c->n", al, crit.beta) / al.sum(dim=1)
        pos = F.relu(cdist[a, trip[a, 0]] - beta + crit.margin)
        neg = F.relu(beta - cdist[a, trip[a, 1]] + crit.margin)
        return int(torch.sum((pos > 0.0) + (neg > 0.0)))


def condition(x, y, lab, beta, trip):
    """(gap, err) of one call on its triplets: see the module docstring"""
    exact = dw.margin_loss(x, y, lab, beta, trip)
    d32 = ref_cdist(t(x), t(y)).numpy().astype(np.float64)
    used = [(i, j) for i in range(len(trip)) if trip[i, 0] >= 0 for j in trip[i]]
    err = max([abs(d32[i, j] - exact["D"][i, j]) for i, j in used], default=0.0)
    return float(exact["gap"]), float(err)


def passes(gap, err):
    return gap >= 100.0 * err


def call(mod, c, mode, seed):
    """one reference call under np.random.seed(seed) -> dict of what is stored"""
    crit = ref_crit(mod, c["beta"])
    x = t(c["x"]).requires_grad_()
    y = x if mode == "intra" else t(c["y"]).requires_grad_()
    B = x.shape[0]
    cd = ref_cdist(x.detach(), y.detach())
    np.random.seed(seed)
    trip = as_rows(B, *crit.miner(cd, t(c["lab"])))
    np.random.seed(seed)
    loss = crit(x, t(c["lab"])) if mode == "intra" else crit(x, t(c["lab"]), y)
    zeros = np.zeros_like(c["x"])
    if torch.is_tensor(loss):
        loss.backward()
        out = dict(loss=np.float64(float(loss.detach())), gx=x.grad.numpy().copy(), gbeta=crit.beta.grad.numpy().copy())
        if mode == "cross":
            out["gy"] = y.grad.numpy().copy()
    else:                                                           # no triplet: the reference returns the tuple (0, 0)
        assert loss == (0, 0) and (trip < 0).all()
        out = dict(loss=np.float64(0.0), gx=zeros, gbeta=np.zeros_like(c["beta"]))
        if mode == "cross":
            out["gy"] = zeros
    gap, err = condition(c["x"], c["x"] if mode == "intra" else c["y"], c["lab"], c["beta"], trip)
    out.update(trip=trip, q=ref_q(mod, cd, c["lab"]), count=np.int64(ref_count(crit, cd, c["lab"], trip)), gap=np.float64(min(gap, 1e300)),
               err=np.float64(err))
    return out


def step_ref(crit, hi, ht, lab):
    """the loss line of the reference's loop body (hash_train.py:68)"""
    return crit(hi, lab) + crit(ht, lab) + crit(hi, lab, ht)


def step_trips(crit, hi, ht, lab, seed):
    """the triplets of a step's three calls, in the order the step draws them under one seed"""
    np.random.seed(seed)
    B = hi.shape[0]
    return np.stack([as_rows(B, *crit.miner(ref_cdist(a, b), lab)) for a, b in ((hi, hi), (ht, ht), (hi, ht))])


def valid_anchors(c):
    return int(dw.positives(c["lab"])[1].sum())


def gen_cases(mod):
    out = {}
    for c in dw.all_cases():
        tag, B = c["tag"], c["x"].shape[0]
        worst = {}
        for mode in dw.MODES:
            r = call(mod, c, mode, c["seed"])
            if (r["trip"] >= 0).any():
                assert passes(r["gap"], r["err"]), f"{tag} {mode}: gap {r['gap']:.3e} < 100 x {r['err']:.3e}: step the seed (--search)"
            for k, v in r.items():
                out[f"{tag}_{mode}_{k}"] = v
            w = dw.sphere_weights(dw.mining_matrix(dw.distances(c["x"], c["x"] if mode == "intra" else c["y"]), c["x"].shape[1])[0], c["lab"], B)
            tot = w.sum(1, keepdims=True)
            worst[mode] = float(np.abs(w / np.where(tot > 0, tot, 1.0) - r["q"]).max())
            print(f"{tag} {mode}: loss {float(r['loss']):.6f} count {int(r['count'])} triplets {int((r['trip'][:, 0] >= 0).sum())} of "
                  f"{valid_anchors(c)} valid anchors, gap {float(r['gap']):.3e} err {float(r['err']):.3e}, q deviation {worst[mode]:.3e}")
        # the paper's space, intra only: the miner on the unit rows themselves (dim = K)
        crit = ref_crit(mod, c["beta"])
        xn = F.normalize(t(c["x"]))
        np.random.seed(c["seed"])
        out[f"{tag}_emb_trip"] = as_rows(B, *crit.miner(xn, t(c["lab"])))
        out[f"{tag}_emb_q"] = ref_q(mod, xn, c["lab"])
        w = dw.sphere_weights(dw.mining_matrix(dw.distances(c["x"], c["x"]), c["x"].shape[1], space="embeddings")[0], c["lab"], c["x"].shape[1])
        tot = w.sum(1, keepdims=True)
        print(f"{tag} embeddings: q deviation {float(np.abs(w / np.where(tot > 0, tot, 1.0) - out[f'{tag}_emb_q']).max()):.3e}")
        # the step's three calls under one seed
        if valid_anchors(c):
            crit = ref_crit(mod, c["beta"])
            hi, ht, lab = t(c["x"]).requires_grad_(), t(c["y"]).requires_grad_(), t(c["lab"])
            trips = step_trips(crit, hi.detach(), ht.detach(), lab, c["seed"])
            for (a, b), tr in zip(((c["x"], c["x"]), (c["y"], c["y"]), (c["x"], c["y"])), trips):
                gap, err = condition(a, b, c["lab"], c["beta"], tr)
                assert passes(gap, err), f"{tag} step: gap {gap:.3e} < 100 x {err:.3e}: step the seed (--search)"
            np.random.seed(c["seed"])
            loss = step_ref(crit, hi, ht, lab)
            loss.backward()
            out[f"{tag}_step_loss"], out[f"{tag}_step_trips"] = np.float64(float(loss.detach())), trips
            out[f"{tag}_step_gi"], out[f"{tag}_step_gt"], out[f"{tag}_step_gbeta"] = hi.grad.numpy(), ht.grad.numpy(), crit.beta.grad.numpy().copy()
    save("ddwsh.npz", **out)


def gen_traj(mod):
    clip = build_ref_clip(du.CFG, du.SEED)
    LinearHash = ref_import("model.modelbase").LinearHash
    BertAdam = ref_import("model.base.optimization").BertAdam
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()   # (no dropout draw)
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    crit = ref_crit(mod, dw.traj_beta(du.C))
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}, {"params": crit.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    losses, trips, worst = [], [], np.inf
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        hi, ht = ih(clip.encode_image(img)), th(clip.encode_text(txt))
        tr = step_trips(crit, hi.detach(), ht.detach(), lab, dw.TRAJ_NP_SEED + step)
        a, b, beta = hi.detach().numpy(), ht.detach().numpy(), crit.beta.detach().numpy()
        for name, (x, y), rows in zip(("ii", "tt", "it"), ((a, a), (b, b), (a, b)), tr):
            gap, err = condition(x, y, lab.numpy(), beta, rows)
            print(f"trajectory step {step} {name}: {int((rows[:, 0] >= 0).sum())} triplets, gap {gap:.3e} err {err:.3e}")
            assert (rows[:, 0] >= 0).any() and passes(gap, err), f"trajectory step {step} {name}: change ddwshutil.TRAJ_NP_SEED"
            worst = min(worst, gap / max(err, 1e-300))
        np.random.seed(dw.TRAJ_NP_SEED + step)
        loss = step_ref(crit, hi, ht, lab.float())
        losses.append(float(loss.detach()))
        trips.append(tr)
        opt.zero_grad()
        loss.backward()
        opt.step()
    out = {"losses": np.array(losses, np.float64), "trips": np.stack(trips), "gap_over_err": np.float64(min(worst, 1e300)),
           "beta": crit.beta.detach().numpy().copy()}
    for name, p in list(clip.named_parameters()) + [("image_hash." + n, p) for n, p in ih.named_parameters()] + \
            [("text_hash." + n, p) for n, p in th.named_parameters()]:
        out["p_" + name] = ms.cut(p.detach().numpy())
    save("ddwsh_traj.npz", **out)
    print("losses", losses)


def search(mod):
    for (B, K, C, seed, p) in dw.CASES:
        for s in range(seed, seed + 4000):
            c = dw.ddwsh_case(B, K, C, s, p)
            if 2 * valid_anchors(c) < B:
                continue
            crit = ref_crit(mod, c["beta"])
            ok = all(passes(r["gap"], r["err"]) for r in (call(mod, c, mode, s) for mode in dw.MODES))
            if ok:
                trips = step_trips(crit, t(c["x"]), t(c["y"]), t(c["lab"]), s)
                ok = all(passes(*condition(a, b, c["lab"], c["beta"], tr))
                         for (a, b), tr in zip(((c["x"], c["x"]), (c["y"], c["y"]), (c["x"], c["y"])), trips))
            if ok:
                print(f"{c['tag']}: seed {s}")
                break
        else:
            print(f"B{B}_K{K}_C{C}: no seed in {seed} .. {seed + 3999}")


if __name__ == "__main__":
    install_stubs()
    m = ref_import("train.DDWSH.loss")
    if "--search" in sys.argv:
        search(m)
    else:
        gen_cases(m)
        gen_traj(m)
