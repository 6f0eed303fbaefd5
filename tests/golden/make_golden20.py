#!/usr/bin/env python3
"""Twentieth golden generator — DDBH: the REFERENCE's BPLoss (train/DDBH/loss.py:5-101) and its autograd gradients on the CPU, the
trainer's five-term sum (train/DDBH/hash_train.py:64-78) with its gradients, and three steps of the training loop body on the tiny CLIP.
The reference's constructor calls super() on a name its module never binds (:7); the generator binds that name to the module's own BPLoss
for the run (a stand-in in the module's namespace, as make_golden15.py's for torch.cuda.FloatTensor; no reference text is altered).

    ddbh.npz       per case and mode (intra: v is u; cross): loss, u.grad (and v.grad); per case the step's sum and its two gradients;
                   per case and mode `gap` (the smallest |inner - BP|, |inner - BP_ds| over the kept classes, float64) and `err` (the
                   largest float32-against-float64 difference of inner, BP and BP_ds)
    ddbh_traj.npz  the three losses and the final parameters (cut as dchmtutil.cut does)

A flipped easy / hard decision changes one gradient entry by the factor a = 2, so a case is accepted only when gap >= 100 err; --search
prints, per case, the first seed from the committed one on that passes (put it into tests/ddbhutil.py::CASES / TRAJ_SEEDS)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ddbhutil as dd  # noqa: E402
import dchmtutil as du  # noqa: E402
from make_golden import build_ref_clip, install_stubs, ref_import, save, t  # noqa: E402


def ref_loss_module():
    mod = ref_import("train.DDBH.loss")
    mod.DAMHLoss = mod.BPLoss
    return mod


def condition(u, v, lab, sc):
    """(gap, err) of one (u, v) call: see the module docstring"""
    exact = dd.bp_loss(u, v, lab, sc, round_means=False)
    single = dd.bp_loss(u, v, lab, sc, inner=(t(u) @ t(v).t()).numpy(), round_means=True)
    act = exact["active"]
    err = float(np.abs((t(u) @ t(v).t()).numpy().astype(np.float64) - np.asarray(u, np.float64) @ np.asarray(v, np.float64).T).max())
    if act.any():
        err = max(err, float(np.abs(exact["bp"][act] - single["bp"][act]).max()), float(np.abs(exact["bpds"][act] - single["bpds"][act]).max()))
    return float(exact["gap"]), err


def passes(gap, err):
    return gap >= 100.0 * err


def step_loss_ref(bp, hi, ht, label):
    """the loss lines of the reference's train_epoch (hash_train.py:64-78), on given head outputs"""
    s = ((label @ label.t()) > 0).float()
    intra_i, intra_t, inter = bp(hi, hi, label), bp(ht, ht, label), bp(hi, ht, label)
    iq = torch.matmul(s, (hi - hi.sign()).pow(2)).mean()
    tq = torch.matmul(s, (ht - ht.sign()).pow(2)).mean()
    return (intra_i + intra_t + inter) + 0.1 * (iq + tq)


def gen_cases(mod):
    out = {}
    for (B, K, C, kind, seed) in dd.CASES:
        c = dd.ddbh_case(B, K, C, kind, seed)
        tag, sc, lab = c["tag"], dd.scalars(K), t(c["lab"])
        bp = mod.BPLoss(bit=K)
        for mode in dd.MODES:
            u = t(c["u"]).requires_grad_()
            v = u if mode == "intra" else t(c["v"]).requires_grad_()
            gap, err = condition(c["u"], c["u"] if mode == "intra" else c["v"], c["lab"], sc)
            assert passes(gap, err), f"{tag} {mode}: gap {gap:.3e} < 100 x {err:.3e}: step the seed (--search)"
            loss = bp(u, v, lab)
            if torch.is_tensor(loss):
                loss.backward()
            out[f"{tag}_{mode}_loss"] = np.float64(float(loss))
            out[f"{tag}_{mode}_gu"] = u.grad.numpy() if u.grad is not None else np.zeros((B, K), np.float32)
            if mode == "cross":
                out[f"{tag}_{mode}_gv"] = v.grad.numpy() if v.grad is not None else np.zeros((B, K), np.float32)
            out[f"{tag}_{mode}_gap"], out[f"{tag}_{mode}_err"] = np.float64(gap), np.float64(err)
            print(f"{tag} {mode}: loss {float(loss):.6f} gap {gap:.3e} err {err:.3e}")
        hi, ht = t(c["u"]).requires_grad_(), t(c["v"]).requires_grad_()
        loss = step_loss_ref(bp, hi, ht, lab)
        loss.backward()
        out[f"{tag}_step_loss"], out[f"{tag}_step_gi"], out[f"{tag}_step_gt"] = np.float64(float(loss)), hi.grad.numpy(), ht.grad.numpy()
    save("ddbh.npz", **out)


def gen_traj(mod):
    clip = build_ref_clip(du.CFG, du.SEED)
    LinearHash = ref_import("model.modelbase").LinearHash
    BertAdam = ref_import("model.base.optimization").BertAdam
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()   # (no dropout draw)
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    bp, sc = mod.BPLoss(bit=dd.TRAJ_K), dd.scalars(dd.TRAJ_K)
    losses, worst = [], np.inf
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        hi, ht = ih(clip.encode_image(img)), th(clip.encode_text(txt))
        a, b = hi.detach().numpy(), ht.detach().numpy()
        for name, (x, y) in (("ii", (a, a)), ("tt", (b, b)), ("it", (a, b))):
            gap, err = condition(x, y, lab.numpy(), sc)
            print(f"trajectory step {step} {name}: gap {gap:.3e} err {err:.3e}")
            assert passes(gap, err), f"trajectory step {step} {name}: gap {gap:.3e} < 100 x {err:.3e}: change TRAJ_SEEDS[{step}]"
            worst = min(worst, gap / max(err, 1e-300))
        loss = step_loss_ref(bp, hi, ht, lab.float())
        losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    out = {"losses": np.array(losses, np.float64), "gap_over_err": np.float64(worst)}
    for name, p in list(clip.named_parameters()) + [("image_hash." + n, p) for n, p in ih.named_parameters()] + \
            [("text_hash." + n, p) for n, p in th.named_parameters()]:
        out["p_" + name] = du.cut(p.detach().numpy())
    save("ddbh_traj.npz", **out)
    print("losses", losses)


def search():
    for (B, K, C, kind, seed) in dd.CASES:
        for s in range(seed, seed + 200):
            c = dd.ddbh_case(B, K, C, kind, s)
            if all(passes(*condition(c["u"], c["u"] if m == "intra" else c["v"], c["lab"], dd.scalars(K))) for m in dd.MODES):
                print(f"{c['tag']}: seed {s}")
                break
        else:
            print(f"B{B}_K{K}_C{C}_{kind}: no seed in {seed} .. {seed + 199}")


if __name__ == "__main__":
    install_stubs()
    if "--search" in sys.argv:
        search()
    else:
        m = ref_loss_module()
        gen_cases(m)
        gen_traj(m)
