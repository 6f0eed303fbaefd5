#!/usr/bin/env python3
"""Twenty-first golden generator — MSCH: the REFERENCE's Multi_Semantic_Correlation_Loss (train/DPSIH/Loss.py:78-137) and its autograd
gradients on the CPU, the step's sum (:61-62) with its gradients, and three steps of a training loop body on the tiny CLIP.

The reference's trainer constructs the loss with the string "all" and indexes it with 0 or 1 (:39, :115-116), so it always mines `all`;
the generator selects a rule by passing the two-element list [rule, rule] as `hardness`, which alters no reference text.

    msch.npz       per case, rule (all, semi: semi-hard), mode (intra: no `inputs`; cross) and normalisation (n0 / n1): loss, count, u.grad
                   (and v.grad), `gap` (the smallest |tm - m| over the eligible triplets, under semi-hard also the smallest |tm|, float64)
                   and `err` (the largest float32-against-float64 difference of the similarities); per case the step's sum x 100 (rule
                   all, no normalisation: what DPSIH runs) and its two gradients
    msch_traj.npz  the three losses and the final parameters (cut as mschutil.cut does)

A triplet on the wrong side of a threshold changes the count and two coefficients by one, so a case is accepted only when gap >= 100 err;
--search prints, per case, the first seed from the committed one on that passes (put it into tests/mschutil.py::CASES)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import mschutil as ms  # noqa: E402
import ddbhutil as dd  # noqa: E402
import dchmtutil as du  # noqa: E402
from make_golden import build_ref_clip, install_stubs, ref_import, save, t  # noqa: E402

SHORT = {"all": "all", "semi-hard": "semi"}


def condition(u, v, lab, rule, normalize):
    """(gap, err) of one call: see the module docstring"""
    exact = ms.msc_loss(u, v, lab, ms.MARGIN, rule, normalize)
    a, b = t(u), t(v)
    if normalize:
        a, b = torch.nn.functional.normalize(a, p=2, dim=1), torch.nn.functional.normalize(b, p=2, dim=1)
    err = float(np.abs((-(a @ b.t())).numpy().astype(np.float64) - exact["s"]).max())
    return float(exact["gap"]), err


def passes(gap, err):
    return gap >= 100.0 * err


def variants(norms):
    return [(rule, mode, nz) for rule in ms.RULES for mode in ms.MODES for nz in norms]


def ref_call(mod, rule, nz, u, v, lab):
    """the reference's forward as its step calls it: `inputs` only on the cross-modal call (:61)"""
    loss_fn = mod.Multi_Semantic_Correlation_Loss(ms.MARGIN, [rule, rule], nz)
    return loss_fn(u, lab) if v is u else loss_fn(u, lab, v)


def step_loss_ref(mod, hi, ht, label):
    """the loss lines of DPSIHLoss.forward (:61-62) on given head outputs, with the loss as its constructor builds it (:39)"""
    fn = mod.Multi_Semantic_Correlation_Loss(ms.MARGIN, "all", False)
    return (fn(hi, label)[0] + fn(ht, label)[0] + fn(hi, label, ht)[0]) * 100


def gen_cases(mod):
    out = {}
    for (B, K, C, seed, norms) in ms.CASES:
        c = ms.msch_case(B, K, C, seed)
        tag, lab = c["tag"], t(c["lab"])
        for rule, mode, nz in variants(norms):
            key = f"{tag}_{SHORT[rule]}_{mode}_n{int(nz)}"
            gap, err = condition(c["u"], c["u"] if mode == "intra" else c["v"], c["lab"], rule, nz)
            assert passes(gap, err), f"{key}: gap {gap:.3e} < 100 x {err:.3e}: step the seed (--search)"
            u = t(c["u"]).requires_grad_()
            v = u if mode == "intra" else t(c["v"]).requires_grad_()
            loss, count = ref_call(mod, rule, nz, u, v, lab)
            if torch.is_tensor(loss):
                loss.backward()
            out[f"{key}_loss"], out[f"{key}_count"] = np.float64(float(loss)), np.int64(count)
            out[f"{key}_gu"] = u.grad.numpy() if u.grad is not None else np.zeros((B, K), np.float32)
            if mode == "cross":
                out[f"{key}_gv"] = v.grad.numpy() if v.grad is not None else np.zeros((B, K), np.float32)
            out[f"{key}_gap"], out[f"{key}_err"] = np.float64(gap), np.float64(err)
            print(f"{key}: loss {float(loss):.6f} count {count} gap {gap:.3e} err {err:.3e}")
        hi, ht = t(c["u"]).requires_grad_(), t(c["v"]).requires_grad_()
        loss = step_loss_ref(mod, hi, ht, lab)
        loss.backward()
        out[f"{tag}_step_loss"], out[f"{tag}_step_gi"], out[f"{tag}_step_gt"] = np.float64(float(loss)), hi.grad.numpy(), ht.grad.numpy()
    save("msch.npz", **out)


def gen_traj(mod):
    clip = build_ref_clip(du.CFG, du.SEED)
    LinearHash = ref_import("model.modelbase").LinearHash
    BertAdam = ref_import("model.base.optimization").BertAdam
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()   # (no dropout draw)
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    losses, worst = [], np.inf
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        hi, ht = ih(clip.encode_image(img)), th(clip.encode_text(txt))
        a, b = hi.detach().numpy(), ht.detach().numpy()
        for name, (x, y) in (("ii", (a, a)), ("tt", (b, b)), ("it", (a, b))):
            gap, err = condition(x, y, lab.numpy(), "all", False)
            print(f"trajectory step {step} {name}: gap {gap:.3e} err {err:.3e}")
            assert passes(gap, err), f"trajectory step {step} {name}: gap {gap:.3e} < 100 x {err:.3e}: change ddbhutil.TRAJ_SEEDS[{step}]"
            worst = min(worst, gap / max(err, 1e-300))
        loss = step_loss_ref(mod, hi, ht, lab.float())
        losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    out = {"losses": np.array(losses, np.float64), "gap_over_err": np.float64(min(worst, 1e300))}
    for name, p in list(clip.named_parameters()) + [("image_hash." + n, p) for n, p in ih.named_parameters()] + \
            [("text_hash." + n, p) for n, p in th.named_parameters()]:
        out["p_" + name] = ms.cut(p.detach().numpy())
    save("msch_traj.npz", **out)
    print("losses", losses)


def search():
    for (B, K, C, seed, norms) in ms.CASES:
        for s in range(seed, seed + 4000):
            c = ms.msch_case(B, K, C, s)
            if all(passes(*condition(c["u"], c["u"] if mode == "intra" else c["v"], c["lab"], rule, nz)) for rule, mode, nz in variants(norms)):
                print(f"{c['tag']}: seed {s}")
                break
        else:
            print(f"B{B}_K{K}_C{C}: no seed in {seed} .. {seed + 3999}")


if __name__ == "__main__":
    install_stubs()
    if "--search" in sys.argv:
        search()
    else:
        m = ref_import("train.DPSIH.Loss")
        gen_cases(m)
        gen_traj(m)
