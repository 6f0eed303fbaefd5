#!/usr/bin/env python3
"""Twenty-second golden generator — DScPH: the REFERENCE's own CPF (train/DScPH/CPF_loss.py), HouseHolder and bit_var_loss
(train/DScPH/FAST_HPP.py) on the CPU with their autograd gradients, as the step uses them (train/DScPH/hash_train.py:64-70), and three
steps of that loop body on the tiny CLIP with the reference's four BertAdam groups (:37-44).

    dscph.npz       per case: the CPF loss, q_img and q_txt THROUGH the reference's rot (and `rot_dev`, the largest |rot(X) + X|: the
                    identity HouseHolder is X -> -X exactly), the step's sum, the gradients for hi and ht of the CPF part, of the two q
                    terms alone (the reference's modules in float64, see gen_cases) and (up to B = 33: the files stay small) of the whole step, the gradient for weight (the q terms do
                    not see it), `above` (the negatives and positives above tau), `gap` (the smallest of |c - tau| and |c| over both
                    modalities' non-zero cosines, float64) and `err` (the largest float32-against-float64 difference of the cosines)
    dscph_traj.npz  the three CPF losses and step sums, the final parameters (cut as mschutil.cut does) and the final proxies

A cosine on the wrong side of a threshold moves ln by about 0.2 e^-0.13, so a case is accepted only when gap >= 100 err; --search
prints, per case, the first seed from the committed one on that passes (put it into tests/dscphutil.py::CASES)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dscphutil as ds  # noqa: E402
import mschutil as ms  # noqa: E402
import ddbhutil as dd  # noqa: E402
import dchmtutil as du  # noqa: E402
from make_golden import build_ref_clip, install_stubs, ref_import, save, t  # noqa: E402


def ref_cpf(mod, W):
    cpf = mod.CPF(W.shape[1], W.shape[0], "cpu")
    cpf.weight.data = t(W).clone()
    return cpf


def condition(cpf, c):
    """(gap, err) of one case: see the module docstring"""
    exact = ds.cpf_step(c["hi"], c["ht"], c["W"], c["lab"])
    with torch.no_grad():
        wn = F.normalize(cpf.weight)
        cos32 = np.stack([F.linear(F.normalize(t(c[k])), wn).numpy() for k in ("hi", "ht")])
    return float(exact["gap"]), float(np.abs(cos32.astype(np.float64) - exact["cos"]).max())


def passes(gap, err):
    return gap >= 100.0 * err


def step_ref(cpf, rot, bit_var_loss, hi, ht, lab):
    """the loss lines of the reference's loop body (hash_train.py:64-70) -> CPF loss, q_img, q_txt, their sum (cpf None: the q lines alone)"""
    loss = cpf(hi, ht, lab) if cpf is not None else 0.0
    criterion = bit_var_loss()
    q_img, q_txt = criterion(F.normalize(rot(hi.T).T)), criterion(F.normalize(rot(ht.T).T))
    return loss, q_img, q_txt, loss + q_img + q_txt


def gen_cases(mod, fast):
    out = {}
    for c in ds.all_cases():
        tag, K = c["tag"], c["hi"].shape[1]
        cpf, rot = ref_cpf(mod, c["W"]), fast.HouseHolder(dim=K)
        gap, err = condition(cpf, c)
        assert passes(gap, err), f"{tag}: gap {gap:.3e} < 100 x {err:.3e}: step the seed (--search)"
        lab = t(c["lab"])
        # q: the two quantisation terms alone, about 1e-3 of the CPF gradient.  Their gradient is the remainder of a projection (in unit
        # space it is nearly parallel to the row), and the reference's float32 autograd carries up to 4e-5 of its maximum - more than the
        # tests' 2e-5: the reference's own rot and bit_var_loss are run in float64 for this one
        for part in ("q", "cpf", "step"):                            # (the step last: its values are what is stored below)
            wide = (lambda x: x.double()) if part == "q" else (lambda x: x)
            hi, ht = wide(t(c["hi"])).requires_grad_(), wide(t(c["ht"])).requires_grad_()
            cpf.weight.grad = None
            modules = (None, fast.HouseHolder(dim=K).double()) if part == "q" else (cpf, rot)
            loss, q_img, q_txt, total = step_ref(*modules, fast.bit_var_loss, hi, ht, lab)
            {"cpf": loss, "step": total, "q": q_img + q_txt}[part].backward()
            if part != "step" or hi.shape[0] <= ds.STEP_GRAD_MAX_B:   # (larger cases: the step's gradient is cpf + q, dscphutil.step_grad)
                out[f"{tag}_{part}_gi"], out[f"{tag}_{part}_gt"] = hi.grad.numpy().astype(np.float32), ht.grad.numpy().astype(np.float32)
            if part == "cpf":
                out[f"{tag}_cpf_gw"] = cpf.weight.grad.numpy().copy()
            elif part == "step":                                     # the q terms do not see the proxies
                assert np.array_equal(cpf.weight.grad.numpy(), out[f"{tag}_cpf_gw"])
        with torch.no_grad():
            x = t(c["hi"]).T
            out[f"{tag}_rot_dev"] = np.float64(float((rot(x) + x).abs().max()))
            above = [(F.linear(F.normalize(t(c[k])), F.normalize(cpf.weight)) > 0.9).numpy() for k in ("hi", "ht")]
        n_neg = sum(int((a & (c["lab"] == 0)).sum()) for a in above)
        n_pos = sum(int((a & (c["lab"] == 1)).sum()) for a in above)
        out[f"{tag}_cpf"] = np.float64(float(loss.detach()))
        out[f"{tag}_q_img"], out[f"{tag}_q_txt"] = np.float64(float(q_img.detach())), np.float64(float(q_txt.detach()))
        out[f"{tag}_step"], out[f"{tag}_gap"], out[f"{tag}_err"] = np.float64(float(total.detach())), np.float64(gap), np.float64(err)
        out[f"{tag}_above"] = np.array([n_neg, n_pos], np.int64)
        print(f"{tag}: cpf {float(loss):.6f} q {float(q_img):.6f} {float(q_txt):.6f} above tau: {n_neg} negatives, {n_pos} positives; "
              f"gap {gap:.3e} err {err:.3e} rot_dev {out[f'{tag}_rot_dev']:.1e}")
    save("dscph.npz", **out)


def gen_traj(mod, fast):
    clip = build_ref_clip(du.CFG, du.SEED)
    LinearHash = ref_import("model.modelbase").LinearHash
    BertAdam = ref_import("model.base.optimization").BertAdam
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()   # (no dropout draw)
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    cpf, rot = ref_cpf(mod, ds.traj_proxies()), fast.HouseHolder(dim=dd.TRAJ_K)
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}, {"params": cpf.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    losses, totals, worst = [], [], np.inf
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        hi, ht = ih(clip.encode_image(img)), th(clip.encode_text(txt))
        gap, err = condition(cpf, dict(hi=hi.detach().numpy(), ht=ht.detach().numpy(), W=cpf.weight.detach().numpy(), lab=lab.numpy()))
        print(f"trajectory step {step}: gap {gap:.3e} err {err:.3e}")
        assert passes(gap, err), f"trajectory step {step}: gap {gap:.3e} < 100 x {err:.3e}: change dscphutil.PROXY_SEED"
        worst = min(worst, gap / max(err, 1e-300))
        loss, _, _, total = step_ref(cpf, rot, fast.bit_var_loss, hi, ht, lab.float())
        losses.append(float(loss))
        totals.append(float(total))
        opt.zero_grad()
        total.backward()
        opt.step()
    out = {"losses": np.array(losses, np.float64), "totals": np.array(totals, np.float64), "gap_over_err": np.float64(min(worst, 1e300)),
           "proxies": cpf.weight.detach().numpy().copy()}
    for name, p in list(clip.named_parameters()) + [("image_hash." + n, p) for n, p in ih.named_parameters()] + \
            [("text_hash." + n, p) for n, p in th.named_parameters()]:
        out["p_" + name] = ms.cut(p.detach().numpy())
    save("dscph_traj.npz", **out)
    print("losses", losses, "totals", totals)


def search(mod):
    for (B, K, C, seed) in ds.CASES:
        for s in range(seed, seed + 4000):
            c = ds.dscph_case(B, K, C, s)
            if passes(*condition(ref_cpf(mod, c["W"]), c)):
                print(f"{c['tag']}: seed {s}")
                break
        else:
            print(f"B{B}_K{K}_C{C}: no seed in {seed} .. {seed + 3999}")


if __name__ == "__main__":
    install_stubs()
    m, f = ref_import("train.DScPH.CPF_loss"), ref_import("train.DScPH.FAST_HPP")
    if "--search" in sys.argv:
        search(m)
    else:
        gen_cases(m, f)
        gen_traj(m, f)
