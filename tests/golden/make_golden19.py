#!/usr/bin/env python3
"""Nineteenth golden generator — the anchor of tests/mithedgeutil.py: the REFERENCE's LocalizedTokenAggregation.forward
(model/MITH.py:317-376) on three tiny seeded inputs (one with ties at the top_k-th value, one with a key-padding mask that empties a
concept column, one with top_k = 3) with its autograd gradient w.r.t. the tokens, and BitwiseHashing.forward (:276-293) on one input
with its autograd gradients w.r.t. x, W and b.  The inputs come from mithedgeutil.anchor_*; only the reference's outputs are stored.
The reference is imported at generation time only.  The file is written with fixed zip timestamps, so a rerun gives the same bytes."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_stubs, meta, ref_import  # noqa: E402

import mithedgeutil as U  # noqa: E402


def save_fixed(name, **arrays):
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def gen():
    mm = ref_import("model.MITH")
    out = {}
    for i, (B, L, K, D, top_k, with_kpm, ties) in enumerate(U.ANCHOR_LTA):
        c = U.anchor_lta_case(i)
        x = c["tokens"].permute(1, 0, 2).clone().requires_grad_()                  # LND
        sim = c["sim"].permute(1, 0, 2).clone()                                    # LNK (the module masks it in place)
        merge, pseudo = mm.LocalizedTokenAggregation(top_k)(x, sim, None if c["kpm"] is None else c["kpm"].clone())
        merge.backward(c["dmerge"].permute(1, 0, 2))                               # KND
        out[f"lta{i}_merge"] = merge.detach().permute(1, 0, 2).numpy()             # -> [B, K, D]
        out[f"lta{i}_pseudo"] = pseudo.permute(1, 0, 2).numpy().astype(np.uint8)   # -> [B, L, K]
        out[f"lta{i}_dtokens"] = x.grad.permute(1, 0, 2).numpy()                   # -> [B, L, D]
    c = U.anchor_bithash_case()
    Bn, K, D = c["x"].shape
    bh = mm.BitwiseHashing(D, k_bits=K)
    with torch.no_grad():
        for k, fc in enumerate(bh.fc_list):
            fc.weight.copy_(c["w"][k:k + 1])
            fc.bias.copy_(c["b"][k:k + 1])
    x = c["x"].permute(1, 0, 2).clone().requires_grad_()                           # KND
    y = bh(x)
    y.backward(c["dy"])
    out.update(bh_y=y.detach().numpy(), bh_dx=x.grad.permute(1, 0, 2).numpy(),
               bh_dw=torch.cat([fc.weight.grad for fc in bh.fc_list]).numpy(), bh_db=torch.cat([fc.bias.grad for fc in bh.fc_list]).numpy())
    save_fixed("mith_edges.npz", meta=meta(), **out)


if __name__ == "__main__":
    install_stubs()
    torch.manual_seed(0)
    gen()
