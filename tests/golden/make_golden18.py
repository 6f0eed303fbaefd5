#!/usr/bin/env python3
"""Eighteenth golden generator — patch 14 (ViT-L/14's conv1, K = 3 * 14^2 = 588): the REFERENCE's CLIP.encode_image
(model/base/model.py, F.conv2d with any kernel size) on the tiny widths of recipe.CLIP_TINY with patch 14 at resolutions 56, 112 and
336 (T = 17, 65, 577), and its fp32 autograd gradients of L = sum(encode_image(image) * G) with respect to every visual parameter.
Outputs only; tensors above 4096 elements every 37th element (cut)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import recipe  # noqa: E402
from make_golden import build_ref_clip, install_stubs, save, t  # noqa: E402

SEED = 7
SLICE = 37
CASES = ((56, 3), (112, 3), (336, 2))          # (resolution, batch)


def cfg_p14(res):
    return dict(recipe.CLIP_TINY, vision_patch_size=14, image_resolution=res)


def cut(a):
    a = np.asarray(a).reshape(-1)
    return a[::SLICE].copy() if a.size > 4096 else a.copy()


def cotangent(B, E, res):
    return torch.randn(B, E, generator=torch.Generator().manual_seed(4000 + res))


def gen():
    out = {}
    for res, B in CASES:
        cfg = cfg_p14(res)
        clip = build_ref_clip(cfg, SEED)
        image = t(recipe.images(B, res, SEED))
        fi = clip.encode_image(image)
        (fi * cotangent(B, cfg["embed_dim"], res)).sum().backward()
        out[f"r{res}_img_feat"] = fi.detach().numpy()
        names = []
        for name, p in clip.visual.named_parameters():
            names.append(name)
            out[f"r{res}_g_{name}"] = cut(p.grad.numpy())
            out[f"r{res}_n_{name}"] = np.float64(p.grad.double().norm().item())
        out[f"r{res}_names"] = np.array(names)
        print(res, B, fi.shape, len(names), float(fi.detach().abs().max()))
    save("clip_p14.npz", **out)


if __name__ == "__main__":
    install_stubs()
    gen()
