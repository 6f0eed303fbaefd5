"""oracle/clip_autograd.py at patch 14 (ViT-L/14's conv1, K = 588) against what the REFERENCE itself produced
(tests/golden/make_golden18.py: tiny widths, resolutions 56 / 112 / 336, T = 17 / 65 / 577): its encode_image features and its fp32
autograd gradients of L = sum(feat * G) with respect to every visual parameter.  This pins the fp64 yardstick of
tests/test_gpu_clip_p14.py to the reference at the patch size it checks."""
import numpy as np
import pytest
import torch

import make_golden18 as mg
import recipe
from oracle import clip_autograd as ca


@pytest.mark.parametrize("res,B", mg.CASES)
def test_patch14_visual_gradients_match_reference_autograd(golden, res, B):
    g = golden("clip_p14.npz")
    cfg = mg.cfg_p14(res)
    sd = {k: v for k, v in recipe.clip_state_dict(cfg, mg.SEED).items() if k.startswith("visual.")}
    p = ca.leaves(sd)
    fi = ca.encode_image(p, recipe.images(B, res, mg.SEED))
    (fi * mg.cotangent(B, cfg["embed_dim"], res).double()).sum().backward()
    np.testing.assert_allclose(fi.detach().numpy(), g[f"r{res}_img_feat"], rtol=1e-5, atol=1e-5)
    names = [str(n) for n in g[f"r{res}_names"]]
    assert sorted("visual." + n for n in names) == sorted(sd)
    worst = 0.0
    for name in names:
        got, ref, norm = p["visual." + name].grad.numpy(), g[f"r{res}_g_{name}"], float(g[f"r{res}_n_{name}"])
        assert abs(float(np.linalg.norm(got)) - norm) <= 2e-5 * max(norm, 1e-3), (name, float(np.linalg.norm(got)), norm)
        err = np.abs(mg.cut(got) - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err < 5e-5, (name, err)
    print(f"patch 14 at {res} px: fp64 oracle vs reference fp32 autograd, worst error {worst:.2e} of max over {len(names)} tensors")
