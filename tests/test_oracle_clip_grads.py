"""oracle/clip_autograd.py (the fp64 autograd restatement of the two towers, checker of tests/test_gpu_train_real_size.py) against
what the REFERENCE itself produced: its fp32 autograd gradients on the tiny configuration (tests/golden/make_golden5.py) and its
ViT-B/32 features (tests/golden/make_golden.py, clip_vitb32.npz)."""
import numpy as np
import torch

import make_golden5 as mg
import recipe
from oracle import clip_autograd as ca


def test_tiny_tower_gradients_match_reference_autograd(golden):
    """Same seed, inputs, cotangents and cut() sampling as make_golden5.py.  The bounds are those of
    test_tower_gradients_match_reference_autograd (features 1e-4, gradient norms 2e-4, elements 5e-4 of max) or tighter: fp64 here
    against the reference's fp32 differs by the reference's own rounding only."""
    g = golden("clip_tiny_grads.npz")
    cfg, seed, B, L = recipe.CLIP_TINY, 7, 3, 16
    gi, gt = mg.cotangents(B, cfg["embed_dim"], 23)
    fi, ft, grads = ca.towers(recipe.clip_state_dict(cfg, seed), recipe.images(B, cfg["image_resolution"], seed),
                              recipe.captions(B, L, cfg["vocab_size"], seed), gi, gt)
    assert fi.dtype == torch.float64 and all(v.dtype == torch.float64 for v in grads.values())
    np.testing.assert_allclose(fi.numpy(), g["img_feat"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ft.numpy(), g["txt_feat"], rtol=1e-5, atol=1e-5)
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(grads), set(names) ^ set(grads)         # every tensor on the path, logit_scale off it
    worst = 0.0
    for name in names:
        got, ref, norm = grads[name].numpy(), g["g_" + name], float(g["n_" + name])
        assert abs(float(np.linalg.norm(got)) - norm) <= 2e-5 * max(norm, 1e-3), (name, float(np.linalg.norm(got)), norm)
        err = np.abs(mg.cut(got) - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err < 5e-5, (name, err)
    print(f"fp64 oracle vs reference fp32 autograd: worst error {worst:.2e} of max over {len(names)} tensors")


def test_vitb32_forward_matches_reference(golden):
    """The real-size configuration the GPU gradient tests run, B = 2: the feature rows the reference produced (fp32 reference against
    fp64 here, 12 blocks: the bound of test_oracle_clip.py's ViT-B/32 check)."""
    g = golden("clip_vitb32.npz")
    cfg, seed = recipe.CLIP_VITB32, int(g["seed"])
    p = ca.leaves(recipe.clip_state_dict(cfg, seed))
    with torch.no_grad():
        img = ca.encode_image(p, recipe.images(2, 224, seed)).numpy()
        txt = ca.encode_text(p, recipe.captions(2, 77, cfg["vocab_size"], seed)).numpy()
        txt32 = ca.encode_text(p, recipe.captions(2, 32, cfg["vocab_size"], seed + 1)).numpy()
    np.testing.assert_allclose(img, g["img_feat"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(txt, g["txt_feat_L77"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(txt32, g["txt_feat_L32"], rtol=1e-3, atol=1e-4)


def test_gradients_follow_the_loss():
    """The oracle's gradients are those of L = sum(img * Gi) + sum(txt * Gt): a central difference along a random direction of a few
    tensors agrees with <grad, direction> (fp64: to ~1e-8 relative), so the checker itself cannot be off by a transposition or a
    factor."""
    cfg = recipe.CLIP_TINY
    sd = recipe.clip_state_dict(cfg, 3)
    img, txt = recipe.images(2, cfg["image_resolution"], 3), recipe.captions(2, 16, cfg["vocab_size"], 3)
    txt[1, 1], txt[1, 2:] = cfg["vocab_size"] - 1, 0                        # EOT at position 1
    gi, gt = mg.cotangents(2, cfg["embed_dim"], 5)
    _, _, grads = ca.towers(sd, img, txt, gi, gt)
    gen = torch.Generator().manual_seed(0)
    for name in ("visual.conv1.weight", "visual.transformer.resblocks.1.attn.in_proj_weight", "token_embedding.weight",
                 "transformer.resblocks.0.mlp.c_fc.bias", "ln_final.weight", "positional_embedding"):
        v = torch.randn(sd[name].shape, generator=gen, dtype=torch.float64)
        v /= v.norm()

        def loss(eps):
            p = ca.leaves({**sd, name: torch.from_numpy(sd[name]).double() + eps * v})
            with torch.no_grad():
                return float((ca.encode_image(p, img) * gi.double()).sum() + (ca.encode_text(p, txt) * gt.double()).sum())
        h = 1e-5
        fd = (loss(h) - loss(-h)) / (2 * h)
        an = float((grads[name] * v).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (name, fd, an)
