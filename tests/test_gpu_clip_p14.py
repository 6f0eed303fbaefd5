"""Patch-14 CLIP towers (ViT-L/14, ViT-L/14@336px) on the GPU.  3 * 14^2 = 588 is not a multiple of the GEMM K-step and 14 not a
multiple of the patch gather's float4, so conv1 runs on a K-padded patch matrix (csrc/cmh_common.h: conv1_k, 588 -> 768).

- tiny widths (recipe.CLIP_TINY) with patch 14 at 56 / 112 / 336 px against the REFERENCE's own features and fp32 autograd gradients
  (tests/golden/make_golden18.py);
- ViT-L/14 size (24 layers, image width 1024 / 16 heads, text width 768 / 12 heads, embed 768) against oracle/clip_autograd.py in
  float64 on the GPU, bars of test_gpu_train_real_size_b16.py: f32 mode features within 1e-4, every gradient within 1e-4 of its
  largest element and its norm within 1e-4; bf16 mode every gradient's cosine >= 0.9995 and norm within 1 %;
- the pair paths, the per-launch GEMM route and the pad columns (workspace / tape filled with NaN first) at that geometry;
- the refusals that stay (fp8, MITH) and one product trainer end to end at 336 px."""
import numpy as np
import pytest
import torch

import make_golden18 as mg
import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 13
CFG_L14 = dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14, context_length=77,
               vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12)
CFG_L14_336 = dict(CFG_L14, image_resolution=336)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_after_module():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _get(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _state_dict(cfg):
    def make():
        if cfg is CFG_L14_336:
            # the 224 px tensors, and a positional embedding of 577 rows drawn from the recipe (a layer-free config: only that tensor is
            # read from it) - one full-size draw instead of two
            sd = dict(_state_dict(CFG_L14))
            small = recipe.clip_state_dict(dict(cfg, vision_layers=0, transformer_layers=0), SEED)
            sd["visual.positional_embedding"] = small["visual.positional_embedding"]
            return sd
        return recipe.clip_state_dict(cfg, SEED)
    return _get(("sd", id(cfg)), make)


def _model(cfg, sd=None, key=None):
    def make():
        from model.base.model import CLIP
        m = CLIP(cfg["embed_dim"], cfg["image_resolution"], cfg["vision_layers"], cfg["vision_width"], cfg["vision_patch_size"],
                 cfg["context_length"], cfg["vocab_size"], cfg["transformer_width"], cfg["transformer_heads"], cfg["transformer_layers"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in (sd if sd is not None else _state_dict(cfg)).items()}, strict=True)
        return m.to(DEV).float()
    return _get(("model", key or id(cfg)), make)


def _inputs(cfg, B):
    def make():
        image = recipe.images(B, cfg["image_resolution"], SEED)
        text = recipe.captions(B, cfg["context_length"], cfg["vocab_size"], SEED)
        g = torch.Generator().manual_seed(2000 + B)
        gi, gt = torch.randn(B, cfg["embed_dim"], generator=g), torch.randn(B, cfg["embed_dim"], generator=g)
        return tuple(torch.as_tensor(a).to(DEV) for a in (image, text, gi, gt))
    return _get(("inputs", id(cfg), B), make)


# ---------------------------------------------------------------------------------------------------- tiny, against the reference
def _tiny(res):
    cfg = mg.cfg_p14(res)
    return _model(cfg, recipe.clip_state_dict(cfg, mg.SEED), key=("tiny", res))


def _tiny_visual_grads(res, B, mode):
    cfg = mg.cfg_p14(res)
    m = _tiny(res).set_gemm_dtype(mode)
    m.zero_grad(set_to_none=True)
    image = torch.from_numpy(recipe.images(B, res, mg.SEED)).to(DEV)
    fi = m.encode_image(image)
    (fi * mg.cotangent(B, cfg["embed_dim"], res).to(DEV)).sum().backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in m.visual.named_parameters()}
    m.zero_grad(set_to_none=True)
    return fi.detach().cpu().numpy(), grads


@pytest.mark.parametrize("res,B", mg.CASES)
def test_tiny_p14_f32_mode_matches_reference(golden, res, B):
    g = golden("clip_p14.npz")
    fi, grads = _tiny_visual_grads(res, B, "f32")
    df = float(np.abs(fi - g[f"r{res}_img_feat"]).max())
    worst = 0.0
    for name in (str(n) for n in g[f"r{res}_names"]):
        ref = g[f"r{res}_g_{name}"]
        err = float(np.abs(mg.cut(grads[name]) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
        worst = max(worst, err)
        assert err <= 1e-4, (name, err)
    print(f"\npatch 14 at {res} px, f32: features max|d| {df:.2e}, worst gradient error {worst:.2e} of max")
    assert df <= 1e-4, df


@pytest.mark.parametrize("res,B", mg.CASES)
def test_tiny_p14_bf16_mode_tracks_reference(golden, res, B):
    g = golden("clip_p14.npz")
    fi, grads = _tiny_visual_grads(res, B, "bf16")
    r = g[f"r{res}_img_feat"]
    cos = (fi * r).sum(-1) / np.linalg.norm(fi, axis=-1) / np.linalg.norm(r, axis=-1)
    assert cos.min() > 0.9995 and np.abs(fi - r).max() < 0.05 * np.abs(r).max(), (cos.min(), np.abs(fi - r).max())
    stats = {}
    for name in (str(n) for n in g[f"r{res}_names"]):
        ref, got = g[f"r{res}_g_{name}"].astype(np.float64), mg.cut(grads[name]).astype(np.float64)
        stats[name] = (float(got @ ref / (np.linalg.norm(got) * np.linalg.norm(ref) + 1e-300)),
                       float(np.linalg.norm(grads[name].astype(np.float64))) / float(g[f"r{res}_n_{name}"]))
    worst = min(stats, key=lambda n: stats[n][0])
    print(f"\npatch 14 at {res} px, bf16: feature cosine min {cos.min():.6f}; worst gradient cosine {stats[worst][0]:.6f} ({worst}); "
          f"worst |norm ratio - 1| {max(abs(v[1] - 1) for v in stats.values()):.2e}")
    bad = {n: v for n, v in stats.items() if not (v[0] >= 0.9995 and abs(v[1] - 1) <= 0.01)}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- ViT-L/14 size, fp64 oracle
def _reference(cfg, B):
    def make():
        from oracle import clip_autograd as ca
        out = ca.towers(_state_dict(cfg), *_inputs(cfg, B), device=DEV)
        torch.cuda.empty_cache()
        return out
    return _get(("ref", id(cfg), B), make)


def _train(cfg, B, mode):
    m = _model(cfg).set_gemm_dtype(mode)
    m.zero_grad(set_to_none=True)
    image, text, gi, gt = _inputs(cfg, B)
    fi, ft = m.encode_image(image), m.encode_text(text)
    ((fi * gi).sum() + (ft * gt).sum()).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return fi.detach(), ft.detach(), grads


def _compare(got, ref, cfg):
    assert got.keys() == ref.keys(), set(got) ^ set(ref)
    assert len(ref) == 8 + 5 + 12 * (cfg["vision_layers"] + cfg["transformer_layers"])
    out = {}
    for n, r in ref.items():
        g = got[n].double()
        cos = float(g.flatten() @ r.flatten() / (g.norm() * r.norm() + 1e-300))
        out[n] = (float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300), float(g.norm() / r.norm()), cos)
    return out


L14_CASES = [pytest.param(CFG_L14, 8, id="224-B8"), pytest.param(CFG_L14, 5, id="224-B5"), pytest.param(CFG_L14_336, 2, id="336-B2")]


@pytest.mark.parametrize("cfg,B", L14_CASES)
def test_l14_f32_mode_gradients_match_fp64_autograd(cfg, B):
    rfi, rft, ref = _reference(cfg, B)
    fi, ft, got = _train(cfg, B, "f32")
    df = max(float((fi.double() - rfi).abs().max()), float((ft.double() - rft).abs().max()))
    st = _compare(got, ref, cfg)
    worst = max(st, key=lambda n: st[n][0])
    print(f"\nf32 ViT-L/14 {cfg['image_resolution']} px B={B}: features max|d| {df:.2e}; worst err/max {st[worst][0]:.2e} ({worst}); "
          f"worst |norm ratio - 1| {max(abs(v[1] - 1) for v in st.values()):.2e}")
    assert df <= 1e-4, df
    bad = {n: v for n, v in st.items() if not (v[0] <= 1e-4 and abs(v[1] - 1) <= 1e-4)}
    assert not bad, bad


@pytest.mark.parametrize("cfg,B", L14_CASES)
def test_l14_bf16_mode_gradients_track_fp64_autograd(cfg, B):
    _, _, ref = _reference(cfg, B)
    _, _, got = _train(cfg, B, "bf16")
    st = _compare(got, ref, cfg)
    worst = min(st, key=lambda n: st[n][2])
    print(f"\nbf16 ViT-L/14 {cfg['image_resolution']} px B={B}: worst cosine {st[worst][2]:.6f} ({worst}); worst |norm ratio - 1| "
          f"{max(abs(v[1] - 1) for v in st.values()):.2e}")
    bad = {n: v for n, v in st.items() if not (v[2] >= 0.9995 and abs(v[1] - 1) <= 0.01)}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- same bits, other paths
def test_l14_pair_paths_are_bit_identical_to_one_tower_calls():
    """cmh_clip_encode_pair / _pair2 with 24 image blocks (width 1024, T = 257) against 12 text blocks (width 768), and the two-stream
    training path (streams.overlapped, as the trainers call the towers) against one tower after the other.  token_embedding's
    gradient is a scatter of the rows' gradients with atomicAdd (csrc/encoders_bwd.hip, embed_scatter_kernel): ids that repeat in the
    batch (SOT, EOT) sum in arrival order, so that one tensor is compared to rounding, not bit for bit, on either path."""
    from streams import overlapped
    m = _model(CFG_L14).set_gemm_dtype("bf16")
    image, text, gi, gt = _inputs(CFG_L14, 5)
    with torch.no_grad():
        fi, ft = m.encode_image(image), m.encode_text(text)
        pi, pt = m.encode_pair(image, text)
        qi, qt = m.encode_pair2(image[:3], text[:3], image[3:], text[3:])
    assert torch.equal(pi, fi) and torch.equal(pt, ft)
    assert torch.equal(qi, fi) and torch.equal(qt, ft)

    def grads(two_streams):
        m.zero_grad(set_to_none=True)
        if two_streams:
            a, b = overlapped(lambda: m.encode_image(image), lambda: m.encode_text(text))
        else:
            a, b = m.encode_image(image), m.encode_text(text)
        ((a * gi).sum() + (b * gt).sum()).backward()
        out = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        return a.detach(), b.detach(), out
    si, st_, sg = grads(False)
    oi, ot, og = grads(True)
    assert torch.equal(si, fi) and torch.equal(oi, fi) and torch.equal(ot, st_)
    scatter = "token_embedding.weight"
    assert sg.keys() == og.keys() and scatter in sg
    assert all(torch.equal(sg[n], og[n]) for n in sg if n != scatter), [n for n in sg if n != scatter and not torch.equal(sg[n], og[n])]
    assert float((sg[scatter] - og[scatter]).abs().max()) <= 1e-5 * float(sg[scatter].abs().max())


def _l14_routes(B):
    """route of every ViT-L/14 block GEMM at batch B under the default mode, with the encoder's own epilogues (as
    tests/test_gemm_route.py): image tower (T = 257, width 1024), text tower (77 tokens, width 768: the dense row count, an upper bound
    of the packed one) and the pair path's grouped image + text launches.  0 the wide kernel, 3 the 12-wave 160-row form."""
    import cmh_native as N
    bias, res, gelu = N.EPI_BIAS | N.EPI_OUT_BF16, N.EPI_BIAS | N.EPI_RESIDUAL | N.EPI_RES_F16 | N.EPI_OUT_F16, \
        N.EPI_BIAS | N.EPI_QUICKGELU | N.EPI_OUT_BF16
    blocks = {"qkv": (3, 1, bias), "out": (1, 1, res), "fc1": (4, 1, gelu), "fc2": (1, 4, res)}      # N / width, K / width, epilogue
    routes = {}
    for name, (n, k, epi) in blocks.items():
        img, txt = (B * 257, n * 1024, k * 1024), (B * 77, n * 768, k * 768)
        routes["image_" + name] = N.gemm_route(img, None, epi)
        routes["text_" + name] = N.gemm_route(txt, None, epi)
        routes["pair_" + name] = N.gemm_route(img, txt, epi)
    return routes


def _reaches_lc3(routes):
    return any(v == 3 for k, v in routes.items() if k.startswith("image_")) and any(v == 3 for k, v in routes.items() if k.startswith("pair_"))


def test_l14_gemm_route_equals_wide_kernel():
    """The default per-launch route (wide kernel or the 160-row loader / consumer form, whichever the cost model prices lower) against
    the wide kernel alone, bit for bit, on ViT-L/14's launch shapes: N / K of 1024, 3072, 4096 in the image tower, 768 / 2304 / 3072
    in the text tower, and the grouped image-1024 / text-768 launches of the pair path.  The batch is the first of 32, 64 at which
    an image launch and a grouped launch take the 160-row form (the cost model gives it the image and grouped qkv and fc1 launches
    from B = 32; fc1 alone from B = 8)."""
    import cmh_native as N
    N.set_gemm_lc(-1)
    B = next((b for b in (32, 64) if _reaches_lc3(_l14_routes(b))), None)
    assert B is not None, {b: _l14_routes(b) for b in (32, 64)}
    routes = _l14_routes(B)
    print(f"\nViT-L/14 block launches, B = {B}: on the 160-row form {sorted(k for k, v in routes.items() if v == 3)}")
    m = _model(CFG_L14).set_gemm_dtype("bf16")
    image, text, _, _ = _inputs(CFG_L14, B)
    try:
        with torch.no_grad():
            fi, ft = m.encode_image(image), m.encode_text(text)
            pi, pt = m.encode_pair(image, text)
            N.set_gemm_lc(0)
            wi, wt = m.encode_image(image), m.encode_text(text)
            xi, xt = m.encode_pair(image, text)
    finally:
        N.set_gemm_lc(-1)
    assert torch.equal(fi, wi) and torch.equal(ft, wt)
    assert torch.equal(pi, xi) and torch.equal(pt, xt)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_p14_pad_columns_do_not_depend_on_dirty_scratch(monkeypatch, mode):
    """The patch matrix aliases scratch that earlier layers leave behind, and the tape is fresh memory: with both filled with NaN bytes
    first, the padded columns (zeros written on every call) keep the encode and the training forward and backward bit-identical"""
    import cmh_native as N
    from model.base import train_ops
    res, B = 112, 3
    m = _tiny(res).set_gemm_dtype(mode)
    image = torch.from_numpy(recipe.images(B, res, mg.SEED)).to(DEV)
    g = mg.cotangent(B, 64, res).to(DEV)

    def encode(fill):
        with torch.no_grad():
            m.encode_image(image)                           # sizes the cached workspace
            torch.cuda.synchronize()
            for key, buf in N._ws_cache.items():
                if key[2].startswith("vit@"):
                    buf.fill_(fill)
            return m.encode_image(image)
    clean, dirty = encode(0), encode(0xFF)
    assert torch.isfinite(clean).all() and torch.equal(clean, dirty)

    def train():
        m.zero_grad(set_to_none=True)
        f = m.encode_image(image)
        (f * g).sum().backward()
        out = {n: p.grad.clone() for n, p in m.visual.named_parameters()}
        m.zero_grad(set_to_none=True)
        return f.detach(), out
    f0, g0 = train()
    empty = torch.empty

    def poisoned(*a, **k):
        t = empty(*a, **k)
        if t.dtype == torch.uint8 and t.is_cuda:
            t.fill_(0xFF)
        return t
    monkeypatch.setattr(train_ops.torch, "empty", poisoned)
    f1, g1 = train()
    monkeypatch.undo()
    assert torch.isfinite(g0["conv1.weight"]).all()
    assert torch.equal(f0, f1)
    assert all(torch.equal(g0[n], g1[n]) for n in g0), [n for n in g0 if not torch.equal(g0[n], g1[n])]


# ---------------------------------------------------------------------------------------------------- what stays refused
def test_p14_fp8_mode_is_refused():
    import cmh_native as N
    m = _tiny(56)                                     # 17 image tokens: under the fp8 mode's token limit, refused for the patch
    with pytest.raises(N.NativeError, match="fp8 mode is not built for patch 14"):
        m.set_gemm_dtype("fp8")
    assert m._gemm_dtype != N.FP8


def test_p14_mith_is_refused_above_80_tokens():
    from model.MITH import build_model
    cfg = mg.cfg_p14(224)                             # 256 patch tokens, as ViT-L/14
    with pytest.raises(NotImplementedError, match="at most 80 tokens"):
        build_model({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, 7).items()})


# ---------------------------------------------------------------------------------------------------- a product trainer
def test_dsph_trains_a_patch14_checkpoint_at_336(tmp_path, monkeypatch):
    """main.py's DSPH trainer with a tiny patch-14 checkpoint at --resolution 336 (T = 577) on the synthetic set: the loss stays finite
    and falls from the first epoch to the last, and the evaluation returns four mAPs"""
    import argparse
    import sys
    import main
    import dataset.synthetic as ds
    ck = tmp_path / "clip_p14.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(mg.cfg_p14(336), 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510)
    monkeypatch.setattr(ds, "EOT", 511)
    monkeypatch.setattr(ds.SyntheticPairs, "signal", 2.0)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16",
                                      "--num-workers", "0", "--resolution", "336", "--max-words", "16", "--query-num", "32",
                                      "--train-num", "64", "--synthetic-size", "128", "--epochs", "0", "--gemm-dtype", "bf16",
                                      "--lr", "0.001", "--clip-lr", "0.0003"])
    torch.manual_seed(0)
    tr = main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    epochs = 4
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = epochs * len(tr.train_loader)
    losses = []
    step = tr._step
    monkeypatch.setattr(tr, "_step", lambda *a: losses.append(float(step(*a))) or torch.tensor(losses[-1]))
    for epoch in range(epochs):
        tr.train_epoch(epoch)
    per = len(tr.train_loader)
    first, last = np.mean(losses[:per]), np.mean(losses[-per:])
    maps = tr.valid(0)
    maps = [float(v) for v in (maps["long"] if isinstance(maps, dict) else maps)[:4]]
    print(f"\nDSPH, patch 14 at 336 px: loss {first:.4f} -> {last:.4f} over {len(losses)} steps; mAPs {maps}")
    assert len(losses) == epochs * per and np.isfinite(losses).all()
    assert last < first, losses
    assert len(maps) == 4 and all(0.0 <= v <= 1.0 for v in maps), maps
