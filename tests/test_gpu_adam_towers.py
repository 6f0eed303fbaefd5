"""The bf16 weight copies through the towers: after training steps, a CLIP whose copies were rewritten in place by the fused BertAdam step
encodes exactly what a fresh CLIP of the same f32 weights encodes, whose copies are cast anew.

The `bf16` case trains and encodes in the bf16 mode.  The fp8 mode is inference-only (a training forward in it is refused), so the `fp8`
case trains in the bf16 mode like the trainers do and then encodes in the fp8 mode, both models calibrated on the same batch: there conv1
reads the copy the optimiser kept, the blocks' e4m3 weights are lowered from the f32 values, and the transposed projections have no copy
at all and rely on the version bump of the step.  The fp8 kernels need a width that is a multiple of 256, which recipe.CLIP_TINY (128) is
not: the fp8 case runs CLIP_TINY at width 256, the configuration test_gpu_fp8.py uses for the same reason."""
import pytest
import torch

import adamutil as au
import recipe

pytestmark = pytest.mark.gpu
DEV = au.DEV
GEMM_WEIGHTS = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


FP8_TINY = dict(recipe.CLIP_TINY, vision_width=256, transformer_width=256, transformer_heads=4)     # as in test_gpu_fp8.py


def _clip(cfg, sd, mode):
    from model.base.model import CLIP
    m = CLIP(**cfg)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to(DEV).float().set_gemm_dtype(mode)


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_copies_stay_coherent_through_training_steps(mode):
    from model.base.optimization import BertAdam
    cfg, seed, B = (FP8_TINY if mode == "fp8" else recipe.CLIP_TINY), 5, 6
    sd = {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, seed).items()}
    m = _clip(cfg, sd, "bf16").train()
    img = torch.from_numpy(recipe.images(B, cfg["image_resolution"], seed)).to(DEV)
    txt = torch.from_numpy(recipe.captions(B, cfg["context_length"], cfg["vocab_size"], seed)).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    ci, ct = (torch.randn(B, cfg["embed_dim"], generator=gen).to(DEV) for _ in range(2))
    opt = BertAdam(m.parameters(), **au.CONFIGS["trainer"])
    names = {id(p): n for n, p in m.named_parameters()}
    expected = {f"{root}.resblocks.{i}.{w}" for root, layers in (("visual.transformer", cfg["vision_layers"]),
                                                               ("transformer", cfg["transformer_layers"]))
                for i in range(layers) for w in GEMM_WEIGHTS} | {"visual.conv1.weight"}
    assert expected <= set(names.values())
    copies_seen = None
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss = (m.encode_image(img) * ci).sum() + (m.encode_text(txt) * ct).sum()
        loss.backward()
        before = {n: p.detach().clone() for n, p in m.named_parameters() if n in expected}
        opt.step()
        with_copy = {names[id(p)]: p for p in m.parameters() if getattr(p, "_cmh_bf16", None) is not None}
        assert expected <= set(with_copy), sorted(expected - set(with_copy))
        for n, p in with_copy.items():
            c = p._cmh_bf16
            assert c.dtype == torch.bfloat16 and c.numel() == p.numel()
            assert p._cmh_bf16_version == (p.data_ptr(), p._version), n
            assert torch.equal(au.bf16_bits(c).reshape(-1), au.rne_bf16_bits(p).reshape(-1)), f"step {step}: copy of {n} != rne({n})"
        if step:                                                   # (step 0 of the warm-up has lr = 0)
            assert all(not torch.equal(before[n], with_copy[n].detach()) for n in expected)
            assert all(with_copy[n]._cmh_bf16 is copies_seen[n] for n in expected), "a copy was re-cast instead of rewritten in place"
        copies_seen = {n: p._cmh_bf16 for n, p in with_copy.items()}
    m.eval()
    fresh = _clip(cfg, m.state_dict(), "bf16").eval()
    assert not any(hasattr(p, "_cmh_bf16") for p in fresh.parameters())
    with torch.no_grad():
        if mode == "fp8":
            for model in (m, fresh):
                model.calibrate_fp8(img, txt)
                model.set_gemm_dtype("fp8")
            assert m._fp8_amax == fresh._fp8_amax
        fi, ft = m.encode_image(img), m.encode_text(txt)
        gi, gt = fresh.encode_image(img), fresh.encode_text(txt)
    assert m.gemm_dtype == fresh.gemm_dtype == mode
    assert torch.isfinite(fi).all() and torch.isfinite(ft).all() and fi.abs().sum() > 0
    assert torch.equal(fi.view(torch.int32), gi.view(torch.int32)), f"{mode}: image features of the trained model != a fresh model's"
    assert torch.equal(ft.view(torch.int32), gt.view(torch.int32)), f"{mode}: text features of the trained model != a fresh model's"
    assert m.visual.conv1.weight._cmh_bf16 is copies_seen["visual.conv1.weight"]                       # still the optimiser's copy
