"""Timings at ViT-B/16 (T = 197) and ViT-L/14 (T = 257) geometry on one GPU, one JSON line per measurement:
  attention forward (bf16) and attention backward (f32 / bf16, the tiled kernel past 128 tokens) at the image towers' shapes,
    with the achieved FLOP/s from the shapes (forward 4 B H T^2 64; backward 10 B H T^2 64: the five products of the statement,
    though the tiled kernel forms S and dO V^T three times each);
  ViT-B/16 image-tower encode and forward + backward (L = sum(feat * G)) ms per step at batch 256, bf16;
  ViT-L/14 and ViT-L/14@336px image towers (patch 14: the K-padded conv1), bf16: encode ms and pairs/s at batch 256; forward +
    backward of one step at batch `--train-batch` with the peak device memory of that step; and, from a kernel trace of one encode,
    the patchify, padded-weight copy and conv1 GEMM kernel times.
Timed by CUDA events around `--iters` back-to-back calls after `--warmup` calls (`--l14-iters` for the ViT-L/14 rows).
    python tools/vit_variant_bench.py [--iters 20] [--warmup 3] [--skip-attention] [--skip-tower] [--skip-l14] [--train-batch 64]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def attention(args):
    import backward_ops as Bo
    import cmh_native as N
    for name, B, T, d in (("ViT-B/16", 256, 197, 768), ("ViT-L/14", 32, 257, 1024)):
        H = d // 64
        for mode, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            qkv = torch.randn(B * T, 3 * d, device=DEV).to(dt)
            dout = torch.randn(B * T, d, device=DEV).to(dt)
            o = N.attention(qkv, B, T, False)
            rows = []
            if mode == "bf16":
                rows.append(("attention_forward", timed(lambda: N.attention(qkv, B, T, False), args.iters, args.warmup), 4))
            rows.append(("attention_backward", timed(lambda: Bo.attention_backward(qkv, o, dout, B, T, False), args.iters, args.warmup), 10))
            for kernel, ms, k in rows:
                flop = k * B * H * T * T * 64
                print(json.dumps({"what": kernel, "model": name, "mode": mode, "B": B, "T": T, "d": d, "ms": round(ms, 4),
                                  "tflops": round(flop / ms / 1e9, 2)}), flush=True)
            del qkv, dout, o
            torch.cuda.empty_cache()


def tower(args):
    import recipe
    from model.base.model import CLIP
    cfg = dict(recipe.CLIP_VITB32, vision_patch_size=16)
    B = 256
    m = CLIP(cfg["embed_dim"], cfg["image_resolution"], cfg["vision_layers"], cfg["vision_width"], cfg["vision_patch_size"],
             cfg["context_length"], cfg["vocab_size"], cfg["transformer_width"], cfg["transformer_heads"], cfg["transformer_layers"])
    m = m.to(DEV).float().set_gemm_dtype("bf16")
    image = torch.randn(B, 3, 224, 224, device=DEV)
    g = torch.randn(B, cfg["embed_dim"], device=DEV)

    def encode():
        with torch.no_grad():
            m.encode_image(image)

    def train():
        m.zero_grad(set_to_none=True)
        (m.encode_image(image) * g).sum().backward()

    for what, fn in (("vit_b16_image_encode", encode), ("vit_b16_image_forward_backward", train)):
        ms = timed(fn, args.iters, args.warmup)
        print(json.dumps({"what": what, "B": B, "mode": "bf16", "ms": round(ms, 3)}), flush=True)


def _clip(cfg):
    from model.base.model import CLIP
    return CLIP(cfg["embed_dim"], cfg["image_resolution"], cfg["vision_layers"], cfg["vision_width"], cfg["vision_patch_size"],
                cfg["context_length"], cfg["vocab_size"], cfg["transformer_width"], cfg["transformer_heads"], cfg["transformer_layers"])


def conv1_kernels(m, image):
    """Kernel times (us) of one encode's conv1: patchify, the padded-weight copy and the GEMM launched right after the copy."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
        m.encode_image(image)
        torch.cuda.synchronize()
    ks = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    out = {}
    for i, e in enumerate(ks):
        if "patchify" in e.name and "patchify_us" not in out:
            out["patchify_us"] = round(e.time_range.elapsed_us(), 1)
        if "copy_cols" in e.name and "weight_copy_us" not in out:
            out["weight_copy_us"] = round(e.time_range.elapsed_us(), 1)
            if i + 1 < len(ks):
                out["conv1_gemm_us"] = round(ks[i + 1].time_range.elapsed_us(), 1)
                out["conv1_gemm_kernel"] = ks[i + 1].name[:60]
    return out


def tower_l14(args):
    """ViT-L/14 (224 px, T = 257) and ViT-L/14@336px (T = 577): 24 layers, width 1024, 16 heads; patch 14 -> K = 588 padded to 768"""
    import recipe
    base = dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14, context_length=77,
                vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12)
    for name, res in (("ViT-L/14", 224), ("ViT-L/14@336px", 336)):
        cfg = dict(base, image_resolution=res)
        m = _clip(cfg).to(DEV).float().set_gemm_dtype("bf16")
        B = 256
        image = torch.randn(B, 3, res, res, device=DEV)

        def encode():
            with torch.no_grad():
                m.encode_image(image)

        ms = timed(encode, args.l14_iters, args.warmup)
        print(json.dumps({"what": "image_encode", "model": name, "B": B, "T": (res // 14) ** 2 + 1, "mode": "bf16", "ms": round(ms, 3),
                          "pairs_per_s": round(B / ms * 1e3, 1), **conv1_kernels(m, image)}), flush=True)
        del image
        Bt = args.train_batch
        image = torch.randn(Bt, 3, res, res, device=DEV)
        g = torch.randn(Bt, cfg["embed_dim"], device=DEV)

        def train():
            m.zero_grad(set_to_none=True)
            (m.encode_image(image) * g).sum().backward()

        train()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(train, args.l14_iters, 1)
        print(json.dumps({"what": "image_forward_backward", "model": name, "B": Bt, "mode": "bf16", "ms": round(ms, 3),
                          "peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)
        del m, image, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--skip-tower", action="store_true")
    ap.add_argument("--skip-l14", action="store_true")
    ap.add_argument("--l14-iters", type=int, default=5)
    ap.add_argument("--train-batch", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if not args.skip_attention:
        attention(args)
    if not args.skip_tower:
        tower(args)
    if not args.skip_l14:
        tower_l14(args)


if __name__ == "__main__":
    main()
