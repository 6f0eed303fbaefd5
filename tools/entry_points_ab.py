"""Every forward entry point of the two towers, once, on seeded inputs: the check behind a change of the block sequencing
(csrc/encoders.hip, csrc/encoders_bwd.hip), which must leave every output bit and every launch as they were.

    python tools/entry_points_ab.py run OUT.json [towers|mith]        one library (CMH_LIB picks it), a fresh process each; every leg
                                                                       or one: the towers' entry points, or MITH (trunk + HashingModel:
                                                                       forward, three BertAdam steps) - the check behind a change of
                                                                       the Python layer, run on two Python trees over ONE library
    python tools/entry_points_ab.py compare A.json B.json [A2.json]   per-entry-point verdict; exit status 1 on any difference
                                                                       (A2: a second run of A - what it does not reproduce is named, not compared)
    python tools/entry_points_ab.py launches TRACE_DIR [TRACE_DIR_B]  digest of the ordered (kernel, grid, workgroup) list per stream
                                                                       of `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- ... run`
                                                                       runs; with two, their first difference and exit status 1

`run` records the sha256 of every output's bytes (features, token matrices, amax arrays, every gradient).  The device is synchronised
between entry-point calls, so that the packed text path's tile-height hint (the previous call's row count, taken only when its event
has completed) is the same in every run.

Training legs: every tower's forward + backward with the pooled tail on and off (the bridges' three backward parts), the backward
again as two parts (cmh_*_backward_part over layers .. a, a .. 0), and - at the `tiny` and `vitb32` bf16 configs - once with each of
the block backward's two switches off: the 16-bit gradient stream (cmh_set_grad_stream16(0)) and the one-launch wgrad
(CMH_WGRAD_MULTI=0, which the library reads at every call: `run` sets it for that leg and takes it away again, in one process)."""
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

VITL14_CUT = dict(embed_dim=768, image_resolution=224, vision_layers=3, vision_width=1024, vision_patch_size=14, context_length=77,
                  vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=3)       # ViT-L/14 shapes, 3 blocks
MIXED = dict(embed_dim=256, image_resolution=224, vision_layers=3, vision_width=768, vision_patch_size=32, context_length=77,
             vocab_size=49408, transformer_width=384, transformer_heads=6, transformer_layers=2)             # fp16 / f32 streams, 3 / 2 blocks


def run(out_path, legs="all"):
    import numpy as np
    import torch
    import cmh_native as N
    import mith_ops
    import mith_train_ops
    import recipe
    from model.base import train_ops as T
    from model.base.model import CLIP, _fill_blocks

    dev = "cuda:0"
    digests = {}

    def keep(key, t):
        torch.cuda.synchronize()
        a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
        assert key not in digests, key
        digests[key] = f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.dtype} {list(a.shape)}"

    def inputs(cfg, B, L, seed):
        img = torch.from_numpy(recipe.images(B, cfg["image_resolution"], seed)).to(dev)
        txt = torch.from_numpy(recipe.captions(B, L, cfg["vocab_size"], seed)).to(dev)
        return img, txt, (txt == 0)

    def model(cfg, seed):
        torch.manual_seed(seed)
        return CLIP(**cfg).to(dev).float()

    def inference(tag, m, img, txt, kpm, modes, full):
        m.assume_frozen = True
        with torch.no_grad():
            for mode in modes:
                if mode == "fp8":
                    m.set_gemm_dtype("bf16")
                    fi, ft = m.calibrate_fp8(img, txt)
                    keep(f"{tag}/calibrate/image", fi), keep(f"{tag}/calibrate/text", ft)
                    keep(f"{tag}/calibrate/amax_vit", np.asarray(m._fp8_amax["vit"], np.float32))
                    keep(f"{tag}/calibrate/amax_text", np.asarray(m._fp8_amax["text"], np.float32))
                m.set_gemm_dtype(mode)
                for tail in (True, False):
                    N.set_pooled_tail(tail)
                    k = f"{tag}/{mode}/tail{int(tail)}"
                    keep(f"{k}/vit_encode", m.encode_image(img))
                    for pack in (False, True):
                        m.pack_text = pack
                        keep(f"{k}/text_encode{'_packed' if pack else ''}", m.encode_text(txt))
                        m.drop_pair_stash()
                        fi, ft = m.encode_pair(img, txt)
                        keep(f"{k}/pair/pack{int(pack)}/image", fi), keep(f"{k}/pair/pack{int(pack)}/text", ft)
                        h = img.shape[0] // 2
                        fi, ft = m.encode_pair2(img[:h].contiguous(), txt[:h], img[h:].contiguous(), txt[h:])
                        keep(f"{k}/pair2/pack{int(pack)}/image", fi), keep(f"{k}/pair2/pack{int(pack)}/text", ft)
                N.set_pooled_tail(True)
                if mode == "fp8" or not full:
                    continue
                keep(f"{tag}/{mode}/text_encode_mask", m.encode_text(txt, key_padding_mask=kpm))
                keep(f"{tag}/{mode}/vit_encode_tokens", mith_ops.vit_encode_tokens(m, img))
                for packed in (False, True):
                    tok, rows = mith_ops.text_encode_tokens(m, txt, kpm, padded_unused=packed)
                    keep(f"{tag}/{mode}/text_encode_tokens{'_packed' if packed else ''}", tok)
                    keep(f"{tag}/{mode}/text_encode_tokens{'_packed' if packed else ''}/eot", rows)
                if mode == "f32":
                    s = m._vit_struct()
                    Tn = (s.resolution // s.patch) ** 2 + 1
                    taps = [torch.empty(img.shape[0] * Tn, s.width, device=dev) for _ in range(1 + s.layers)]
                    keep(f"{tag}/f32/vit_encode_taps", m.encode_image(img, taps=taps))
                    for i, t in enumerate(taps):
                        keep(f"{tag}/f32/vit_encode_taps/{i}", t)
                    s = m._text_struct()
                    taps = [None] + [torch.empty(txt.numel(), s.width, device=dev) for _ in range(s.layers)]
                    keep(f"{tag}/f32/text_encode_taps", m.encode_text(txt, taps=taps))
                    for i, t in enumerate(taps[1:]):
                        keep(f"{tag}/f32/text_encode_taps/{1 + i}", t)
                # a bare stack of blocks (the concept transformer): two of the text tower's
                blocks, held = m.transformer.resblocks[:2], []
                arr = _fill_blocks(blocks, N.BF16 if mode == "bf16" else N.F32, held)
                d = blocks[0].ln_1.weight.shape[0]
                x = torch.randn(32 * 8, d, device=dev, generator=torch.Generator(dev).manual_seed(5))
                keep(f"{tag}/{mode}/transformer_blocks", mith_ops.transformer_blocks(arr, 2, x, 32, 8, N.BF16 if mode == "bf16" else N.F32))

    def grads_of(key, params):
        for i, p in enumerate(params):
            keep(f"{key}/grad{i}", p.grad)
            p.grad = None

    def training(tag, m, img, txt, kpm, modes, full, switches=False):
        m.assume_frozen = False
        gen = torch.Generator(dev).manual_seed(3)
        vp, tp = T.vit_params(m.visual), T.text_params(m)
        calls = (("vit", vp, lambda: m.encode_image(img)), ("text", tp, lambda: m.encode_text(txt)),
                 ("text_mask", tp, lambda: m.encode_text(txt, key_padding_mask=kpm)))

        def towers(k, some):
            for name, params, call in some:
                f = call()
                keep(f"{k}/{name}_forward_train", f)
                f.backward(torch.randn(f.shape, device=dev, generator=gen))
                grads_of(f"{k}/{name}_backward", params)

        for mode in modes:
            m.set_gemm_dtype(mode)
            for tail in (True, False):
                N.set_pooled_tail(tail)
                k = f"{tag}/{mode}/tail{int(tail)}"
                towers(k, calls)
            N.set_pooled_tail(True)
            T.PARTS = 2                             # the backward as (layers .. a, a .. 0)
            towers(f"{tag}/{mode}/parts2", calls[:2])
            T.PARTS = 3
            if mode == "bf16" and switches:
                N.set_grad_stream16(0)
                towers(f"{tag}/bf16/stream16_off", calls[:2])
                N.set_grad_stream16(-1)
                os.environ["CMH_WGRAD_MULTI"] = "0"
                towers(f"{tag}/bf16/wgrad_multi_off", calls[:2])
                del os.environ["CMH_WGRAD_MULTI"]
            if not full:
                continue
            tok = T.VitTrainTokens.apply(m, img, *vp)
            keep(f"{tag}/{mode}/vit_forward_train_tokens", tok)
            tok.backward(torch.randn(tok.shape, device=dev, generator=gen))
            grads_of(f"{tag}/{mode}/vit_backward_tokens", vp)
            for packed in (False, True):
                m.padded_tokens_unused = packed
                tok, rows = T.TextTrainTokens.apply(m, txt, kpm.to(torch.uint8).contiguous(), *tp)
                k = f"{tag}/{mode}/text_forward_train_tokens{'_packed' if packed else ''}"
                keep(k, tok), keep(f"{k}/eot", rows)
                tok.backward(torch.randn(tok.shape, device=dev, generator=gen) * (~kpm).reshape(-1, 1))
                grads_of(f"{k}/backward", tp)
            m.padded_tokens_unused = False
            blocks, held = m.transformer.resblocks[:2], []
            dt = N.BF16 if mode == "bf16" else N.F32
            arr, bp = _fill_blocks(blocks, dt, held), mith_train_ops.blocks_params(blocks)
            d = blocks[0].ln_1.weight.shape[0]
            x = torch.randn(32 * 8, d, device=dev, generator=gen).requires_grad_()
            y = mith_train_ops.BlocksTrain.apply(x, 32, 8, dt, arr, held, *bp)
            keep(f"{tag}/{mode}/blocks_forward_train", y)
            y.backward(torch.randn(y.shape, device=dev, generator=gen))
            keep(f"{tag}/{mode}/blocks_backward/dx", x.grad)
            grads_of(f"{tag}/{mode}/blocks_backward", bp)

    def mith(tag, B=6, L=16, steps=3):
        """MITH at tiny shapes (token-returning trunk + HashingModel): the forward in both modes, then `steps` BertAdam steps on a
        fixed cotangent, with the loss and the codes of every step.  The token embedding stays out of the optimiser: its gradient
        is a float atomicAdd scatter, and a step on it would make every later array irreproducible."""
        from types import SimpleNamespace
        from model.MITH import HashingModel, build_model
        from model.base.optimization import BertAdam
        cfg = dict(recipe.CLIP_TINY, embed_dim=512)
        args = SimpleNamespace(output_dim=16, dropout=0.0, transformer_layers=2, activation="gelu", top_k_label=8, res_mlp_layers=2)
        img, txt, kpm = inputs(cfg, B, L, 6)
        for mode in ("f32", "bf16"):
            torch.manual_seed(6)
            clip = build_model({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, 6).items()}).to(dev).float()
            clip.set_gemm_dtype(mode).padded_tokens_unused = True
            clip.token_embedding.weight.requires_grad_(False)
            hm = HashingModel(clip_embed_dim=512, args=args).to(dev).set_gemm_dtype(mode)

            def forward():
                (it, _, ic), (tt, _, nk, te) = clip.encode_image(img), clip.encode_text(txt, kpm)
                return sorted(hm(it, tt, ic, te, nk).items())
            with torch.no_grad():
                for name, v in forward():
                    keep(f"{tag}/{mode}/forward/{name}", v)
            params = [p for p in list(clip.parameters()) + list(hm.parameters()) if p.requires_grad and p is not clip.logit_scale]
            opt = BertAdam(params, lr=1e-3, warmup=0.1, t_total=10 * steps)
            gen = torch.Generator(dev).manual_seed(8)
            for step in range(steps):
                out = forward()
                loss = sum((v * torch.randn(v.shape, device=dev, generator=gen)).sum() for _, v in out)
                opt.zero_grad()
                loss.backward()
                opt.step()
                keep(f"{tag}/{mode}/train/step{step}/loss", loss)
                for name, v in out:
                    if name.endswith("_hash"):
                        keep(f"{tag}/{mode}/train/step{step}/{name}", v)
            with torch.no_grad():                                  # the weights the steps left, through the inference path
                for name, v in forward():
                    keep(f"{tag}/{mode}/after/{name}", v)

    def towers():
        cfg = recipe.CLIP_VITB32
        m = model(cfg, 1)
        img, txt, kpm = inputs(cfg, 32, 77, 1)
        inference("vitb32", m, img, txt, kpm, ("f32", "bf16", "fp8"), True)
        training("vitb32", m, img, txt, kpm, ("f32", "bf16"), True, switches=True)
        del m
        m = model(VITL14_CUT, 2)
        img, txt, kpm = inputs(VITL14_CUT, 8, 77, 2)
        inference("vitl14", m, img, txt, kpm, ("f32", "bf16"), False)
        training("vitl14", m, img, txt, kpm, ("bf16",), False)
        del m
        m = model(MIXED, 3)
        img, txt, kpm = inputs(MIXED, 16, 77, 3)
        inference("mixed", m, img, txt, kpm, ("bf16",), False)
        del m
        cfg = recipe.CLIP_TINY
        m = model(cfg, 4)
        img, txt, kpm = inputs(cfg, 32, 16, 4)
        inference("tiny", m, img, txt, kpm, ("f32", "bf16"), True)
        training("tiny", m, img, txt, kpm, ("f32", "bf16"), True, switches=True)

    try:
        if legs in ("all", "towers"):
            towers()
        if legs in ("all", "mith"):
            mith("mith")
    finally:
        N.set_pooled_tail(True)
        N.set_grad_stream16(-1)
        T.PARTS = 3
        os.environ.pop("CMH_WGRAD_MULTI", None)
    with open(out_path, "w") as f:
        json.dump({"lib": N.LIB_PATH, "outputs": digests}, f, indent=0)
    print(f"{len(digests)} outputs of {N.LIB_PATH} -> {out_path}")


def compare(pa, pb, pa2=None):
    a, b = json.load(open(pa)), json.load(open(pb))
    print(f"A = {a['lib']}\nB = {b['lib']}")
    keys = sorted(set(a["outputs"]) | set(b["outputs"]))
    bad = {k for k in keys if a["outputs"].get(k) != b["outputs"].get(k)}
    # control: arrays that differ between TWO runs of library A itself (float atomicAdd: the token embedding's gradient scatter)
    loose = {k for k in keys if a["outputs"].get(k) != json.load(open(pa2))["outputs"].get(k)} if pa2 else set()
    entry = {}
    for k in keys:      # an entry point = the key up to the array's own name
        entry.setdefault(k.split("/grad")[0], []).append(k)
    for e, ks in entry.items():
        word = "DIFFERENT" if any(k in bad - loose for k in ks) else "identical"
        n_loose = sum(k in loose for k in ks)
        print(f"{word}  {e}  ({len(ks)} arrays" + (f", {n_loose} not reproducible by A itself" if n_loose else "") + ")")
    print(f"{len(keys)} arrays, {len(entry)} entry-point calls: {len(bad - loose)} reproducible arrays differ; "
          f"{len(loose)} arrays differ between two runs of A ({sorted({k.rsplit('/', 1)[1] for k in loose})}), {len(bad & loose)} of them between A and B")
    return 1 if bad - loose else 0


def launch_lists(trace_dir):
    streams = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            s = (r.get("Process_Id", ""), r.get("Stream_Id") or r.get("Queue_Id", ""))
            streams.setdefault(s, []).append((int(r["Start_Timestamp"]), r["Kernel_Name"],
                                              [int(r[f"Grid_Size_{c}"]) for c in "XYZ"], [int(r[f"Workgroup_Size_{c}"]) for c in "XYZ"]))
    lists = [[[n, g, w] for _, n, g, w in sorted(v)] for v in streams.values()]
    return sorted(lists, key=lambda l: (-len(l), json.dumps(l)))


def launches(dirs):
    got = [launch_lists(d) for d in dirs]
    for d, lists in zip(dirs, got):
        print(f"{d}: {[len(l) for l in lists]} launches per stream, sha256 {hashlib.sha256(json.dumps(lists).encode()).hexdigest()}")
    if len(got) == 2 and got[0] != got[1]:
        for la, lb in zip(*got):
            for i, (x, y) in enumerate(zip(la, lb)):
                if x != y:
                    print(f"first difference at launch {i}:\n  {x}\n  {y}")
                    return 1
        print("the lists differ in length")
        return 1
    return 0


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run":
        run(*sys.argv[2:4])
    elif cmd == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    elif cmd == "launches":
        sys.exit(launches(sys.argv[2:]))
    else:
        sys.exit(__doc__)
