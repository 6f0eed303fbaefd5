"""A training tape filled by one build of the library, read by another: the check that a change of csrc/encoders_bwd.hip moved no slot.

    CMH_LIB=<library A> python tools/tape_across_libs.py fill DIR    A's cmh_vit_forward_train / cmh_text_forward_train -> DIR/*.npy
    python tools/tape_across_libs.py back DIR                        B's backward on A's tapes against B's backward on its own:
                                                                     every gradient byte for byte; exit status 1 on any difference

The `tiny` config at batch 32 (tapes of a few MB), f32 and bf16.  The token embedding's gradient (a float atomicAdd scatter) is
compared too but only reported: two runs of one library do not reproduce it either."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def main(cmd, d):
    import numpy as np
    import torch
    import cmh_native as N
    import recipe
    from model.base import train_ops as T
    from model.base.model import CLIP

    dev, cfg, B, L = torch.device("cuda:0"), recipe.CLIP_TINY, 32, 16
    torch.manual_seed(4)
    m = CLIP(**cfg).to(dev).float()
    img = torch.from_numpy(recipe.images(B, cfg["image_resolution"], 4)).to(dev)
    txt = torch.from_numpy(recipe.captions(B, L, cfg["vocab_size"], 4)).to(dev)
    lib, st, bad = N.lib(), N.stream_ptr(dev), 0
    os.makedirs(d, exist_ok=True)
    for mode in ("f32", "bf16"):
        m.set_gemm_dtype(mode)
        vs, ts = m._vit_struct(), m._text_struct()
        towers = {      # name: (tape bytes, parameters, head parameters, gradient struct, forward(feat, tape), backward(dfeat, grads, tape))
            "vit": (lib.cmh_vit_train_bytes(C.byref(vs), B), T.vit_params(m.visual), 8, N.VitGrads,
                    lambda f, t: lib.cmh_vit_forward_train(C.byref(vs), N.ptr(img), B, N.ptr(f), N.ptr(t), t.numel(), st),
                    lambda df, g, t: lib.cmh_vit_backward(C.byref(vs), B, N.ptr(df), C.byref(g), N.ptr(t), t.numel(), st)),
            "text": (lib.cmh_text_train_bytes(C.byref(ts), B, L), T.text_params(m), 5, N.TextGrads,
                     lambda f, t: lib.cmh_text_forward_train(C.byref(ts), N.ptr(txt), B, L, None, N.ptr(f), N.ptr(t), t.numel(), st),
                     lambda df, g, t: lib.cmh_text_backward(C.byref(ts), N.ptr(txt), B, L, None, N.ptr(df), C.byref(g), N.ptr(t), t.numel(), st))}
        for name, (nbytes, params, nhead, struct, forward, backward) in towers.items():
            path = os.path.join(d, f"{name}_{mode}_tape.npy")
            own, feat = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(B, cfg["embed_dim"], device=dev)
            N.check(forward(feat, own), f"{name} forward")
            if cmd == "fill":
                np.save(path, own.cpu().numpy())
                print(f"{N.LIB_PATH}: {name} {mode} tape of {nbytes} bytes -> {path}")
                continue
            dfeat = torch.randn(feat.shape, device=dev, generator=torch.Generator(dev).manual_seed(5))
            flats = []
            for tape in (own, torch.from_numpy(np.load(path)).to(dev)):
                assert tape.numel() == nbytes, (tape.numel(), nbytes)
                grads, flat, _blocks, g = T._grad_call(params, nhead, struct)
                N.check(backward(dfeat, g, tape), f"{name} backward")
                flats.append([x.clone() for x in grads])
            diff = [i for i, (a, b) in enumerate(zip(*flats)) if not torch.equal(a, b)]
            loose = [i for i in diff if name == "text" and i == 0]       # token_embedding
            bad += len(diff) - len(loose)
            print(f"{name} {mode}: {len(flats[0])} gradients, {len(diff) - len(loose)} differ between the other library's tape and this one's"
                  + (f" (+ the token embedding's, max |d| {float((flats[0][0] - flats[1][0]).abs().max()):.3g})" if loose else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]) if len(sys.argv) == 3 and sys.argv[1] in ("fill", "back") else __doc__)
