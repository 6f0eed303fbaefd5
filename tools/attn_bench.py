"""Attention micro-benchmark at the encoder's shapes (cmh_attention / cmh_attention_pair, bf16): us per call and effective HBM rate.
The text shape runs dense here (256 x 77 rows); the encoder's packed captions move about 60 % of its bytes."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))
import torch, cmh_native as N
dev = torch.device("cuda:0")
SHAPES = {"vision": (256, 50, 768, 0), "text": (256, 77, 512, 1)}


def timed(call, reps=100):
    for _ in range(20): call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def report(name, what, us, mb):
    print(f"{name:7s} {what}: {us:7.2f} us  {mb / us * 1e6 / 1e6:6.2f} TB/s ({mb:.0f} MB)", flush=True)


qkvs, mbs = {}, {}
for name, (B, T, d, causal) in SHAPES.items():
    qkvs[name] = torch.randn(B * T, 3 * d, device=dev).bfloat16()
    mbs[name] = B * T * d * 2 * 4 / 1e6
    report(name, f"B={B} T={T} d={d}", timed(lambda: N.attention(qkvs[name], B, T, causal)), mbs[name])
(Bv, Tv, dv, cv), (Bt, Tt, dt_, ct) = SHAPES["vision"], SHAPES["text"]
both = lambda: (N.attention(qkvs["vision"], Bv, Tv, cv), N.attention(qkvs["text"], Bt, Tt, ct))
report("singly", "vision, then text (two launches)", timed(both), mbs["vision"] + mbs["text"])
outs = (torch.empty(Bv * Tv, dv, dtype=torch.bfloat16, device=dev), torch.empty(Bt * Tt, dt_, dtype=torch.bfloat16, device=dev))
pair = lambda: N.attention_pair(qkvs["vision"], Bv, Tv, cv, qkvs["text"], Bt, Tt, ct, out=outs)
if pair() is None:
    print("pair    the library has no pair kernel for these shapes (or CMH_PAIR_KERNELS=0)", flush=True)
else:
    report("pair", "vision + text (one launch)", timed(pair), mbs["vision"] + mbs["text"])
    assert all(torch.equal(a, b) for a, b in zip(outs, both())), "the pair launch's bits differ from the single launches'"
