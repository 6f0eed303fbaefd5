"""Case tables, the fp64 reference and the checks of the attention edge tests (tests/test_attention_cases_host.py on the CPU,
tests/test_gpu_attention_edges.py on the GPU).  Pure torch: importable without a GPU, and every function runs on whatever device its
operands are on.

The lengths sit on the tile edges of the fifteen kernel forms that csrc/attention.hip and csrc/attention_bwd.hip compile and that
launch_attention_varlen / launch_attention_backward pick by T and dtype alone; `forward_form` / `backward_form` restate that choice.
Masks are deterministic functions of (batch row, T); True = the key is masked, as in nn.MultiheadAttention's key_padding_mask.
A query row whose keys are all masked is outside the kernels' contract (the reference gives NaN, the kernels 0 / 0, inf or P = 0):
no case contains one, which tests/test_attention_cases_host.py asserts."""
import torch

EDGE_T = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 95, 96, 97, 112, 127, 128, 129, 160]
MODES = ("f32", "bf16")
VARIANTS = ("none", "tail", "holes", "tile", "lead")
CAUSAL_OK = ("none", "tail", "holes", "tile")          # these keep key 0 visible; `lead` hides it and is never combined with causal
MAIN_SHAPE = (3, 128)                                  # B, d (2 heads)
EXTRA_SHAPES = ((2, 192), (5, 64))                     # 3 heads / 1 head: (batch, head) index arithmetic and kpm[b * Tmax + key]
EXTRA_T = (33, 97, 129)
GUARD_T = (17, 33, 97, 129)
GUARD_ROWS = 64

FORWARD_FORMS = tuple(f"attention_mfma_kernel<{n}>" for n in (2, 4, 6, 8)) + ("attention_kernel<float>", "attention_kernel<bf16_t>")
BACKWARD_FORMS = tuple(f"attention_bwd_mfma_kernel<{n}>" for n in range(1, 7)) + (
    "attention_bwd_kernel<bf16_t>", "attention_bwd_kernel<float>", "attention_bwd_tiled_kernel<float>", "attention_bwd_tiled_kernel<bf16_t>")


def forward_form(T, mode):
    if mode == "f32":
        return "attention_kernel<float>"
    if T > 128:
        return "attention_kernel<bf16_t>"
    return f"attention_mfma_kernel<{2 if T <= 32 else 4 if T <= 64 else 6 if T <= 96 else 8}>"


def backward_form(T, mode):
    if T > 128:
        return f"attention_bwd_tiled_kernel<{'float' if mode == 'f32' else 'bf16_t'}>"
    if mode == "f32":
        return "attention_bwd_kernel<float>"
    return f"attention_bwd_mfma_kernel<{(T + 15) // 16}>" if T <= 96 else "attention_bwd_kernel<bf16_t>"


def backward_reads_o(T, mode):
    """whether the form takes D = rowsum(dO o O) from the forward's o (else from its own P and dP, i.e. O = P V)"""
    return backward_form(T, mode).startswith("attention_bwd_kernel")


def shapes(T):
    return (MAIN_SHAPE,) + (EXTRA_SHAPES if T in EXTRA_T else ())


def variants(T, causal):
    out = []
    for v in (CAUSAL_OK if causal else VARIANTS):
        if (v == "tile" and T <= 16) or (v == "lead" and T < 2):
            continue
        out.append(v)
    return out


def cases(T):
    """every (B, d, causal, variant) the tests run at length T"""
    return [(B, d, causal, v) for B, d in shapes(T) for causal in (0, 1) for v in variants(T, causal)]


def key_mask(variant, B, T):
    """bool [B, T], True = masked; None for `none`.  Batch rows differ on purpose; rows beyond 3 cycle through the three patterns."""
    if variant == "none":
        return None
    key = torch.arange(T)
    m = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        i = b % 3
        if variant == "tail":
            m[b] = key >= (1, T, (T + 1) // 2)[i]
        elif variant == "holes":
            m[b] = key % 3 == 1
        elif variant == "tile":
            lo, hi = ((16, min(32, T)), (32, min(64, T)), (16, min(96, T)))[i]
            m[b] = (key >= lo) & (key < hi)                      # (b = 1 at T <= 32: lo >= hi, nothing masked)
        elif variant == "lead":
            m[b] = key < (min(16, T - 1), min(32, T - 1), T - 1)[i]      # i = 2: only the last key is visible
        else:
            raise KeyError(variant)
    return m


def visible(B, T, causal, mask, device="cpu"):
    """bool [B, T(query), T(key)]: the keys a query attends to"""
    vis = torch.ones(B, T, T, dtype=torch.bool, device=device)
    if causal:
        vis &= torch.ones(T, T, dtype=torch.bool, device=device).tril()
    if mask is not None:
        vis &= ~mask.to(device)[:, None, :]
    return vis


def heads_of(x, B, T, n):
    """[B*T, n*d] -> n tensors [B, H, T, 64] in float64"""
    H = x.shape[1] // n // 64
    return x.double().view(B, T, n, H, 64).permute(2, 0, 3, 1, 4)


def rows_of(x, B, T):
    """[B, H, T, 64] -> [B*T, H*64]"""
    return x.permute(0, 2, 1, 3).reshape(B * T, -1)


def reference_forward(qkv, B, T, vis):
    """fp64 statement of the op on the operands as given (round them first for the bf16 mode) -> o [B*T, d], P [B, H, T, T]"""
    q, k, v = heads_of(qkv, B, T, 3)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    return rows_of(p @ v, B, T), p


def reference_backward(qkv, dout, p, B, T, o_for_d=None):
    """dqkv [B*T, 3d] in fp64: dV = P^T dO, dS = P o (dO V^T - D) / 8, dQ = dS K, dK = dS^T Q with D = rowsum(dO o O); O is `o_for_d`
    ([B*T, d], what a kernel that reads the forward's output sees) or the exact P V"""
    q, k, v = heads_of(qkv, B, T, 3)
    do = heads_of(dout, B, T, 1)[0]
    dp = do @ v.transpose(-1, -2)
    # (O = P V: D = rowsum(P o dP), the same number, and exactly dP where a query has one visible key - dS = 0 there as in the kernels)
    dsum = (p * dp).sum(-1, keepdim=True) if o_for_d is None else (do * heads_of(o_for_d, B, T, 1)[0]).sum(-1, keepdim=True)
    ds = p * (dp - dsum) / 8.0
    return torch.stack((ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do)).permute(1, 3, 0, 2, 4).reshape(B * T, -1)


def random_inputs(B, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, 3 * d, generator=g), torch.randn(B * T, d, generator=g)


def slice_errors(got, ref, d, skip_below=0.0):
    """per d-wide column slice (Q / K / V of dqkv, the one slice of o): (error max / slice max, error 2-norm / slice 2-norm), worst of each;
    a slice whose reference is exactly zero has to be exactly zero (else: inf).  `skip_below`: slices whose reference max is below it
    are left out (f32 figures only: a case whose queries all have one visible key leaves the cancellation residue of dO . o there)"""
    worst = [0.0, 0.0]
    for i in range(ref.shape[1] // d):
        r, e = ref[:, i * d:(i + 1) * d], got[:, i * d:(i + 1) * d] - ref[:, i * d:(i + 1) * d]
        if 0.0 < float(r.abs().max()) < skip_below:
            continue
        if float(r.abs().max()) == 0.0:
            emax = enorm = 0.0 if float(e.abs().max()) == 0.0 else float("inf")
        else:
            emax, enorm = float(e.abs().max() / r.abs().max()), float(e.norm() / r.norm())
        worst = [max(worst[0], emax), max(worst[1], enorm)]
    return worst


# ---- visible-set decode ---------------------------------------------------------------------------------------------------------
# Q = 0 makes every score 0, so every visible key weighs exactly 1 / nvis; V[key, c] = 2^(key // 64) for c = key % 64 (else 0) makes
# round(o[q, c] * nvis(q)) the bit mask of the visible keys = c (mod 64): at T <= 160 three bits, values <= 7.  What is left of
# rounding is 1 / l and the bf16 output (2^-8 relative at worst): 7 * 2^-8 < 0.03 against the decision threshold 0.5.
def decode_values(T):
    key = torch.arange(T)
    v = torch.zeros(T, 64, dtype=torch.float64)
    v[key, key % 64] = 2.0 ** (key // 64).double()
    return v


def decode_inputs(B, T, d, seed):
    """qkv [B*T, 3d] f32: Q = 0, K random (different per head), V the code above (the same for every head); exact in bf16 but for K"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(B, T, 3, d // 64, 64)
    qkv[:, :, 1] = torch.randn(B, T, d // 64, 64, generator=g)
    qkv[:, :, 2] = decode_values(T).float()[None, :, None, :]
    return qkv.reshape(B * T, 3 * d)


def decode_check(o, B, T, vis, what=""):
    """o [B*T, d] (any float dtype / device) must decode to exactly the visible sets `vis` [B, T, T], for every (batch, head, query)"""
    o = o.detach().double().cpu().view(B, T, -1, 64)
    vis = vis.cpu()
    assert bool(torch.isfinite(o).all()), (what, "non-finite output")
    nvis = vis.sum(-1)
    assert int(nvis.min()) >= 1, (what, "a query without a visible key is outside the contract")
    got = torch.round(o * nvis[:, :, None, None].double())
    want = (vis.double() @ decode_values(T))[:, :, None, :]                # [B, T, 1, 64] bit masks
    bad = (got != want).nonzero()
    if len(bad):
        b, q, h, c = (int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} decoded words differ; first at batch {b} query {q} head {h} column {c}: keys "
                             f"{[c + 64 * i for i in range(3) if int(got[b, q, h, c]) >> i & 1]} (mod-64 class {c}) visible, expected "
                             f"{[c + 64 * i for i in range(3) if int(want[b, q, 0, c]) >> i & 1]}")
    return float((o * nvis[:, :, None, None].double() - got).abs().max())


# ---- deliberate defects of the visible set (tests/test_attention_cases_host.py: the decode check must notice each) ---------------
def defect_drop_one_key(B, T, causal, mask):
    vis = visible(B, T, causal, mask)
    b, q = (int(i) for i in (vis.sum(-1) > 1).nonzero()[-1])              # the last query that can spare a key
    vis[b, q, int(vis[b, q].nonzero()[-1])] = False
    return vis


def defect_causal_off_by_one(B, T, causal, mask):
    assert causal
    vis = visible(B, T, 0, mask)
    return vis & torch.ones(T, T, dtype=torch.bool).tril(-1)              # key < query


def defect_next_rows_mask(B, T, causal, mask):
    return visible(B, T, causal, mask.roll(-1, 0))                        # batch row b reads row b + 1's mask


def defect_short_sequence(B, T, causal, mask):
    vis = visible(B, T, causal, mask)
    vis[:, :, T - 1] = False                                              # Tn replaced by T - 1: the last key is never read
    return vis


DEFECTS = {"drop_one_key": defect_drop_one_key, "causal_off_by_one": defect_causal_off_by_one,
           "next_rows_mask": defect_next_rows_mask, "short_sequence": defect_short_sequence}


# ---- packed rows: a small text tower whose seq_off runs through every form ------------------------------------------------------
PACK_L = (33, 64, 65, 97, 128, 129, 160)
PACK_TRAIN_L = (33, 65, 97, 129)
PACK_B = 6


def pack_cfg():
    import mithutil as mu
    return dict(mu.CLIP_TINY512, context_length=160, transformer_width=256, transformer_heads=4)      # width 256: device-side row count


def pack_captions(L, vocab, seed=7):
    """ragged captions of test_gpu_mith._ragged_text (EOT anywhere, zeros behind, one inner zero in the longest caption), with caption 1
    forced to 3 tokens and caption 2 to full length without any padding"""
    import numpy as np
    from test_gpu_mith import _ragged_text
    text = _ragged_text(PACK_B, L, vocab, seed)
    text[1] = 0
    text[1, :3] = (vocab - 2, 17, vocab - 1)
    text[2] = np.arange(L) % (vocab - 3) + 1
    text[2, 0], text[2, L - 1] = vocab - 2, vocab - 1
    return text
