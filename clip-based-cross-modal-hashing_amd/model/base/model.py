"""CLIP ViT trunk with the reference's module tree and state_dict, executed by libcmh.so.

Mirror of the reference's model/base/model.py (ViT path only; the ModifiedResNet path is not
reachable with a ViT-B/32 checkpoint):
  LayerNorm / QuickGELU            model/base/model.py:153-164
  ResidualAttentionBlock           :167-196
  Transformer                      :199-207
  VisionTransformer                :210-252
  CLIP (encode_image/encode_text)  :255-372
  convert_weights / build_model    :391-455
The nn.Modules here are parameter containers with the SAME names and shapes (302 tensors for
ViT-B/32, so OpenAI `ViT-B-32.pt` and reference `model-N.pth` checkpoints load strict); `forward`
never touches ATen math: encode_image / encode_text call cmh_vit_encode / cmh_text_encode.

Arithmetic mode (`CLIP.set_gemm_dtype`): "f32" = exact fp32 MFMA, the parity mode for the
reference's `model.float()` trainers; "bf16" = bf16 MFMA operands with fp32 accumulation,
LayerNorm/softmax/residual in fp32 (the throughput mode, BASELINE.json configs[1]).
Training: when gradients are enabled and a tower parameter asks for them, encode_image / encode_text run
the tape-keeping forward and the native backward (model/base/train_ops.py, which also holds the tables of
which parameter goes to which struct field).  Outputs of the inference-only calls carry a grad_fn that
raises, so `loss.backward()` fails loudly instead of silently training nothing.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch
from torch import nn

import cmh_native as N
from model.base import train_ops as T


class LayerNorm(nn.LayerNorm):
    """Parameter container; statistics are always fp32 inside the HIP kernel."""


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x): fused into the c_fc GEMM epilogue."""


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int, attn_mask=None):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", nn.Linear(d_model, d_model * 4)),
            ("gelu", QuickGELU()),
            ("c_proj", nn.Linear(d_model * 4, d_model)),
        ]))
        self.ln_2 = LayerNorm(d_model)
        self.attn_mask = attn_mask


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, attn_mask=None):
        super().__init__()
        self.width = width
        self.layers = layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask) for _ in range(layers)])


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution = input_resolution
        self.output_dim = output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))


class _NoBackward(torch.autograd.Function):
    """Attaches a grad_fn to outputs of the inference-only entry points so that a backward pass through them fails loudly
    instead of silently stopping (the training entry points keep a tape and are used whenever gradients are wanted)."""

    @staticmethod
    def forward(ctx, out, anchor):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError(
            "this output came from an inference-only call (per-block taps, `assume_frozen`, or an operand that did not ask for "
            "gradients when it was produced): it carries no tape, so nothing can be propagated through it")


def no_backward(out: torch.Tensor, anchor: torch.Tensor) -> torch.Tensor:
    if torch.is_grad_enabled() and anchor.requires_grad:
        return _NoBackward.apply(out, anchor)
    return out


class _TowerCache:
    """Device-resident weights in the layout libcmh wants + the ctypes structs that point at them.  A new entry is made when any
    parameter changed (data_ptr/_version) or the arithmetic mode changed; a training tape keeps the entry it ran with."""

    def __init__(self, key=None, struct=None, blocks=None, keep=()):
        self.key, self.struct, self.blocks = key, struct, blocks
        self.keep = keep        # tensors that must outlive the structs


def _prep(p: torch.Tensor, keep: list) -> torch.Tensor:
    t = p.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    keep.append(t)
    return t


def _gemm_w(p: torch.Tensor, dt: int, keep: list, transpose: bool = False) -> torch.Tensor:
    if dt in (N.BF16, N.FP8) and not transpose and p.dtype == torch.float32 and p.is_contiguous():
        # the bf16 copy lives on the parameter: the fused BertAdam step rewrites it together with the f32 values (cmh_adam_tensor.
        # p_bf16) and stamps the version it is current for, so a training step pays no cast pass over the weights
        t = getattr(p, "_cmh_bf16", None)
        if N.bf16_copy_of(p) is None or getattr(p, "_cmh_bf16_version", None) != (p.data_ptr(), p._version):
            t = N.cast_bf16(p.detach().reshape(p.shape[0], -1))
            p._cmh_bf16, p._cmh_bf16_version = t, (p.data_ptr(), p._version)
        keep.append(t)
        return t
    t = p.detach().float()
    t = t.t().contiguous() if transpose else t.contiguous()
    t = t.reshape(t.shape[0], -1)
    if dt in (N.BF16, N.FP8):       # outside the blocks the fp8 mode is the bf16 mode (conv1, the final projections)
        t = N.cast_bf16(t)
    keep.append(t)
    return t


def _fp8_w(p: torch.Tensor, keep: list):
    """Linear weight [out, in] -> (e4m3 bytes, per-output-channel scales): the tensors convert_weights lowers upstream."""
    q, cs = N.fp8_quantize_weight(p.detach().float().contiguous())
    keep.extend((q, cs))
    return q.data_ptr(), cs.data_ptr()


FP8_HEADROOM = 2.0     # act_scale = FP8_HEADROOM * amax(calibration batch) / 448: later batches may exceed the calibration maximum


def _fill_blocks(resblocks, dt: int, keep: list, act_amax=None):
    """cmh_block_weights array from train_ops.BLOCK_TABLE.  The fp8 mode differs only in how the four GEMM weights are lowered (e4m3
    bytes + per-channel scales in the `*_cs` field next to each `*_w`) and in the activation scales."""
    if dt == N.FP8 and act_amax is None and len(resblocks):
        raise N.NativeError("fp8 mode needs activation scales: call clip.calibrate_fp8(images, texts) first")
    arr = (N.BlockWeights * len(resblocks))()
    for i, blk in enumerate(resblocks):
        b = arr[i]
        for field, get, is_gemm in T.BLOCK_TABLE:
            if is_gemm and dt == N.FP8:
                w, cs = _fp8_w(get(blk), keep)
                setattr(b, field, w), setattr(b, field[:-1] + "cs", cs)
            else:
                setattr(b, field, (_gemm_w(get(blk), dt, keep) if is_gemm else _prep(get(blk), keep)).data_ptr())
        if dt == N.FP8:
            for j in range(4):
                b.act_scale[j] = max(float(act_amax[i][j]), 1e-6) * FP8_HEADROOM / 448.0
    return arr


# one tower's share of an inference call (CLIP._open): struct, operand (`more`: the further image batches of a two-batch call),
# (B,) / (B, L), result buffer, scratch, the packed row count's device word or None, stream
_Call = namedtuple("_Call", "tower s x more dims out ws rows stream")

FP8_MAX_IMAGE_TOKENS = 128  # the fp8 mode's e4m3-output attention (csrc/attention.hip) is built for T <= 128 (ViT-B/32: 50)

_DT = {"f32": N.F32, "fp32": N.F32, "float32": N.F32, "bf16": N.BF16, "bfloat16": N.BF16, "fp8": N.FP8, "e4m3": N.FP8}


class CLIP(nn.Module):
    def __init__(self, embed_dim: int, image_resolution: int, vision_layers, vision_width: int,
                 vision_patch_size: int, context_length: int, vocab_size: int, transformer_width: int,
                 transformer_heads: int, transformer_layers: int):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet (RN50) visual towers are out of scope; ViT checkpoints only")
        self.context_length = context_length
        self.vision_heads = vision_width // 64
        self.visual = VisionTransformer(input_resolution=image_resolution, patch_size=vision_patch_size,
                                        width=vision_width, layers=vision_layers, heads=self.vision_heads,
                                        output_dim=embed_dim)
        self.transformer = Transformer(width=transformer_width, layers=transformer_layers, heads=transformer_heads,
                                       attn_mask=self.build_attention_mask)
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.initialize_parameters()
        self._gemm_dtype = _DT[os.environ.get("CMH_GEMM_DTYPE", "f32").lower()]
        self._check_fp8_tokens(self._gemm_dtype)
        self._tower_cache = {"vit": _TowerCache(), "text": _TowerCache()}
        self.assume_frozen = False     # True: skip the per-call parameter-version scan (pure inference)
        self._fp8_amax = {"vit": None, "text": None}     # [layers, 4] calibration maxima of the four GEMM inputs per block
        self._fp8_amax_key = {"vit": None, "text": None}  # the parameter versions those maxima were measured with

    # -- reference API ---------------------------------------------------------------------------
    def initialize_parameters(self):
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        for tr in (self.transformer,):
            proj_std = (tr.width ** -0.5) * ((2 * tr.layers) ** -0.5)
            attn_std = tr.width ** -0.5
            fc_std = (2 * tr.width) ** -0.5
            for block in tr.resblocks:
                nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
                nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
                nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
                nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    def build_attention_mask(self, context_length):
        """Kept for API parity; the kernel applies the causal mask itself."""
        mask = torch.empty(context_length, context_length)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask.to(self.device)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    @property
    def device(self):
        return self.visual.conv1.weight.device

    def set_gemm_dtype(self, name: str):
        """"f32" (parity mode), "bf16" (throughput mode) or "fp8" (BASELINE configs[4]: the blocks' four GEMMs on e4m3 operands;
        inference only; activation scales come from `calibrate_fp8`, run on the first batch if it was not called)."""
        dt = _DT[name.lower()]
        self._check_fp8_tokens(dt)
        self._gemm_dtype = dt
        return self

    def _check_fp8_tokens(self, dt):
        tokens = self.visual.positional_embedding.shape[0]
        p = self.visual.conv1.weight.shape[-1]
        if dt == N.FP8 and (p % 4 or 3 * p * p % 64):
            raise N.NativeError(f"the fp8 mode is not built for patch {p}: its conv1 (K = 3*{p}^2 = {3 * p * p}) needs the K-padded "
                                "patch matrix, built for the f32 and bf16 modes only: use set_gemm_dtype('bf16' | 'f32')")
        if dt == N.FP8 and tokens > FP8_MAX_IMAGE_TOKENS:
            raise N.NativeError(f"the fp8 mode is built for at most {FP8_MAX_IMAGE_TOKENS} image tokens; this checkpoint has {tokens} "
                                "(ViT-B/16 and larger): use set_gemm_dtype('bf16' | 'f32')")

    def calibrate_fp8(self, image=None, text=None, reset=True, _versions=None):
        """Calibration pass of the fp8 mode: runs the batch(es) in bf16 mode and records, per block, the largest magnitude of the
        four GEMM inputs (ln_1 output, attention output, ln_2 output, QuickGELU(c_fc) output).  The per-tensor quantisation
        scales are FP8_HEADROOM * amax / 448.  Call again with reset=False to widen the maxima with more batches.
        Returns the bf16-mode features of the batches it was given.  (_versions: the scans an entry point that calibrates on its
        first batch has made already.)"""
        mode, self._gemm_dtype = self._gemm_dtype, N.BF16
        out = []
        try:
            with torch.no_grad():
                for tower, x in ((T.VIT, image), (T.TEXT, text)):
                    if x is None:
                        continue
                    name, scan = tower.name, (_versions or {}).get(tower.name)
                    if scan is None or scan == "frozen":
                        scan = self._scan(tower)                 # the maxima belong to these very weights, frozen or not
                    c, = self._open("calibrate_fp8", **{"texts" if tower.text else "images": [x]},
                                    versions={name: "frozen" if self.assume_frozen else scan})
                    amax = torch.zeros(c.s.layers * 4, dtype=torch.float32, device=x.device)
                    if self._fp8_amax[name] is not None and not reset:
                        amax.copy_(torch.as_tensor(self._fp8_amax[name], dtype=torch.float32).reshape(-1))
                    fn = f"cmh_{name}_calibrate_fp8"
                    N.check(getattr(N.lib(), fn)(C.byref(c.s), N.ptr(c.x), *c.dims, N.ptr(c.out), N.ptr(amax), N.ptr(c.ws), c.ws.numel(),
                                                 c.stream), fn)
                    vals = amax.cpu().reshape(c.s.layers, 4)
                    if not bool(torch.isfinite(vals).all()):
                        raise N.NativeError("calibrate_fp8: non-finite activations in the calibration batch")
                    self._fp8_amax[name] = vals.tolist()
                    self._fp8_amax_key[name] = scan[len(tower.head):]          # the blocks' versions
                    self._tower_cache[name].key = None                        # scales changed: rebuild the fp8 structs
                    out.append(c.out)
        finally:
            self._gemm_dtype = mode
        return tuple(out)

    # encode_text skips the padding after each caption's EOT (bit-identical pooled features, cmh_text_encode_packed);
    # CMH_TEXT_PACK=0 or `clip.pack_text = False` computes all context_length positions like the reference
    pack_text = os.environ.get("CMH_TEXT_PACK", "1") != "0"
    _last_text_rows = None

    @property
    def last_text_rows(self):
        """(rows computed, batch * seq_len) of the last packed encode_text, or None; reading it fetches the count from the device
        (the only synchronisation: the encode itself never waits for it)."""
        if self._last_text_rows is None:
            return None
        rows, dense = self._last_text_rows
        return int(rows.item()), dense

    @property
    def gemm_dtype(self) -> str:
        return {N.BF16: "bf16", N.FP8: "fp8"}.get(self._gemm_dtype, "f32")

    def _fp8_scales_current(self, tower, versions):
        """Activation scales belong to the weights they were calibrated with: after load_state_dict or a training step the blocks
        produce other magnitudes, and stale per-tensor scales saturate at +-448 or waste range.  A change of any block parameter
        since the calibration drops the maxima, so that the next fp8 batch calibrates itself (assume_frozen skips the check)."""
        name = tower.name
        if self._fp8_amax[name] is not None and versions != "frozen" and self._fp8_amax_key[name] != versions[len(tower.head):]:
            import warnings
            warnings.warn(f"fp8 mode: the {name} tower's weights changed since calibrate_fp8; re-calibrating on this batch")
            self._fp8_amax[name] = None
        return self._fp8_amax[name] is not None

    # -- native weight structs -------------------------------------------------------------------
    def _scan(self, tower):
        """(data_ptr, _version) of every parameter of a tower (train_ops.VIT / TEXT), in the order of its table: the one walk over
        the parameters that every key is made of.  A public call makes it at most once per tower and hands the result down."""
        return tuple((p.data_ptr(), p._version) for p in tower.params(self))

    def _versions(self, tower):
        return "frozen" if self.assume_frozen else self._scan(tower)      # assume_frozen: no scan at all

    def _key(self, tower, versions=None):
        """what a tower's structs and features depend on besides the input: the arithmetic mode, the device, the weights' versions"""
        return (self._gemm_dtype, str(self.device), self._versions(tower) if versions is None else versions)

    def _tower_entry(self, tower, versions=None):
        key = self._key(tower, versions)
        if self._tower_cache[tower.name].key != key:
            root, keep, dt = tower.root(self), [], self._gemm_dtype
            s = tower.weights(gemm_dtype=dt, layers=len(root.transformer.resblocks), **tower.geometry(root))
            for field, grad_field, get, is_gemm in tower.head:
                t = _gemm_w(get(root), dt, keep, transpose=field != grad_field) if is_gemm else _prep(get(root), keep)
                setattr(s, field, t.data_ptr())
            blocks = _fill_blocks(root.transformer.resblocks, dt, keep, self._fp8_amax[tower.name])
            s.blocks = C.cast(blocks, C.POINTER(N.BlockWeights))
            self._tower_cache[tower.name] = _TowerCache(key, s, blocks, keep)
        return self._tower_cache[tower.name]

    def _tower_struct(self, tower, versions=None):
        return self._tower_entry(tower, versions).struct

    def _vit_struct(self):
        return self._tower_struct(T.VIT)

    def _text_struct(self):
        return self._tower_struct(T.TEXT)

    @staticmethod
    def _taps(tap_list):
        if not tap_list:
            return None, None
        arr = (C.c_void_p * len(tap_list))(*[None if t is None else t.data_ptr() for t in tap_list])
        taps = N.Taps(C.cast(arr, C.POINTER(C.c_void_p)), len(tap_list))
        return taps, arr

    # -- the two hot-path entry points -----------------------------------------------------------
    def _wants_tape(self, *towers):
        """the one tape-or-encode decision: a training forward when gradients are enabled and a tower parameter asks for them"""
        if self.assume_frozen or not torch.is_grad_enabled() or not any(p.requires_grad for t in towers for p in t.params(self)):
            return False
        if self._gemm_dtype == N.FP8:
            raise N.NativeError("the fp8 mode is inference-only: use torch.no_grad() or set_gemm_dtype('bf16' | 'f32') to train")
        return True

    def _operands(self, who, images=(), texts=()):
        """Batches in the kernels' types (f32 / i64, contiguous), on the GPU like the weights, every image batch [n,3,R,R] with n its
        caption batch's where there is one -> (images, texts)"""
        images, texts = [N.f32c(i) for i in images], [t.to(torch.int64).contiguous() for t in texts]
        N.require_gpu(*images, *texts, *([self.visual.proj] if images else []), *([self.text_projection] if texts else []))
        R = self.visual.input_resolution
        for k, im in enumerate(images):
            want = ((texts[k] if texts else im).shape[0], 3, R, R)
            if tuple(im.shape) != want:
                raise N.NativeError(f"{who}: expected images {list(want)}, got {tuple(im.shape)}")
        return images, texts

    def _open(self, who, images=(), texts=(), versions=None, tokens=False, packed=False):
        """What every inference entry point does before its native call, for each tower it has batches for: the operands
        (_operands), fp8 activation scales calibrated on the first batch, the struct under one scan of the parameters (`versions`:
        scans the caller made already), the result buffer ([B, E] pooled, [B*T, E] tokens), the tower's scratch of the current
        stream, the device word that receives a packed text call's row count -> [_Call per tower, image first]"""
        images, texts = self._operands(who, images, texts)
        ops = [(T.VIT, images)] * bool(images) + [(T.TEXT, texts)] * bool(texts)
        given = versions or {}
        ver = {t.name: given[t.name] if t.name in given else self._versions(t) for t, _ in ops}
        if self._gemm_dtype == N.FP8 and not all(self._fp8_scales_current(t, ver[t.name]) for t, _ in ops):
            # the first batch (or the first after a weight change) calibrates the activation scales
            self.calibrate_fp8(image=images[0] if images else None, text=texts[0] if texts else None, _versions=ver)
        dev = (images or texts)[0].device
        stream, calls = N.stream_ptr(dev), []
        for tower, xs in ops:
            s = self._tower_struct(tower, ver[tower.name])
            B = sum(x.shape[0] for x in xs)
            dims = (B, xs[0].shape[1]) if tower.text else (B,)
            per = 1 if not tokens else dims[1] if tower.text else (s.resolution // s.patch) ** 2 + 1
            out = torch.empty(B * per, s.embed_dim, dtype=torch.float32, device=dev)
            need = getattr(N.lib(), f"cmh_{tower.name}_workspace_bytes")(C.byref(s), *dims)
            ws = N.workspace(need, dev, f"{tower.name}@{stream}")         # one scratch per stream: sub-batches may overlap
            rows = torch.empty(1, dtype=torch.int32, device=dev) if packed and tower.text else None    # stays on the device
            x = torch.cat(xs, 0) if tower.text and len(xs) > 1 else xs[0]
            calls.append(_Call(tower, s, x, xs[1:], dims, out, ws, rows, stream))
        return calls

    def _finish(self, *calls):
        """... and after it: a packed call's row count is kept for `last_text_rows`; the features refuse a backward pass"""
        for c in calls:
            if c.rows is not None:
                self._last_text_rows = (c.rows, c.dims[0] * c.dims[1])
        return tuple(no_backward(c.out, c.tower.projection(self)) for c in calls)

    def encode_image(self, image, taps=None):
        """image f32 [B,3,R,R] -> [B, embed_dim] f32  (reference model/base/model.py:356-357,228-252)."""
        if taps is None and self._wants_tape(T.VIT):         # training: tape-keeping forward with a real backward
            (image,), _ = self._operands("encode_image", images=[image])
            return T.VitTrain.apply(self, image, *T.VIT.params(self))
        versions = self._versions(T.VIT)
        hit = self._stashed("image", image, self._key(T.VIT, versions)) if taps is None else None
        if hit is not None:
            return hit
        c, = self._open("encode_image", images=[image], versions={"vit": versions})
        tp, _arr = self._taps(taps)
        N.check(N.lib().cmh_vit_encode(C.byref(c.s), N.ptr(c.x), *c.dims, N.ptr(c.out), N.ptr(c.ws), c.ws.numel(),
                                       None if tp is None else C.byref(tp), c.stream), "cmh_vit_encode")
        return self._finish(c)[0]

    def patch_embed(self, image, image_b=None, keep_patches=False):
        """conv1 alone, as the image tower runs it (cmh_vit_patch_embed): image f32 [B,3,R,R] (+ image_b: the batch as two tensors)
        -> (patch_out f32 [B*g*g, width], the patch matrix [B*g*g, K] in the GEMM dtype or None).  keep_patches=False is the
        inference stem (one fused launch where N.set_conv1_fused allows), True the training forward's two launches."""
        images, _ = self._operands("patch_embed", images=[image] if image_b is None else [image, image_b])
        s = self._tower_struct(T.VIT)
        B, g2, dev = sum(x.shape[0] for x in images), (s.resolution // s.patch) ** 2, images[0].device
        f32 = self._gemm_dtype == N.F32
        e, pk = (4 if f32 else 2), 3 * s.patch * s.patch
        K = pk if s.patch % 4 == 0 and pk % (32 if f32 else 64) == 0 else -(-pk // 256) * 256      # (csrc/cmh_common.h: conv1_k)
        scratch = torch.empty(-(-B * g2 * K * e // 256) * 256 + s.width * K * e + 256, dtype=torch.uint8, device=dev)
        out = torch.empty(B * g2, s.width, dtype=torch.float32, device=dev)
        N.check(N.lib().cmh_vit_patch_embed(C.byref(s), N.ptr(images[0]), images[0].shape[0], N.ptr(images[1]) if image_b is not None else None,
                                            B, 1 if keep_patches else 0, N.ptr(scratch), scratch.numel(), N.ptr(out), N.stream_ptr(dev)),
                "cmh_vit_patch_embed")
        patches = scratch[:B * g2 * K * e].view(torch.float32 if f32 else torch.bfloat16).view(B * g2, K) if keep_patches else None
        return out, patches

    def encode_text(self, text, key_padding_mask=None, taps=None):
        """text i64 [B,L] -> [B, embed_dim] f32  (reference model/base/model.py:359-372)."""
        kpm = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
        if taps is None and self._wants_tape(T.TEXT):
            _, (text,) = self._operands("encode_text", texts=[text])
            return T.TextTrain.apply(self, text, kpm, *T.TEXT.params(self))
        versions, plain = self._versions(T.TEXT), taps is None and kpm is None
        hit = self._stashed("text", text, (self.pack_text, self._key(T.TEXT, versions))) if plain else None
        if hit is not None:
            return hit
        # only the tokens up to each caption's EOT can reach the pooled row under the causal mask: the packed call skips the padding
        c, = self._open("encode_text", texts=[text], versions={"text": versions}, packed=plain and self.pack_text)
        if c.rows is not None:
            N.check(N.lib().cmh_text_encode_packed(C.byref(c.s), N.ptr(c.x), *c.dims, N.ptr(c.out), N.ptr(c.rows), N.ptr(c.ws),
                                                   c.ws.numel(), c.stream), "cmh_text_encode_packed")
        else:
            tp, _arr = self._taps(taps)
            N.check(N.lib().cmh_text_encode(C.byref(c.s), N.ptr(c.x), *c.dims, N.ptr(kpm), N.ptr(c.out), N.ptr(c.ws), c.ws.numel(),
                                            None if tp is None else C.byref(tp), c.stream), "cmh_text_encode")
        return self._finish(c)[0]

    def prefetch_pair(self, image, text):
        """Inference helper for code that calls encode_image(image) and encode_text(text) back to back (every method model's
        encode_* does, model/modelbase.py:88-92): run both towers NOW in lock-step (encode_pair) and hand the two features out to
        the next encode_image / encode_text call on these very tensors.  Bit-identical to the separate calls; a no-op when a
        gradient is wanted."""
        self.prefetch_pairs([(image, text)])

    def prefetch_pairs(self, batches):
        """prefetch_pair for TWO loader batches [(image_a, text_a), (image_b, text_b)] in one native call (cmh_clip_encode_pair2: the
        batches' rows share every launch; a launch's fixed costs are paid once per 2 x 256 pairs).  Each batch's features are handed
        out to its own encode_image / encode_text calls; bit-identical to two prefetch_pair calls."""
        if torch.is_grad_enabled() and not self.assume_frozen:
            return
        # what a stashed feature depends on besides its input tensor: the arithmetic mode and its tower's weights (and the packing)
        versions = {t.name: self._versions(t) for t in (T.VIT, T.TEXT)}
        fi, ft = self._encode_pairs(batches, versions)
        keys = (self._key(T.VIT, versions["vit"]), (self.pack_text, self._key(T.TEXT, versions["text"])))
        self._pair_stash, lo = {"image": [], "text": []}, 0
        for image, text in batches:
            hi = lo + image.shape[0]
            self._pair_stash["image"].append((image, fi[lo:hi], keys[0]))
            self._pair_stash["text"].append((text, ft[lo:hi], keys[1]))
            lo = hi

    def _stashed(self, side, x, key):
        st = getattr(self, "_pair_stash", None)
        for i, (src, feat, its_key) in enumerate(st.get(side, ()) if st else ()):
            if src is x and its_key == key:
                del st[side][i]
                if not st[side]:
                    del st[side]
                return feat
        return None

    def drop_pair_stash(self):
        """Forget features prefetch_pair computed and nobody picked up; counts them (`pair_stash_misses`) so that a model whose
        encode_* calls never hit the stash - a mask, taps, other tensors - shows up instead of silently paying for both paths."""
        st = getattr(self, "_pair_stash", None)
        if st:
            self.pair_stash_misses = getattr(self, "pair_stash_misses", 0) + sum(len(v) for v in st.values())
        self._pair_stash = {}

    def encode_pair(self, image, text):
        """(encode_image(image), encode_text(text)) with the two towers in lock-step: layer i of both shares its GEMM launches
        (cmh_clip_encode_pair; reference model/modelbase.py:105-108 calls the two encoders back to back).  Bit-identical to the two
        separate calls.  Inference (no tape); training, taps and masks take the single-tower entry points."""
        if self._wants_tape(T.VIT, T.TEXT):
            return self.encode_image(image), self.encode_text(text)
        return self._encode_pairs([(image, text)])

    def encode_pair2(self, image_a, text_a, image_b, text_b):
        """encode_pair of two batches in one native call: (features of [a; b] images, of [a; b] captions).  The images stay two
        tensors (cmh_clip_encode_pair2 patchifies them into one matrix), the captions are concatenated (157 KB).  Inference only."""
        return self._encode_pairs([(image_a, text_a), (image_b, text_b)])

    def _encode_pairs(self, batches, versions=None):
        v, t = self._open("encode_pair" if len(batches) == 1 else "encode_pair2", *zip(*batches), versions=versions, packed=self.pack_text)
        pack, (B, L) = 1 if self.pack_text else 0, t.dims
        tail = (N.ptr(v.out), N.ptr(t.out), N.ptr(t.rows), N.ptr(v.ws), v.ws.numel(), N.ptr(t.ws), t.ws.numel(), v.stream)
        if len(batches) == 1:
            N.check(N.lib().cmh_clip_encode_pair(C.byref(v.s), N.ptr(v.x), C.byref(t.s), N.ptr(t.x), B, L, pack, *tail),
                    "cmh_clip_encode_pair")
        else:
            N.check(N.lib().cmh_clip_encode_pair2(C.byref(v.s), N.ptr(v.x), v.x.shape[0], N.ptr(v.more[0]), v.more[0].shape[0],
                                                  C.byref(t.s), N.ptr(t.x), L, pack, *tail), "cmh_clip_encode_pair2")
        return self._finish(v, t)

    def forward(self, image, text):
        """Cosine-similarity logits (reference :374-388); assembled from the two native encodes."""
        i = self.encode_image(image)
        t = self.encode_text(text)
        i = i / i.norm(dim=-1, keepdim=True)
        t = t / t.norm(dim=-1, keepdim=True)
        logits = self.logit_scale.exp() * i @ t.t()
        return logits, logits.t()


def convert_weights(model: nn.Module):
    """Reference :391-412: Conv/Linear weight+bias, MHA in_proj/bias and the two projections go to fp16.
    Checkpoints loaded afterwards are therefore rounded through fp16, exactly as upstream."""

    def _convert(l):
        if isinstance(l, (nn.Conv1d, nn.Conv2d, nn.Linear)):
            l.weight.data = l.weight.data.half()
            if l.bias is not None:
                l.bias.data = l.bias.data.half()
        if isinstance(l, nn.MultiheadAttention):
            for attr in [*[f"{s}_proj_weight" for s in ["in", "q", "k", "v"]], "in_proj_bias", "bias_k", "bias_v"]:
                tensor = getattr(l, attr)
                if tensor is not None:
                    tensor.data = tensor.data.half()
        for name in ["text_projection", "proj"]:
            if hasattr(l, name):
                attr = getattr(l, name)
                if attr is not None:
                    attr.data = attr.data.half()

    model.apply(_convert)


def infer_shapes(state_dict: dict) -> dict:
    """Reference :415-437: the constructor's arguments from the checkpoint's tensor shapes."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("only ViT CLIP checkpoints are supported (no visual.proj in state_dict)")
    patch = state_dict["visual.conv1.weight"].shape[-1]
    width = state_dict["ln_final.weight"].shape[0]
    return dict(embed_dim=state_dict["text_projection"].shape[1],
                image_resolution=patch * round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5),
                vision_layers=len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")]),
                vision_width=state_dict["visual.conv1.weight"].shape[0], vision_patch_size=patch,
                context_length=state_dict["positional_embedding"].shape[0], vocab_size=state_dict["token_embedding.weight"].shape[0],
                transformer_width=width, transformer_heads=width // 64,
                transformer_layers=len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks"))))


def build_model(state_dict: dict, cls=CLIP, accept=None):
    """Reference :415-455: infer the architecture from tensor shapes, fp16-convert, load strict.  `accept(shapes)` may refuse them."""
    shapes = infer_shapes(state_dict)
    if accept is not None:
        accept(shapes)
    model = cls(**shapes)
    for key in ["input_resolution", "context_length", "vocab_size"]:
        if key in state_dict:
            del state_dict[key]
    convert_weights(model)
    model.load_state_dict(state_dict)
    return model

