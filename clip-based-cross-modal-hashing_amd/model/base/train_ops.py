"""The towers' parameter tables and autograd bridges.

Tables: which parameter goes to which field of the ctypes structs (include/cmh.h), written once; the parameter lists, the weight
structs (model/base/model.py), the gradient structs and every cache key are derived from them.
Bridges: forward = cmh_*_forward_train (keeps a tape), backward = cmh_*_backward, which writes one f32 gradient per parameter
(include/cmh.h "Training forward ... and backward").  Used by CLIP.encode_image / encode_text whenever gradients are enabled and
a tower parameter requires them; under torch.no_grad() the plain encode entry points run instead."""
import ctypes as C
from operator import attrgetter

import torch

import cmh_native as N

# (cmh_block_weights / cmh_block_grads field, the parameter inside a ResidualAttentionBlock, is a GEMM weight), in the structs' order
BLOCK_TABLE = tuple((f, attrgetter(a), g) for f, a, g in (
    ("in_proj_w", "attn.in_proj_weight", True), ("in_proj_b", "attn.in_proj_bias", False),
    ("out_proj_w", "attn.out_proj.weight", True), ("out_proj_b", "attn.out_proj.bias", False),
    ("ln1_w", "ln_1.weight", False), ("ln1_b", "ln_1.bias", False), ("ln2_w", "ln_2.weight", False), ("ln2_b", "ln_2.bias", False),
    ("fc_w", "mlp.c_fc.weight", True), ("fc_b", "mlp.c_fc.bias", False),
    ("proj_w", "mlp.c_proj.weight", True), ("proj_b", "mlp.c_proj.bias", False)))


class Tower:
    """One tower: where its module sits in a CLIP, its two structs, the head rows the first backward part completes, the integer
    fields of its weights struct, and its head table (weights-struct field, grads-struct field, parameter, is a GEMM weight) in
    the grads struct's order.  A GEMM weight whose two fields differ (`proj_t` / `proj`) is handed to the library transposed."""

    def __init__(self, name, root, weights, grads, first, geometry, head):
        self.name, self.root, self.weights, self.grads, self.first, self.geometry = name, root, weights, grads, first, geometry
        self.head = tuple((w, g, attrgetter(a), gemm) for w, g, a, gemm in head)
        self.text = name == "text"          # operands [B, L] with a key-padding mask; the image tower's are [B, ...]

    def params(self, clip):
        return _params(self.head, self.root(clip))

    def projection(self, clip):
        """the head's last parameter: the projection the tower's output leaves through"""
        return self.head[-1][2](self.root(clip))


def _params(head, root):
    return [get(root) for *_, get, _ in head] + blocks_params(root.transformer.resblocks)


VIT = Tower("vit", attrgetter("visual"), N.VitWeights, N.VitGrads, (5, 6, 7),        # ln_post.weight / bias, proj: first part
            lambda v: dict(resolution=v.input_resolution, patch=v.conv1.weight.shape[-1], width=v.conv1.weight.shape[0],
                           embed_dim=v.proj.shape[1]),
            (("conv1_w", "conv1_w", "conv1.weight", True), ("class_embedding", "class_embedding", "class_embedding", False),
             ("positional_embedding", "positional_embedding", "positional_embedding", False),
             ("ln_pre_w", "ln_pre_w", "ln_pre.weight", False), ("ln_pre_b", "ln_pre_b", "ln_pre.bias", False),
             ("ln_post_w", "ln_post_w", "ln_post.weight", False), ("ln_post_b", "ln_post_b", "ln_post.bias", False),
             ("proj_t", "proj", "proj", True)))
TEXT = Tower("text", lambda clip: clip, N.TextWeights, N.TextGrads, (2, 3, 4),        # ln_final.weight / bias, text_projection
             lambda c: dict(context_length=c.positional_embedding.shape[0], vocab_size=c.token_embedding.weight.shape[0],
                            width=c.ln_final.weight.shape[0], embed_dim=c.text_projection.shape[1]),
             (("token_embedding", "token_embedding", "token_embedding.weight", False),
              ("positional_embedding", "positional_embedding", "positional_embedding", False),
              ("ln_final_w", "ln_final_w", "ln_final.weight", False), ("ln_final_b", "ln_final_b", "ln_final.bias", False),
              ("text_projection_t", "text_projection", "text_projection", True)))


def block_params(blk):
    """the 12 parameters of one ResidualAttentionBlock in cmh_block_weights order"""
    return [get(blk) for _, get, _ in BLOCK_TABLE]


def blocks_params(resblocks):
    return [p for blk in resblocks for p in block_params(blk)]


def vit_params(v):
    return _params(VIT.head, v)


def text_params(clip):
    return _params(TEXT.head, clip)


# Data-parallel hook (dist_utils.GradSync): called as BUCKET_SINK(flat_slice, params, views) from inside a tower's backward the
# moment a part of the pass has written its last gradient, with the 1-D f32 slice of the flat buffer that holds exactly that part's
# gradients (views[i] = the gradient of params[i] inside it); the sink may queue an in-place all-reduce on the slice: the values
# reach the parameters' .grad (those very views, once autograd has adopted them) without any packing or copy-back.
BUCKET_SINK = None
PARTS = 3          # tower backward calls per step: blocks in PARTS near-equal ranges, last layers first


def _grad_buffers(params, order=None):
    """One flat f32 buffer for all gradients of a tower call; returns (grads as views in `params` order, flat).  `order` lists
    the parameter indices in the order the backward pass completes them, so that every part is one contiguous slice."""
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise N.NativeError("training needs contiguous float32 parameters (model.float())")
    order = list(range(len(params))) if order is None else order
    sizes = [(params[i].numel() + 3) // 4 * 4 for i in order]                 # 16-byte aligned views
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=params[0].device)
    grads, off = [None] * len(params), 0
    for i, n in zip(order, sizes):
        grads[i] = flat[off:off + params[i].numel()].view_as(params[i])
        off += n
    return grads, flat


def _layer_parts(layers, parts=None):
    """[(hi, lo), ...] block ranges of the backward calls, last layers first"""
    parts = max(1, min(parts or PARTS, layers)) if layers > 0 else 1
    cuts = [layers - (layers * k) // parts for k in range(parts + 1)]
    return [(cuts[k], cuts[k + 1]) for k in range(parts)]


def _part_order(nhead, head_first, layers, ranges):
    """Flat-buffer order and slice boundaries: [head parameters that the first part completes][blocks of part 0, last first] ...
    [blocks of the last part][head parameters that the last part completes].  -> (order, element boundaries per part)"""
    order, bounds = list(head_first), []
    for k, (hi, lo) in enumerate(ranges):
        for layer in range(hi - 1, lo - 1, -1):
            order += list(range(nhead + 12 * layer, nhead + 12 * (layer + 1)))
        if k == len(ranges) - 1:
            order += [i for i in range(nhead) if i not in head_first]
        bounds.append(len(order))
    return order, bounds


def _sink(flat, params, grads, order, bounds, k):
    if BUCKET_SINK is None:
        return
    size = lambda i: (params[i].numel() + 3) // 4 * 4
    lo = sum(size(i) for i in order[:bounds[k - 1]]) if k else 0
    hi = sum(size(i) for i in order[:bounds[k]])
    idx = order[(bounds[k - 1] if k else 0):bounds[k]]
    BUCKET_SINK(flat[lo:hi], [params[i] for i in idx], [grads[i] for i in idx])


def _block_grads(grads, nhead=0):
    """cmh_block_grads array over `grads`, a tower's (after its `nhead` head gradients) or a bare stack's, in block_params order"""
    layers = (len(grads) - nhead) // len(BLOCK_TABLE)
    arr = (N.BlockGrads * layers)()
    for i in range(layers):
        for j, (field, *_) in enumerate(BLOCK_TABLE):
            setattr(arr[i], field, grads[nhead + len(BLOCK_TABLE) * i + j].data_ptr())
    return arr


def _grad_call(params, nhead, struct, order=None):
    """What every backward bridge sets up: the flat buffer and its views, the block array (returned to be kept alive) and the
    tower's gradient struct over them -> (grads, flat, blocks, struct)"""
    grads, flat = _grad_buffers(params, order)
    blocks = _block_grads(grads, nhead)
    return grads, flat, blocks, struct(*[t.data_ptr() for t in grads[:nhead]], C.cast(blocks, C.POINTER(N.BlockGrads)))


def _forward(ctx, tower, tokens, clip, x, kpm, params):
    """The four bridges' forward: pooled -> features [B, E]; tokens -> every position projected [B*T, E] (+ the text tower's EOT
    rows i32 [B]).  The ctx holds the cache entry the struct came from: its `keep` tensors and block array are what the struct
    points at, and a later rebuild of the cache must not free them under the backward."""
    held = clip._tower_entry(tower)
    s, dev = held.struct, x.device
    dims = tuple(x.shape[:2]) if tower.text else (x.shape[0],)
    name = f"cmh_{tower.name}_forward_train"
    outs = [torch.empty(dims[0], s.embed_dim, dtype=torch.float32, device=dev)]
    if tokens:
        per = dims[1] if tower.text else (s.resolution // s.patch) ** 2 + 1
        outs = [torch.empty(dims[0] * per, s.embed_dim, dtype=torch.float32, device=dev)]
        name += "_tokens"
        if tower.text:
            outs.append(torch.empty(dims[0], dtype=torch.int32, device=dev))
            # (padded_tokens_unused, set by MITH: nobody reads the padded positions - they are neither computed nor differentiated)
            name += "_packed" if getattr(clip, "padded_tokens_unused", False) and kpm is not None else ""
    tape = torch.empty(getattr(N.lib(), f"cmh_{tower.name}_train_bytes")(C.byref(s), *dims), dtype=torch.uint8, device=dev)
    N.check(getattr(N.lib(), name)(C.byref(s), N.ptr(x), *dims, *([N.ptr(kpm)] if tower.text else []), *map(N.ptr, outs), N.ptr(tape),
                                   tape.numel(), N.stream_ptr(dev)), name)
    ctx.tape, ctx.held, ctx.dims, ctx.params = tape, held, dims, params
    ctx.x, ctx.kpm = (x, kpm) if tower.text else (None, None)          # the text backward reads the captions again
    return outs


def _backward(ctx, tower, tokens, dout):
    """The four bridges' backward -> the parameters' gradients.  Pooled: PARTS calls over block ranges, each part's slice of the flat
    buffer reported to BUCKET_SINK as it completes; tokens: one call, one report."""
    s, params, nhead = ctx.held.struct, ctx.params, len(tower.head)
    ranges = [()] if tokens else _layer_parts(s.layers)
    order, bounds = (None, None) if tokens else _part_order(nhead, tower.first, s.layers, ranges)
    grads, flat, _blocks, g = _grad_call(params, nhead, tower.grads, order)
    dout = N.f32c(dout)
    operand = (N.ptr(ctx.x), *ctx.dims, N.ptr(ctx.kpm)) if tower.text else ctx.dims
    name = f"cmh_{tower.name}_backward_{'tokens' if tokens else 'part'}"
    for k, part in enumerate(ranges):
        N.check(getattr(N.lib(), name)(C.byref(s), *operand, N.ptr(dout), C.byref(g), N.ptr(ctx.tape), ctx.tape.numel(), *part,
                                       N.stream_ptr(dout.device)), name)
        if not tokens:
            _sink(flat, params, grads, order, bounds, k)
        elif BUCKET_SINK is not None:
            BUCKET_SINK(flat, list(params), list(grads))
    ctx.tape = None
    return tuple(grads)


class VitTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip, image, *params):
        return _forward(ctx, VIT, False, clip, image, None, params)[0]

    @staticmethod
    def backward(ctx, dfeat):
        return (None, None) + _backward(ctx, VIT, False, dfeat)


class TextTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip, text, kpm, *params):
        return _forward(ctx, TEXT, False, clip, text, kpm, params)[0]

    @staticmethod
    def backward(ctx, dfeat):
        return (None, None, None) + _backward(ctx, TEXT, False, dfeat)


class VitTrainTokens(torch.autograd.Function):
    """The MITH trunk's image tower under training: every token projected (model/MITH.py:56-82) -> [B*T, E]."""

    @staticmethod
    def forward(ctx, clip, image, *params):
        return _forward(ctx, VIT, True, clip, image, None, params)[0]

    @staticmethod
    def backward(ctx, dtok):
        return (None, None) + _backward(ctx, VIT, True, dtok)


class TextTrainTokens(torch.autograd.Function):
    """The MITH trunk's text tower under training (model/MITH.py:120-144) -> ([B*L, E] tokens, eot rows i32 [B])."""

    @staticmethod
    def forward(ctx, clip, text, kpm, *params):
        tok, rows = _forward(ctx, TEXT, True, clip, text, kpm, params)
        ctx.mark_non_differentiable(rows)
        return tok, rows

    @staticmethod
    def backward(ctx, dtok, _drows):
        return (None, None, None) + _backward(ctx, TEXT, True, dtok)
