"""ORACLE — TEST INFRASTRUCTURE ONLY.  The reference's two CLIP towers as a DIFFERENTIABLE restatement in plain PyTorch ops, in
any dtype on any device (the checker of the training towers' gradients runs it in float64 on the GPU: torch's own fp64 ops, nothing
of libcmh).  Written fresh; the ops are the ones the reference's modules call:
  LayerNorm / QuickGELU / ResidualAttentionBlock   reference model/base/model.py:153-196  (F.layer_norm, F.multi_head_attention_forward)
  VisionTransformer.forward                          reference model/base/model.py:228-252  (F.conv2d patches, class token, ln_pre, ln_post, proj)
  CLIP.build_attention_mask / encode_text            reference model/base/model.py:340-346, :359-372  (causal -inf mask, EOT pooling by argmax)
Unlike oracle/torch_cpu.py (the timed CPU baseline, inference only) every state-dict tensor is a leaf that collects its gradient.
Pinned against the reference's own fp32 autograd (tests/golden/clip_tiny_grads.npz) and forward (clip_vitb32.npz) in
tests/test_oracle_clip_grads.py."""
import torch
import torch.nn.functional as F


def leaves(state_dict, device="cpu", dtype=torch.float64):
    """{name: leaf tensor of `dtype` on `device` with requires_grad} from a state dict of numpy arrays or tensors"""
    return {k: torch.as_tensor(v).to(device=device, dtype=dtype).detach().requires_grad_(True) for k, v in state_dict.items()}


def _layers(p, prefix):
    n = 0
    while f"{prefix}{n}.ln_1.weight" in p:
        n += 1
    return n


def _block(x, p, pre, heads, mask):
    """x [L, N, d] (sequence first, as nn.MultiheadAttention takes it) -> x + attn(ln_1(x)) + mlp(ln_2(.))"""
    d = x.shape[-1]
    h = F.layer_norm(x, (d,), p[pre + "ln_1.weight"], p[pre + "ln_1.bias"], 1e-5)
    a = F.multi_head_attention_forward(h, h, h, d, heads, p[pre + "attn.in_proj_weight"], p[pre + "attn.in_proj_bias"], None, None,
                                       False, 0.0, p[pre + "attn.out_proj.weight"], p[pre + "attn.out_proj.bias"], training=False,
                                       need_weights=False, attn_mask=mask)[0]
    x = x + a
    h = F.layer_norm(x, (d,), p[pre + "ln_2.weight"], p[pre + "ln_2.bias"], 1e-5)
    h = F.linear(h, p[pre + "mlp.c_fc.weight"], p[pre + "mlp.c_fc.bias"])
    h = h * torch.sigmoid(1.702 * h)
    return x + F.linear(h, p[pre + "mlp.c_proj.weight"], p[pre + "mlp.c_proj.bias"])


def encode_image(p, image):
    """p: leaves(...); image [B, 3, R, R] -> [B, embed_dim] in p's dtype"""
    w = p["visual.conv1.weight"]
    x = F.conv2d(torch.as_tensor(image).to(device=w.device, dtype=w.dtype), w, stride=w.shape[-1])
    B, d = x.shape[0], x.shape[1]
    x = x.reshape(B, d, -1).permute(0, 2, 1)
    x = torch.cat([p["visual.class_embedding"].expand(B, 1, d), x], 1) + p["visual.positional_embedding"]
    x = F.layer_norm(x, (d,), p["visual.ln_pre.weight"], p["visual.ln_pre.bias"], 1e-5).permute(1, 0, 2)
    for i in range(_layers(p, "visual.transformer.resblocks.")):
        x = _block(x, p, f"visual.transformer.resblocks.{i}.", d // 64, None)
    x = F.layer_norm(x[0], (d,), p["visual.ln_post.weight"], p["visual.ln_post.bias"], 1e-5)
    return x @ p["visual.proj"]


def encode_text(p, text):
    """p: leaves(...); text int [B, L] (EOT = the largest id of each row) -> [B, embed_dim] in p's dtype"""
    emb = p["token_embedding.weight"]
    text = torch.as_tensor(text).to(device=emb.device, dtype=torch.int64)
    L = text.shape[1]
    x = emb[text] + p["positional_embedding"][:L]
    d = x.shape[-1]
    mask = torch.full((L, L), float("-inf"), dtype=emb.dtype, device=emb.device).triu_(1)
    x = x.permute(1, 0, 2)
    for i in range(_layers(p, "transformer.resblocks.")):
        x = _block(x, p, f"transformer.resblocks.{i}.", d // 64, mask)
    x = F.layer_norm(x.permute(1, 0, 2), (d,), p["ln_final.weight"], p["ln_final.bias"], 1e-5)
    return x[torch.arange(x.shape[0], device=x.device), text.argmax(-1)] @ p["text_projection"]


def towers(state_dict, image, text, gi, gt, device="cpu", dtype=torch.float64):
    """-> (img_feat, txt_feat, grads): the features and, for L = sum(img_feat * gi) + sum(txt_feat * gt), the gradient of every
    state-dict tensor L depends on ({name: tensor}; logit_scale is not on the towers' path and has none), all in `dtype` on
    `device`.  One tower at a time: the image tower's graph is freed before the text tower's is built."""
    p = leaves(state_dict, device, dtype)
    feats = []
    for fn, x, g in ((encode_image, image, gi), (encode_text, text, gt)):
        f = fn(p, x)
        (f * torch.as_tensor(g).to(device=device, dtype=dtype)).sum().backward()
        feats.append(f.detach())
        del f
    grads = {k: v.grad for k, v in p.items() if v.grad is not None}
    return feats[0], feats[1], grads
