// What encoders.hip (inference) and encoders_bwd.hip (training forward) share: the launch sequence of one
// ResidualAttentionBlock, stated once (block_forward, defined in encoders.hip), and the few pieces around it that both towers'
// stems and heads use.  Host code only.
#pragma once

#include "cmh_common.h"

namespace cmh {

// 256-byte bump allocator over a caller-owned workspace; base == nullptr only measures (off = the bytes needed)
struct Arena {
  char* base;
  size_t off = 0;
  explicit Arena(void* p) : base(static_cast<char*>(p)) {}
  template <typename T = void> T* take(size_t bytes) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(bytes, 256);
    return p;
  }
};

// One tower's view of one block: what block_forward needs to know, and nothing a kernel does not read.
//   head (M rows):  h1 = ln_1(x_in);  qkv = in_proj(h1);  attn = attention(qkv)
//   tail (Mt rows): x_mid = x_res + out_proj(attn);  h2 = ln_2(x_mid);  act = QuickGELU(c_fc(h2));  x_out = x_mid + c_proj(act)
// Inference runs one stream in place (x_in = x_mid = x_out, h1 = attn = h2); training points every stage at its own tape slot.
struct Lane {
  const cmh_block_weights* w = nullptr;                  // this layer's weights (the caller sets it per layer)
  int dtb = 0, xh = 0;                                   // arithmetic of the four GEMMs (CMH_F32 | CMH_BF16 | CMH_FP8); x holds fp16
  int B = 0, T = 0, d = 0, causal = 0, M = 0;            // M: rows of the head (an upper bound when md is set)
  const uint8_t* kpm = nullptr;                          // key padding mask [B, T]
  const int32_t* seq_off = nullptr;                      // packed text: per-caption row offsets
  const int32_t* md = nullptr;                           // packed text: the row count on the device
  int mh = -1;                                           // ... and its likely value (tile heights only)
  const void* x_in = nullptr;
  void *h1 = nullptr, *qkv = nullptr, *attn = nullptr, *x_mid = nullptr, *h2 = nullptr, *act = nullptr, *x_out = nullptr;
  // options
  float* amax = nullptr;       // [4] fp8 calibration (bf16 mode): running maxima of the four GEMM inputs, a reduction after each producer
  void* pre = nullptr;         // training: c_fc's PRE-activation [Mt, 4d] is kept here for the backward
  // The pooled tail: after the attention nothing mixes rows any more, so only the B rows pooled[b] are carried on: x_in's rows are
  // gathered into x_mid (and updated there in place), attn's into attn_p, and the tail runs on Mt = B rows (few-row kernels).
  const int32_t* pooled = nullptr;
  void* attn_p = nullptr;
};

// The block for one tower (b == nullptr) or for two in lock-step (grouped GEMM launches; see encoders.hip)
int block_forward(const Lane& a, const Lane* b, hipStream_t st);

// fp16 residual stream?  The bf16 mode's rule, for inference and training alike: the residual GEMMs must take the wide kernel
// (width % 256 == 0); CMH_RESID_F16=0 keeps the stream f32.
int resid_f16(int dt, int d);

// conv1 (kernel = stride = patch, no bias) as a patch-matrix GEMM into patch_out [B*g2, d] f32  (model/base/model.py:215,231-235).
// image_b / batch_a: the batch comes as two tensors, rows [0, batch_a) from `image`.  conv1_w_pad: scratch of the K-padded weight.
// keep_patches: the caller reads the patch matrix afterwards (training: conv1's weight gradient), so it must be written; false lets
// the fused stem (conv1_stem.hip) run instead where it is built for the shape and switched on - `patches` is then left untouched.
int conv1_stem(const cmh_vit_weights* w, int dt, const float* image, const float* image_b, int batch_a, int B, void* patches,
               bool keep_patches, void* conv1_w_pad, float* patch_out, hipStream_t st);

// feat [B, embed] f32 = pool [B, d] . w_t^T: the last projection of either tower (no bias)
int final_projection(int dt, const void* pool, const void* w_t, float* feat, int B, int embed, int d, hipStream_t st);

}  // namespace cmh
