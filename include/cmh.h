/*
 * cmh.h — C ABI of libcmh.so, the MI355X (gfx950) native hot path of CLIP-based cross-modal hashing.
 *
 * Drop-in boundary.  The reference (QinLab-WFU/CLIP-based-Cross-Modal-Hashing) is pure Python on
 * PyTorch and has no FFI of its own; these entry points are what a ctypes binding
 * for its hot path binds.  Each one names the reference interface it replaces (paths relative to
 * the reference root).  The Python mirror of the reference API that calls them lives in
 * clip-based-cross-modal-hashing_amd/ (model/modelbase.py, model/base/model.py, utils/calc_utils.py ...);
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch types.  All data pointers are DEVICE pointers unless
 *    a parameter says "host".  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - the library never allocates or frees DEVICE memory: scratch comes from the caller
 *    (`workspace`, size from the matching *_workspace_bytes()).  It owns two small page-locked HOST
 *    buffers, created on first use and kept for the life of the process: the staging ring of
 *    cmh_bert_adam_step's tensor tables and one 64-byte word through which the packed text
 *    encoders learn, without waiting, how many rows earlier calls packed.
 *  - the inference entry points (cmh_vit_encode*, cmh_text_encode*, heads, losses, codes, ranking)
 *    only enqueue kernels on `stream` and never wait for the device (graph-capturable).  The
 *    calls that DO wait for `stream` say so at their declaration: the fp8 calibration pass
 *    (cmh_*_calibrate_fp8), cmh_prof_gemm_end, the packed TRAINING forward of the text tower
 *    (cmh_text_forward_train reads the packed row count once: it sizes the tape's grids and the
 *    backward's split-K plans), and towers whose width is not a multiple of 256 when they take
 *    packed captions (test-sized configurations).
 *  - return value: 0 on success, negative cmh_status on error; cmh_last_error() gives the text
 *    (thread-local).  No exceptions cross the ABI.
 *  - matrices are dense row-major.  Linear weights are [out_features, in_features] exactly as
 *    torch.nn.Linear / nn.MultiheadAttention store them.
 *  - activations are token-major [B*T, d] (batch folded into rows), not the reference's [T,B,d];
 *    values are identical.
 */
#ifndef CMH_H_
#define CMH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMH_VERSION 6   /* = the round that last changed a struct layout or a signature; cmh_native.lib() refuses any other */

typedef enum cmh_status {
  CMH_OK = 0,
  CMH_ERR_INVALID = -1,     /* bad argument / unsupported shape */
  CMH_ERR_WORKSPACE = -2,   /* workspace too small */
  CMH_ERR_LAUNCH = -3,      /* HIP launch / runtime error */
  CMH_ERR_DATA = -4         /* input data outside the domain (e.g. codes not in {-1,0,+1}) */
} cmh_status;

/* GEMM arithmetic of the encoder.  CMH_F32: f32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 FMA
 * chain; the parity mode against the fp32 reference, train/.../hash_train.py `self.model.float()`).
 * CMH_BF16: bf16 operands, fp32 accumulate on v_mfma_f32_16x16x32_bf16; LayerNorm/softmax/residual
 * stream stay fp32. */
typedef enum cmh_dtype { CMH_F32 = 0, CMH_BF16 = 1, CMH_FP8 = 2 } cmh_dtype;
/* CMH_FP8 (BASELINE configs[4] "fp8 MFMA CLIP encoders"): the four GEMMs of every block (QKV, out_proj, c_fc, c_proj) take OCP
 * e4m3 operands on v_mfma_scale_f32_16x16x128_f8f6f4 (f32 accumulate): weights quantised per output channel, activations per
 * tensor with scales from a calibration pass; everything else as CMH_BF16 (fp16 residual stream, f32 LayerNorm statistics and
 * softmax; conv1 and the final projections stay bf16).  Needs width % 256 == 0.  See "fp8 encoder mode" below. */

const char* cmh_last_error(void);
int cmh_version(void);

/* ---------------------------------------------------------------------------------------------
 * Encoder weights.  Pointers borrow caller-owned device memory.  `*_w` GEMM weights are in the
 * dtype named by cmh_*_weights.gemm_dtype (f32 or bf16 copies made with cmh_cast_f32_to_bf16);
 * biases, LayerNorm parameters and embeddings are always f32.
 * One transformer block = reference model/base/model.py:167-196 ResidualAttentionBlock.
 * ------------------------------------------------------------------------------------------- */
typedef struct cmh_block_weights {
  const void* in_proj_w;    /* [3d, d]  attn.in_proj_weight */
  const float* in_proj_b;   /* [3d]     attn.in_proj_bias   */
  const void* out_proj_w;   /* [d, d]   attn.out_proj.weight */
  const float* out_proj_b;  /* [d] */
  const float* ln1_w;       /* [d] ln_1 */
  const float* ln1_b;
  const float* ln2_w;       /* [d] ln_2 */
  const float* ln2_b;
  const void* fc_w;         /* [4d, d]  mlp.c_fc.weight */
  const float* fc_b;        /* [4d] */
  const void* proj_w;       /* [d, 4d]  mlp.c_proj.weight */
  const float* proj_b;      /* [d] */
  /* CMH_FP8 only (ignored otherwise): the four `*_w` above are e4m3 bytes from cmh_fp8_quantize_weight */
  const float* in_proj_cs;  /* [3d] per-output-channel scales of in_proj_w */
  const float* out_proj_cs; /* [d] */
  const float* fc_cs;       /* [4d] */
  const float* proj_cs;     /* [d] */
  float act_scale[4];       /* per-tensor scales of the four GEMM inputs: ln_1 output, attention output, ln_2 output,
                             * QuickGELU(c_fc) output; x_fp8 = e4m3(x / act_scale).  From cmh_*_calibrate_fp8: headroom * amax / 448 */
} cmh_block_weights;

/* Image tower = reference model/base/model.py:210-252 VisionTransformer. */
typedef struct cmh_vit_weights {
  int32_t gemm_dtype;       /* cmh_dtype of every `const void*` weight below and in blocks[] */
  int32_t resolution;       /* input H = W (224) */
  int32_t patch;            /* 32 */
  int32_t width;            /* 768; heads = width/64 (model.py:284) */
  int32_t layers;           /* 12 */
  int32_t embed_dim;        /* 512 */
  const void* conv1_w;      /* [width, 3*patch*patch]  visual.conv1.weight flattened (c,py,px) */
  const float* class_embedding;      /* [width] */
  const float* positional_embedding; /* [grid*grid+1, width] */
  const float* ln_pre_w;  const float* ln_pre_b;
  const float* ln_post_w; const float* ln_post_b;
  const void* proj_t;       /* [embed_dim, width] = visual.proj TRANSPOSED (Linear layout) */
  const cmh_block_weights* blocks;   /* host array [layers] */
} cmh_vit_weights;

/* Text tower = reference model/base/model.py:359-372 CLIP.encode_text (+ :340-346 causal mask). */
typedef struct cmh_text_weights {
  int32_t gemm_dtype;
  int32_t context_length;   /* 77 */
  int32_t vocab_size;       /* 49408 */
  int32_t width;            /* 512; heads = width/64 (model.py:437) */
  int32_t layers;           /* 12 */
  int32_t embed_dim;        /* 512 */
  const float* token_embedding;      /* [vocab, width] */
  const float* positional_embedding; /* [context_length, width] */
  const float* ln_final_w; const float* ln_final_b;
  const void* text_projection_t;     /* [embed_dim, width] = text_projection TRANSPOSED */
  const cmh_block_weights* blocks;   /* host array [layers] */
} cmh_text_weights;

/* Optional taps for parity tests: when non-NULL the f32 residual stream [B*T, width] after
 * ln_pre (vision only, index 0) / after block i (index 1+i) is copied to taps[index]. */
typedef struct cmh_taps {
  float* const* ptrs;       /* host array of device pointers (entries may be NULL) */
  int32_t count;
} cmh_taps;

size_t cmh_vit_workspace_bytes(const cmh_vit_weights* w, int32_t batch);
size_t cmh_text_workspace_bytes(const cmh_text_weights* w, int32_t batch, int32_t seq_len);

/* encode_image: replaces CLIP.encode_image / VisionTransformer.forward (model/base/model.py:228-252,
 * :356-357).  image f32 [B,3,R,R] NCHW -> feat f32 [B, embed_dim]. */
int cmh_vit_encode(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat,
                   void* workspace, size_t workspace_bytes, const cmh_taps* taps, void* stream);

/* encode_text: replaces CLIP.encode_text (model/base/model.py:359-372).
 * tokens i64 [B, L] (L <= context_length) -> feat f32 [B, embed_dim]; the pooled row is
 * argmax(tokens[b]) (first maximum), as the reference takes it.
 * key_padding_mask (optional, u8 [B,L], 1 = ignore key) serves the MITH trunk (model/MITH.py:120-144). */
int cmh_text_encode(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                    const uint8_t* key_padding_mask, float* feat, void* workspace,
                    size_t workspace_bytes, const cmh_taps* taps, void* stream);

/* Calibration pass of the fp8 mode: the CMH_BF16 encode of this batch (`w` holds bf16 weights; feat as cmh_vit_encode /
 * cmh_text_encode_packed) which also records, per block i, the largest magnitude of the four GEMM inputs into
 * amax[4*i + {0: ln_1 output, 1: attention output, 2: ln_2 output, 3: QuickGELU(c_fc) output}] (device f32 [4*layers], running
 * maximum: zero it before the first batch).  The host turns it into cmh_block_weights.act_scale. */
int cmh_vit_calibrate_fp8(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, float* amax, void* workspace,
                          size_t workspace_bytes, void* stream);
int cmh_text_calibrate_fp8(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len, float* feat,
                           float* amax, void* workspace, size_t workspace_bytes, void* stream);

/* encode_text without the padding: under the causal mask (model/base/model.py:340-346) no token after a caption's EOT can
 * influence the EOT row that encode_text returns (:366-370), so only the tokens 0..EOT of every caption are computed, packed
 * into one matrix of <= batch*seq_len rows.  `feat` is bit-identical to cmh_text_encode's.  Nothing is synchronised: the packed row
 * count stays on the device - LayerNorm and the GEMM kernels read it themselves (their grids are sized for batch*seq_len rows) - and
 * rows_computed_dev (DEVICE int32 [1], may be NULL) receives a copy for the caller to read whenever it likes.  The GEMMs' tile
 * height is chosen for the count of an earlier call with the same (batch, seq_len), fetched without ever waiting; the first call
 * assumes batch*seq_len.  (Widths that are not a multiple of 256 - test-sized towers on the 128 x 128 fallback GEMMs - read the count
 * back once instead.)  Same workspace as cmh_text_encode. */
int cmh_text_encode_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len, float* feat,
                           int32_t* rows_computed_dev, void* workspace, size_t workspace_bytes, void* stream);
/* encode_image + encode_text of one batch with the two towers in lock-step (reference model/modelbase.py:105-108 calls them back to
 * back): layer i of both towers shares its GEMM launches (cmh_linear_gemm_grouped's kernel).  image f32 [batch,3,R,R], tokens i64
 * [batch, seq_len]; packed != 0: the text tower skips the positions after each caption's EOT like cmh_text_encode_packed
 * (rows_computed_dev as there, may be NULL).  Workspaces as for cmh_vit_encode / cmh_text_encode.  feat_image / feat_text
 * [batch, embed_dim] f32: bit-identical to the two single-tower calls.  Both towers must share gemm_dtype. */
int cmh_clip_encode_pair(const cmh_vit_weights* vw, const float* image, const cmh_text_weights* tw, const int64_t* tokens,
                         int32_t batch, int32_t seq_len, int32_t packed, float* feat_image, float* feat_text,
                         int32_t* rows_computed_dev, void* ws_image, size_t ws_image_bytes, void* ws_text, size_t ws_text_bytes,
                         void* stream);
/* The same for TWO loader batches in one call (the evaluation loop train/base.py:130-148 walks independent batches): the images of
 * the two batches stay two tensors (batch_a, batch_b rows), their captions come as one [batch_a + batch_b, seq_len] matrix; feat_image /
 * feat_text [batch_a + batch_b, embed_dim], batch a's rows first.  Same bits per row as cmh_clip_encode_pair on each batch; the
 * workspaces are sized for batch_a + batch_b. */
int cmh_clip_encode_pair2(const cmh_vit_weights* vw, const float* image_a, int32_t batch_a, const float* image_b, int32_t batch_b,
                          const cmh_text_weights* tw, const int64_t* tokens, int32_t seq_len, int32_t packed,
                          float* feat_image, float* feat_text, int32_t* rows_computed_dev, void* ws_image,
                          size_t ws_image_bytes, void* ws_text, size_t ws_text_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Building blocks of the towers, exported for unit-level parity tests and for heads that want them.
 * ------------------------------------------------------------------------------------------- */
#define CMH_EPI_BIAS 1        /* + bias[n] */
#define CMH_EPI_QUICKGELU 2   /* x*sigmoid(1.702x), model/base/model.py:162-164 */
#define CMH_EPI_RESIDUAL 4    /* + residual[m,n] (f32; may alias out) */
#define CMH_EPI_OUT_BF16 8    /* out is bf16 instead of f32 */
/* out[M,N] = epi(x[M,K] . w[N,K]^T): nn.Linear with the epilogue fused.  x,w in `dtype`.
 * Needs N % 128 == 0 and K % 32 (f32) / 64 (bf16) == 0. */
int cmh_linear_gemm(int32_t dtype, const void* x, const void* w, const float* bias, const float* residual,
                    void* out, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream);
/* LayerNorm over the last dim of x f32 [M,d] (eps 1e-5, fp32 statistics; model/base/model.py:153-159). */
int cmh_layernorm(const float* x, const float* w, const float* b, void* out, int32_t out_dtype, int32_t M,
                  int32_t d, void* stream);
/* Two GEMMs of the same kind as ONE launch (round 4: grouped launches; csrc/gemm_wide.hip, template parameter GRP).  The image and
 * the text tower are 12 blocks of the same four Linear layers (reference model/base/model.py:167-207, instantiated twice by CLIP.__init__,
 * :254-306): layer i of both runs as one persistent grid that walks the tiles of the longer-K problem first and continues into the
 * other's.  Both problems share `dtype`, the output kind and `epilogue` (the flags of cmh_linear_gemm / cmh_linear_gemm_fp8); each
 * brings its own pointers, shape and - CMH_FP8 - scales.  m_dev (optional, device int32): the real row count when M is an upper bound
 * (packed captions).  Every output element is computed exactly as by the single launch: identical bits.  Shapes the wide kernel cannot
 * take together (N % 256, M <= 2048 rows) run as two plain launches - the result never depends on the grouping. */
typedef struct cmh_gemm_problem {
  const void* x;          /* [M, K] dtype */
  const void* w;          /* [N, K] dtype */
  const float* bias;      /* [N] or NULL */
  const void* residual;   /* [M, N] f32 / fp16 (CMH_EPI_RES_F16) or NULL */
  void* out;              /* [M, N] */
  int32_t M, N, K;
  const int32_t* m_dev;   /* NULL, or the device word holding the real row count (<= M) */
  const float* colscale;  /* CMH_FP8: [N] weight scales */
  float alpha;            /* CMH_FP8: activation scale of x */
  float out_scale;        /* CMH_FP8 with CMH_EPI_OUT_FP8: out = e4m3(clamp(v / out_scale, +-448)), as cmh_linear_gemm_fp8; > 0 */
} cmh_gemm_problem;
int cmh_linear_gemm_grouped(int32_t dtype, const cmh_gemm_problem* a, const cmh_gemm_problem* b, int32_t epilogue, void* stream);
/* on = 0: grouped requests run as two plain launches (A/B measurements, the equality tests); 1 = grouped; -1 = environment
 * (CMH_GEMM_GROUPED=0 is off).  Process-wide, not thread-safe. */
int cmh_set_gemm_grouped(int32_t on);
/* softmax(q k^T / 8 [+causal] [+key padding]) v per head (head dim 64) on packed qkv [B*T, 3d] -> o [B*T, d]. */
int cmh_attention(int32_t dtype, const void* qkv, void* o, int32_t B, int32_t T, int32_t d, int32_t causal,
                  const uint8_t* key_padding_mask, void* stream);
/* Two attention problems (arguments as cmh_attention, each with its own B, T, d, causal flag and mask) as ONE launch: the lock-step
 * pair path's kernel, here for tests and benchmarks.  bf16, both T <= 80.  Returns CMH_OK when launched, 1 when there is no such
 * kernel for the pair (f32, T > 80, key-tile counts not instantiated, CMH_PAIR_KERNELS=0): nothing was launched and the caller
 * calls cmh_attention twice; < 0 on error.  Every output element has cmh_attention's bits. */
int cmh_attention_pair(int32_t dtype, const void* qkv0, void* o0, int32_t B0, int32_t T0, int32_t d0, int32_t causal0,
                       const uint8_t* key_padding_mask0, const void* qkv1, void* o1, int32_t B1, int32_t T1, int32_t d1,
                       int32_t causal1, const uint8_t* key_padding_mask1, void* stream);

/* Measurement hook (bench.py `roofline`): while enabled, every GEMM launch of the library is timed with a pair of HIP events
 * on the launch stream.  The two hand-written GEMM kernels launch through hipExtLaunchKernelGGL, which stamps the pair with the
 * dispatch's own begin / end - the duration rocprofv3's kernel trace reports; the 128 x 128 fallback kernels are bracketed by two
 * recorded events (CMH_GEMM_PROF_BRACKET=1: every launch, round 1-2's method, which adds the marker packets' gaps to each launch).
 * _end() synchronises on those events and returns the summed launch durations, the summed algorithmic FLOPs (2*M*N*K, real rows
 * only) and the launch count over ALL GEMM launches; _by_kernel() (after _end) splits the same sums by kernel:
 * [0] gemm_wide_kernel (N % 256 == 0: every large GEMM), [1] gemm_rows_kernel (M <= 512: the pooled-row tail), [2] the fallbacks.
 * Not thread-safe; single-stream benchmarking only. */
int cmh_prof_gemm_begin(int32_t max_launches);
int cmh_prof_gemm_end(double* total_ms, double* total_flops, int64_t* launches);
int cmh_prof_gemm_by_kernel(double* ms3, double* flops3, int64_t* launches3);
/* ... and (after _end) the share of the fused conv1 stem (cmh_set_conv1_fused: conv1_stem_kernel), which _end's sums include and the
 * three names of _by_kernel do not. */
int cmh_prof_gemm_conv1_fused(double* ms, double* flops, int64_t* launches);

/* Tuning overrides of the N % 256 == 0 GEMM kernel, for A/B measurements and for tests that must reach every variant:
 * tile_rows in {96, 128, 160} pins the tile height (-1: chosen per launch from M, N, K and the CU count); order_group picks the
 * tile order: -1 chosen per launch (the n-blocked order for N >= 1024: panel blocks outermost, so an XCD keeps its block of W in
 * its L2), 0 plain n-fastest, 1..64 n-panels per group inside each XCD's band (round 2), -2..-8 the n-blocked order with that many
 * blocks.  Results do not depend on either.
 * Process-wide, not thread-safe.  (No reference counterpart: upstream's GEMMs are ATen's, model/base/model.py:167-196.) */
int cmh_gemm_tuning(int32_t tile_rows, int32_t order_group);
/* GEMMs of few rows (M <= 512: the pooled-row tail of the towers, small heads) run on 64 x 64 tiles (csrc/gemm_rows.hip) instead of
 * the wide kernel's 96..160 x 256 ones: same bits per output element (same MFMA chain over K, same epilogue order), more workgroups.
 * on = 0 sends them to the wide kernel again (A/B, tests), 1 forces the default, -1 = environment (CMH_GEMM_ROWS=0 is off). */
int cmh_set_gemm_rows(int32_t on);
/* Round 5: the loader / consumer form of the N % 256 == 0 GEMM (csrc/gemm_lc.hip: four waves of a workgroup only stage operands by
 * LDS-DMA, the other four only multiply; 128 x 256 tiles; bf16 operands with 16-bit outputs and the forward epilogues of a transformer
 * block: bias, + QuickGELU, + fp16 residual; plain and grouped launches).  Same bits per output element as the wide kernel (same MFMA
 * chain over K, same epilogue order).  mode 0: never; 1, 2, 3: the 8-wave kernel for every launch it can take (the three differ only
 * in mode 2 leaving the QuickGELU launches to the wide kernel); 4: the 12-wave form (4 staging + 8 MFMA waves, stores deferred, 128-row
 * tiles) for every block launch with K >= 512, the wide kernel elsewhere; 7: the form on e4m3 operands (fp8 QKV launches);
 * 8: per bf16 launch without a residual, the 12-wave 160-row form where the host's cost model prices it below the wide kernel, the
 * wide kernel elsewhere (the 128-row form is never picked); 9: the 12-wave 160-row form for every block launch with K >= 512;
 * -1: the environment's CMH_GEMM_LC (default; unset = 8, CMH_GEMM_LC=0 = the wide kernel only).  Process-wide, not thread-safe. */
int cmh_set_gemm_lc(int32_t mode);
/* Which kernel the current cmh_set_gemm_lc mode gives a launch of operand type dt (CMH_BF16, ...) and epilogue flags epi:
 * Ma x Na x Ka alone (Mb = 0) or grouped with Mb x Nb x Kb.  0 the wide kernel, 1 the 8-wave loader / consumer kernel, 2 the
 * 12-wave 128-row form, 3 the 12-wave 160-row form.  Host-only: nothing is launched.  Returns -1 on a bad shape. */
int cmh_gemm_route(int32_t dt, int32_t Ma, int32_t Na, int32_t Ka, int32_t Mb, int32_t Nb, int32_t Kb, int32_t epi);
/* The whole plan of a GEMM request under the current switches, as the launch path itself computes it (csrc/gemm.hip: plan_gemm).
 * Host-only: nothing is launched, no GPU is needed (256 CUs are assumed without one).  dt: CMH_F32 / CMH_BF16 / CMH_FP8; epi: the
 * epilogue flags; a5 / b5: {M, N, K, device-side row count present (0 / 1), its hint (<= 0: none)} of the problem, b5 the second
 * problem of a grouped request or NULL.  out16: [0] launches - 1, or 2 when the grouped request runs as two plain launches, a then b;
 * [1] what cmh_gemm_route returns for the same shapes (the loader / consumer form of the route step alone: no row counts, before the
 * few-row kernel and the grouping decision); then 7 integers per launch ([2..8], and [9..15] for the second of two): kernel family
 * (0 gemm_wide_kernel, 1 gemm_rows_kernel, 2 the 128 x 128 fallback, 3 the 8-wave loader / consumer kernel, 4 its 12-wave 128-row
 * form, 5 its 12-wave 160-row form, 6 the 12-wave form on e4m3 operands), tile rows, grid (workgroups), tile-order group, deferred
 * QuickGELU (0 / 1), residual form (0 none, 1 first, 2 behind the bias), grouped (1: both problems in this launch).  Returns what the
 * launch would return for a bad shape or flag combination (operand pointers are not part of the plan). */
int cmh_gemm_plan(int32_t dt, int32_t epi, const int32_t* a5, const int32_t* b5, int32_t* out16);

/* encode_image / encode_text return one pooled row per sample (model/base/model.py:247-250, 366-370), and past the last block's
 * attention every operation is row-wise, so cmh_vit_encode / cmh_text_encode[_packed] carry only those B rows through the last
 * block's out_proj, ln_2 and MLP (bit-identical features, three GEMMs of M = B instead of M = B*T).  on = 0 switches that off
 * (A/B measurements, the equality test); also CMH_POOLED_TAIL=0 in the environment.  Process-wide, not thread-safe. */
int cmh_set_pooled_tail(int32_t on);

/* The image tower's stem in inference (cmh_vit_encode, cmh_clip_encode_pair[2], ...): conv1 (kernel = stride = patch, no bias;
 * model/base/model.py:215,231-235) runs as ONE implicit-GEMM launch (csrc/conv1_stem.hip) whose loader waves build the bf16 patch tile
 * from the f32 image, instead of a patch-matrix kernel followed by a GEMM.  Taken for bf16 conv1 (the bf16 and fp8 modes), patch 16 / 32
 * / 64, resolution % 4 == 0, width % 256 == 0; every other shape, the f32 mode and the training forward (whose
 * tape keeps the patch matrix for conv1's weight gradient) run the two launches.  Same bits either way.  on = 0 switches it off (A/B
 * measurements, the equality test), 1 on, -1 = environment (CMH_CONV1_FUSED=0 is off; default on).  Process-wide, not thread-safe. */
int cmh_set_conv1_fused(int32_t on);
/* conv1 alone, as the towers run it: patch_out [batch * g^2, width] f32 from image [batch_a, 3, R, R] f32 (+ image_b
 * [batch - batch_a, 3, R, R] when the batch comes as two tensors; NULL / batch_a ignored otherwise).  Only w's resolution, patch,
 * width, gemm_dtype and conv1_w are read.  keep_patches != 0: the caller wants the patch matrix [batch * g^2, K] (K = 3 patch^2, or
 * padded as the GEMMs need it) at the start of `scratch` - the two-launch stem; 0: the inference stem, fused where cmh_set_conv1_fused
 * allows, `scratch` then untouched.  scratch: 256-byte aligned, the patch matrix (+ a K-padded copy of the weight behind it). */
int cmh_vit_patch_embed(const cmh_vit_weights* w, const float* image, int32_t batch_a, const float* image_b, int32_t batch,
                        int32_t keep_patches, void* scratch, size_t scratch_bytes, float* patch_out, void* stream);

/* bf16 training mode: the residual-gradient stream between the blocks of a tower's backward pass (cmh_vit_backward[_part],
 * cmh_text_backward[_part], cmh_blocks_backward; reference: autograd through model/base/model.py:167-207) is carried as bf16 - the
 * copy the LayerNorm backward kernels leave as the next GEMMs' operand anyway - instead of f32 beside that copy: each LayerNorm
 * backward forms (new dx + stream) in f32 and rounds once.  on = 0 keeps the f32 stream (also CMH_GRAD_STREAM16=0); -1: the
 * environment (default on).  The f32 mode never uses it.  Process-wide, not thread-safe. */
int cmh_set_grad_stream16(int32_t on);

/* cmh_text_encode_tokens / cmh_text_forward_train_tokens with a key_padding_mask (the MITH trunk, model/MITH.py:120-144): positions
 * behind a caption's last unpadded token are never read by the reference's HashingModel (LocalizedTokenAggregation gives them weight
 * 0, model/MITH.py:349-376), so only the rows up to that position run through the tower; the projected tokens are written back to
 * their dense [B, L, E] places with ZEROS in the padded positions (the reference computes finite values there that nothing reads), the
 * EOT rows are dense indices as before.  Kept positions: the same bits as the dense path.  on = 0: every position is computed
 * (also CMH_TEXT_PACK_TOKENS=0); -1: the environment (default on).  Process-wide, not thread-safe. */
int cmh_set_text_token_packing(int32_t on);

/* ---------------------------------------------------------------------------------------------
 * fp8 encoder mode (CMH_FP8).  Mirrors the reference's precision hook convert_weights (model/base/model.py:391-412): the same
 * tensors it lowers to fp16 - Linear / MultiheadAttention weights - go to e4m3 here, with the activations that feed them.
 * ------------------------------------------------------------------------------------------- */
#define CMH_EPI_OUT_FP8 4096  /* cmh_linear_gemm_fp8: out is e4m3 of clamp(v / out_scale, +-448) */
#define CMH_FP8_MAX 448.0f

/* w f32 [N,K] -> w_fp8 e4m3 [N,K] and colscale f32 [N] = amax_k|w[n,k]| / 448 (1 for an all-zero row): w ~ w_fp8 * colscale[n]. */
int cmh_fp8_quantize_weight(const float* w, void* w_fp8, float* colscale, int32_t N, int32_t K, void* stream);
/* x (kind 0 f32 / 1 bf16 / 2 fp16, n % 4 == 0 elements) -> x_fp8 = e4m3(clamp(x / scale)); and back: out = f32(x_fp8) * scale. */
int cmh_fp8_quantize(const void* x, int32_t kind, void* x_fp8, int64_t n, float scale, void* stream);
int cmh_fp8_dequantize(const void* x_fp8, float* out, int64_t n, float scale, void* stream);
/* amax_inout[0] = max(amax_inout[0], max|x|) (device scalar, zero it first; a NaN in x reports +inf): calibration of the
 * per-tensor activation scales. */
int cmh_amax(const void* x, int32_t kind, int64_t n, float* amax_inout, void* stream);
/* out[M,N] = epi( alpha * colscale[n] * (x_fp8[M,K] . w_fp8[N,K]^T) ), N % 256 == 0, K % 128 == 0.  `epilogue` takes CMH_EPI_BIAS,
 * _QUICKGELU, _GELU, _RELU, _RESIDUAL (+ _RES_F16) and ONE of _OUT_BF16 / _OUT_F16 / _OUT_FP8 (default f32).  alpha = the
 * activation tensor's scale, colscale = cmh_fp8_quantize_weight's. */
int cmh_linear_gemm_fp8(const void* x_fp8, const void* w_fp8, const float* colscale, float alpha, const float* bias,
                        const float* residual, void* out, float out_scale, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                        void* stream);

/* DNpH quadratic spherical mutual information loss, reference train/DNpH_TMM/loss.py:5-72 `qmi_loss(images, texts, targets)` in
 * its default form (use_cosine, use_square_clamp, M = B^2 / sum(D)): img, txt f32 [B,K] hash outputs, labels bit-packed as by
 * cmh_pack_labels ([B, ceil(C/32)] u32) -> loss f32 [1] and sum_d f32 [1] (the number of label-sharing pairs, kept for the
 * backward).  Backward: dimg, dtxt f32 [B,K] = dloss[0] * d loss / d img, txt.  K <= 1024, C <= 512. */
size_t cmh_qmi_workspace_bytes(int32_t B);
int cmh_qmi_loss(const float* img, const float* txt, const uint32_t* labels_packed, int32_t B, int32_t K, int32_t C, float eps,
                 float* loss, float* sum_d, void* workspace, size_t workspace_bytes, void* stream);
int cmh_qmi_loss_backward(const float* img, const float* txt, const uint32_t* labels_packed, int32_t B, int32_t K, int32_t C,
                          float eps, const float* sum_d, const float* dloss, float* dimg, float* dtxt, void* workspace,
                          size_t workspace_bytes, void* stream);

/* DDBH base-point loss, reference train/DDBH/loss.py:5-101 `BPLoss.forward(u, v, y)` (the Python walk over the rows with its two
 * sorts and four host reads per row), for `calls` (1 .. 4) pairs (u[q], v[q]) of f32 [B,K] code matrices that share the f32 [B,C]
 * labels: u, v are HOST arrays of `calls` device pointers (u[q] == v[q] is the intra-modal call).  The six scalars are BPLoss's
 * attributes y_p, right, left, lowerBound, upperBound, percent (:8-13) -> loss f32 [calls], count i32 [calls] (active rows) and rows
 * [calls, B, 8] 32-bit words (per row: the f32 roundings of BP, BP_ds and the four offsets; the kept counts; kept for the backward).
 * Backward: du[q], dv[q] f32 [B,K] = dloss[q] * d loss[q] / d u[q], v[q] (two separate buffers even where u[q] == v[q]; their sum is
 * that tensor's gradient); it recomputes the inner products and reads no stored matrix.  B <= 8192, K <= 1024, any C >= 1. */
size_t cmh_ddbh_workspace_bytes(int32_t B);
int cmh_ddbh_bp_loss(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B, int32_t K, int32_t C,
                     double y_p, double right, double left, double lower_bound, double upper_bound, double percent, float* loss,
                     void* rows, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int cmh_ddbh_bp_loss_backward(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B, int32_t K,
                              int32_t C, double y_p, double right, double left, double lower_bound, double upper_bound,
                              double percent, const void* rows, const int32_t* count, const float* dloss, float* const* du,
                              float* const* dv, void* stream);
/* DDBH quantisation term, reference train/DDBH/hash_train.py:64-76 `matmul(s, (h - h.sign()).pow(2)).mean()` with s the float
 * indicator (y y^T > 0), for `calls` (1 .. 4) matrices h[q] f32 [B,K] (a HOST array of device pointers) -> loss f32 [calls] and
 * colsum f32 [B] (the column sums of s, kept for the backward).  Backward: dh[q] = dloss[q] * d loss[q] / d h[q]. */
int cmh_ddbh_quant_loss(const float* const* h, int32_t calls, const float* labels, int32_t B, int32_t K, int32_t C, float* loss,
                        float* colsum, void* workspace, size_t workspace_bytes, void* stream);
int cmh_ddbh_quant_loss_backward(const float* const* h, int32_t calls, const float* colsum, int32_t B, int32_t K, const float* dloss,
                                 float* const* dh, void* stream);

/* MSCH all-triplets margin loss, reference train/DPSIH/Loss.py:78-137 `Multi_Semantic_Correlation_Loss.forward(batch_inputs,
 * batch_labels, inputs)` (the [B, B, B] mask, the two gathers of its index vectors and the length read on the host, :105-137; the
 * three calls of a step, :61-62), for `calls` (1 .. 4) pairs (u[q], v[q]) of f32 [B,K] matrices over one f32 [B,C] label matrix:
 * u, v are HOST arrays of `calls` device pointers, u[q] == v[q] is the intra-modal call.  s = -n(u) n(v)^T with n the row normaliser
 * F.normalize (eps 1e-12) when `normalize` is set and the identity otherwise; positives share a label with the anchor and are not
 * the anchor's own column (the reference clears the diagonal of every square mask, :107), negatives share none; a triplet is active
 * when s_an - s_ap <= margin (mining 0, "all") or 0 < s_an - s_ap <= margin (mining 1, "semi-hard") -> loss f32 [calls] = the mean
 * of relu(s_ap - s_an + margin) over the active triplets (0 without any), count i64 [calls] = their number, sim f32 [calls,B,B] = s,
 * coef i32 [calls,B,B] = +(active negatives with a violation > 0) at a positive column, -(such positives) at a negative one, and with
 * `normalize` unit f32 [2 calls,B,K] / divisor f32 [2 calls,B]: the unit rows and norms of every distinct operand, in the slot of
 * its first appearance in u[0], v[0], u[1], ... (both may be NULL otherwise).  Backward, reference: autograd through :99-135:
 * du[q], dv[q] f32 [B,K] = dloss[q] * d loss[q] / d u[q], v[q] from coef, count and the unit rows; on an intra-modal call du[q]
 * holds the whole gradient and dv[q] is not written (it may be NULL).  1 <= B <= 1024, 1 <= K <= 128, any C >= 1; the workspace
 * holds cmh_msc_triplet_workspace_bytes(B) bytes (0 for a B out of range).  Integer counts, fixed-order sums, no atomics: two
 * calls give the same bits. */
size_t cmh_msc_triplet_workspace_bytes(int32_t B);
int cmh_msc_triplet_loss(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B, int32_t K, int32_t C,
                         float margin, int32_t mining, int32_t normalize, float* loss, int64_t* count, float* sim, int32_t* coef,
                         float* unit, float* divisor, void* workspace, size_t workspace_bytes, void* stream);
int cmh_msc_triplet_loss_backward(const float* const* u, const float* const* v, int32_t calls, int32_t B, int32_t K, int32_t normalize,
                                  const int32_t* coef, const int64_t* count, const float* unit, const float* divisor, const float* dloss,
                                  float* const* du, float* const* dv, void* stream);

/* DScPH proxy-fusion (CPF) loss with the step's quantisation term, reference train/DScPH/CPF_loss.py:24-54 `CPF.forward(image, text,
 * labels)` and train/DScPH/hash_train.py:64-70, both modalities in one call.  hi, ht f32 [B,K] head outputs, proxies f32 [C,K],
 * labels f32 [B,C] in {0, 1}; n(x) = x / max(|x|, 1e-12) per row; per modality c = n(h) n(proxies)^T, tp = 2 sum max(c, 0) Y + b,
 * lp = sum (1 - c) exp((1 - c) sp) Y, ln = sum_{c > tau} (c - psi) exp((c - mu) sn) (1 - Y) (the exponentials are constants of the
 * backward), L = 1 - tp / (tp + lp + ln); q = mean(sigma(z) (1 - sigma(z))) over z = n(h) (the reference's identity HouseHolder
 * rotation is z -> -z and the summand is even) -> terms f32 [4] = L_img, L_txt, q_img, q_txt, loss f32 [1] = L_img + L_txt +
 * quant_weight (q_img + q_txt), cos f32 [2,B,C] = the two cosine matrices the thresholds c >= 0 and c > tau were decided on (one
 * k-ascending f32 fmaf chain per element).  tape f32 [cmh_cpf_tape_bytes / 4], 8-byte aligned, or NULL for a forward alone: the six
 * f64 sums (tp, lp, ln per modality), the unit rows and the divisors.  Backward, reference: autograd through the same lines: from
 * labels, cos and the tape, d_hi, d_ht f32 [B,K] and d_proxies f32 [C,K] = dloss[0] * d loss / d hi, ht, proxies (d_proxies adds the
 * image rows in ascending order, then the text rows).  1 <= B <= 1024, 1 <= K <= 128, 1 <= C <= 1024; the workspace is 256-byte
 * aligned and holds cmh_cpf_workspace_bytes(B, K, C) bytes (0 for a shape out of range, as cmh_cpf_tape_bytes).  f64 sums in a fixed
 * order, no atomics: two calls give the same bits.  Launches: forward 5, backward 1. */
size_t cmh_cpf_workspace_bytes(int32_t B, int32_t K, int32_t C);
size_t cmh_cpf_tape_bytes(int32_t B, int32_t K, int32_t C);
int cmh_cpf_loss(const float* hi, const float* ht, const float* labels, const float* proxies, int32_t B, int32_t K, int32_t C, float tau,
                 float psi, float sp, float sn, float mu, float b, float quant_weight, float* terms, float* loss, float* cos,
                 float* tape, void* workspace, size_t workspace_bytes, void* stream);
int cmh_cpf_loss_backward(const float* labels, const float* cos, const float* tape, int32_t B, int32_t K, int32_t C, float tau, float sp,
                          float sn, float mu, float quant_weight, const float* dloss, float* d_hi, float* d_ht, float* d_proxies,
                          void* stream);

/* DDWSH: distance-weighted triplet sampling and the margin loss with per-class boundaries, for `pairs` (1 .. 3) pairs (u[q], v[q]) of
 * f32 [B,K] matrices over one f32 [B,C] label matrix in {0, 1}: u, v are HOST arrays of `pairs` device pointers, u[q] == v[q] is the
 * intra-modal call.  1 <= B <= 1024, 1 <= K <= 128, 1 <= C <= 1024; the workspace is 256-byte aligned and holds
 * cmh_dws_workspace_bytes(B, K, C) bytes (0 for a shape out of range).  f64 sums in a fixed order, no atomics, nothing read back: two
 * calls give the same bits.
 *
 * cmh_dws_distances, reference train/DDWSH/loss.py:17-20: dist f32 [pairs,B,B], D_ij = max(|n(u)_i - n(v)_j|, 1e-8) with n =
 * F.normalize (eps 1e-12), the squared difference summed as one k-ascending fmaf chain (the diagonal of an intra-modal pair is exactly
 * 1e-8); unit f32 [2 pairs,B,K] / divisor f32 [2 pairs,B]: the unit rows and norms of every distinct operand, in the slot of its first
 * appearance in u[0], v[0], u[1], ...
 *
 * cmh_dws_mine, reference train/DDWSH/loss.py:22, :52-72 `inverse_sphere_distances`, :75-79 `pdist`, :91-128
 * `DistanceWeightedMiner.__call__` (the host loop over the anchors, one row read back and two numpy draws per anchor).  space 0
 * ("distances", what the reference runs): M_ij = max(sqrt(max(|D_i: - D_j:|^2, 1e-4)), cutoff), the B terms summed in f64, dim = B;
 * space 1 ("embeddings", the paper's): M = max(D, cutoff), dim = K.  Anchor i is used when it has another positive (an item sharing a label) and not every item is
 * one; log w_j = (2 - dim) log M_ij - ((dim - 3) / 2) log max(1 - M_ij^2 / 4, 1e-8) in f64, 0 on the positives before the maximum is
 * taken, w = exp(log w - max), 0 on the positives.  uniforms f32 [pairs,B,2] in [0, 1) = (u_p, u_n) per anchor: the negative is the
 * first j whose ascending-index running sum of w exceeds u_n times the total (an item of weight 0 is never picked), the positive the
 * floor(u_p n)-th of the n other positives in index order -> triplets i32 [pairs,B,2] = (positive, negative), (-1, -1) for an anchor
 * that is not used; weights f64 [pairs,B,B] = w (zero rows for such anchors), or NULL.
 *
 * cmh_dws_margin_loss, reference train/DDWSH/loss.py:28-49: beta f32 [C]; beta_i = sum_c Y_ic beta_c / sum_c Y_ic, pos_i =
 * relu((D[i,p_i] - beta_i) + margin), neg_i = relu((beta_i - D[i,n_i]) + margin) -> count i64 [pairs] = the anchors with pos_i > 0 or
 * neg_i > 0, loss f32 [pairs] = sum (pos + neg) / count (0 without any), tape f32 [pairs,B,4] = beta_i, [pos_i > 0], [neg_i > 0],
 * sum_c Y_ic.  The triplets may be cmh_dws_mine's or handed in; an entry outside [0, B) skips its anchor.
 *
 * cmh_dws_margin_loss_backward, reference: autograd through train/DDWSH/loss.py:17-47: du[q], dv[q] f32 [B,K] and dbeta f32 [C] =
 * sum_q dloss[q] * d loss[q] / d u[q], v[q], beta (no gradient through an entry of D at its clamp); on an intra-modal pair du[q] holds
 * the whole gradient and dv[q] is not written (it may be NULL).  Launches for three pairs: distances 3, mine 3 (space 1: 2), loss 2,
 * backward 2. */
size_t cmh_dws_workspace_bytes(int32_t B, int32_t K, int32_t C);
int cmh_dws_distances(const float* const* u, const float* const* v, int32_t pairs, int32_t B, int32_t K, float* dist, float* unit,
                      float* divisor, void* stream);
int cmh_dws_mine(const float* dist, int32_t pairs, const float* labels, int32_t B, int32_t K, int32_t C, float cutoff, int32_t space,
                 const float* uniforms, int32_t* triplets, double* weights, void* workspace, size_t workspace_bytes, void* stream);
int cmh_dws_margin_loss(const float* dist, const int32_t* triplets, int32_t pairs, const float* labels, const float* beta, int32_t B,
                        int32_t C, float margin, float* loss, int64_t* count, float* tape, void* workspace, size_t workspace_bytes,
                        void* stream);
int cmh_dws_margin_loss_backward(const float* const* u, const float* const* v, int32_t pairs, const float* labels, int32_t B, int32_t K,
                                 int32_t C, const float* dist, const int32_t* triplets, const float* tape, const int64_t* count,
                                 const float* unit, const float* divisor, const float* dloss, float* const* du, float* const* dv,
                                 float* dbeta, void* stream);

/* DJSRH joint-semantics target and reconstruction loss (Su, Zhong, Zhang: Deep Joint-Semantics Reconstructing Hashing, ICCV 2019;
 * no upstream counterpart), label-free.  n(x) = x / max(|x|, 1e-12) per row.  1 <= B <= 1024, 1 <= K <= 128, 1 <= D <= 4096; every
 * workspace is 256-byte aligned and holds cmh_djsrh_workspace_bytes(B, K, D) bytes (0 for a shape out of range).
 * Target: fi, ft f32 [B,D] the stock towers' features of the batch -> S f32 [B,B] =
 * mu ((1 - eta) St + (eta / B) St St^T) with St = beta (2 n(fi) n(fi)^T - 1) + (1 - beta) (2 n(ft) n(ft)^T - 1); symmetric bit for bit.
 * Loss: hi, ht f32 [B,K] the heads' outputs, b = n(h) -> terms f32 [3] = the means of (b_I b_I^T - S)^2, (b_I b_T^T - S)^2,
 * (b_T b_T^T - S)^2 and loss f32 [1] = lambda1 terms[0] + terms[1] + lambda2 terms[2]; tape (NULL: nothing is kept) f32
 * [2B + 3 B^2] receives the row norms of hi and ht and the three residual matrices.  Backward: d_hi, d_ht f32 [B,K] = dloss[0] *
 * d loss / d hi, ht from the tape (it takes S as symmetric, as the target is; S and the features get no gradient).  f32 sums in a
 * fixed order, no atomics: two calls give the same bits. */
size_t cmh_djsrh_workspace_bytes(int32_t B, int32_t K, int32_t D);
int cmh_djsrh_target(const float* fi, const float* ft, int32_t B, int32_t D, float beta, float eta, float mu, float* S, void* workspace,
                     size_t workspace_bytes, void* stream);
int cmh_djsrh_loss(const float* hi, const float* ht, const float* S, int32_t B, int32_t K, float lambda1, float lambda2, float* terms,
                   float* loss, float* tape, void* workspace, size_t workspace_bytes, void* stream);
int cmh_djsrh_loss_backward(const float* hi, const float* ht, const float* tape, int32_t B, int32_t K, float lambda1, float lambda2,
                            const float* dloss, float* d_hi, float* d_ht, void* workspace, size_t workspace_bytes, void* stream);

/* DMsH-LN multi-similarity loss, reference train/DMsH_LN/MSLOSS.py:13-55 `MultiSimilarityLoss.forward(feats, labels, feat2)` in the
 * branch its trainer takes (train/DMsH_LN/hash_train.py:58-60; not the "cifar10-1" branch): feats (and feat2, NULL = feats) f32
 * [B,K] hash outputs, labels f32 [B,Kl] = the LabelNet codes (two samples are similar when their codes' dot product is > 0)
 * -> loss f32 [1]; thresh 0.5, margin 0.1, scales 2 / 40 as the reference fixes them.  Backward: dfeats (and dfeat2 when feat2 is
 * given; with feat2 = NULL both roles' gradients are summed into dfeats) = dloss[0] (NULL: 1) * d loss / d feats; it recomputes
 * the forward's statistics, so the workspace need not be kept between the two calls.  B <= 8192 (the global batch under data parallelism: B * 4 bytes of
 * dynamic LDS per backward launch, two [B, B] f32 matrices of workspace), K, Kl <= 1024. */
size_t cmh_msl_workspace_bytes(int32_t B);
int cmh_msl_loss(const float* feats, const float* feat2, const float* labels, int32_t B, int32_t K, int32_t Kl, float* loss,
                 void* workspace, size_t workspace_bytes, void* stream);
int cmh_msl_loss_backward(const float* feats, const float* feat2, const float* labels, int32_t B, int32_t K, int32_t Kl,
                          const float* dloss, float* dfeats, float* dfeat2, void* workspace, size_t workspace_bytes, void* stream);

/* DHaPH self-paced contrastive loss, reference train/DHaPH/MSLoss.py:13-33 `MSLoss.forward(image_feature, text_feature, labels,
 * epoch)`: a (and b, NULL = a: the image-image / text-text calls of train/DHaPH/hash_train.py:68-69) f32 [B,K] hash outputs, labels
 * f32 [B,C] multi-hot -> loss f32 [1] = mean_i -log(P_i / (P_i + N_i)) over exp(cos / temperature) of the label-sharing / other
 * pairs, with the detached self-paced weights exp(-1 - cos)^(delta/4) / exp(-1 + cos)^delta; delta in [0, 1] is what :23-27 derive
 * from (epoch, totalepoch) (0 = self_paced off).  Backward: da (and db; with b = NULL both roles' gradients are summed into da) =
 * dloss[0] (NULL: 1) * d loss / d a; it recomputes the forward's statistics.  B <= 8192 (as above), K, C <= 1024. */
size_t cmh_spl_workspace_bytes(int32_t B);
int cmh_spl_loss(const float* a, const float* b, const float* labels, int32_t B, int32_t K, int32_t C, float temperature, float delta,
                 float* loss, void* workspace, size_t workspace_bytes, void* stream);
int cmh_spl_loss_backward(const float* a, const float* b, const float* labels, int32_t B, int32_t K, int32_t C, float temperature,
                          float delta, const float* dloss, float* da, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* f32 -> bf16 (round-to-nearest-even) copy used to prepare CMH_BF16 GEMM weights. */
int cmh_cast_f32_to_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hash heads and code generation.
 * ------------------------------------------------------------------------------------------- */
typedef enum cmh_act { CMH_ACT_NONE = 0, CMH_ACT_TANH = 1, CMH_ACT_RELU = 2 } cmh_act;

/* y[M,N] = act( scale_mask ? (x W^T + b) * drop_mask/(1-p) : x W^T + b ), all f32.
 * Replaces LinearHash.forward (model/modelbase.py:25-35: fc -> dropout(0.2) -> tanh; drop_mask
 * NULL = eval), HashLayer.fc (model/DCHMT.py:13,20-21), Pre_Layer (model/DNPH_TOMM.py:7-14).
 * drop_mask: optional f32 [M,N] of {0,1}; keep_scale = 1/(1-p). */
int cmh_linear_act(const float* x, const float* w, const float* b, const float* drop_mask,
                   float keep_scale, int32_t act, float* y, int32_t M, int32_t N, int32_t K,
                   void* stream);

/* DCHMT select head: softmax over each adjacent pair of z[M, 2K] -> p[M, 2K]
 * (model/DCHMT.py:24 torch.softmax(item(embed), -1) for the K two-way Linears, concatenated as the
 * trainer does at train/DCHMT/hash_train.py:55-57). */
int cmh_pair_softmax(const float* z, float* p, int32_t M, int32_t K, void* stream);

/* codes = sign(h) in {-1,0,+1} f32 (train/base.py:141-143 torch.sign). */
int cmh_sign_codes(const float* h, float* codes, int64_t n, void* stream);

/* codes[M,K] from pair probabilities p[M,2K]: argmax of the pair, index 0 -> -1, 1 -> +1, tie -> -1
 * (train/base.py:150-158 make_hash_code_DCHMT). */
int cmh_pair_argmax_codes(const float* p, float* codes, int32_t M, int32_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hamming ranking / mAP  (reference utils/calc_utils.py).
 * Codes are packed to two bit-planes of W = ceil(K/32) u32 words per code:
 *   sign plane bit t = (code[t] > 0), nz plane bit t = (code[t] != 0).
 * Labels are packed to ceil(C/32) u32 words, bit c = (label[c] != 0).
 * ------------------------------------------------------------------------------------------- */
/* bad_flag (device i32, caller zeroes it) is set to 1 if any code is not exactly -1, 0 or +1. */
int cmh_pack_codes(const float* codes, int64_t n, int32_t bits, uint32_t* sign_plane,
                   uint32_t* nz_plane, int32_t* bad_flag, void* stream);
/* The inverse of cmh_pack_codes: codes f32 [n, bits] in {-1, 0, +1} from the two bit planes.  Data-parallel evaluation exchanges the
 * PLANES (16 bytes per 64-bit code pair instead of 512 bytes of floats: SURVEY 8e "all-gather packed DB codes") and restores the
 * reference's float code matrices (train/base.py:130-148 img_buffer / text_buffer) on every rank with this call. */
int cmh_unpack_codes(const uint32_t* sign_plane, const uint32_t* nz_plane, int64_t n, int32_t bits, float* codes, void* stream);
/* bad_flag set if any label is negative or NaN (the reference's `L.L^T > 0` test then stops
 * being an intersection test). */
int cmh_pack_labels(const float* labels, int64_t n, int32_t classes, uint32_t* packed,
                    int32_t* bad_flag, void* stream);

/* calc_hammingDist (utils/calc_utils.py:8-13): dist[Q,N] f32 = 0.5*(K - q.r), exact for codes in
 * {-1,0,+1}, computed by AND/XOR + popcount on the packed planes. */
int cmh_hamming_dist(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign,
                     const uint32_t* r_nz, int32_t Q, int64_t N, int32_t bits, float* dist,
                     void* stream);

/* calc_neighbor (utils/calc_utils.py:42-45): sim[A,B] f32 = (la . lb^T > 0). */
int cmh_calc_neighbor(const uint32_t* la, const uint32_t* lb, int32_t A, int32_t B, int32_t classes,
                      float* sim, void* stream);

typedef enum cmh_tie_order {
  CMH_TIE_REFERENCE = 0,    /* torch.sort(stable=False) on CPU == libstdc++ introsort order */
  CMH_TIE_STABLE = 1        /* ties by ascending database index (torch.sort(stable=True)): LSD radix sort, ~4x faster */
} cmh_tie_order;

size_t cmh_map_workspace_bytes(int32_t Q, int64_t N, int32_t bits, int32_t tie_order);

/* calc_map_k_matrix (utils/calc_utils.py:16-39).  topk <= 0 means k = N (the reference's k=None).
 *   ap[Q]   f32  per-query AP (0 for queries with no relevant item; they still count in the mean)
 *   map[1]  f32  sum(ap)/Q accumulated in f32 in query order like the reference's `map += ...`
 *   perm    optional i32 [Q,N]: the full ranking `ind` (utils/calc_utils.py:31) per query
 * depth_limit_override < 0 : libstdc++'s 2*floor(log2 N); >= 0 forces the introsort depth limit
 * (test hook for the heapsort fallback). */
int cmh_hamming_map(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label,
                    const uint32_t* r_sign, const uint32_t* r_nz, const uint32_t* r_label,
                    int32_t Q, int64_t N, int32_t bits, int32_t classes, int64_t topk,
                    int32_t tie_order, int32_t depth_limit_override, float* ap, float* map,
                    int32_t* perm, void* workspace, size_t workspace_bytes, void* stream);
/* map[1] = (((ap[0] + ap[1]) + ...) / Q), f32, in query order: the mean cmh_hamming_map itself appends, exposed for per-query APs
 * that were computed on query shards by several ranks and gathered (utils/calc_utils.py:37-38 `map += AP`; `map / num_query`). */
int cmh_map_mean(const float* ap, int32_t Q, float* map, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Retrieval on the same packed operands (csrc/retrieval.hip): what the reference leaves to an offline step on the
 * .mat files under PR_cruve/ of train/base.py::save_mat. Distances are calc_hammingDist's (utils/calc_utils.py:8-13) in half-units
 * h = K - q.r, 0 <= h <= 2K; relevance is calc_neighbor's test (:42-45).  Labels are optional: pass both label pointers or
 * neither (classes is then ignored).  Q <= 65535, N <= 524287, bits <= 2048, classes <= 2048.
 * ------------------------------------------------------------------------------------------- */
#define CMH_TOPK_MAX 524287   /* largest k of cmh_hamming_topk: the select keeps no list of k entries, so it is the largest N */
size_t cmh_retrieval_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
/* counts u32 [Q, 2K+1, 2]: counts[i, h, 1] = database items at half-distance h from query i that share a label with it,
 * counts[i, h, 0] = the others (all of them without labels): precision / recall by Hamming radius, tie-free. */
int cmh_hamming_hist(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                     const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                     uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* The k nearest database items of EVERY query (also of one without relevant items, which cmh_hamming_map skips), ordered by
 * (distance, database index): the first k columns of torch.sort(calc_hammingDist(q, r), stable=True) and of the CMH_TIE_STABLE
 * ranking.  1 <= k <= min(N, CMH_TOPK_MAX).  idx i32 [Q, k]; dist f32 [Q, k] = 0.5 * h exactly; rel u8 [Q, k] (optional, needs
 * labels) = the item is relevant; counts (optional) as cmh_hamming_hist. */
int cmh_hamming_topk(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                     const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                     int64_t k, int32_t* idx, float* dist, uint8_t* rel, uint32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Graded relevance: the grade of a pair is the NUMBER of labels it shares, popcount(label_q & label_r) = the entry of
 * label1.matmul(label2.T) that calc_neighbor (:42-45) thresholds; NDCG@n, ACG@n and WAP@n are sums over it.  A grade is one byte:
 * both entry points take classes <= 255 and refuse more.  Label bits at or above `classes` are zero (cmh_pack_labels writes them so).
 *
 * cmh_hamming_topk with grade u8 [Q, k] = the grade of every neighbour (saturated at 255).  Labels and grade are required; idx and
 * dist are cmh_hamming_topk's bit for bit, rel (optional) == grade > 0, counts (optional) as cmh_hamming_hist.  Workspace:
 * cmh_retrieval_workspace_bytes. */
int cmh_hamming_topk_graded(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                            const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                            int64_t k, int32_t* idx, float* dist, uint8_t* rel, uint8_t* grade, uint32_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream);
/* grade_counts u32 [Q, classes+1]: grade_counts[i, g] = database items that share exactly g labels with query i (every row sums to
 * N; N - grade_counts[i, 0] = the query's relevant items).  It depends on the labels only, so one call serves every direction of
 * an evaluation; the ideal DCG of a query follows from its row without sorting.  Written once, deterministic.  Workspace: its own
 * query below (cmh_retrieval_workspace_bytes is sized by the code length, which this pass does not have). */
size_t cmh_label_overlap_workspace_bytes(int32_t Q, int64_t N, int32_t classes);
int cmh_label_overlap_hist(const uint32_t* q_label, const uint32_t* r_label, int32_t Q, int64_t N, int32_t classes,
                           uint32_t* grade_counts, void* workspace, size_t workspace_bytes, void* stream);
/* mAP by counting: cmh_hamming_map's AP with CMH_TIE_STABLE ties, without a ranking.  For a relevant item j at half-distance h,
 *   rank(j) = #{items at h' < h} + #{items at h with index < j} + 1,  relrank(j) = the same counts over the relevant items + 1,
 *   AP = (1 / total) * sum over the relevant j with relrank(j) <= total of relrank(j) / rank(j),  total = min(k, R)
 * (utils/calc_utils.py:26-38 `count / tindex` term by term: every term the f32 quotient of the two f32 numbers, summed in float64).
 * The database of one call may be ONE SHARD of a larger one whose shards are taken in ascending index order:
 *   total_counts u32 [Q, 2K+1, 2]  cmh_hamming_hist's histogram of the whole database; null = this call's own (a single shard)
 *   prior_counts u32 [Q, 2K+1, 2]  the histogram of the shards before this one; null = zeros
 *   counts_out   u32 [Q, 2K+1, 2]  optional: this shard's histogram
 *   ap_sum       f64 [Q]           this shard's sum of relrank / rank: written, not accumulated.  The sums of the shards add.
 * topk <= 0 means k = the size of the whole database.  Labels are required.  Q <= 65535, N <= 524287 per call as above; refused
 * with -1 before any launch: null operands, sizes outside the limits, a workspace below cmh_map_count_workspace_bytes (0 outside
 * the limits).  Every output word is written once: two calls give equal bits. */
size_t cmh_map_count_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_hamming_ap_partial(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                           const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                           int64_t topk, const uint32_t* total_counts, const uint32_t* prior_counts, uint32_t* counts_out,
                           double* ap_sum, void* workspace, size_t workspace_bytes, void* stream);
/* ap f32 [Q] = ap_sum / min(k, R) in float64, rounded once (0 where R = 0; R = the relevant items of total_counts);
 * map f32 [1] = the mean over all Q queries as cmh_map_mean forms it.  Any Q >= 1. */
int cmh_ap_finish(const double* ap_sum, const uint32_t* total_counts, int32_t Q, int32_t bits, int64_t topk, float* ap, float* map,
                  void* stream);
/* Radius search: EVERY database item at half-distance h <= radius_h from a query (its Hamming ball), as a ragged list per query in
 * the order (distance, database index): bit for bit the first ball(q) columns of cmh_hamming_topk.  The caller sizes the lists from
 * cmh_hamming_hist (ball(q) = the items of its bins 0..radius_h) and passes where each starts:
 *   row_off      i64 [Q]           start of query q's list in idx / dist / rel (an exclusive prefix sum of the balls, or any other
 *                                  layout in which the rows [row_off[q], row_off[q] + ball(q)) are disjoint)
 *   total_counts u32 [Q, 2K+1, 2]  cmh_hamming_hist's histogram of the whole database; null = this call's own (a single shard)
 *   prior_counts u32 [Q, 2K+1, 2]  the histogram of the shards before this one; null = zeros
 *   idx_base     added to every index written: the database row at which this call's shard starts (idx_base + N <= 2^31 - 1)
 *   counts_out   u32 [Q, 2K+1, 2]  optional: this shard's histogram
 * An item j of this call at h <= radius_h is written, once, at
 *   row_off[q] + #{items of total at h' < h} + prior[q, h] + #{items of this call at h with index < j}
 * with idx = idx_base + j, dist = 0.5 * h exactly and rel (optional, needs labels) = the item is relevant.  Shards taken in ascending
 * index order therefore fill one set of buffers with the list of the whole database.  Nothing outside a query's rows is touched
 * (a position at or behind the ball of total_counts is dropped), there are no atomics on the outputs, two calls give equal bits.
 * 0 <= radius_h <= 2 * bits.  Q <= 65535, N <= 524287 per call as above; refused with -1 before any launch: null operands, labels on
 * one side only, rel without labels, radius_h or sizes outside the limits, a workspace below cmh_range_workspace_bytes (0 outside
 * the limits). */
size_t cmh_range_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_hamming_range(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                      const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                      int32_t radius_h, const uint32_t* total_counts, const uint32_t* prior_counts, const int64_t* row_off,
                      int32_t idx_base, int32_t* idx, float* dist, uint8_t* rel, uint32_t* counts_out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Ranks of given targets by counting (instance-level recall: Recall@K, MedR, MRR over paired items).  The 0-based position of
 * database item t in the stable ranking of query q (its column in cmh_hamming_topk's row) is
 *   #{j : h(q, j) < h(q, t)} + #{j < t : h(q, j) = h(q, t)},
 * so one walk over the database gives it: no list, no sort.  It replaces cmh_hamming_topk with k = N followed by a search of the
 * [Q, N] index matrix for the target (8 bytes per pair, k <= CMH_TOPK_MAX, no sum over shards).  Every query has G target slots:
 *   t_sign, t_nz u32 [Q*G, W]  the packed planes of the targets (W = ceil(bits / 32)): slot g of query q is row q * G + g
 *   bound        i32 [Q*G]     0..N: database items with index < bound count as "before" among the ties (the target's own index
 *                              in this call's database; for one shard [a, b) of a larger database clamp(t - a, 0, b - a));
 *                              -1: the slot has no target, its planes are not read and its three outputs are 0
 *   out          i32 [Q, G, 3] (less, ties_before, ties): items at a smaller half-distance than the target, items at the target's
 *                              half-distance with index < bound, items at the target's half-distance (the target itself included
 *                              when it lies in this call's database).  The counts of the shards of a database add.
 * 1 <= G <= 8; Q <= 65535, N <= 524287, bits <= 2048 per call as above.  Refused with a negative status before any launch: null
 * operands, sizes outside the limits, a workspace below cmh_rank_workspace_bytes (0 outside the limits).  Every output word is
 * written once, without atomics: two calls give equal bits. */
size_t cmh_rank_workspace_bytes(int32_t Q, int64_t N, int32_t bits, int32_t G);
int cmh_hamming_rank(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q, int64_t N,
                     int32_t bits, const uint32_t* t_sign, const uint32_t* t_nz, const int32_t* bound, int32_t G, int32_t* out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* A database larger than N <= 524287 is searched as shards (utils/retrieval.py: row slices of the packed planes, each within the
 * limits above) and the per-shard lists are folded together in ascending shard order (csrc/retrieval_merge.hip); the result is bit
 * for bit the list of one cmh_hamming_topk over the whole database, i.e. of torch.sort(calc_hammingDist(q, r), stable=True).
 *
 * Two top-k lists of the same queries -> the first k entries of their union in the order of cmh_hamming_topk.
 * Every row of a and of b is ascending by (dist, idx).  The caller guarantees that every index of b (after b_base is added)
 * is larger than every index of a, so "a before b at equal distance" IS ascending database index.
 * idx[q, :] / dist[q, :] / tag[q, :] = the first k of merge(a[q, :], b[q, :]); b's indices come out as b_idx + b_base.
 * tag = the hit flag or the grade that travels with an entry: a_tag, b_tag and tag are all given or all null.
 * 1 <= ka, 1 <= kb, 1 <= k <= ka + kb, 1 <= Q <= 65535 (as the searches that make the lists: more queries go in blocks);
 * outputs must not alias inputs.  No workspace. */
int cmh_topk_merge(const int32_t* a_idx, const float* a_dist, const uint8_t* a_tag, int32_t ka,
                   const int32_t* b_idx, const float* b_dist, const uint8_t* b_tag, int32_t kb, int32_t b_base,
                   int32_t Q, int32_t k, int32_t* idx, float* dist, uint8_t* tag, void* stream);

/* Few queries against a database of any size (csrc/retrieval_few.hip): the interactive case, one caption or one image against an
 * index.  The entry points above let lanes own queries (64 per wave: with one query 63 lanes repeat it); here lanes own items, the
 * query words are wave-uniform, and one call takes any database up to 2^31 - 1 items: no shards, no merge.
 *   idx i32 [Q, k], dist f32 [Q, k] = 0.5 * h exactly: row q holds the first k columns of torch.sort(calc_hammingDist(q, r),
 *   stable=True), ordered by (distance, ascending database index): for N <= 524287 bit for bit what cmh_hamming_topk writes, beyond
 *   that what the fold of its per-shard lists through cmh_topk_merge gives.
 * 1 <= Q <= CMH_FEW_Q_MAX (one tile of the entry points above: beyond it their lanes are full), 1 <= N <= 2^31 - 1,
 * 1 <= bits <= CMH_FEW_BITS_MAX, 1 <= k <= min(N, CMH_FEW_K_MAX) (a result page, not a ranking).  No labels: the caller gathers
 * the k results' label words.  Database planes of 2 (4) words per row are read as 8 (16) bytes: aligned so (rows of a 256-byte
 * aligned buffer are).  Refused with -1 before any launch: null operands, sizes outside the limits, misaligned planes; -2: a
 * workspace below cmh_topk_few_workspace_bytes (0 outside the limits).  No atomics on idx / dist, every element is written once: two
 * calls give equal bits, on any stream. */
#define CMH_FEW_Q_MAX 64
#define CMH_FEW_K_MAX 4096
#define CMH_FEW_BITS_MAX 128
size_t cmh_topk_few_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_hamming_topk_few(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q, int64_t N,
                         int32_t bits, int32_t k, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream);

/* Soft-query search (csrc/retrieval_soft.hip): few queries given as the head's REAL-VALUED output u (before sign() / the pair
 * argmax) against the packed database.  calc_hammingDist = 0.5 (K - q . r) evaluated on u instead of its sign: an unsure bit costs
 * little when it disagrees, a confident one a lot, which orders the items a Hamming ranking leaves tied.  Nothing is stored per
 * item: the database is cmh_pack_codes' planes.
 * cmh_soft_query_planes quantises: per row s = max_i |u_i|; s == 0: every weight 0; else w_i = rint((u_i / s) * 15), three f32
 * operations, each rounded once (IEEE division, IEEE multiplication, round half to even), so w_i in [-CMH_SOFT_LEVELS,
 * CMH_SOFT_LEVELS].
 *   u f32 [Q, bits] -> q_sign u32 [Q, W] (bit i set: w_i > 0), q_mag u32 [Q, 4, W] (plane b = bit b of |w_i|; zero at and behind
 *   `bits`), wsum i32 [Q] = sum |w_i|, scale f32 [Q] = s; W = ceil(bits / 32).  *bad (i32, the caller zeroes it) is set when an entry
 *   is not finite; that row's weights, wsum and scale are then 0.  1 <= Q <= 65535, 1 <= bits <= CMH_SOFT_BITS_MAX.
 * cmh_soft_topk ranks: for an item r in {-1, 0, +1}^bits
 *   wdist(u, r) = sum |w_i| - sum w_i r_i = sum_{r_i = 0} |w_i| + 2 sum_{r_i != 0, sign differs} |w_i|,
 *   an integer in [0, 2 wsum]; (scale / 30) * wdist = 0.5 (sum |u~_i| - u~ . r) for the quantised query u~ = (s / 15) w: the
 *   reference's distance on u~ minus the per-query constant 0.5 (bits - sum |u~_i|).  A query with every |w_i| = 15 gives
 *   wdist = 15 h, h the half-units of cmh_hamming_topk_few; a zero weight takes its bit out of the distance.
 *   idx i32 [Q, k], wdist i32 [Q, k]: row q holds the first k database items in ascending (wdist, database index).  The q_mag
 *   words are cut to `bits` bits in the kernel: what the database planes hold behind `bits` is never counted.
 * Limits and refusals as cmh_hamming_topk_few: 1 <= Q <= CMH_SOFT_Q_MAX, 1 <= N <= 2^31 - 1 in one call, 1 <= bits <=
 * CMH_SOFT_BITS_MAX, 1 <= k <= min(N, CMH_SOFT_K_MAX); database rows of 2 (4) words are read as 8 (16) bytes: aligned so.  -1 before
 * any launch: null operands, sizes outside the limits, misaligned planes; -2: a workspace below cmh_soft_topk_workspace_bytes
 * (0 outside the limits).  The stable counting sort of cmh_hamming_topk_few over 30 bits + 1 bins: exact, no atomics on idx /
 * wdist, every element written once: two calls give equal bits, on any stream. */
#define CMH_SOFT_LEVELS 15
#define CMH_SOFT_Q_MAX 64
#define CMH_SOFT_K_MAX 4096
#define CMH_SOFT_BITS_MAX 128
int cmh_soft_query_planes(const float* u, int32_t Q, int32_t bits, uint32_t* q_sign, uint32_t* q_mag, int32_t* wsum, float* scale,
                          int32_t* bad, void* stream);
size_t cmh_soft_topk_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_soft_topk(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q, int64_t N,
                  int32_t bits, int32_t k, int32_t* idx, int32_t* wdist, void* workspace, size_t workspace_bytes, void* stream);

/* Filtered search: the two searches above over only the items an ALLOW-MASK admits (the nearest items among those that carry a
 * label, are not in a deny list, lie in an id range ...), without a packed copy of the admitted rows.
 *   allow u64 [ceil(N / 64)], 8-byte aligned, on the GPU: bit j % 64 of word j / 64 set = database item j is admitted.  Bits at
 *   and behind N in the last word may hold anything: they are never read as admitted.
 * cmh_hamming_topk_few_masked / cmh_soft_topk_masked: operands, limits and refusals of cmh_hamming_topk_few / cmh_soft_topk.  k is
 * checked against N, not against the number A of admitted items (it lives on the device; the call does not synchronise):
 *   row q of idx / dist (wdist) holds the first min(k, A) ADMITTED items in ascending (distance, database index); the indices are
 *   database indices, not positions in the subset: bit for bit what the unmasked call gives on a database of the admitted rows
 *   alone, mapped back.  found i32 [Q] = min(k, A).  The columns at and behind found[q] hold idx = -1 and dist = +inf (wdist =
 *   INT32_MAX).
 * Every element of idx, dist and found is written exactly once by some kernel of the call, without atomics: two calls give equal
 * bytes, on any stream.  -1 before any launch: a null or misaligned allow, a null found, and everything the unmasked call refuses;
 * -2: a workspace below cmh_topk_few_masked_workspace_bytes / cmh_soft_topk_masked_workspace_bytes (0 outside the limits; the
 * unmasked calls' sizes). */
size_t cmh_topk_few_masked_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_hamming_topk_few_masked(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz,
                                const uint64_t* allow, int32_t Q, int64_t N, int32_t bits, int32_t k, int32_t* idx, float* dist,
                                int32_t* found, void* workspace, size_t workspace_bytes, void* stream);
size_t cmh_soft_topk_masked_workspace_bytes(int32_t Q, int64_t N, int32_t bits);
int cmh_soft_topk_masked(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz,
                         const uint64_t* allow, int32_t Q, int64_t N, int32_t bits, int32_t k, int32_t* idx, int32_t* wdist,
                         int32_t* found, void* workspace, size_t workspace_bytes, void* stream);
/* mAP, relevant counts and rank sums of soft queries over the WHOLE database, by counting (csrc/retrieval_soft.hip).
 * Distance, quantiser and planes are cmh_soft_topk's; the ranking is by (wdist, database index) ascending; item j is relevant to
 * query q iff (q_lab[q] & r_lab[j]) != 0 on cmh_pack_labels' words (q_lab u32 [Q, label_words], r_lab u32 [N, label_words]).
 *   rank(j)    = #{items with wdist < wdist(j)} + #{items with equal wdist and index < j} + 1
 *   relrank(j) = the same two counts over the relevant items + 1
 *   relevant i32 [Q] = R, the number of relevant items; total = min(k, R), k = 0 meaning N
 *   ap f32 [Q]       = (1 / total) sum over the relevant j with relrank(j) <= total of relrank(j) / rank(j); 0 when R = 0.  Every term
 *                      is the f32 quotient of two f32 numbers, the terms are added in float64 (per lane in index order, the lanes by
 *                      a fixed tree, the chunks in chunk order), the sum is divided by total in float64 and rounded to f32 once
 *   rank_sum i64 [Q] = sum over ALL relevant j of rank(j), whatever k: exact, and 1 - (rank_sum - R (R + 1) / 2) / (R (N - R)) is the
 *                      query's ROC-AUC with ties broken by index
 * No ranking is formed and nothing of Q x N entries exists; no atomics on any output: two calls give equal bytes, on any stream.
 * Limits as cmh_soft_topk: 1 <= Q <= CMH_SOFT_Q_MAX, 1 <= N <= 2^31 - 1 in one call, 1 <= bits <= CMH_SOFT_BITS_MAX; label_words >= 1;
 * k in [1, N] or 0.  -1 before any launch: null operands, sizes outside the limits, misaligned planes or rank_sum; -2: a workspace
 * below cmh_soft_ap_workspace_bytes (0 outside the limits; it holds 8 bytes per database item beside the histograms). */
size_t cmh_soft_ap_workspace_bytes(int32_t Q, int64_t N, int32_t bits, int32_t label_words);
int cmh_soft_ap(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz, const uint32_t* q_lab,
                const uint32_t* r_lab, int32_t label_words, int32_t Q, int64_t N, int32_t bits, int32_t k, float* ap, int32_t* relevant,
                int64_t* rank_sum, void* workspace, size_t workspace_bytes, void* stream);
/* Allow-masks made on the GPU (csrc/retrieval_mask.hip).
 * cmh_mask_from_labels: r_label u32 [N, LW] (cmh_pack_labels, LW = ceil(classes / 32)), need u32 [LW] on the GPU -> allow.  Item j is
 * admitted under mode CMH_MASK_ANY iff (label & need) != 0, CMH_MASK_ALL iff (label & need) == need, CMH_MASK_NONE iff (label &
 * need) == 0 (an empty need: any admits nothing, all and none admit everything).  Every word of allow is written once, the bits at
 * and behind N zero; no atomics.  1 <= N <= 2^31 - 1, classes >= 1.
 * cmh_mask_from_ids: sets (value 1) or clears (value 0) the bits of the items ids i32 [M] in an EXISTING mask; duplicates are
 * legal, M = 0 does nothing.  An id outside [0, N) changes nothing and sets *bad (i32 on the GPU, the caller zeroes it).  The bits
 * go in by atomic OR / AND on the mask words: the result does not depend on the order.
 * -1 before any launch: null operands, a misaligned allow, a mode or value that is none of the above, sizes outside the limits. */
#define CMH_MASK_ANY 0
#define CMH_MASK_ALL 1
#define CMH_MASK_NONE 2
int cmh_mask_from_labels(const uint32_t* r_label, const uint32_t* need, int32_t mode, int64_t N, int32_t classes, uint64_t* allow,
                         void* stream);
int cmh_mask_from_ids(const int32_t* ids, int64_t M, int64_t N, int32_t value, uint64_t* allow, int32_t* bad, void* stream);

/* Code diagnostics (csrc/retrieval_stats.hip): the integers behind bit balance, bit correlation, the agreement of an item's two
 * codes and the class / bit tables, from the packed planes, without a float copy of the codes.
 *   Operands A and B hold the same N items: each a pair of planes in cmh_pack_codes' layout, sign and nz u32 [N, ceil(bits / 32)].
 *   Item n carries a in {-1, 0, +1}^abits (a_i = nz_i ? (sign_i ? +1 : -1) : 0) and b in {-1, 0, +1}^bbits.  A packed label matrix
 *   (cmh_pack_labels) passed as sign = nz gives entries 0 / 1; a code's nz plane passed as both planes gives |a|.
 *   gram i64 [abits, bbits]: gram[i][j] = sum_n a_i(n) b_j(n);  a_sum, a_abs i64 [abits] = sum_n a_i, sum_n |a_i|;  b_sum, b_abs
 *   i64 [bbits] likewise (each of the four may be NULL).  Exact integers; the call WRITES every element of every output it is given.
 * Bits at and above abits / bbits in a row's last word are ignored, whatever they hold.  1 <= N <= 2^31 - 1 in one call, 1 <= abits,
 * bbits <= CMH_GRAM_BITS_MAX.  chunk_items: 0 = the plan's choice; else the number of items one workgroup owns, a multiple of 64 up
 * to CMH_GRAM_CHUNK_MAX (for tests that want many chunks and a ragged tail at a small N; the result does not depend on it).
 * -1 before any launch: null operands or gram, sizes outside the limits, such a chunk_items, B planes whose rows are read as 8-byte
 * pairs (an even number of words per row) but are not aligned to 8 bytes (A rows are read word by word); -2: a
 * workspace below cmh_code_gram_workspace_bytes (0 outside the limits).  The partial sums of a chunk are 32-bit (a chunk holds at
 * most 2^20 items) and meet in int64 by integer atomics, whose sum does not depend on the order: two calls give equal bytes, on any
 * stream.  No float arithmetic anywhere. */
#define CMH_GRAM_BITS_MAX 256
#define CMH_GRAM_CHUNK_MAX 1048576
size_t cmh_code_gram_workspace_bytes(int64_t N, int32_t abits, int32_t bbits, int64_t chunk_items);
int cmh_code_gram(const uint32_t* a_sign, const uint32_t* a_nz, const uint32_t* b_sign, const uint32_t* b_nz, int64_t N, int32_t abits,
                  int32_t bbits, int64_t chunk_items, int64_t* gram, int64_t* a_sum, int64_t* a_abs, int64_t* b_sum, int64_t* b_abs,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Hash-table lookup (csrc/retrieval_buckets.hip): the items of a database grouped by equal code, and the groups
 * found by key, at a cost that does not grow with N.  The table holds codes in {-1, +1} (every nz bit inside `bits` set: the caller
 * checks, no entry point reads an nz plane); for those, calc_hammingDist (utils/calc_utils.py:8-13) of two codes is the number of
 * sign bits that differ, a whole number, which is the distance the probes reproduce.
 *   The KEY of a row is its W = ceil(bits / 32) sign words with the bits at and behind `bits` cleared (whatever the plane holds
 *   there), compared as one W-word unsigned integer, word W - 1 most significant.
 * cmh_code_sort: sign u32 [N, W] -> order i32 [N], the item indices in ascending key order, equal keys by ascending item index
 * (stable).  A least-significant-digit radix sort, ceil(bits / 8) passes of 8 bits; a pass in which every key has the same digit is
 * skipped on the device.  `sign` is only read.  1 <= N <= 2^31 - 1, 1 <= bits <= 2048.
 * cmh_code_bucket_count: sorted position i is a bucket head when its key differs from position i - 1's (position 0 always is);
 * head i32 [N] = the inclusive scan of those marks (position i lies in bucket head[i] - 1), *n_buckets (i64 on the GPU, aligned
 * to 8 bytes) = U, the number of heads = of distinct codes.  The caller reads this one number to size the next call's outputs.
 * Workspace: cmh_code_sort_workspace_bytes(N, bits), as cmh_code_sort.
 * cmh_code_bucket_fill: starts i32 [U + 1], bucket b is order[starts[b] : starts[b + 1]] (starts[U] = N); codes i32 [U, W] = the
 * key of each bucket, ascending.  1 <= U <= N.  No workspace.
 * cmh_bucket_probe_count / cmh_bucket_probe_fill: q_sign u32 [Q, W] (keys are cut to `bits` in the kernel) against a table's codes
 * and starts.  A query's probes, in this order: its own key; the key with bit i flipped, i ascending (radius >= 1); with bits
 * i < j flipped, (i, j) in lexicographic order (radius 2): P = 1 + bits + bits (bits - 1) / 2 keys at radius 2, each found or not
 * by one binary search over codes.
 *   count: n_hit_buckets i32 [Q] = the probes that are a bucket's key, n_hit_items i64 [Q] (aligned to 8 bytes) = the items of
 *          those buckets = the query's Hamming ball
 *   fill:  bucket_offsets i64 [Q + 1] = the exclusive prefix sum of n_hit_buckets (aligned to 8 bytes); hit_bucket, hit_dist i32
 *          [capacity], capacity >= bucket_offsets[Q]: query q's hits at bucket_offsets[q] .., in probe order (so ascending distance),
 *          as (bucket, whole-bit distance 0 / 1 / 2).  Nothing at or behind min(bucket_offsets[q + 1], capacity) is written.
 * 1 <= Q <= 65535 per call, 1 <= U <= 2^31 - 1, 1 <= bits <= CMH_BUCKET_BITS_MAX, 0 <= radius <= CMH_BUCKET_RADIUS_MAX.  Both
 * passes search; nothing per probe is kept between them.
 * All six: -1 before any launch for null operands, sizes outside the limits (the message names the limit), misaligned 64-bit
 * operands; -2 for a workspace below cmh_code_sort_workspace_bytes (0 outside the limits).  No atomics on any output, every output
 * word written once, no kernel waits for another workgroup: two calls give equal bytes, on any stream. */
#define CMH_SORT_TILE 2048          /* sorted positions per workgroup of a pass: the unit whose edges the tests aim at */
#define CMH_BUCKET_BITS_MAX 128
#define CMH_BUCKET_RADIUS_MAX 2
size_t cmh_code_sort_workspace_bytes(int64_t N, int32_t bits);
int cmh_code_sort(const uint32_t* sign, int64_t N, int32_t bits, int32_t* order, void* workspace, size_t workspace_bytes, void* stream);
int cmh_code_bucket_count(const uint32_t* sign, const int32_t* order, int64_t N, int32_t bits, int32_t* head, int64_t* n_buckets,
                          void* workspace, size_t workspace_bytes, void* stream);
int cmh_code_bucket_fill(const uint32_t* sign, const int32_t* order, const int32_t* head, int64_t N, int32_t bits, int64_t U,
                         int32_t* starts, int32_t* codes, void* stream);
int cmh_bucket_probe_count(const uint32_t* q_sign, int32_t Q, const int32_t* codes, const int32_t* starts, int64_t U, int32_t bits,
                           int32_t radius, int32_t* n_hit_buckets, int64_t* n_hit_items, void* stream);
int cmh_bucket_probe_fill(const uint32_t* q_sign, int32_t Q, const int32_t* codes, const int32_t* starts, int64_t U, int32_t bits,
                          int32_t radius, const int64_t* bucket_offsets, int64_t capacity, int32_t* hit_bucket, int32_t* hit_dist,
                          void* stream);

/* Radius search past 2 bits: multi-index hashing on 16-bit substrings (csrc/retrieval_mih.hip).  Codes in
 * {-1, +1} as above, 1 <= bits <= CMH_BUCKET_BITS_MAX.  m = ceil(bits / 16); substring j is bits [16 j, 16 j + s_j) of a row's
 * sign words (s_j = 16 but for a shorter last one) and its key those bits as an unsigned integer below 2^s_j.
 * cmh_mih_build: sign u32 [N, W] -> order i32 [m, N], row j = the item indices by ascending (key_j, index), and starts i32
 * [m, 65537]: bucket `key` of table j is order[j][starts[j][key] : starts[j][key + 1]]; the starts of the keys >= 2^s_j of a short
 * last substring, and starts[j][65536], are N.  1 <= N <= 2^31 - 1.  Workspace: cmh_mih_build_workspace_bytes(N, bits) (0 outside
 * the limits).
 * cmh_mih_count / cmh_mih_fill: q_sign u32 [Q, W] against db_sign u32 [N, W] (rows of 2 / 4 words aligned to 8 / 16 bytes) and its
 * tables.  With a, b = divmod(radius, m), substring j is probed at radius a_j = a for j <= b and a - 1 behind (-1: not probed):
 * the keys that are the query's with at most a_j bits flipped, in the order none, single bits ascending, pairs (i, i'), i < i', in
 * lexicographic order.  Every item of a probed bucket is verified with the full distance d, and item x reached through substring j
 * is emitted iff d <= radius and no probed j' < j has d_j' <= a_j': every item within `radius` whole bits, exactly once.
 *   count: n_hits i32 [Q] = the items within `radius` of each query
 *   fill:  offsets i64 [Q + 1] = the exclusive prefix sum of n_hits (aligned to 8 bytes); idx, dist i32 [capacity], capacity >=
 *          offsets[Q] >= 1: query q's items at offsets[q] .., as (database index, whole-bit distance), in the order of the walk
 *          (substring, probe, position in the bucket) - the same on every call; the caller sorts by (distance, index).  Nothing at
 *          or behind min(offsets[q + 1], capacity) is written.
 * 1 <= Q <= 65535 per call, 0 <= radius <= 3 m - 1 (a <= CMH_MIH_SUB_RADIUS_MAX).  Both passes walk; nothing per candidate is kept
 * between them.  All: -1 before any launch for null operands, sizes outside the limits (the message names the limit), misaligned
 * operands; -2 for a workspace that is too small.  No atomics on any output, every output word written once, every index read from
 * a table checked against N, no kernel waits for another workgroup: two calls give equal bytes, on any stream. */
#define CMH_MIH_SUB_BITS 16
#define CMH_MIH_SUB_RADIUS_MAX 2
size_t cmh_mih_build_workspace_bytes(int64_t N, int32_t bits);
int cmh_mih_build(const uint32_t* sign, int64_t N, int32_t bits, int32_t* order, int32_t* starts, void* workspace,
                  size_t workspace_bytes, void* stream);
int cmh_mih_count(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t radius,
                  const int32_t* order, const int32_t* starts, int32_t* n_hits, void* stream);
int cmh_mih_fill(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t radius,
                 const int32_t* order, const int32_t* starts, const int64_t* offsets, int64_t capacity, int32_t* idx, int32_t* dist,
                 void* stream);

/* The k nearest through the same tables, the radius grown per query (csrc/retrieval_mih.hip).  GROWTH STEP
 * s = t m + j (t = 0, 1, 2; j < m) probes substring j at exactly level t: the keys that are the query's with exactly t of its s_j
 * bits flipped, in the order above (1, s_j or s_j (s_j - 1) / 2 probes).  After steps 0 .. r the substrings have been probed at
 * the radii a_j of radius r, so every item within r has been reached; item x is first reached at step f(x) = min_j (d_j m + j), a
 * unique minimum, and a candidate reached through (j, t) counts, or is emitted, iff f(x) = t m + j.  One workgroup of 256 threads
 * per query walks the steps in order and verifies every candidate with the full distance d.
 *   cmh_mih_knn_count: r*(q) = the smallest r <= r_cap with |ball(q, r)| >= k, decided after step r (the numbers of the items at
 *          every distance d <= r are complete then).  radius i32 [Q] = r*, n_ball i32 [Q] = |ball(r*)|, n_less i32 [Q] =
 *          |ball(r* - 1)| (0 at r* = 0); fewer than k items within r_cap: radius = -1 and n_ball = n_less = |ball(r_cap)|.
 *   cmh_mih_knn_fill: radius i32 [Q] is READ; the walk over steps 0 .. radius[q] emits every item with d <= radius[q] exactly once
 *          at offsets[q] .. as (database index, whole-bit distance), in walk order (step, probe, position in the bucket) - the
 *          same on every call.  offsets i64 [Q + 1] (aligned to 8 bytes) = the exclusive prefix sum of the lists' sizes (n_ball,
 *          0 where nothing is walked); idx, dist i32 [capacity], capacity >= 1.  Nothing is written for radius[q] < 0 or
 *          radius[q] > 3 m - 1 (such a query is not walked: the loop bound is never an operand's word beyond 3 m - 1), and
 *          nothing at or behind min(offsets[q + 1], capacity).
 * 1 <= Q <= 65535 per call, 1 <= N <= 2^31 - 1, 1 <= bits <= CMH_BUCKET_BITS_MAX, 1 <= k <= N, 0 <= r_cap <= 3 m - 1, db_sign rows
 * aligned as for cmh_mih_count.  -1 before any launch for null operands, sizes outside the limits (the message names the limit),
 * misaligned operands.  No atomics on any output, every output word written once, every index read from a table checked against
 * N, bucket bounds clamped to [0, N], no kernel waits for another workgroup: two calls give equal bytes, on any stream. */
int cmh_mih_knn_count(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t k, int32_t r_cap,
                      const int32_t* order, const int32_t* starts, int32_t* radius, int32_t* n_ball, int32_t* n_less, void* stream);
int cmh_mih_knn_fill(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, const int32_t* radius,
                     const int32_t* order, const int32_t* starts, const int64_t* offsets, int64_t capacity, int32_t* idx,
                     int32_t* dist, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pairwise similarity / quantisation losses (forward).  All f32; `loss` is a device scalar.
 * ------------------------------------------------------------------------------------------- */
size_t cmh_loss_workspace_bytes(int32_t B, int32_t K, int32_t C);

/* DSPH HyP.forward (train/DSPH/loss.py:22-72).  x,y [B,K] hash outputs, label [B,C] in {0,1},
 * proxies [C,K]. */
int cmh_dsph_hyp_loss(const float* x, const float* y, const float* label, const float* proxies,
                      int32_t B, int32_t K, int32_t C, float threshold, float alpha, float* loss,
                      void* workspace, size_t workspace_bytes, void* stream);

/* DCHMT our_loss with hash_layer == "select" (train/DCHMT/hash_train.py:82-150).
 * img,txt [B,D] (D = 2*output_dim), label [B,C].  similarity: 0 = euclidean, 1 = cosine;
 * loss_type: 1 = l1, 2 = l2. */
int cmh_dchmt_loss(const float* img, const float* txt, const float* label, int32_t B, int32_t D,
                   int32_t C, int32_t output_dim, int32_t similarity, int32_t loss_type,
                   float vartheta, float sim_threshold, float* loss, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DNPH (TOMM) and TwDH heads / losses (BASELINE.json configs 4 and 5).
 * ------------------------------------------------------------------------------------------- */
/* nn.BatchNorm1d in TRAINING mode (batch mean, biased batch variance): the TwDH image head's `norm`
 * (model/TwDH.py:61,78), which the reference never switches to eval.  x,y f32 [B,d]. */
int cmh_batchnorm1d_train(const float* x, const float* w, const float* b, float eps, float* y, int32_t B,
                          int32_t d, void* stream);

/* The module side effect of that forward: running_mean / running_var (momentum 0.1, unbiased variance), part of the checkpoint. */
int cmh_batchnorm1d_update_running(const float* x, float momentum, float* running_mean, float* running_var, int32_t B,
                                   int32_t d, void* stream);
/* Backward of cmh_batchnorm1d_train: dx [B,d], dw [d], db [d] from dy [B,d] (statistics recomputed from x). */
int cmh_batchnorm1d_backward(const float* x, const float* w, float eps, const float* dy, float* dx, float* dw, float* db,
                             int32_t B, int32_t d, void* stream);
/* Backward of cmh_twdh_loss: dp_img / dp_txt f32 [B,2K] from the upstream gradients of the two scalars (device pointers to one
 * float each; NULL = 0).  BCELoss as ATen differentiates it: (p - t) / max((1 - p) p, 1e-12) / numel. */
int cmh_twdh_loss_backward(const float* p_img, const float* p_txt, const float* target, int32_t B, int32_t K,
                           const float* d_nce, const float* d_quan, float* dp_img, float* dp_txt, void* stream);

/* hash_center_multilables (train/TwDH/hash_train.py:93-115): code[b,k] = sign(mean of the centers of b's
 * classes), exact zeros replaced by random_center[k] (a +-1 vector drawn once per call by the caller).
 * label f32 [B,C], center f32 [C,K] (+-1), code f32 [B,K]. */
int cmh_twdh_targets(const float* label, const float* center, const float* random_center, float* code,
                     int32_t B, int32_t C, int32_t K, void* stream);

/* TwDH loss terms for one code length (train/TwDH/hash_train.py:117-139): p_img/p_txt f32 [B,2K] pair
 * probabilities, target f32 [B,K] in {-1,+1}.  out2[0] = (BCE_img + BCE_txt)/2 with hash_convert one-hot
 * targets, out2[1] = ((1-mean((2p_img-1)^2)) + (1-mean((2p_txt-1)^2)))/2.  workspace >= 256 bytes. */
int cmh_twdh_loss(const float* p_img, const float* p_txt, const float* target, int32_t B, int32_t K,
                  float* out2, void* workspace, size_t workspace_bytes, void* stream);

/* DNPH_out.forward + the noise term of the DNPH step (train/DNPH_TOMM/loss.py:14-32,
 * train/DNPH_TOMM/hash_train.py:70-81).  hash_* f32 [B,K], pre_* f32 [B,C], label f32 [B,C], proxies [C,K],
 * noise_* f32 [B,K] (the Hungarian-assigned +-1 rows: cmh_assign_rows, or upstream's host path) or both NULL.
 * out3[0] = p_loss + d_loss - noise_weight*noise, out3[1] = p_loss + d_loss, out3[2] = noise. */
int cmh_dnph_loss(const float* hash_img, const float* hash_txt, const float* pre_img, const float* pre_txt,
                  const float* label, const float* proxies, const float* noise_img, const float* noise_txt,
                  int32_t B, int32_t K, int32_t C, float margin, float noise_weight, float* out3,
                  void* workspace, size_t workspace_bytes, void* stream);

/* gene_noise of the DNPH step (train/DNPH_TOMM/b_reg.py:5-40) for P modalities that share one noise matrix, on the device:
 * cost[p][i][j] = || emb[p][i] - rows[j] ||_2 in f64 (f32 inputs widened, the sum over k in index order), the square linear
 * assignment problem of each p solved exactly (shortest augmenting paths, f64 duals - scipy's algorithm family), and
 * out[p][i] = rows[col4row[p][i]].  emb f32 [P,B,K], rows f32 [B,K] (upstream: +-1), out f32 [P,B,K], col_out i32 [P,B] or NULL.
 * 1 <= B <= 1024, K >= 1, P >= 1.  Where several assignments have exactly the optimal cost, the one returned is fixed by the
 * solver's tie rule (lowest reduced cost, then an unassigned column, then the lowest column index): the same on every run, not
 * necessarily scipy's.  Values must be finite.  workspace >= cmh_assign_rows_workspace_bytes(P, B) (0 for sizes out of range). */
size_t cmh_assign_rows_workspace_bytes(int32_t P, int32_t B);
int cmh_assign_rows(const float* emb, const float* rows, int32_t P, int32_t B, int32_t K, float* out, int32_t* col_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-free hash heads from paired features: LSH, PCAH, ITQ (csrc/itq.hip).  No upstream counterpart.  The fit runs in f64 on
 * f32 features image F_i / text F_t [N, D] and ends in one affine map per modality, code = sign(W_m f + b_m): a LinearHash head.
 * Limits: 1 <= D <= 1024, 1 <= K <= min(D, 128), rows <= 65535 * 2048.  Every output element is one sum in a fixed order (row
 * chunks of 2048 summed in row order, then the chunks in order; fixed reduction trees; no atomics), so two calls give equal bits.
 * Each call checks its arguments on the host before any launch: a null pointer, a size outside the limits or a workspace
 * smaller than its *_workspace_bytes query (0 for sizes out of range) comes back as CMH_ERR_INVALID with a message.
 * ------------------------------------------------------------------------------------------- */
/* sum [D] (+)= sum_n F[n], sq [D,D] (+)= sum_n F[n] F[n]^T, f64; accumulate = 0 overwrites, 1 adds this batch to the running sums. */
size_t cmh_itq_moments_workspace_bytes(int64_t N, int32_t D);
int cmh_itq_moments(const float* F, int64_t N, int32_t D, double* sum, double* sq, int32_t accumulate, void* workspace,
                    size_t workspace_bytes, void* stream);
/* From the running sums over N pairs: mu_m [D] = sum_m / N; alpha2[m] = 1 / sqrt(mean_n |f - mu_m|^2) (0 where that is not
 * positive), m = 0 image, 1 text; C [D,D] = 1/2 sum_m alpha_m^2 (sq_m / N - mu_m mu_m^T), symmetric bit for bit. */
int cmh_itq_covariance(const double* sum_i, const double* sq_i, const double* sum_t, const double* sq_t, int64_t N, int32_t D,
                       double* mu_i, double* mu_t, double* alpha2, double* C, void* stream);
/* Symmetric eigen-solver: cyclic Jacobi in round-robin order (one launch per set of disjoint rotations) on the upper triangle
 * of C [D,D].  A pair is rotated where |a_pq| > eps_f64 sqrt(|a_pp a_qq|); a sweep that rotates nothing ends the run (one 4-byte
 * host read per sweep).  evals [D] descending, ties by index; evecs [D,D], column j the vector of evals[j], signed so that its
 * entry of largest magnitude (lowest row on a tie) is positive.  info2 (host): sweeps run, and 1 if the run converged within
 * max_sweeps (1..1024), else 0 (the outputs are then the state after max_sweeps). */
size_t cmh_itq_eigh_workspace_bytes(int32_t D, int32_t max_sweeps);
int cmh_itq_eigh(const double* C, int32_t D, int32_t max_sweeps, double* evals, double* evecs, int32_t* info2, void* workspace,
                 size_t workspace_bytes, void* stream);
/* V [N,K] f64 = alpha[0] * (F - mu) P, the sum over d in index order; mu [D], alpha one f64 on the device, P [D,K] f64. */
int cmh_itq_project(const float* F, int64_t N, int32_t D, int32_t K, const double* mu, const double* alpha, const double* P,
                    double* V, void* stream);
/* One ITQ pass over V [rows,K] with rotation R [K,K]: Z = V R, B i8 = +1 where Z >= 0 else -1, M [K,K] = B^T V,
 * obj2 = (|B - Z|^2, |Z|^2). */
size_t cmh_itq_step_workspace_bytes(int64_t rows, int32_t K);
int cmh_itq_step(const double* V, int64_t rows, int32_t K, const double* R, double* Z, int8_t* B, double* M, double* obj2,
                 void* workspace, size_t workspace_bytes, void* stream);
/* R [K,K] = (orthogonal polar factor of M [K,K])^T, ITQ's UA UB^T for M = UB S UA^T, by a one-sided Jacobi SVD in one workgroup
 * (a pair of columns is rotated where |g_p . g_q| > sqrt(K) eps_f64 |g_p| |g_q|, at most 60 sweeps).  Unique for non-singular M; for a singular one the null
 * directions (column norm <= sqrt(K) eps_f64 |M|_F) are completed to an orthonormal basis, so R is orthogonal and R M symmetric.
 * sweeps (device i32, may be NULL): sweeps run. */
size_t cmh_itq_polar_workspace_bytes(int32_t K);
int cmh_itq_polar(const double* M, int32_t K, double* R, int32_t* sweeps, void* workspace, size_t workspace_bytes, void* stream);
/* ITQ: R = R0, then `iters` times (step, R <- polar(M)); obj [iters + 1] (device): |B - Z|^2 at the start of each iteration and,
 * last, for the R returned; zz (device): |V R|^2 for that R.  iters = 0 leaves R = R0.  Nothing is read back in the loop. */
size_t cmh_itq_rotate_workspace_bytes(int64_t rows, int32_t K);
int cmh_itq_rotate(const double* V, int64_t rows, int32_t K, const double* R0, int32_t iters, double* R, double* obj, double* zz,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The heads: s = 0.5 / sqrt(zz[0] / (rows K)) (s_out, device, may be NULL), W_m f32 [K,D] = s alpha2[m] (P R)^T,
 * b_m f32 [K] = -W_m mu_m (from the f64 products). */
int cmh_itq_heads(const double* P, const double* R, const double* mu_i, const double* mu_t, const double* alpha2, const double* zz,
                  int64_t rows, int32_t D, int32_t K, float* W_i, float* b_i, float* W_t, float* b_t, double* s_out, void* stream);
/* The same with one projection per modality: W_m = s alpha2[m] (P_m R)^T.  cmh_itq_heads is the case P_i = P_t, bit for bit. */
int cmh_itq_heads_pair(const double* P_i, const double* P_t, const double* R, const double* mu_i, const double* mu_t,
                       const double* alpha2, const double* zz, int64_t rows, int32_t D, int32_t K, float* W_i, float* b_i, float* W_t,
                       float* b_t, double* s_out, void* stream);
/* CCA projections (the cross-modal variant of the ITQ paper): one P_m per modality from the whitened cross-covariance.  The same
 * limits, determinism and host checks as the block above.
 * cross [D,D] (+)= sum_n F_i[n] F_t[n]^T, f64, not symmetric: the row chunks, chunk order and accumulate flag of cmh_itq_moments. */
size_t cmh_itq_cross_moments_workspace_bytes(int64_t N, int32_t D);
int cmh_itq_cross_moments(const float* F_i, const float* F_t, int64_t N, int32_t D, double* cross, int32_t accumulate, void* workspace,
                          size_t workspace_bytes, void* stream);
/* mu_m and alpha2 as cmh_itq_covariance; S_ii, S_tt [D,D] = alpha_m^2 (sq_m / N - mu_m mu_m^T) (trace 1, symmetric bit for bit),
 * S_it [D,D] = alpha_i alpha_t (cross / N - mu_i mu_t^T). */
int cmh_itq_cca_covariance(const double* sum_i, const double* sq_i, const double* sum_t, const double* sq_t, const double* cross,
                           int64_t N, int32_t D, double* mu_i, double* mu_t, double* alpha2, double* S_ii, double* S_tt, double* S_it,
                           void* stream);
/* out[j] = 1 / sqrt(values[j] + shift), 0 where values[j] + shift <= 0; root[j] (may be NULL) = sqrt(max(values[j] + shift, 0)).
 * 1 <= n <= 1024, shift >= 0: the whitener's (lambda + r)^-1/2, and sigma and 1 / sigma from the eigenvalues of T T^T. */
int cmh_itq_inv_sqrt(const double* values, int32_t n, double shift, double* out, double* root, void* stream);
/* C [M,N] = op(A) diag(d) op(B) diag(col_scale), f64, 1 <= M, N, Kc <= 1024.  op(A) is A [M,Kc], or with trans_a = 1 the
 * transpose of A [Kc,M]; op(B) is B [Kc,N], or with trans_b = 1 the transpose of B [N,Kc]; d [Kc] and col_scale [N] may be NULL.
 * Each C[i][j] is one chain over k ascending, acc = fma(a b, d_k, acc) (fma(a, b, acc) without d), whatever the grid: two calls
 * give equal bits, a transposed operand gives the bits of its materialised transpose, and op(A) = op(B)^T gives a C that is
 * symmetric bit for bit.  C must not be an operand. */
int cmh_itq_matmul(const double* A, const double* B, const double* d, const double* col_scale, int32_t M, int32_t N, int32_t Kc,
                   int32_t trans_a, int32_t trans_b, double* C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Supervised training-free heads (csrc/dch.hip).  No upstream counterpart: discrete cross-modal hashing on frozen features (DCH,
 * Xu et al., TIP 2017; the cross-modal form of SDH, Shen et al., CVPR 2015), the fit utils/dch.py runs with the cmh_itq_* pieces
 * above (moments, eigen-solver, small products, projection, heads).  B int8 [N,K] holds +1 / -1; labels Y are f32 [N,C]; everything
 * else is f64.  Limits: 1 <= D <= 1024, 1 <= K <= min(D, 128) (K <= 128 where no D is passed), 1 <= C <= 1024, 1 <= N <= 65535 * 2048.
 * Determinism as the block above: every output element is one sum in a fixed order (rows in chunks of 2048, chunks in chunk order,
 * block trees, partials in block order), no atomics, no kernel waits for another workgroup; two calls give equal bits.  Every call
 * refuses, before any launch, a null pointer, a size out of range or a workspace one byte short with CMH_ERR_INVALID and a message
 * that names it; the *_workspace_bytes queries return 0 for sizes out of range.
 * S [D,D] = alpha[0]^2 (sq / N - mu mu^T) of one modality (trace 1; cmh_itq_cca_covariance's S_mm without a cross moment). */
int cmh_dch_covariance(const double* sq, const double* mu, const double* alpha, int64_t N, int32_t D, double* S, void* stream);
/* The start: B[n][k] = +1 where Za[n][k] + Zb[n][k] >= 0, else -1 (Za, Zb [N,K]: both modalities' rows on the leading eigenvectors). */
int cmh_dch_start(const double* Za, const double* Zb, int64_t N, int32_t K, int8_t* B, void* stream);
/* out [Dx,K] (+)= X^T B for X f32 [N,Dx] (F_m with Dx = D, Y with Dx = C; 1 <= Dx <= 1024) and, where bsum is not NULL,
 * bsum [K] (+)= 1^T B: one fma per row in row order within a chunk, the chunks in chunk order; accumulate = 1 adds to out / bsum. */
size_t cmh_dch_xtb_workspace_bytes(int64_t N, int32_t Dx, int32_t K);
int cmh_dch_xtb(const float* X, const int8_t* B, int64_t N, int32_t Dx, int32_t K, double* out, double* bsum, int32_t accumulate,
                void* workspace, size_t workspace_bytes, void* stream);
/* out [K,K] = B^T B: integers below 2^53, so exact, symmetric and free of any order. */
size_t cmh_dch_btb_workspace_bytes(int64_t N, int32_t K);
int cmh_dch_btb(const int8_t* B, int64_t N, int32_t K, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* U [D,K] = (alpha[0] (T[d][k] - mu[d] bsum[k])) / N for T = F^T B [D,K]: X^T B / N with X = alpha (F - mu), the right-hand side of
 * the feature regression P = A U. */
int cmh_dch_center(const double* T, const double* bsum, const double* mu, const double* alpha, int64_t N, int32_t D, int32_t K, double* U,
                   void* stream);
/* W [K,C] = (A + shift I)^-1 R for a symmetric positive definite A [K,K] (the lower triangle is read) and R [K,C], shift >= 0, by
 * a Cholesky factorisation in one workgroup with the factor in LDS (pitch K + 1: 132 096 bytes at K = 128), then a forward and a
 * backward substitution per column of R; every inner sum is one fma chain over k ascending.  info (device): 0, or 1 + the index of
 * the first pivot that is not positive - then W is zeros.  W must not be an operand. */
int cmh_dch_solve(const double* A, double shift, const double* R, int32_t K, int32_t C, double* W, int32_t* info, void* stream);
/* Qt [K,N] (bit-major; may be NULL) = (Y W^T + mu Z_i + mu Z_t)^T: q = sum_c Y[n][c] W[l][c] (c ascending), then fma(mu, z_i, q),
 * then fma(mu, z_t, .).  obj2 (device): obj2[0] = (|Y - B W|^2 + lam |W|^2) + mu (|B - Z_i|^2 + |B - Z_t|^2), obj2[1] = |Z_i|^2 +
 * |Z_t|^2; W [K,C], Z_i, Z_t [N,K].  Per-block partials, added in block order by a finishing kernel. */
size_t cmh_dch_targets_workspace_bytes(int64_t N);
int cmh_dch_targets(const float* Y, const int8_t* B, const double* W, const double* Z_i, const double* Z_t, double mu, double lam,
                    int64_t N, int32_t K, int32_t C, double* Qt, double* obj2, void* workspace, size_t workspace_bytes, void* stream);
/* Discrete cyclic coordinate descent, in place on B: `rounds` (1 .. 64) Gauss-Seidel rounds over the bits l = 0 .. K - 1 of every
 * item n: t = Qt[l][n], then t = fma(-b_k, G[k][l], t) for k ascending, k != l; b_l = +1 where t > 0, -1 where t < 0, unchanged
 * where t == 0.  G [K,K].  flips int64 [rounds] (device): the bits changed in each round; min_margin (device): the smallest |t|
 * over all rounds x K x N decisions of the call. */
size_t cmh_dch_dcc_workspace_bytes(int64_t N, int32_t rounds);
int cmh_dch_dcc(const double* Qt, const double* G, int8_t* B, int64_t N, int32_t K, int32_t rounds, int64_t* flips, double* min_margin,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MITH (BASELINE.json config 3): token-returning trunk, HashingModel pieces, losses.
 * Activations are batch-major: [N, K, D] where the reference holds [K, N, D].
 * ------------------------------------------------------------------------------------------- */
#define CMH_EPI_GELU 16       /* exact GELU (nn.GELU()) in cmh_linear_gemm's epilogue, model/MITH.py:224-233 */
#define CMH_EPI_RELU 32
#define CMH_EPI_RES_F16 64    /* residual is IEEE fp16 (the bf16 mode's residual stream); needs N % 256 == 0 */
#define CMH_EPI_OUT_F16 128   /* out is fp16 instead of f32; needs N % 256 == 0, excludes CMH_EPI_OUT_BF16 */
#define CMH_EPI_MUL_DQGELU 1024  /* out *= QuickGELU'(aux[m,n]), aux = the saved pre-activation passed as `residual`, typed like
                                  * the output (bf16 with CMH_EPI_OUT_BF16, else f32); N % 256 == 0; excludes CMH_EPI_RESIDUAL */

/* ViT.forward of the MITH trunk (model/MITH.py:56-82): ln_post + proj on EVERY token.
 * tokens_out f32 [B*(g*g+1), embed_dim]; row b*(g*g+1) is the class token, the rest the patch tokens. */
int cmh_vit_encode_tokens(const cmh_vit_weights* w, const float* image, int32_t batch, float* tokens_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* CLIP1.encode_text (model/MITH.py:120-144): causal mask + key_padding_mask in every block, ln_final +
 * text_projection on every token.  tokens_out f32 [B*L, embed_dim]; eot_rows_out i32 [B] = b*L + argmax(tokens[b]). */
int cmh_text_encode_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                           const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The same, with the caller's promise that nothing reads the padded positions of tokens_out - MITH's HashingModel gives them weight 0
 * (model/MITH.py:349-376): rows behind a caption's last unpadded token are not computed and come back as ZEROS; every other position
 * carries the bits of cmh_text_encode_tokens.  key_padding_mask NULL, or cmh_set_text_token_packing(0): exactly cmh_text_encode_tokens. */
int cmh_text_encode_tokens_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                  const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* `layers` ResidualAttentionBlocks applied in place to a caller-owned residual stream x f32 [B*T, d]
 * (MITH's 2-layer concept transformer, model/MITH.py:385-395). */
size_t cmh_blocks_workspace_bytes(int32_t dtype, int32_t B, int32_t T, int32_t d);
int cmh_transformer_blocks(const cmh_block_weights* blocks, int32_t layers, int32_t dtype, float* x, int32_t B,
                           int32_t T, int32_t d, int32_t causal, const uint8_t* key_padding_mask,
                           void* workspace, size_t workspace_bytes, void* stream);

/* LocalizedTokenAggregation.forward (model/MITH.py:317-376).  tokens f32 [B*Ltot, D], sim f32 [B*Ltot, K] (tanh
 * concept scores of every token); the L tokens l0..l0+L-1 of each sample take part (image: Ltot=50, l0=1, L=49).
 * key_padding_mask u8 [B, L] optional.  out f32 [B, K, D].  L <= 80, K <= 128, top_k <= 8. */
int cmh_mith_lta(const float* tokens, const float* sim, const uint8_t* key_padding_mask, float* out, int32_t B,
                 int32_t Ltot, int32_t l0, int32_t L, int32_t K, int32_t D, int32_t top_k, void* stream);
/* x[b,t,:] += pe[t,:]   (PositionalEncoding.forward, model/MITH.py:270-273; pe is the registered buffer). */
int cmh_add_positional(float* x, const float* pe, int32_t B, int32_t T, int32_t D, void* stream);
/* BitwiseHashing (model/MITH.py:276-293): out[b,k] = tanh(x[b,k,:] . w[k,:] + bias[k]). */
int cmh_bitwise_hash(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t K,
                     int32_t D, void* stream);
/* F.normalize(x, dim=-1) (eps 1e-12) over rows of x f32 [R, D]. */
int cmh_l2_normalize_rows(const float* x, float* y, int32_t R, int32_t D, void* stream);
/* B = sign(lambda*(img_cls+txt_cls) + (1-lambda)*(img_tok+txt_tok)); H_img = .5 img_cls + .5 img_tok; H_txt likewise
 * (train/MITH/hash_train.py:80-83,179-180). */
int cmh_mith_mix(const float* img_cls, const float* img_tok, const float* txt_cls, const float* txt_tok,
                 float hyper_lambda, float* B_codes, float* H_img, float* H_txt, int64_t n, void* stream);
/* out[0] = sum (a-b)^2   (F.mse_loss(reduction='sum'): quantisation and distillation terms, :146-147,193-200). */
int cmh_sq_diff_sum(const float* a, const float* b, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                    void* stream);
/* bayesian_loss (train/MITH/hash_train.py:138-144) of a memory bank [Mb,K] against the batch codes [B,K] with
 * label_sim = (bank_label . label^T > 0) computed on the fly (bank_label f32 [Mb,C], label f32 [B,C]). */
int cmh_mith_bayesian_loss(const float* bank, const float* batch, const float* bank_label, const float* label,
                           int32_t Mb, int32_t B, int32_t K, int32_t C, float* out, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Symmetric InfoNCE with diagonal targets inside groups of G consecutive rows: G = R reproduces info_nce_loss
 * (:103-114), a/b = [N*L, D] with G = L reproduces info_nce_loss_bmm (:116-136). */
int cmh_info_nce(const float* a, const float* b, int32_t R, int32_t G, int32_t D, float temperature, float* out,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Workspace that lets cmh_info_nce / cmh_info_nce_backward form the R x G score matrix once, as 16 x 16 tiles on the f32 matrix
 * pipe (round 3; needs D % 64 == 0).  With a smaller workspace (>= 256 bytes forward, >= 8 R + 256 backward) both calls keep the
 * per-row kernels of round 1: same values up to f32 summation order. */
size_t cmh_info_nce_workspace_bytes(int32_t R, int32_t G);

/* ---------------------------------------------------------------------------------------------
 * BertAdam, one fused multi-tensor step (model/base/optimization.py:103-168; SURVEY 8f "next" #1).
 * `tensors` is a HOST array; p/g/m/v are device pointers to f32 tensors of n elements (m = state['next_m'],
 * v = state['next_v']).  Per tensor: g *= min(1, max_grad_norm/(||g||+1e-6)) in place when max_grad_norm > 0 (:135-136);
 * m = m*b1 + (1-b1)*g (:141); v = v*b2 + (1-b2)*g*g (:143); p -= lr * (m/(sqrt(v)+eps) + weight_decay*p) (:144-164),
 * with lr = the caller's already scheduled rate (lr * schedule(step/t_total, warmup), :157-161).
 * Synchronises `stream` once on entry (it re-uses a host staging table).
 * ------------------------------------------------------------------------------------------- */
typedef struct cmh_adam_tensor {
  float* p; float* g; float* m; float* v;
  int64_t n;
  float lr, weight_decay, max_grad_norm;
  void* p_bf16;             /* optional (NULL): bf16 [n] copy of p - the encoder's CMH_BF16 GEMM operand - rewritten with the updated
                             * values (round-to-nearest-even, as cmh_cast_f32_to_bf16), so that no cast pass follows the step */
} cmh_adam_tensor;
size_t cmh_bert_adam_workspace_bytes(int32_t count, int64_t total_elems);
/* b1 / b2 / eps are doubles because the reference forms 1 - b in python doubles before ATen rounds it to f32. */
int cmh_bert_adam_step(const cmh_adam_tensor* tensors, int32_t count, double b1, double b2, double eps,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward building blocks of the towers (SURVEY 8f "next" #2).  Element kinds: 0 = f32, 1 = bf16, 2 = fp16.
 * ------------------------------------------------------------------------------------------- */
#define CMH_KIND_F32 0
#define CMH_KIND_BF16 1
#define CMH_KIND_F16 2
/* dst[c, r] = cast(src[r, c]): wgrad operands (dW = dY^T . X contracts over rows). */
int cmh_transpose(const void* src, int32_t src_kind, void* dst, int32_t dst_kind, int32_t rows, int32_t cols, void* stream);
/* out[c] = sum_r x[r, c] (bias gradients), f32 result, deterministic two-pass reduction. */
size_t cmh_colsum_workspace_bytes(int32_t rows, int32_t cols);
int cmh_colsum(const void* x, int32_t kind, int32_t rows, int32_t cols, float* out, void* workspace, size_t workspace_bytes,
               void* stream);
/* nn.LayerNorm backward (model/base/model.py:153-159, eps 1e-5): x f32|fp16 [M,d] (the forward's input), dy f32|bf16 [M,d],
 * dx f32 [M,d] (accumulate != 0: dx += ...), dgamma / dbeta f32 [d]. */
size_t cmh_layernorm_backward_workspace_bytes(int32_t M, int32_t d);
int cmh_layernorm_backward(const void* x, int32_t x_kind, const void* dy, int32_t dy_kind, const float* gamma, int32_t M,
                           int32_t d, float* dx, int32_t accumulate, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Backward of cmh_attention (same layouts and masks): qkv [B*T,3d], o = the forward output [B*T,d], dout [B*T,d] ->
 * dqkv [B*T,3d]; softmax probabilities are recomputed.  T <= 4096 (whole-sequence kernels up to 128, the tiled kernel beyond; the
 * tiled kernel and the bf16 kernel at T <= 96 do not read o). */
int cmh_attention_backward(int32_t dtype, const void* qkv, const void* o, const void* dout, void* dqkv, int32_t B, int32_t T,
                           int32_t d, int32_t causal, const uint8_t* key_padding_mask, void* stream);
/* out = pre * sigmoid(1.702 pre) element-wise from a saved pre-activation (model/base/model.py:162-164). */
int cmh_quick_gelu(const void* pre, void* out, int64_t n, int32_t kind, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training forward (keeps a tape of activations) and backward of the two towers.  Gradients are WRITTEN (not accumulated) into
 * caller-owned f32 buffers shaped like the reference's parameters (model/base/model.py; note `proj` / `text_projection` are in
 * the parameter's own [width, embed_dim] layout, not transposed).  `tape` (cmh_*_train_bytes) holds the activations between
 * the forward and the backward call plus all scratch, so one tape serves one (forward, backward) pair at a time.
 * ------------------------------------------------------------------------------------------- */
typedef struct cmh_block_grads {
  float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b, *fc_w, *fc_b, *proj_w, *proj_b;
} cmh_block_grads;
typedef struct cmh_vit_grads {
  float* conv1_w;               /* [width, 3*patch*patch] */
  float* class_embedding;       /* [width] */
  float* positional_embedding;  /* [grid*grid+1, width] */
  float *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b;
  float* proj;                  /* [width, embed_dim] */
  const cmh_block_grads* blocks;   /* host array [layers] */
} cmh_vit_grads;
typedef struct cmh_text_grads {
  float* token_embedding;       /* [vocab, width]  (zeroed, then scatter-added) */
  float* positional_embedding;  /* [context_length, width] */
  float *ln_final_w, *ln_final_b;
  float* text_projection;       /* [width, embed_dim] */
  const cmh_block_grads* blocks;
} cmh_text_grads;
/* Weight / bias gradient of y = x W^T + b: dw[O,I] f32 = dy^T x, db[O] f32 = column sums of dy (db may be NULL).  dy [M,O]
 * and x [M,I] are given in CMH_KIND_* element types and are transposed + cast to `dtype` (the GEMM arithmetic) internally;
 * the product runs on the encoder's GEMM kernel, split over K = M when the output has few tiles. */
size_t cmh_linear_wgrad_workspace_bytes(int32_t dtype, int32_t M, int32_t O, int32_t I);
int cmh_linear_wgrad(int32_t dtype, const void* dy, int32_t dy_kind, const void* x, int32_t x_kind, int32_t M, int32_t O,
                     int32_t I, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of cmh_linear_act (LinearHash, model/modelbase.py:25-35): y = the forward output, dy its gradient, drop_mask /
 * keep_scale / act as in the forward call -> dx [M,K], dw [N,K], db [N].  workspace >= M*N*4 + 256 bytes. */
int cmh_linear_act_backward(const float* x, const float* w, const float* y, const float* dy, const float* drop_mask,
                            float keep_scale, int32_t act, float* dx, float* dw, float* db, int32_t M, int32_t N, int32_t K,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Backward of cmh_dsph_hyp_loss (train/DSPH/loss.py:22-72): dloss = optional device scalar (NULL = 1) ->
 * dx, dy [B,K], dproxies [C,K].  K <= 512. */
size_t cmh_head_backward_workspace_bytes(int32_t B, int32_t K, int32_t C);
int cmh_dsph_hyp_loss_backward(const float* x, const float* y, const float* label, const float* proxies, int32_t B, int32_t K,
                               int32_t C, float threshold, float alpha, const float* dloss, float* dx, float* dy,
                               float* dproxies, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of cmh_pair_softmax (DCHMT select head): p = the forward output [M,2K], dp its gradient -> dz [M,2K]. */
int cmh_pair_softmax_backward(const float* p, const float* dp, float* dz, int32_t M, int32_t K, void* stream);
/* Backward of cmh_dchmt_loss (train/DCHMT/hash_train.py:82-150): same arguments, dloss = optional device scalar (NULL = 1)
 * -> dimg, dtxt [B,D].  D <= 512; workspace >= cmh_head_backward_workspace_bytes(B, D, C). */
int cmh_dchmt_loss_backward(const float* img, const float* txt, const float* label, int32_t B, int32_t D, int32_t C,
                            int32_t output_dim, int32_t similarity, int32_t loss_type, float vartheta, float sim_threshold,
                            const float* dloss, float* dimg, float* dtxt, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of cmh_dnph_loss (train/DNPH_TOMM/loss.py:14-32 + the noise term of hash_train.py:65-81; pass NULL noises for
 * DNPH_out alone): gradients w.r.t. both hash outputs [B,K], both classifier outputs [B,C] and the proxies [C,K]. */
size_t cmh_dnph_backward_workspace_bytes(int32_t B, int32_t K, int32_t C);
int cmh_dnph_loss_backward(const float* hash_img, const float* hash_txt, const float* pre_img, const float* pre_txt,
                           const float* label, const float* proxies, const float* noise_img, const float* noise_txt, int32_t B,
                           int32_t K, int32_t C, float margin, float noise_weight, const float* dloss, float* dhash_img,
                           float* dhash_txt, float* dpre_img, float* dpre_txt, float* dproxies, void* workspace,
                           size_t workspace_bytes, void* stream);
/* ---- input pipeline, image side ---------------------------------------------------------------------
 * dataset/base.py:35-44 (the two transform chains) and :55-64 (_load_image) for a whole batch of DECODED images:
 * train != 0: Resize(R, BICUBIC) -> CenterCrop(R) -> ToTensor -> Normalize(mean, std); train == 0: Resize((R, R), BICUBIC) -> ...
 * Bit-identical to Pillow's Image.resize + torchvision's rules (tests/golden/preprocess.npz).
 *   pixels  device, uint8 RGB HWC images back to back;  offsets device int64 [batch] byte offset of each image;
 *   hw      device int32 [batch, 2] = (height, width);  max_h / max_w >= every image's size (sizes the launch and the workspace);
 *   mean / stdv  HOST float[3];  out device f32 [batch, 3, R, R] and/or out_u8 device uint8 [batch, R, R, 3] (the image that
 *   reaches ToTensor; either may be NULL). */
size_t cmh_image_preprocess_workspace_bytes(int32_t batch, int32_t max_h, int32_t max_w, int32_t R);
int cmh_image_preprocess(const uint8_t* pixels, const int64_t* offsets, const int32_t* hw, int32_t batch, int32_t max_h,
                         int32_t max_w, int32_t R, int32_t train, const float* mean, const float* stdv, float* out,
                         uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream);

/* ToTensor + Normalize of resized images that already live on the device (dataset/base.py:38-39 / :43-44 alone): u8 uint8
 * [N, R, R, 3]; rows (optional, device int64 [batch]) picks the images, else the first `batch`; out f32 [batch, 3, R, R].
 * Serves a device-resident cache of the resized dataset: identical floats to cmh_image_preprocess's, no decode / resize / PCIe. */
int cmh_image_normalize(const uint8_t* u8, const int64_t* rows, int32_t batch, int32_t R, const float* mean, const float* stdv,
                        float* out, void* stream);

/* ---- input pipeline, text side: host code, no GPU involved ------------------------------------------------
 * model/base/simple_tokenizer.py:62-79 (tables from the merges text: pass the gunzipped bpe_simple_vocab_16e6.txt) and
 * dataset/base.py:66-83 (_load_text) for n captions at once: clean -> lower -> split -> BPE -> [SOT] ids [EOT] cut to
 * max_words, zero padded, int64 [n, max_words].  texts = the captions' UTF-8 bytes back to back, offsets int64 [n + 1].
 * status[i] = 0: row i is filled; 1: caption i holds bytes outside printable ASCII / tab / CR / LF, or '&' — ftfy / html.unescape
 * territory — and must go through the Python path (row i is zeroed).  threads <= 0: one per hardware thread (at most 64). */
typedef struct cmh_bpe cmh_bpe;
int cmh_bpe_create(const char* merges_utf8, size_t bytes, cmh_bpe** out);
void cmh_bpe_destroy(cmh_bpe* tokenizer);
int32_t cmh_bpe_vocab_size(const cmh_bpe* tokenizer);
int cmh_bpe_encode_captions(const cmh_bpe* tokenizer, const char* texts, const int64_t* offsets, int32_t n, int32_t max_words,
                            int64_t* out, uint8_t* status, int32_t threads);

size_t cmh_vit_train_bytes(const cmh_vit_weights* w, int32_t batch);
/* same `feat` as cmh_vit_encode (c_fc's QuickGELU runs as a separate pass over the stored pre-activation) */
int cmh_vit_forward_train(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, void* tape, size_t tape_bytes,
                          void* stream);
int cmh_vit_backward(const cmh_vit_weights* w, int32_t batch, const float* dfeat, const cmh_vit_grads* grads, void* tape,
                     size_t tape_bytes, void* stream);
/* cmh_vit_backward in parts, for a data-parallel trainer that sends each bucket of gradients while the next part runs: one call
 * runs the head (ln_post, proj) iff layer_hi == layers, then blocks layer_hi-1 .. layer_lo, then the embeddings (ln_pre, positional,
 * class, conv1) iff layer_lo == 0; the gradient stream between parts stays in the tape.  Consecutive parts (layers..a, a..b, b..0)
 * on one tape write exactly the gradients of the one-call form; the parameters of a part are final when its call returns.
 * (Upstream: one loss.backward(), train/DSPH/hash_train.py:66.) */
int cmh_vit_backward_part(const cmh_vit_weights* w, int32_t batch, const float* dfeat, const cmh_vit_grads* grads, void* tape,
                          size_t tape_bytes, int32_t layer_hi, int32_t layer_lo, void* stream);
/* The same two calls for the MITH trunk (model/MITH.py:56-82): ln_post + proj on EVERY token.  tokens_out / dtokens f32
 * [batch * (g*g + 1), embed_dim] (row b*(g*g+1) is the class token); tape as for cmh_vit_forward_train. */
int cmh_vit_forward_train_tokens(const cmh_vit_weights* w, const float* image, int32_t batch, float* tokens_out, void* tape,
                                 size_t tape_bytes, void* stream);
int cmh_vit_backward_tokens(const cmh_vit_weights* w, int32_t batch, const float* dtokens, const cmh_vit_grads* grads, void* tape,
                            size_t tape_bytes, void* stream);
size_t cmh_text_train_bytes(const cmh_text_weights* w, int32_t batch, int32_t seq_len);
int cmh_text_forward_train(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                           const uint8_t* key_padding_mask, float* feat, void* tape, size_t tape_bytes, void* stream);
int cmh_text_backward(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                      const uint8_t* key_padding_mask, const float* dfeat, const cmh_text_grads* grads, void* tape,
                      size_t tape_bytes, void* stream);
/* cmh_text_backward in parts (see cmh_vit_backward_part): head = ln_final + text_projection, embeddings = token + positional. */
int cmh_text_backward_part(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                           const uint8_t* key_padding_mask, const float* dfeat, const cmh_text_grads* grads, void* tape,
                           size_t tape_bytes, int32_t layer_hi, int32_t layer_lo, void* stream);

/* CLIP1.encode_text of the MITH trunk under training (model/MITH.py:120-144): causal mask + key_padding_mask, every position is
 * run (no packing), ln_final + text_projection on every token.  tokens_out / dtokens f32 [batch * seq_len, embed_dim];
 * eot_rows_out i32 [batch] = b * seq_len + argmax(tokens[b]) (may be NULL). */
int cmh_text_forward_train_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                  const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out, void* tape,
                                  size_t tape_bytes, void* stream);
/* cmh_text_forward_train_tokens with the promise of cmh_text_encode_tokens_packed (then the padded positions' gradient is zero too):
 * tape and backward run on the kept rows; cmh_text_backward_tokens on this tape takes the dense [B*L, embed_dim] gradient as before
 * and ignores its padded rows. */
int cmh_text_forward_train_tokens_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                         const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out, void* tape,
                                         size_t tape_bytes, void* stream);
int cmh_text_backward_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                             const uint8_t* key_padding_mask, const float* dtokens, const cmh_text_grads* grads, void* tape,
                             size_t tape_bytes, void* stream);

/* ---- MITH HashingModel under training (model/MITH.py:217-453) -------------------------------------------------------------
 * A bare stack of ResidualAttentionBlocks (the concept transformer, :379-396) with a tape: x / y / dy / dx f32 [B*T, d]. */
size_t cmh_blocks_train_bytes(int32_t dtype, int32_t B, int32_t T, int32_t d, int32_t layers);
int cmh_blocks_forward_train(const cmh_block_weights* blocks, int32_t layers, int32_t dtype, const float* x, float* y, int32_t B,
                             int32_t T, int32_t d, void* tape, size_t tape_bytes, void* stream);
int cmh_blocks_backward(const cmh_block_weights* blocks, const cmh_block_grads* grads, int32_t layers, int32_t dtype,
                        const float* dy, float* dx, int32_t B, int32_t T, int32_t d, void* tape, size_t tape_bytes, void* stream);
/* Gradient of cmh_mith_lta w.r.t. the tokens (the similarities are detached upstream, :345): dtokens f32 [B, Ltot, D]. */
int cmh_mith_lta_backward(const float* sim, const uint8_t* key_padding_mask, const float* dmerge, float* dtokens, int32_t B,
                          int32_t Ltot, int32_t l0, int32_t L, int32_t K, int32_t D, int32_t top_k, void* stream);
/* nn.GELU() (exact, erf) and its backward, element-wise f32 (the ResidualMLPs' activation, :224-233). */
int cmh_gelu(const float* x, float* y, int64_t n, void* stream);
int cmh_gelu_backward(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* Backward of cmh_l2_normalize_rows (F.normalize, eps 1e-12) and of cmh_bitwise_hash (x [B,K,D], w [K,D], y = the forward output). */
int cmh_l2_normalize_backward(const float* x, const float* dy, float* dx, int32_t R, int32_t D, void* stream);
int cmh_bitwise_hash_backward(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* db,
                              int32_t B, int32_t K, int32_t D, void* stream);

/* Backward of the three MITH loss primitives (train/MITH/hash_train.py:103-147); dloss = device pointer to the upstream scalar
 * gradient (NULL = 1).  Bayesian: gradient w.r.t. the batch codes only (the bank holds detached codes).  InfoNCE: da, db f32
 * [R, D].  Squared difference: da / db f32 [n], either may be NULL. */
size_t cmh_mith_bayesian_backward_workspace_bytes(int32_t B, int32_t K);
int cmh_mith_bayesian_loss_backward(const float* bank, const float* batch, const float* bank_label, const float* label, int32_t Mb,
                                    int32_t B, int32_t K, int32_t C, const float* dloss, float* dbatch, void* workspace,
                                    size_t workspace_bytes, void* stream);
int cmh_info_nce_backward(const float* a, const float* b, int32_t R, int32_t G, int32_t D, float temperature, const float* dloss,
                          float* da, float* db, void* workspace, size_t workspace_bytes, void* stream);
int cmh_sq_diff_sum_backward(const float* a, const float* b, int64_t n, const float* dloss, float* da, float* db, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* CMH_H_ */
