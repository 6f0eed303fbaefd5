// C-ABI entry points of the two CLIP towers: kernel sequencing only (every kernel lives in gemm.hip,
// norm_embed.hip, attention.hip, heads.hip).  Nothing here allocates or synchronises: all launches go
// to the caller's stream and all scratch comes from the caller's workspace, so a whole encode is
// graph-capturable.
//
// Data layout in HBM (per call, M = B*T rows, d = width, e = GEMM element size 4|2):
//   x    f32 [M, d]    residual stream.  f32 mode: fp32 (the parity mode for the trainers' model.float()).
//                      bf16 mode (throughput): IEEE fp16, as a raw build_model CLIP keeps it on a GPU (convert_weights,
//                      model/base/model.py:391-412): halves the bytes of the 4 read-modify-write passes per layer
//                      (2 LayerNorms, 2 residual GEMMs).
//                      CMH_RESID_F16=0, widths that are not a multiple of 256 or a taps request keep it fp32.
//   h    e   [M, d]    LayerNorm output / attention output (GEMM A operand)
//   qkv  e   [M, 3d]   packed in_proj output            (vision: patch_out f32 [B*g2, d] aliases it)
//   mlp  e   [M, 4d]   c_fc output after QuickGELU      (vision: patches e [B*g2, pk] aliases it, pk = conv1_k: 3p^2 or padded)
//   rows i32 [B]       pooled row per sample (class token / EOT token)
//   pool e   [B, d]    ln_post / ln_final of the pooled rows
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "encoder_blocks.h"
#include "attention_pair.h"

namespace cmh {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

struct TowerBufs {
  float* x;
  void* h;
  void* qkv;
  void* mlp;
  int32_t* rows;
  void* pool;
  int32_t* seq;     // [B + 2] packed text: row offsets of the captions, seq[B] = the packed row count (read by the kernels themselves)
  void* conv1_w;    // vision, K-padded conv1 only: the weight with zero columns [d, pk] e
  size_t total;
};

static TowerBufs carve(void* ws, size_t M, size_t B, size_t d, size_t e, size_t extra_qkv, size_t extra_mlp, size_t conv1_w_bytes = 0) {
  Arena a(ws);
  TowerBufs t;
  t.x = a.take<float>(M * d * 4);
  t.h = a.take(M * d * e);
  size_t qkv_b = M * 3 * d * e, mlp_b = M * 4 * d * e;
  t.qkv = a.take(qkv_b > extra_qkv ? qkv_b : extra_qkv);
  t.mlp = a.take(mlp_b > extra_mlp ? mlp_b : extra_mlp);
  t.rows = a.take<int32_t>(B * 4);
  t.pool = a.take(B * d * e);
  t.seq = a.take<int32_t>((B + 2) * 4);
  t.conv1_w = a.take(conv1_w_bytes);
  t.total = a.off;
  return t;
}

static int tap(const cmh_taps* taps, int idx, const float* x, size_t bytes, hipStream_t st) {
  if (!taps || idx >= taps->count || !taps->ptrs[idx]) return CMH_OK;
  if (hipMemcpyAsync(taps->ptrs[idx], x, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "tap copy failed");
  return CMH_OK;
}

// ---- the block recipe -------------------------------------------------------------------------------------------------------------
// One ResidualAttentionBlock (model/base/model.py:191-196):
//   x += out_proj(attn(in_proj(ln_1(x))));  x += c_proj(QuickGELU(c_fc(ln_2(x))))
// This is the only statement of its launch sequence: inference and training, one tower or two in lock-step, every arithmetic mode,
// full-size or pooled tail are options of block_forward (fields of Lane, encoder_blocks.h), so that the paths the tests compare bit for
// bit run the same launches by construction.  The two stage helpers below hide the arithmetic mode and the tower count.
// fp8 mode (CMH_FP8): the four GEMMs on e4m3 operands.  Activations are quantised by their producers with the per-tensor
// scales of cmh_block_weights.act_scale (LayerNorm -> launch_layernorm_q, attention -> its fp8 store, QuickGELU -> the c_fc
// epilogue); the GEMM epilogues undo act_scale * colscale[n].  Residual stream fp16, qkv bf16 (attention is the bf16 kernel).
static int check_lane(const Lane& l) {
  CMH_CHECK_ARG(!l.amax || l.dtb == CMH_BF16, "fp8 calibration runs in bf16 mode");
  if (l.dtb != CMH_FP8) return CMH_OK;
  const cmh_block_weights& w = *l.w;
  const float* a = w.act_scale;
  CMH_CHECK_ARG(l.xh, "fp8 mode runs on the fp16 residual stream (width %% 256 == 0, no taps)");
  CMH_CHECK_ARG(w.in_proj_cs && w.out_proj_cs && w.fc_cs && w.proj_cs, "fp8 mode: weight scales missing");
  CMH_CHECK_ARG(a[0] > 0.f && a[1] > 0.f && a[2] > 0.f && a[3] > 0.f, "fp8 mode: activation scales missing (run the calibration pass)");
  return CMH_OK;
}

// GEMM operand i of a block: 0 ln_1's output, 1 the attention's, 2 ln_2's, 3 QuickGELU's.  fp8 mode: its producer stores
// e4m3(v * 1 / scale(i)), the GEMM that reads it multiplies scale(i) back (alpha); calibration: amax[i] is its running maximum.
enum { OP_LN1 = 0, OP_ATTN = 1, OP_LN2 = 2, OP_ACT = 3 };
static float scale(const Lane& l, int i) { return l.w->act_scale[i]; }
static int amax_stage(const Lane& l, int i, const void* v, size_t n, hipStream_t st) {
  return l.amax ? launch_amax(v, kBF16, n, l.amax + i, st) : CMH_OK;
}

struct Rows { int M; const int32_t* md; int mh; };     // a stage's row count: upper bound, the count on the device, its likely value
static Rows head_rows(const Lane& l) { return Rows{l.M, l.md, l.mh}; }
static Rows tail_rows(const Lane& l) { return l.pooled ? Rows{l.B, nullptr, -1} : head_rows(l); }

// LayerNorm stage (OP_LN1 | OP_LN2) of one tower or two
struct LnArgs { const void* x; const float *g, *b; void* out; Rows r; };
static LnArgs ln_args(const Lane& l, int op) {
  if (op == OP_LN1) return LnArgs{l.x_in, l.w->ln1_w, l.w->ln1_b, l.h1, head_rows(l)};
  return LnArgs{l.x_mid, l.w->ln2_w, l.w->ln2_b, l.h2, tail_rows(l)};
}
static int ln_stage(const Lane* const* L, int n, int op, hipStream_t st) {
  const LnArgs p = ln_args(*L[0], op);
  int rc = 1;
  if (n == 2 && L[0]->dtb == CMH_BF16 && L[0]->xh && L[1]->xh) {     // fp16 stream -> bf16 rows: both towers' rows in one launch
    const LnArgs q = ln_args(*L[1], op);
    rc = launch_layernorm_h2b_pair(p.x, p.g, p.b, p.out, p.r.M, L[0]->d, p.r.md, q.x, q.g, q.b, q.out, q.r.M, L[1]->d, q.r.md, st);
    if (rc < 0) return rc;
  }
  for (int i = 0; i < n; ++i) {
    const Lane& l = *L[i];
    const LnArgs a = i ? ln_args(l, op) : p;
    if (rc > 0) {      // (no pair kernel for these widths: one launch per tower)
      const int r1 = l.dtb == CMH_FP8 ? launch_layernorm_q(a.x, a.g, a.b, a.out, 1.0f / scale(l, op), a.r.M, l.d, st, a.r.md)
                                      : launch_layernorm_x(a.x, l.xh, nullptr, a.g, a.b, a.out, l.dtb == CMH_BF16, a.r.M, l.d, st, a.r.md);
      if (r1) return r1;
    }
    if (int r2 = amax_stage(l, op, a.out, static_cast<size_t>(a.r.M) * l.d, st)) return r2;
  }
  return CMH_OK;
}

// GEMM stage of one tower (launch_gemm / launch_gemm_fp8) or two (launch_gemm_grouped): everything about the four GEMMs in one table
enum { G_IN_PROJ, G_OUT_PROJ, G_FC, G_PROJ };
static bool fc_pre_fused(const Lane& l) {     // the N % 256 == 0 GEMM kernel stores the pre-activation from its epilogue
  static const bool fuse_act = []() { const char* e = getenv("CMH_FUSE_PRE"); return !(e && e[0] == '0'); }();
  return l.dtb == CMH_BF16 && (4 * l.d) % 256 == 0 && fuse_act;
}
static GemmProblem gemm_problem(const Lane& l, int which, int* epi) {
  const cmh_block_weights& w = *l.w;
  const bool q = l.dtb == CMH_FP8;
  const int d = l.d;
  const int obf = l.dtb == CMH_F32 ? 0 : EPI_OUT_BF16;
  const int rx = EPI_BIAS | EPI_RESIDUAL | (l.xh ? EPI_RES_F16 | EPI_OUT_F16 : 0);
  struct Row { const void* A; const void* W; const float* bias; const float* cs; const void* res; void* out; int N, K, op; float oscale; int epi; };
  const Row tab[4] = {
      {l.h1, w.in_proj_w, w.in_proj_b, w.in_proj_cs, nullptr, l.qkv, 3 * d, d, OP_LN1, 1.f, EPI_BIAS | obf},
      {l.pooled ? l.attn_p : l.attn, w.out_proj_w, w.out_proj_b, w.out_proj_cs, l.pooled ? l.x_mid : l.x_in, l.x_mid, d, d, OP_ATTN, 1.f, rx},
      {l.h2, w.fc_w, w.fc_b, w.fc_cs, nullptr, l.act, 4 * d, d, OP_LN2, q ? 1.0f / scale(l, OP_ACT) : 1.f,
       EPI_BIAS | EPI_QUICKGELU | (q ? EPI_OUT_FP8 : obf)},
      {l.act, w.proj_w, w.proj_b, w.proj_cs, l.x_mid, l.x_out, d, 4 * d, OP_ACT, 1.f, rx}};
  Row r = tab[which];
  if (which == G_FC && l.pre) {
    // training keeps c_fc's pre-activation.  One launch (EPI_SAVE_PRE): the activation from the f32 accumulator into act, the bf16
    // pre-activation into pre through the residual slot; else the GEMM writes pre and QuickGELU is a pass of its own (block_tail)
    if (fc_pre_fused(l)) { r.res = l.pre; r.epi |= EPI_SAVE_PRE; }
    else { r.out = l.pre; r.epi &= ~EPI_QUICKGELU; }
  }
  const Rows m = which == G_IN_PROJ ? head_rows(l) : tail_rows(l);
  *epi = r.epi;
  return GemmProblem{r.A, r.W, r.bias, static_cast<const float*>(r.res), r.out, m.M, r.N, r.K, m.md, m.mh, q ? r.cs : nullptr,
                     q ? scale(l, r.op) : 1.f, r.oscale};
}
static int gemm_stage(const Lane* const* L, int n, int which, hipStream_t st) {
  int epi = 0, epi_b = 0;
  const GemmProblem p = gemm_problem(*L[0], which, &epi);
  if (n == 2) return launch_gemm_grouped(L[0]->dtb, p, gemm_problem(*L[1], which, &epi_b), epi, st);
  if (L[0]->dtb == CMH_FP8)
    return launch_gemm_fp8(p.A, p.W, p.colscale, p.alpha, p.bias, p.residual, p.out, p.oscale, p.M, p.N, p.K, epi, st, p.m_dev, p.m_hint);
  return launch_gemm(L[0]->dtb, p.A, p.W, p.bias, p.residual, p.out, p.M, p.N, p.K, epi, st, p.m_dev, p.m_hint);
}

// everything behind the attention: row-wise, so on the pooled rows only where the lane says so
static int block_tail(const Lane* const* L, int n, hipStream_t st) {
  int rc;
  for (int i = 0; i < n; ++i) {
    const Lane& l = *L[i];
    const int xe = l.xh ? 2 : 4, e = l.dtb == CMH_FP8 ? 1 : l.dtb == CMH_BF16 ? 2 : 4;      // (fp8: the attention stored e4m3)
    if (l.pooled && (rc = launch_gather_rows2(l.x_in, l.x_mid, l.d * xe, l.attn, l.attn_p, l.d * e, l.pooled, l.B, st))) return rc;
  }
  if ((rc = gemm_stage(L, n, G_OUT_PROJ, st))) return rc;
  if ((rc = ln_stage(L, n, OP_LN2, st))) return rc;
  if ((rc = gemm_stage(L, n, G_FC, st))) return rc;
  for (int i = 0; i < n; ++i) {
    const Lane& l = *L[i];
    const size_t n_act = static_cast<size_t>(tail_rows(l).M) * 4 * l.d;
    if (l.pre && !fc_pre_fused(l) &&
        (rc = cmh_quick_gelu(l.pre, l.act, static_cast<int64_t>(n_act), l.dtb == CMH_BF16 ? kBF16 : kF32, st))) return rc;
    if ((rc = amax_stage(l, OP_ACT, l.act, n_act, st))) return rc;
  }
  return gemm_stage(L, n, G_PROJ, st);
}

// ---- both towers in lock-step (round 4: grouped launches) ---------------------------------------------------------------------------
// The image and the text tower are 12 blocks of the same four GEMMs (model/base/model.py:167-207, built twice by CLIP.__init__:
// :254-306); run one after the other - or on two streams - every GEMM is a launch of its own whose fixed third (first stage landing
// on 256 CUs at once, last tile's epilogue and store drain) the short-K text launches cannot amortise, and whose last round leaves
// CUs idle.  Here layer i of BOTH towers is one grouped launch of the wide kernel (gemm_wide.hip, GRP): ~50 GEMM launches per encoded
// batch instead of ~100, text tiles filling the image launches' last round.  Every output element sees the arithmetic of the
// single-tower path: the features are bit-identical (tests/test_gpu_grouped.py).
int block_forward(const Lane& a, const Lane* b, hipStream_t st) {
  const Lane* const L[2] = {&a, b};
  const int n = b ? 2 : 1;
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_lane(*L[i]))) return rc;
  CMH_CHECK_ARG(n == 1 || a.xh == b->xh,
                "block_forward: the towers' residual streams differ in kind (the caller runs such towers one by one)");
  if ((rc = ln_stage(L, n, OP_LN1, st))) return rc;
  if ((rc = gemm_stage(L, n, G_IN_PROJ, st))) return rc;
  // Both attentions as one launch where attention.hip has a pair kernel (bf16 forms, both T <= 80), else one launch per tower.  A
  // kernel has one register budget: round 4's pair ran the text side on six key tiles and with it every wave at 2 per SIMD (36.3 us
  // against 16.6 + 16.1, removed again); with the five-tile body both sides keep 3.  ViT-B/32 at batch 256, packed captions,
  // per layer in the serialized trace: 26.6 us against 33.6 for the two launches (profiles/r08_a_attention_pair_ab.txt)
  auto attn_problem = [](const Lane& l) {
    const bool q = l.dtb == CMH_FP8;
    return AttnProblem{l.qkv, l.attn, q ? CMH_BF16 : l.dtb, l.B, l.T, l.d, l.causal, l.kpm, l.seq_off, q ? 1.0f / scale(l, OP_ATTN) : 0.f};
  };
  int singly = 1;
  if (n == 2 && attention_pair_routed() && (singly = launch_attention_pair(attn_problem(a), attn_problem(*b), st)) < 0) return singly;
  for (int i = 0; i < n; ++i) {
    const Lane& l = *L[i];
    const AttnProblem p = attn_problem(l);
    if (singly && (rc = launch_attention_varlen(p.qkv, p.o, p.dt, p.B, p.T, p.d, p.causal, p.kpm, p.seq_off, st, p.o8_inv_scale))) return rc;
    if ((rc = amax_stage(l, OP_ATTN, l.attn, static_cast<size_t>(l.M) * l.d, st))) return rc;
  }
  if (n == 2 && (a.pooled || b->pooled)) {      // the rest of the last block on the pooled rows of each tower (few-row kernels)
    if ((rc = block_tail(&L[0], 1, st))) return rc;
    return block_tail(&L[1], 1, st);
  }
  return block_tail(L, n, st);
}

// The LAST block when only the pooled feature is wanted (encode_image / encode_text, model/base/model.py:247-250, 366-370): after its
// attention nothing mixes rows any more - out_proj, ln_2, the MLP, ln_post / ln_final and the projection are all row-wise - so only the
// B pooled rows (class token / EOT) are carried through them: three GEMMs of M = B instead of M = B*T.  Every kept row sees the
// arithmetic of the full-size path (same kernels, same K order), so the features are bit-identical.  The compact rows live in the qkv
// scratch, which is dead once the attention has run (pool_the_tail).
static int g_pooled_tail = -1;   // -1: from the environment (default on)
bool pooled_tail_enabled() {
  static const bool env_on = []() { const char* e = getenv("CMH_POOLED_TAIL"); return !(e && !strcmp(e, "0")); }();
  return g_pooled_tail < 0 ? env_on : g_pooled_tail != 0;
}

// CMH_TEXT_PACK_TOKENS=0 / cmh_set_text_token_packing(0): the all-token text trunk computes every position, as in rounds 1-4
static int g_pack_tokens = -1;
bool text_token_packing() {
  static const bool env_on = []() { const char* e = getenv("CMH_TEXT_PACK_TOKENS"); return !(e && !strcmp(e, "0")); }();
  return g_pack_tokens < 0 ? env_on : g_pack_tokens != 0;
}

// One tower of an encode call: its lane over the workspace buffers (one stream, updated in place)
struct TowerRun : Lane {
  TowerBufs t;
  bool packed_tokens = false;                            // packed text, every kept row is an output (the MITH trunk)
};
static void lane_in_place(TowerRun& r) {
  r.x_in = r.x_mid = r.x_out = r.t.x;
  r.h1 = r.attn = r.h2 = r.t.h;
  r.qkv = r.t.qkv;
  r.act = r.t.mlp;
}
// the pooled tail (above) for the block that runs next: the gathered residual rows [B, d] at the start of the qkv scratch - they
// become the block's output, x_out - and the gathered operand rows behind them
static void pool_the_tail(TowerRun& r) {
  char* scratch = static_cast<char*>(r.t.qkv);
  r.pooled = r.t.rows;
  r.x_mid = r.x_out = scratch;
  r.attn_p = r.h2 = scratch + align_up(static_cast<size_t>(r.B) * r.d * 4, 256);
}

// The packed row count of the LAST finished call for a (batch, seq_len), as a hint for the next call's tile heights: every call
// queues an asynchronous copy of its count into a pinned host word and records an event; the next call takes the value if that
// event has completed (hipEventQuery never blocks) and keeps its previous hint otherwise.  Results never depend on the hint.
namespace {
struct RowsHint { int B = 0, L = 0, hint = -1; int32_t* pinned = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
std::mutex g_hint_mu;
RowsHint g_hint;
}  // namespace
static int rows_hint_exchange(const int32_t* count_dev, int B, int L, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  RowsHint& h = g_hint;
  if (!h.pinned) {
    if (hipHostMalloc(reinterpret_cast<void**>(&h.pinned), 64, hipHostMallocDefault) != hipSuccess) { h.pinned = nullptr; return -1; }
    if (hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess) { h.ev = nullptr; return -1; }
  }
  if (!h.ev) return -1;
  if (h.pending && hipEventQuery(h.ev) == hipSuccess) {
    h.pending = false;
    if (h.B == B && h.L == L && *h.pinned > 0 && *h.pinned <= B * L) h.hint = *h.pinned;
  }
  const int out = (h.B == B && h.L == L) ? h.hint : -1;
  if (!h.pending) {          // one copy in flight at a time: the pinned word is not rewritten under a reader
    if (h.B != B || h.L != L) { h.B = B; h.L = L; h.hint = -1; }
    if (hipMemcpyAsync(h.pinned, count_dev, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(h.ev, st) == hipSuccess) h.pending = true;
  }
  return out;
}

int final_projection(int dt, const void* pool, const void* w_t, float* feat, int B, int embed, int d, hipStream_t st) {
  const int bk = dt == CMH_F32 ? 32 : 64;
  if (embed % 128 == 0 && d % bk == 0) return launch_gemm(dt, pool, w_t, nullptr, nullptr, feat, B, embed, d, 0, st);
  return launch_small_linear(dt, pool, w_t, nullptr, nullptr, 1.f, CMH_ACT_NONE, feat, B, embed, d, st);
}

int resid_f16(int dt, int d) {
  static const bool off = []() { const char* e = getenv("CMH_RESID_F16"); return e && !strcmp(e, "0"); }();
  return dt == CMH_BF16 && d % 256 == 0 && !off;
}
// ... of an inference tower: the fp8 mode always runs on it; taps are defined on an f32 stream
static int tower_xh(int dtb, int d, const cmh_taps* taps) {
  if (taps) return 0;
  return dtb == CMH_FP8 ? d % 256 == 0 : resid_f16(dtb, d);
}

// K-padded (conv1_k): the patch rows and a copy of the weight carry zero columns pk..pkp-1, which add exact zeros - the K = pk
// product in the same k order.
// keep_patches false (inference: nothing reads the patch matrix but this GEMM) and a shape conv1_stem.hip's kernel is built for: ONE
// launch whose loader waves build the patch tile from the image, `patches` untouched; the same bits in patch_out.
int conv1_stem(const cmh_vit_weights* w, int dt, const float* image, const float* image_b, int batch_a, int B, void* patches,
               bool keep_patches, void* conv1_w_pad, float* patch_out, hipStream_t st) {
  const int g = w->resolution / w->patch, g2 = g * g, d = w->width;
  const int pk = 3 * w->patch * w->patch, pkp = conv1_k(w->patch, dt);    // pkp != pk: the K-padded conv1
  const size_t e = dt == CMH_BF16 ? 2 : 4;
  int rc;
  if (image_b) CMH_CHECK_ARG(batch_a > 0 && batch_a < B, "vit_encode: split batch %d of %d", batch_a, B);
  if (!keep_patches && conv1_fused_enabled() && conv1_fused_takes(dt, w->patch, w->resolution, d))
    return launch_conv1_fused(image, image_b, batch_a, B, w->resolution, w->patch, w->conv1_w, patch_out, d, st);
  if (image_b) {
    if ((rc = launch_patchify(image, patches, dt, batch_a, w->resolution, w->patch, pkp, st))) return rc;
    if ((rc = launch_patchify(image_b, static_cast<char*>(patches) + static_cast<size_t>(batch_a) * g2 * pkp * e, dt, B - batch_a, w->resolution,
                              w->patch, pkp, st))) return rc;
  } else if ((rc = launch_patchify(image, patches, dt, B, w->resolution, w->patch, pkp, st))) return rc;
  const void* conv1_w = w->conv1_w;
  if (pkp != pk) {
    if ((rc = launch_copy_cols(w->conv1_w, pk, conv1_w_pad, pkp, d, pk, static_cast<int>(e), st))) return rc;
    conv1_w = conv1_w_pad;
  }
  return launch_gemm(dt, patches, conv1_w, nullptr, nullptr, patch_out, B * g2, d, pkp, 0, st);
}

static int check_tower(int dt, int width, int layers, int embed, const cmh_block_weights* blocks) {
  CMH_CHECK_ARG(dt == CMH_F32 || dt == CMH_BF16 || dt == CMH_FP8, "bad gemm_dtype %d", dt);
  CMH_CHECK_ARG(width > 0 && width % 128 == 0 && width <= 1024, "width %d must be a multiple of 128, <= 1024", width);
  CMH_CHECK_ARG(dt != CMH_FP8 || width % 256 == 0, "fp8 mode needs width %% 256 == 0 (width %d)", width);
  CMH_CHECK_ARG(layers >= 0 && embed > 0 && embed % 4 == 0, "bad layers/embed_dim");
  CMH_CHECK_ARG(layers == 0 || blocks, "blocks is null");
  return CMH_OK;
}

}  // namespace cmh

using namespace cmh;

extern "C" const char* cmh_last_error(void) { return err_buf(); }
extern "C" int cmh_set_pooled_tail(int32_t on) { g_pooled_tail = on ? 1 : 0; return CMH_OK; }
extern "C" int cmh_set_text_token_packing(int32_t on) {
  CMH_CHECK_ARG(on >= -1 && on <= 1, "set_text_token_packing: %d (-1 environment, 0 off, 1 on)", on);
  g_pack_tokens = on;
  return CMH_OK;
}
extern "C" int cmh_version(void) { return CMH_VERSION; }

extern "C" int cmh_vit_patch_embed(const cmh_vit_weights* w, const float* image, int32_t batch_a, const float* image_b, int32_t batch,
                                   int32_t keep_patches, void* scratch, size_t scratch_bytes, float* patch_out, void* stream) {
  CMH_CHECK_ARG(w && image && scratch && patch_out && batch > 0, "vit_patch_embed: null pointer or empty batch");
  CMH_CHECK_ARG(w->gemm_dtype == CMH_F32 || w->gemm_dtype == CMH_BF16 || w->gemm_dtype == CMH_FP8, "bad gemm_dtype %d", w->gemm_dtype);
  CMH_CHECK_ARG(w->patch > 0 && w->resolution % w->patch == 0 && w->width % 128 == 0, "vit_patch_embed: resolution %d / patch %d / width %d",
                w->resolution, w->patch, w->width);
  const int dt = w->gemm_dtype == CMH_FP8 ? CMH_BF16 : w->gemm_dtype;
  const size_t e = dt == CMH_BF16 ? 2 : 4, g = w->resolution / w->patch, pk = 3ull * w->patch * w->patch, pkp = conv1_k(w->patch, dt);
  Arena a(scratch);
  void* patches = a.take(static_cast<size_t>(batch) * g * g * pkp * e);
  void* w_pad = a.take(pkp != pk ? static_cast<size_t>(w->width) * pkp * e : 0);
  if (scratch_bytes < a.off) return fail(CMH_ERR_WORKSPACE, "vit_patch_embed: scratch %zu < %zu bytes", scratch_bytes, a.off);
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "vit_patch_embed: scratch must be 256-byte aligned");
  return conv1_stem(w, dt, image, image_b, batch_a, batch, patches, keep_patches != 0, w_pad, patch_out, as_stream(stream));
}

extern "C" size_t cmh_vit_workspace_bytes(const cmh_vit_weights* w, int32_t batch) {
  if (!w || batch <= 0 || w->patch <= 0) return 0;
  const size_t g = w->resolution / w->patch, g2 = g * g, T = g2 + 1, d = w->width;
  const size_t e = w->gemm_dtype == CMH_F32 ? 4 : 2;   // fp8 mode: sized like bf16 (conv1 and the stream are the bf16 mode's)
  const size_t B = batch, pk = 3ull * w->patch * w->patch, pkp = conv1_k(w->patch, w->gemm_dtype);
  // the patch matrix [B*g2, pkp] aliases the MLP buffer, which carve sizes for the larger of the two
  return carve(nullptr, B * T, B, d, e, B * g2 * d * 4, B * g2 * pkp * e, pkp != pk ? d * pkp * e : 0).total;
}

// validation + everything before the first block: conv1 as a patch-matrix GEMM, [class ; patches] + positional, ln_pre
// image_b / batch_a (cmh_clip_encode_pair2): the batch's images come as TWO tensors - rows [0, batch_a) from `image`, the rest from
// image_b - patchified into consecutive rows of the one patch matrix; nothing behind that knows.
static int vit_begin(const cmh_vit_weights* w, const float* image, int32_t batch, bool want_out, void* workspace, size_t workspace_bytes,
                     const cmh_taps* taps, hipStream_t st, float* amax, TowerRun& r, const float* image_b = nullptr, int32_t batch_a = 0) {
  CMH_CHECK_ARG(w && image && want_out && workspace, "vit_encode: null pointer");
  CMH_CHECK_ARG(batch > 0, "vit_encode: batch %d", batch);
  int rc = check_tower(w->gemm_dtype, w->width, w->layers, w->embed_dim, w->blocks);
  if (rc) return rc;
  CMH_CHECK_ARG(w->patch > 0 && w->resolution % w->patch == 0, "vit_encode: resolution %d / patch %d", w->resolution, w->patch);
  const int dtb = w->gemm_dtype, d = w->width, B = batch;   // dtb: arithmetic of the blocks' GEMMs
  const int dt = dtb == CMH_FP8 ? CMH_BF16 : dtb;             // everything outside the blocks (conv1, LayerNorms, projections)
  const int g = w->resolution / w->patch, g2 = g * g, T = g2 + 1, M = B * T;
  const int pk = 3 * w->patch * w->patch, pkp = conv1_k(w->patch, dt);    // pkp != pk: the K-padded conv1
  const size_t e = dt == CMH_BF16 ? 2 : 4;
  CMH_CHECK_ARG(!amax || dtb == CMH_BF16, "vit_calibrate_fp8: weights must be the bf16 mode's");
  CMH_CHECK_ARG(dtb != CMH_FP8 || pkp == pk, "fp8 mode: patch %d (3*patch^2 = %d) needs the K-padded conv1, which is not built for fp8",
                w->patch, pk);
  const size_t need = cmh_vit_workspace_bytes(w, batch);
  if (workspace_bytes < need) return fail(CMH_ERR_WORKSPACE, "vit_encode: workspace %zu < %zu bytes", workspace_bytes, need);
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "vit_encode: workspace must be 256-byte aligned");
  TowerBufs& t = r.t;
  t = carve(workspace, static_cast<size_t>(M), B, d, e, static_cast<size_t>(B) * g2 * d * 4, static_cast<size_t>(B) * g2 * pkp * e,
            pkp != pk ? static_cast<size_t>(d) * pkp * e : 0);
  r.dtb = dtb; r.xh = tower_xh(dtb, d, taps); r.d = d; r.B = B; r.T = T; r.M = M; r.causal = 0;
  lane_in_place(r);
  float* patch_out = static_cast<float*>(t.qkv);
  if ((rc = conv1_stem(w, dt, image, image_b, batch_a, B, /*patches=*/t.mlp, /*keep_patches=*/false, t.conv1_w, patch_out, st))) return rc;
  // [class ; patches] + positional, ln_pre  (:237-239)
  if ((rc = launch_vit_assemble_lnpre(patch_out, w->class_embedding, w->positional_embedding, w->ln_pre_w,
                                      w->ln_pre_b, t.x, r.xh, B, g2, d, st))) return rc;
  return tap(taps, 0, t.x, static_cast<size_t>(M) * d * 4, st);
}

// ln_post (+ proj) after the last block: on every token (MITH trunk) and / or on the class token
static int vit_finish(const cmh_vit_weights* w, const TowerRun& r, float* feat, float* tokens_out, hipStream_t st) {
  const TowerBufs& t = r.t;
  const void* x_pooled = r.pooled ? r.x_out : nullptr;      // the last block ran its tail on the pooled rows
  const int dt = r.dtb == CMH_FP8 ? CMH_BF16 : r.dtb, d = r.d, B = r.B, T = r.T, M = r.M;
  int rc;
  if (tokens_out) {
    // MITH trunk (model/MITH.py:70-80): ln_post and proj on EVERY token
    if ((rc = launch_layernorm_x(t.x, r.xh, nullptr, w->ln_post_w, w->ln_post_b, t.h, dt == CMH_BF16, M, d, st))) return rc;
    if ((rc = final_projection(dt, t.h, w->proj_t, tokens_out, M, w->embed_dim, d, st))) return rc;
  }
  if (feat) {
    // ln_post on the class token, @ proj  (:247-250)
    if (x_pooled) {
      if ((rc = launch_layernorm_x(x_pooled, r.xh, nullptr, w->ln_post_w, w->ln_post_b, t.pool, dt == CMH_BF16, B, d, st))) return rc;
    } else {
      if ((rc = launch_iota_rows(t.rows, B, T, st))) return rc;
      if ((rc = launch_layernorm_x(t.x, r.xh, t.rows, w->ln_post_w, w->ln_post_b, t.pool, dt == CMH_BF16, B, d, st))) return rc;
    }
    if ((rc = final_projection(dt, t.pool, w->proj_t, feat, B, w->embed_dim, d, st))) return rc;
  }
  return CMH_OK;
}

// every block of one tower, in place; pool_last: the last block's tail runs on the pooled rows only
static int run_tower(TowerRun& r, const cmh_block_weights* blocks, int layers, bool pool_last, float* amax, const cmh_taps* taps,
                     hipStream_t st) {
  int rc;
  for (int i = 0; i < layers; ++i) {
    r.w = &blocks[i];
    r.amax = amax ? amax + 4 * i : nullptr;
    if (pool_last && i == layers - 1) pool_the_tail(r);
    if ((rc = block_forward(r, nullptr, st))) return rc;
    if ((rc = tap(taps, 1 + i, r.t.x, static_cast<size_t>(r.B) * r.T * r.d * 4, st))) return rc;
  }
  return CMH_OK;
}

static int vit_encode_impl(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, float* tokens_out,
                           void* workspace, size_t workspace_bytes, const cmh_taps* taps, void* stream, float* amax = nullptr) {
  hipStream_t st = as_stream(stream);
  TowerRun r;
  int rc = vit_begin(w, image, batch, feat || tokens_out, workspace, workspace_bytes, taps, st, amax, r);
  if (rc) return rc;
  const bool tail = feat && !tokens_out && !taps && !amax && w->layers > 0 && pooled_tail_enabled();
  if (tail && (rc = launch_iota_rows(r.t.rows, r.B, r.T, st))) return rc;
  if ((rc = run_tower(r, w->blocks, w->layers, tail, amax, taps, st))) return rc;
  return vit_finish(w, r, feat, tokens_out, st);
}

extern "C" int cmh_vit_encode(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat,
                              void* workspace, size_t workspace_bytes, const cmh_taps* taps, void* stream) {
  CMH_CHECK_ARG(feat, "vit_encode: null pointer");
  return vit_encode_impl(w, image, batch, feat, nullptr, workspace, workspace_bytes, taps, stream);
}

extern "C" int cmh_vit_encode_tokens(const cmh_vit_weights* w, const float* image, int32_t batch, float* tokens_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "vit_encode_tokens: null pointer");
  return vit_encode_impl(w, image, batch, nullptr, tokens_out, workspace, workspace_bytes, nullptr, stream);
}

extern "C" size_t cmh_text_workspace_bytes(const cmh_text_weights* w, int32_t batch, int32_t seq_len) {
  if (!w || batch <= 0 || seq_len <= 0) return 0;
  const size_t e = w->gemm_dtype == CMH_F32 ? 4 : 2;
  return carve(nullptr, static_cast<size_t>(batch) * seq_len, batch, w->width, e, 0, 0).total;
}

// validation + everything before the first block: the pack plan (packed mode), token + positional embedding, the EOT rows
static int text_begin(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len, const uint8_t* key_padding_mask,
                      bool want_out, bool tokens_wanted, void* workspace, size_t workspace_bytes, const cmh_taps* taps, hipStream_t st,
                      bool packed, int32_t* rows_out, float* amax, TowerRun& r, bool pack_tokens_req = false) {   // rows_out: optional
  CMH_CHECK_ARG(w && tokens && want_out && workspace, "text_encode: null pointer");
  CMH_CHECK_ARG(batch > 0 && seq_len > 0, "text_encode: batch %d seq_len %d", batch, seq_len);
  int rc = check_tower(w->gemm_dtype, w->width, w->layers, w->embed_dim, w->blocks);
  if (rc) return rc;
  CMH_CHECK_ARG(seq_len <= w->context_length, "text_encode: seq_len %d > context_length %d", seq_len, w->context_length);
  const int dtb = w->gemm_dtype, d = w->width, B = batch, L = seq_len, M = B * L;
  const int dt = dtb == CMH_FP8 ? CMH_BF16 : dtb;
  const size_t e = dt == CMH_BF16 ? 2 : 4;
  CMH_CHECK_ARG(!amax || dtb == CMH_BF16, "text_calibrate_fp8: weights must be the bf16 mode's");
  const size_t need = cmh_text_workspace_bytes(w, batch, seq_len);
  if (workspace_bytes < need) return fail(CMH_ERR_WORKSPACE, "text_encode: workspace %zu < %zu bytes", workspace_bytes, need);
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "text_encode: workspace must be 256-byte aligned");
  TowerBufs& t = r.t;
  t = carve(workspace, static_cast<size_t>(M), B, d, e, 0, 0);
  r.xh = tower_xh(dtb, d, taps);
  lane_in_place(r);

  // Packed mode (pooled output only): under the causal mask nothing after a caption's EOT can reach the EOT row that
  // encode_text returns (model.py:366-370), so only the tokens 0..EOT of every caption are embedded and run through the
  // blocks - rows [seq_off[b], seq_off[b+1]) of one packed matrix; every kept row goes through exactly the arithmetic of
  // the dense path (row-wise kernels, per-row dot products, attention over the same key tiles), so the features are
  // bit-identical.  The row count is read back once (the GEMM grids need it on the host).
  const int32_t* seq_off = nullptr;
  const int32_t* md = nullptr;      // device-side row count of the packed matrix (the kernels read it themselves)
  int rows = M, mh = -1;
  // Round 5: the all-token trunk of MITH (model/MITH.py:120-144 returns every position; HashingModel gives the padded ones weight 0
  // in LocalizedTokenAggregation, :349-376, and reads them nowhere else) is packed too: a caption's rows run to its last unpadded
  // position, the projected tokens go back to their dense [B, L, E] places with zeros behind (text_finish).  Kept rows see the dense
  // path's arithmetic (the mask is still applied to the keys inside the kept prefix): same bits there.
  // (asked for per call - cmh_text_encode_tokens_packed: the caller promises not to read the padded positions - and only then)
  const bool pack_tokens = pack_tokens_req && tokens_wanted && key_padding_mask && !packed && !taps && !amax && text_token_packing() &&
                           w->embed_dim % 128 == 0 && d % (dt == CMH_F32 ? 32 : 64) == 0 &&      // the packed projection is a GEMM launch
                           static_cast<size_t>(w->embed_dim) * 4 <= static_cast<size_t>(4) * d * e;   // ... into the MLP scratch
  r.packed_tokens = pack_tokens;
  if (packed || pack_tokens) {
    CMH_CHECK_ARG(pack_tokens || (!key_padding_mask && !tokens_wanted && !taps), "text_encode_packed: pooled features only, no mask / taps");
    if ((rc = launch_text_pack_plan(tokens, B, L, t.seq, st, pack_tokens ? key_padding_mask : nullptr, pack_tokens ? t.rows : nullptr))) return rc;
    seq_off = t.seq;
    if (amax || d % 256 != 0 || !gemm_wide_enabled()) {
      // the calibration pass reduces over whole buffers on the host's row count, and widths that are not a multiple of 256 (the
      // test-sized towers) - or any width under the CMH_GEMM_WIDE=0 diagnostic - run on the 128 x 128 fallback GEMMs, which take
      // their row count from the host: these alone read the count back (one synchronisation)
      int32_t total = 0;
      if (hipMemcpyAsync(&total, t.seq + B, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(CMH_ERR_LAUNCH, "text_encode_packed: reading the packed row count failed");
      CMH_CHECK_ARG(total > 0 && total <= M, "text_encode_packed: bad packed row count %d", total);
      rows = total;
    } else {
      // LayerNorm and the GEMMs take M = B*L as an upper bound and read the real count from seq[B]; the tile height is chosen for
      // the count of an earlier call (rows_hint: captions of one dataset are alike), never waited for
      md = t.seq + B;
      mh = rows_hint_exchange(t.seq + B, B, L, st);
    }
    if (packed && rows_out && hipMemcpyAsync(rows_out, t.seq + B, 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "text_encode_packed: copying the row count failed");
  }

  // token_embedding gather + positional_embedding[:L]; EOT row = argmax(tokens)  (model.py:360-362,370)
  r.dtb = dtb; r.d = d; r.B = B; r.T = L; r.M = rows; r.causal = 1; r.kpm = key_padding_mask; r.seq_off = seq_off; r.md = md; r.mh = mh;
  return launch_text_embed_packed(tokens, w->token_embedding, w->positional_embedding, t.x, r.xh, t.rows, B, L, d, w->vocab_size, seq_off, st,
                                  pack_tokens);
}

// ln_final (+ text_projection) after the last block: on every token (MITH trunk) and / or on the EOT rows
static int text_finish(const cmh_text_weights* w, const TowerRun& r, float* feat, float* tokens_out, int32_t* eot_rows_out, hipStream_t st) {
  const TowerBufs& t = r.t;
  const void* x_pooled = r.pooled ? r.x_out : nullptr;      // the last block ran its tail on the pooled rows
  const int dt = r.dtb == CMH_FP8 ? CMH_BF16 : r.dtb, d = r.d, B = r.B, M = r.B * r.T;
  int rc;
  if (tokens_out && r.packed_tokens) {
    // the kept rows only (device row count), then back to their dense places; the EOT rows leave as dense indices with them
    float* tmp = static_cast<float*>(t.mlp);      // [rows, E] f32: the MLP scratch is free behind the last block (text_begin checked the sizes)
    if ((rc = launch_layernorm_x(t.x, r.xh, nullptr, w->ln_final_w, w->ln_final_b, t.h, dt == CMH_BF16, r.M, d, st, r.md))) return rc;
    if ((rc = launch_gemm(dt, t.h, w->text_projection_t, nullptr, nullptr, tmp, r.M, w->embed_dim, d, 0, st, r.md, r.mh))) return rc;
    if ((rc = launch_unpack_token_rows(tmp, r.seq_off, tokens_out, B, r.T, w->embed_dim, t.rows, eot_rows_out, st))) return rc;
  } else if (tokens_out) {
    // MITH trunk (model/MITH.py:136-139): ln_final and text_projection on EVERY token
    if ((rc = launch_layernorm_x(t.x, r.xh, nullptr, w->ln_final_w, w->ln_final_b, t.h, dt == CMH_BF16, M, d, st))) return rc;
    if ((rc = final_projection(dt, t.h, w->text_projection_t, tokens_out, M, w->embed_dim, d, st))) return rc;
  }
  if (eot_rows_out && !(tokens_out && r.packed_tokens) &&
      hipMemcpyAsync(eot_rows_out, t.rows, static_cast<size_t>(B) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "text_encode: eot row copy failed");
  if (feat) {
    // ln_final (row-wise, so only the pooled rows are normalised), @ text_projection  (:366-370)
    if ((rc = launch_layernorm_x(x_pooled ? x_pooled : t.x, r.xh, x_pooled ? nullptr : t.rows, w->ln_final_w, w->ln_final_b, t.pool,
                                 dt == CMH_BF16, B, d, st))) return rc;
    if ((rc = final_projection(dt, t.pool, w->text_projection_t, feat, B, w->embed_dim, d, st))) return rc;
  }
  return CMH_OK;
}

static int text_encode_impl(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                            const uint8_t* key_padding_mask, float* feat, float* tokens_out, int32_t* eot_rows_out,
                            void* workspace, size_t workspace_bytes, const cmh_taps* taps, void* stream,
                            bool packed = false, int32_t* rows_out = nullptr, float* amax = nullptr, bool pack_tokens_req = false) {
  hipStream_t st = as_stream(stream);
  TowerRun r;
  int rc = text_begin(w, tokens, batch, seq_len, key_padding_mask, feat || tokens_out, tokens_out != nullptr, workspace, workspace_bytes,
                      taps, st, packed, rows_out, amax, r, pack_tokens_req);
  if (rc) return rc;
  const bool tail = feat && !tokens_out && !taps && !amax && !eot_rows_out && w->layers > 0 && pooled_tail_enabled();
  if ((rc = run_tower(r, w->blocks, w->layers, tail, amax, taps, st))) return rc;
  return text_finish(w, r, feat, tokens_out, eot_rows_out, st);
}

extern "C" int cmh_text_encode(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                               const uint8_t* key_padding_mask, float* feat, void* workspace,
                               size_t workspace_bytes, const cmh_taps* taps, void* stream) {
  CMH_CHECK_ARG(feat, "text_encode: null pointer");
  return text_encode_impl(w, tokens, batch, seq_len, key_padding_mask, feat, nullptr, nullptr, workspace,
                          workspace_bytes, taps, stream);
}

extern "C" int cmh_text_encode_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len, float* feat,
                                      int32_t* rows_computed_dev, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(feat, "text_encode_packed: null pointer");
  return text_encode_impl(w, tokens, batch, seq_len, nullptr, feat, nullptr, nullptr, workspace, workspace_bytes, nullptr, stream,
                          /*packed=*/true, rows_computed_dev);
}

// encode_image + encode_text of one batch with the two towers in lock-step (reference model/modelbase.py:105-108 runs them back to
// back; model/base/model.py:340-372): layer i of both towers shares its launches (block_forward on two lanes).  Same features, bit for bit, as
// cmh_vit_encode + cmh_text_encode[_packed].
static int clip_encode_pair_impl(const cmh_vit_weights* vw, const float* image, const float* image_b, int32_t batch_a,
                                 const cmh_text_weights* tw, const int64_t* tokens,
                                 int32_t batch, int32_t seq_len, int32_t packed, float* feat_image, float* feat_text,
                                 int32_t* rows_computed_dev, void* ws_image, size_t ws_image_bytes, void* ws_text,
                                 size_t ws_text_bytes, void* stream) {
  CMH_CHECK_ARG(vw && tw && feat_image && feat_text, "clip_encode_pair: null pointer");
  CMH_CHECK_ARG(vw->gemm_dtype == tw->gemm_dtype, "clip_encode_pair: both towers must run in one arithmetic mode (%d / %d)", vw->gemm_dtype,
                tw->gemm_dtype);
  hipStream_t st = as_stream(stream);
  TowerRun a, b;
  int rc;
  if ((rc = vit_begin(vw, image, batch, true, ws_image, ws_image_bytes, nullptr, st, nullptr, a, image_b, batch_a))) return rc;
  if ((rc = text_begin(tw, tokens, batch, seq_len, nullptr, true, false, ws_text, ws_text_bytes, nullptr, st, packed != 0, rows_computed_dev,
                       nullptr, b))) return rc;
  const bool tail = pooled_tail_enabled();
  if (tail && vw->layers > 0 && (rc = launch_iota_rows(a.t.rows, a.B, a.T, st))) return rc;
  const int deepest = vw->layers > tw->layers ? vw->layers : tw->layers;
  for (int i = 0; i < deepest; ++i) {
    const bool has_a = i < vw->layers, has_b = i < tw->layers;
    const bool last_a = tail && i == vw->layers - 1, last_b = tail && i == tw->layers - 1;
    if (has_a) a.w = &vw->blocks[i];
    if (has_b) b.w = &tw->blocks[i];
    if (last_a) pool_the_tail(a);
    if (last_b) pool_the_tail(b);
    // lock-step only when both towers carry the same kind of residual stream (fp16 for widths that are multiples of 256 in the bf16
    // mode, else f32: resid_f16 decides per tower): a grouped launch has ONE set of epilogue flags
    if (has_a && has_b && last_a == last_b && a.xh == b.xh) {
      if ((rc = block_forward(a, &b, st))) return rc;
      continue;
    }
    if (has_a && (rc = block_forward(a, nullptr, st))) return rc;
    if (has_b && (rc = block_forward(b, nullptr, st))) return rc;
  }
  if ((rc = vit_finish(vw, a, feat_image, nullptr, st))) return rc;
  return text_finish(tw, b, feat_text, nullptr, nullptr, st);
}

extern "C" int cmh_clip_encode_pair(const cmh_vit_weights* vw, const float* image, const cmh_text_weights* tw, const int64_t* tokens,
                                    int32_t batch, int32_t seq_len, int32_t packed, float* feat_image, float* feat_text,
                                    int32_t* rows_computed_dev, void* ws_image, size_t ws_image_bytes, void* ws_text,
                                    size_t ws_text_bytes, void* stream) {
  return clip_encode_pair_impl(vw, image, nullptr, 0, tw, tokens, batch, seq_len, packed, feat_image, feat_text, rows_computed_dev, ws_image,
                               ws_image_bytes, ws_text, ws_text_bytes, stream);
}

// TWO loader batches as one: images as two tensors (batch_a + batch_b rows), the captions of both as one [batch_a + batch_b, seq_len]
// matrix.  Every row sees the arithmetic of cmh_clip_encode_pair on its own batch: the same features, half as many launches per pair.
extern "C" int cmh_clip_encode_pair2(const cmh_vit_weights* vw, const float* image_a, int32_t batch_a, const float* image_b, int32_t batch_b,
                                     const cmh_text_weights* tw, const int64_t* tokens, int32_t seq_len, int32_t packed,
                                     float* feat_image, float* feat_text, int32_t* rows_computed_dev, void* ws_image,
                                     size_t ws_image_bytes, void* ws_text, size_t ws_text_bytes, void* stream) {
  CMH_CHECK_ARG(image_a && image_b && batch_a > 0 && batch_b > 0, "clip_encode_pair2: two non-empty batches");
  return clip_encode_pair_impl(vw, image_a, image_b, batch_a, tw, tokens, batch_a + batch_b, seq_len, packed, feat_image, feat_text,
                               rows_computed_dev, ws_image, ws_image_bytes, ws_text, ws_text_bytes, stream);
}

extern "C" int cmh_linear_gemm_grouped(int32_t dtype, const cmh_gemm_problem* pa, const cmh_gemm_problem* pb, int32_t epilogue, void* stream) {
  CMH_CHECK_ARG(pa && pb, "linear_gemm_grouped: null pointer");
  CMH_CHECK_ARG(dtype == CMH_F32 || dtype == CMH_BF16 || dtype == CMH_FP8, "linear_gemm_grouped: bad dtype %d", dtype);
  auto conv = [](const cmh_gemm_problem* g) {
    return GemmProblem{g->x, g->w, g->bias, static_cast<const float*>(g->residual), g->out, g->M, g->N, g->K, g->m_dev, -1, g->colscale,
                       g->alpha, g->out_scale > 0.f ? 1.0f / g->out_scale : 1.0f};      // (out = e4m3(v / out_scale), as cmh_linear_gemm_fp8)
  };
  for (const cmh_gemm_problem* g : {pa, pb})
    CMH_CHECK_ARG(g->x && g->w && g->out && g->M > 0 && g->N > 0 && g->K > 0, "linear_gemm_grouped: null pointer / empty problem");
  return launch_gemm_grouped(dtype, conv(pa), conv(pb), epilogue, as_stream(stream));
}

extern "C" int cmh_vit_calibrate_fp8(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, float* amax,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(feat && amax, "vit_calibrate_fp8: null pointer");
  return vit_encode_impl(w, image, batch, feat, nullptr, workspace, workspace_bytes, nullptr, stream, amax);
}

extern "C" int cmh_text_calibrate_fp8(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len, float* feat,
                                      float* amax, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(feat && amax, "text_calibrate_fp8: null pointer");
  // the packed path: calibrate on the rows the fp8 mode will compute
  return text_encode_impl(w, tokens, batch, seq_len, nullptr, feat, nullptr, nullptr, workspace, workspace_bytes, nullptr, stream,
                          /*packed=*/true, nullptr, amax);
}

extern "C" int cmh_text_encode_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                      const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "text_encode_tokens: null pointer");
  return text_encode_impl(w, tokens, batch, seq_len, key_padding_mask, nullptr, tokens_out, eot_rows_out, workspace,
                          workspace_bytes, nullptr, stream);
}

// The same with the promise that nothing reads the padded positions of tokens_out (MITH: HashingModel masks them, model/MITH.py:349-376):
// positions behind a caption's last unpadded token are not computed and come back as zeros (cmh_set_text_token_packing)
extern "C" int cmh_text_encode_tokens_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                             const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "text_encode_tokens_packed: null pointer");
  return text_encode_impl(w, tokens, batch, seq_len, key_padding_mask, nullptr, tokens_out, eot_rows_out, workspace,
                          workspace_bytes, nullptr, stream, false, nullptr, nullptr, /*pack_tokens_req=*/true);
}

// A stack of ResidualAttentionBlocks on a caller-owned f32 residual stream x [B*T, d] (in place): the 2-layer
// concept transformer of MITH's LocalConceptTransforming (model/MITH.py:379-396 over model/MITH.py:11-46 blocks).
extern "C" size_t cmh_blocks_workspace_bytes(int32_t dtype, int32_t B, int32_t T, int32_t d) {
  if (B <= 0 || T <= 0 || d <= 0) return 0;
  return carve(nullptr, static_cast<size_t>(B) * T, B, d, dtype == CMH_BF16 ? 2 : 4, 0, 0).total;
}

extern "C" int cmh_transformer_blocks(const cmh_block_weights* blocks, int32_t layers, int32_t dtype, float* x, int32_t B,
                                      int32_t T, int32_t d, int32_t causal, const uint8_t* key_padding_mask,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(blocks && x && workspace && layers > 0 && B > 0 && T > 0, "transformer_blocks: bad arguments");
  CMH_CHECK_ARG(dtype != CMH_FP8, "transformer_blocks: f32 / bf16 only (the fp8 mode runs on the towers' fp16 residual stream)");
  int rc = check_tower(dtype, d, layers, 4, blocks);
  if (rc) return rc;
  if (workspace_bytes < cmh_blocks_workspace_bytes(dtype, B, T, d)) return fail(CMH_ERR_WORKSPACE, "transformer_blocks: workspace too small");
  hipStream_t st = as_stream(stream);
  const size_t M = static_cast<size_t>(B) * T;
  TowerRun r;
  r.t = carve(workspace, M, B, d, dtype == CMH_BF16 ? 2 : 4, 0, 0);
  r.dtb = dtype; r.d = d; r.B = B; r.T = T; r.M = B * T; r.causal = causal; r.kpm = key_padding_mask;
  lane_in_place(r);
  if (hipMemcpyAsync(r.t.x, x, M * d * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "transformer_blocks: copy failed");
  if ((rc = run_tower(r, blocks, layers, false, nullptr, nullptr, st))) return rc;
  if (hipMemcpyAsync(x, r.t.x, M * d * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "transformer_blocks: copy failed");
  return CMH_OK;
}

extern "C" int cmh_linear_gemm(int32_t dtype, const void* x, const void* w, const float* bias, const float* residual,
                               void* out, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream) {
  CMH_CHECK_ARG(x && w && out, "linear_gemm: null pointer");
  return launch_gemm(dtype, x, w, bias, residual, out, M, N, K, epilogue, as_stream(stream));
}

extern "C" int cmh_layernorm(const float* x, const float* w, const float* b, void* out, int32_t out_dtype, int32_t M,
                             int32_t d, void* stream) {
  CMH_CHECK_ARG(x && w && b && out && M > 0, "layernorm: bad arguments");
  return launch_layernorm(x, nullptr, w, b, out, out_dtype == CMH_BF16, M, d, as_stream(stream));
}

extern "C" int cmh_attention(int32_t dtype, const void* qkv, void* o, int32_t B, int32_t T, int32_t d, int32_t causal,
                             const uint8_t* key_padding_mask, void* stream) {
  CMH_CHECK_ARG(qkv && o, "attention: null pointer");
  CMH_CHECK_ARG(dtype == CMH_F32 || dtype == CMH_BF16, "attention: bad dtype");
  return launch_attention(qkv, o, dtype, B, T, d, causal, key_padding_mask, as_stream(stream));
}

extern "C" int cmh_attention_pair(int32_t dtype, const void* qkv0, void* o0, int32_t B0, int32_t T0, int32_t d0, int32_t causal0,
                                  const uint8_t* key_padding_mask0, const void* qkv1, void* o1, int32_t B1, int32_t T1, int32_t d1,
                                  int32_t causal1, const uint8_t* key_padding_mask1, void* stream) {
  CMH_CHECK_ARG(qkv0 && o0 && qkv1 && o1, "attention (pair): null pointer");
  CMH_CHECK_ARG(dtype == CMH_F32 || dtype == CMH_BF16, "attention (pair): bad dtype");
  CMH_CHECK_ARG(B0 > 0 && T0 > 0 && B1 > 0 && T1 > 0, "attention (pair): empty batch");
  CMH_CHECK_ARG(d0 > 0 && d0 % 64 == 0 && d1 > 0 && d1 % 64 == 0, "attention (pair): widths %d, %d are not multiples of 64", d0, d1);
  const AttnProblem p0{qkv0, o0, dtype, B0, T0, d0, causal0, key_padding_mask0, nullptr, 0.f};
  const AttnProblem p1{qkv1, o1, dtype, B1, T1, d1, causal1, key_padding_mask1, nullptr, 0.f};
  return launch_attention_pair(p0, p1, as_stream(stream));
}
