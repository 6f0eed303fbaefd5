// Training forward (keeps a tape) and backward of the two CLIP towers (SURVEY §8f "next" #2): kernel sequencing only.
//
// Forward with a tape = the forward of encoders.hip (the same block_forward, on lanes that point into the tape: tape_forward) with
// three differences: every block reads its input x_in and writes x_mid / the next block's x_in to fresh tape buffers instead of
// updating one stream in place (the residual GEMMs already take residual and output separately); c_fc also stores the
// PRE-activation (from its epilogue, or with QuickGELU as a pass of its own); LayerNorm and attention outputs are kept.  Per block the tape holds x_in, h1 = ln_1(x_in), qkv, attn, x_mid, h2 = ln_2(x_mid), pre:
// M*(2*xs*d + 10*e*d) bytes (xs = residual element size, e = GEMM element size): 236 MB per vision block at batch 256, bf16.
//
// Backward of one block, given dx = dL/dx_out (f32 gradient stream, updated in place to dL/dx_in).  With Y = X W^T + b:
//   dX = dY W          -> the forward GEMM kernel on (dY, W^T): W is transposed once per use (<= 4.7 MB);
//   dW = dY^T X        -> the same kernel on (dY^T, X^T): both activations are transposed (and cast to the GEMM dtype) first,
//                         zero-padded along M to the K-step; f32 output straight into the gradient buffer;
//   db = column sums of dY.
//   1. dpre = (dx W_proj) o QuickGELU'(pre)     [epilogue EPI_MUL_DQGELU]     dW_proj = dx^T gelu(pre),  db_proj = sum dx
//   2. dh2  = dpre W_fc                                                       dW_fc = dpre^T h2,        db_fc = sum dpre
//   3. dx  += LayerNorm_bwd(x_mid, dh2) (+ dln_2)
//   4. dattn = dx W_out                                                       dW_out = dx^T attn,       db_out = sum dx
//   5. dqkv = attention_bwd(qkv, attn, dattn)
//   6. dh1  = dqkv W_in                                                       dW_in = dqkv^T h1,        db_in = sum dqkv
//   7. dx  += LayerNorm_bwd(x_in, dh1) (+ dln_1)
// Gradients are WRITTEN (not accumulated) into caller-owned f32 buffers shaped like the reference's parameters.
// Host structure: TrainDims (a call's sizes) -> carve_train / open_tape / open_backward (the shared checks, the tape's slots); BlockRun (one
// tower's walk) -> tape_forward, blocks_backward (the per-layer rules) -> block_backward (its four Linears: one table; its scratch: BlockRed).
#include <cstring>
#include <mutex>
#include <vector>

#include "encoder_blocks.h"

namespace cmh {

namespace {

struct LayerTape { void *x_in, *h1, *qkv, *attn, *x_mid, *h2, *pre, *act; };   // act = QuickGELU(pre): c_proj's operand, kept for its wgrad

struct TrainBufs {
  std::vector<LayerTape> L;
  void* x_last;        // [M,d] xs   output of the last block
  void* patches;       // vision: [B*g2, pk] e   (pk = conv1_k: 3p^2, or padded with zero columns)
  float* x_pre;        // vision: [M,d] f32 tokens + positional before ln_pre;   text: unused
  float* patch_out;    // vision: [B*g2, d] f32
  int32_t* rows;       // [B] pooled row of every sample
  int32_t* seq_off;    // [B+1] packed text: row offsets of the captions (tokens 0..EOT only)
  void* pool;          // [B,d] e    ln_post / ln_final of the pooled rows
  // scratch
  float* dx;           // [M,d] f32 gradient stream
  float* dx2;          // [M,d] f32
  void* dxe;           // [M,d] e
  void* dpre;          // [M,4d] e
  float* part;         // split-K partial planes of the wgrad GEMMs (kPartBytes)
  void* dh;            // [M,d] e
  void* dqkv;          // [M,3d] e
  void* tA;            // [rmax, Mpad] e   dY^T
  void* tB;            // [rmax, Mpad] e   X^T
  void* wT;            // [max(12 d, rmax) * d] e   W^T of the block's four weight matrices (one launch), or of one head matrix
  void* tokE;          // [M, embed] e
  float* tokP;         // [M, embed] f32   packed all-token head: projected rows before they go to their dense places / packed dtokens
  float* projT;        // [embed, d] f32
  float* small;        // [2*B*max(d,E)] f32
  void* red;           // reduction workspace
  size_t red_bytes;
  size_t tAB_bytes;
  void* conv1_w;       // vision, K-padded conv1 only: [d, pk] e   the weight with zero columns
  float* conv1_dw;     // vision, K-padded conv1 only: [d, pk] f32 its gradient before the compaction to [d, 3p^2]
  size_t total;
};

size_t pad64(size_t m) { return (m + 63) / 64 * 64; }
constexpr size_t kPartBytes = static_cast<size_t>(256 + 64) * 160 * 256 * 4;      // split-K planes: <= one round of 160x256 f32 tiles
float* aligned_f32(void* p) {      // where a reduction's f32 partials start in a workspace: its first 256-byte boundary
  return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p) + 255) & ~static_cast<uintptr_t>(255));
}

// The sizes of one training call: every entry point (forward, backward, *_train_bytes) derives them here and opens its tape with them.
// e / xs: bytes of a GEMM operand / of a residual-stream element (xh: the fp16 stream); M = B * T rows; E: the head's width.
struct TrainDims {
  int dt, xh, B, T, M, d, E, layers;
  size_t e, xs, g2rows = 0;      // g2rows (vision): rows of the patch matrix
  int pk = 0, pkp = 0;           // vision: conv1's K = 3 p^2 and the K it runs with (conv1_k); pkp != pk: the K-padded conv1
  // a bare stack of blocks: f32 stream, no head (E = 4 keeps the head's slots at their smallest)
  TrainDims(int dtype, int B_, int T_, int d_, int layers_, int E_ = 4, int xh_ = 0)
      : dt(dtype), xh(xh_), B(B_), T(T_), M(B_ * T_), d(d_), E(E_), layers(layers_), e(dtype == CMH_BF16 ? 2 : 4), xs(xh_ ? 2 : 4) {}
  TrainDims(const cmh_text_weights* w, int batch, int seq_len)
      : TrainDims(w->gemm_dtype, batch, seq_len, w->width, w->layers, w->embed_dim, resid_f16(w->gemm_dtype, w->width)) {}
  TrainDims(const cmh_vit_weights* w, int batch)
      : TrainDims(w->gemm_dtype, batch, 1, w->width, w->layers, w->embed_dim, resid_f16(w->gemm_dtype, w->width)) {
    const int g = w->patch > 0 ? w->resolution / w->patch : 0;      // T = the patch grid + the class token
    T = g * g + 1, M = B * T, g2rows = static_cast<size_t>(B) * g * g, pk = 3 * w->patch * w->patch, pkp = conv1_k(w->patch, dt);
  }
};

// A block's six deferred reductions keep their partial sums side by side in t.red: 9 slices of a [M, d] bias gradient's partials
// (proj 1, fc 4, out 1, in 3), then the two LayerNorm workspaces.  carve_train sizes t.red for bytes(); block_backward reads the offsets.
struct BlockRed {
  size_t db_slice, ln_ws, proj, fc, out, in, ln2, ln1;
  BlockRed(int M, int d)
      : db_slice(align_up(static_cast<size_t>((M + 63) / 64) * d * 4 + 256, 256)), ln_ws(align_up(cmh_layernorm_backward_workspace_bytes(M, d), 256)),
        proj(0), fc(db_slice), out(5 * db_slice), in(6 * db_slice), ln2(9 * db_slice), ln1(ln2 + ln_ws) {}
  size_t bytes() const { return ln1 + ln_ws; }
};

TrainBufs carve_train(void* ws, const TrainDims& D) {
  const size_t M = static_cast<size_t>(D.B) * D.T, B = D.B, d = D.d, e = D.e, xs = D.xs, g2rows = D.g2rows, pk = D.pkp, embed = D.E;
  const bool conv1_padded = D.pkp != D.pk;
  Arena a(ws);
  TrainBufs t;
  t.L.resize(D.layers);
  for (int i = 0; i < D.layers; ++i) {
    t.L[i].x_in = a.take(M * d * xs);
    t.L[i].h1 = a.take(M * d * e);
    t.L[i].qkv = a.take(M * 3 * d * e);
    t.L[i].attn = a.take(M * d * e);
    t.L[i].x_mid = a.take(M * d * xs);
    t.L[i].h2 = a.take(M * d * e);
    t.L[i].pre = a.take(M * 4 * d * e);
    t.L[i].act = a.take(M * 4 * d * e);
  }
  t.x_last = a.take(M * d * xs);
  t.patches = a.take(g2rows * pk * e);
  t.x_pre = a.take<float>(g2rows ? M * d * 4 : 0);
  t.patch_out = a.take<float>(g2rows * d * 4);
  t.rows = a.take<int32_t>(B * 4);
  t.seq_off = a.take<int32_t>((B + 1) * 4);
  t.pool = a.take(B * d * e);
  t.dx = a.take<float>(M * d * 4);
  t.dx2 = a.take<float>(M * d * 4);
  t.dxe = a.take(M * d * e);
  t.dpre = a.take(M * 4 * d * e);
  t.part = a.take<float>(kPartBytes);
  t.dh = a.take(M * d * e);
  t.dqkv = a.take(M * 3 * d * e);
  size_t rmax = 4 * d > pk ? 4 * d : pk;
  rmax = rmax > embed ? rmax : embed;                       // the all-token head's wgrad / dgrad have `embed` rows
  const size_t mp = pad64(M > g2rows ? M : g2rows);
  t.tAB_bytes = rmax * mp * e;
  t.tA = a.take(t.tAB_bytes);
  t.tB = a.take(t.tAB_bytes);
  t.wT = a.take((12 * d > rmax ? 12 * d : rmax) * d * e);   // the four W^T of a block side by side (12 d^2), or one head matrix
  t.tokE = a.take(M * embed * e);                           // all-token head: dtokens as a GEMM operand
  t.tokP = a.take<float>(g2rows ? 0 : M * embed * 4);       // text only
  t.projT = a.take<float>(embed * d * 4);                   //                 d(proj^T) [embed, d] before its transpose
  const size_t wide = d > embed ? d : embed;
  t.small = a.take<float>(2 * B * wide * 4);
  size_t rb = cmh_layernorm_backward_workspace_bytes(static_cast<int>(M), static_cast<int>(d));
  const size_t cands[] = {cmh_colsum_workspace_bytes(static_cast<int>(M), static_cast<int>(4 * d)),
                          cmh_colsum_workspace_bytes(static_cast<int>(B), static_cast<int>((M / B) * d))};
  for (size_t c : cands) rb = c > rb ? c : rb;
  const size_t batched = BlockRed(static_cast<int>(M), static_cast<int>(d)).bytes();
  rb = batched > rb ? batched : rb;
  t.red_bytes = rb;
  t.red = a.take(rb);
  t.conv1_w = a.take(conv1_padded ? d * pk * e : 0);
  t.conv1_dw = a.take<float>(conv1_padded ? d * pk * 4 : 0);
  t.total = a.off;
  return t;
}

int check_train_tower(const TrainDims& D, const cmh_block_weights* blocks) {
  CMH_CHECK_ARG(D.dt == CMH_F32 || D.dt == CMH_BF16, "bad gemm_dtype %d", D.dt);
  CMH_CHECK_ARG(D.d > 0 && D.d % 128 == 0 && D.d <= 1024, "width %d must be a multiple of 128, <= 1024", D.d);
  CMH_CHECK_ARG(D.layers >= 0 && D.E > 0 && D.E % 4 == 0, "bad layers/embed_dim");
  CMH_CHECK_ARG(D.layers == 0 || blocks, "blocks is null");
  return CMH_OK;
}
// Entry point `what` opens its tape: it holds carve_train's total and, where the call fills it (need_aligned), is 256-byte aligned.
int open_tape(const char* what, const TrainDims& D, void* tape, size_t tape_bytes, bool need_aligned, TrainBufs* t) {
  if (tape_bytes < carve_train(nullptr, D).total) return fail(CMH_ERR_WORKSPACE, "%s: tape too small", what);
  CMH_CHECK_ARG(!need_aligned || (reinterpret_cast<uintptr_t>(tape) & 255) == 0, "%s: tape must be 256-byte aligned", what);
  *t = carve_train(tape, D);
  return CMH_OK;
}

// the last block's row-wise tail on the pooled rows only (tape_forward / block_backward): the rule both calls of a step apply,
// so cmh_set_pooled_tail must not change between a tape's forward and its backward; CMH_TRAIN_POOLED_TAIL=0 keeps the training
// towers on the full-size path
bool train_pooled_tail() {
  static const bool off = []() { const char* e = getenv("CMH_TRAIN_POOLED_TAIL"); return e && e[0] == '0'; }();
  return !off && pooled_tail_enabled();
}
int xkind(int xh) { return xh ? kF16 : kF32; }
int ekind(int dt) { return dt == CMH_BF16 ? kBF16 : kF32; }

// One tower's walk over its blocks, forward with a tape or backward: what no layer changes (the role Lane plays for block_forward).
struct BlockRun {
  const TrainDims& D; const cmh_block_weights* blocks; TrainBufs& t; hipStream_t st;
  int M;                                                                       // rows of the stream (a packed text tape: its packed row count)
  int causal = 0; const uint8_t* kpm = nullptr; const int32_t* seq_off = nullptr;      // text: the mask; packed rows: per-caption row offsets
  bool tail = false;                                                           // the last block's row-wise tail runs on the pooled rows t.rows only
};

// Every block of a tower with its tape: block i reads t.L[i].x_in and writes the next block's x_in (the last one t.x_last).
// r.tail (the LAST block of a tower whose only output is the pooled feature, like the inference towers' pooled tail): after the
// attention the block's row-wise tail - out_proj, ln_2, the MLP - runs on the B pooled rows only.  The tape slots then hold B-row
// matrices: x_mid, h2, pre, act rows [0, B); the pooled attention rows (out_proj's wgrad operand) sit in h2 rows [B, 2B); x_last
// receives B rows.  block_backward(..., pooled) reads them back the same way.
int tape_forward(const BlockRun& r) {
  const TrainDims& D = r.D;
  Lane base;
  base.dtb = D.dt; base.xh = D.xh; base.B = D.B; base.T = D.T; base.d = D.d;
  base.causal = r.causal; base.kpm = r.kpm; base.M = r.M; base.seq_off = r.seq_off;
  for (int i = 0; i < D.layers; ++i) {
    const LayerTape& L = r.t.L[i];
    Lane l = base;
    l.w = &r.blocks[i];
    l.x_in = L.x_in; l.h1 = L.h1; l.qkv = L.qkv; l.attn = L.attn; l.x_mid = L.x_mid; l.h2 = L.h2; l.pre = L.pre; l.act = L.act;
    l.x_out = i + 1 < D.layers ? r.t.L[i + 1].x_in : r.t.x_last;
    if (r.tail && i == D.layers - 1) {
      l.pooled = r.t.rows;
      l.attn_p = static_cast<char*>(L.h2) + static_cast<size_t>(D.B) * D.d * D.e;
    }
    if (int rc = block_forward(l, nullptr, r.st)) return rc;
  }
  return CMH_OK;
}

// dW[O, I] = dY^T X with dY [M, O] (kind ky) and X [M, I] (kind kx); db[O] = column sums of dY
struct WgradScratch { void* tA; void* tB; float* part; size_t part_bytes; void* red; size_t red_bytes; FinalJobs* defer = nullptr; };

// dYe (optional): dY as a bf16 GEMM operand when dY itself is f32 (the residual-stream gradient keeps both)
int wgrad_core(int dt, const void* dY, int ky, int O, const void* X, int kx, int I, int M, float* dW, float* db,
               const WgradScratch& w, hipStream_t st, const void* dYe = nullptr) {
  const int mp = static_cast<int>(pad64(M));
  int rc;
  // bf16 mode: dW = dY^T X straight from the row-major operands (TN GEMM, transposing LDS reads): no transposed copies
  const void* dYb = ky == kBF16 ? dY : dYe;
  if (dt == CMH_BF16 && kx == kBF16 && dYb && gemm_wide_tn_supported(O, I, M)) {
    // the bias gradient's first stage (column sums of dY per K split) is a by-product of the same launch
    float* dbp = aligned_f32(w.red);
    const bool cs = db && w.red_bytes >= static_cast<size_t>(64) * O * 4 + 256;
    int slices = 0;
    if ((rc = launch_gemm_wide_tn(dYb, X, dW, w.part, w.part_bytes, O, I, M, st, cs ? dbp : nullptr, &slices))) return rc;
    if (cs) {
      if (w.defer && w.defer->n < FinalJobs::kMax) w.defer->add(dbp, slices, O, db);
      else if ((rc = launch_colsum_final(dbp, slices, O, db, st))) return rc;
    } else if (db && (rc = cmh_colsum(dY, ky, M, O, db, w.red, w.red_bytes, st))) return rc;
    return CMH_OK;
  }
  // db = column sums of dY: their first stage rides on the transpose of dY when that takes the tiled path
  const bool fuse_db = db && transpose_is_vectorised(dY, w.tA, M, O, mp) && w.red_bytes >= static_cast<size_t>((M + 63) / 64) * O * 4 + 256;
  float* dbp = aligned_f32(w.red);
  if ((rc = launch_transpose(dY, ky, w.tA, ekind(dt), M, O, mp, st, fuse_db ? dbp : nullptr))) return rc;
  if (fuse_db && w.defer && w.defer->n < FinalJobs::kMax) w.defer->add(dbp, (M + 63) / 64, O, db);     // final stage queued
  else if (fuse_db && (rc = launch_colsum_final(dbp, (M + 63) / 64, O, db, st))) return rc;
  if ((rc = launch_transpose(X, kx, w.tB, ekind(dt), M, I, mp, st))) return rc;
  const int S = gemm_wide_splitk_plan(dt, O, I, mp);
  if (S > 1 && static_cast<size_t>(S) * O * I * 4 <= w.part_bytes) {
    // few output tiles, K = M rows: split K over S groups of workgroups, partial planes summed afterwards
    if ((rc = launch_gemm_wide_splitk(dt, w.tA, w.tB, dW, w.part, S, O, I, mp, st))) return rc;
  } else if ((rc = launch_gemm(dt, w.tA, w.tB, nullptr, nullptr, dW, O, I, mp, 0, st))) return rc;
  if (db && !fuse_db && (rc = cmh_colsum(dY, ky, M, O, db, w.red, w.red_bytes, st))) return rc;
  return CMH_OK;
}

int wgrad(int dt, const void* dY, int ky, int O, const void* X, int kx, int I, int M, float* dW, float* db, TrainBufs& t,
          hipStream_t st, FinalJobs* defer = nullptr, size_t red_off = 0, const void* dYe = nullptr) {
  return wgrad_core(dt, dY, ky, O, X, kx, I, M, dW, db,
                    WgradScratch{t.tA, t.tB, t.part, kPartBytes, static_cast<char*>(t.red) + red_off, t.red_bytes - red_off, defer}, st,
                    dYe);
}

int zero_pad_buffers(TrainBufs& t, size_t M, hipStream_t st) {
  if (pad64(M) == M) return CMH_OK;     // no padding columns: nothing to clear
  if (hipMemsetAsync(t.tA, 0, t.tAB_bytes, st) != hipSuccess || hipMemsetAsync(t.tB, 0, t.tAB_bytes, st) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "backward: memset failed");
  return CMH_OK;
}

static int g_grad_stream16 = -1;      // cmh_set_grad_stream16: -1 = from the environment (CMH_GRAD_STREAM16=0 switches it off)
bool grad_stream16_enabled() {
  static const bool env_on = []() { const char* e = getenv("CMH_GRAD_STREAM16"); return !(e && e[0] == '0'); }();
  return g_grad_stream16 < 0 ? env_on : g_grad_stream16 != 0;
}

// One of a block's four Linears, Y = X W^T + b over `rows` rows, as its backward needs it.  dY (kind ky) is what the bias gradient
// sums; dYe is the same gradient as a bf16 GEMM operand where dY itself is f32 (the residual stream keeps both).
struct BlockLinear {
  const void* W; int O, I;
  const void* dY; int ky; const void* dYe; const void* X; int rows;
  float *dW, *db;
  size_t red;                    // its bias partials in t.red (BlockRed)
  void* Wt;                      // W^T [I, O] in t.wT
  const void* operand() const { return dYe ? dYe : dY; }
};

// Block `layer`: t.dx holds dL/dx_out and leaves as dL/dx_in.  dxe_ready: the block before (or the all-token head) left its bf16 copy in t.dxe.
// pooled (the last block of a run with r.tail): the incoming gradient is t.dx2 [B, d] f32 on the pooled rows t.rows;
// steps 1-4 run on those B rows, then the two gradients that go on - d(attention output) and the residual stream - are scattered into
// zeroed full-size buffers for the attention backward and ln_1.
// keep_f32: the caller reads the f32 gradient stream (t.dx) behind this block (the embeddings' backward after block 0; the
// caller-visible dx of cmh_blocks_backward) - see the 16-bit stream below.
int block_backward(const BlockRun& r, int layer, const cmh_block_grads& g, bool dxe_ready, bool pooled, bool keep_f32) {
  const cmh_block_weights& w = r.blocks[layer];
  TrainBufs& t = r.t;
  const LayerTape& L = t.L[layer];
  hipStream_t st = r.st;
  const int dt = r.D.dt, B = r.D.B, d = r.D.d, M = r.M;
  const int Mt = pooled ? B : M;                       // rows of the row-wise tail (steps 1-4)
  float* dxt = pooled ? t.dx2 : t.dx;                  // its gradient stream
  const int obf = dt == CMH_BF16 ? EPI_OUT_BF16 : 0, ek = ekind(dt), xk = xkind(r.D.xh);
  const size_t esz = r.D.e, md = static_cast<size_t>(M) * d, mtd = static_cast<size_t>(Mt) * d;
  // bf16 mode: the LayerNorm backward kernels also leave the new dx as the bf16 GEMM operand (t.dxe)
  void* dx_copy = dt == CMH_BF16 ? t.dxe : nullptr;
  int rc;
  // The final stage of the block's six small reductions (four bias gradients, two LayerNorm parameter pairs) is queued and
  // launched once at the end of the block; their partial sums live side by side in t.red (BlockRed).
  FinalJobs jobs;
  const BlockRed R(M, d);
  const bool batched = R.bytes() <= t.red_bytes;
  FinalJobs* dj = batched ? &jobs : nullptr;
  char* red = static_cast<char*>(t.red);
  // The four Linears in the order the backward meets them; what concerns all four - the W^T launch, the one-launch wgrad and its fit
  // test, the per-layer wgrads, the bias jobs - is derived from this table.  (pooled: out_proj's X, the gathered attention rows, is
  // parked behind the first B rows of the h2 slot.  out_proj's dYe is filled in once ln_2's copy has its place.)
  const void* attn_rows = pooled ? static_cast<const char*>(L.h2) + static_cast<size_t>(B) * d * esz : L.attn;
  enum { kProj, kFc, kOut, kIn };
  BlockLinear lin[4] = {{w.proj_w, d, 4 * d, dxt, kF32, dx_copy, L.act, Mt, g.proj_w, g.proj_b, R.proj},
                        {w.fc_w, 4 * d, d, t.dpre, ek, nullptr, L.h2, Mt, g.fc_w, g.fc_b, R.fc},
                        {w.out_proj_w, d, d, dxt, kF32, nullptr, attn_rows, Mt, g.out_proj_w, g.out_proj_b, R.out},
                        {w.in_proj_w, 3 * d, d, t.dqkv, ek, nullptr, L.h1, M, g.in_proj_w, g.in_proj_b, R.in}};
  const void* wsrc[4];      // W^T of the four weight matrices side by side in t.wT, one launch
  void* wdst[4];
  int wR[4], wC[4];
  TnMultiJob probe[4];      // the one-launch wgrad's shapes
  char* wt = static_cast<char*>(t.wT);
  for (int j = 0; j < 4; ++j) {
    lin[j].Wt = wt;
    wt += static_cast<size_t>(lin[j].O) * lin[j].I * esz;
    wsrc[j] = lin[j].W; wdst[j] = lin[j].Wt; wR[j] = lin[j].O; wC[j] = lin[j].I;
    probe[j] = TnMultiJob{nullptr, nullptr, nullptr, nullptr, lin[j].O, lin[j].I, lin[j].rows};
  }
  if ((rc = launch_transpose_multi(wsrc, wdst, wR, wC, 4, ek, st))) return rc;
  if (pooled && (rc = zero_pad_buffers(t, static_cast<size_t>(B), st))) return rc;      // the tail's transposes are B rows wide
  // Round 4: the block's four weight gradients as ONE launch (gemm_wide.hip: gemm_wide_tn_multi_kernel), issued after the last dgrad
  // and before ln_1's backward: together they are one round of the chip with little or no K split, no partial planes, one launch's
  // fixed cost instead of four.  Their operands must all still be there at that point: the residual gradient as a GEMM operand exists
  // in two versions per block (at the block's entry: c_proj's dY; after ln_2: out_proj's), so ln_2's backward writes its copy to a
  // second buffer (t.dx2, otherwise only the pooled tail's) and ln_1's, as before, to t.dxe - the next block's entry.
  const bool multi = dt == CMH_BF16 && !pooled && batched && dx_copy && gemm_wide_tn_multi_enabled() && gemm_wide_tn_multi_fits(probe, 4) &&
                     R.db_slice >= static_cast<size_t>(64) * d * 4 + 256;
  void* dx_copy2 = multi ? static_cast<void*>(t.dx2) : dx_copy;      // where ln_2's backward leaves the bf16 copy of the new dx
  lin[kOut].dYe = dx_copy2;
  // Round 5: the 16-bit gradient stream.  The residual gradient is needed twice per block as a bf16 GEMM operand (c_proj's and
  // out_proj's dY) and twice as the sum a LayerNorm backward adds to; kept in f32 the two LayerNorm launches read AND write it
  // beside the bf16 copy they leave anyway (14 bytes per element: x 2, dy 2, dx 4 + 4, copy 2).  In the bf16 mode's multi-launch
  // blocks the bf16 copy IS the stream: ln_2 adds to the entry copy (t.dxe) and writes t.dx2, ln_1 adds to t.dx2 and writes t.dxe
  // - 8 bytes per element; the sum is formed in f32 and rounded to bf16 once per LayerNorm (24 roundings along a 12-block tower,
  // each 2^-9 relative: below what the bf16 GEMM operands already cost, tests/test_gpu_backward.py).  t.dx is written only where
  // somebody reads it (keep_f32).  The f32 mode, the pooled last block and CMH_GRAD_STREAM16=0 keep the f32 stream.
  const bool s16 = multi && grad_stream16_enabled();
  // one Linear's stage: dX [rows, I] = dY . W on (dY, W^T), through `epi` and typed like the GEMM operands; then - unless the one
  // launch takes all four - dW and db
  auto stage = [&](const BlockLinear& l, const void* aux, void* dX, int epi) {
    int rc = launch_gemm(dt, l.operand(), l.Wt, nullptr, static_cast<const float*>(aux), dX, l.rows, l.I, l.O, epi | obf, st);
    if (rc || multi) return rc;
    return wgrad(dt, l.dY, l.ky, l.O, l.X, ek, l.I, l.rows, l.dW, l.db, t, st, dj, batched ? l.red : 0, l.dYe);
  };
  // 1. MLP projection: the incoming gradient as a GEMM operand first (f32 mode: the stream itself)
  if (dx_copy && !dxe_ready && (rc = cmh_cast_f32_to_bf16(dxt, t.dxe, static_cast<int64_t>(mtd), st))) return rc;
  if ((rc = stage(lin[kProj], L.pre, t.dpre, EPI_MUL_DQGELU))) return rc;
  // 2. c_fc
  if ((rc = stage(lin[kFc], nullptr, t.dh, 0))) return rc;
  // 3. ln_2
  if ((rc = launch_layernorm_backward(L.x_mid, xk, t.dh, ek, w.ln2_w, nullptr, Mt, d, dxt, s16 ? 0 : 1, g.ln2_w, g.ln2_b,
                                      batched ? red + R.ln2 : red, batched ? R.ln_ws : t.red_bytes, st, dx_copy2, dj,
                                      s16 ? dx_copy : nullptr, !s16))) return rc;
  // 4. out_proj
  if ((rc = stage(lin[kOut], nullptr, t.dh, 0))) return rc;
  const void* dattn = t.dh;
  if (pooled) {
    // back to full size: d(attention output) is zero off the pooled rows (t.dxe is free now), the residual gradient likewise
    if (hipMemsetAsync(t.dxe, 0, md * esz, st) != hipSuccess || hipMemsetAsync(t.dx, 0, md * 4, st) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "backward: memset failed");
    if ((rc = launch_scatter_rows(t.dh, t.rows, t.dxe, B, static_cast<int>(d * esz), st))) return rc;
    if ((rc = launch_scatter_rows(t.dx2, t.rows, t.dx, B, d * 4, st))) return rc;
    dattn = t.dxe;
    if ((rc = zero_pad_buffers(t, static_cast<size_t>(M), st))) return rc;       // the B-row transposes left their rows in the padding
  }
  // 5. attention
  if ((rc = launch_attention_backward(dt, L.qkv, L.attn, dattn, t.dqkv, B, r.D.T, d, r.causal, r.kpm, r.seq_off, st))) return rc;
  // 6. in_proj
  if ((rc = stage(lin[kIn], nullptr, t.dh, 0))) return rc;
  if (multi) {
    TnMultiJob jobs4[4];
    for (int j = 0; j < 4; ++j)
      jobs4[j] = TnMultiJob{lin[j].operand(), lin[j].X, lin[j].dW, aligned_f32(red + lin[j].red), lin[j].O, lin[j].I, lin[j].rows};
    int slices[4] = {0, 0, 0, 0};
    if ((rc = launch_gemm_wide_tn_multi(jobs4, 4, t.part, kPartBytes, st, slices))) return rc;
    for (int j = 0; j < 4; ++j) jobs.add(jobs4[j].colsum, slices[j], lin[j].O, lin[j].db);
  }
  // 7. ln_1
  if ((rc = launch_layernorm_backward(L.x_in, xk, t.dh, ek, w.ln1_w, nullptr, M, d, t.dx, s16 ? 0 : 1, g.ln1_w, g.ln1_b,
                                      batched ? red + R.ln1 : red, batched ? R.ln_ws : t.red_bytes, st, dx_copy, dj,
                                      s16 ? dx_copy2 : nullptr, !s16 || keep_f32))) return rc;
  return launch_final_jobs(jobs, st);
}

// What every backward entry point `what` checks after its own arguments, in this order, then its tape: the layer range [lo, *hi)
// (*hi < 0: every layer), the tower, the head's gradient pointers (head_grads: the caller's null test of its own struct), the blocks'.
int open_backward(const char* what, const TrainDims& D, const cmh_block_weights* blocks, bool head_grads, const cmh_block_grads* grads,
                  void* tape, size_t tape_bytes, int* hi, int lo, TrainBufs* t) {
  if (*hi < 0) *hi = D.layers;
  CMH_CHECK_ARG(0 <= lo && lo <= *hi && *hi <= D.layers, "%s: layers [%d, %d) of %d", what, lo, *hi, D.layers);
  int rc = check_train_tower(D, blocks);
  if (rc) return rc;
  CMH_CHECK_ARG(head_grads && grads, "%s: null gradient pointer", what);
  for (int i = 0; i < D.layers; ++i) {
    const cmh_block_grads& p = grads[i];
    CMH_CHECK_ARG(p.in_proj_w && p.in_proj_b && p.out_proj_w && p.out_proj_b && p.ln1_w && p.ln1_b && p.ln2_w && p.ln2_b && p.fc_w &&
                  p.fc_b && p.proj_w && p.proj_b, "backward: block %d has a null gradient pointer", i);
  }
  return open_tape(what, D, tape, tape_bytes, /*need_aligned=*/false, t);
}

// Blocks hi-1 .. lo of a tower, last first, with the rules that depend on the layer: the LAST block finds a bf16 copy of its incoming
// gradient only behind the all-token head, and it alone runs the pooled tail; block 0 leaves the f32 stream for whoever comes after.
int blocks_backward(const BlockRun& r, const cmh_block_grads* grads, int hi, int lo, bool dtokens_head) {
  for (int i = hi - 1; i >= lo; --i) {
    const bool last = i == r.D.layers - 1;
    if (int rc = block_backward(r, i, grads[i], /*dxe_ready=*/!last || dtokens_head, /*pooled=*/r.tail && last, /*keep_f32=*/i == 0)) return rc;
  }
  return CMH_OK;
}

// ---- pooled rows: feat = LN(x_last[rows]) . proj ------------------------------------------------------------------------------
// dpool[b, i] = sum_j dfeat[b, j] * proj_t[j, i]   (dfeat row in LDS, 8 independent partial sums per thread; 32 chains or 8 rows per workgroup: 217 / 68-109 us against 72)
template <typename T>
__global__ __launch_bounds__(256) void pool_dgrad_kernel(const float* __restrict__ dfeat, const T* __restrict__ proj_t,
                                                         float* __restrict__ dpool, int B, int d, int E) {
  __shared__ float row[2048];
  const int b = blockIdx.x;
  constexpr int kind = sizeof(T) == 4 ? kF32 : kBF16;
  for (int j = threadIdx.x; j < E; j += 256) row[j] = dfeat[static_cast<size_t>(b) * E + j];
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += 256) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j + 8 <= E; j += 8)
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = fmaf(row[j + u], load_as_f32(proj_t, static_cast<size_t>(j + u) * d + i, kind), acc[u]);
    for (; j < E; ++j) acc[0] = fmaf(row[j], load_as_f32(proj_t, static_cast<size_t>(j) * d + i, kind), acc[0]);
    dpool[static_cast<size_t>(b) * d + i] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
}
// bf16 weights, d % 8 == 0: a thread owns 8 consecutive outputs and reads them as ONE 16-byte load per j (the kernel above issues a
// 2-byte load per output and j: 3 x 512 of them per thread in chains of 8 - 72 us at batch 256, and more of them in flight was slower,
// not faster).  Every output keeps the kernel above's arithmetic: chain u = j mod 8, the same final tree - same bits.
__global__ __launch_bounds__(128) void pool_dgrad_v8_kernel(const float* __restrict__ dfeat, const bf16_t* __restrict__ proj_t,
                                                            float* __restrict__ dpool, int B, int d, int E) {
  __shared__ float row[2048];
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < E; j += 128) row[j] = dfeat[static_cast<size_t>(b) * E + j];
  __syncthreads();
  for (int i8 = threadIdx.x; i8 < d / 8; i8 += 128) {
    float acc[8][8];                                   // [column][chain]
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[c][u] = 0.f;
    auto fma8 = [&](const uint4& q, float x, int u) __attribute__((always_inline)) {
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        acc[2 * h][u] = fmaf(x, __uint_as_float(w[h] << 16), acc[2 * h][u]);
        acc[2 * h + 1][u] = fmaf(x, __uint_as_float(w[h] & 0xffff0000u), acc[2 * h + 1][u]);
      }
    };
    int j = 0;
    for (; j + 8 <= E; j += 8) {
      uint4 q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = *reinterpret_cast<const uint4*>(proj_t + static_cast<size_t>(j + u) * d + i8 * 8);
#pragma unroll
      for (int u = 0; u < 8; ++u) fma8(q[u], row[j + u], u);
    }
    for (; j < E; ++j) fma8(*reinterpret_cast<const uint4*>(proj_t + static_cast<size_t>(j) * d + i8 * 8), row[j], 0);
#pragma unroll
    for (int c = 0; c < 8; ++c)
      dpool[static_cast<size_t>(b) * d + i8 * 8 + c] =
          ((acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3])) + ((acc[c][4] + acc[c][5]) + (acc[c][6] + acc[c][7]));
  }
}
// dproj[i, j] = sum_b pool[b, i] * dfeat[b, j]      (the reference's [width, embed_dim] parameter layout)
template <typename T>
__global__ __launch_bounds__(256) void pool_wgrad_kernel(const T* __restrict__ pool, const float* __restrict__ dfeat,
                                                         float* __restrict__ dproj, int B, int d, int E) {
  const int i = blockIdx.x;
  constexpr int kind = sizeof(T) == 4 ? kF32 : kBF16;
  for (int j = threadIdx.x; j < E; j += 256) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // eight independent chains over the batch (one chain: 137 us)
    int b = 0;
    for (; b + 8 <= B; b += 8)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        acc[u] = fmaf(load_as_f32(pool, static_cast<size_t>(b + u) * d + i, kind), dfeat[static_cast<size_t>(b + u) * E + j], acc[u]);
    for (; b < B; ++b) acc[0] = fmaf(load_as_f32(pool, static_cast<size_t>(b) * d + i, kind), dfeat[static_cast<size_t>(b) * E + j], acc[0]);
    dproj[static_cast<size_t>(i) * E + j] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
}

// A tower's head: its parameters (out = LN(rows of x_last) . proj) and, for the backward, where their gradients go
struct Head { const float *ln_w, *ln_b; const void* proj_t; float *dproj = nullptr, *dln_w = nullptr, *dln_b = nullptr; };

// compact = the forward carried only the pooled rows through the last block (x_last holds B rows): the gradient stays compact too,
// B rows of t.dx2, for block_backward(..., pooled).  M: rows of the gradient stream otherwise.
int pooled_backward(const TrainDims& D, TrainBufs& t, const Head& h, const float* dfeat, int M, bool compact, hipStream_t st) {
  const int dt = D.dt, B = D.B, d = D.d, E = D.E;
  const void *pool = t.pool, *proj_t = h.proj_t;
  float *dpool = t.small, *dproj = h.dproj;
  if (dt == CMH_F32) {
    hipLaunchKernelGGL(pool_dgrad_kernel<float>, dim3(B), dim3(256), 0, st, dfeat, static_cast<const float*>(proj_t), dpool, B, d, E);
    hipLaunchKernelGGL(pool_wgrad_kernel<float>, dim3(d), dim3(256), 0, st, static_cast<const float*>(pool), dfeat, dproj, B, d, E);
  } else {
    if (d % 8 == 0 && E <= 2048 && (reinterpret_cast<uintptr_t>(proj_t) & 15) == 0)
      hipLaunchKernelGGL(pool_dgrad_v8_kernel, dim3(B), dim3(128), 0, st, dfeat, static_cast<const bf16_t*>(proj_t), dpool, B, d, E);
    else
      hipLaunchKernelGGL(pool_dgrad_kernel<bf16_t>, dim3(B), dim3(256), 0, st, dfeat, static_cast<const bf16_t*>(proj_t), dpool, B, d, E);
    hipLaunchKernelGGL(pool_wgrad_kernel<bf16_t>, dim3(d), dim3(256), 0, st, static_cast<const bf16_t*>(pool), dfeat, dproj, B, d, E);
  }
  CMH_CHECK_LAUNCH("pooled projection backward");
  if (!compact && hipMemsetAsync(t.dx, 0, static_cast<size_t>(M) * d * 4, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "backward: memset failed");
  return launch_layernorm_backward(t.x_last, xkind(D.xh), dpool, kF32, h.ln_w, compact ? nullptr : t.rows, B, d, compact ? t.dx2 : t.dx, 0,
                                   h.dln_w, h.dln_b, t.red, t.red_bytes, st);
}

// token embedding: dE[token[r], :] += dx[r, :]
__global__ __launch_bounds__(256) void embed_scatter_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ dx,
                                                            float* __restrict__ dE, int rows, int d, int vocab) {
  const int r = blockIdx.x;
  int64_t id = tokens[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  for (int c = threadIdx.x; c < d; c += 256) atomicAdd(dE + static_cast<size_t>(id) * d + c, dx[static_cast<size_t>(r) * d + c]);
}

// packed text: the training tower follows encode_text's packing rule (no mask, CMH_TEXT_PACK != 0)
bool text_packing(const uint8_t* kpm) {
  static const bool off = []() { const char* e = getenv("CMH_TEXT_PACK"); return e && !strcmp(e, "0"); }();
  return !kpm && !off;
}

// dpos[t, :] = sum over the captions that have a token t of dx[seq_off[b] + t, :]   (deterministic: fixed caption order)
__global__ __launch_bounds__(256) void packed_dpos_kernel(const float* __restrict__ dx, const int32_t* __restrict__ seq_off, int B, int d,
                                                          float* __restrict__ dpos) {
  const int t = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  float acc = 0.f;
  // eight captions' rows in flight, added in caption order (one dependent load per caption made this 75 us of pure latency)
  int b = 0;
  for (; b + 8 <= B; b += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = seq_off[b + u];
      const bool has = t < seq_off[b + u + 1] - o;
      v[u] = has ? dx[static_cast<size_t>(o + t) * d + c] : 0.f;
      v[u] = has ? v[u] : -0.f;                                // (x + -0 == x for every x: a caption without token t adds nothing, bit for bit)
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; b < B; ++b) {
    const int o = seq_off[b];
    if (t < seq_off[b + 1] - o) acc += dx[static_cast<size_t>(o + t) * d + c];
  }
  dpos[static_cast<size_t>(t) * d + c] = acc;
}

// token embedding from packed rows: dE[tokens[b, t], :] += dx[seq_off[b] + t, :]
__global__ __launch_bounds__(256) void packed_embed_scatter_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ dx,
                                                                   const int32_t* __restrict__ seq_off, float* __restrict__ dE, int B,
                                                                   int L, int d, int vocab) {
  const int b = blockIdx.x / L, t = blockIdx.x - b * L;
  if (t >= seq_off[b + 1] - seq_off[b]) return;
  int64_t id = tokens[blockIdx.x];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const size_t r = static_cast<size_t>(seq_off[b] + t);
  for (int c = threadIdx.x; c < d; c += 256) atomicAdd(dE + static_cast<size_t>(id) * d + c, dx[r * d + c]);
}

}  // namespace
}  // namespace cmh

using namespace cmh;

// ================================================================================================================ wgrad
extern "C" size_t cmh_linear_wgrad_workspace_bytes(int32_t dtype, int32_t M, int32_t O, int32_t I) {
  if (M <= 0 || O <= 0 || I <= 0) return 0;
  const size_t e = dtype == CMH_BF16 ? 2 : 4, mp = pad64(static_cast<size_t>(M));
  return align_up(static_cast<size_t>(O) * mp * e, 256) + align_up(static_cast<size_t>(I) * mp * e, 256) + kPartBytes +
         align_up(cmh_colsum_workspace_bytes(M, O), 256) + 256;
}

extern "C" int cmh_linear_wgrad(int32_t dtype, const void* dy, int32_t dy_kind, const void* x, int32_t x_kind, int32_t M, int32_t O,
                                int32_t I, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(dy && x && dw && workspace && M > 0 && O > 0 && I > 0, "linear_wgrad: bad arguments");
  CMH_CHECK_ARG(dtype == CMH_F32 || dtype == CMH_BF16, "linear_wgrad: bad dtype");
  if (workspace_bytes < cmh_linear_wgrad_workspace_bytes(dtype, M, O, I)) return fail(CMH_ERR_WORKSPACE, "linear_wgrad: workspace too small");
  const size_t e = dtype == CMH_BF16 ? 2 : 4, mp = pad64(static_cast<size_t>(M));
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  WgradScratch w;
  w.tA = ws; ws += align_up(static_cast<size_t>(O) * mp * e, 256);
  w.tB = ws; ws += align_up(static_cast<size_t>(I) * mp * e, 256);
  w.part = reinterpret_cast<float*>(ws); w.part_bytes = kPartBytes; ws += kPartBytes;
  w.red = ws; w.red_bytes = cmh_colsum_workspace_bytes(M, O);
  hipStream_t st = as_stream(stream);
  if (mp != static_cast<size_t>(M) &&
      (hipMemsetAsync(w.tA, 0, static_cast<size_t>(O) * mp * e, st) != hipSuccess || hipMemsetAsync(w.tB, 0, static_cast<size_t>(I) * mp * e, st) != hipSuccess))
    return fail(CMH_ERR_LAUNCH, "linear_wgrad: memset failed");
  return wgrad_core(dtype, dy, dy_kind, O, x, x_kind, I, M, dw, db, w, st);
}

// ================================================================================================================ heads
// forward of either head over `rows` rows: out = LN(x_last, rows gathered by `gather` if given) . proj, the normalised rows through
// `normed`.  All-token head (MITH trunk, model/MITH.py:70-80,136-139): every row, through t.dxe (free during the forward pass);
// pooled head: the B pooled rows (tail: the last block left only those in x_last), through t.pool, which the backward reads.
static int head_forward(const TrainDims& D, const TrainBufs& t, const Head& h, const int32_t* gather, void* normed, float* out, int rows,
                        hipStream_t st) {
  int rc;
  if ((rc = launch_layernorm_x(t.x_last, D.xh, gather, h.ln_w, h.ln_b, normed, D.dt == CMH_BF16, rows, D.d, st))) return rc;
  return final_projection(D.dt, normed, h.proj_t, out, rows, D.E, D.d, st);
}
// all-token head, backward: dproj (reference layout [d, E]) = (dtok^T h)^T, dh = dtok . proj_t, then LayerNorm backward over every row into t.dx
// (+ its bf16 operand copy in t.dxe).  Scratch: h in t.dxe, dtok operand in t.tokE, dproj^T in t.projT.
static int tokens_head_backward(const TrainDims& D, TrainBufs& t, const Head& h, const float* dtok, int M, hipStream_t st) {
  const int dt = D.dt, d = D.d, E = D.E;
  int rc;
  if ((rc = launch_layernorm_x(t.x_last, D.xh, nullptr, h.ln_w, h.ln_b, t.dxe, dt == CMH_BF16, M, d, st))) return rc;   // h again
  if ((rc = wgrad(dt, dtok, kF32, E, t.dxe, ekind(dt), d, M, t.projT, nullptr, t, st))) return rc;                    // [E, d]
  if ((rc = launch_transpose(t.projT, kF32, h.dproj, kF32, E, d, E, st))) return rc;                                   // -> [d, E]
  const void* dtok_e = dt == CMH_BF16 ? t.tokE : static_cast<const void*>(dtok);      // dtok as a GEMM operand (f32 mode: itself)
  if (dt == CMH_BF16 && (rc = cmh_cast_f32_to_bf16(dtok, t.tokE, static_cast<int64_t>(M) * E, st))) return rc;
  if ((rc = launch_transpose(h.proj_t, ekind(dt), t.wT, ekind(dt), E, d, E, st))) return rc;                           // proj [d, E]
  if ((rc = launch_gemm(dt, dtok_e, t.wT, nullptr, nullptr, t.dh, M, d, E, dt == CMH_BF16 ? EPI_OUT_BF16 : 0, st))) return rc;
  return launch_layernorm_backward(t.x_last, xkind(D.xh), t.dh, ekind(dt), h.ln_w, nullptr, M, d, t.dx, 0, h.dln_w, h.dln_b, t.red,
                                   t.red_bytes, st, dt == CMH_BF16 ? t.dxe : nullptr);
}
// either head's backward over a gradient stream of M rows: dtokens [M, E] (all-token) or dfeat [B, E] (pooled; tail: pooled_backward)
static int head_backward(const TrainDims& D, TrainBufs& t, const Head& h, const float* dfeat, const float* dtokens, int M, bool tail, hipStream_t st) {
  return dtokens ? tokens_head_backward(D, t, h, dtokens, M, st) : pooled_backward(D, t, h, dfeat, M, tail, st);
}

// ================================================================================================================ vision
extern "C" size_t cmh_vit_train_bytes(const cmh_vit_weights* w, int32_t batch) {
  return !w || batch <= 0 || w->patch <= 0 ? 0 : carve_train(nullptr, TrainDims(w, batch)).total;
}

static int vit_forward_train_impl(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, float* tokens_out,
                                  void* tape, size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(w && image && (feat || tokens_out) && tape && batch > 0, "vit_forward_train: bad arguments");
  const TrainDims D(w, batch);      // D.pkp != D.pk: the K-padded conv1 (encoders.hip: vit_begin)
  int rc = check_train_tower(D, w->blocks);
  if (rc) return rc;
  CMH_CHECK_ARG(w->layers > 0, "vit_forward_train: no layers");
  CMH_CHECK_ARG(w->patch > 0 && w->resolution % w->patch == 0, "vit_forward_train: resolution / patch");
  TrainBufs t;
  if ((rc = open_tape("vit_forward_train", D, tape, tape_bytes, /*need_aligned=*/true, &t))) return rc;
  const int B = D.B, T = D.T, M = D.M, d = D.d;
  const Head head{w->ln_post_w, w->ln_post_b, w->proj_t};
  hipStream_t st = as_stream(stream);
  // (the tape keeps the patch matrix: conv1's weight gradient reads it)
  if ((rc = conv1_stem(w, D.dt, image, nullptr, 0, B, t.patches, /*keep_patches=*/true, t.conv1_w, t.patch_out, st))) return rc;
  // x_pre = [cls ; patches] + positional (kept for ln_pre's backward), x_0 = ln_pre(x_pre)
  if ((rc = launch_vit_assemble(t.patch_out, w->class_embedding, w->positional_embedding, t.x_pre, B, T - 1, d, st))) return rc;
  if ((rc = launch_layernorm_any(t.x_pre, kF32, nullptr, w->ln_pre_w, w->ln_pre_b, t.L[0].x_in, xkind(D.xh), M, d, st))) return rc;
  const bool tail = !tokens_out && train_pooled_tail();      // the same rule in vit_backward_impl
  if ((rc = launch_iota_rows(t.rows, B, T, st))) return rc;
  if ((rc = tape_forward(BlockRun{D, w->blocks, t, st, M, /*causal=*/0, nullptr, nullptr, tail}))) return rc;
  if (tokens_out) return head_forward(D, t, head, nullptr, t.dxe, tokens_out, M, st);
  return head_forward(D, t, head, tail ? nullptr : t.rows, t.pool, feat, B, st);
}

extern "C" int cmh_vit_forward_train(const cmh_vit_weights* w, const float* image, int32_t batch, float* feat, void* tape,
                                     size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(feat, "vit_forward_train: null feature pointer");
  return vit_forward_train_impl(w, image, batch, feat, nullptr, tape, tape_bytes, stream);
}

extern "C" int cmh_vit_forward_train_tokens(const cmh_vit_weights* w, const float* image, int32_t batch, float* tokens_out,
                                            void* tape, size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "vit_forward_train_tokens: null output pointer");
  return vit_forward_train_impl(w, image, batch, nullptr, tokens_out, tape, tape_bytes, stream);
}

// layer_hi / layer_lo: the part of the backward pass this call runs - the head (ln_post, proj) iff layer_hi == layers, then blocks
// layer_hi-1 .. layer_lo, then the embeddings (ln_pre, positional, class, conv1) iff layer_lo == 0.  The gradient stream between
// parts lives in the tape, so consecutive parts (layers .. a, a .. b, b .. 0) equal the one-call form bit for bit; each part's
// parameter gradients are final when it returns (a data-parallel trainer sends that bucket while the next part runs).
static int vit_backward_impl(const cmh_vit_weights* w, int32_t batch, const float* dfeat, const float* dtokens, const cmh_vit_grads* gr,
                             void* tape, size_t tape_bytes, void* stream, int layer_hi = -1, int layer_lo = 0) {
  CMH_CHECK_ARG(w && (dfeat || dtokens) && gr && tape && batch > 0, "vit_backward: bad arguments");
  const TrainDims D(w, batch);
  const bool head_grads = gr->conv1_w && gr->class_embedding && gr->positional_embedding && gr->ln_pre_w && gr->ln_pre_b && gr->ln_post_w &&
                          gr->ln_post_b && gr->proj;
  TrainBufs t;
  int rc = open_backward("vit_backward", D, w->blocks, head_grads, gr->blocks, tape, tape_bytes, &layer_hi, layer_lo, &t);
  if (rc) return rc;
  const int dt = D.dt, B = D.B, T = D.T, M = D.M, d = D.d, g2 = T - 1, pk = D.pk, pkp = D.pkp;
  hipStream_t st = as_stream(stream);
  BlockRun run{D, w->blocks, t, st, M};
  run.tail = !dtokens && train_pooled_tail();
  if (layer_hi == w->layers) {
    if ((rc = zero_pad_buffers(t, static_cast<size_t>(M), st))) return rc;
    if ((rc = head_backward(D, t, Head{w->ln_post_w, w->ln_post_b, w->proj_t, gr->proj, gr->ln_post_w, gr->ln_post_b}, dfeat, dtokens, M,
                            run.tail, st))) return rc;
  }
  if ((rc = blocks_backward(run, gr->blocks, layer_hi, layer_lo, dtokens != nullptr))) return rc;
  if (layer_lo > 0) return CMH_OK;
  // ln_pre, then the embeddings: x_pre[b,0] = cls + pos[0], x_pre[b,1+i] = patch_out[b*g2+i] + pos[1+i]
  if ((rc = launch_layernorm_backward(t.x_pre, kF32, t.dx, kF32, w->ln_pre_w, nullptr, M, d, t.dx2, 0, gr->ln_pre_w, gr->ln_pre_b,
                                      t.red, t.red_bytes, st))) return rc;
  if ((rc = cmh_colsum(t.dx2, kF32, B, T * d, gr->positional_embedding, t.red, t.red_bytes, st))) return rc;
  if (hipMemcpyAsync(gr->class_embedding, gr->positional_embedding, static_cast<size_t>(d) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "vit_backward: copy failed");
  // conv1: dW[d, pk] = dpatch_out^T patches, dpatch_out = the non-class rows of dx2 (compacted into dx)
  if (hipMemcpy2DAsync(t.dx, static_cast<size_t>(g2) * d * 4, t.dx2 + d, static_cast<size_t>(T) * d * 4, static_cast<size_t>(g2) * d * 4,
                       B, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "vit_backward: compaction failed");
  if ((rc = zero_pad_buffers(t, static_cast<size_t>(B) * g2, st))) return rc;
  if (pkp == pk) return wgrad(dt, t.dx, kF32, d, t.patches, ekind(dt), pk, B * g2, gr->conv1_w, nullptr, t, st);
  // K-padded conv1: dW [d, pkp] into scratch (its pad columns are dY^T . 0), then the caller's [d, 3, p, p] = its first pk columns -
  // the gradient is a view into the trainer's flat gradient buffer, so exactly d * pk contiguous floats are written
  if ((rc = wgrad(dt, t.dx, kF32, d, t.patches, ekind(dt), pkp, B * g2, t.conv1_dw, nullptr, t, st))) return rc;
  return launch_copy_cols(t.conv1_dw, pkp, gr->conv1_w, pk, d, pk, 4, st);
}

extern "C" int cmh_set_grad_stream16(int32_t on) {
  CMH_CHECK_ARG(on >= -1 && on <= 1, "set_grad_stream16: %d (-1 environment, 0 off, 1 on)", on);
  g_grad_stream16 = on;
  return CMH_OK;
}

extern "C" int cmh_vit_backward(const cmh_vit_weights* w, int32_t batch, const float* dfeat, const cmh_vit_grads* gr, void* tape,
                                size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(dfeat, "vit_backward: null gradient");
  return vit_backward_impl(w, batch, dfeat, nullptr, gr, tape, tape_bytes, stream);
}

extern "C" int cmh_vit_backward_part(const cmh_vit_weights* w, int32_t batch, const float* dfeat, const cmh_vit_grads* gr, void* tape,
                                     size_t tape_bytes, int32_t layer_hi, int32_t layer_lo, void* stream) {
  CMH_CHECK_ARG(dfeat && layer_hi >= 0, "vit_backward_part: bad arguments");
  return vit_backward_impl(w, batch, dfeat, nullptr, gr, tape, tape_bytes, stream, layer_hi, layer_lo);
}

extern "C" int cmh_vit_backward_tokens(const cmh_vit_weights* w, int32_t batch, const float* dtokens, const cmh_vit_grads* gr,
                                       void* tape, size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(dtokens, "vit_backward_tokens: null gradient");
  return vit_backward_impl(w, batch, nullptr, dtokens, gr, tape, tape_bytes, stream);
}

// ================================================================================================================ text
// The packed row count of a text tape (the GEMM grids need it on the host): text_forward_train reads it back once and remembers
// it here, keyed by the tape's address, so that the backward call(s) on the same tape need no stream synchronisation of their own.
namespace {
std::mutex g_tape_rows_mu;
struct { const void* tape; int rows; } g_tape_rows[64];      // a ring: the OLDEST entry goes when a new tape comes - tapes of long-gone
size_t g_tape_next = 0;                                       // steps; a forward's entry outlives the 63 forwards after it
void remember_tape_rows(const void* tape, int rows) {
  std::lock_guard<std::mutex> lk(g_tape_rows_mu);
  for (auto& e : g_tape_rows)
    if (e.tape == tape) { e.rows = rows; return; }
  g_tape_rows[g_tape_next++ % 64] = {tape, rows};
}
int recall_tape_rows(const void* tape) {
  std::lock_guard<std::mutex> lk(g_tape_rows_mu);
  for (const auto& e : g_tape_rows)
    if (e.tape == tape) return e.rows;
  return -1;
}
// The packed row count of a tape for the call `what`: the count the forward call remembered (no synchronisation here); for a tape this
// process did not fill (or tape == nullptr: the forward call itself) a synchronous read-back of the plan's seq_off[B]; then the range
// check.  dense_ok: 0 is an answer too - an all-token tape filled densely (its forward remembered 0 and zeroed seq_off).
int tape_packed_rows(const char* what, const void* tape, const TrainBufs& t, const TrainDims& D, bool dense_ok, hipStream_t st, int* rows) {
  int32_t total = tape ? recall_tape_rows(tape) : -1;
  if (total < 0 && (hipMemcpyAsync(&total, t.seq_off + D.B, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
    return fail(CMH_ERR_LAUNCH, "%s: reading the packed row count failed", what);
  CMH_CHECK_ARG(total >= (dense_ok ? 0 : 1) && total <= D.M, "%s: the tape holds a bad packed row count %d (of %d rows)", what, total, D.M);
  *rows = total;
  return CMH_OK;
}
}  // namespace

extern "C" size_t cmh_text_train_bytes(const cmh_text_weights* w, int32_t batch, int32_t seq_len) {
  return !w || batch <= 0 || seq_len <= 0 ? 0 : carve_train(nullptr, TrainDims(w, batch, seq_len)).total;
}

static int text_forward_train_impl(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                   const uint8_t* key_padding_mask, float* feat, float* tokens_out, int32_t* eot_rows_out, void* tape,
                                   size_t tape_bytes, void* stream, bool pack_tokens_req = false) {
  CMH_CHECK_ARG(w && tokens && (feat || tokens_out) && tape && batch > 0 && seq_len > 0, "text_forward_train: bad arguments");
  const TrainDims D(w, batch, seq_len);
  int rc = check_train_tower(D, w->blocks);
  if (rc) return rc;
  CMH_CHECK_ARG(w->layers > 0 && seq_len <= w->context_length, "text_forward_train: layers / seq_len");
  TrainBufs t;
  if ((rc = open_tape("text_forward_train", D, tape, tape_bytes, /*need_aligned=*/true, &t))) return rc;
  const int dt = D.dt, xh = D.xh, B = D.B, L = D.T, M = D.M, d = D.d;
  const Head head{w->ln_final_w, w->ln_final_b, w->text_projection_t};
  hipStream_t st = as_stream(stream);
  // packed like encode_text (encoders.hip): only the tokens 0..EOT of every caption are run through the blocks (run.M of them)
  BlockRun run{D, w->blocks, t, st, M, /*causal=*/1, key_padding_mask};
  // the all-token trunk (MITH): packed only on the caller's word that the padded positions of tokens_out are read by nobody
  // (cmh_text_forward_train_tokens_packed; encoders.hip text_begin has the reasoning) - their gradient is then exactly zero as well
  const int bk0 = dt == CMH_F32 ? 32 : 64;
  const bool pack_tokens = tokens_out && pack_tokens_req && key_padding_mask && text_token_packing() && w->embed_dim % 128 == 0 && d % bk0 == 0;
  if (tokens_out && !pack_tokens) remember_tape_rows(tape, 0);      // 0: this tape's all-token head is dense (text_backward_impl)
  if ((!tokens_out && text_packing(key_padding_mask)) || pack_tokens) {
    if ((rc = launch_text_pack_plan(tokens, B, L, t.seq_off, st, pack_tokens ? key_padding_mask : nullptr, pack_tokens ? t.rows : nullptr))) return rc;
    // the producer of the count: its own read (tape = nullptr: nothing to recall), through the check every reader applies
    if ((rc = tape_packed_rows("text_forward_train", nullptr, t, D, /*dense_ok=*/false, st, &run.M))) return rc;
    run.seq_off = t.seq_off;
    remember_tape_rows(tape, run.M);
  }
  if ((rc = launch_text_embed_packed(tokens, w->token_embedding, w->positional_embedding, t.L[0].x_in, xh, t.rows, B, L, d,
                                     w->vocab_size, run.seq_off, st, pack_tokens))) return rc;
  // (the gathered attention rows are parked behind the first B rows of the h2 slot: the pooled tail needs 2 B rows of tape there)
  run.tail = !tokens_out && train_pooled_tail() && run.M >= 2 * B;      // the same rule in text_backward_impl
  if ((rc = tape_forward(run))) return rc;
  if (tokens_out && pack_tokens) {
    if ((rc = head_forward(D, t, head, nullptr, t.dxe, t.tokP, run.M, st))) return rc;
    return launch_unpack_token_rows(t.tokP, t.seq_off, tokens_out, B, L, w->embed_dim, t.rows, eot_rows_out, st);
  }
  if (tokens_out) {
    if (eot_rows_out && hipMemcpyAsync(eot_rows_out, t.rows, static_cast<size_t>(B) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "text_forward_train_tokens: eot row copy failed");
    if (hipMemsetAsync(t.seq_off, 0, static_cast<size_t>(B + 1) * 4, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "text_forward_train_tokens: memset failed");
    return head_forward(D, t, head, nullptr, t.dxe, tokens_out, M, st);
  }
  return head_forward(D, t, head, run.tail ? nullptr : t.rows, t.pool, feat, B, st);
}

extern "C" int cmh_text_forward_train(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                      const uint8_t* key_padding_mask, float* feat, void* tape, size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(feat, "text_forward_train: null feature pointer");
  return text_forward_train_impl(w, tokens, batch, seq_len, key_padding_mask, feat, nullptr, nullptr, tape, tape_bytes, stream);
}

extern "C" int cmh_text_forward_train_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                             const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out, void* tape,
                                             size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "text_forward_train_tokens: null output pointer");
  return text_forward_train_impl(w, tokens, batch, seq_len, key_padding_mask, nullptr, tokens_out, eot_rows_out, tape, tape_bytes, stream);
}

extern "C" int cmh_text_forward_train_tokens_packed(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                                    const uint8_t* key_padding_mask, float* tokens_out, int32_t* eot_rows_out, void* tape,
                                                    size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(tokens_out, "text_forward_train_tokens_packed: null output pointer");
  return text_forward_train_impl(w, tokens, batch, seq_len, key_padding_mask, nullptr, tokens_out, eot_rows_out, tape, tape_bytes, stream,
                                 /*pack_tokens_req=*/true);
}

static int text_backward_impl(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                              const uint8_t* key_padding_mask, const float* dfeat, const float* dtokens, const cmh_text_grads* gr,
                              void* tape, size_t tape_bytes, void* stream, int layer_hi = -1, int layer_lo = 0) {   // parts: see vit_backward_impl
  CMH_CHECK_ARG(w && tokens && (dfeat || dtokens) && gr && tape && batch > 0 && seq_len > 0, "text_backward: bad arguments");
  const TrainDims D(w, batch, seq_len);
  const bool head_grads = gr->token_embedding && gr->positional_embedding && gr->ln_final_w && gr->ln_final_b && gr->text_projection;
  TrainBufs t;
  int rc = open_backward("text_backward", D, w->blocks, head_grads, gr->blocks, tape, tape_bytes, &layer_hi, layer_lo, &t);
  if (rc) return rc;
  const int B = D.B, L = D.T, M = D.M, d = D.d, E = D.E;
  hipStream_t st = as_stream(stream);
  BlockRun run{D, w->blocks, t, st, M, /*causal=*/1, key_padding_mask};
  // Is the tape packed?  Pooled head: by the forward call's own rule.  All-token head: a tape that
  // cmh_text_forward_train_tokens_packed filled holds a packed plan, a dense one the count 0.
  if (dtokens || text_packing(key_padding_mask)) {
    int total = 0;
    if ((rc = tape_packed_rows(dtokens ? "text_backward_tokens" : "text_backward", tape, t, D, /*dense_ok=*/dtokens != nullptr, st, &total)))
      return rc;
    if (total > 0) { run.seq_off = t.seq_off; run.M = total; }
  }
  run.tail = !dtokens && train_pooled_tail() && run.M >= 2 * B;
  if (layer_hi == w->layers) {
    if ((rc = zero_pad_buffers(t, static_cast<size_t>(run.M), st))) return rc;
    const float* dtok = dtokens;
    if (dtokens && run.seq_off) {   // the kept rows of the dense [B, L, E] gradient (the padded rows' gradient is zero by the caller's promise)
      if ((rc = launch_pack_token_rows(dtokens, run.seq_off, t.tokP, B, L, E, st))) return rc;
      dtok = t.tokP;
    }
    if ((rc = head_backward(D, t, Head{w->ln_final_w, w->ln_final_b, w->text_projection_t, gr->text_projection, gr->ln_final_w, gr->ln_final_b},
                            dfeat, dtok, run.M, run.tail, st))) return rc;
  }
  if ((rc = blocks_backward(run, gr->blocks, layer_hi, layer_lo, dtokens != nullptr))) return rc;
  if (layer_lo > 0) return CMH_OK;
  // x_0[b, t] = token_embedding[tokens[b, t]] + positional_embedding[t]
  if (hipMemsetAsync(gr->positional_embedding, 0, static_cast<size_t>(w->context_length) * d * 4, st) != hipSuccess ||
      hipMemsetAsync(gr->token_embedding, 0, static_cast<size_t>(w->vocab_size) * d * 4, st) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "text_backward: memset failed");
  if (run.seq_off) {
    hipLaunchKernelGGL(packed_dpos_kernel, dim3(L, (d + 255) / 256), dim3(256), 0, st, t.dx, run.seq_off, B, d, gr->positional_embedding);
    hipLaunchKernelGGL(packed_embed_scatter_kernel, dim3(M), dim3(256), 0, st, tokens, t.dx, run.seq_off, gr->token_embedding, B, L, d,
                       w->vocab_size);
  } else {
    if ((rc = cmh_colsum(t.dx, kF32, B, L * d, gr->positional_embedding, t.red, t.red_bytes, st))) return rc;
    hipLaunchKernelGGL(embed_scatter_kernel, dim3(M), dim3(256), 0, st, tokens, t.dx, gr->token_embedding, M, d, w->vocab_size);
  }
  CMH_CHECK_LAUNCH("embedding scatter");
  return CMH_OK;
}

extern "C" int cmh_text_backward(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                 const uint8_t* key_padding_mask, const float* dfeat, const cmh_text_grads* gr, void* tape,
                                 size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(dfeat, "text_backward: null gradient");
  return text_backward_impl(w, tokens, batch, seq_len, key_padding_mask, dfeat, nullptr, gr, tape, tape_bytes, stream);
}

extern "C" int cmh_text_backward_part(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                      const uint8_t* key_padding_mask, const float* dfeat, const cmh_text_grads* gr, void* tape,
                                      size_t tape_bytes, int32_t layer_hi, int32_t layer_lo, void* stream) {
  CMH_CHECK_ARG(dfeat && layer_hi >= 0, "text_backward_part: bad arguments");
  return text_backward_impl(w, tokens, batch, seq_len, key_padding_mask, dfeat, nullptr, gr, tape, tape_bytes, stream, layer_hi, layer_lo);
}

extern "C" int cmh_text_backward_tokens(const cmh_text_weights* w, const int64_t* tokens, int32_t batch, int32_t seq_len,
                                        const uint8_t* key_padding_mask, const float* dtokens, const cmh_text_grads* gr, void* tape,
                                        size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(dtokens, "text_backward_tokens: null gradient");
  return text_backward_impl(w, tokens, batch, seq_len, key_padding_mask, nullptr, dtokens, gr, tape, tape_bytes, stream);
}

// ================================================================================================ a bare stack of blocks
// MITH's concept transformer (model/MITH.py:379-396: 2 ResidualAttentionBlocks over the K "concept tokens" of every sample, no
// mask) under training: f32 residual stream in and out, GEMM operands in `dtype`.
extern "C" size_t cmh_blocks_train_bytes(int32_t dtype, int32_t B, int32_t T, int32_t d, int32_t layers) {
  return B <= 0 || T <= 0 || d <= 0 || layers <= 0 ? 0 : carve_train(nullptr, TrainDims(dtype, B, T, d, layers)).total;
}

extern "C" int cmh_blocks_forward_train(const cmh_block_weights* blocks, int32_t layers, int32_t dtype, const float* x, float* y,
                                        int32_t B, int32_t T, int32_t d, void* tape, size_t tape_bytes, void* stream) {
  CMH_CHECK_ARG(blocks && x && y && tape && layers > 0 && B > 0 && T > 0, "blocks_forward_train: bad arguments");
  const TrainDims D(dtype, B, T, d, layers);
  int rc = check_train_tower(D, blocks);
  if (rc) return rc;
  TrainBufs t;
  if ((rc = open_tape("blocks_forward_train", D, tape, tape_bytes, /*need_aligned=*/true, &t))) return rc;
  const size_t bytes = static_cast<size_t>(D.M) * d * 4;
  hipStream_t st = as_stream(stream);
  if (hipMemcpyAsync(t.L[0].x_in, x, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "blocks_forward_train: copy failed");
  if ((rc = tape_forward(BlockRun{D, blocks, t, st, D.M}))) return rc;
  if (hipMemcpyAsync(y, t.x_last, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "blocks_forward_train: copy failed");
  return CMH_OK;
}

extern "C" int cmh_blocks_backward(const cmh_block_weights* blocks, const cmh_block_grads* grads, int32_t layers, int32_t dtype,
                                   const float* dy, float* dx, int32_t B, int32_t T, int32_t d, void* tape, size_t tape_bytes,
                                   void* stream) {
  CMH_CHECK_ARG(blocks && grads && dy && dx && tape && layers > 0 && B > 0 && T > 0, "blocks_backward: bad arguments");
  const TrainDims D(dtype, B, T, d, layers);
  TrainBufs t;
  int hi = layers, rc = open_backward("blocks_backward", D, blocks, /*head_grads=*/true, grads, tape, tape_bytes, &hi, 0, &t);
  if (rc) return rc;
  const size_t bytes = static_cast<size_t>(D.M) * d * 4;
  hipStream_t st = as_stream(stream);
  if ((rc = zero_pad_buffers(t, static_cast<size_t>(D.M), st))) return rc;
  if (hipMemcpyAsync(t.dx, dy, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "blocks_backward: copy failed");
  if ((rc = blocks_backward(BlockRun{D, blocks, t, st, D.M}, grads, layers, 0, /*dtokens_head=*/false))) return rc;
  if (hipMemcpyAsync(dx, t.dx, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CMH_ERR_LAUNCH, "blocks_backward: copy failed");
  return CMH_OK;
}
