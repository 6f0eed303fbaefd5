// MSCH all-triplets margin loss: reference train/DPSIH/Loss.py:78-137 `Multi_Semantic_Correlation_Loss.forward(batch_inputs, batch_labels,
// inputs)` in its two-dimensional branch (:98-99), as DPSIH's step calls it three times (:61-62), forward and backward.
//
//   n(x) = x / max(|x|, 1e-12) per row when `normalize` is set (:86-93), x itself otherwise;  s = -n(u) n(v)^T                    (:99)
//   same = (y y^T > 0) without its diagonal, diff = not (y y^T > 0) taken BEFORE the diagonal leaves                          (:105-108)
//   (the reference clears the diagonal of every SQUARE mask, :107, and both calls of a step have B rows on either side: the cross-modal
//   call loses its diagonal as the intra-modal one does)
//   eligible (a, p, n): same[a, p] and diff[a, n];  tm = s_an - s_ap;  active: tm <= m, semi-hard: 0 < tm <= m                (:110-120)
//   loss = sum_active relu((s_ap - s_an) + m) / count, count = the number of active triplets; 0 without any                   (:128-137)
//   d loss / d s_ap = +n_act(a, p) / count, d loss / d s_an = -p_act(a, n) / count: the active partners whose violation is > 0 (relu'(0) = 0)
//
// The reference materialises the [B, B, B] mask, gathers three index vectors of up to B^3 / 4 entries twice and reads a length back.  Here
// workgroup (a, pair) owns anchor a: thread j forms s[a, j] (one k-ascending fmaf chain over the anchor's row in LDS) and the two mask bits
// from the labels; a wave's ballot is 64 bits of the anchor's `same` / `diff` bit row in LDS (no float copy of y y^T exists).  Then thread j
// walks ALL partners of its column in ascending order through the other bit row - at most 262 144 pairs per anchor at B = 1024, under a
// microsecond of VALU work per workgroup - and decides each triplet on the f32 difference the reference decides on; a sorted side with a
// search would save nothing measurable and would have to reproduce the rounding of that difference at the threshold.  A positive column
// gives the anchor's active count, its violation sum (f64) and +n_act; a negative column gives -p_act: integers, exact in any order.  One
// wave per pair then folds the anchors in a fixed order.  Backward: G = coef dloss / count; workgroup (b, side, pair) adds the rows of the
// other side weighted by row b (side 0) or column b (side 1) of G, wave w the rows w, w + 4, ... in order, lane l the code columns l and
// l + 64, the four partials left to right; the intra-modal call adds row and column as integers first and writes du alone.  The
// normaliser's backward (mith.hip's l2norm_bwd_kernel arithmetic on the saved unit rows and divisors) finishes the row in the same
// launch.  No atomics, no kernel waits on another workgroup, every floating sum has a fixed order: two calls give the same bits.
// Launches per call: one normalize_rows per DISTINCT operand when `normalize` is set (two for a step's three pairs), the anchor kernel,
// the fold; backward: one.
#include "head_common.h"

namespace cmh {

constexpr int kMscMaxB = 1024, kMscMaxK = 128, kMscMaxCalls = 4, kMscWords = kMscMaxB / 64;

// a, b: the rows the similarities are formed from (the unit rows, or the operands themselves); na, nb: their divisors (null without
// normalisation); da, db: the gradients' buffers; intra: v == u
struct MscCalls {
  const float* a[kMscMaxCalls]; const float* b[kMscMaxCalls]; const float* na[kMscMaxCalls]; const float* nb[kMscMaxCalls];
  float* da[kMscMaxCalls]; float* db[kMscMaxCalls]; int intra[kMscMaxCalls];
};

// y_i . y_j > 0, c ascending in one FMA chain (symmetric in i and j bit for bit)
__device__ __forceinline__ bool msc_similar(const float* __restrict__ yi, const float* __restrict__ yj, int C) {
  float a = 0.f;
  for (int c = 0; c < C; ++c) a = fmaf(yi[c], yj[c], a);
  return a > 0.f;
}

// one triplet as the reference decides it (:113-120, :134-135): *strict = the violation is > 0 (it then is the relu's value)
__device__ __forceinline__ bool msc_active(float ap, float an, float margin, int semi, float* viol, bool* strict) {
  const float tm = __fsub_rn(an, ap);
  const bool act = tm <= margin && (!semi || tm > 0.f);
  *viol = __fadd_rn(__fsub_rn(ap, an), margin);
  *strict = act && *viol > 0.f;
  return act;
}

// grid (B, calls).  sim, coef [calls, B, B]; part [calls, B] f64 violation sums; cnt [calls, B] active triplets
__global__ __launch_bounds__(256) void msc_anchor_kernel(MscCalls p, const float* __restrict__ y, int B, int K, int C, float margin, int semi,
                                                         float* __restrict__ sim, int32_t* __restrict__ coef, double* __restrict__ part,
                                                         int32_t* __restrict__ cnt) {
  __shared__ float sa[kMscMaxK];                             // the anchor's row
  __shared__ float ss[kMscMaxB];                             // s[a, :]
  __shared__ unsigned long long same[kMscWords], diff[kMscWords];
  __shared__ double red[4];
  const int a = blockIdx.x, call = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* u = p.a[call];
  const float* v = p.b[call];
  const float* ya = y + static_cast<size_t>(a) * C;
  const size_t row = (static_cast<size_t>(call) * B + a) * B;
  for (int k = tid; k < K; k += 256) sa[k] = u[static_cast<size_t>(a) * K + k];
  __syncthreads();
  const int rounds = (B + 255) / 256;                        // uniform: every wave ballots in every round
  for (int q = 0; q < rounds; ++q) {
    const int j = q * 256 + tid;
    bool sm = false, df = false;
    if (j < B) {
      const float* vj = v + static_cast<size_t>(j) * K;
      float d = 0.f;
      for (int k = 0; k < K; ++k) d = fmaf(sa[k], vj[k], d);
      ss[j] = -d;
      sim[row + j] = -d;
      const bool s = msc_similar(ya, y + static_cast<size_t>(j) * C, C);
      sm = s && j != a;
      df = !s;
    }
    const unsigned long long ms = __ballot(sm), md = __ballot(df);
    if (lane == 0) { same[q * 4 + w] = ms; diff[q * 4 + w] = md; }
  }
  __syncthreads();
  const int words = rounds * 4;
  double sum = 0.0;
  int active = 0;
  for (int q = 0; q < rounds; ++q) {
    const int j = q * 256 + tid;
    if (j >= B) continue;
    const bool pos = (same[j >> 6] >> (j & 63)) & 1ull, neg = (diff[j >> 6] >> (j & 63)) & 1ull;
    const float sj = ss[j];
    int c = 0;
    float viol;
    bool strict;
    if (pos) {                                               // partners: the negatives, ascending
      for (int wd = 0; wd < words; ++wd)
        for (unsigned long long m = diff[wd]; m; m &= m - 1) {
          const int n = wd * 64 + __builtin_ctzll(m);
          active += msc_active(sj, ss[n], margin, semi, &viol, &strict) ? 1 : 0;
          if (strict) { ++c; sum += static_cast<double>(viol); }
        }
    } else if (neg) {                                        // partners: the positives; a row without labels is its own negative
      for (int wd = 0; wd < words; ++wd)
        for (unsigned long long m = same[wd]; m; m &= m - 1) {
          msc_active(ss[wd * 64 + __builtin_ctzll(m)], sj, margin, semi, &viol, &strict);
          if (strict) --c;
        }
    }
    coef[row + j] = c;
  }
  sum = block_sum_ltr(sum, red);
  const double act = block_sum_ltr(static_cast<double>(active), red);     // <= 262 144: exact
  if (tid == 0) {
    part[static_cast<size_t>(call) * B + a] = sum;
    cnt[static_cast<size_t>(call) * B + a] = static_cast<int32_t>(act);
  }
}

// one wave per pair: lane l adds anchors l, l + 64, ... in order, the butterfly adds the lanes
__global__ __launch_bounds__(64) void msc_fold_kernel(const double* __restrict__ part, const int32_t* __restrict__ cnt, int B,
                                                      float* __restrict__ loss, int64_t* __restrict__ count) {
  const int call = blockIdx.x;
  double s = 0.0, n = 0.0;                                   // n <= 2^28: exact
  for (int i = threadIdx.x; i < B; i += 64) {
    s += part[static_cast<size_t>(call) * B + i];
    n += static_cast<double>(cnt[static_cast<size_t>(call) * B + i]);
  }
  s = wave_sum(s); n = wave_sum(n);
  if (threadIdx.x == 0) {
    loss[call] = n > 0.0 ? static_cast<float>(s / n) : 0.f;
    count[call] = static_cast<int64_t>(n);
  }
}

// grid (B, 2, calls).  side 0: d a[b] = -sum_j G[b, j] b_j; side 1: d b[b] = -sum_i G[i, b] a_i; intra: side 0 takes both, side 1 nothing
__global__ __launch_bounds__(256) void msc_backward_kernel(MscCalls p, int B, int K, const int32_t* __restrict__ coef,
                                                           const int64_t* __restrict__ count, const float* __restrict__ dloss) {
  __shared__ float sg[kMscMaxB];
  __shared__ float wave_part[4][kMscMaxK];
  __shared__ float red[4];
  const int b = blockIdx.x, side = blockIdx.y, call = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int intra = p.intra[call];
  if (intra && side) return;                                 // uniform over the workgroup
  const float* own = side ? p.b[call] : p.a[call];
  const float* other = side ? p.a[call] : p.b[call];
  const float* n_own = side ? p.nb[call] : p.na[call];
  float* out = (side ? p.db[call] : p.da[call]) + static_cast<size_t>(b) * K;
  const int64_t n = count[call];
  if (n == 0) {
    for (int k = tid; k < K; k += 256) out[k] = 0.f;
    return;
  }
  const float scale = -static_cast<float>(static_cast<double>(dloss[call]) / static_cast<double>(n));     // s = -a b^T
  const int32_t* cf = coef + static_cast<size_t>(call) * B * B;
  for (int j = tid; j < B; j += 256) {
    const int32_t r = cf[static_cast<size_t>(b) * B + j], c = cf[static_cast<size_t>(j) * B + b];
    sg[j] = static_cast<float>(intra ? r + c : (side ? c : r)) * scale;
  }
  __syncthreads();
  const int k_lo = lane, k_hi = lane + 64;
  float acc0 = 0.f, acc1 = 0.f;
  for (int j = w; j < B; j += 4) {
    const float* oj = other + static_cast<size_t>(j) * K;
    const float g = sg[j];
    acc0 = fmaf(g, k_lo < K ? oj[k_lo] : 0.f, acc0);
    acc1 = fmaf(g, k_hi < K ? oj[k_hi] : 0.f, acc1);
  }
  wave_part[w][k_lo] = acc0;
  wave_part[w][k_hi] = acc1;
  __syncthreads();
  float g = 0.f, u = 0.f;
  if (tid < K) g = ((wave_part[0][tid] + wave_part[1][tid]) + wave_part[2][tid]) + wave_part[3][tid];
  if (!n_own) {                                              // no normalisation: the operand's gradient as it is
    if (tid < K) out[tid] = g;
    return;
  }
  // the normaliser's backward (l2norm_bwd_kernel's arithmetic): dx = (g - u (u . g)) / n; below the eps clamp u = x / eps is linear
  if (tid < K) u = own[static_cast<size_t>(b) * K + tid];
  const float dot = block_sum_ltr(u * g, red), nrm = n_own[b];
  const float proj = nrm > 1e-12f ? dot : 0.f;
  if (tid < K) out[tid] = (g - u * proj) / nrm;
}

}  // namespace cmh

using namespace cmh;

struct MscWs { double* part; int32_t* cnt; size_t total; };  // [kMscMaxCalls, B] each
static MscWs carve_msc(void* ws, size_t B) {
  Carver c(ws);
  return {c.take<double>(kMscMaxCalls * B * sizeof(double)), c.take<int32_t>(kMscMaxCalls * B * sizeof(int32_t)), c.total()};
}

extern "C" size_t cmh_msc_triplet_workspace_bytes(int32_t B) { return B > 0 && B <= kMscMaxB ? carve_msc(nullptr, B).total : 0; }

static int msc_shape(const char* what, int n, int B, int K, int C) {
  CMH_CHECK_ARG(n >= 1 && n <= kMscMaxCalls, "%s: calls=%d (1 .. %d)", what, n, kMscMaxCalls);
  CMH_CHECK_ARG(B >= 1 && B <= kMscMaxB && K >= 1 && K <= kMscMaxK && C > 0, "%s: B=%d (1 .. %d) K=%d (1 .. %d) C=%d (>= 1)", what, B, kMscMaxB,
                K, kMscMaxK, C);
  return CMH_OK;
}

// The operands of the n calls.  With `unit` ([2 calls, B, K]) and `divisor` ([2 calls, B]) the similarities come from the unit rows: every
// DISTINCT operand pointer has one slot, the index of its first appearance in u[0], v[0], u[1], ... - the forward fills the slots, the
// backward finds them again from the same pointers.  slot_of (optional) receives each slot's operand, null for a slot that is not used.
static int msc_calls(const char* what, int n, const float* const* u, const float* const* v, float* const* du, float* const* dv, int B, int K,
                     const float* unit, const float* divisor, MscCalls* out, const float** slot_of) {
  const float* seen[2 * kMscMaxCalls] = {};
  for (int q = 0; q < kMscMaxCalls; ++q) {
    const int s = q < n ? q : 0;                              // unused entries repeat the first call's
    CMH_CHECK_ARG(u[s] && v[s], "%s: null pointer in call %d", what, s);
    const bool intra = u[s] == v[s];
    CMH_CHECK_ARG(!du || (du[s] && (intra || dv[s])), "%s: null gradient pointer in call %d", what, s);
    const float* op[2] = {u[s], v[s]};
    const float* rows[2];
    const float* div[2];
    for (int t = 0; t < 2; ++t) {
      if (!unit) { rows[t] = op[t]; div[t] = nullptr; continue; }
      int slot = 0;
      while (seen[slot] && seen[slot] != op[t]) ++slot;       // at most 2 n distinct operands: a free slot exists
      seen[slot] = op[t];
      rows[t] = unit + static_cast<size_t>(slot) * B * K;
      div[t] = divisor + static_cast<size_t>(slot) * B;
    }
    out->a[q] = rows[0]; out->b[q] = rows[1]; out->na[q] = div[0]; out->nb[q] = div[1];
    out->da[q] = du ? du[s] : nullptr; out->db[q] = du && !intra ? dv[s] : nullptr; out->intra[q] = intra;
  }
  if (slot_of)
    for (int t = 0; t < 2 * kMscMaxCalls; ++t) slot_of[t] = seen[t];
  return CMH_OK;
}

extern "C" int cmh_msc_triplet_loss(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B, int32_t K,
                                    int32_t C, float margin, int32_t mining, int32_t normalize, float* loss, int64_t* count, float* sim,
                                    int32_t* coef, float* unit, float* divisor, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(u && v && labels && loss && count && sim && coef, "msc_triplet_loss: null pointer");
  CMH_CHECK_ARG(!normalize || (unit && divisor), "msc_triplet_loss: null pointer (normalize needs unit and divisor)");
  CMH_CHECK_ARG(mining == 0 || mining == 1, "msc_triplet_loss: mining=%d (0: all, 1: semi-hard)", mining);
  int rc = msc_shape("msc_triplet_loss", calls, B, K, C);
  if (rc) return rc;
  MscCalls p;
  const float* slot_of[2 * kMscMaxCalls];
  if ((rc = msc_calls("msc_triplet_loss", calls, u, v, nullptr, nullptr, B, K, normalize ? unit : nullptr, divisor, &p, slot_of))) return rc;
  if ((rc = open_ws("msc_triplet_loss", workspace, workspace_bytes, carve_msc(nullptr, B).total, CMH_ERR_INVALID))) return rc;
  const MscWs w = carve_msc(workspace, B);
  hipStream_t st = as_stream(stream);
  if (normalize)
    for (int t = 0; t < 2 * kMscMaxCalls && slot_of[t]; ++t)
      launch_normalize_rows(slot_of[t], unit + static_cast<size_t>(t) * B * K, divisor + static_cast<size_t>(t) * B, B, K, 1e-12f, nullptr, st);
  hipLaunchKernelGGL(msc_anchor_kernel, dim3(B, calls), dim3(256), 0, st, p, labels, B, K, C, margin, mining, sim, coef, w.part, w.cnt);
  hipLaunchKernelGGL(msc_fold_kernel, dim3(calls), dim3(64), 0, st, w.part, w.cnt, B, loss, count);
  CMH_CHECK_LAUNCH("msc_triplet_loss");
  return CMH_OK;
}

extern "C" int cmh_msc_triplet_loss_backward(const float* const* u, const float* const* v, int32_t calls, int32_t B, int32_t K,
                                             int32_t normalize, const int32_t* coef, const int64_t* count, const float* unit,
                                             const float* divisor, const float* dloss, float* const* du, float* const* dv, void* stream) {
  CMH_CHECK_ARG(u && v && coef && count && dloss && du && dv, "msc_triplet_loss_backward: null pointer");
  CMH_CHECK_ARG(!normalize || (unit && divisor), "msc_triplet_loss_backward: null pointer (normalize needs unit and divisor)");
  int rc = msc_shape("msc_triplet_loss_backward", calls, B, K, 1);
  if (rc) return rc;
  MscCalls p;
  if ((rc = msc_calls("msc_triplet_loss_backward", calls, u, v, du, dv, B, K, normalize ? unit : nullptr, divisor, &p, nullptr))) return rc;
  hipLaunchKernelGGL(msc_backward_kernel, dim3(B, 2, calls), dim3(256), 0, as_stream(stream), p, B, K, coef, count, dloss);
  CMH_CHECK_LAUNCH("msc_triplet_loss_backward");
  return CMH_OK;
}
