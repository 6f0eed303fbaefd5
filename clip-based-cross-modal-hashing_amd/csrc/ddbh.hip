// DDBH (TCSVT 2025) base-point loss and quantisation term: reference train/DDBH/loss.py:5-101 `BPLoss.forward(u, v, y)` and
// train/DDBH/hash_train.py:64-78, forward and backward.
//
//   s = (y y^T > 0), inner = u v^T; row i is active when it has a similar and a dissimilar column                  (loss.py:16-23)
//   meanS = clamp(mean(S)), dMax = mean of the n_d - int(n_d * percent) largest of D, BP = meanS - (ub - meanS)/ub |meanS - dMax|   (:33-37)
//   meanDS = clamp(mean(D)), sMin = mean of the n_s - int(n_s * percent) smallest of S, BP_ds = meanDS - meanDS/ub |meanDS - sMin|   (:41-43)
//   c, d, a, g from the base point (:89-101); f = c x + d on the easy side of the base point, a c x + g on the hard side   (:47-61)
//   element = [similar] f + log(1 + e^-f); row means of the kept similar / dissimilar elements, summed, / active rows      (:66-78, :80-86)
//
// The reference walks the rows in Python with two sorts and four host reads each.  Here workgroup i owns row i: its B inner products
// and flags live in LDS, counts and sums are fixed-order block reductions, and the two tail means come from ONE radix select without a
// sort: with theta the t-th largest entry of D, the mean of the t largest is (sum_{x > theta} x + (t - #{x > theta}) theta) / t, since
// tied entries are equal - so no index tie-break exists.  theta is found over the order-preserving 32-bit image of the floats, a byte
// per pass; the histogram of a pass counts D (descending: complemented key) in the low and S (ascending) in the high half of each
// 32-bit bin (B <= 8192 < 2^16), so one block scan serves both.  Base points and coefficients are formed in double and rounded to f32
// once, where torch rounds them (a Python / numpy double against an f32 tensor); log(1 + e^-f) is max(-f, 0) + log1p(e^-|f|).
// grid.y = the calls of one step (the trainer's three (u, v) pairs share one launch).  The backward recomputes inner (the same FMA chain,
// so every easy / hard decision repeats) and G from the per-row values the forward saved; rows give du, a transposed walk gives dv,
// each output element is written by one thread in a fixed order: no atomics.
#include "head_common.h"

#include <cmath>

namespace cmh {

constexpr int kDdbhMaxB = 8192, kDdbhMaxK = 1024, kDdbhMaxCalls = 4, kDdbhRow = 8;

struct DdbhCalls { const float* u[kDdbhMaxCalls]; const float* v[kDdbhMaxCalls]; float* du[kDdbhMaxCalls]; float* dv[kDdbhMaxCalls]; };
// c = ln(y_p / (99 (1 - y_p))) / right, ac = a c with a = -ln(99 y_p / (1 - y_p)) / (left c), l2 = ln((1 - y_p) / y_p)
struct DdbhCoef { double c, ac, l2, lower, upper, percent; };
// what the forward keeps per row ([n, B, 8] 32-bit words): the f32 roundings of BP, BP_ds, d, g (similar), d, g (dissimilar); the kept
// counts m_s, m_d as integers (-1: the row is not active)
struct DdbhRow { float bp, bpds, ds, gs, dd, gd; int ms, md; };
static_assert(sizeof(DdbhRow) == kDdbhRow * 4, "DdbhRow is eight words");

// order-preserving image of a float: a < b  <=>  key(a) < key(b)  (-0 sorts below +0; both are the value 0)
__device__ __forceinline__ uint32_t ord_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ord_val(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// own (LDS) . other (a global row), k ascending in one FMA chain: the forward and both backward walks get the same bits
__device__ __forceinline__ float ddbh_dot(const float* own, const float* __restrict__ other, int K, bool vec) {
  float a = 0.f;
  if (vec) {
    for (int k = 0; k < K; k += 4) {
      const float4 o = *reinterpret_cast<const float4*>(other + k);
      const float4 w = *reinterpret_cast<const float4*>(own + k);
      a = fmaf(w.x, o.x, a); a = fmaf(w.y, o.y, a); a = fmaf(w.z, o.z, a); a = fmaf(w.w, o.w, a);
    }
  } else {
    for (int k = 0; k < K; ++k) a = fmaf(own[k], other[k], a);
  }
  return a;
}
// y_i . y_j > 0, c ascending in one FMA chain (symmetric in i and j bit for bit)
__device__ __forceinline__ bool ddbh_similar(const float* __restrict__ yi, const float* __restrict__ yj, int C) {
  float a = 0.f;
  for (int c = 0; c < C; ++c) a = fmaf(yi[c], yj[c], a);
  return a > 0.f;
}
__device__ __forceinline__ float softplus_neg(float f) { return fmaxf(-f, 0.f) + log1pf(expf(-fabsf(f))); }   // log(1 + e^-f)
__device__ __forceinline__ float sigmoidf(float f) {
  const float e = expf(-fabsf(f));
  return f >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// c x + d as torch forms it: the product rounded, then the sum (no contraction)
__device__ __forceinline__ float ddbh_line(float slope, float x, float off) { return __fadd_rn(__fmul_rn(slope, x), off); }

// inclusive scan of one value per thread over the 256 threads (wt: four words of LDS)
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* wt) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  __syncthreads();
  if (lane == 63) wt[w] = v;
  __syncthreads();
  for (int q = 0; q < w; ++q) v += wt[q];
  return v;
}

__global__ __launch_bounds__(256) void ddbh_rows_kernel(DdbhCalls p, const float* __restrict__ y, int B, int K, int C, int vec, DdbhCoef cf,
                                                        double* __restrict__ part, DdbhRow* __restrict__ rows) {
  extern __shared__ float4 ddbh_lds[];
  const int Kp = (K + 3) & ~3;
  float* su = reinterpret_cast<float*>(ddbh_lds);            // [Kp] u_i
  float* sx = su + Kp;                                       // [B] inner[i, :]
  uint8_t* sf = reinterpret_cast<uint8_t*>(sx + B);          // [B] 1 = similar
  __shared__ uint32_t hist[256], wt[4], sel[4];
  __shared__ double red[4];
  const int i = blockIdx.x, call = blockIdx.y, tid = threadIdx.x;
  const float* u = p.u[call];
  const float* v = p.v[call];
  for (int k = tid; k < K; k += 256) su[k] = u[static_cast<size_t>(i) * K + k];
  __syncthreads();
  double cnt_s = 0.0, sum_s = 0.0, sum_d = 0.0;
  for (int j = tid; j < B; j += 256) {
    const float x = ddbh_dot(su, v + static_cast<size_t>(j) * K, K, vec);
    const bool s = ddbh_similar(y + static_cast<size_t>(i) * C, y + static_cast<size_t>(j) * C, C);
    sx[j] = x;
    sf[j] = s ? 1 : 0;
    if (s) { cnt_s += 1.0; sum_s += x; } else { sum_d += x; }
  }
  const int ns = static_cast<int>(block_sum_ltr(cnt_s, red)), nd = B - ns;
  sum_s = block_sum_ltr(sum_s, red);
  sum_d = block_sum_ltr(sum_d, red);
  double* out = part + (static_cast<size_t>(call) * B + i) * 2;
  DdbhRow* row = rows + static_cast<size_t>(call) * B + i;
  if (ns == 0 || nd == 0) {                                  // not active (loss.py:23); uniform over the workgroup
    if (tid == 0) { out[0] = 0.0; out[1] = 0.0; *row = DdbhRow{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, -1}; }
    return;
  }
  // tail lengths (:35, :42): a double product, truncated, as Python's int(len * percent)
  const int ts = ns - static_cast<int>(static_cast<double>(ns) * cf.percent), td = nd - static_cast<int>(static_cast<double>(nd) * cf.percent);
  int rem_s = ts > 0 ? ts : 1, rem_d = td > 0 ? td : 1;      // (an empty tail is NaN below; the select still runs on a valid rank)
  uint32_t pre_s = 0, pre_d = 0;                             // the leading bytes of the two thresholds' keys
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < B; j += 256) {
      const uint32_t key = ord_key(sx[j]);
      if (sf[j]) {                                           // S ascending: the rem_s-th smallest key
        if (pass == 0 || (key >> (shift + 8)) == pre_s) atomicAdd(&hist[(key >> shift) & 255u], 1u << 16);
      } else {                                               // D descending: the rem_d-th smallest complemented key
        const uint32_t kd = ~key;
        if (pass == 0 || (kd >> (shift + 8)) == pre_d) atomicAdd(&hist[(kd >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    const uint32_t h = hist[tid], incl = block_scan_incl(h, wt);
    const int incl_d = incl & 0xffffu, excl_d = incl_d - static_cast<int>(h & 0xffffu);
    const int incl_s = incl >> 16, excl_s = incl_s - static_cast<int>(h >> 16);
    if (excl_d < rem_d && rem_d <= incl_d) { sel[0] = tid; sel[1] = rem_d - excl_d; }
    if (excl_s < rem_s && rem_s <= incl_s) { sel[2] = tid; sel[3] = rem_s - excl_s; }
    __syncthreads();
    pre_d = (pre_d << 8) | sel[0]; rem_d = static_cast<int>(sel[1]);
    pre_s = (pre_s << 8) | sel[2]; rem_s = static_cast<int>(sel[3]);
  }
  // rem_*: how many entries EQUAL to the threshold the tail takes; the others of the tail lie strictly beyond it
  const float th_d = ord_val(~pre_d), th_s = ord_val(pre_s);
  double beyond_d = 0.0, beyond_s = 0.0;
  for (int j = tid; j < B; j += 256) {
    const float x = sx[j];
    const uint32_t key = ord_key(x);
    if (sf[j]) { if (key < pre_s) beyond_s += x; } else { if (~key < pre_d) beyond_d += x; }
  }
  beyond_d = block_sum_ltr(beyond_d, red);
  beyond_s = block_sum_ltr(beyond_s, red);
  const float nanf_ = __uint_as_float(0x7fc00000u);
  const float d_max = td > 0 ? static_cast<float>((beyond_d + static_cast<double>(rem_d) * th_d) / td) : nanf_;
  const float s_min = ts > 0 ? static_cast<float>((beyond_s + static_cast<double>(rem_s) * th_s) / ts) : nanf_;
  // the four means are f32 values read as doubles; everything on them is double (:33-43, :89-101)
  const float lo = static_cast<float>(cf.lower), hi = static_cast<float>(cf.upper);
  const double mean_s = fminf(fmaxf(static_cast<float>(sum_s / ns), lo), hi), mean_d = fminf(fmaxf(static_cast<float>(sum_d / nd), lo), hi);
  // every product and difference rounded on its own, as numpy's doubles upstream: a contracted a - b c can leave 1e-17 where the
  // two-step result is exactly 0 (ub = 5), and an entry equal to its base point would be kept as a hard one
  const double bp = __dsub_rn(mean_s, __dmul_rn((cf.upper - mean_s) / cf.upper, fabs(mean_s - static_cast<double>(d_max))));
  const double bpds = __dsub_rn(mean_d, __dmul_rn(mean_d / cf.upper, fabs(mean_d - static_cast<double>(s_min))));
  const float c32 = static_cast<float>(cf.c), ac32 = static_cast<float>(cf.ac);
  const float bp32 = static_cast<float>(bp), bpds32 = static_cast<float>(bpds);
  const float ds = static_cast<float>(__dsub_rn(cf.l2, __dmul_rn(cf.c, bp))), gs = static_cast<float>(__dsub_rn(cf.l2, __dmul_rn(cf.ac, bp)));
  const float dd = static_cast<float>(__dsub_rn(cf.l2, __dmul_rn(cf.c, bpds))), gd = static_cast<float>(__dsub_rn(cf.l2, __dmul_rn(cf.ac, bpds)));
  double pos = 0.0, neg = 0.0, ms = 0.0, md = 0.0;
  for (int j = tid; j < B; j += 256) {
    const float x = sx[j];
    if (sf[j]) {
      if (x > bp32) { const float f = ddbh_line(c32, x, ds); pos += f + softplus_neg(f); ms += 1.0; }
      else if (x < bp32) { const float f = ddbh_line(ac32, x, gs); pos += f + softplus_neg(f); ms += 1.0; }
    } else {
      if (x < bpds32) { md += 1.0; neg += softplus_neg(ddbh_line(c32, x, dd)); }
      else if (x > bpds32) { md += 1.0; neg += softplus_neg(ddbh_line(ac32, x, gd)); }
    }
  }
  pos = block_sum_ltr(pos, red);
  neg = block_sum_ltr(neg, red);
  ms = block_sum_ltr(ms, red);
  md = block_sum_ltr(md, red);
  if (tid == 0) {
    out[0] = pos / ms;                                       // an empty kept set: 0 / 0 = NaN, the mean of nothing upstream
    out[1] = neg / md;
    *row = DdbhRow{bp32, bpds32, ds, gs, dd, gd, static_cast<int>(ms), static_cast<int>(md)};
  }
}

// loss[call] = sum_i pos_i / count + sum_i neg_i / count over the active rows (0 without any); one wave per call, lane l adds rows
// l, l + 64, ... in order and the butterfly adds the lanes: the same bits every run
__global__ __launch_bounds__(64) void ddbh_finalize_kernel(const double* __restrict__ part, const DdbhRow* __restrict__ rows, int B,
                                                           float* __restrict__ loss, int32_t* __restrict__ count) {
  const int call = blockIdx.x;
  double pos = 0.0, neg = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) {
    const size_t r = static_cast<size_t>(call) * B + i;
    if (rows[r].ms >= 0) { pos += part[2 * r]; neg += part[2 * r + 1]; n += 1.0; }
  }
  pos = wave_sum(pos); neg = wave_sum(neg); n = wave_sum(n);
  if (threadIdx.x == 0) {
    loss[call] = n > 0.0 ? static_cast<float>(pos / n + neg / n) : 0.f;
    count[call] = static_cast<int32_t>(n);
  }
}

// blockIdx.y = 0: du[b] = sum_j G[b, j] v_j (row b of G); 1: dv[b] = sum_i G[i, b] u_i (column b).  G_ij = slope w / (m count) dloss
__global__ __launch_bounds__(256) void ddbh_backward_kernel(DdbhCalls p, const float* __restrict__ y, int B, int K, int C, int vec, float c32,
                                                            float ac32, const DdbhRow* __restrict__ rows, const int32_t* __restrict__ count,
                                                            const float* __restrict__ dloss) {
  extern __shared__ float4 ddbh_lds[];
  const int Kp = (K + 3) & ~3;
  float* so = reinterpret_cast<float*>(ddbh_lds);            // [Kp] the block's own vector
  float* sacc = so + Kp;                                     // [4, Kp] one partial per wave
  float* sg = sacc + 4 * Kp;                                 // [B] G along the walk
  const int b = blockIdx.x, side = blockIdx.y, call = blockIdx.z, tid = threadIdx.x;
  const float* own = (side ? p.v[call] : p.u[call]) + static_cast<size_t>(b) * K;
  const float* other = side ? p.u[call] : p.v[call];
  float* out = (side ? p.dv[call] : p.du[call]) + static_cast<size_t>(b) * K;
  const DdbhRow* rw = rows + static_cast<size_t>(call) * B;
  const int n = count[call];
  if (n == 0 || (side == 0 && rw[b].ms < 0)) {               // nothing active on this walk (uniform)
    for (int k = tid; k < K; k += 256) out[k] = 0.f;
    return;
  }
  for (int k = tid; k < K; k += 256) so[k] = own[k];
  __syncthreads();
  const float scale = dloss[call] / static_cast<float>(n);
  for (int j = tid; j < B; j += 256) {
    const DdbhRow r = rw[side ? j : b];
    float g = 0.f;
    if (r.ms >= 0) {
      const float x = ddbh_dot(so, other + static_cast<size_t>(j) * K, K, vec);
      if (ddbh_similar(y + static_cast<size_t>(b) * C, y + static_cast<size_t>(j) * C, C)) {
        if (x > r.bp) g = c32 * sigmoidf(ddbh_line(c32, x, r.ds)) / static_cast<float>(r.ms);
        else if (x < r.bp) g = ac32 * sigmoidf(ddbh_line(ac32, x, r.gs)) / static_cast<float>(r.ms);
      } else {
        if (x < r.bpds) g = -c32 * sigmoidf(-ddbh_line(c32, x, r.dd)) / static_cast<float>(r.md);
        else if (x > r.bpds) g = -ac32 * sigmoidf(-ddbh_line(ac32, x, r.gd)) / static_cast<float>(r.md);
      }
    }
    sg[j] = g * scale;
  }
  __syncthreads();
  // wave w adds j = w, w + 4, ... in order, lane l the columns l, l + 64, ...: 256 contiguous bytes of `other` per wave and j
  const int lane = tid & 63, w = tid >> 6;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    float acc = 0.f;
    if (k < K)
      for (int j = w; j < B; j += 4) acc = fmaf(sg[j], other[static_cast<size_t>(j) * K + k], acc);
    if (k < K) sacc[w * Kp + k] = acc;
  }
  __syncthreads();
  for (int k = tid; k < K; k += 256) out[k] = ((sacc[k] + sacc[Kp + k]) + sacc[2 * Kp + k]) + sacc[3 * Kp + k];
}

// q(h) = mean(s @ (h - sign h)^2) = sum_j colsum_j sum_k (h_jk - sign h_jk)^2 / (B K), colsum_j = sum_i s_ij   (hash_train.py:64-76)
__global__ __launch_bounds__(256) void ddbh_quant_rows_kernel(DdbhCalls p, const float* __restrict__ y, int B, int K, int C,
                                                              double* __restrict__ part, float* __restrict__ colsum) {
  __shared__ double red[4];
  const int j = blockIdx.x, call = blockIdx.y, tid = threadIdx.x;
  const float* h = p.u[call] + static_cast<size_t>(j) * K;
  double cs = 0.0, r = 0.0;
  for (int i = tid; i < B; i += 256) cs += ddbh_similar(y + static_cast<size_t>(j) * C, y + static_cast<size_t>(i) * C, C) ? 1.0 : 0.0;
  for (int k = tid; k < K; k += 256) {
    const float x = h[k], d = x - (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
    r += static_cast<double>(d) * d;
  }
  cs = block_sum_ltr(cs, red);
  r = block_sum_ltr(r, red);
  if (tid == 0) {
    part[static_cast<size_t>(call) * B + j] = cs * r;
    if (call == 0) colsum[j] = static_cast<float>(cs);
  }
}

__global__ __launch_bounds__(64) void ddbh_quant_finalize_kernel(const double* __restrict__ part, int B, int K, float* __restrict__ loss) {
  const int call = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) a += part[static_cast<size_t>(call) * B + i];
  a = wave_sum(a);
  if (threadIdx.x == 0) loss[call] = static_cast<float>(a / (static_cast<double>(B) * static_cast<double>(K)));
}

// dh_jk = dloss * 2 (h_jk - sign h_jk) colsum_j / (B K)
__global__ __launch_bounds__(256) void ddbh_quant_backward_kernel(DdbhCalls p, const float* __restrict__ colsum, int B, int K,
                                                                  const float* __restrict__ dloss) {
  const int call = blockIdx.y;
  const size_t n = static_cast<size_t>(B) * K, e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n) return;
  const float x = p.u[call][e], d = x - (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
  p.du[call][e] = dloss[call] * 2.f * d * colsum[e / K] / (static_cast<float>(B) * static_cast<float>(K));
}

}  // namespace cmh

using namespace cmh;

struct DdbhWs { double* part; size_t total; };               // [kDdbhMaxCalls, B, 2] row means (bp) / [kDdbhMaxCalls, B] row terms (quant)
static DdbhWs carve_ddbh(void* ws, size_t B) { Carver c(ws); return {c.take<double>(kDdbhMaxCalls * B * 2 * sizeof(double)), c.total()}; }

extern "C" size_t cmh_ddbh_workspace_bytes(int32_t B) { return B > 0 ? carve_ddbh(nullptr, B).total : 0; }

static int ddbh_shape(const char* what, int n, int B, int K, int C) {
  CMH_CHECK_ARG(n >= 1 && n <= kDdbhMaxCalls, "%s: calls=%d (1 .. %d)", what, n, kDdbhMaxCalls);
  CMH_CHECK_ARG(B > 0 && B <= kDdbhMaxB && K > 0 && K <= kDdbhMaxK && C > 0, "%s: B=%d (<= %d) K=%d (<= %d) C=%d (>= 1)", what, B, kDdbhMaxB,
                K, kDdbhMaxK, C);
  return CMH_OK;
}
// every pointer of the n calls present; *vec = all rows of every matrix can be read as float4
static int ddbh_calls(const char* what, int n, const float* const* a, const float* const* b, float* const* da, float* const* db, int K,
                      DdbhCalls* out, int* vec) {
  *vec = K % 4 == 0;
  for (int q = 0; q < kDdbhMaxCalls; ++q) {
    const int s = q < n ? q : 0;                              // unused slots repeat the first call's pointers
    CMH_CHECK_ARG(a[s] && (!b || b[s]) && (!da || da[s]) && (!db || db[s]), "%s: null pointer in call %d", what, s);
    out->u[q] = a[s]; out->v[q] = b ? b[s] : a[s]; out->du[q] = da ? da[s] : nullptr; out->dv[q] = db ? db[s] : nullptr;
    if ((reinterpret_cast<uintptr_t>(out->u[q]) | reinterpret_cast<uintptr_t>(out->v[q])) & 15) *vec = 0;
  }
  return CMH_OK;
}
static int ddbh_coef(const char* what, double y_p, double right, double left, double lower, double upper, double percent, DdbhCoef* cf) {
  CMH_CHECK_ARG(y_p > 0.0 && y_p < 1.0 && right > 0.0 && left > 0.0 && upper > 0.0 && lower <= upper && percent >= 0.0 && percent <= 1.0,
                "%s: y_p=%g (0 .. 1) right=%g left=%g (> 0) lowerBound=%g upperBound=%g (> 0) percent=%g (0 .. 1)", what, y_p, right, left,
                lower, upper, percent);
  const double c = 1.0 / right * std::log(y_p / (99.0 * (1.0 - y_p)));            // loss.py:92
  const double a = -1.0 / (left * c) * std::log((99.0 * y_p) / (1.0 - y_p));      // :97
  *cf = DdbhCoef{c, a * c, std::log((1.0 - y_p) / y_p), lower, upper, percent};
  return CMH_OK;
}

extern "C" int cmh_ddbh_bp_loss(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B, int32_t K,
                                int32_t C, double y_p, double right, double left, double lower_bound, double upper_bound, double percent,
                                float* loss, void* rows, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(u && v && labels && loss && rows && count, "ddbh_bp_loss: null pointer");
  int rc = ddbh_shape("ddbh_bp_loss", calls, B, K, C), vec = 0;
  if (rc) return rc;
  DdbhCalls p;
  DdbhCoef cf;
  if ((rc = ddbh_calls("ddbh_bp_loss", calls, u, v, nullptr, nullptr, K, &p, &vec))) return rc;
  if ((rc = ddbh_coef("ddbh_bp_loss", y_p, right, left, lower_bound, upper_bound, percent, &cf))) return rc;
  if ((rc = open_ws("ddbh_bp_loss", workspace, workspace_bytes, carve_ddbh(nullptr, B).total, CMH_ERR_INVALID))) return rc;
  const DdbhWs w = carve_ddbh(workspace, B);
  hipStream_t st = as_stream(stream);
  const size_t Kp = align_up(K, 4), lds = (Kp + B) * sizeof(float) + align_up(B, 16);
  hipLaunchKernelGGL(ddbh_rows_kernel, dim3(B, calls), dim3(256), lds, st, p, labels, B, K, C, vec, cf, w.part, static_cast<DdbhRow*>(rows));
  hipLaunchKernelGGL(ddbh_finalize_kernel, dim3(calls), dim3(64), 0, st, w.part, static_cast<const DdbhRow*>(rows), B, loss, count);
  CMH_CHECK_LAUNCH("ddbh_bp_loss");
  return CMH_OK;
}

extern "C" int cmh_ddbh_bp_loss_backward(const float* const* u, const float* const* v, int32_t calls, const float* labels, int32_t B,
                                         int32_t K, int32_t C, double y_p, double right, double left, double lower_bound,
                                         double upper_bound, double percent, const void* rows, const int32_t* count, const float* dloss,
                                         float* const* du, float* const* dv, void* stream) {
  CMH_CHECK_ARG(u && v && labels && rows && count && dloss && du && dv, "ddbh_bp_loss_backward: null pointer");
  int rc = ddbh_shape("ddbh_bp_loss_backward", calls, B, K, C), vec = 0;
  if (rc) return rc;
  DdbhCalls p;
  DdbhCoef cf;
  if ((rc = ddbh_calls("ddbh_bp_loss_backward", calls, u, v, du, dv, K, &p, &vec))) return rc;
  if ((rc = ddbh_coef("ddbh_bp_loss_backward", y_p, right, left, lower_bound, upper_bound, percent, &cf))) return rc;
  const size_t Kp = align_up(K, 4), lds = (5 * Kp + B) * sizeof(float);
  hipLaunchKernelGGL(ddbh_backward_kernel, dim3(B, 2, calls), dim3(256), lds, as_stream(stream), p, labels, B, K, C, vec, static_cast<float>(cf.c),
                     static_cast<float>(cf.ac), static_cast<const DdbhRow*>(rows), count, dloss);
  CMH_CHECK_LAUNCH("ddbh_bp_loss_backward");
  return CMH_OK;
}

extern "C" int cmh_ddbh_quant_loss(const float* const* h, int32_t calls, const float* labels, int32_t B, int32_t K, int32_t C, float* loss,
                                   float* colsum, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(h && labels && loss && colsum, "ddbh_quant_loss: null pointer");
  int rc = ddbh_shape("ddbh_quant_loss", calls, B, K, C), vec = 0;
  if (rc) return rc;
  DdbhCalls p;
  if ((rc = ddbh_calls("ddbh_quant_loss", calls, h, nullptr, nullptr, nullptr, K, &p, &vec))) return rc;
  if ((rc = open_ws("ddbh_quant_loss", workspace, workspace_bytes, carve_ddbh(nullptr, B).total, CMH_ERR_INVALID))) return rc;
  const DdbhWs w = carve_ddbh(workspace, B);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ddbh_quant_rows_kernel, dim3(B, calls), dim3(256), 0, st, p, labels, B, K, C, w.part, colsum);
  hipLaunchKernelGGL(ddbh_quant_finalize_kernel, dim3(calls), dim3(64), 0, st, w.part, B, K, loss);
  CMH_CHECK_LAUNCH("ddbh_quant_loss");
  return CMH_OK;
}

extern "C" int cmh_ddbh_quant_loss_backward(const float* const* h, int32_t calls, const float* colsum, int32_t B, int32_t K, const float* dloss,
                                            float* const* dh, void* stream) {
  CMH_CHECK_ARG(h && colsum && dloss && dh, "ddbh_quant_loss_backward: null pointer");
  int rc = ddbh_shape("ddbh_quant_loss_backward", calls, B, K, 1), vec = 0;
  if (rc) return rc;
  DdbhCalls p;
  if ((rc = ddbh_calls("ddbh_quant_loss_backward", calls, h, nullptr, dh, nullptr, K, &p, &vec))) return rc;
  const size_t n = static_cast<size_t>(B) * K;
  hipLaunchKernelGGL(ddbh_quant_backward_kernel, dim3(static_cast<unsigned>((n + 255) / 256), calls), dim3(256), 0, as_stream(stream), p, colsum,
                     B, K, dloss);
  CMH_CHECK_LAUNCH("ddbh_quant_loss_backward");
  return CMH_OK;
}
