// DDWSH: the margin loss with learnable per-class boundaries over distance-weighted triplets, forward and backward: reference
// train/DDWSH/loss.py:16-49 `MarginLoss.forward(batch, labels, y)`, its miner (:91-128 `DistanceWeightedMiner.__call__`, :52-72
// `inverse_sphere_distances`, :75-79 `pdist`) and the three calls of a step (train/DDWSH/hash_train.py:68).
//
//   x^ = x / max(|x|, 1e-12) per row, y^ likewise;  D_ij = max(|x^_i - y^_j|, 1e-8)                                               (:17-20)
//   mining matrix: "distances" (what the reference runs, :22 hands the miner D itself): M_ij = max(sqrt(max(|D_i: - D_j:|^2, 1e-4)), cutoff)
//   with dim = B (:54, :75-79, :96);  "embeddings" (Wu et al., ICCV 2017): M = max(D, cutoff) with dim = K
//   anchor i: pos_j = (Y_j . Y_i > 0); used when sum(pos) > 1 and sum(pos) < B                                                     (:103-118)
//   log w_j = (2 - dim) log M_ij - ((dim - 3) / 2) log max(1 - M_ij^2 / 4, 1e-8), 0 where pos_j, BEFORE the maximum is taken;
//   w = exp(log w - max), 0 where pos_j;  the negative is drawn from w / sum w, the positive uniformly from pos without i          (:56-70, :120-122)
//   beta_i = sum_c Y_ic beta_c / sum_c Y_ic;  pos_i = relu((D[i, p_i] - beta_i) + m), neg_i = relu((beta_i - D[i, n_i]) + m)        (:37-43)
//   count = #{i: pos_i > 0 or neg_i > 0};  loss = sum (pos + neg) / count, the plain sum (0) when count = 0                      (:45-47)
//
// The reference copies the labels to the host, loops over the B anchors in Python, reads one row of M back per anchor and draws twice per
// anchor with numpy: 768 device-to-host reads per step at batch 256.  Here nothing leaves the GPU and the two uniforms per anchor are an
// INPUT (u [pairs, B, 2] in [0, 1)): the negative is the first j with cdf_j > u_n total over the ascending-index f64 running sum of w
// (numpy's searchsorted(side="right") on the normalised cdf; an item of weight 0 is never picked), the positive is the
// floor(u_p n)-th of the n positives other than i in index order.
//
// Launches.  cmh_dws_distances: one normalize_rows per DISTINCT operand (two for a step's three pairs) and one tile walk for D.
// cmh_dws_mine: the label bit rows, the [B, B, B] walk for M ("distances" only; symmetric, so only the tiles on and above the diagonal
// are computed) and the sampler, one workgroup per (anchor, pair).  cmh_dws_margin_loss: one wave per anchor, then one wave per pair folds
// the anchors in a fixed order.  Backward: one launch for du / dv (workgroup (row, side, pair); the column contributions to y^_j are
// found by a scan over the anchors in ascending order, not scattered) and one for dbeta (a thread per class).  A step's three pairs:
// 8 forward launches ("embeddings": 7), 2 backward.  f32 in and out, f64 sums in a fixed order, no atomics: two calls give the same bits.
//
// Both walks take the DIRECT difference form, sum_k (a_k - b_k)^2 as one k-ascending fmaf chain, where the reference expands
// n_i + n_j - 2 a . b (torch.cdist's matmul route above 25 rows, and its own pdist): the diagonal of an intra-modal D is exactly the
// 1e-8 clamp here, where the reference leaves 7e-4 .. 9e-4 of cancellation noise above 25 rows.  No triplet reads that diagonal.
#include "head_common.h"

namespace cmh {

constexpr int kDwsMaxB = 1024, kDwsMaxK = 128, kDwsMaxC = 1024, kDwsMaxPairs = 3, kDwsWords = kDwsMaxB / 64, kDwsLabelWords = kDwsMaxC / 64;
constexpr int kDwsT = 32, kDwsKC = 32;                       // tile edge and staged columns per chunk of the two walks

// a, b [R, K]: the rows the distances are taken between; sym: b == a, so only the tiles with blockIdx.x >= blockIdx.y are computed
struct DwsWalk { const float* a[kDwsMaxPairs]; const float* b[kDwsMaxPairs]; int sym[kDwsMaxPairs]; };

// ua, ub: the unit rows of the two sides, na, nb their divisors, da, db the gradients' buffers; intra: v == u
struct DwsPairs {
  const float* ua[kDwsMaxPairs]; const float* ub[kDwsMaxPairs]; const float* na[kDwsMaxPairs]; const float* nb[kDwsMaxPairs];
  float* da[kDwsMaxPairs]; float* db[kDwsMaxPairs]; int intra[kDwsMaxPairs];
};

// stage rows [r0, r0 + 32) x columns [k0, k0 + 32) of m [R, K] as s[k][r]; out-of-range entries are zeros on BOTH sides (a zero difference)
__device__ __forceinline__ void dws_stage(const float* __restrict__ m, int R, int K, int r0, int k0, float (*s)[kDwsT + 1]) {
  const int k = threadIdx.x & 31, r = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = r0 + r + 8 * q;
    s[k][r + 8 * q] = (row < R && k0 + k < K) ? m[static_cast<size_t>(row) * K + k0 + k] : 0.f;
  }
}

// grid (tiles, tiles, pairs).  out[pair, i, j] = max(sqrt(max(sum_k (a_ik - b_jk)^2, floor_sq)), floor): thread (ty, tx) of 16 x 16 owns
// (ty, ty + 16) x (tx, tx + 16), each one k-ascending fma chain of the f32 difference's square (symmetric in i and j bit for bit).
// Acc = float for D (K <= 128 terms).  Acc = double for the mining matrix: its chain has B terms and its result is raised to the power
// 2 - B, so a relative error e of M is B e in a weight - an f32 chain of 1024 terms would leave 1e-3 there, the f64 chain leaves the one
// rounding of the result to f32
template <typename Acc>
__global__ __launch_bounds__(256) void dws_walk_kernel(DwsWalk p, int R, int K, float floor_sq, float floor, float* __restrict__ out) {
  __shared__ float si[kDwsKC][kDwsT + 1], sj[kDwsKC][kDwsT + 1];
  const int pair = blockIdx.z, sym = p.sym[pair];
  if (sym && blockIdx.x < blockIdx.y) return;               // the mirror image of a computed tile (uniform over the workgroup)
  const float* a = p.a[pair];
  const float* b = p.b[pair];
  const int i0 = blockIdx.y * kDwsT, j0 = blockIdx.x * kDwsT, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  Acc acc[2][2] = {{0, 0}, {0, 0}};
  for (int k0 = 0; k0 < K; k0 += kDwsKC) {
    __syncthreads();
    dws_stage(a, R, K, i0, k0, si);
    dws_stage(b, R, K, j0, k0, sj);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kDwsKC; ++k) {
      const float a0 = si[k][ty], a1 = si[k][ty + 16], b0 = sj[k][tx], b1 = sj[k][tx + 16];
      const Acc d00 = a0 - b0, d01 = a0 - b1, d10 = a1 - b0, d11 = a1 - b1;
      acc[0][0] = fma(d00, d00, acc[0][0]); acc[0][1] = fma(d01, d01, acc[0][1]);
      acc[1][0] = fma(d10, d10, acc[1][0]); acc[1][1] = fma(d11, d11, acc[1][1]);
    }
  }
  float* o = out + static_cast<size_t>(pair) * R * R;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (i >= R || j >= R) continue;
      const float v = fmaxf(static_cast<float>(sqrt(fmax(acc[r][c], static_cast<Acc>(floor_sq)))), floor);
      o[static_cast<size_t>(i) * R + j] = v;
      if (sym && blockIdx.x != blockIdx.y) o[static_cast<size_t>(j) * R + i] = v;
    }
}

// one wave per row: bits [B, W] = the row's labels as bit words (bit c of word c / 64: Y_ic > 0)
__global__ __launch_bounds__(256) void dws_label_bits_kernel(const float* __restrict__ y, int B, int C, int W, unsigned long long* __restrict__ bits) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;                                     // uniform over the wave
  for (int w = 0; w < W; ++w) {
    const int c = w * 64 + lane;
    const unsigned long long m = __ballot(c < C && y[static_cast<size_t>(row) * C + c] > 0.f);
    if (lane == 0) bits[static_cast<size_t>(row) * W + w] = m;
  }
}

__device__ __forceinline__ double dws_block_max(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// grid (B, pairs).  m [pairs, B, B]: the mining matrix before its cutoff; uni [pairs, B, 2]; trip [pairs, B, 2]; wout [pairs, B, B] or null
__global__ __launch_bounds__(256) void dws_sample_kernel(const float* __restrict__ m, const unsigned long long* __restrict__ bits, int B, int W,
                                                         double dim, float cutoff, const float* __restrict__ uni, int32_t* __restrict__ trip,
                                                         double* __restrict__ wout) {
  __shared__ double cdf[kDwsMaxB];                           // log w, then w, then its running sum
  __shared__ unsigned long long ya[kDwsLabelWords], pos[kDwsWords];
  __shared__ double red[4];
  __shared__ int pick, last;
  const int i = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t anchor = static_cast<size_t>(pair) * B + i, row = anchor * B;
  for (int w = tid; w < W; w += 256) ya[w] = bits[static_cast<size_t>(i) * W + w];
  if (tid == 0) pick = -1;
  __syncthreads();
  const int rounds = (B + 255) / 256;                        // uniform: every wave ballots in every round
  for (int q = 0; q < rounds; ++q) {
    const int j = q * 256 + tid;
    bool s = false;
    if (j < B)
      for (int w = 0; w < W; ++w) s |= (ya[w] & bits[static_cast<size_t>(j) * W + w]) != 0ull;
    const unsigned long long ms = __ballot(s);
    if (lane == 0) pos[q * 4 + wv] = ms;
  }
  __syncthreads();
  const int words = rounds * 4;
  int n_pos = 0;
  for (int w = 0; w < words; ++w) n_pos += __popcll(pos[w]);
  double* wrow = wout ? wout + row : nullptr;
  if (!(n_pos > 1 && n_pos < B)) {                           // (:108, :64) - uniform over the workgroup
    if (wrow)
      for (int j = tid; j < B; j += 256) wrow[j] = 0.0;
    if (tid == 0) { trip[2 * anchor] = -1; trip[2 * anchor + 1] = -1; }
    return;
  }
  double top = 0.0;                                          // the positives' zeros take part in the maximum (:67-68)
  for (int j = tid; j < B; j += 256) {
    double lw = 0.0;
    if (!((pos[j >> 6] >> (j & 63)) & 1ull)) {
      const double d = static_cast<double>(fmaxf(m[row + j], cutoff));
      lw = (2.0 - dim) * log(d) - ((dim - 3.0) / 2.0) * log(fmax(1.0 - 0.25 * d * d, 1e-8));
    }
    cdf[j] = lw;
    top = fmax(top, lw);
  }
  top = dws_block_max(top, red);
  for (int j = tid; j < B; j += 256) {
    const double w = ((pos[j >> 6] >> (j & 63)) & 1ull) ? 0.0 : exp(cdf[j] - top);
    cdf[j] = w;
    if (wrow) wrow[j] = w;
  }
  __syncthreads();
  if (tid == 0) {                                            // the running sum in ascending index, one thread: monotone bit for bit
    double run = 0.0;
    int l = -1;
    for (int j = 0; j < B; ++j) {
      const double w = cdf[j];
      if (w > 0.0) l = j;
      run += w;
      cdf[j] = run;
    }
    last = l;
  }
  __syncthreads();
  const double total = cdf[B - 1], target = static_cast<double>(uni[2 * anchor + 1]) * total;
  for (int j = tid; j < B; j += 256)
    if (cdf[j] > target && (j == 0 ? 0.0 : cdf[j - 1]) <= target) pick = j;     // one j at most: the sum is monotone
  __syncthreads();
  if (tid == 0) {
    int neg = pick >= 0 ? pick : last;                       // u_n total >= total by rounding: the last item of positive weight
    if (!(total > 0.0)) neg = -1;                            // every weight underflowed: the reference's q is 0 / 0 and its draw raises
    int r = static_cast<int>(static_cast<double>(uni[2 * anchor]) * static_cast<double>(n_pos - 1));
    r = r < 0 ? 0 : (r > n_pos - 2 ? n_pos - 2 : r);
    int p = -1;
    for (int w = 0; w < words && p < 0; ++w) {
      unsigned long long msk = pos[w];
      if ((i >> 6) == w) msk &= ~(1ull << (i & 63));
      const int c = __popcll(msk);
      if (r >= c) { r -= c; continue; }
      for (; r > 0; --r) msk &= msk - 1;
      p = w * 64 + __builtin_ctzll(msk);
    }
    const bool ok = neg >= 0 && p >= 0;
    trip[2 * anchor] = ok ? p : -1;
    trip[2 * anchor + 1] = ok ? neg : -1;
  }
}

// a triplet handed in is checked before it indexes anything
__device__ __forceinline__ bool dws_triplet(const int32_t* __restrict__ trip, size_t anchor, int B, int* p, int* n) {
  *p = trip[2 * anchor];
  *n = trip[2 * anchor + 1];
  return *p >= 0 && *n >= 0 && *p < B && *n < B;
}

// one wave per anchor, grid (ceil(B / 4)).  tape [pairs, B, 4] = beta_i, [pos_i > 0], [neg_i > 0], sum_c Y_ic (zeros for a skipped anchor);
// part [pairs, B] f64 = pos_i + neg_i; act [pairs, B] = the OR of the two flags
__global__ __launch_bounds__(256) void dws_anchor_kernel(const float* __restrict__ dist, const int32_t* __restrict__ trip, int pairs,
                                                         const float* __restrict__ y, const float* __restrict__ beta, int B, int C, float margin,
                                                         float* __restrict__ tape, double* __restrict__ part, int32_t* __restrict__ act) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;                                       // uniform over the wave
  double num = 0.0, den = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double yc = static_cast<double>(y[static_cast<size_t>(i) * C + c]);
    num += yc * static_cast<double>(beta[c]);
    den += yc;
  }
  num = wave_sum(num); den = wave_sum(den);
  if (lane != 0) return;
  const float bi = den > 0.0 ? static_cast<float>(num / den) : 0.f;
  for (int pair = 0; pair < pairs; ++pair) {
    const size_t anchor = static_cast<size_t>(pair) * B + i;
    int p, n;
    float fp = 0.f, fn = 0.f, b = 0.f, ys = 0.f;
    double sum = 0.0;
    if (den > 0.0 && dws_triplet(trip, anchor, B, &p, &n)) {
      const float lp = fmaxf(__fadd_rn(__fsub_rn(dist[anchor * B + p], bi), margin), 0.f);
      const float ln = fmaxf(__fadd_rn(__fsub_rn(bi, dist[anchor * B + n]), margin), 0.f);
      fp = lp > 0.f ? 1.f : 0.f; fn = ln > 0.f ? 1.f : 0.f; b = bi; ys = static_cast<float>(den);
      sum = static_cast<double>(lp) + static_cast<double>(ln);
    }
    tape[4 * anchor] = b; tape[4 * anchor + 1] = fp; tape[4 * anchor + 2] = fn; tape[4 * anchor + 3] = ys;
    part[anchor] = sum;
    act[anchor] = (fp > 0.f || fn > 0.f) ? 1 : 0;
  }
}

// one wave per pair: lane l adds anchors l, l + 64, ... in order, the butterfly adds the lanes
__global__ __launch_bounds__(64) void dws_fold_kernel(const double* __restrict__ part, const int32_t* __restrict__ act, int B,
                                                      float* __restrict__ loss, int64_t* __restrict__ count) {
  const int pair = blockIdx.x;
  double s = 0.0, n = 0.0;                                   // n <= 1024: exact
  for (int i = threadIdx.x; i < B; i += 64) {
    s += part[static_cast<size_t>(pair) * B + i];
    n += static_cast<double>(act[static_cast<size_t>(pair) * B + i]);
  }
  s = wave_sum(s); n = wave_sum(n);
  if (threadIdx.x == 0) {
    loss[pair] = static_cast<float>(n > 0.0 ? s / n : s);
    count[pair] = static_cast<int64_t>(n);
  }
}

// d loss / d D[i, j] / D[i, j] for the one or two entries of anchor i's row, through the clamp (nothing where D <= 1e-8)
__device__ __forceinline__ float dws_edge(const float* __restrict__ dist, size_t anchor, int B, int j, float flag, float scale) {
  const float d = dist[anchor * B + j];
  return (flag > 0.f && d > 1e-8f) ? scale / d : 0.f;
}

// grid (B, 2, pairs).  side 0: row b of u as the ANCHOR, g = cp (x^_b - y^_p) + cn (x^_b - y^_n); side 1: row b of v as a positive or a
// negative of the anchors i in ascending order, g = sum_i c_i (y^_b - x^_i); intra: side 0 takes both, side 1 nothing.  Then the
// normaliser's backward on the row (l2norm_bwd_kernel's arithmetic, as msc.hip)
__global__ __launch_bounds__(256) void dws_backward_kernel(DwsPairs q, int B, int K, const float* __restrict__ dist, const int32_t* __restrict__ trip,
                                                           const float* __restrict__ tape, const int64_t* __restrict__ count,
                                                           const float* __restrict__ dloss) {
  __shared__ float coef[kDwsMaxB];                           // the anchors' coefficients on column b
  __shared__ float red[4];
  const int b = blockIdx.x, side = blockIdx.y, pair = blockIdx.z, tid = threadIdx.x;
  const int intra = q.intra[pair];
  if (intra && side) return;                                 // uniform over the workgroup
  const float* own = side ? q.ub[pair] : q.ua[pair];
  const float* n_own = side ? q.nb[pair] : q.na[pair];
  float* out = (side ? q.db[pair] : q.da[pair]) + static_cast<size_t>(b) * K;
  const int64_t cnt = count[pair];
  const float scale = static_cast<float>(static_cast<double>(dloss[pair]) / static_cast<double>(cnt > 0 ? cnt : 1));
  const size_t base = static_cast<size_t>(pair) * B;
  const bool cols = side || intra;
  if (cols)
    for (int i = tid; i < B; i += 256) {
      int p, n;
      float c = 0.f;
      if (dws_triplet(trip, base + i, B, &p, &n)) {           // p != n: one shares a label with the anchor, the other does not
        if (p == b) c = dws_edge(dist, base + i, B, p, tape[4 * (base + i) + 1], scale);
        else if (n == b) c = -dws_edge(dist, base + i, B, n, tape[4 * (base + i) + 2], scale);
      }
      coef[i] = c;
    }
  __syncthreads();
  float g = 0.f, u = 0.f;
  if (tid < K) {
    u = own[static_cast<size_t>(b) * K + tid];
    int p, n;
    if (!side && dws_triplet(trip, base + b, B, &p, &n)) {
      const float cp = dws_edge(dist, base + b, B, p, tape[4 * (base + b) + 1], scale);
      const float cn = -dws_edge(dist, base + b, B, n, tape[4 * (base + b) + 2], scale);
      g = fmaf(cp, u - q.ub[pair][static_cast<size_t>(p) * K + tid], g);
      g = fmaf(cn, u - q.ub[pair][static_cast<size_t>(n) * K + tid], g);
    }
    if (cols)
      for (int i = 0; i < B; ++i) {
        const float c = coef[i];
        if (c != 0.f) g = fmaf(c, u - q.ua[pair][static_cast<size_t>(i) * K + tid], g);
      }
  }
  // dx = (g - u (u . g)) / n; below the eps clamp u = x / eps is linear
  const float dot = block_sum_ltr(u * g, red), nrm = n_own[b];
  const float proj = nrm > 1e-12f ? dot : 0.f;
  if (tid < K) out[tid] = (g - u * proj) / nrm;
}

// a thread per class: dbeta_c = sum_pairs sum_i (-[pos_i > 0] + [neg_i > 0]) dloss / count  Y_ic / sum_c Y_ic, pairs then anchors ascending
__global__ __launch_bounds__(256) void dws_dbeta_kernel(const float* __restrict__ y, const float* __restrict__ tape, const int64_t* __restrict__ count,
                                                        const float* __restrict__ dloss, int pairs, int B, int C, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double g = 0.0;
  for (int pair = 0; pair < pairs; ++pair) {
    const int64_t cnt = count[pair];
    const double scale = static_cast<double>(dloss[pair]) / static_cast<double>(cnt > 0 ? cnt : 1);
    for (int i = 0; i < B; ++i) {
      const float* t = tape + 4 * (static_cast<size_t>(pair) * B + i);
      const float e = t[2] - t[1];
      if (e != 0.f) g += scale * static_cast<double>(e) * static_cast<double>(y[static_cast<size_t>(i) * C + c]) / static_cast<double>(t[3]);
    }
  }
  dbeta[c] = static_cast<float>(g);
}

}  // namespace cmh

using namespace cmh;

// bits [B, W] label words; mine [pairs, B, B] the mining matrix; part / act [pairs, B] the anchors' terms
struct DwsWs { unsigned long long* bits; float* mine; double* part; int32_t* act; size_t total; };
static DwsWs carve_dws(void* ws, size_t B, size_t C) {
  Carver c(ws);
  return {c.take<unsigned long long>(B * ((C + 63) / 64) * 8), c.f32(kDwsMaxPairs * B * B * 4), c.take<double>(kDwsMaxPairs * B * 8),
          c.take<int32_t>(kDwsMaxPairs * B * 4), c.total()};
}

static bool dws_in_range(int B, int K, int C) { return B >= 1 && B <= kDwsMaxB && K >= 1 && K <= kDwsMaxK && C >= 1 && C <= kDwsMaxC; }

extern "C" size_t cmh_dws_workspace_bytes(int32_t B, int32_t K, int32_t C) { return dws_in_range(B, K, C) ? carve_dws(nullptr, B, C).total : 0; }

static int dws_shape(const char* what, int pairs, int B, int K, int C) {
  CMH_CHECK_ARG(pairs >= 1 && pairs <= kDwsMaxPairs, "%s: pairs=%d (1 .. %d)", what, pairs, kDwsMaxPairs);
  CMH_CHECK_ARG(dws_in_range(B, K, C), "%s: B=%d (1 .. %d) K=%d (1 .. %d) C=%d (1 .. %d)", what, B, kDwsMaxB, K, kDwsMaxK, C, kDwsMaxC);
  return CMH_OK;
}

static int dws_open(const char* what, void* workspace, size_t bytes, int B, int C) {
  if (int rc = open_ws(what, workspace, bytes, carve_dws(nullptr, B, C).total, CMH_ERR_INVALID)) return rc;
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace is not 256-byte aligned", what);
  return CMH_OK;
}

// The operands of the pairs: every DISTINCT operand pointer has one slot of unit [2 pairs, B, K] / divisor [2 pairs, B], the index of its
// first appearance in u[0], v[0], u[1], ... (msc.hip's rule) - the forward fills the slots, the backward finds them again from the same
// pointers.  slot_of (optional) receives each slot's operand, null for a slot that is not used.
static int dws_pairs(const char* what, int n, const float* const* u, const float* const* v, float* const* du, float* const* dv, int B, int K,
                     const float* unit, const float* divisor, DwsPairs* out, const float** slot_of) {
  const float* seen[2 * kDwsMaxPairs] = {};
  for (int q = 0; q < kDwsMaxPairs; ++q) {
    const int s = q < n ? q : 0;                              // unused entries repeat the first pair's
    CMH_CHECK_ARG(u[s] && v[s], "%s: null pointer in pair %d", what, s);
    const bool intra = u[s] == v[s];
    CMH_CHECK_ARG(!du || (du[s] && (intra || dv[s])), "%s: null gradient pointer in pair %d", what, s);
    const float* op[2] = {u[s], v[s]};
    const float* rows[2];
    const float* div[2];
    for (int t = 0; t < 2; ++t) {
      int slot = 0;
      while (seen[slot] && seen[slot] != op[t]) ++slot;       // at most 2 n distinct operands: a free slot exists
      seen[slot] = op[t];
      rows[t] = unit + static_cast<size_t>(slot) * B * K;
      div[t] = divisor + static_cast<size_t>(slot) * B;
    }
    out->ua[q] = rows[0]; out->ub[q] = rows[1]; out->na[q] = div[0]; out->nb[q] = div[1];
    out->da[q] = du ? du[s] : nullptr; out->db[q] = du && !intra ? dv[s] : nullptr; out->intra[q] = intra;
  }
  if (slot_of)
    for (int t = 0; t < 2 * kDwsMaxPairs; ++t) slot_of[t] = seen[t];
  return CMH_OK;
}

extern "C" int cmh_dws_distances(const float* const* u, const float* const* v, int32_t pairs, int32_t B, int32_t K, float* dist, float* unit,
                                 float* divisor, void* stream) {
  CMH_CHECK_ARG(u && v && dist && unit && divisor, "dws_distances: null pointer");
  int rc = dws_shape("dws_distances", pairs, B, K, 1);
  if (rc) return rc;
  DwsPairs p;
  const float* slot_of[2 * kDwsMaxPairs];
  if ((rc = dws_pairs("dws_distances", pairs, u, v, nullptr, nullptr, B, K, unit, divisor, &p, slot_of))) return rc;
  hipStream_t st = as_stream(stream);
  for (int t = 0; t < 2 * kDwsMaxPairs && slot_of[t]; ++t)
    launch_normalize_rows(slot_of[t], unit + static_cast<size_t>(t) * B * K, divisor + static_cast<size_t>(t) * B, B, K, 1e-12f, nullptr, st);
  DwsWalk w;
  for (int q = 0; q < kDwsMaxPairs; ++q) { w.a[q] = p.ua[q]; w.b[q] = p.ub[q]; w.sym[q] = p.intra[q]; }
  const int tiles = (B + kDwsT - 1) / kDwsT;
  hipLaunchKernelGGL(dws_walk_kernel<float>, dim3(tiles, tiles, pairs), dim3(256), 0, st, w, B, K, 0.f, 1e-8f, dist);
  CMH_CHECK_LAUNCH("dws_distances");
  return CMH_OK;
}

extern "C" int cmh_dws_mine(const float* dist, int32_t pairs, const float* labels, int32_t B, int32_t K, int32_t C, float cutoff, int32_t space,
                            const float* uniforms, int32_t* triplets, double* weights, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(dist && labels && uniforms && triplets, "dws_mine: null pointer");
  CMH_CHECK_ARG(space == 0 || space == 1, "dws_mine: space=%d (0: distances, 1: embeddings)", space);
  int rc = dws_shape("dws_mine", pairs, B, K, C);
  if (rc) return rc;
  if ((rc = dws_open("dws_mine", workspace, workspace_bytes, B, C))) return rc;
  const DwsWs w = carve_dws(workspace, B, C);
  hipStream_t st = as_stream(stream);
  const int W = (C + 63) / 64;
  hipLaunchKernelGGL(dws_label_bits_kernel, dim3((B + 3) / 4), dim3(256), 0, st, labels, B, C, W, w.bits);
  const float* mine = dist;
  if (space == 0) {                                          // the rows of D as the miner's batch (reference :22, :96)
    DwsWalk k;
    for (int q = 0; q < kDwsMaxPairs; ++q) {
      k.a[q] = k.b[q] = dist + static_cast<size_t>(q < pairs ? q : 0) * B * B;
      k.sym[q] = 1;
    }
    const int tiles = (B + kDwsT - 1) / kDwsT;
    hipLaunchKernelGGL(dws_walk_kernel<double>, dim3(tiles, tiles, pairs), dim3(256), 0, st, k, B, B, 1e-4f, 0.f, w.mine);
    mine = w.mine;
  }
  hipLaunchKernelGGL(dws_sample_kernel, dim3(B, pairs), dim3(256), 0, st, mine, w.bits, B, W, static_cast<double>(space == 0 ? B : K), cutoff,
                     uniforms, triplets, weights);
  CMH_CHECK_LAUNCH("dws_mine");
  return CMH_OK;
}

extern "C" int cmh_dws_margin_loss(const float* dist, const int32_t* triplets, int32_t pairs, const float* labels, const float* beta, int32_t B,
                                   int32_t C, float margin, float* loss, int64_t* count, float* tape, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  CMH_CHECK_ARG(dist && triplets && labels && beta && loss && count && tape, "dws_margin_loss: null pointer");
  int rc = dws_shape("dws_margin_loss", pairs, B, 1, C);
  if (rc) return rc;
  if ((rc = dws_open("dws_margin_loss", workspace, workspace_bytes, B, C))) return rc;
  const DwsWs w = carve_dws(workspace, B, C);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dws_anchor_kernel, dim3((B + 3) / 4), dim3(256), 0, st, dist, triplets, pairs, labels, beta, B, C, margin, tape, w.part, w.act);
  hipLaunchKernelGGL(dws_fold_kernel, dim3(pairs), dim3(64), 0, st, w.part, w.act, B, loss, count);
  CMH_CHECK_LAUNCH("dws_margin_loss");
  return CMH_OK;
}

extern "C" int cmh_dws_margin_loss_backward(const float* const* u, const float* const* v, int32_t pairs, const float* labels, int32_t B, int32_t K,
                                            int32_t C, const float* dist, const int32_t* triplets, const float* tape, const int64_t* count,
                                            const float* unit, const float* divisor, const float* dloss, float* const* du, float* const* dv,
                                            float* dbeta, void* stream) {
  CMH_CHECK_ARG(u && v && labels && dist && triplets && tape && count && unit && divisor && dloss && du && dv && dbeta,
                "dws_margin_loss_backward: null pointer");
  int rc = dws_shape("dws_margin_loss_backward", pairs, B, K, C);
  if (rc) return rc;
  DwsPairs p;
  if ((rc = dws_pairs("dws_margin_loss_backward", pairs, u, v, du, dv, B, K, unit, divisor, &p, nullptr))) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dws_backward_kernel, dim3(B, 2, pairs), dim3(256), 0, st, p, B, K, dist, triplets, tape, count, dloss);
  hipLaunchKernelGGL(dws_dbeta_kernel, dim3((C + 255) / 256), dim3(256), 0, st, labels, tape, count, dloss, pairs, B, C, dbeta);
  CMH_CHECK_LAUNCH("dws_margin_loss_backward");
  return CMH_OK;
}
