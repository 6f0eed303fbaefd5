// DJSRH joint-semantics target and reconstruction loss, forward and backward.  No upstream counterpart; the method is Su, Zhong, Zhang:
// "Deep Joint-Semantics Reconstructing Hashing for Large-Scale Unsupervised Cross-Modal Retrieval", ICCV 2019.
//
//   n(x) = x / max(|x|, 1e-12) per row (F.normalize)
//   target (no gradient):  St = beta (2 n(fi) n(fi)^T - 1) + (1 - beta) (2 n(ft) n(ft)^T - 1)          [B, B], symmetric
//                          S  = mu ((1 - eta) St + (eta / B) St St^T)                                    [B, B], symmetric
//   loss, b = n(h):        R_II = b_I b_I^T - S,  R_IT = b_I b_T^T - S,  R_TT = b_T b_T^T - S
//                          loss = lambda1 mean(R_II^2) + mean(R_IT^2) + lambda2 mean(R_TT^2)
//   backward, c = 2 dloss / B^2 (S symmetric, so R_II and R_TT are):
//                          g_I = c (2 lambda1 R_II b_I + R_IT b_T),  g_T = c (2 lambda2 R_TT b_T + R_IT^T b_I)
//                          dh  = (g - b (b . g)) / max(|h|, 1e-12) per row
//
// All three [B, B] builders are one walk (tile_walk): a 32 x 32 tile of row-by-row inner products per workgroup, the operand rows staged in LDS
// a chunk of 32 columns at a time, k-major with a pad column so that neither the staging store nor the reads meet a bank twice; thread
// (ty, tx) of 16 x 16 owns the outputs (ty, ty + 16) x (tx, tx + 16).  The products run on the f32 VALU, not the f32 MFMA: both have the same
// peak (64 FLOP / clk / SIMD) and the same bits (a k-ascending fmaf chain), and at these sizes (the default batch is 300: 100 tiles on 256
// CUs, 0.2 GFLOP) the calls are bound by launches and by how many tiles there are, not by issue rate; the VALU walk takes ragged B, K and
// D without a padded operand copy.  Every output element is one thread's fmaf chain in ascending k, so St and S are symmetric bit for bit
// (only the tiles on and above the diagonal are computed; each writes its mirror image) and two calls give the same bits.  The loss folds
// each tile's three sums of squares by a fixed-order workgroup sum, then one wave adds the tiles in ascending order: no atomics.
// The backward gives each workgroup four rows of one modality: the two coefficient rows per output row (R / the other side's norm) sit in
// LDS, wave w adds the batch rows w, w + 4, ... in order, lane l the code columns l and l + 64, the four waves' partials are added left
// to right, and the normaliser's backward finishes the rows in the same launch.
#include "head_common.h"

namespace cmh {

constexpr int kDjsrhMaxB = 1024, kDjsrhMaxK = 128, kDjsrhMaxD = 4096;
constexpr int kDjT = 32, kDjKC = 32, kDjRows = 4;                // tile edge, staged columns per chunk, rows per backward workgroup

// stage rows [r0, r0 + 32) x columns [k0, k0 + 32) of m [R, K] as s[k][r]; out-of-range entries are zeros (they add nothing to a chain)
__device__ __forceinline__ void stage_rows(const float* __restrict__ m, int R, int K, int r0, int k0, float (*s)[kDjT + 1]) {
  const int k = threadIdx.x & 31, r = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = r0 + r + 8 * q;
    s[k][r + 8 * q] = (row < R && k0 + k < K) ? m[static_cast<size_t>(row) * K + k0 + k] : 0.f;
  }
}

// acc[p][a][b] += rows (i0 + ty + 16 a) . rows (j0 + tx + 16 b) over all K columns, k ascending.  NM = 1: p = 0 is m0 . m0.
// NM = 2: p = 0 is m0 . m0 and p = 1 is m1 . m1; with CROSS, p = 2 is m0 (row side) . m1 (column side).
template <int NM, bool CROSS>
__device__ __forceinline__ void tile_walk(const float* __restrict__ m0, const float* __restrict__ m1, int R, int K, int i0, int j0,
                                          float (&acc)[3][2][2]) {
  __shared__ float si[NM][kDjKC][kDjT + 1], sj[NM][kDjKC][kDjT + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int p = 0; p < 3; ++p) acc[p][0][0] = acc[p][0][1] = acc[p][1][0] = acc[p][1][1] = 0.f;
  for (int k0 = 0; k0 < K; k0 += kDjKC) {
    __syncthreads();
    stage_rows(m0, R, K, i0, k0, si[0]);
    stage_rows(m0, R, K, j0, k0, sj[0]);
    if (NM == 2) {
      stage_rows(m1, R, K, i0, k0, si[NM - 1]);
      stage_rows(m1, R, K, j0, k0, sj[NM - 1]);
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kDjKC; ++k) {
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const float a0 = si[m][k][ty], a1 = si[m][k][ty + 16], b0 = sj[m][k][tx], b1 = sj[m][k][tx + 16];
        acc[m][0][0] = fmaf(a0, b0, acc[m][0][0]); acc[m][0][1] = fmaf(a0, b1, acc[m][0][1]);
        acc[m][1][0] = fmaf(a1, b0, acc[m][1][0]); acc[m][1][1] = fmaf(a1, b1, acc[m][1][1]);
      }
      if (CROSS) {
        const float a0 = si[0][k][ty], a1 = si[0][k][ty + 16], b0 = sj[NM - 1][k][tx], b1 = sj[NM - 1][k][tx + 16];
        acc[2][0][0] = fmaf(a0, b0, acc[2][0][0]); acc[2][0][1] = fmaf(a0, b1, acc[2][0][1]);
        acc[2][1][0] = fmaf(a1, b0, acc[2][1][0]); acc[2][1][1] = fmaf(a1, b1, acc[2][1][1]);
      }
    }
  }
}

// St, tiles with blockIdx.x >= blockIdx.y; fnorm [2B]: |fi rows| then |ft rows|, floored
__global__ __launch_bounds__(256) void djsrh_stilde_kernel(const float* __restrict__ fi, const float* __restrict__ ft,
                                                           const float* __restrict__ fnorm, int B, int D, float beta, float* __restrict__ st) {
  if (blockIdx.x < blockIdx.y) return;                      // the mirror image of a computed tile (uniform over the workgroup)
  const int i0 = blockIdx.y * kDjT, j0 = blockIdx.x * kDjT, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[3][2][2];
  tile_walk<2, false>(fi, ft, B, D, i0, j0, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i >= B || j >= B) continue;
      const float ci = acc[0][a][b] / (fnorm[i] * fnorm[j]), ct = acc[1][a][b] / (fnorm[B + i] * fnorm[B + j]);
      const float v = beta * (2.f * ci - 1.f) + (1.f - beta) * (2.f * ct - 1.f);
      st[static_cast<size_t>(i) * B + j] = v;
      if (blockIdx.x != blockIdx.y) st[static_cast<size_t>(j) * B + i] = v;
    }
}

// S = mu ((1 - eta) St + (eta / B) St St^T), tiles with blockIdx.x >= blockIdx.y
__global__ __launch_bounds__(256) void djsrh_s_kernel(const float* __restrict__ st, int B, float eta, float mu, float* __restrict__ S) {
  if (blockIdx.x < blockIdx.y) return;
  const int i0 = blockIdx.y * kDjT, j0 = blockIdx.x * kDjT, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[3][2][2];
  tile_walk<1, false>(st, nullptr, B, B, i0, j0, acc);
  const float keep = 1.f - eta, mix = eta / static_cast<float>(B);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i >= B || j >= B) continue;
      const float v = mu * (keep * st[static_cast<size_t>(i) * B + j] + mix * acc[0][a][b]);
      S[static_cast<size_t>(i) * B + j] = v;
      if (blockIdx.x != blockIdx.y) S[static_cast<size_t>(j) * B + i] = v;
    }
}

// every tile: the three cosines per (i, j) minus S; res (null: not kept) [3, B, B]; part [tiles, 3] the tile's sums of squares
__global__ __launch_bounds__(256) void djsrh_loss_tiles_kernel(const float* __restrict__ hi, const float* __restrict__ ht,
                                                               const float* __restrict__ hnorm, const float* __restrict__ S, int B, int K,
                                                               float* __restrict__ res, float* __restrict__ part) {
  __shared__ float red[4];
  const int i0 = blockIdx.y * kDjT, j0 = blockIdx.x * kDjT, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const size_t bb = static_cast<size_t>(B) * B;
  float acc[3][2][2];
  tile_walk<2, true>(hi, ht, B, K, i0, j0, acc);
  float sq_ii = 0.f, sq_it = 0.f, sq_tt = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i >= B || j >= B) continue;
      const size_t e = static_cast<size_t>(i) * B + j;
      const float s = S[e];
      const float r_ii = acc[0][a][b] / (hnorm[i] * hnorm[j]) - s;
      const float r_tt = acc[1][a][b] / (hnorm[B + i] * hnorm[B + j]) - s;
      const float r_it = acc[2][a][b] / (hnorm[i] * hnorm[B + j]) - s;
      if (res) { res[e] = r_ii; res[bb + e] = r_it; res[2 * bb + e] = r_tt; }
      sq_ii = fmaf(r_ii, r_ii, sq_ii); sq_it = fmaf(r_it, r_it, sq_it); sq_tt = fmaf(r_tt, r_tt, sq_tt);
    }
  sq_ii = block_sum_ltr(sq_ii, red);
  sq_it = block_sum_ltr(sq_it, red);
  sq_tt = block_sum_ltr(sq_tt, red);
  if (threadIdx.x == 0) {
    float* out = part + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * 3;
    out[0] = sq_ii; out[1] = sq_it; out[2] = sq_tt;
  }
}

// one wave: lane l adds tiles l, l + 64, ... in order, the butterfly adds the lanes; terms = (mean R_II^2, mean R_IT^2, mean R_TT^2)
__global__ __launch_bounds__(64) void djsrh_loss_finalize_kernel(const float* __restrict__ part, int tiles, int B, float lambda1, float lambda2,
                                                                 float* __restrict__ terms, float* __restrict__ loss) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < tiles; t += 64)
    for (int p = 0; p < 3; ++p) s[p] += static_cast<double>(part[static_cast<size_t>(t) * 3 + p]);
  const double n = static_cast<double>(B) * static_cast<double>(B);
  const float m_ii = static_cast<float>(wave_sum(s[0]) / n), m_it = static_cast<float>(wave_sum(s[1]) / n),
              m_tt = static_cast<float>(wave_sum(s[2]) / n);
  if (threadIdx.x == 0) {
    terms[0] = m_ii; terms[1] = m_it; terms[2] = m_tt;
    loss[0] = lambda1 * m_ii + m_it + lambda2 * m_tt;
  }
}

// blockIdx.y = 0: d_hi rows, 1: d_ht rows; four rows per workgroup.  own: the side's own codes, other: the other side's.
__global__ __launch_bounds__(256) void djsrh_backward_kernel(const float* __restrict__ hi, const float* __restrict__ ht,
                                                             const float* __restrict__ hnorm, const float* __restrict__ res, int B, int K,
                                                             float lambda1, float lambda2, const float* __restrict__ dloss,
                                                             float* __restrict__ d_hi, float* __restrict__ d_ht) {
  __shared__ float coef_own[kDjRows][kDjsrhMaxB], coef_other[kDjRows][kDjsrhMaxB];
  __shared__ float wave_part[4][kDjRows][kDjsrhMaxK];
  __shared__ float red[4];
  const int side = blockIdx.y, r0 = blockIdx.x * kDjRows, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t bb = static_cast<size_t>(B) * B;
  const float* own = side ? ht : hi;
  const float* other = side ? hi : ht;
  const float* n_own = hnorm + (side ? B : 0);
  const float* n_other = hnorm + (side ? 0 : B);
  const float* r_own = res + (side ? 2 * bb : 0);            // R_II or R_TT (symmetric)
  const float* r_it = res + bb;
  const float weight = 2.f * (side ? lambda2 : lambda1);
  float* out = side ? d_ht : d_hi;
  // coef_own[q][j] = 2 lambda R_own[i, j] / |own_j|;  coef_other[q][j] = R_IT[i, j] (image side) or R_IT[j, i] (text side) / |other_j|
  for (int e = tid; e < kDjRows * B; e += 256) {
    const int q = e / B, j = e - q * B, i = r0 + q;
    float co = 0.f, cx = 0.f;
    if (i < B) {
      co = weight * r_own[static_cast<size_t>(i) * B + j] / n_own[j];
      cx = (side ? r_it[static_cast<size_t>(j) * B + i] : r_it[static_cast<size_t>(i) * B + j]) / n_other[j];
    }
    coef_own[q][j] = co;
    coef_other[q][j] = cx;
  }
  __syncthreads();
  float acc[kDjRows][2];
#pragma unroll
  for (int q = 0; q < kDjRows; ++q) acc[q][0] = acc[q][1] = 0.f;
  const int k_lo = lane, k_hi = lane + 64;
  for (int j = w; j < B; j += 4) {
    const float* oj = own + static_cast<size_t>(j) * K;
    const float* xj = other + static_cast<size_t>(j) * K;
    const float o0 = k_lo < K ? oj[k_lo] : 0.f, o1 = k_hi < K ? oj[k_hi] : 0.f;
    const float x0 = k_lo < K ? xj[k_lo] : 0.f, x1 = k_hi < K ? xj[k_hi] : 0.f;
#pragma unroll
    for (int q = 0; q < kDjRows; ++q) {
      const float co = coef_own[q][j], cx = coef_other[q][j];
      acc[q][0] = fmaf(cx, x0, fmaf(co, o0, acc[q][0]));
      acc[q][1] = fmaf(cx, x1, fmaf(co, o1, acc[q][1]));
    }
  }
#pragma unroll
  for (int q = 0; q < kDjRows; ++q) { wave_part[w][q][k_lo] = acc[q][0]; wave_part[w][q][k_hi] = acc[q][1]; }
  __syncthreads();
  const float c = 2.f * dloss[0] / (static_cast<float>(B) * static_cast<float>(B));
  // the normaliser's backward: thread k < K of each row; b = h / n, dh = (g - b (b . g)) / n
  for (int q = 0; q < kDjRows; ++q) {
    const int i = r0 + q;                                    // uniform over the workgroup
    if (i >= B) break;
    const float n = n_own[i];
    float g = 0.f, b = 0.f;
    if (tid < K) {
      g = c * (((wave_part[0][q][tid] + wave_part[1][q][tid]) + wave_part[2][q][tid]) + wave_part[3][q][tid]);
      b = own[static_cast<size_t>(i) * K + tid] / n;
    }
    const float dot = block_sum_ltr(b * g, red);
    if (tid < K) out[static_cast<size_t>(i) * K + tid] = (g - b * dot) / n;
  }
}

}  // namespace cmh

using namespace cmh;

// fnorm / hnorm [2B]: row norms of the two feature (target) or code (loss without a tape) matrices; st [B, B]; part [tiles, 3]
struct DjsrhWs { float* norms; float* st; float* part; size_t total; };
static DjsrhWs carve_djsrh(void* ws, size_t B) {
  Carver c(ws);
  const size_t t = (B + kDjT - 1) / kDjT;
  return {c.f32(2 * B * sizeof(float)), c.f32(B * B * sizeof(float)), c.f32(t * t * 3 * sizeof(float)), c.total()};
}
static bool djsrh_in_range(int B, int K, int D) {
  return B >= 1 && B <= kDjsrhMaxB && K >= 1 && K <= kDjsrhMaxK && D >= 1 && D <= kDjsrhMaxD;
}

extern "C" size_t cmh_djsrh_workspace_bytes(int32_t B, int32_t K, int32_t D) {
  return djsrh_in_range(B, K, D) ? carve_djsrh(nullptr, B).total : 0;
}

// the shape, then the workspace: present, 256-byte aligned (the carver's slots assume it) and large enough
static int djsrh_open(const char* what, int B, int K, int D, const void* ws, size_t ws_bytes) {
  CMH_CHECK_ARG(djsrh_in_range(B, K, D), "%s: B=%d (1 .. %d) K=%d (1 .. %d) D=%d (1 .. %d)", what, B, kDjsrhMaxB, K, kDjsrhMaxK, D, kDjsrhMaxD);
  int rc = open_ws(what, ws, ws_bytes, carve_djsrh(nullptr, B).total, CMH_ERR_INVALID);
  if (rc) return rc;
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace is not 256-byte aligned", what);
  return CMH_OK;
}

extern "C" int cmh_djsrh_target(const float* fi, const float* ft, int32_t B, int32_t D, float beta, float eta, float mu, float* S,
                                void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(fi && ft && S, "djsrh_target: null pointer");
  int rc = djsrh_open("djsrh_target", B, 1, D, workspace, workspace_bytes);
  if (rc) return rc;
  const DjsrhWs w = carve_djsrh(workspace, B);
  hipStream_t st = as_stream(stream);
  const unsigned t = (B + kDjT - 1) / kDjT;
  launch_row_norms2(fi, ft, B, D, 1e-12f, w.norms, st);
  hipLaunchKernelGGL(djsrh_stilde_kernel, dim3(t, t), dim3(256), 0, st, fi, ft, w.norms, B, D, beta, w.st);
  hipLaunchKernelGGL(djsrh_s_kernel, dim3(t, t), dim3(256), 0, st, w.st, B, eta, mu, S);
  CMH_CHECK_LAUNCH("djsrh_target");
  return CMH_OK;
}

// tape f32 [2B + 3 B^2]: |hi rows|, |ht rows| (floored), then R_II, R_IT, R_TT
extern "C" int cmh_djsrh_loss(const float* hi, const float* ht, const float* S, int32_t B, int32_t K, float lambda1, float lambda2,
                              float* terms, float* loss, float* tape, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(hi && ht && S && terms && loss, "djsrh_loss: null pointer");
  int rc = djsrh_open("djsrh_loss", B, K, 1, workspace, workspace_bytes);
  if (rc) return rc;
  const DjsrhWs w = carve_djsrh(workspace, B);
  hipStream_t st = as_stream(stream);
  const unsigned t = (B + kDjT - 1) / kDjT;
  float* norms = tape ? tape : w.norms;
  launch_row_norms2(hi, ht, B, K, 1e-12f, norms, st);
  hipLaunchKernelGGL(djsrh_loss_tiles_kernel, dim3(t, t), dim3(256), 0, st, hi, ht, norms, S, B, K, tape ? tape + 2 * B : nullptr, w.part);
  hipLaunchKernelGGL(djsrh_loss_finalize_kernel, dim3(1), dim3(64), 0, st, w.part, static_cast<int>(t * t), B, lambda1, lambda2, terms, loss);
  CMH_CHECK_LAUNCH("djsrh_loss");
  return CMH_OK;
}

extern "C" int cmh_djsrh_loss_backward(const float* hi, const float* ht, const float* tape, int32_t B, int32_t K, float lambda1,
                                       float lambda2, const float* dloss, float* d_hi, float* d_ht, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(hi && ht && tape && dloss && d_hi && d_ht, "djsrh_loss_backward: null pointer");
  int rc = djsrh_open("djsrh_loss_backward", B, K, 1, workspace, workspace_bytes);      // (the tape holds all it reads; no slot is used)
  if (rc) return rc;
  hipLaunchKernelGGL(djsrh_backward_kernel, dim3((B + kDjRows - 1) / kDjRows, 2), dim3(256), 0, as_stream(stream), hi, ht, tape, tape + 2 * B,
                     B, K, lambda1, lambda2, dloss, d_hi, d_ht);
  CMH_CHECK_LAUNCH("djsrh_loss_backward");
  return CMH_OK;
}
