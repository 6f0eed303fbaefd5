// Training-free hash heads from paired features (no upstream counterpart): LSH, PCAH and ITQ (Gong & Lazebnik, CVPR 2011) fitted on
// the GPU in f64.  The fit ends in one affine map per modality, code = sign(W_m f + b_m), which is a LinearHash head.
//
//   moments      running sums  sum_n f  and  sum_n f f^T  of one batch of f32 features (widened to f64)
//   covariance   mu_m, alpha_m = 1 / sqrt(mean_n |f - mu_m|^2), C = 1/2 sum_m alpha_m^2 (sum f f^T / N - mu_m mu_m^T)
//   eigh         cyclic Jacobi on C in round-robin order: one launch per set of disjoint rotations
//   project      V = alpha_m (F_m - mu_m) P
//   step         Z = V R, B = (Z >= 0 ? +1 : -1), M = B^T V, |B - Z|^2, |Z|^2
//   polar        R <- (orthogonal polar factor of M)^T by a one-sided Jacobi SVD, one workgroup
//   rotate       `iters` times step + polar, then one more step for the final objective; no host read in the loop
//   heads        s = 0.5 / rms(V R), W_m = s alpha_m (P_m R)^T as f32, b_m = -W_m mu_m
//
// CCA projections (one P_m per modality, the cross-modal variant of the same paper) add
//   cross moments    running sum  sum_n f_i f_t^T  (the X^T Y kernel with X != Y)
//   cca covariance   S_mm = alpha_m^2 (sum f f^T / N - mu_m mu_m^T), S_it = alpha_i alpha_t (sum f_i f_t^T / N - mu_i mu_t^T)
//   inv_sqrt         1 / sqrt(lambda + shift): the whitener's spectrum and 1 / sigma
//   matmul           C = op(A) diag(d) op(B) diag(cs), sizes up to 1024: the whiteners H_m = E_m diag((lambda + r)^-1/2) E_m^T,
//                    T = H_i S_it H_t, G = T T^T, v_j = T^T u_j / sigma_j and A_m = H_m [U_K | V_K]
//
// Determinism: fit_common.h states it, with the chunked products, the block reduction and the covariance element that dch.hip shares.
#include "fit_common.h"

#include <cfloat>
#include <cmath>

namespace cmh {
namespace {

// ---- covariance ---------------------------------------------------------------------------------------------------------------
// block m (0 image, 1 text): mu_m = sum / N; alpha_m = 1 / sqrt(sum_d (sq[d][d] / N - mu[d]^2)), 0 where that trace is not positive
__global__ __launch_bounds__(256) void moments_finish_kernel(const double* __restrict__ sum_i, const double* __restrict__ sq_i,
                                                             const double* __restrict__ sum_t, const double* __restrict__ sq_t, double inv_n,
                                                             int D, double* __restrict__ mu_i, double* __restrict__ mu_t,
                                                             double* __restrict__ alpha2) {
  __shared__ double sh[256];
  const double* sum = blockIdx.x ? sum_t : sum_i;
  const double* sq = blockIdx.x ? sq_t : sq_i;
  double* mu = blockIdx.x ? mu_t : mu_i;
  double tr = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) {
    const double m = sum[d] * inv_n;
    mu[d] = m;
    tr += sq[static_cast<size_t>(d) * D + d] * inv_n - m * m;
  }
  tr = block_sum<256>(tr, sh);
  if (threadIdx.x == 0) alpha2[blockIdx.x] = tr > 0.0 ? 1.0 / sqrt(tr) : 0.0;
}

__global__ __launch_bounds__(256) void covariance_kernel(const double* __restrict__ sq_i, const double* __restrict__ sq_t,
                                                         const double* __restrict__ mu_i, const double* __restrict__ mu_t,
                                                         const double* __restrict__ alpha2, double inv_n, int D, double* __restrict__ C) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<size_t>(D) * D) return;
  const int i = static_cast<int>(e / D), j = static_cast<int>(e % D);
  const double ai = alpha2[0] * alpha2[0], at = alpha2[1] * alpha2[1];
  // the scales come in below, where ai ci + at ct is one contraction: the elements are taken with scale 1, which is no operation
  const double ci = cov_element(1.0, sq_i[e], inv_n, mu_i[i], mu_i[j]), ct = cov_element(1.0, sq_t[e], inv_n, mu_t[i], mu_t[j]);
  C[e] = 0.5 * (ai * ci + at * ct);
}

// S_ii, S_tt (symmetric bit for bit: sq is, and mu[i] mu[j] commutes) and S_it for the CCA projections
__global__ __launch_bounds__(256) void cca_covariance_kernel(const double* __restrict__ sq_i, const double* __restrict__ sq_t,
                                                             const double* __restrict__ cross, const double* __restrict__ mu_i,
                                                             const double* __restrict__ mu_t, const double* __restrict__ alpha2, double inv_n,
                                                             int D, double* __restrict__ S_ii, double* __restrict__ S_tt,
                                                             double* __restrict__ S_it) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<size_t>(D) * D) return;
  const int i = static_cast<int>(e / D), j = static_cast<int>(e % D);
  const double ai = alpha2[0], at = alpha2[1];
  S_ii[e] = cov_element(ai * ai, sq_i[e], inv_n, mu_i[i], mu_i[j]);
  S_tt[e] = cov_element(at * at, sq_t[e], inv_n, mu_t[i], mu_t[j]);
  S_it[e] = cov_element(ai * at, cross[e], inv_n, mu_i[i], mu_t[j]);
}

// out[j] = 1 / sqrt(v[j] + shift), 0 where v[j] + shift is not positive; root[j] (optional) = sqrt(max(v[j] + shift, 0))
__global__ __launch_bounds__(256) void inv_sqrt_kernel(const double* __restrict__ v, int n, double shift, double* __restrict__ out,
                                                       double* __restrict__ root) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double x = v[j] + shift;
  const double r = x > 0.0 ? sqrt(x) : 0.0;
  out[j] = x > 0.0 ? 1.0 / r : 0.0;
  if (root) root[j] = r;
}

// ---- a small dense product ----------------------------------------------------------------------------------------------------
// C[i][j] = cs[j] * sum_k op(A)[i][k] d[k] op(B)[k][j], k ascending: one chain acc = fma(a b, d, acc) (fma(a, b, acc) without d),
// whatever the grid is.  a b is rounded before d comes in, and a b = b a, so op(A) = op(B)^T gives C[i][j] and C[j][i] the same
// bits, with or without d.  op(A) is A [M, Kc] or (TA) the transpose of A [Kc, M]; op(B) is B [Kc, N] or (TB) the transpose of
// B [N, Kc]; d [Kc] and cs [N] are optional.  Every operand goes through LDS: an operand whose contraction index is the fast one in
// memory is read 16 consecutive doubles per row of the tile, the other 64, so no read strides through memory.  One block: a
// 64 x 64 tile of C, thread (ti, tj) holds i = 4 ti + a, j = tj + 16 b, as in the X^T Y kernel.
template <bool TA, bool TB, bool HasD>
__global__ __launch_bounds__(256) void matmul_kernel(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ d,
                                                     const double* __restrict__ cs, double* __restrict__ C, int M, int N, int Kc) {
  __shared__ double xs[kStage][kTile + 1];      // op(A)[i0 + c][k0 + r]
  __shared__ double ys[kStage][kTile + 1];      // op(B)[k0 + r][j0 + c]
  __shared__ double ds[kStage];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int j0 = blockIdx.x * kTile, i0 = blockIdx.y * kTile;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < Kc; k0 += kStage) {
    for (int t = tid; t < kStage * kTile; t += 256) {
      {
        const int r = TA ? t >> 6 : t & 15, c = TA ? t & 63 : t >> 4;
        const bool in = k0 + r < Kc && i0 + c < M;
        xs[r][c] = in ? (TA ? A[static_cast<size_t>(k0 + r) * M + i0 + c] : A[static_cast<size_t>(i0 + c) * Kc + k0 + r]) : 0.0;
      }
      {
        const int r = TB ? t & 15 : t >> 6, c = TB ? t >> 4 : t & 63;
        const bool in = k0 + r < Kc && j0 + c < N;
        ys[r][c] = in ? (TB ? B[static_cast<size_t>(j0 + c) * Kc + k0 + r] : B[static_cast<size_t>(k0 + r) * N + j0 + c]) : 0.0;
      }
    }
    if (HasD && tid < kStage) ds[tid] = k0 + tid < Kc ? d[k0 + tid] : 0.0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kStage; ++r) {
      double xv[4], yv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xv[a] = xs[r][ti * 4 + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) yv[b] = ys[r][tj + 16 * b];
      const double dv = HasD ? ds[r] : 1.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = HasD ? fma(xv[a] * yv[b], dv, acc[a][b]) : fma(xv[a], yv[b], acc[a][b]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ti * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tj + 16 * b;
      if (i < M && j < N) C[static_cast<size_t>(i) * N + j] = cs ? cs[j] * acc[a][b] : acc[a][b];
    }
  }
}

// ---- symmetric eigen-solver: cyclic Jacobi, round-robin order ----------------------------------------------------------------
// The n = D rounded up to even indices meet in n - 1 steps of n / 2 disjoint pairs (a round-robin tournament; index D of an odd D
// is a bye).  Step `step`: pair 0 = (n - 1, step), pair k = ((step + k) mod (n - 1), (step - k) mod (n - 1)).
__host__ __device__ __forceinline__ void rr_pair(int n, int step, int k, int& p, int& q) {
  int a, b;
  if (k == 0) {
    a = n - 1;
    b = step;
  } else {
    a = (step + k) % (n - 1);
    b = (step - k + (n - 1)) % (n - 1);
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

__device__ __forceinline__ double rot_lo(double c, double s, double x0, double x1) { return fma(c, x0, -(s * x1)); }   // c x0 - s x1
__device__ __forceinline__ double rot_hi(double c, double s, double x0, double x1) { return fma(s, x0, c * x1); }      // s x0 + c x1

// A0[i][j] = C[min(i,j)][max(i,j)] (the upper triangle is read); E = I; cnt = 0
__global__ __launch_bounds__(256) void jacobi_init_kernel(const double* __restrict__ C, double* __restrict__ A, double* __restrict__ E,
                                                          int32_t* __restrict__ cnt, int D, int max_sweeps) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e < static_cast<size_t>(max_sweeps)) cnt[e] = 0;
  if (e >= static_cast<size_t>(D) * D) return;
  const int i = static_cast<int>(e / D), j = static_cast<int>(e % D);
  A[e] = i <= j ? C[e] : C[static_cast<size_t>(j) * D + i];
  E[e] = i == j ? 1.0 : 0.0;
}

// One step: Aout = J^T Ain J and E <- E J, J the product of the step's disjoint rotations.  Every block forms all n / 2 rotations
// from Ain (thread k: pair k), then block b writes the rows of its own pair: thread k the 2 x 2 block at the columns of pair k.
// Row rotation first where b < k, column rotation first where b > k: the block (b, k) and its transpose (k, b) then run the same
// operations on the same numbers, so a symmetric Ain gives a symmetric Aout, bit for bit.  Pair k is rotated where
// |a_pq| > eps sqrt(|a_pp a_qq|); block 0 adds the number of rotated pairs to *cnt (launches of one stream run in order).
template <int T>
__global__ __launch_bounds__(T) void jacobi_step_kernel(const double* __restrict__ Ain, double* __restrict__ Aout, double* __restrict__ E,
                                                        int32_t* __restrict__ cnt, int D, int n, int step, double eps) {
  __shared__ double cs[T], sn[T];
  const int k = threadIdx.x, half = n >> 1, b = blockIdx.x;
  int pk = 0, qk = 0, rotated = 0;
  double c = 1.0, s = 0.0, t = 0.0;
  if (k < half) {
    rr_pair(n, step, k, pk, qk);
    if (qk < D) {
      const double app = Ain[static_cast<size_t>(pk) * D + pk], aqq = Ain[static_cast<size_t>(qk) * D + qk];
      const double apq = Ain[static_cast<size_t>(pk) * D + qk];
      if (apq != 0.0 && fabs(apq) > eps * sqrt(fabs(app) * fabs(aqq))) {
        const double theta = (aqq - app) / (2.0 * apq);
        t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
        c = 1.0 / sqrt(1.0 + t * t);
        s = t * c;
        rotated = 1;
      }
    }
    cs[k] = c;
    sn[k] = s;
  }
  const int total = __syncthreads_count(rotated);
  if (b == 0 && k == 0) *cnt += total;
  if (k >= half) return;
  int P, Q;
  rr_pair(n, step, b, P, Q);
  const bool hasQ = Q < D, hasq = qk < D;
  const double cb = cs[b], sb = sn[b];
  const size_t rP = static_cast<size_t>(P) * D, rQ = static_cast<size_t>(Q) * D;
  double x00 = Ain[rP + pk], x01 = hasq ? Ain[rP + qk] : 0.0;
  double x10 = hasQ ? Ain[rQ + pk] : 0.0, x11 = (hasQ && hasq) ? Ain[rQ + qk] : 0.0;
  if (k == b) {
    if (rotated) {              // the pair's own 2 x 2 block: a_pp - t a_pq, a_qq + t a_pq, and the pivot exactly zero
      const double d = t * x01;
      x00 -= d;
      x11 += d;
      x01 = 0.0;
      x10 = 0.0;
    }
  } else if (b < k) {
    const double y00 = rot_lo(cb, sb, x00, x10), y10 = rot_hi(cb, sb, x00, x10);
    const double y01 = rot_lo(cb, sb, x01, x11), y11 = rot_hi(cb, sb, x01, x11);
    x00 = rot_lo(c, s, y00, y01);
    x01 = rot_hi(c, s, y00, y01);
    x10 = rot_lo(c, s, y10, y11);
    x11 = rot_hi(c, s, y10, y11);
  } else {
    const double y00 = rot_lo(c, s, x00, x01), y01 = rot_hi(c, s, x00, x01);
    const double y10 = rot_lo(c, s, x10, x11), y11 = rot_hi(c, s, x10, x11);
    x00 = rot_lo(cb, sb, y00, y10);
    x10 = rot_hi(cb, sb, y00, y10);
    x01 = rot_lo(cb, sb, y01, y11);
    x11 = rot_hi(cb, sb, y01, y11);
  }
  Aout[rP + pk] = x00;
  if (hasq) Aout[rP + qk] = x01;
  if (hasQ) {
    Aout[rQ + pk] = x10;
    if (hasq) Aout[rQ + qk] = x11;
  }
  if (hasq) {                   // E <- E J on the block's rows
    const double e0 = E[rP + pk], e1 = E[rP + qk];
    E[rP + pk] = rot_lo(c, s, e0, e1);
    E[rP + qk] = rot_hi(c, s, e0, e1);
    if (hasQ) {
      const double f0 = E[rQ + pk], f1 = E[rQ + qk];
      E[rQ + pk] = rot_lo(c, s, f0, f1);
      E[rQ + qk] = rot_hi(c, s, f0, f1);
    }
  }
}

// Block j: eigenvalue j = A[j][j] goes to position rank = #{i : lambda_i > lambda_j, or lambda_i == lambda_j and i < j} (descending,
// ties by index); its vector, column j of E, is signed so that its entry of largest magnitude (lowest row on a tie) is positive.
__global__ __launch_bounds__(256) void jacobi_finish_kernel(const double* __restrict__ A, const double* __restrict__ E, int D,
                                                            double* __restrict__ evals, double* __restrict__ evecs) {
  __shared__ double sh[256];
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  const double lj = A[static_cast<size_t>(j) * D + j];
  double cnt = 0.0;
  double best = -1.0;
  int best_i = D;
  for (int i = tid; i < D; i += 256) {
    const double li = A[static_cast<size_t>(i) * D + i];
    if (li > lj || (li == lj && i < j)) cnt += 1.0;
    const double m = fabs(E[static_cast<size_t>(i) * D + j]);
    if (m > best) {             // rows ascend within a thread: a tie keeps the lower row
      best = m;
      best_i = i;
    }
  }
  const int rank = static_cast<int>(block_sum<256>(cnt, sh));
  bv[tid] = best;
  bi[tid] = best_i;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o && (bv[tid + o] > bv[tid] || (bv[tid + o] == bv[tid] && bi[tid + o] < bi[tid]))) {
      bv[tid] = bv[tid + o];
      bi[tid] = bi[tid + o];
    }
    __syncthreads();
  }
  const double sign = (bi[0] < D && E[static_cast<size_t>(bi[0]) * D + j] < 0.0) ? -1.0 : 1.0;
  if (tid == 0) evals[rank] = lj;
  for (int i = tid; i < D; i += 256) evecs[static_cast<size_t>(i) * D + rank] = sign * E[static_cast<size_t>(i) * D + j];
}

// ---- rows times a small matrix -----------------------------------------------------------------------------------------------
// out[n][k] = scale * sum_d (x[n][d] - mu[d]) W[d][k], d in index order (one fma each); mu and scale optional.  One block: 32 rows
// x 64 columns; thread (rg, kk) holds rows rg + 4 a.
template <typename TX>
__global__ __launch_bounds__(256) void rows_times_kernel(const TX* __restrict__ X, const double* __restrict__ mu, const double* __restrict__ scale,
                                                         const double* __restrict__ W, double* __restrict__ out, long long N, int D, int K) {
  __shared__ double xs[32][33];
  __shared__ double ws[32][64];
  const int tid = threadIdx.x, kk = tid & 63, rg = tid >> 6;
  const long long n0 = static_cast<long long>(blockIdx.x) * 32;
  const int k0 = blockIdx.y * 64;
  double acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) acc[a] = 0.0;
  for (int d0 = 0; d0 < D; d0 += 32) {
    for (int t = tid; t < 32 * 32; t += 256) {
      const int r = t >> 5, c = t & 31;
      const long long n = n0 + r;
      const int d = d0 + c;
      xs[r][c] = (n < N && d < D) ? static_cast<double>(X[n * D + d]) - (mu ? mu[d] : 0.0) : 0.0;
    }
    for (int t = tid; t < 32 * 64; t += 256) {
      const int r = t >> 6, c = t & 63;
      ws[r][c] = (d0 + r < D && k0 + c < K) ? W[static_cast<size_t>(d0 + r) * K + k0 + c] : 0.0;
    }
    __syncthreads();
    const int dn = D - d0 < 32 ? D - d0 : 32;
    for (int dd = 0; dd < dn; ++dd) {
      const double w = ws[dd][kk];
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[a] = fma(xs[rg + 4 * a][dd], w, acc[a]);
    }
    __syncthreads();
  }
  const double sc = scale ? *scale : 1.0;
  if (k0 + kk < K) {
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const long long n = n0 + rg + 4 * a;
      if (n < N) out[n * K + k0 + kk] = scale ? sc * acc[a] : acc[a];
    }
  }
}

// ---- B, |B - Z|^2 and |Z|^2 ---------------------------------------------------------------------------------------------------
// block c: the rows of chunk c; B = +1 where Z >= 0, else -1 (a NaN gives -1); part[c] = (sum (b - z)^2, sum z^2), each thread its
// elements in index order, then the block's tree
__global__ __launch_bounds__(256) void sign_obj_kernel(const double* __restrict__ Z, int8_t* __restrict__ B, double* __restrict__ part,
                                                       long long M2, int K) {
  __shared__ double sh[256];
  const long long lo = static_cast<long long>(blockIdx.x) * kChunk * K;
  const long long end = static_cast<long long>(M2) * K;
  const long long hi = lo + static_cast<long long>(kChunk) * K < end ? lo + static_cast<long long>(kChunk) * K : end;
  double obj = 0.0, zz = 0.0;
  for (long long e = lo + threadIdx.x; e < hi; e += 256) {
    const double z = Z[e];
    const double b = z >= 0.0 ? 1.0 : -1.0;
    B[e] = z >= 0.0 ? 1 : -1;
    obj = fma(b - z, b - z, obj);
    zz = fma(z, z, zz);
  }
  obj = block_sum<256>(obj, sh);
  zz = block_sum<256>(zz, sh);
  if (threadIdx.x == 0) {
    part[2 * static_cast<size_t>(blockIdx.x)] = obj;
    part[2 * static_cast<size_t>(blockIdx.x) + 1] = zz;
  }
}

// one thread: the chunks in order
__global__ void obj_reduce_kernel(const double* __restrict__ part, int chunks, double* __restrict__ obj_out, double* __restrict__ zz_out) {
  if (threadIdx.x || blockIdx.x) return;
  double obj = 0.0, zz = 0.0;
  for (int c = 0; c < chunks; ++c) {
    obj += part[2 * c];
    zz += part[2 * c + 1];
  }
  if (obj_out) *obj_out = obj;
  if (zz_out) *zz_out = zz;
}

// ---- polar factor -------------------------------------------------------------------------------------------------------------
// One workgroup.  One-sided Jacobi (Hestenes) on the columns of G = M in round-robin order: each wave takes up to kPolarPairs pairs
// of columns per step, its lanes the rows (two per lane up to K = 128); the three dot products are a wave butterfly, the same tree
// on every run.  A pair is rotated where |g_p . g_q| > tol |g_p| |g_q| with tol = sqrt(K) eps: a K-term dot product carries
// that much rounding itself, so a tighter test would rotate noise until the sweep cap (LAPACK's dgesvj uses the same tolerance).
// At the end G = U S (orthogonal columns) and J holds the right vectors, so the polar factor is Q = U J^T and R = Q^T:
// R[r][c] = sum_j (G[c][j] / s_j) J[r][j], j in index order; a null column (singular M) is replaced by a unit vector orthogonal
// to the others, so R is orthogonal for every M (and not unique for a singular one).  G and J are kept
// transposed (a column is contiguous) in the workspace; the block's waves share them through L2 between barriers, and a wave
// issues the loads of all its pairs of a step before it reduces the first, so a step costs one round trip, not one per pair.
// The butterfly is head_common.h's wave_sum (xor, 32 down to 1).
constexpr int kPolarT = 1024, kPolarSweeps = 60, kPolarWaves = kPolarT / 64, kPolarPairs = (kMaxK / 2 + kPolarWaves - 1) / kPolarWaves;

__global__ __launch_bounds__(kPolarT) void polar_kernel(const double* __restrict__ M, int K, double* Gt, double* Jt,
                                                        double* __restrict__ sig, double* __restrict__ R, int32_t* __restrict__ sweeps_out,
                                                        double tol) {
  __shared__ int any[2];
  __shared__ double sh[kPolarT];
  __shared__ unsigned char nullcol[kMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kPolarWaves;
  double fro = 0.0;
  for (int e = tid; e < K * K; e += kPolarT) {
    const int c = e / K, r = e % K;
    const double m = M[static_cast<size_t>(r) * K + c];
    Gt[e] = m;
    Jt[e] = r == c ? 1.0 : 0.0;
    fro = fma(m, m, fro);
  }
  if (tid < 2) any[tid] = 0;
  // a column whose norm falls to tol |M|_F is a null direction of M (rounding level): it is left alone, and completed below
  const double floor2 = tol * tol * block_sum<kPolarT>(fro, sh);
  const int n = (K + 1) & ~1, half = n >> 1;
  const int r0 = lane, r1 = lane + 64;
  const bool in0 = r0 < K, in1 = r1 < K;
  int sweeps = 0;
  for (int sweep = 0; sweep < kPolarSweeps && K > 1; ++sweep) {
    for (int step = 0; step < n - 1; ++step) {
      int pp[kPolarPairs], qq[kPolarPairs];
      bool act[kPolarPairs];
      double a0[kPolarPairs], a1[kPolarPairs], b0[kPolarPairs], b1[kPolarPairs];
      double u0[kPolarPairs], u1[kPolarPairs], v0[kPolarPairs], v1[kPolarPairs];
#pragma unroll
      for (int i = 0; i < kPolarPairs; ++i) {
        const int k = wave + i * NW;
        pp[i] = qq[i] = 0;
        act[i] = k < half;
        if (act[i]) {
          rr_pair(n, step, k, pp[i], qq[i]);
          act[i] = qq[i] < K;                     // index K of an odd K is the bye
        }
        const size_t op = static_cast<size_t>(pp[i]) * K, oq = static_cast<size_t>(qq[i]) * K;
        a0[i] = act[i] && in0 ? Gt[op + r0] : 0.0;
        a1[i] = act[i] && in1 ? Gt[op + r1] : 0.0;
        b0[i] = act[i] && in0 ? Gt[oq + r0] : 0.0;
        b1[i] = act[i] && in1 ? Gt[oq + r1] : 0.0;
        u0[i] = act[i] && in0 ? Jt[op + r0] : 0.0;
        u1[i] = act[i] && in1 ? Jt[op + r1] : 0.0;
        v0[i] = act[i] && in0 ? Jt[oq + r0] : 0.0;
        v1[i] = act[i] && in1 ? Jt[oq + r1] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < kPolarPairs; ++i) {
        if (!act[i]) continue;                    // wave-uniform
        const double alpha = wave_sum(fma(a1[i], a1[i], a0[i] * a0[i])), beta = wave_sum(fma(b1[i], b1[i], b0[i] * b0[i]));
        const double gamma = wave_sum(fma(a1[i], b1[i], a0[i] * b0[i]));
        if (gamma != 0.0 && alpha > floor2 && beta > floor2 && fabs(gamma) > tol * sqrt(alpha * beta)) {          // wave-uniform
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
          const size_t op = static_cast<size_t>(pp[i]) * K, oq = static_cast<size_t>(qq[i]) * K;
          if (in0) {
            Gt[op + r0] = rot_lo(c, s, a0[i], b0[i]);
            Gt[oq + r0] = rot_hi(c, s, a0[i], b0[i]);
            Jt[op + r0] = rot_lo(c, s, u0[i], v0[i]);
            Jt[oq + r0] = rot_hi(c, s, u0[i], v0[i]);
          }
          if (in1) {
            Gt[op + r1] = rot_lo(c, s, a1[i], b1[i]);
            Gt[oq + r1] = rot_hi(c, s, a1[i], b1[i]);
            Jt[op + r1] = rot_lo(c, s, u1[i], v1[i]);
            Jt[oq + r1] = rot_hi(c, s, u1[i], v1[i]);
          }
          if (lane == 0) any[sweep & 1] = 1;
        }
      }
      __syncthreads();
    }
    sweeps = sweep + 1;
    const int rotated = any[sweep & 1];
    __syncthreads();
    if (tid == 0) any[(sweep + 1) & 1] = 0;      // the next sweep's flag: nobody reads or sets it before the barrier below
    __syncthreads();
    if (!rotated) break;
  }
  for (int j = wave; j < K; j += NW) {
    const double* g = Gt + static_cast<size_t>(j) * K;
    const double a0 = lane < K ? g[lane] : 0.0, a1 = lane + 64 < K ? g[lane + 64] : 0.0;
    const double nn = wave_sum(fma(a1, a1, a0 * a0));
    if (lane == 0) {
      sig[j] = nn > floor2 ? 1.0 / sqrt(nn) : 0.0;
      nullcol[j] = nn > floor2 ? 0 : 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < K * K; e += kPolarT) Gt[e] *= sig[e / K];      // G^T <- U^T, null directions zero
  __syncthreads();
  // Singular M: every null direction j gets a unit vector orthogonal to the columns that stand (the others and the null ones
  // completed before it), so that R stays orthogonal; which completion is taken does not matter to R M = the symmetric factor.
  // Wave 0: the unit vector e_i with the largest residual against those columns (lowest i on a tie), projected twice, normalised.
  for (int j = 0; j < K; ++j) {
    if (!nullcol[j]) continue;                    // block-uniform: nullcol is not written after the barrier above
    if (wave == 0) {
      double best = -1.0;
      int best_i = K;
      for (int i = lane; i < K; i += 64) {
        double res = 1.0;
        for (int l = 0; l < K; ++l)
          if (!nullcol[l] || l < j) {
            const double u = Gt[static_cast<size_t>(l) * K + i];
            res = fma(-u, u, res);
          }
        if (res > best) {
          best = res;
          best_i = i;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (ob > best || (ob == best && oi < best_i)) {
          best = ob;
          best_i = oi;
        }
      }
      double w0 = r0 == best_i ? 1.0 : 0.0, w1 = r1 == best_i ? 1.0 : 0.0;
      for (int pass = 0; pass < 2; ++pass)
        for (int l = 0; l < K; ++l)
          if (!nullcol[l] || l < j) {
            const double x0 = in0 ? Gt[static_cast<size_t>(l) * K + r0] : 0.0, x1 = in1 ? Gt[static_cast<size_t>(l) * K + r1] : 0.0;
            const double d = wave_sum(fma(w1, x1, w0 * x0));
            w0 = fma(-d, x0, w0);
            w1 = fma(-d, x1, w1);
          }
      const double nn = wave_sum(fma(w1, w1, w0 * w0));
      const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
      if (in0) Gt[static_cast<size_t>(j) * K + r0] = w0 * inv;
      if (in1) Gt[static_cast<size_t>(j) * K + r1] = w1 * inv;
    }
    __syncthreads();
  }
  for (int e = tid; e < K * K; e += kPolarT) {
    const int r = e / K, c = e % K;
    double acc = 0.0;
    for (int j = 0; j < K; ++j) acc = fma(Gt[static_cast<size_t>(j) * K + c], Jt[static_cast<size_t>(j) * K + r], acc);
    R[e] = acc;
  }
  if (tid == 0 && sweeps_out) *sweeps_out = sweeps;
}

// ---- heads --------------------------------------------------------------------------------------------------------------------
// block (k, m): W_m[k][d] = s alpha_m sum_j P_m[d][j] R[j][k] (j in index order) as f32; b_m[k] = -sum_d W_m[k][d] mu_m[d] from the
// f64 products (each thread its d in order, then the block's tree); s = 0.5 / sqrt(zz / (M2 K)), 0 where zz is not positive
__global__ __launch_bounds__(256) void heads_kernel(const double* __restrict__ P_i, const double* __restrict__ P_t, const double* __restrict__ R,
                                                    const double* __restrict__ mu_i, const double* __restrict__ mu_t, const double* __restrict__ alpha2,
                                                    const double* __restrict__ zz, double count, int D, int K, float* __restrict__ W_i,
                                                    float* __restrict__ b_i, float* __restrict__ W_t, float* __restrict__ b_t,
                                                    double* __restrict__ s_out) {
  __shared__ double sh[256];
  __shared__ double rk[kMaxK];
  const int k = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const double* mu = m ? mu_t : mu_i;
  const double* P = m ? P_t : P_i;
  float* W = m ? W_t : W_i;
  float* bias = m ? b_t : b_i;
  for (int j = tid; j < K; j += 256) rk[j] = R[static_cast<size_t>(j) * K + k];
  __syncthreads();
  const double ms = *zz / count;
  const double s = ms > 0.0 ? 0.5 / sqrt(ms) : 0.0;
  const double sa = s * alpha2[m];
  double dot = 0.0;
  for (int d = tid; d < D; d += 256) {
    double acc = 0.0;
    for (int j = 0; j < K; ++j) acc = fma(P[static_cast<size_t>(d) * K + j], rk[j], acc);
    const double w = sa * acc;
    W[static_cast<size_t>(k) * D + d] = static_cast<float>(w);
    dot = fma(w, mu[d], dot);
  }
  dot = block_sum<256>(dot, sh);
  if (tid == 0) {
    bias[k] = static_cast<float>(-dot);
    if (k == 0 && m == 0 && s_out) *s_out = s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct StepWs {
  double* part;       // [chunks][K][K]
  double* objpart;    // [chunks][2]
  size_t total;
};
StepWs carve_step(void* ws, long long M2, int K) {
  Carver c(ws);
  return {c.take<double>(xty_part_bytes(M2, K, K)), c.take<double>(static_cast<size_t>(chunks_of(M2)) * 2 * sizeof(double)), c.total()};
}

struct PolarWs {
  double *Gt, *Jt, *sig;      // [K][K], [K][K], [K]
  size_t total;
};
PolarWs carve_polar(void* ws, int K) {
  Carver c(ws);
  const size_t kk = static_cast<size_t>(K) * K * sizeof(double);
  return {c.take<double>(kk), c.take<double>(kk), c.take<double>(static_cast<size_t>(K) * sizeof(double)), c.total()};
}

struct RotateWs {
  double* Z;          // [M2][K]
  int8_t* B;          // [M2][K]
  double* Mm;         // [K][K]
  char* step;         // carve_step's
  char* polar;        // carve_polar's
  size_t total;
};
RotateWs carve_rotate(void* ws, long long M2, int K) {
  Carver c(ws);
  const size_t rows = static_cast<size_t>(M2) * K;
  return {c.take<double>(rows * sizeof(double)), c.take<int8_t>(rows),   c.take<double>(static_cast<size_t>(K) * K * sizeof(double)),
          c.take<char>(carve_step(nullptr, M2, K).total), c.take<char>(carve_polar(nullptr, K).total), c.total()};
}

struct EighWs {
  double *A0, *A1, *E;      // [D][D] each: the matrix before and after a step, the vectors
  int32_t* cnt;             // [max_sweeps]
  size_t total;
};
EighWs carve_eigh(void* ws, int D, int max_sweeps) {
  Carver c(ws);
  const size_t mat = static_cast<size_t>(D) * D * sizeof(double);
  return {c.take<double>(mat), c.take<double>(mat), c.take<double>(mat), c.take<int32_t>(static_cast<size_t>(max_sweeps) * sizeof(int32_t)), c.total()};
}

// Z = V R, B, M = B^T V, *obj = |B - Z|^2, *zz = |Z|^2 (M, obj, zz optional)
void run_step(const double* V, long long M2, int K, const double* R, double* Z, int8_t* B, double* Mout, double* obj, double* zz,
              void* ws, hipStream_t st) {
  const StepWs w = carve_step(ws, M2, K);
  const int ch = chunks_of(M2);
  hipLaunchKernelGGL((rows_times_kernel<double>), dim3(static_cast<unsigned>((M2 + 31) / 32), (K + 63) / 64), dim3(256), 0, st, V,
                     static_cast<const double*>(nullptr), static_cast<const double*>(nullptr), R, Z, M2, K, K);
  hipLaunchKernelGGL(sign_obj_kernel, dim3(ch), dim3(256), 0, st, static_cast<const double*>(Z), B, w.objpart, M2, K);
  hipLaunchKernelGGL(obj_reduce_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(w.objpart), ch, obj, zz);
  if (Mout) launch_xty(static_cast<const int8_t*>(B), V, M2, K, K, w.part, Mout, 0, st);
}

void run_polar(const double* M, int K, double* R, int32_t* sweeps, void* ws, hipStream_t st) {
  const PolarWs w = carve_polar(ws, K);
  hipLaunchKernelGGL(polar_kernel, dim3(1), dim3(kPolarT), 0, st, M, K, w.Gt, w.Jt, w.sig, R, sweeps, sqrt(static_cast<double>(K)) * DBL_EPSILON);
}

bool dims_ok(long long D, long long K) { return D >= 1 && D <= kMaxD && K >= 1 && K <= kMaxK && K <= D; }

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_itq_moments_workspace_bytes(int64_t N, int32_t D) {
  if (!rows_ok(N) || D < 1 || D > kMaxD) return 0;
  return carve_product(nullptr, N, D, D, true).total;
}

extern "C" int cmh_itq_moments(const float* F, int64_t N, int32_t D, double* sum, double* sq, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "itq_moments: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "itq_moments: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(F && sum && sq && workspace, "itq_moments: null pointer");
  const size_t need = cmh_itq_moments_workspace_bytes(N, D);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_moments: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const ProductWs w = carve_product(workspace, N, D, D, true);
  launch_xty(F, F, N, D, D, w.part, sq, accumulate, st);
  launch_colsum(F, N, D, w.part_sum, sum, accumulate, st);
  CMH_CHECK_LAUNCH("itq_moments");
  return CMH_OK;
}

extern "C" int cmh_itq_covariance(const double* sum_i, const double* sq_i, const double* sum_t, const double* sq_t, int64_t N, int32_t D,
                                  double* mu_i, double* mu_t, double* alpha2, double* C, void* stream) {
  CMH_CHECK_ARG(N >= 1, "itq_covariance: N = %lld, need N >= 1", static_cast<long long>(N));
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "itq_covariance: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(sum_i && sq_i && sum_t && sq_t && mu_i && mu_t && alpha2 && C, "itq_covariance: null pointer");
  hipStream_t st = as_stream(stream);
  const double inv_n = 1.0 / static_cast<double>(N);
  hipLaunchKernelGGL(moments_finish_kernel, dim3(2), dim3(256), 0, st, sum_i, sq_i, sum_t, sq_t, inv_n, D, mu_i, mu_t, alpha2);
  const size_t e2 = static_cast<size_t>(D) * D;
  hipLaunchKernelGGL(covariance_kernel, dim3(static_cast<unsigned>((e2 + 255) / 256)), dim3(256), 0, st, sq_i, sq_t,
                     static_cast<const double*>(mu_i), static_cast<const double*>(mu_t), static_cast<const double*>(alpha2), inv_n, D, C);
  CMH_CHECK_LAUNCH("itq_covariance");
  return CMH_OK;
}

extern "C" size_t cmh_itq_eigh_workspace_bytes(int32_t D, int32_t max_sweeps) {
  if (D < 1 || D > kMaxD || max_sweeps < 1 || max_sweeps > 1024) return 0;
  return carve_eigh(nullptr, D, max_sweeps).total;
}

extern "C" int cmh_itq_eigh(const double* C, int32_t D, int32_t max_sweeps, double* evals, double* evecs, int32_t* info2, void* workspace,
                            size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "itq_eigh: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(max_sweeps >= 1 && max_sweeps <= 1024, "itq_eigh: max_sweeps = %d, need 1 <= max_sweeps <= 1024", max_sweeps);
  CMH_CHECK_ARG(C && evals && evecs && info2 && workspace, "itq_eigh: null pointer");
  const size_t need = cmh_itq_eigh_workspace_bytes(D, max_sweeps);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_eigh: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const EighWs w = carve_eigh(workspace, D, max_sweeps);
  double* A[2] = {w.A0, w.A1};
  double* E = w.E;
  int32_t* cnt = w.cnt;
  const size_t e2 = static_cast<size_t>(D) * D, init = e2 > static_cast<size_t>(max_sweeps) ? e2 : static_cast<size_t>(max_sweeps);
  hipLaunchKernelGGL(jacobi_init_kernel, dim3(static_cast<unsigned>((init + 255) / 256)), dim3(256), 0, st, C, A[0], E, cnt, D, max_sweeps);
  const int n = (D + 1) & ~1, half = n / 2;
  int cur = 0, sweeps = 0, converged = 0;
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    for (int step = 0; step < n - 1; ++step) {
#define CMH_JACOBI_CASE(T_) \
  if (half <= T_) hipLaunchKernelGGL((jacobi_step_kernel<T_>), dim3(half), dim3(T_), 0, st, static_cast<const double*>(A[cur]), A[cur ^ 1], E, cnt + sweep, D, n, step, DBL_EPSILON); else
      CMH_JACOBI_CASE(64)
      CMH_JACOBI_CASE(128)
      CMH_JACOBI_CASE(256)
      CMH_JACOBI_CASE(512) {}
#undef CMH_JACOBI_CASE
      cur ^= 1;
    }
    CMH_CHECK_LAUNCH("itq_eigh");
    int32_t rotated = -1;      // one 4-byte read per sweep: whether this sweep still rotated a pair
    hipError_t e = hipMemcpyAsync(&rotated, cnt + sweep, sizeof(rotated), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CMH_ERR_LAUNCH, "itq_eigh: %s", hipGetErrorString(e));
    sweeps = sweep + 1;
    if (rotated == 0) {
      converged = 1;
      break;
    }
  }
  hipLaunchKernelGGL(jacobi_finish_kernel, dim3(D), dim3(256), 0, st, static_cast<const double*>(A[cur]), static_cast<const double*>(E), D, evals, evecs);
  CMH_CHECK_LAUNCH("itq_eigh");
  info2[0] = sweeps;
  info2[1] = converged;
  return CMH_OK;
}

extern "C" int cmh_itq_project(const float* F, int64_t N, int32_t D, int32_t K, const double* mu, const double* alpha, const double* P,
                               double* V, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "itq_project: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(dims_ok(D, K), "itq_project: D = %d, K = %d, need 1 <= D <= %d and 1 <= K <= min(D, %d)", D, K, kMaxD, kMaxK);
  CMH_CHECK_ARG(F && mu && alpha && P && V, "itq_project: null pointer");
  hipLaunchKernelGGL((rows_times_kernel<float>), dim3(static_cast<unsigned>((N + 31) / 32), (K + 63) / 64), dim3(256), 0, as_stream(stream), F, mu,
                     alpha, P, V, static_cast<long long>(N), D, K);
  CMH_CHECK_LAUNCH("itq_project");
  return CMH_OK;
}

extern "C" size_t cmh_itq_step_workspace_bytes(int64_t M2, int32_t K) {
  if (!rows_ok(M2) || K < 1 || K > kMaxK) return 0;
  return carve_step(nullptr, M2, K).total;
}

extern "C" int cmh_itq_step(const double* V, int64_t M2, int32_t K, const double* R, double* Z, int8_t* B, double* M, double* obj2,
                            void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(M2), "itq_step: rows = %lld, need 1 <= rows <= %lld", static_cast<long long>(M2), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "itq_step: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(V && R && Z && B && M && obj2 && workspace, "itq_step: null pointer");
  const size_t need = cmh_itq_step_workspace_bytes(M2, K);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_step: workspace of %zu bytes, need %zu", workspace_bytes, need);
  run_step(V, M2, K, R, Z, B, M, obj2, obj2 + 1, workspace, as_stream(stream));
  CMH_CHECK_LAUNCH("itq_step");
  return CMH_OK;
}

extern "C" size_t cmh_itq_polar_workspace_bytes(int32_t K) {
  if (K < 1 || K > kMaxK) return 0;
  return carve_polar(nullptr, K).total;
}

extern "C" int cmh_itq_polar(const double* M, int32_t K, double* R, int32_t* sweeps, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "itq_polar: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(M && R && workspace, "itq_polar: null pointer");
  const size_t need = cmh_itq_polar_workspace_bytes(K);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_polar: workspace of %zu bytes, need %zu", workspace_bytes, need);
  run_polar(M, K, R, sweeps, workspace, as_stream(stream));
  CMH_CHECK_LAUNCH("itq_polar");
  return CMH_OK;
}

extern "C" size_t cmh_itq_rotate_workspace_bytes(int64_t M2, int32_t K) {
  if (!rows_ok(M2) || K < 1 || K > kMaxK) return 0;
  return carve_rotate(nullptr, M2, K).total;
}

extern "C" int cmh_itq_rotate(const double* V, int64_t M2, int32_t K, const double* R0, int32_t iters, double* R, double* obj, double* zz,
                              void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(M2), "itq_rotate: rows = %lld, need 1 <= rows <= %lld", static_cast<long long>(M2), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "itq_rotate: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(iters >= 0 && iters <= 100000, "itq_rotate: iters = %d, need 0 <= iters <= 100000", iters);
  CMH_CHECK_ARG(V && R0 && R && obj && zz && workspace, "itq_rotate: null pointer");
  const size_t need = cmh_itq_rotate_workspace_bytes(M2, K);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_rotate: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const RotateWs w = carve_rotate(workspace, M2, K);
  if (R != R0) {
    const hipError_t e = hipMemcpyAsync(R, R0, static_cast<size_t>(K) * K * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(CMH_ERR_LAUNCH, "itq_rotate: %s", hipGetErrorString(e));
  }
  for (int it = 0; it < iters; ++it) {
    run_step(V, M2, K, R, w.Z, w.B, w.Mm, obj + it, nullptr, w.step, st);
    run_polar(w.Mm, K, R, nullptr, w.polar, st);
  }
  run_step(V, M2, K, R, w.Z, w.B, nullptr, obj + iters, zz, w.step, st);
  CMH_CHECK_LAUNCH("itq_rotate");
  return CMH_OK;
}

extern "C" int cmh_itq_heads_pair(const double* P_i, const double* P_t, const double* R, const double* mu_i, const double* mu_t,
                                  const double* alpha2, const double* zz, int64_t M2, int32_t D, int32_t K, float* W_i, float* b_i, float* W_t,
                                  float* b_t, double* s_out, void* stream) {
  CMH_CHECK_ARG(M2 >= 1, "itq_heads: rows = %lld, need rows >= 1", static_cast<long long>(M2));
  CMH_CHECK_ARG(dims_ok(D, K), "itq_heads: D = %d, K = %d, need 1 <= D <= %d and 1 <= K <= min(D, %d)", D, K, kMaxD, kMaxK);
  CMH_CHECK_ARG(P_i && P_t && R && mu_i && mu_t && alpha2 && zz && W_i && b_i && W_t && b_t, "itq_heads: null pointer");
  hipLaunchKernelGGL(heads_kernel, dim3(K, 2), dim3(256), 0, as_stream(stream), P_i, P_t, R, mu_i, mu_t, alpha2, zz,
                     static_cast<double>(M2) * static_cast<double>(K), D, K, W_i, b_i, W_t, b_t, s_out);
  CMH_CHECK_LAUNCH("itq_heads");
  return CMH_OK;
}

extern "C" int cmh_itq_heads(const double* P, const double* R, const double* mu_i, const double* mu_t, const double* alpha2, const double* zz,
                             int64_t M2, int32_t D, int32_t K, float* W_i, float* b_i, float* W_t, float* b_t, double* s_out, void* stream) {
  return cmh_itq_heads_pair(P, P, R, mu_i, mu_t, alpha2, zz, M2, D, K, W_i, b_i, W_t, b_t, s_out, stream);
}

// ---- CCA projections ----------------------------------------------------------------------------------------------------------
extern "C" size_t cmh_itq_cross_moments_workspace_bytes(int64_t N, int32_t D) {
  if (!rows_ok(N) || D < 1 || D > kMaxD) return 0;
  return carve_product(nullptr, N, D, D, false).total;
}

extern "C" int cmh_itq_cross_moments(const float* F_i, const float* F_t, int64_t N, int32_t D, double* cross, int32_t accumulate,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "itq_cross_moments: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "itq_cross_moments: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(F_i && F_t && cross && workspace, "itq_cross_moments: null pointer");
  const size_t need = cmh_itq_cross_moments_workspace_bytes(N, D);
  CMH_CHECK_ARG(workspace_bytes >= need, "itq_cross_moments: workspace of %zu bytes, need %zu", workspace_bytes, need);
  launch_xty(F_i, F_t, N, D, D, carve_product(workspace, N, D, D, false).part, cross, accumulate, as_stream(stream));
  CMH_CHECK_LAUNCH("itq_cross_moments");
  return CMH_OK;
}

extern "C" int cmh_itq_cca_covariance(const double* sum_i, const double* sq_i, const double* sum_t, const double* sq_t, const double* cross,
                                      int64_t N, int32_t D, double* mu_i, double* mu_t, double* alpha2, double* S_ii, double* S_tt,
                                      double* S_it, void* stream) {
  CMH_CHECK_ARG(N >= 1, "itq_cca_covariance: N = %lld, need N >= 1", static_cast<long long>(N));
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "itq_cca_covariance: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(sum_i && sq_i && sum_t && sq_t && cross && mu_i && mu_t && alpha2 && S_ii && S_tt && S_it, "itq_cca_covariance: null pointer");
  hipStream_t st = as_stream(stream);
  const double inv_n = 1.0 / static_cast<double>(N);
  hipLaunchKernelGGL(moments_finish_kernel, dim3(2), dim3(256), 0, st, sum_i, sq_i, sum_t, sq_t, inv_n, D, mu_i, mu_t, alpha2);
  const size_t e2 = static_cast<size_t>(D) * D;
  hipLaunchKernelGGL(cca_covariance_kernel, dim3(static_cast<unsigned>((e2 + 255) / 256)), dim3(256), 0, st, sq_i, sq_t, cross,
                     static_cast<const double*>(mu_i), static_cast<const double*>(mu_t), static_cast<const double*>(alpha2), inv_n, D, S_ii,
                     S_tt, S_it);
  CMH_CHECK_LAUNCH("itq_cca_covariance");
  return CMH_OK;
}

extern "C" int cmh_itq_inv_sqrt(const double* values, int32_t n, double shift, double* out, double* root, void* stream) {
  CMH_CHECK_ARG(n >= 1 && n <= kMaxD, "itq_inv_sqrt: n = %d, need 1 <= n <= %d", n, kMaxD);
  CMH_CHECK_ARG(shift >= 0.0, "itq_inv_sqrt: shift = %g, need shift >= 0", shift);      // a NaN fails the comparison too
  CMH_CHECK_ARG(values && out, "itq_inv_sqrt: null pointer");
  hipLaunchKernelGGL(inv_sqrt_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), values, n, shift, out, root);
  CMH_CHECK_LAUNCH("itq_inv_sqrt");
  return CMH_OK;
}

extern "C" int cmh_itq_matmul(const double* A, const double* B, const double* d, const double* col_scale, int32_t M, int32_t N, int32_t Kc,
                              int32_t trans_a, int32_t trans_b, double* C, void* stream) {
  CMH_CHECK_ARG(M >= 1 && M <= kMaxD && N >= 1 && N <= kMaxD && Kc >= 1 && Kc <= kMaxD,
                "itq_matmul: M = %d, N = %d, Kc = %d, need 1 <= M, N, Kc <= %d", M, N, Kc, kMaxD);
  CMH_CHECK_ARG((trans_a == 0 || trans_a == 1) && (trans_b == 0 || trans_b == 1), "itq_matmul: trans_a = %d, trans_b = %d, need 0 or 1",
                trans_a, trans_b);
  CMH_CHECK_ARG(A && B && C, "itq_matmul: null pointer");
  CMH_CHECK_ARG(C != A && C != B, "itq_matmul: the output must not be an operand");
  hipStream_t st = as_stream(stream);
  const dim3 grid((N + kTile - 1) / kTile, (M + kTile - 1) / kTile);
#define CMH_MATMUL_CASE(TA_, TB_)                                                                                                       \
  if (trans_a == TA_ && trans_b == TB_) {                                                                                                \
    if (d) hipLaunchKernelGGL((matmul_kernel<TA_ != 0, TB_ != 0, true>), grid, dim3(256), 0, st, A, B, d, col_scale, C, M, N, Kc);      \
    else hipLaunchKernelGGL((matmul_kernel<TA_ != 0, TB_ != 0, false>), grid, dim3(256), 0, st, A, B, d, col_scale, C, M, N, Kc);       \
  }
  CMH_MATMUL_CASE(0, 0)
  CMH_MATMUL_CASE(0, 1)
  CMH_MATMUL_CASE(1, 0)
  CMH_MATMUL_CASE(1, 1)
#undef CMH_MATMUL_CASE
  CMH_CHECK_LAUNCH("itq_matmul");
  return CMH_OK;
}
