// Shared by the training-free fits (itq, dch): the fixed-order f64 pieces.  The O(N) products over row chunks with their host launchers,
// the fixed-tree workgroup reduction and the covariance element.  wave_sum and the workspace Carver come from head_common.h.
//
// Determinism: every output element is one sum in a fixed order.  The O(N) products cut the rows into chunks of kChunk (a constant,
// not a property of the device), sum each chunk in row order and then the chunks in chunk order; block reductions are fixed trees and
// per-block partials are added in block order; nothing is accumulated with atomics, and no kernel waits for another workgroup.  This
// is what makes a fit reproducible to the bit, and the file that holds it is the only place a product or a reduction is written.
//
// Everything here has internal linkage (an anonymous namespace): each including object gets its own kernels and exports none.
#pragma once

#include "head_common.h"

namespace cmh {
namespace {

constexpr int kMaxD = 1024, kMaxK = 128;
constexpr int kChunk = 2048;                  // rows per partial sum of the O(N) products
constexpr int kTile = 64, kStage = 16;        // X^T Y: output tile and rows per LDS stage
constexpr long long kMaxRows = 65535ll * kChunk;      // the chunk index is a grid dimension (y or z: at most 65535)

inline int chunks_of(long long n) { return static_cast<int>((n + kChunk - 1) / kChunk); }
inline bool rows_ok(long long n) { return n >= 1 && n <= kMaxRows; }

// ---- X^T Y over row chunks ----------------------------------------------------------------------------------------------------
// part[c][i][j] = sum over the rows n of chunk c, in row order, of X[n][i] * Y[n][j] (one fma per row).  One block: a 64 x 64 tile
// of (i, j) for one chunk; thread (ti, tj) holds i = 4 ti + a, j = tj + 16 b.
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void xty_partial_kernel(const TX* __restrict__ X, const TY* __restrict__ Y, double* __restrict__ part,
                                                          long long N, int Da, int Db) {
  __shared__ double xs[kStage][kTile];
  __shared__ double ys[kStage][kTile];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int j0 = blockIdx.x * kTile, i0 = blockIdx.y * kTile;
  const long long n_lo = static_cast<long long>(blockIdx.z) * kChunk;
  const long long n_hi = n_lo + kChunk < N ? n_lo + kChunk : N;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (long long n0 = n_lo; n0 < n_hi; n0 += kStage) {
    for (int t = tid; t < kStage * kTile; t += 256) {
      const int r = t >> 6, c = t & 63;
      const long long n = n0 + r;
      const bool row = n < n_hi;
      xs[r][c] = (row && i0 + c < Da) ? static_cast<double>(X[n * Da + i0 + c]) : 0.0;
      ys[r][c] = (row && j0 + c < Db) ? static_cast<double>(Y[n * Db + j0 + c]) : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kStage; ++r) {
      double xv[4], yv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xv[a] = xs[r][ti * 4 + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) yv[b] = ys[r][tj + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(xv[a], yv[b], acc[a][b]);
    }
    __syncthreads();
  }
  double* out = part + static_cast<size_t>(blockIdx.z) * Da * Db;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ti * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tj + 16 * b;
      if (i < Da && j < Db) out[static_cast<size_t>(i) * Db + j] = acc[a][b];
    }
  }
}

// part[c][d] = sum over the rows of chunk c, in row order, of X[n][d]
template <typename T>
__global__ __launch_bounds__(64) void colsum_partial_kernel(const T* __restrict__ X, double* __restrict__ part, long long N, int D) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  const long long n_lo = static_cast<long long>(blockIdx.y) * kChunk;
  const long long n_hi = n_lo + kChunk < N ? n_lo + kChunk : N;
  double acc = 0.0;
  for (long long n = n_lo; n < n_hi; ++n) acc += static_cast<double>(X[n * D + d]);
  part[static_cast<size_t>(blockIdx.y) * D + d] = acc;
}

// out[e] = (accumulate ? out[e] : 0) + (part[0][e] + part[1][e] + ...), the chunks in order
__global__ __launch_bounds__(256) void chunk_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int chunks, size_t elems,
                                                           int accumulate) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= elems) return;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc += part[static_cast<size_t>(c) * elems + e];
  out[e] = accumulate ? out[e] + acc : acc;
}

// ---- the host side of a chunked product -----------------------------------------------------------------------------------------
// Bytes of the partials, not rounded: an entry that keeps a column sum puts its partials right behind the product's.
inline size_t xty_part_bytes(long long n, int Da, int Db) { return static_cast<size_t>(chunks_of(n)) * Da * Db * sizeof(double); }
inline size_t colsum_part_bytes(long long n, int D) { return static_cast<size_t>(chunks_of(n)) * D * sizeof(double); }

inline void launch_chunk_reduce(const double* part, long long n, size_t elems, double* out, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(chunk_reduce_kernel, dim3(static_cast<unsigned>((elems + 255) / 256)), dim3(256), 0, st, part, out, chunks_of(n), elems,
                     accumulate ? 1 : 0);
}
// out [Da, Db] (+)= X^T Y over the n rows of X [n, Da] and Y [n, Db]: the chunks' products into part, then the chunks in order
template <typename TX, typename TY>
void launch_xty(const TX* X, const TY* Y, long long n, int Da, int Db, double* part, double* out, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL((xty_partial_kernel<TX, TY>), dim3((Db + kTile - 1) / kTile, (Da + kTile - 1) / kTile, chunks_of(n)), dim3(256), 0, st, X,
                     Y, part, n, Da, Db);
  launch_chunk_reduce(part, n, static_cast<size_t>(Da) * Db, out, accumulate, st);
}
// out [D] (+)= 1^T X over the n rows of X [n, D]
template <typename T>
void launch_colsum(const T* X, long long n, int D, double* part, double* out, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL((colsum_partial_kernel<T>), dim3((D + 63) / 64, chunks_of(n)), dim3(64), 0, st, X, part, n, D);
  launch_chunk_reduce(part, n, static_cast<size_t>(D), out, accumulate, st);
}

// The workspace of an entry that is one product [Da, Db], with or without the column sum of its right operand: the product's
// partials, the column sum's right behind them (not aligned), the total rounded up to 256.
struct ProductWs {
  double *part, *part_sum;
  size_t total;
};
inline ProductWs carve_product(void* ws, long long n, int Da, int Db, bool with_colsum) {
  Carver c(ws);
  return {c.take<double>(xty_part_bytes(n, Da, Db), 8), c.take<double>(with_colsum ? colsum_part_bytes(n, Db) : 0, 8), align_up(c.total(), 256)};
}

// ---- block reduction: one fixed tree, the operation a parameter ------------------------------------------------------------------
// sh: T elements of LDS.  Thread t folds sh[t + o] into sh[t] for o = T / 2, T / 4, ..., 1; every thread ends with the result.
template <int T, typename Op>
__device__ __forceinline__ double block_reduce(double v, double* sh, Op fold) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) fold(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
template <int T>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  return block_reduce<T>(v, sh, [](double& a, double b) { a += b; });
}
template <int T>
__device__ __forceinline__ double block_min(double v, double* sh) {
  return block_reduce<T>(v, sh, [](double& a, double b) { a = fmin(a, b); });
}

// ---- covariance ---------------------------------------------------------------------------------------------------------------
// One element of a normalised covariance: scale (sq / N - mu_a mu_b).  The library is built with -ffp-contract=on, and the contraction
// is picked inside this one expression: keep its shape.
__device__ __forceinline__ double cov_element(double scale, double sq, double inv_n, double mu_a, double mu_b) {
  return scale * (sq * inv_n - mu_a * mu_b);
}

}  // namespace
}  // namespace cmh
