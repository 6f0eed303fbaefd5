// Supervised training-free hash heads (no upstream counterpart): discrete cross-modal hashing on frozen features (DCH, Xu et al.,
// TIP 2017, the cross-modal form of SDH, Shen et al., CVPR 2015).  B in {+-1}^{N x K} is fitted so that it predicts the labels
// linearly (W) and is predicted linearly from each modality's features (P_m); its bits are set by discrete cyclic coordinate
// descent, with no relaxation.  utils/dch.py runs the fit; moments, eigen-solver, small products, projection and heads are itq.hip's.
//
//   covariance   S_mm = alpha_m^2 (sum f f^T / N - mu_m mu_m^T) of one modality (trace 1), without a cross moment
//   start        B = +1 where z_a + z_b >= 0, else -1 (the PCAH code of the summed modalities)
//   xtb          X^T B over row chunks (X = F_m or Y) and 1^T B
//   btb          B^T B (exact integers)
//   center       U_m = alpha_m (F_m^T B - mu_m (1^T B)^T) / N = X_m^T B / N, the right-hand side of P_m = A_m U_m
//   solve        W = (A + shift I)^-1 R by a Cholesky factorisation in one workgroup, the factor in LDS
//   targets      Qt [K, N] = (Y W^T + mu Z_i + mu Z_t)^T and the objective of (B, W, Z)
//   dcc          `rounds` Gauss-Seidel rounds over the bits of every item; flips per round and the smallest |t|
//
// Determinism: fit_common.h states it, with the chunked products (X^T B and B^T B are its X^T Y kernel with int8 operands), the column
// sum, the block reductions and the covariance element, all shared with itq.hip.
#include "fit_common.h"

#include <cfloat>
#include <cmath>

namespace cmh {
namespace {

constexpr int kMaxC = 1024, kMaxRounds = 64;

// ---- small element-wise pieces -------------------------------------------------------------------------------------------------
// S[i][j] = alpha^2 (sq[i][j] / N - mu[i] mu[j]): cmh_itq_cca_covariance's S_mm, symmetric bit for bit where sq is
__global__ __launch_bounds__(256) void covariance_kernel(const double* __restrict__ sq, const double* __restrict__ mu,
                                                         const double* __restrict__ alpha, double inv_n, int D, double* __restrict__ S) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<size_t>(D) * D) return;
  const int i = static_cast<int>(e / D), j = static_cast<int>(e % D);
  const double a = alpha[0];
  S[e] = cov_element(a * a, sq[e], inv_n, mu[i], mu[j]);
}

// B = +1 where za + zb >= 0, else -1 (a NaN gives -1)
__global__ __launch_bounds__(256) void start_kernel(const double* __restrict__ Za, const double* __restrict__ Zb, size_t elems,
                                                    int8_t* __restrict__ B) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= elems) return;
  B[e] = Za[e] + Zb[e] >= 0.0 ? 1 : -1;
}

// U[d][k] = (alpha (T[d][k] - mu[d] bsum[k])) / N, the difference one fma
__global__ __launch_bounds__(256) void center_kernel(const double* __restrict__ T, const double* __restrict__ bsum, const double* __restrict__ mu,
                                                     const double* __restrict__ alpha, double inv_n, int D, int K, double* __restrict__ U) {
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<size_t>(D) * K) return;
  const int d = static_cast<int>(e / K), k = static_cast<int>(e % K);
  U[e] = (alpha[0] * fma(-mu[d], bsum[k], T[e])) * inv_n;
}

// ---- W = (A + shift I)^-1 R ----------------------------------------------------------------------------------------------------
// One workgroup.  The factor L (A + shift I = L L^T, lower, left-looking) lives in LDS with a row pitch of K + 1 doubles: 132 096
// bytes at K = 128, inside gfx950's 160 KB.  Column j: thread i (j <= i < K) runs acc = a_ij, acc = fma(-L[i][k], L[j][k], acc) for
// k ascending below j; L[j][j] = sqrt(acc), L[i][j] = acc / L[j][j].  A pivot that is not positive (a NaN included) ends the
// factorisation: *info = j + 1 and W is filled with zeros.  The solves run one column of R per thread, in W itself: forward
// y_i = (r_i - sum_{k < i} L[i][k] y_k) / L[i][i], then backward w_i = (y_i - sum_{k > i} L[k][i] w_k) / L[i][i], k ascending in both;
// every thread reads the same L entry at the same time (a broadcast).
constexpr int kSolveT = 1024;

__global__ __launch_bounds__(kSolveT) void solve_kernel(const double* __restrict__ A, double shift, const double* __restrict__ R, int K, int C,
                                                        double* __restrict__ W, int32_t* __restrict__ info) {
  extern __shared__ double solve_lds[];      // L [K][K + 1]
  __shared__ int bad;
  double* L = solve_lds;
  const int tid = threadIdx.x, P = K + 1;
  for (int e = tid; e < K * K; e += kSolveT) {
    const int i = e / K, j = e % K;
    L[i * P + j] = A[e] + (i == j ? shift : 0.0);
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  int failed = 0;
  for (int j = 0; j < K; ++j) {
    const int i = j + tid;
    double acc = 0.0;
    if (i < K) {
      acc = L[i * P + j];
      for (int k = 0; k < j; ++k) acc = fma(-L[i * P + k], L[j * P + k], acc);
      if (i == j) {
        if (acc > 0.0) L[j * P + j] = sqrt(acc);
        else bad = j + 1;
      }
    }
    __syncthreads();
    failed = bad;
    if (failed) break;                         // block-uniform: every thread reads the word the barrier published
    if (i > j && i < K) L[i * P + j] = acc / L[j * P + j];
    __syncthreads();
  }
  if (tid == 0) *info = failed;
  if (failed) {
    for (int e = tid; e < K * C; e += kSolveT) W[e] = 0.0;
    return;
  }
  for (int c = tid; c < C; c += kSolveT) {
    for (int i = 0; i < K; ++i) {
      double acc = R[static_cast<size_t>(i) * C + c];
      for (int k = 0; k < i; ++k) acc = fma(-L[i * P + k], W[static_cast<size_t>(k) * C + c], acc);
      W[static_cast<size_t>(i) * C + c] = acc / L[i * P + i];
    }
    for (int i = K - 1; i >= 0; --i) {
      double acc = W[static_cast<size_t>(i) * C + c];
      for (int k = i + 1; k < K; ++k) acc = fma(-L[k * P + i], W[static_cast<size_t>(k) * C + c], acc);
      W[static_cast<size_t>(i) * C + c] = acc / L[i * P + i];
    }
  }
}

// ---- targets and objective -----------------------------------------------------------------------------------------------------
// One block: 64 items (the lanes) x all bits; wave w takes the bits l = w, w + 4, ....  q[n][l] = sum_c Y[n][c] W[l][c] (c
// ascending, one fma each), then q = fma(mu, z_i, q), q = fma(mu, z_t, q); Qt[l][n] = q, so a wave writes 64 consecutive doubles
// per bit.  The same pass sums the feature terms of its items: part[block] = (sum (b - z_i)^2 + (b - z_t)^2, sum z_i^2 + z_t^2),
// each thread its bits in ascending order, then the block's tree.  WriteQ = false runs the sums alone.
constexpr int kQC = 32;                       // labels per LDS stage

template <bool WriteQ>
__global__ __launch_bounds__(256) void targets_kernel(const float* __restrict__ Y, const int8_t* __restrict__ B, const double* __restrict__ W,
                                                      const double* __restrict__ Zi, const double* __restrict__ Zt, double mu, long long N, int K,
                                                      int C, double* __restrict__ Qt, double* __restrict__ part) {
  __shared__ double ys[kQC][65];              // ys[c][item]
  __shared__ double wl[kQC][kMaxK + 1];       // wl[c][l]
  __shared__ double sh[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n0 = static_cast<long long>(blockIdx.x) * 64, n = n0 + lane;
  const bool in = n < N;
  const int nb = K > wave ? (K - wave + 3) >> 2 : 0;      // this wave's bits
  double acc[kMaxK / 4];
#pragma unroll
  for (int j = 0; j < kMaxK / 4; ++j) acc[j] = 0.0;
  if (WriteQ) {
    for (int c0 = 0; c0 < C; c0 += kQC) {
      for (int t = tid; t < 64 * kQC; t += 256) {
        const int r = t >> 5, cc = t & 31;
        ys[cc][r] = (n0 + r < N && c0 + cc < C) ? static_cast<double>(Y[(n0 + r) * C + c0 + cc]) : 0.0;
      }
      for (int t = tid; t < K * kQC; t += 256) {
        const int l = t >> 5, cc = t & 31;
        wl[cc][l] = c0 + cc < C ? W[static_cast<size_t>(l) * C + c0 + cc] : 0.0;
      }
      __syncthreads();
      const int cn = C - c0 < kQC ? C - c0 : kQC;
      for (int cc = 0; cc < cn; ++cc) {
        const double y = ys[cc][lane];
#pragma unroll
        for (int j = 0; j < kMaxK / 4; ++j)
          if (j < nb) acc[j] = fma(y, wl[cc][wave + 4 * j], acc[j]);      // wave-uniform
      }
      __syncthreads();
    }
  }
  double feat = 0.0, zz = 0.0;
#pragma unroll
  for (int j = 0; j < kMaxK / 4; ++j) {
    if (j < nb && in) {
      const int l = wave + 4 * j;
      const size_t e = static_cast<size_t>(n) * K + l;
      const double zi = Zi[e], zt = Zt[e], b = static_cast<double>(B[e]);
      if (WriteQ) Qt[static_cast<size_t>(l) * N + n] = fma(mu, zt, fma(mu, zi, acc[j]));
      feat = fma(b - zi, b - zi, feat);
      feat = fma(b - zt, b - zt, feat);
      zz = fma(zi, zi, zz);
      zz = fma(zt, zt, zz);
    }
  }
  feat = block_sum<256>(feat, sh);
  zz = block_sum<256>(zz, sh);
  if (tid == 0) {
    part[2 * static_cast<size_t>(blockIdx.x)] = feat;
    part[2 * static_cast<size_t>(blockIdx.x) + 1] = zz;
  }
}

// An item's K bits in four words: bit k of word k / 32 is set where b_k = +1.
struct Bits {
  uint32_t w[4];
};
__device__ __forceinline__ Bits load_bits(const int8_t* __restrict__ row, int K) {
  Bits b;
#pragma unroll
  for (int wi = 0; wi < 4; ++wi) {
    uint32_t v = 0;
    const int kn = K - wi * 32 < 32 ? K - wi * 32 : 32;
    for (int j = 0; j < kn; ++j) v |= (row[wi * 32 + j] > 0 ? 1u : 0u) << j;
    b.w[wi] = v;
  }
  return b;
}

// One block: 256 items, one per thread.  part[block] = sum over its items and c of (Y[n][c] - sum_k b_k W[k][c])^2: the residual is
// one chain r = y, r = fma(-b_k, W[k][c], r) for k ascending; an item adds its c in ascending order, then the block's tree.
__global__ __launch_bounds__(256) void residual_kernel(const float* __restrict__ Y, const int8_t* __restrict__ B, const double* __restrict__ W,
                                                       long long N, int K, int C, double* __restrict__ part) {
  __shared__ double wk[kMaxK][kQC + 1];       // wk[k][c]
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const long long n = static_cast<long long>(blockIdx.x) * 256 + tid;
  const bool in = n < N;
  Bits bits = {{0u, 0u, 0u, 0u}};
  if (in) bits = load_bits(B + static_cast<size_t>(n) * K, K);
  double total = 0.0;
  for (int c0 = 0; c0 < C; c0 += kQC) {
    for (int t = tid; t < K * kQC; t += 256) {
      const int k = t >> 5, cc = t & 31;
      wk[k][cc] = c0 + cc < C ? W[static_cast<size_t>(k) * C + c0 + cc] : 0.0;
    }
    __syncthreads();
    const int cn = C - c0 < kQC ? C - c0 : kQC;
    if (in) {
      for (int cc = 0; cc < cn; ++cc) {
        double r = static_cast<double>(Y[static_cast<size_t>(n) * C + c0 + cc]);
#pragma unroll
        for (int wi = 0; wi < 4; ++wi) {
          const int kn = K - wi * 32 < 32 ? K - wi * 32 : 32;
          const uint32_t v = bits.w[wi];
          for (int j = 0; j < kn; ++j) {
            const double g = wk[wi * 32 + j][cc];
            r = (v >> j) & 1u ? r - g : r + g;      // fma(-b_k, g, r): b_k g is exact
          }
        }
        total = fma(r, r, total);
      }
    }
    __syncthreads();
  }
  total = block_sum<256>(total, sh);
  if (tid == 0) part[blockIdx.x] = total;
}

// One block: obj2[0] = (sum of the residual partials + lam |W|^2) + mu (sum of the feature partials), obj2[1] = sum of the |Z|^2
// partials, every list in block order by one thread; |W|^2: each thread its elements in index order, then the block's tree
__global__ __launch_bounds__(256) void objective_finish_kernel(const double* __restrict__ rpart, int rblocks, const double* __restrict__ fpart,
                                                               int fblocks, const double* __restrict__ W, int elems, double lam, double mu,
                                                               double* __restrict__ obj2) {
  __shared__ double sh[256];
  double ww = 0.0;
  for (int e = threadIdx.x; e < elems; e += 256) ww = fma(W[e], W[e], ww);
  ww = block_sum<256>(ww, sh);
  if (threadIdx.x) return;
  double resid = 0.0, feat = 0.0, zz = 0.0;
  for (int b = 0; b < rblocks; ++b) resid += rpart[b];
  for (int b = 0; b < fblocks; ++b) {
    feat += fpart[2 * static_cast<size_t>(b)];
    zz += fpart[2 * static_cast<size_t>(b) + 1];
  }
  obj2[0] = (resid + lam * ww) + mu * feat;
  obj2[1] = zz;
}

// ---- the coordinate descent ----------------------------------------------------------------------------------------------------
// Lanes own items; an item's bits live in NW 32-bit words of registers; G [K][K] sits in LDS and every lane reads the same entry at
// the same time (a broadcast).  Round r, bit l: acc = Qt[l][n] (64 consecutive doubles per wave), then for k ascending, k != l,
// acc = fma(-b_k, G[k][l], acc) - b_k G is exact, so the fma is acc - G or acc + G; b_l = +1 where acc > 0, -1 where acc < 0,
// unchanged where acc == 0.  Per block: the flipped bits of each round (integers, any order) and the smallest |acc|.
template <int NW>
__global__ __launch_bounds__(256) void dcc_kernel(const double* __restrict__ Qt, const double* __restrict__ G, int8_t* __restrict__ B, long long N,
                                                  int K, int rounds, long long* __restrict__ fpart, double* __restrict__ mpart) {
  extern __shared__ double dcc_g[];           // G [K][K]
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const long long n = static_cast<long long>(blockIdx.x) * 256 + tid;
  const bool in = n < N;
  for (int e = tid; e < K * K; e += 256) dcc_g[e] = G[e];
  uint32_t w[NW];
#pragma unroll
  for (int wi = 0; wi < NW; ++wi) w[wi] = 0u;
  if (in) {
    const Bits b = load_bits(B + static_cast<size_t>(n) * K, K);
#pragma unroll
    for (int wi = 0; wi < NW; ++wi) w[wi] = b.w[wi];
  }
  __syncthreads();
  double least = INFINITY;
  for (int r = 0; r < rounds; ++r) {
    int flipped = 0;
    for (int l = 0; l < K; ++l) {
      double acc = in ? Qt[static_cast<size_t>(l) * N + n] : 1.0;
#pragma unroll
      for (int wi = 0; wi < NW; ++wi) {
        const int kn = K - wi * 32 < 32 ? K - wi * 32 : 32;
        const uint32_t v = w[wi];
        for (int j = 0; j < kn; ++j) {
          const int k = wi * 32 + j;
          if (k == l) continue;                 // uniform
          const double g = dcc_g[k * K + l];
          acc = (v >> j) & 1u ? acc - g : acc + g;
        }
      }
      if (in) least = fmin(least, fabs(acc));
      const uint32_t mask = 1u << (l & 31);
#pragma unroll
      for (int wi = 0; wi < NW; ++wi) {
        if (wi == (l >> 5)) {                   // uniform
          const uint32_t old = w[wi] & mask;
          const uint32_t now = acc > 0.0 ? mask : (acc < 0.0 ? 0u : old);
          flipped += (in && now != old) ? 1 : 0;
          w[wi] = (w[wi] & ~mask) | now;
        }
      }
    }
    const double total = block_sum<256>(static_cast<double>(flipped), sh);      // at most 256 x 128: exact
    if (tid == 0) fpart[static_cast<size_t>(blockIdx.x) * rounds + r] = static_cast<long long>(total);
  }
  least = block_min<256>(least, sh);
  if (tid == 0) mpart[blockIdx.x] = least;
  if (in) {
    int8_t* row = B + static_cast<size_t>(n) * K;
#pragma unroll
    for (int wi = 0; wi < NW; ++wi) {
      const int kn = K - wi * 32 < 32 ? K - wi * 32 : 32;
      for (int j = 0; j < kn; ++j) row[wi * 32 + j] = (w[wi] >> j) & 1u ? 1 : -1;
    }
  }
}

// thread r < rounds: flips[r] = sum of the blocks' counts; thread 0 also the smallest of the blocks' |t|
__global__ __launch_bounds__(64) void dcc_finish_kernel(const long long* __restrict__ fpart, const double* __restrict__ mpart, int blocks, int rounds,
                                                        long long* __restrict__ flips, double* __restrict__ min_margin) {
  const int r = threadIdx.x;
  if (r < rounds) {
    long long total = 0;
    for (int b = 0; b < blocks; ++b) total += fpart[static_cast<size_t>(b) * rounds + r];
    flips[r] = total;
  }
  if (r == 0) {
    double least = INFINITY;
    for (int b = 0; b < blocks; ++b) least = fmin(least, mpart[b]);
    *min_margin = least;
  }
}

// ---- workspaces ----------------------------------------------------------------------------------------------------------------
struct TargetsWs {
  double* fpart;      // [ceil(N / 64)][2]
  double* rpart;      // [ceil(N / 256)]
  size_t total;
};
TargetsWs carve_targets(void* ws, long long N) {
  Carver c(ws);
  const size_t fb = static_cast<size_t>((N + 63) / 64), rb = static_cast<size_t>((N + 255) / 256);
  return {c.take<double>(fb * 2 * sizeof(double)), c.take<double>(rb * sizeof(double)), c.total()};
}

struct DccWs {
  long long* fpart;   // [ceil(N / 256)][rounds]
  double* mpart;      // [ceil(N / 256)]
  size_t total;
};
DccWs carve_dcc(void* ws, long long N, int rounds) {
  Carver c(ws);
  const size_t blocks = static_cast<size_t>((N + 255) / 256);
  return {c.take<long long>(blocks * rounds * sizeof(long long)), c.take<double>(blocks * sizeof(double)), c.total()};
}

bool reserve_lds(const void* kernel, size_t lds) {
  return lds <= 48 * 1024 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) == hipSuccess;
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" int cmh_dch_covariance(const double* sq, const double* mu, const double* alpha, int64_t N, int32_t D, double* S, void* stream) {
  CMH_CHECK_ARG(N >= 1, "dch_covariance: N = %lld, need N >= 1", static_cast<long long>(N));
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD, "dch_covariance: D = %d, need 1 <= D <= %d", D, kMaxD);
  CMH_CHECK_ARG(sq && mu && alpha && S, "dch_covariance: null pointer");
  const size_t e2 = static_cast<size_t>(D) * D;
  hipLaunchKernelGGL(covariance_kernel, dim3(static_cast<unsigned>((e2 + 255) / 256)), dim3(256), 0, as_stream(stream), sq, mu, alpha,
                     1.0 / static_cast<double>(N), D, S);
  CMH_CHECK_LAUNCH("dch_covariance");
  return CMH_OK;
}

extern "C" int cmh_dch_start(const double* Za, const double* Zb, int64_t N, int32_t K, int8_t* B, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "dch_start: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "dch_start: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(Za && Zb && B, "dch_start: null pointer");
  const size_t elems = static_cast<size_t>(N) * K;
  hipLaunchKernelGGL(start_kernel, dim3(static_cast<unsigned>((elems + 255) / 256)), dim3(256), 0, as_stream(stream), Za, Zb, elems, B);
  CMH_CHECK_LAUNCH("dch_start");
  return CMH_OK;
}

extern "C" size_t cmh_dch_xtb_workspace_bytes(int64_t N, int32_t Dx, int32_t K) {
  if (!rows_ok(N) || Dx < 1 || Dx > kMaxD || K < 1 || K > kMaxK) return 0;
  return carve_product(nullptr, N, Dx, K, true).total;
}

extern "C" int cmh_dch_xtb(const float* X, const int8_t* B, int64_t N, int32_t Dx, int32_t K, double* out, double* bsum, int32_t accumulate,
                           void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "dch_xtb: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(Dx >= 1 && Dx <= kMaxD && K >= 1 && K <= kMaxK, "dch_xtb: Dx = %d, K = %d, need 1 <= Dx <= %d and 1 <= K <= %d", Dx, K, kMaxD,
                kMaxK);
  CMH_CHECK_ARG(X && B && out && workspace, "dch_xtb: null pointer");
  const size_t need = cmh_dch_xtb_workspace_bytes(N, Dx, K);
  CMH_CHECK_ARG(workspace_bytes >= need, "dch_xtb: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const ProductWs w = carve_product(workspace, N, Dx, K, true);
  launch_xty(X, B, N, Dx, K, w.part, out, accumulate, st);
  if (bsum) launch_colsum(B, N, K, w.part_sum, bsum, accumulate, st);
  CMH_CHECK_LAUNCH("dch_xtb");
  return CMH_OK;
}

extern "C" size_t cmh_dch_btb_workspace_bytes(int64_t N, int32_t K) {
  if (!rows_ok(N) || K < 1 || K > kMaxK) return 0;
  return carve_product(nullptr, N, K, K, false).total;
}

extern "C" int cmh_dch_btb(const int8_t* B, int64_t N, int32_t K, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "dch_btb: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "dch_btb: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(B && out && workspace, "dch_btb: null pointer");
  const size_t need = cmh_dch_btb_workspace_bytes(N, K);
  CMH_CHECK_ARG(workspace_bytes >= need, "dch_btb: workspace of %zu bytes, need %zu", workspace_bytes, need);
  launch_xty(B, B, N, K, K, carve_product(workspace, N, K, K, false).part, out, 0, as_stream(stream));
  CMH_CHECK_LAUNCH("dch_btb");
  return CMH_OK;
}

extern "C" int cmh_dch_center(const double* T, const double* bsum, const double* mu, const double* alpha, int64_t N, int32_t D, int32_t K,
                              double* U, void* stream) {
  CMH_CHECK_ARG(N >= 1, "dch_center: N = %lld, need N >= 1", static_cast<long long>(N));
  CMH_CHECK_ARG(D >= 1 && D <= kMaxD && K >= 1 && K <= kMaxK && K <= D, "dch_center: D = %d, K = %d, need 1 <= D <= %d and 1 <= K <= min(D, %d)", D,
                K, kMaxD, kMaxK);
  CMH_CHECK_ARG(T && bsum && mu && alpha && U, "dch_center: null pointer");
  const size_t elems = static_cast<size_t>(D) * K;
  hipLaunchKernelGGL(center_kernel, dim3(static_cast<unsigned>((elems + 255) / 256)), dim3(256), 0, as_stream(stream), T, bsum, mu, alpha,
                     1.0 / static_cast<double>(N), D, K, U);
  CMH_CHECK_LAUNCH("dch_center");
  return CMH_OK;
}

extern "C" int cmh_dch_solve(const double* A, double shift, const double* R, int32_t K, int32_t C, double* W, int32_t* info, void* stream) {
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK && C >= 1 && C <= kMaxC, "dch_solve: K = %d, C = %d, need 1 <= K <= %d and 1 <= C <= %d", K, C, kMaxK, kMaxC);
  CMH_CHECK_ARG(shift >= 0.0, "dch_solve: shift = %g, need shift >= 0", shift);      // a NaN fails the comparison too
  CMH_CHECK_ARG(A && R && W && info, "dch_solve: null pointer");
  CMH_CHECK_ARG(W != R && W != A, "dch_solve: the output must not be an operand");
  const size_t lds = static_cast<size_t>(K) * (K + 1) * sizeof(double);
  if (!reserve_lds(reinterpret_cast<const void*>(solve_kernel), lds)) return fail(CMH_ERR_LAUNCH, "dch_solve: cannot reserve %zu bytes of LDS", lds);
  hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(kSolveT), lds, as_stream(stream), A, shift, R, K, C, W, info);
  CMH_CHECK_LAUNCH("dch_solve");
  return CMH_OK;
}

extern "C" size_t cmh_dch_targets_workspace_bytes(int64_t N) {
  if (!rows_ok(N)) return 0;
  return carve_targets(nullptr, N).total;
}

extern "C" int cmh_dch_targets(const float* Y, const int8_t* B, const double* W, const double* Z_i, const double* Z_t, double mu, double lam,
                               int64_t N, int32_t K, int32_t C, double* Qt, double* obj2, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "dch_targets: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK && C >= 1 && C <= kMaxC, "dch_targets: K = %d, C = %d, need 1 <= K <= %d and 1 <= C <= %d", K, C, kMaxK,
                kMaxC);
  CMH_CHECK_ARG(Y && B && W && Z_i && Z_t && obj2 && workspace, "dch_targets: null pointer");
  const size_t need = cmh_dch_targets_workspace_bytes(N);
  CMH_CHECK_ARG(workspace_bytes >= need, "dch_targets: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const TargetsWs w = carve_targets(workspace, N);
  const unsigned fb = static_cast<unsigned>((N + 63) / 64), rb = static_cast<unsigned>((N + 255) / 256);
  if (Qt)
    hipLaunchKernelGGL((targets_kernel<true>), dim3(fb), dim3(256), 0, st, Y, B, W, Z_i, Z_t, mu, static_cast<long long>(N), K, C, Qt, w.fpart);
  else
    hipLaunchKernelGGL((targets_kernel<false>), dim3(fb), dim3(256), 0, st, Y, B, W, Z_i, Z_t, mu, static_cast<long long>(N), K, C, Qt, w.fpart);
  hipLaunchKernelGGL(residual_kernel, dim3(rb), dim3(256), 0, st, Y, B, W, static_cast<long long>(N), K, C, w.rpart);
  hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(w.rpart), static_cast<int>(rb),
                     static_cast<const double*>(w.fpart), static_cast<int>(fb), W, K * C, lam, mu, obj2);
  CMH_CHECK_LAUNCH("dch_targets");
  return CMH_OK;
}

extern "C" size_t cmh_dch_dcc_workspace_bytes(int64_t N, int32_t rounds) {
  if (!rows_ok(N) || rounds < 1 || rounds > kMaxRounds) return 0;
  return carve_dcc(nullptr, N, rounds).total;
}

extern "C" int cmh_dch_dcc(const double* Qt, const double* G, int8_t* B, int64_t N, int32_t K, int32_t rounds, int64_t* flips, double* min_margin,
                           void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(rows_ok(N), "dch_dcc: N = %lld, need 1 <= N <= %lld", static_cast<long long>(N), kMaxRows);
  CMH_CHECK_ARG(K >= 1 && K <= kMaxK, "dch_dcc: K = %d, need 1 <= K <= %d", K, kMaxK);
  CMH_CHECK_ARG(rounds >= 1 && rounds <= kMaxRounds, "dch_dcc: rounds = %d, need 1 <= rounds <= %d", rounds, kMaxRounds);
  CMH_CHECK_ARG(Qt && G && B && flips && min_margin && workspace, "dch_dcc: null pointer");
  const size_t need = cmh_dch_dcc_workspace_bytes(N, rounds);
  CMH_CHECK_ARG(workspace_bytes >= need, "dch_dcc: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const DccWs w = carve_dcc(workspace, N, rounds);
  const unsigned blocks = static_cast<unsigned>((N + 255) / 256);
  const size_t lds = static_cast<size_t>(K) * K * sizeof(double);
#define CMH_DCC_CASE(NW_)                                                                                                              \
  if (K <= 32 * NW_) {                                                                                                                 \
    if (!reserve_lds(reinterpret_cast<const void*>(dcc_kernel<NW_>), lds)) return fail(CMH_ERR_LAUNCH, "dch_dcc: cannot reserve %zu bytes of LDS", lds); \
    hipLaunchKernelGGL((dcc_kernel<NW_>), dim3(blocks), dim3(256), lds, st, Qt, G, B, static_cast<long long>(N), K, rounds, w.fpart, w.mpart); \
  } else
  CMH_DCC_CASE(1)
  CMH_DCC_CASE(2)
  CMH_DCC_CASE(3)
  CMH_DCC_CASE(4) {}
#undef CMH_DCC_CASE
  hipLaunchKernelGGL(dcc_finish_kernel, dim3(1), dim3(64), 0, st, static_cast<const long long*>(w.fpart), static_cast<const double*>(w.mpart),
                     static_cast<int>(blocks), rounds, reinterpret_cast<long long*>(flips), min_margin);
  CMH_CHECK_LAUNCH("dch_dcc");
  return CMH_OK;
}
