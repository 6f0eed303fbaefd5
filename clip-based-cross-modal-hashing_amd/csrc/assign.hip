// DNPH's noise assignment on the GPU (reference train/DNPH_TOMM/b_reg.py:5-40): P square linear assignment problems that share one
// noise matrix.  Three launches per call:
//   assign_cost_kernel    C[p][i][j] = || e[p][i] - s[j] ||_2 in f64 (inputs widened from f32, the sum over k in index order)
//   assign_solve_kernel   one workgroup per problem: shortest augmenting paths with f64 duals (the algorithm family of
//                         scipy.optimize.linear_sum_assignment, so the optimum is exact), deterministic argmin
//   assign_gather_kernel  out[p][i] = s[col4row[p][i]]
#include "cmh_common.h"

#include <cstdlib>

namespace cmh {
namespace {

constexpr int kMaxB = 1024;

// ---- cost matrix ------------------------------------------------------------------------------------------------------
// One block: 64 noise rows (j) x 16 embedding rows (i) of problem blockIdx.z; thread (jj, ig) forms 4 distances.  s and e pass
// through LDS in chunks of 32 columns, so global reads are coalesced; every sum adds its K terms in index order, the square
// and the add rounded separately (no FMA), so a host loop `acc += d * d` gives the same bits.
constexpr int kCJ = 64, kCI = 16, kCK = 32;

__global__ __launch_bounds__(256) void assign_cost_kernel(const float* __restrict__ emb, const float* __restrict__ rows,
                                                          double* __restrict__ cost, int B, int K) {
  __shared__ float sT[kCJ][kCK + 1];
  __shared__ float eT[kCI][kCK];
  const int tid = threadIdx.x, jj = tid & 63, ig = tid >> 6;
  const int j0 = blockIdx.x * kCJ, i0 = blockIdx.y * kCI;
  const float* e = emb + static_cast<size_t>(blockIdx.z) * B * K;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += kCK) {
    const int kn = min(kCK, K - k0);
    for (int t = tid; t < kCJ * kCK; t += 256) {
      const int r = t / kCK, c = t % kCK, j = j0 + r;
      sT[r][c] = (j < B && c < kn) ? rows[static_cast<size_t>(j) * K + k0 + c] : 0.f;
    }
    for (int t = tid; t < kCI * kCK; t += 256) {
      const int r = t / kCK, c = t % kCK, i = i0 + r;
      eT[r][c] = (i < B && c < kn) ? e[static_cast<size_t>(i) * K + k0 + c] : 0.f;
    }
    __syncthreads();
    for (int kk = 0; kk < kn; ++kk) {
      const double sv = static_cast<double>(sT[jj][kk]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double d = static_cast<double>(eT[ig * 4 + r][kk]) - sv;
        acc[r] = __dadd_rn(acc[r], __dmul_rn(d, d));
      }
    }
    __syncthreads();
  }
  const int j = j0 + jj;
  if (j < B) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + ig * 4 + r;
      if (i < B) cost[(static_cast<size_t>(blockIdx.z) * B + i) * B + j] = __dsqrt_rn(acc[r]);   // the norm, not its square
    }
  }
}

// ---- solver -----------------------------------------------------------------------------------------------------------
// f64 -> u64 with the same order (-0 folded into +0; a NaN sorts above +inf or below -inf, so the order is total)
__device__ __forceinline__ unsigned long long order_key(double x) {
  unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
  if (b == 0x8000000000000000ull) b = 0;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __longlong_as_double(static_cast<long long>((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct alignas(16) AssignSlot {
  unsigned long long key;   // order_key(shortest[j])
  uint32_t aux;             // (column j is assigned) << 16 | j; 0xffffffff = no candidate
  int32_t row;              // row4col[j], -1 = unassigned
};

constexpr uint32_t kNoCand = 0xffffffffu;

// Thread t owns the CPT columns t*CPT .. t*CPT+CPT-1 (so within a wave, and across waves, a lower thread holds lower columns) and
// keeps their shortest / path / v / scanned flag and a copy of row4col in registers; u, row4col, col4row live in LDS.  One
// Dijkstra step = one cost row from L2, the register update, a wave argmin, ONE barrier, and the argmin over the waves' slots,
// which every thread forms for itself from the same LDS words (so every thread takes the same branch).  The slots are double
// buffered: a wave writes slot[p ^ 1] of step n + 1 only behind barrier n, which every wave reaches after it has written slot[p] of
// step n, and it rewrites slot[p] in step n + 2 only behind barrier n + 1, which every wave reaches after reading slot[p] of step n.
//
// Argmin order: lowest shortest[j], then an unassigned column before an assigned one, then the lowest column.  It is a total
// order on integers, so the result does not depend on the run; no atomics anywhere.
//
// Termination and validity, whatever the cost matrix holds (non-finite values included):
//  * every loop runs to a bound that depends on B and the loop counters alone: B augmentations; at most cur + 1 <= B Dijkstra
//    steps in augmentation cur; at most B hops in the path walk.
//  * a Dijkstra step picks, by that total order, one real column that this augmentation has not scanned: at step s (s <= cur <=
//    B - 1) there are B - s >= 1 of them, and a real candidate's aux (< 2^17) sorts below the "no candidate" word even where the
//    keys are equal.  The step scans that column.  Only `cur` columns are assigned, so after at most `cur` steps every assigned
//    column is scanned and step cur at the latest picks an unassigned one: the sink exists when the loop ends.
//  * path[j] starts as `cur` and is only ever overwritten with the row being expanded, that is, a row that entered the tree at a
//    step <= the step that scans j.  The walk goes from column j to row path[j] and on to that row's old column, which was
//    scanned when the row entered, hence strictly earlier than j: the scan steps along the walk strictly decrease, so the walk
//    never meets a row twice and ends at `cur` (the only row that entered without a column) within B hops.  Each row on it takes
//    the column before it and gives up its own to the next, so row4col / col4row stay a matching, now with cur + 1 pairs.
//  After B augmentations col4row is a permutation of 0 .. B-1.
template <int T, int CPT>
__global__ __launch_bounds__(T) void assign_solve_kernel(const double* __restrict__ cost, int32_t* __restrict__ col, int B) {
  constexpr int NW = T / 64;
  constexpr int NC = T * CPT < kMaxB ? T * CPT : kMaxB;
  __shared__ double u[NC];
  __shared__ int32_t row4col[NC], col4row[NC], path[NC];
  __shared__ AssignSlot slot[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* C = cost + static_cast<size_t>(blockIdx.x) * B * B;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  for (int j = tid; j < B; j += T) {
    u[j] = 0.0;
    row4col[j] = -1;
    col4row[j] = -1;
  }
  double v[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) v[c] = 0.0;
  int par = 0;
  __syncthreads();

  for (int cur = 0; cur < B; ++cur) {
    double sh[CPT];
    int32_t pth[CPT], myrow[CPT];
    uint32_t scanned = 0;          // bit c: column c of mine is scanned in this augmentation (columns >= B: always)
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = tid * CPT + c;
      sh[c] = inf;
      pth[c] = cur;
      myrow[c] = j < B ? row4col[j] : -1;
      if (j >= B) scanned |= 1u << c;
    }
    int i = cur, sink = -1;
    double minVal = 0.0;
    for (int step = 0; step <= cur; ++step) {
      const double ui = u[i];
      const double* Ci = C + static_cast<size_t>(i) * B;
      unsigned long long bk = ~0ull;
      uint32_t ba = kNoCand;
      int32_t br = -1;
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int j = tid * CPT + c;
        if (!((scanned >> c) & 1u)) {
          const double r = minVal + Ci[j] - ui - v[c];
          if (r < sh[c]) {
            sh[c] = r;
            pth[c] = i;
          }
          const unsigned long long k = order_key(sh[c]);
          const uint32_t a = (myrow[c] >= 0 ? 0x10000u : 0u) | static_cast<uint32_t>(j);
          if (k < bk || (k == bk && a < ba)) {
            bk = k;
            ba = a;
            br = myrow[c];
          }
        }
      }
      // wave argmin: the lowest key by butterfly, then the first lane (= lowest column) among the unassigned holders of it,
      // else among all real holders
      unsigned long long mk = bk;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(mk, o, 64);
        mk = other < mk ? other : mk;
      }
      const bool real = ba != kNoCand, eq = bk == mk;
      const unsigned long long free_m = __ballot(eq && real && ba < 0x10000u), real_m = __ballot(eq && real);
      const int win = free_m ? __ffsll(static_cast<long long>(free_m)) - 1 : (real_m ? __ffsll(static_cast<long long>(real_m)) - 1 : 0);
      if (lane == win) slot[par][wave] = AssignSlot{bk, ba, br};
      __syncthreads();
      AssignSlot best = slot[par][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const AssignSlot s = slot[par][w];
        if (s.key < best.key || (s.key == best.key && s.aux < best.aux)) best = s;
      }
      par ^= 1;
      const int jb = static_cast<int>(best.aux & 0xffffu);
      minVal = key_value(best.key);
#pragma unroll
      for (int c = 0; c < CPT; ++c)
        if (tid * CPT + c == jb) scanned |= 1u << c;
      if (best.row < 0) {
        sink = jb;
        break;
      }
      i = best.row;
    }
    // duals (scipy's update, per scanned column instead of per visited row: the visited rows other than cur are exactly the
    // owners of the scanned assigned columns) and the path into LDS for the walk
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = tid * CPT + c;
      if (j < B) {
        path[j] = pth[c];
        if (((scanned >> c) & 1u) && myrow[c] >= 0) {
          const double d = minVal - sh[c];
          u[myrow[c]] += d;
          v[c] -= d;
        }
      }
    }
    if (tid == 0) u[cur] += minVal;
    __syncthreads();
    if (tid == 0 && sink >= 0) {
      int j = sink;
      for (int hop = 0; hop < B; ++hop) {
        const int r = path[j];
        row4col[j] = r;
        const int jn = col4row[r];
        col4row[r] = j;
        j = jn;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  for (int r = tid; r < B; r += T) col[static_cast<size_t>(blockIdx.x) * B + r] = col4row[r];
}

// ---- gather -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void assign_gather_kernel(const float* __restrict__ rows, const int32_t* __restrict__ col,
                                                            float* __restrict__ out, int32_t* __restrict__ col_out, int B, int K) {
  const int i = blockIdx.x, p = blockIdx.y;
  const int j = col[static_cast<size_t>(p) * B + i];
  const float* src = rows + static_cast<size_t>(j) * K;
  float* dst = out + (static_cast<size_t>(p) * B + i) * K;
  for (int k = threadIdx.x; k < K; k += 128) dst[k] = src[k];
  if (col_out && threadIdx.x == 0) col_out[static_cast<size_t>(p) * B + i] = j;
}

// columns per thread: 1 by default; CMH_ASSIGN_CPT = 1 | 2 | 4 is a measuring switch, results do not depend on it
int assign_cpt() {
  static const int cpt = [] {
    const char* e = getenv("CMH_ASSIGN_CPT");
    const int v = e ? atoi(e) : 1;
    return (v == 2 || v == 4) ? v : 1;
  }();
  return cpt;
}

template <int CPT>
void launch_solve(const double* cost, int32_t* col, int P, int B, hipStream_t st) {
  const int need = (B + CPT - 1) / CPT;
#define CMH_ASSIGN_CASE(T_) \
  if (need <= T_) { hipLaunchKernelGGL((assign_solve_kernel<T_, CPT>), dim3(P), dim3(T_), 0, st, cost, col, B); return; }
  CMH_ASSIGN_CASE(64)
  CMH_ASSIGN_CASE(128)
  CMH_ASSIGN_CASE(256)
  CMH_ASSIGN_CASE(512)
  CMH_ASSIGN_CASE(1024)
#undef CMH_ASSIGN_CASE
}

size_t cost_bytes(int P, int B) { return align_up(static_cast<size_t>(P) * B * B * sizeof(double), 256); }

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_assign_rows_workspace_bytes(int32_t P, int32_t B) {
  if (P < 1 || B < 1 || B > kMaxB) return 0;
  return cost_bytes(P, B) + align_up(static_cast<size_t>(P) * B * sizeof(int32_t), 256);
}

extern "C" int cmh_assign_rows(const float* emb, const float* rows, int32_t P, int32_t B, int32_t K, float* out, int32_t* col_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(P >= 1 && P <= 65535, "assign_rows: P = %d, need 1 <= P <= 65535", P);
  CMH_CHECK_ARG(B >= 1 && B <= kMaxB, "assign_rows: B = %d, need 1 <= B <= %d", B, kMaxB);
  CMH_CHECK_ARG(K >= 1, "assign_rows: K = %d, need K >= 1", K);
  CMH_CHECK_ARG(emb && rows && out && workspace, "assign_rows: null pointer");
  const size_t need = cmh_assign_rows_workspace_bytes(P, B);
  if (workspace_bytes < need)
    return fail(CMH_ERR_WORKSPACE, "assign_rows: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  double* cost = static_cast<double*>(workspace);
  int32_t* col = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + cost_bytes(P, B));
  hipLaunchKernelGGL(assign_cost_kernel, dim3((B + kCJ - 1) / kCJ, (B + kCI - 1) / kCI, P), dim3(256), 0, st, emb, rows, cost, B, K);
  switch (assign_cpt()) {
    case 2: launch_solve<2>(cost, col, P, B, st); break;
    case 4: launch_solve<4>(cost, col, P, B, st); break;
    default: launch_solve<1>(cost, col, P, B, st); break;
  }
  hipLaunchKernelGGL(assign_gather_kernel, dim3(B, P), dim3(128), 0, st, rows, col, out, col_out, B, K);
  CMH_CHECK_LAUNCH("assign_rows");
  return CMH_OK;
}
