// Shared by the head and loss translation units (heads, heads2, heads_bwd, losses, msl, qmi, mith, ddbh, djsrh, msc, cpf, dws): the wave and workgroup reductions,
// the workspace carver with its size check, and the row kernels of losses.hip that the other files launch.  The training-free fits (itq, dch)
// take wave_sum and the Carver from here through fit_common.h.
#pragma once

#include <cassert>

#include "cmh_common.h"

namespace cmh {

// ---- reductions, named for their order ------------------------------------------------------------------------------------------------
// over the 64 lanes of a wave: the xor butterfly from 32 down to 1; every lane ends with the result
template <typename T>      // float or double
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Over the 256 threads of a workgroup (sh: four elements of LDS), in one of two orders that round differently: keep each caller's.
// Left to right, ((r0 + r1) + r2) + r3: the f64 accumulator kernels of losses.hip and mith.hip, and qmi.hip's row sums.  (The f64 callers
// used to start from 0.0 + r0, which differs for r0 = -0.0 alone; they only test the sum against zero and add it to an accumulator.)
template <typename T>
__device__ __forceinline__ T block_sum_ltr(T v, T* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
// Pairwise, (r0 op r1) op (r2 op r3): msl.hip's row statistics (heads_bwd.hip's hyp_counts_kernel adds its two counts the same way)
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce_pairwise(T v, T* sh, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(sh[0], sh[1]), op(sh[2], sh[3]));
}

// ---- workspaces -------------------------------------------------------------------------------------------------------------------------
// The f64 accumulators (`double acc[..]`, zeroed at the start of a call) of the DSPH, DCHMT, TwDH, DNPH, sq-diff, Bayesian and InfoNCE
// forwards, and DCHMT's two any-non-zero flags behind them: a 256-byte block each.  Several calls get a workspace of exactly kAccBytes.
constexpr size_t kAccBytes = 256, kFlagBytes = 256;

// Bump allocator over a caller's workspace.  A null base only counts, so one carve_* function gives an entry point's *_workspace_bytes,
// the need of its size check and its pointers.  It returns its struct as one brace list (evaluated in order): the list is the layout.
struct Carver {
  char* base;
  size_t off = 0, slack = 0;
  // align: for the entries that accept any base, start at its first 256-byte boundary and budget the bytes that may skip
  explicit Carver(void* ws, bool align = false) : base(static_cast<char*>(ws)) {
    if (align && base) base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 255) & ~static_cast<uintptr_t>(255));
    if (align) slack = 256;
  }
  // the next slot; `round` is what the slot's size is rounded up to (4: the next slot follows at once)
  template <typename T = void>
  T* take(size_t bytes, size_t round = 256) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(bytes, round);
    return p;
  }
  float* f32(size_t bytes, size_t round = 256) { return take<float>(bytes, round); }
  size_t total(size_t unused = 0) const { return off + slack + unused; }   // unused: bytes a query has always asked for and no slot uses
};

// The workspace check of every entry point: present, and at least `need` bytes (code: what a short one returns, as the entry always did)
inline int open_ws(const char* what, const void* workspace, size_t bytes, size_t need, int code = CMH_ERR_WORKSPACE) {
  if (!workspace) return fail(CMH_ERR_INVALID, "%s: null workspace", what);
  if (bytes < need) return fail(code, "%s: workspace too small (%zu < %zu bytes)", what, bytes, need);
  return CMH_OK;
}

// ---- row kernels of losses.hip ----------------------------------------------------------------------------------------------------------
// out[r, :] = a[r, :] / n_r with n_r = |a[r, :]|, or max(|a[r, :]|, eps) when eps > 0 (F.normalize: 1e-12); optionally divisor[r] = n_r
// and anynz[0] |= (a has a non-zero element).  One wave per row.
void launch_normalize_rows(const float* a, float* out, float* divisor, int R, int K, float eps, int* anynz, hipStream_t st);
// norms[r] = |a[r, :]| (r < B), norms[B + r] = |b[r, :]|, each at least `floor` when floor > 0.  One wave per row.
void launch_row_norms2(const float* a, const float* b, int B, int K, float floor, float* norms, hipStream_t st);

}  // namespace cmh
