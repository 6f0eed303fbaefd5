// Merge of two top-k lists of the same queries (cmh_topk_merge): what lets the retrieval layer search a database larger than
// cmh_hamming_topk takes (N <= 524 287) as shards and still return, bit for bit, the answer of one search over the whole
// database (utils/retrieval.py).  Both rows are ascending by (dist, idx) and every index of b is larger than every index of a, so
// the order of cmh_hamming_topk over the union is "by distance, a before b at equal distance".
//
// Merge by RANK, as everything in retrieval.hip: nothing is sorted, nothing is compared and swapped, every output is written once.
//   a[q, i] goes to column i + #{j : b_dist[q, j] <  a_dist[q, i]}      (a strict lower bound in b's row)
//   b[q, j] goes to column j + #{i : a_dist[q, i] <= b_dist[q, j]}      (an upper bound in a's row)
// The two rules are a bijection of the ka + kb entries onto the columns 0 .. ka + kb - 1; an entry whose column is >= k is
// dropped.  Distances are 0.5 * h exactly, so the float comparisons are exact; there are no atomics and no workspace.
// An entry at position >= k of its own row can never reach a column < k, and a count that reaches k drops the entry whatever lies
// behind: only the first min(ka, k) / min(kb, k) entries of a row are read, staged or searched (na / nb below).
//
// Mapping: one entry per thread and round, a binary search per entry.  A 256-thread workgroup takes R rows, R = 4 (one wave per
// row) while a row's na + nb entries fit one wave's four rounds (<= 256), else 1.  The distances of the R rows (a's first na, then
// b's first nb) are staged in LDS, (na + nb) * 4 bytes per row, so the ~log2(k) probes of a search cost LDS reads; rows longer than
// kStageMax = 16 384 floats (64 KiB) are searched in global memory instead (STAGED = false), and there the grid's y dimension cuts a row
// into slices of kSlice entries (more where the grid's y limit asks for it) so that a few long rows still spread over the chip.
#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kThreads = 256;
constexpr int kStageMax = 16384;      // floats of LDS per workgroup: 64 KiB (two workgroups per CU)
constexpr int kSlice = 4096;          // entries per workgroup of the unstaged form, at least
constexpr int kQueriesMax = 65535;    // rows per call, as the searches that make the lists: the grid's x stays far below its limit

struct MergeArgs {
  const int32_t *a_idx, *b_idx;
  const float *a_dist, *b_dist;
  const uint8_t *a_tag, *b_tag;
  int32_t* idx;
  float* dist;
  uint8_t* tag;
  int ka, kb, na, nb, k, Q, b_base, rows, slice;      // rows = R: query rows per workgroup; slice: entries per workgroup (unstaged)
};

// #{j < n : p[j] < v} (strict = true) or #{j < n : p[j] <= v}: p ascending
template <bool STRICT>
__device__ __forceinline__ int rank_in(const float* p, int n, float v) {
  int lo = 0;
  while (n > 0) {
    const int half = n >> 1;
    const float m = p[lo + half];
    const bool below = STRICT ? m < v : m <= v;
    lo = below ? lo + half + 1 : lo;
    n = below ? n - half - 1 : half;
  }
  return lo;
}

template <bool STAGED>
__global__ __launch_bounds__(kThreads) void topk_merge_kernel(MergeArgs a) {
  extern __shared__ float stage[];
  const int per = kThreads / a.rows;                       // threads per row: 256 or 64
  const int slot = threadIdx.x / per, t = threadIdx.x - slot * per;
  const int total = a.na + a.nb;
  const int qa = blockIdx.x * a.rows + slot;
  const bool live = qa < a.Q;
  const size_t q = static_cast<size_t>(live ? qa : a.Q - 1);      // slots behind the last row stage it once more and write nothing
  const float* ad = a.a_dist + q * a.ka;
  const float* bd = a.b_dist + q * a.kb;
  const float* sa = ad;
  const float* sb = bd;
  int e0 = 0, e1 = total;
  if (STAGED) {
    float* mine = stage + static_cast<size_t>(slot) * total;
    for (int e = t; e < a.na; e += per) mine[e] = ad[e];
    for (int e = t; e < a.nb; e += per) mine[a.na + e] = bd[e];
    __syncthreads();
    sa = mine;
    sb = mine + a.na;
  } else {
    e0 = blockIdx.y * a.slice;                             // (< total <= INT32_MAX: the host sized the grid so)
    e1 = total - e0 > a.slice ? e0 + a.slice : total;
  }
  if (!live) return;
  for (int e = e0 + t; e < e1; e += per) {
    const bool from_a = e < a.na;
    const int i = from_a ? e : e - a.na;
    const float v = from_a ? sa[i] : sb[i];
    const int col = i + (from_a ? rank_in<true>(sb, a.nb, v) : rank_in<false>(sa, a.na, v));
    if (col < a.k) {
      const size_t o = q * a.k + col;
      const size_t s = from_a ? q * a.ka + i : q * a.kb + i;
      a.idx[o] = from_a ? a.a_idx[s] : a.b_idx[s] + a.b_base;
      a.dist[o] = v;
      if (a.tag) a.tag[o] = from_a ? a.a_tag[s] : a.b_tag[s];
    }
  }
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" int cmh_topk_merge(const int32_t* a_idx, const float* a_dist, const uint8_t* a_tag, int32_t ka, const int32_t* b_idx,
                              const float* b_dist, const uint8_t* b_tag, int32_t kb, int32_t b_base, int32_t Q, int32_t k,
                              int32_t* idx, float* dist, uint8_t* tag, void* stream) {
  CMH_CHECK_ARG(a_idx && a_dist && b_idx && b_dist && idx && dist, "topk_merge: null pointer");
  CMH_CHECK_ARG((a_tag != nullptr) == (b_tag != nullptr) && (a_tag != nullptr) == (tag != nullptr),
                "topk_merge: tags on some of a, b and the output only");
  CMH_CHECK_ARG(ka >= 1 && kb >= 1 && Q >= 1 && Q <= kQueriesMax, "topk_merge: ka=%d kb=%d Q=%d (Q <= %d)", ka, kb, Q, kQueriesMax);
  CMH_CHECK_ARG(k >= 1 && static_cast<int64_t>(k) <= static_cast<int64_t>(ka) + kb, "topk_merge: k=%d outside [1, ka + kb = %lld]", k,
                static_cast<long long>(ka) + kb);
  CMH_CHECK_ARG(b_base >= 0, "topk_merge: b_base=%d", b_base);
  MergeArgs a;
  a.a_idx = a_idx; a.a_dist = a_dist; a.a_tag = a_tag; a.b_idx = b_idx; a.b_dist = b_dist; a.b_tag = b_tag;
  a.idx = idx; a.dist = dist; a.tag = tag;
  a.ka = ka; a.kb = kb; a.k = k; a.Q = Q; a.b_base = b_base;
  a.na = ka < k ? ka : k;
  a.nb = kb < k ? kb : k;
  a.slice = 0;
  const int64_t total = static_cast<int64_t>(a.na) + a.nb;      // the kernel counts entries in an int, one round of threads past the end
  CMH_CHECK_ARG(total <= INT32_MAX - kThreads, "topk_merge: k=%d: rows of %lld entries", k, static_cast<long long>(total));
  hipStream_t st = as_stream(stream);
  if (total <= kStageMax) {
    a.rows = total <= kThreads ? 4 : 1;
    const size_t lds = static_cast<size_t>(a.rows) * total * sizeof(float);
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(topk_merge_kernel<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "topk_merge: cannot reserve %zu bytes of LDS", lds);
    hipLaunchKernelGGL((topk_merge_kernel<true>), dim3((Q + a.rows - 1) / a.rows), dim3(kThreads), lds, st, a);
  } else {
    a.rows = 1;
    const int64_t by_grid = (total + 65534) / 65535;      // grid.y <= 65535
    a.slice = static_cast<int>(by_grid > kSlice ? by_grid : kSlice);
    hipLaunchKernelGGL((topk_merge_kernel<false>), dim3(Q, static_cast<unsigned>((total + a.slice - 1) / a.slice)), dim3(kThreads), 0, st, a);
  }
  CMH_CHECK_LAUNCH("topk_merge");
  return CMH_OK;
}
