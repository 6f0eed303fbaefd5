// Hash-table lookup on packed codes: the items of a database grouped by EQUAL code, and the groups found by key.
//   cmh_code_sort           order[N]: the item indices in ascending key order, ties by ascending item index (stable)
//   cmh_code_bucket_count   head[N]: inclusive scan of "this sorted position starts a new key"; U = the number of distinct keys
//   cmh_code_bucket_fill    starts[U + 1] (offsets into order) and codes[U, W] (each bucket's key), ascending
//   cmh_bucket_probe_count / _fill   per query the buckets whose key is the query with at most `radius` bits flipped
//
// The key of a row is its W = ceil(bits / 32) sign words with the bits at and behind `bits` cleared, compared as one W-word unsigned
// integer with word W - 1 most significant.  Codes are in {-1, +1} (the nz plane is all ones; the Python layer refuses others), so
// two items are equal iff their keys are, and the Hamming distance of two items is the number of key bits that differ - the
// distance of utils/calc_utils.py:8-13 in whole units.
//
// The sort is a least-significant-digit radix sort over ceil(bits / 8) digits of 8 bits (the digits behind them are zero for every
// key: no pass): the passes and the scans of retrieval_sort.h, which the substring tables of retrieval_mih.hip share.  No kernel
// waits for another workgroup.  Every loop is bounded by an argument, every access checked against N, U or Q, every offset 64-bit.
// Every output word is written once, without atomics: two calls give equal bytes, on any stream.
//
// The probes.  A query has P = 1 + bits + bits (bits - 1) / 2 candidate keys within radius 2: itself, one flipped bit i ascending,
// pairs (i, j), i < j, in lexicographic order (radius 0 / 1: the first 1 / 1 + bits of them).  One workgroup owns a query and takes
// its probes kProbeThreads at a time in probe order; a thread builds its key (a pair is unranked from the probe's number), finds it by one
// binary search over codes (<= 32 steps, word W - 1 first), and a hit's place in the query's list is the hits of the rounds before
// + the hits of the waves before it in this round (LDS) + the hits of the lower lanes (ballot): the list is in probe order on every
// run.  Distinct probes are distinct keys, so a bucket is hit at most once per query.  The count pass and the fill pass both
// search; nothing per probe is stored.
#include "retrieval_sort.h"

namespace cmh {
namespace {

constexpr int kProbeThreads = 1024;
constexpr int kProbeWaves = kProbeThreads / 64;
constexpr int kProbeWords = CMH_BUCKET_BITS_MAX / 32;

// ---- buckets ------------------------------------------------------------------------------------------------------------------
// head[i] = 1 when sorted position i starts a new key
__global__ __launch_bounds__(256) void bucket_mark_kernel(const uint32_t* __restrict__ sign, const int32_t* __restrict__ order, int64_t N,
                                                          int W, int bits, uint32_t* __restrict__ head) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= N) return;
  uint32_t differs = i == 0;
  if (i > 0) {
    const int64_t a = order[i], b = order[i - 1];
    if (a < 0 || a >= N || b < 0 || b >= N) {          // not a permutation of the items: nothing is read outside the planes
      head[i] = 0;
      return;
    }
    for (int w = 0; w < W; ++w) differs |= key_word(sign, a, W, w, bits) != key_word(sign, b, W, w, bits);
  }
  head[i] = differs;
}

__global__ __launch_bounds__(256) void bucket_fill_kernel(const uint32_t* __restrict__ sign, const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ head, int64_t N, int W, int bits, int64_t U,
                                                          int32_t* __restrict__ starts, uint32_t* __restrict__ codes) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i == 0) starts[U] = static_cast<int32_t>(N);
  if (i >= N) return;
  const int64_t b = static_cast<int64_t>(head[i]) - 1;
  if ((i > 0 && head[i] == head[i - 1]) || b < 0 || b >= U) return;      // not a bucket's first position / not this table's head
  const int64_t item = order[i];
  if (item < 0 || item >= N) return;
  starts[b] = static_cast<int32_t>(i);
  for (int w = 0; w < W; ++w) codes[static_cast<size_t>(b) * W + w] = key_word(sign, item, W, w, bits);
}

// ---- probes -------------------------------------------------------------------------------------------------------------------
struct ProbeArgs {
  const uint32_t* q_sign;
  const uint32_t* codes;
  const int32_t* starts;
  int64_t U;
  int Q, W, bits, probes;
  int32_t* n_buckets;            // count pass
  long long* n_items;
  const long long* offsets;      // fill pass: [Q + 1]
  int64_t capacity;
  int32_t* hit_bucket;
  int32_t* hit_dist;
};

// pairs (i, j), i < j < B in lexicographic order: the pairs before row i
__device__ __forceinline__ int pairs_before(int i, int B) { return i * (2 * B - i - 1) / 2; }

// -> the bucket whose key is k, or -1
__device__ __forceinline__ int64_t probe_find(const uint32_t* __restrict__ codes, int64_t U, int W, const uint32_t (&k)[kProbeWords]) {
  int64_t lo = 0, hi = U;                              // the first bucket whose key is not below k
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint32_t* c = codes + static_cast<size_t>(mid) * W;
    int less = 0;                                      // codes[mid] < k ?  (word W - 1 is the most significant)
#pragma unroll
    for (int w = kProbeWords - 1; w >= 0; --w) {
      if (w < W && less == 0) {
        const uint32_t cw = c[w];
        less = cw < k[w] ? 1 : cw > k[w] ? -1 : 0;
      }
    }
    if (less > 0) lo = mid + 1; else hi = mid;
  }
  if (lo != hi || lo >= U) return -1;
  bool equal = true;
#pragma unroll
  for (int w = 0; w < kProbeWords; ++w)
    if (w < W) equal = equal && codes[static_cast<size_t>(lo) * W + w] == k[w];
  return equal ? lo : -1;
}

template <bool FILL>
__global__ __launch_bounds__(kProbeThreads) void probe_kernel(ProbeArgs a) {
  __shared__ uint32_t wave_hits[kProbeWaves];
  __shared__ unsigned long long wave_items[kProbeWaves];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (q >= a.Q) return;
  uint32_t key[kProbeWords];
#pragma unroll
  for (int w = 0; w < kProbeWords; ++w) key[w] = w < a.W ? a.q_sign[static_cast<size_t>(q) * a.W + w] & word_mask(w, a.bits) : 0u;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t done = 0;                                    // hits of the rounds before this one
  unsigned long long items = 0;                        // (count pass) this thread's share of the hit buckets' sizes
  int64_t list_lo = 0, list_hi = 0;
  if (FILL) {
    list_lo = a.offsets[q];
    list_hi = a.offsets[q + 1] < a.capacity ? a.offsets[q + 1] : a.capacity;
  }
  for (int first = 0; first < a.probes; first += kProbeThreads) {
    const int p = first + tid;
    int64_t found = -1;
    int dist = 0;
    if (p < a.probes) {
      uint32_t k[kProbeWords];
#pragma unroll
      for (int w = 0; w < kProbeWords; ++w) k[w] = key[w];
      int i = -1, j = -1;
      if (p >= 1 && p <= a.bits) {
        i = p - 1;
        dist = 1;
      } else if (p > a.bits) {
        const int t = p - 1 - a.bits, B = a.bits;
        const float s = static_cast<float>(2 * B - 1);
        i = static_cast<int>((s - sqrtf(s * s - 8.0f * static_cast<float>(t))) * 0.5f);
        i = i < 0 ? 0 : i > B - 2 ? B - 2 : i;
        for (int fix = 0; fix < 2 && i > 0 && pairs_before(i, B) > t; ++fix) --i;
        for (int fix = 0; fix < 2 && i < B - 2 && pairs_before(i + 1, B) <= t; ++fix) ++i;
        j = i + 1 + (t - pairs_before(i, B));
        dist = 2;
      }
      const bool legal = dist < 2 || (i >= 0 && i < j && j < a.bits);
#pragma unroll
      for (int w = 0; w < kProbeWords; ++w) {
        if (i >= 0 && (i >> 5) == w) k[w] ^= 1u << (i & 31);
        if (j >= 0 && (j >> 5) == w) k[w] ^= 1u << (j & 31);
      }
      if (legal) found = probe_find(a.codes, a.U, a.W, k);
    }
    const bool hit = found >= 0;
    const unsigned long long votes = __ballot(hit);
    __syncthreads();                                   // (the previous round's wave_hits are read)
    if (lane == 0) wave_hits[wave] = static_cast<uint32_t>(__popcll(votes));
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kProbeWaves; ++w) {
      const uint32_t h = wave_hits[w];
      before += w < wave ? h : 0u;
      all += h;
    }
    if (hit) {
      if (FILL) {
        const int64_t at = list_lo + done + before + __popcll(votes & below);
        if (at >= list_lo && at < list_hi) {
          a.hit_bucket[at] = static_cast<int32_t>(found);
          a.hit_dist[at] = dist;
        }
      } else {
        items += static_cast<unsigned long long>(a.starts[found + 1] - a.starts[found]);
      }
    }
    done += all;
  }
  if (!FILL) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) items += __shfl_down(items, o);
    __syncthreads();
    if (lane == 0) wave_items[wave] = items;
    __syncthreads();
    if (tid == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kProbeWaves; ++w) total += wave_items[w];
      a.n_buckets[q] = static_cast<int32_t>(done);
      a.n_items[q] = static_cast<long long>(total);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

int check_sort_shape(const char* what, int64_t N, int bits) {
  if (N < 1 || N > 2147483647ll)
    return what ? fail(CMH_ERR_INVALID, "%s: N=%lld outside [1, 2^31 - 1]", what, static_cast<long long>(N)) : CMH_ERR_INVALID;
  if (bits < 1 || bits > 32 * kBktMaxWords)
    return what ? fail(CMH_ERR_INVALID, "%s: bits=%d outside [1, %d]", what, bits, 32 * kBktMaxWords) : CMH_ERR_INVALID;
  return CMH_OK;
}

int check_probe_shape(const char* what, int Q, int64_t U, int bits, int radius) {
  CMH_CHECK_ARG(Q >= 1 && Q <= 65535, "%s: Q=%d outside [1, 65535]", what, Q);
  CMH_CHECK_ARG(U >= 1 && U <= 2147483647ll, "%s: U=%lld outside [1, 2^31 - 1]", what, static_cast<long long>(U));
  CMH_CHECK_ARG(bits >= 1 && bits <= CMH_BUCKET_BITS_MAX, "%s: bits=%d outside [1, %d]", what, bits, CMH_BUCKET_BITS_MAX);
  CMH_CHECK_ARG(radius >= 0 && radius <= CMH_BUCKET_RADIUS_MAX, "%s: radius=%d outside [0, %d]", what, radius, CMH_BUCKET_RADIUS_MAX);
  return CMH_OK;
}

int probe_count_of(int bits, int radius) { return radius == 0 ? 1 : radius == 1 ? 1 + bits : 1 + bits + bits * (bits - 1) / 2; }


}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_code_sort_workspace_bytes(int64_t N, int32_t bits) {
  return check_sort_shape(nullptr, N, bits) == CMH_OK ? sort_plan(N, bits).bytes : 0;
}

extern "C" int cmh_code_sort(const uint32_t* sign, int64_t N, int32_t bits, int32_t* order, void* workspace, size_t workspace_bytes,
                             void* stream) {
  CMH_CHECK_ARG(sign && order, "code_sort: null pointer");
  const int rc = check_sort_shape("code_sort", N, bits);
  if (rc != CMH_OK) return rc;
  const SortPlan p = sort_plan(N, bits);
  if (!workspace || workspace_bytes < p.bytes) return fail(CMH_ERR_WORKSPACE, "code_sort: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
  return run_sort("code_sort", sign, N, bits, 0, p.passes, p, aligned_ws(workspace), order, as_stream(stream));
}

extern "C" int cmh_code_bucket_count(const uint32_t* sign, const int32_t* order, int64_t N, int32_t bits, int32_t* head,
                                     int64_t* n_buckets, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(sign && order && head && n_buckets, "code_bucket_count: null pointer");
  const int rc = check_sort_shape("code_bucket_count", N, bits);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(n_buckets) % 8 == 0, "code_bucket_count: n_buckets is a 64-bit integer: aligned to 8 bytes");
  const SortPlan p = sort_plan(N, bits);
  if (!workspace || workspace_bytes < p.bytes)
    return fail(CMH_ERR_WORKSPACE, "code_bucket_count: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
  uint32_t* sums = reinterpret_cast<uint32_t*>(aligned_ws(workspace) + p.off_sums);
  hipStream_t st = as_stream(stream);
  uint32_t* marks = reinterpret_cast<uint32_t*>(head);
  hipLaunchKernelGGL(bucket_mark_kernel, dim3(static_cast<unsigned>((N + 255) / 256)), dim3(256), 0, st, sign, order, N, p.W, bits, marks);
  CMH_CHECK_LAUNCH("code_bucket_count (mark)");
  return launch_scan<true>(marks, N, sums, reinterpret_cast<long long*>(n_buckets), "code_bucket_count (scan)", st);
}

extern "C" int cmh_code_bucket_fill(const uint32_t* sign, const int32_t* order, const int32_t* head, int64_t N, int32_t bits, int64_t U,
                                    int32_t* starts, int32_t* codes, void* stream) {
  CMH_CHECK_ARG(sign && order && head && starts && codes, "code_bucket_fill: null pointer");
  const int rc = check_sort_shape("code_bucket_fill", N, bits);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(U >= 1 && U <= N, "code_bucket_fill: U=%lld outside [1, N=%lld]", static_cast<long long>(U), static_cast<long long>(N));
  hipLaunchKernelGGL(bucket_fill_kernel, dim3(static_cast<unsigned>((N + 255) / 256)), dim3(256), 0, as_stream(stream), sign, order, head,
                     N, (bits + 31) / 32, bits, U, starts, reinterpret_cast<uint32_t*>(codes));
  CMH_CHECK_LAUNCH("code_bucket_fill");
  return CMH_OK;
}

extern "C" int cmh_bucket_probe_count(const uint32_t* q_sign, int32_t Q, const int32_t* codes, const int32_t* starts, int64_t U,
                                      int32_t bits, int32_t radius, int32_t* n_hit_buckets, int64_t* n_hit_items, void* stream) {
  CMH_CHECK_ARG(q_sign && codes && starts && n_hit_buckets && n_hit_items, "bucket_probe_count: null pointer");
  const int rc = check_probe_shape("bucket_probe_count", Q, U, bits, radius);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(n_hit_items) % 8 == 0, "bucket_probe_count: n_hit_items holds 64-bit integers: aligned to 8 bytes");
  ProbeArgs a = {};
  a.q_sign = q_sign; a.codes = reinterpret_cast<const uint32_t*>(codes); a.starts = starts; a.U = U; a.Q = Q; a.W = (bits + 31) / 32;
  a.bits = bits; a.probes = probe_count_of(bits, radius);
  a.n_buckets = n_hit_buckets; a.n_items = reinterpret_cast<long long*>(n_hit_items);
  hipLaunchKernelGGL(probe_kernel<false>, dim3(static_cast<unsigned>(Q)), dim3(kProbeThreads), 0, as_stream(stream), a);
  CMH_CHECK_LAUNCH("bucket_probe_count");
  return CMH_OK;
}

extern "C" int cmh_bucket_probe_fill(const uint32_t* q_sign, int32_t Q, const int32_t* codes, const int32_t* starts, int64_t U,
                                     int32_t bits, int32_t radius, const int64_t* bucket_offsets, int64_t capacity, int32_t* hit_bucket,
                                     int32_t* hit_dist, void* stream) {
  CMH_CHECK_ARG(q_sign && codes && starts && bucket_offsets && hit_bucket && hit_dist, "bucket_probe_fill: null pointer");
  const int rc = check_probe_shape("bucket_probe_fill", Q, U, bits, radius);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(capacity >= 1, "bucket_probe_fill: capacity=%lld below 1 (no hits: no call)", static_cast<long long>(capacity));
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(bucket_offsets) % 8 == 0, "bucket_probe_fill: bucket_offsets holds 64-bit integers: aligned to 8 bytes");
  ProbeArgs a = {};
  a.q_sign = q_sign; a.codes = reinterpret_cast<const uint32_t*>(codes); a.starts = starts; a.U = U; a.Q = Q; a.W = (bits + 31) / 32;
  a.bits = bits; a.probes = probe_count_of(bits, radius);
  a.offsets = reinterpret_cast<const long long*>(bucket_offsets); a.capacity = capacity; a.hit_bucket = hit_bucket; a.hit_dist = hit_dist;
  hipLaunchKernelGGL(probe_kernel<true>, dim3(static_cast<unsigned>(Q)), dim3(kProbeThreads), 0, as_stream(stream), a);
  CMH_CHECK_LAUNCH("bucket_probe_fill");
  return CMH_OK;
}
