// The stable least-significant-digit radix passes over the 8-bit digits of packed sign words, and the scan over workgroups they
// use, written once for the tables that sort item indices by a key cut from the codes:
//   retrieval_buckets.hip   the whole code as the key: digits 0 .. ceil(bits / 8) - 1
//   retrieval_mih.hip       16-bit substring j as the key: digits 2 j and 2 j + 1
// DIGIT d of an item is byte d & 3 of word d >> 2 of its sign row, with the bits at and behind `bits` cleared.  A sort is `passes`
// passes over the digits digit0, digit0 + 1, ...; pass p is, over tiles of kSortTile positions of the current index buffer,
//   sort_hist_kernel      counts[bin][tile]: per-tile digit histogram (LDS counters), stored bin-major, so that
//   scan (three launches) ONE exclusive scan of the flat array is, at [bin][tile], the first destination of the tile's keys of that bin
//   sort_decide_kernel    all N keys in one bin?  Then the pass would be the identity permutation: it is skipped, and the next pass
//                         reads the same buffer.  Writes skip[pass] and src[pass + 1] in the workspace; the host reads nothing
//   sort_scatter_kernel   the stable scatter.  A wave owns kSortTile / 4 consecutive positions and takes them 64 at a time in order;
//                         a key's rank among the wave's keys of its digit = the wave's LDS counter of that digit before the round +
//                         the number of lower lanes with the same digit (eight ballots: the lanes that agree with me on every digit
//                         bit).  After the rounds the counters hold the wave's histogram; a 256-thread step turns them into the
//                         wave's first destination per digit (the tile's, from the scan, plus the waves before it).  No atomics.
// Two index buffers in the workspace ping-pong (the first pass reads no buffer: position = item); the last launch copies the final
// one to `order`.  No kernel waits for another workgroup: every scan over workgroups is block sums / a one-workgroup scan of the
// sums / apply, as separate launches.  Every loop is bounded by an argument, every access checked against N, every offset 64-bit.
// Every output word is written once, without atomics: two calls give equal bytes, on any stream.
#pragma once

#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kBktMaxWords = 64;           // bits <= 2048: what cmh_pack_codes takes
constexpr int kSortTile = CMH_SORT_TILE;   // positions per workgroup of a pass
constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortRounds = kSortTile / kSortThreads;      // 64-position rounds of a wave, positions per thread
constexpr int kSortMaxPasses = 4 * kBktMaxWords;
constexpr int kScanBlock = 2048;           // elements per workgroup of the scans
constexpr int kScanPer = kScanBlock / 256;

static_assert(kSortTile == kSortThreads * kSortRounds && kSortTile / kSortWaves <= (1 << 24), "a rank shares a word with its 8-bit digit");

// src[p]: the buffer pass p reads (-1: none, position = item; 0 / 1: the workspace's buffers); skip[p]: pass p moves nothing
struct SortState {
  int src[kSortMaxPasses + 1];
  int skip[kSortMaxPasses];
};

struct SortArgs {
  const uint32_t* sign;
  int64_t N;
  int W, bits, T;                // words per row, code length, tiles
  int digit0;                    // pass p sorts by digit digit0 + p
  int32_t* buf[2];
  uint32_t* counts;              // [256][T], scanned in place
  SortState* state;
};

__device__ __forceinline__ uint32_t word_mask(int w, int bits) {
  const int rest = bits - 32 * w;
  return rest >= 32 ? 0xffffffffu : rest <= 0 ? 0u : ((1u << rest) - 1u);
}

__device__ __forceinline__ uint32_t key_word(const uint32_t* __restrict__ sign, int64_t item, int W, int w, int bits) {
  return sign[static_cast<size_t>(item) * W + w] & word_mask(w, bits);
}

// item at position pos of the pass's source (pos < N checked by the caller)
__device__ __forceinline__ int32_t sort_item(const SortArgs& a, int src, int64_t pos) {
  return src < 0 ? static_cast<int32_t>(pos) : a.buf[src][pos];
}

__device__ __forceinline__ uint32_t sort_digit(const SortArgs& a, int32_t item, int pass) {
  const int d = a.digit0 + pass;
  return (key_word(a.sign, item, a.W, d >> 2, a.bits) >> (8 * (d & 3))) & 0xffu;
}

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(SortArgs a, int pass) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int src = a.state->src[pass];
  hist[tid] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(tile) * kSortTile;
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const int64_t pos = base + r * kSortThreads + tid;
    if (pos < a.N) atomicAdd(&hist[sort_digit(a, sort_item(a, src, pos), pass)], 1u);      // LDS counters: an integer sum
  }
  __syncthreads();
  if (tile < a.T) a.counts[static_cast<size_t>(tid) * a.T + tile] = hist[tid];
}

// ---- exclusive / inclusive scan of a uint32 array over workgroups: sums, scan of the sums, apply --------------------------------
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// inclusive prefix of v over the 256 threads of the workgroup; *total = the sum.  wsum: 4 words of LDS
__device__ __forceinline__ uint32_t block_inclusive(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_inclusive(v, lane);
  __syncthreads();                        // (wsum may still be read from the caller's previous round)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = wsum[w];
    before += w < wave ? s : 0u;
    all += s;
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(256) void scan_block_sums_kernel(const uint32_t* __restrict__ data, int64_t n, uint32_t* __restrict__ sums,
                                                              int64_t nb) {
  __shared__ uint32_t wsum[4];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kScanBlock;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < n) v += data[i];
  }
  uint32_t total;
  block_inclusive(v, wsum, &total);
  if (threadIdx.x == 0 && blockIdx.x < nb) sums[blockIdx.x] = total;
}

// one workgroup: sums[nb] -> its exclusive scan in place; the total to *total64 (optional)
__global__ __launch_bounds__(256) void scan_sums_kernel(uint32_t* __restrict__ sums, int64_t nb, long long* __restrict__ total64) {
  __shared__ uint32_t wsum[4];
  uint32_t carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? sums[i] : 0u;
    uint32_t total;
    const uint32_t inc = block_inclusive(v, wsum, &total);
    if (i < nb) sums[i] = carry + inc - v;
    carry += total;
  }
  if (total64 && threadIdx.x == 0) *total64 = static_cast<long long>(carry);
}

template <bool INCLUSIVE>
__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* __restrict__ data, int64_t n, const uint32_t* __restrict__ sums,
                                                         int64_t nb) {
  __shared__ uint32_t wsum[4];
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kScanBlock + static_cast<int64_t>(threadIdx.x) * kScanPer;
  uint32_t e[kScanPer], v = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    e[j] = first + j < n ? data[first + j] : 0u;
    v += e[j];
  }
  uint32_t total;
  uint32_t run = block_inclusive(v, wsum, &total) - v + (blockIdx.x < nb ? sums[blockIdx.x] : 0u);
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    if (INCLUSIVE) run += e[j];
    if (first + j < n) data[first + j] = run;
    if (!INCLUSIVE) run += e[j];
  }
}

// after the scan: bin b starts at counts[b][0]; the pass is the identity iff every bin starts at 0 or at N
__global__ __launch_bounds__(256) void sort_decide_kernel(SortArgs a, int pass) {
  const uint32_t start = a.counts[static_cast<size_t>(threadIdx.x) * a.T];
  const int skip = __syncthreads_and(start == 0u || static_cast<int64_t>(start) == a.N);
  if (threadIdx.x == 0) {
    const int src = a.state->src[pass];
    a.state->skip[pass] = skip;
    a.state->src[pass + 1] = skip ? src : (src == 0 ? 1 : 0);
  }
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(SortArgs a, int pass) {
  __shared__ uint32_t cnt[kSortWaves][256];
  if (a.state->skip[pass]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int src = a.state->src[pass];
  int32_t* __restrict__ dst = a.buf[src == 0 ? 1 : 0];
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) cnt[w][tid] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(tile) * kSortTile + static_cast<int64_t>(wave) * (kSortTile / kSortWaves);
  const unsigned long long below = (1ull << lane) - 1ull;
  int32_t item[kSortRounds];
  uint32_t place[kSortRounds];            // rank among the wave's keys of the digit << 8 | digit
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const int64_t pos = base + r * 64 + lane;
    const bool live = pos < a.N;
    item[r] = live ? sort_item(a, src, pos) : 0;
    const uint32_t d = live ? sort_digit(a, item[r], pass) : 0u;
    unsigned long long same = __ballot(live);          // the live lanes with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long vote = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? vote : ~vote;
    }
    const uint32_t before = cnt[wave][d];              // every lane reads before the round's leaders write
    __builtin_amdgcn_wave_barrier();
    if (live && (same & below) == 0ull) cnt[wave][d] = before + static_cast<uint32_t>(__popcll(same));
    __builtin_amdgcn_wave_barrier();
    place[r] = ((before + static_cast<uint32_t>(__popcll(same & below))) << 8) | d;
  }
  __syncthreads();
  {                                                    // thread = digit: the waves' histograms -> their first destinations
    uint32_t run = tile < a.T ? a.counts[static_cast<size_t>(tid) * a.T + tile] : 0u;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
      const uint32_t c = cnt[w][tid];
      cnt[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const int64_t pos = base + r * 64 + lane;
    const int64_t to = static_cast<int64_t>(cnt[wave][place[r] & 0xffu]) + (place[r] >> 8);
    if (pos < a.N && to < a.N) dst[to] = item[r];
  }
}

__global__ __launch_bounds__(256) void sort_finish_kernel(SortArgs a, int passes, int32_t* __restrict__ order) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < a.N) order[i] = sort_item(a, a.state->src[passes], i);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// The workspace of a sort of N items: the state, two index buffers, the counters and the sums of the scans.  It does not depend on
// the number of passes.
struct SortPlan {
  int W, passes;
  int64_t T, n_counts, nb_counts, nb_items;
  size_t off_buf[2], off_counts, off_sums, bytes;
};

SortPlan sort_plan(int64_t N, int bits) {
  SortPlan p = {};
  p.W = (bits + 31) / 32;
  p.passes = (bits + 7) / 8;
  p.T = (N + kSortTile - 1) / kSortTile;
  p.n_counts = 256 * p.T;
  p.nb_counts = (p.n_counts + kScanBlock - 1) / kScanBlock;
  p.nb_items = (N + kScanBlock - 1) / kScanBlock;
  size_t at = align_up(sizeof(SortState), 256);
  for (int b = 0; b < 2; ++b) {
    p.off_buf[b] = at;
    at += align_up(static_cast<size_t>(N) * 4, 256);
  }
  p.off_counts = at;
  at += align_up(static_cast<size_t>(p.n_counts) * 4, 256);
  p.off_sums = at;                                     // the sums of the counts' scan, or of cmh_code_bucket_count's
  at += align_up(static_cast<size_t>(p.nb_counts > p.nb_items ? p.nb_counts : p.nb_items) * 4, 256);
  p.bytes = at + 256;                                  // + the slack of aligning the caller's pointer
  return p;
}

uint8_t* aligned_ws(void* workspace) {
  return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
}

// data[n] -> its scan in place (sums: nb words of scratch); total64 (optional) gets the sum
template <bool INCLUSIVE>
int launch_scan(uint32_t* data, int64_t n, uint32_t* sums, long long* total64, const char* what, hipStream_t st) {
  const int64_t nb = (n + kScanBlock - 1) / kScanBlock;
  hipLaunchKernelGGL(scan_block_sums_kernel, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, data, n, sums, nb);
  CMH_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, st, sums, nb, total64);
  CMH_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(scan_apply_kernel<INCLUSIVE>, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, data, n, sums, nb);
  CMH_CHECK_LAUNCH(what);
  return CMH_OK;
}

// One sort in the carved workspace `ws` (aligned_ws of a buffer of sort_plan(N, bits).bytes): `passes` passes over the digits
// digit0, digit0 + 1, ... of the rows of `sign`, from position = item, and the final buffer copied to order[N].  `what` names the
// caller in a launch error.
int run_sort(const char* what, const uint32_t* sign, int64_t N, int bits, int digit0, int passes, const SortPlan& p, uint8_t* ws,
             int32_t* order, hipStream_t st) {
  SortArgs a = {};
  a.sign = sign; a.N = N; a.W = p.W; a.bits = bits; a.T = static_cast<int>(p.T); a.digit0 = digit0;
  a.buf[0] = reinterpret_cast<int32_t*>(ws + p.off_buf[0]);
  a.buf[1] = reinterpret_cast<int32_t*>(ws + p.off_buf[1]);
  a.counts = reinterpret_cast<uint32_t*>(ws + p.off_counts);
  a.state = reinterpret_cast<SortState*>(ws);
  uint32_t* sums = reinterpret_cast<uint32_t*>(ws + p.off_sums);
  char stage[96];
  auto named = [&](const char* name) -> const char* {
    snprintf(stage, sizeof stage, "%s (%s)", what, name);
    return stage;
  };
  if (hipMemsetAsync(&a.state->src[0], 0xff, sizeof(int), st) != hipSuccess) {      // src[0] = -1: the first pass reads no buffer
    (void)hipGetLastError();
    return fail(CMH_ERR_LAUNCH, "%s: setting the workspace failed", what);
  }
  const dim3 tiles(static_cast<unsigned>(p.T));
  for (int pass = 0; pass < passes; ++pass) {
    hipLaunchKernelGGL(sort_hist_kernel, tiles, dim3(kSortThreads), 0, st, a, pass);
    CMH_CHECK_LAUNCH(named("histogram"));
    const int s = launch_scan<false>(a.counts, p.n_counts, sums, nullptr, named("scan"), st);
    if (s != CMH_OK) return s;
    hipLaunchKernelGGL(sort_decide_kernel, dim3(1), dim3(256), 0, st, a, pass);
    CMH_CHECK_LAUNCH(named("decide"));
    hipLaunchKernelGGL(sort_scatter_kernel, tiles, dim3(kSortThreads), 0, st, a, pass);
    CMH_CHECK_LAUNCH(named("scatter"));
  }
  hipLaunchKernelGGL(sort_finish_kernel, dim3(static_cast<unsigned>((N + 255) / 256)), dim3(256), 0, st, a, passes, order);
  CMH_CHECK_LAUNCH(named("finish"));
  return CMH_OK;
}

}  // namespace
}  // namespace cmh
