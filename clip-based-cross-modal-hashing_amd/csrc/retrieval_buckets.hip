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
// key: no pass).  A pass is, over tiles of kSortTile positions of the current index buffer,
//   sort_hist_kernel      counts[bin][tile]: per-tile digit histogram (LDS counters), stored bin-major, so that
//   scan (three launches) ONE exclusive scan of the flat array is, at [bin][tile], the first destination of the tile's keys of that bin
//   sort_decide_kernel    all N keys in one bin?  Then the pass would be the identity permutation: it is skipped, and the next pass
//                         reads the same buffer.  Writes skip[pass] and src[pass + 1] in the workspace; the host reads nothing
//   sort_scatter_kernel   the stable scatter.  A wave owns kSortTile / 4 consecutive positions and takes them 64 at a time in order;
//                         a key's rank among the wave's keys of its digit = the wave's LDS counter of that digit before the round +
//                         the number of lower lanes with the same digit (eight ballots: the lanes that agree with me on every digit
//                         bit).  After the rounds the counters hold the wave's histogram; a 256-thread step turns them into the
//                         wave's first destination per digit (the tile's, from the scan, plus the waves before it).  No atomics.
// Two index buffers in the workspace ping-pong (the first pass reads no buffer: position = item); cmh_code_sort's last launch copies
// the final one to `order`.  No kernel waits for another workgroup: every scan over workgroups is block sums / a one-workgroup scan
// of the sums / apply, as separate launches.  Every loop is bounded by an argument, every access checked against N, U or Q, every
// offset 64-bit.  Every output word is written once, without atomics: two calls give equal bytes, on any stream.
//
// The probes.  A query has P = 1 + bits + bits (bits - 1) / 2 candidate keys within radius 2: itself, one flipped bit i ascending,
// pairs (i, j), i < j, in lexicographic order (radius 0 / 1: the first 1 / 1 + bits of them).  One workgroup owns a query and takes
// its probes kProbeThreads at a time in probe order; a thread builds its key (a pair is unranked from the probe's number), finds it by one
// binary search over codes (<= 32 steps, word W - 1 first), and a hit's place in the query's list is the hits of the rounds before
// + the hits of the waves before it in this round (LDS) + the hits of the lower lanes (ballot): the list is in probe order on every
// run.  Distinct probes are distinct keys, so a bucket is hit at most once per query.  The count pass and the fill pass both
// search; nothing per probe is stored.
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
constexpr int kProbeThreads = 1024;
constexpr int kProbeWaves = kProbeThreads / 64;
constexpr int kProbeWords = CMH_BUCKET_BITS_MAX / 32;

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
  return (key_word(a.sign, item, a.W, pass >> 2, a.bits) >> (8 * (pass & 3))) & 0xffu;
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
  uint8_t* ws = aligned_ws(workspace);
  SortArgs a = {};
  a.sign = sign; a.N = N; a.W = p.W; a.bits = bits; a.T = static_cast<int>(p.T);
  a.buf[0] = reinterpret_cast<int32_t*>(ws + p.off_buf[0]);
  a.buf[1] = reinterpret_cast<int32_t*>(ws + p.off_buf[1]);
  a.counts = reinterpret_cast<uint32_t*>(ws + p.off_counts);
  a.state = reinterpret_cast<SortState*>(ws);
  uint32_t* sums = reinterpret_cast<uint32_t*>(ws + p.off_sums);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(&a.state->src[0], 0xff, sizeof(int), st) != hipSuccess) {      // src[0] = -1: the first pass reads no buffer
    (void)hipGetLastError();
    return fail(CMH_ERR_LAUNCH, "code_sort: setting the workspace failed");
  }
  const dim3 tiles(static_cast<unsigned>(p.T));
  for (int pass = 0; pass < p.passes; ++pass) {
    hipLaunchKernelGGL(sort_hist_kernel, tiles, dim3(kSortThreads), 0, st, a, pass);
    CMH_CHECK_LAUNCH("code_sort (histogram)");
    const int s = launch_scan<false>(a.counts, p.n_counts, sums, nullptr, "code_sort (scan)", st);
    if (s != CMH_OK) return s;
    hipLaunchKernelGGL(sort_decide_kernel, dim3(1), dim3(256), 0, st, a, pass);
    CMH_CHECK_LAUNCH("code_sort (decide)");
    hipLaunchKernelGGL(sort_scatter_kernel, tiles, dim3(kSortThreads), 0, st, a, pass);
    CMH_CHECK_LAUNCH("code_sort (scatter)");
  }
  hipLaunchKernelGGL(sort_finish_kernel, dim3(static_cast<unsigned>((N + 255) / 256)), dim3(256), 0, st, a, p.passes, order);
  CMH_CHECK_LAUNCH("code_sort (finish)");
  return CMH_OK;
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
