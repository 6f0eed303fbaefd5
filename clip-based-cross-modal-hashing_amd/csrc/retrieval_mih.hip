// Radius search past 2 bits by multi-index hashing on 16-bit substrings (Norouzi, Punjani, Fleet 2012).
//   cmh_mih_build           order[m, N] and starts[m, 65537]: per substring the item indices by ascending (key, index) and the
//                           first position of every key: m direct-addressed tables, no search at lookup time
//   cmh_mih_count / _fill   per query every item within `radius` whole bits, each exactly once
//   cmh_mih_knn_count / _fill   per query the smallest radius whose ball holds k items, found by growing it, and that ball
//
// Codes are in {-1, +1} (the caller checks; no entry point reads an nz plane) and at most 128 bit.  m = ceil(bits / 16); SUBSTRING j
// is bits [16 j, 16 j + s_j) of a row's sign words, s_j = 16 but for a shorter last one, and its KEY those bits as an unsigned
// integer.  For a radius r let a, b = divmod(r, m): substring j is probed at radius a_j = a for j <= b and a - 1 behind (-1: not
// probed).  If every probed j had d_j > a_j, then d >= (b + 1)(a + 1) + (m - b - 1) a = m a + b + 1 > r: an item within r is in a
// probed bucket of some substring.  a <= CMH_MIH_SUB_RADIUS_MAX, so r <= 3 m - 1.
//
// The build.  Key j is digits 2 j and 2 j + 1 of the row in the terms of retrieval_sort.h (the bits at and behind `bits` are
// cleared there, which is the short last substring): table j is that file's stable sort over those two digits from position =
// item, so equal keys keep ascending index.  starts is a per-key lower bound over the sorted keys (<= 32 steps per key).
//
// The lookup.  The PROBES of substring j are the query's key with at most a_j of its s_j bits flipped: none, single bits ascending,
// pairs (i, i'), i < i', in lexicographic order; distinct probes are distinct keys.  A query's probes over all substrings are
// numbered in (substring, probe) order.  One workgroup of 256 threads owns a query and takes its probes 256 at a time: a thread
// reads its probe's bucket bounds, and the inclusive prefix of the bucket lengths (LDS) makes the round's buckets ONE list of
// candidates in (substring, probe, bucket position) order.  The workgroup walks that list 256 candidates at a time, whatever the
// lengths of the buckets behind it: a thread finds its candidate's probe by a binary search over the 256 prefixes, reads the item
// from `order`, checks it against N, loads its row and verifies.
// EXACTLY ONCE: item x reached through substring j is emitted iff d(q, x) <= r and no probed j' < j has d_j'(q, x) <= a_j' (x is
// then emitted through the first such j').  The d_j' are popcounts on the row that the verification loaded: no visited set, no
// hash, no atomics.  A hit's place in the query's list is the hits of the steps before + of the waves before it in this step (LDS)
// + of the lower lanes (ballot).  The count pass and the fill pass walk identically; nothing per candidate is stored.  The list is
// in walk order on every run; the caller sorts it by (distance, index).
// No kernel waits for another workgroup.  Every loop is bounded by an argument (a bucket's bounds are clamped to [0, N]), every
// offset is 64-bit, every index read out of a table is checked against N before it addresses anything, every output word is
// written once.
//
// k nearest by growing the radius.  GROWTH STEP s = t m + j (t = 0, 1, 2; j < m) probes substring j at EXACTLY level t: the keys
// that are the query's with exactly t of the s_j bits flipped, in the order above (1, s_j or s_j (s_j - 1) / 2 probes, at most
// 120: one step is one round of the workgroup).  After steps 0 .. r the substrings have been probed at the radii a_j of radius r,
// so every item within r has been reached (the pigeonhole argument above).  Item x is FIRST REACHED at step f(x) = min_j (d_j m +
// j); the minimum is unique, the j being distinct below m.  A candidate reached through (j, t = d_j) counts, or is emitted, iff
// f(x) = t m + j, that is d_j' m + j' > t m + j for every j' != j: popcounts on the row the verification loaded.  An item within r
// has f(x) <= r, so after step r the numbers of first-reached items at every distance d <= r are complete, and the STOPPING
// RADIUS r*(q) = the smallest r <= r_cap with |ball(q, r)| >= k is decided after step r* with no second look at anything
// (mih_knn_sub / mih_knn_level below are the step's two halves; utils.retrieval.knn_steps restates them on the host).  The count pass keeps the per-distance
// numbers in LDS (d <= r_cap <= 23) and stops, workgroup-uniformly, at r*; the fill pass walks steps 0 .. radius[q] again and
// emits the first-reached items with d <= radius[q] at the place mih_kernel computes.
#include "retrieval_sort.h"

namespace cmh {
namespace {

constexpr int kMihSub = CMH_MIH_SUB_BITS;
constexpr int kMihKeys = 1 << kMihSub;
constexpr int kMihMaxSubs = CMH_BUCKET_BITS_MAX / kMihSub;
constexpr int kMihThreads = 256;
constexpr int kMihWaves = kMihThreads / 64;

static_assert(kMihSub == 16, "a key is two 8-bit digits of the sort");

__host__ __device__ __forceinline__ int mih_subs(int bits) { return (bits + kMihSub - 1) / kMihSub; }
__host__ __device__ __forceinline__ int mih_sub_bits(int bits, int j) { return bits - kMihSub * j < kMihSub ? bits - kMihSub * j : kMihSub; }

// ---- build --------------------------------------------------------------------------------------------------------------------
// starts[j][key] = the first position of row j of order whose key is not below `key`; starts[j][65536] = N
__global__ __launch_bounds__(256) void mih_starts_kernel(const uint32_t* __restrict__ sign, const int32_t* __restrict__ order, int64_t N,
                                                         int W, int bits, int32_t* __restrict__ starts) {
  const int key = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (key > kMihKeys) return;
  const int32_t* __restrict__ row = order + static_cast<size_t>(j) * N;
  int64_t lo = 0, hi = N;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int64_t item = row[mid];
    const bool legal = item >= 0 && item < N;           // (not a row of cmh_mih_build: nothing is read outside the plane)
    const uint32_t k = legal ? (key_word(sign, item, W, j >> 1, bits) >> (kMihSub * (j & 1))) & 0xffffu : 0xffffffffu;
    if (k < static_cast<uint32_t>(key)) lo = mid + 1; else hi = mid;
  }
  starts[static_cast<size_t>(j) * (kMihKeys + 1) + key] = static_cast<int32_t>(lo);
}

// ---- lookup -------------------------------------------------------------------------------------------------------------------
struct MihArgs {
  const uint32_t* q_sign;
  const uint32_t* db_sign;
  const int32_t* order;          // [m, N]
  const int32_t* starts;         // [m, 65537]
  int64_t N;
  int Q, bits, radius, m, probes;
  int sub_radius[kMihMaxSubs];   // a_j; -1 = not probed
  int first[kMihMaxSubs + 1];    // the probes of the substrings before j
  int32_t* n_hits;               // count pass
  const long long* offsets;      // fill pass: [Q + 1]
  int64_t capacity;
  int32_t* idx;
  int32_t* dist;
};

// inclusive prefix of v over the 256 threads of the workgroup.  wsum: kMihWaves words of LDS
__device__ __forceinline__ unsigned long long block_inclusive64(unsigned long long v, unsigned long long* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  __syncthreads();                        // (wsum, and the caller's LDS, may still be read from the previous round)
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kMihWaves; ++w) v += w < wave ? wsum[w] : 0ull;
  return v;
}

// the key of substring j (s bits) of a row whose masked words are qw
template <int W>
__device__ __forceinline__ uint32_t mih_key(const uint32_t (&qw)[W], int j, int s) {
  uint32_t word = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) word = (j >> 1) == w ? qw[w] : word;
  return (word >> (kMihSub * (j & 1))) & ((1u << s) - 1u);
}

// probe number t of a key of s bits: 0 = the key, 1 .. s = single bits ascending, behind them the pairs (i, i'), i < i' < s, in
// lexicographic order.  false: there is no such probe
__device__ __forceinline__ bool mih_probe_key(uint32_t& key, int s, int t) {
  if (t >= 1 && t <= s) {
    key ^= 1u << (t - 1);
  } else if (t > s) {                                  // pair number t - 1 - s
    t -= 1 + s;
    int i = 0;
    for (int row = 0; row < kMihSub - 1 && row < s - 1 && t >= s - 1 - row; ++row) {
      t -= s - 1 - row;
      i = row + 1;
    }
    const int i2 = i + 1 + t;
    if (i2 >= s) return false;
    key ^= (1u << i) ^ (1u << i2);
  }
  return true;
}

// bucket `key` of table j: its length and first position in order (row j included); the bounds are clamped to [0, N]
__device__ __forceinline__ void mih_bucket(const int32_t* __restrict__ starts, int j, uint32_t key, int64_t N, unsigned long long& len,
                                           long long& at) {
  const int32_t* bounds = starts + static_cast<size_t>(j) * (kMihKeys + 1) + key;
  int64_t lo = bounds[0], hi = bounds[1];
  lo = lo < 0 ? 0 : lo > N ? N : lo;
  hi = hi < lo ? lo : hi > N ? N : hi;
  len = static_cast<unsigned long long>(hi - lo);
  at = static_cast<long long>(j) * N + lo;
}

// row `item` of the database with one load
template <int W>
__device__ __forceinline__ void mih_load_row(const uint32_t* __restrict__ db_sign, int64_t item, uint32_t (&x)[W]) {
  const uint32_t* row = db_sign + static_cast<size_t>(item) * W;
  if constexpr (W == 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(row);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else if constexpr (W == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(row);
    x[0] = v.x; x[1] = v.y;
  } else {
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = row[w];
  }
}

// the substring of probe p (p < a.probes: the unprobed substrings lie behind the probed ones and own no probe)
__device__ __forceinline__ int mih_sub_of(const MihArgs& a, int p) {
  int j = 0;
#pragma unroll
  for (int jj = 1; jj < kMihMaxSubs; ++jj) j = (jj < a.m && p >= a.first[jj]) ? jj : j;
  return j;
}

template <bool FILL, int W>
__global__ __launch_bounds__(kMihThreads) void mih_kernel(MihArgs a) {
  __shared__ unsigned long long incl[kMihThreads];     // the round's bucket lengths, inclusive prefix
  __shared__ long long begin[kMihThreads];             // the round's buckets: first position in order (row j included)
  __shared__ unsigned long long wsum[kMihWaves];
  __shared__ uint32_t wave_hits[kMihWaves];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (q >= a.Q) return;
  uint32_t qw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) qw[w] = a.q_sign[static_cast<size_t>(q) * W + w] & word_mask(w, a.bits);
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t done = 0;                                    // hits of the steps before this one
  int64_t list_lo = 0, list_hi = 0;
  if (FILL) {
    list_lo = a.offsets[q];
    list_hi = a.offsets[q + 1] < a.capacity ? a.offsets[q + 1] : a.capacity;
  }
  for (int first = 0; first < a.probes; first += kMihThreads) {
    const int p = first + tid;
    unsigned long long len = 0;
    long long at = 0;
    if (p < a.probes) {
      const int j = mih_sub_of(a, p), s = mih_sub_bits(a.bits, j);
      uint32_t key = mih_key<W>(qw, j, s);
      if (mih_probe_key(key, s, p - a.first[j])) mih_bucket(a.starts, j, key, a.N, len, at);
    }
    const unsigned long long inc = block_inclusive64(len, wsum);
    incl[tid] = inc;
    begin[tid] = at;
    __syncthreads();
    const unsigned long long total = incl[kMihThreads - 1];
    for (unsigned long long c0 = 0; c0 < total; c0 += kMihThreads) {
      const unsigned long long c = c0 + tid;
      bool hit = false;
      int64_t item = 0;
      int d = 0;
      if (c < total) {
        int lo = 0, hi = kMihThreads - 1;              // the first slot whose inclusive prefix is above c
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int mid = (lo + hi) >> 1;
          if (incl[mid] > c) hi = mid; else lo = mid + 1;
        }
        const unsigned long long before = lo ? incl[lo - 1] : 0ull;
        const int j = mih_sub_of(a, first + lo);
        item = a.order[begin[lo] + static_cast<long long>(c - before)];
        if (item >= 0 && item < a.N) {
          uint32_t x[W];
          mih_load_row<W>(a.db_sign, item, x);
          bool earlier = false;                        // a probed substring before j reaches the item: emitted there
#pragma unroll
          for (int w = 0; w < W; ++w) {
            x[w] = (x[w] ^ qw[w]) & word_mask(w, a.bits);
            d += __popc(x[w]);
            earlier = earlier || (2 * w < j && a.sub_radius[2 * w] >= 0 && __popc(x[w] & 0xffffu) <= a.sub_radius[2 * w]);
            earlier = earlier || (2 * w + 1 < j && a.sub_radius[2 * w + 1] >= 0 && __popc(x[w] >> kMihSub) <= a.sub_radius[2 * w + 1]);
          }
          hit = d <= a.radius && !earlier;
        }
      }
      const unsigned long long votes = __ballot(hit);
      __syncthreads();                                 // (the previous step's wave_hits are read)
      if (lane == 0) wave_hits[wave] = static_cast<uint32_t>(__popcll(votes));
      __syncthreads();
      uint32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < kMihWaves; ++w) {
        const uint32_t h = wave_hits[w];
        before += w < wave ? h : 0u;
        all += h;
      }
      if (FILL && hit) {
        const int64_t to = list_lo + done + before + __popcll(votes & below);
        if (to >= list_lo && to < list_hi) {
          a.idx[to] = static_cast<int32_t>(item);
          a.dist[to] = d;
        }
      }
      done += all;
    }
  }
  if (!FILL && tid == 0) a.n_hits[q] = static_cast<int32_t>(done);
}

// ---- k nearest: the radius grown per query ----------------------------------------------------------------------------------------
constexpr int kMihKnnProbes = 128;                                             // a step's probes: at most 16 * 15 / 2 = 120
constexpr int kMihKnnDists = (CMH_MIH_SUB_RADIUS_MAX + 1) * kMihMaxSubs;       // the distances 0 .. r_cap <= 23

static_assert(kMihSub * (kMihSub - 1) / 2 <= kMihKnnProbes && kMihKnnProbes <= kMihThreads, "one growth step is one round");

// growth step s of a code of m substrings -> (substring, level): the rule, stated once for the kernel and the host
__host__ __device__ __forceinline__ int mih_knn_sub(int s, int m) { return s % m; }
__host__ __device__ __forceinline__ int mih_knn_level(int s, int m) { return s / m; }

struct MihKnnArgs {
  const uint32_t* q_sign;
  const uint32_t* db_sign;
  const int32_t* order;          // [m, N]
  const int32_t* starts;         // [m, 65537]
  int64_t N;
  int Q, bits, m, k, r_cap;
  int32_t* radius;               // count pass: r*, or -1
  int32_t* n_ball;
  int32_t* n_less;
  const int32_t* walk_radius;    // fill pass: the radius of every query (< 0 or above 3 m - 1: nothing is walked)
  const long long* offsets;      //            [Q + 1]
  int64_t capacity;
  int32_t* idx;
  int32_t* dist;
};

template <bool FILL, int W>
__global__ __launch_bounds__(kMihThreads) void mih_knn_kernel(MihKnnArgs a) {
  __shared__ unsigned long long incl[kMihKnnProbes];   // the step's bucket lengths, inclusive prefix
  __shared__ long long begin[kMihKnnProbes];           // the step's buckets: first position in order (row j included)
  __shared__ unsigned long long wsum[kMihWaves];
  __shared__ uint32_t wave_hits[kMihWaves];            // fill pass
  __shared__ uint32_t at_dist[kMihKnnDists];           // count pass: the first-reached items at every distance d <= r_cap
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (q >= a.Q) return;
  const int top = (CMH_MIH_SUB_RADIUS_MAX + 1) * a.m - 1;
  int last = a.r_cap;                                  // the last step: never beyond 3 m - 1, whatever an operand says
  if (FILL) {
    last = a.walk_radius[q];
    if (last < 0 || last > top) return;                // (uniform: one query per workgroup)
  }
  last = last < top ? last : top;
  uint32_t qw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) qw[w] = a.q_sign[static_cast<size_t>(q) * W + w] & word_mask(w, a.bits);
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t done = 0;                                    // fill: hits of the steps before this one
  int64_t list_lo = 0, list_hi = 0;
  if (FILL) {
    list_lo = a.offsets[q];
    list_hi = a.offsets[q + 1] < a.capacity ? a.offsets[q + 1] : a.capacity;
  } else if (tid < kMihKnnDists) {
    at_dist[tid] = 0u;                                 // (block_inclusive64 synchronises before the first candidate)
  }
  int64_t ball = 0, less = 0;                          // count: |ball(step)|, |ball(step - 1)|
  int found = -1;
  for (int step = 0; step <= last; ++step) {
    const int j = mih_knn_sub(step, a.m), t = mih_knn_level(step, a.m), s = mih_sub_bits(a.bits, j);
    const int probes = t == 0 ? 1 : t == 1 ? s : s * (s - 1) / 2;
    unsigned long long len = 0;
    long long at = 0;
    if (tid < probes) {
      uint32_t key = mih_key<W>(qw, j, s);             // probe tid of level t is probe tid + (the probes of the levels below) of the key
      if (mih_probe_key(key, s, tid + (t == 0 ? 0 : t == 1 ? 1 : 1 + s))) mih_bucket(a.starts, j, key, a.N, len, at);
    }
    const unsigned long long inc = block_inclusive64(len, wsum);
    if (tid < kMihKnnProbes) {
      incl[tid] = inc;
      begin[tid] = at;
    }
    __syncthreads();
    const unsigned long long total = incl[kMihKnnProbes - 1];
    for (unsigned long long c0 = 0; c0 < total; c0 += kMihThreads) {
      const unsigned long long c = c0 + tid;
      bool hit = false;
      int64_t item = 0;
      int d = 0;
      if (c < total) {
        int lo = 0, hi = kMihKnnProbes - 1;            // the first slot whose inclusive prefix is above c
#pragma unroll
        for (int b = 0; b < 7; ++b) {
          const int mid = (lo + hi) >> 1;
          if (incl[mid] > c) hi = mid; else lo = mid + 1;
        }
        const unsigned long long before = lo ? incl[lo - 1] : 0ull;
        item = a.order[begin[lo] + static_cast<long long>(c - before)];
        if (item >= 0 && item < a.N) {
          uint32_t x[W];
          mih_load_row<W>(a.db_sign, item, x);
          int reached = 0x7fffffff;                    // f(x) = min_j' (d_j' m + j')
#pragma unroll
          for (int w = 0; w < W; ++w) {
            x[w] = (x[w] ^ qw[w]) & word_mask(w, a.bits);
            d += __popc(x[w]);
            const int f0 = __popc(x[w] & 0xffffu) * a.m + 2 * w, f1 = __popc(x[w] >> kMihSub) * a.m + 2 * w + 1;
            reached = 2 * w < a.m && f0 < reached ? f0 : reached;
            reached = 2 * w + 1 < a.m && f1 < reached ? f1 : reached;
          }
          hit = reached == step && d <= last;          // first reached here; (count: last = r_cap, d indexes at_dist)
        }
      }
      if (!FILL) {
        if (hit) atomicAdd(&at_dist[d], 1u);           // (LDS; integer sums: any order gives the same words)
      } else {
        const unsigned long long votes = __ballot(hit);
        __syncthreads();                               // (the previous round's wave_hits are read)
        if (lane == 0) wave_hits[wave] = static_cast<uint32_t>(__popcll(votes));
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kMihWaves; ++w) {
          const uint32_t h = wave_hits[w];
          before += w < wave ? h : 0u;
          all += h;
        }
        if (hit) {
          const int64_t to = list_lo + done + before + __popcll(votes & below);
          if (to >= list_lo && to < list_hi) {
            a.idx[to] = static_cast<int32_t>(item);
            a.dist[to] = d;
          }
        }
        done += all;
      }
    }
    if (!FILL) {
      __syncthreads();                                 // the step's candidates are counted: at_dist[d] is complete for d <= step
      less = ball;
      ball += at_dist[step];                           // one word, the same in every thread: the decision is uniform
      if (ball >= a.k) {                               // (the next write of at_dist lies behind block_inclusive64's barrier)
        found = step;
        break;
      }
    }
  }
  if (!FILL && tid == 0) {
    a.radius[q] = found;
    a.n_ball[q] = static_cast<int32_t>(ball);
    a.n_less[q] = static_cast<int32_t>(found < 0 ? ball : less);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int mih_probes_of(int s, int radius) { return radius < 0 ? 0 : radius == 0 ? 1 : radius == 1 ? 1 + s : 1 + s + s * (s - 1) / 2; }

int check_mih_table(const char* what, int64_t N, int bits) {
  CMH_CHECK_ARG(N >= 1 && N <= 2147483647ll, "%s: N=%lld outside [1, 2^31 - 1]", what, static_cast<long long>(N));
  CMH_CHECK_ARG(bits >= 1 && bits <= CMH_BUCKET_BITS_MAX, "%s: bits=%d outside [1, %d]", what, bits, CMH_BUCKET_BITS_MAX);
  return CMH_OK;
}

int check_mih_queries(const char* what, int Q, int64_t N, int bits) {
  CMH_CHECK_ARG(Q >= 1 && Q <= 65535, "%s: Q=%d outside [1, 65535]", what, Q);
  return check_mih_table(what, N, bits);
}

int check_mih_rows(const char* what, const uint32_t* db_sign, int bits) {
  const int W = (bits + 31) / 32;
  const uintptr_t row = W == 4 ? 16 : W == 2 ? 8 : 4;      // a row is read with one load
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(db_sign) % row == 0, "%s: db_sign holds rows of %d words: aligned to %d bytes", what, W,
                static_cast<int>(row));
  return CMH_OK;
}

// the shape checks of a lookup, then the call's arguments: the substring radii and the numbering of the probes
int mih_args(const char* what, const uint32_t* q_sign, int Q, const uint32_t* db_sign, int64_t N, int bits, int radius,
             const int32_t* order, const int32_t* starts, MihArgs* a) {
  int rc = check_mih_queries(what, Q, N, bits);
  if (rc != CMH_OK) return rc;
  const int m = mih_subs(bits);
  CMH_CHECK_ARG(radius >= 0 && radius <= (CMH_MIH_SUB_RADIUS_MAX + 1) * m - 1,
                "%s: radius=%d outside [0, %d] (%d substrings of %d bits, each probed within %d)", what, radius,
                (CMH_MIH_SUB_RADIUS_MAX + 1) * m - 1, m, CMH_MIH_SUB_BITS, CMH_MIH_SUB_RADIUS_MAX);
  rc = check_mih_rows(what, db_sign, bits);
  if (rc != CMH_OK) return rc;
  *a = MihArgs{};
  a->q_sign = q_sign; a->db_sign = db_sign; a->order = order; a->starts = starts;
  a->N = N; a->Q = Q; a->bits = bits; a->radius = radius; a->m = m;
  const int each = radius / m, more = radius % m;
  int probes = 0;
  for (int j = 0; j < kMihMaxSubs; ++j) {
    a->sub_radius[j] = j >= m ? -1 : j <= more ? each : each - 1;
    a->first[j] = probes;
    if (j < m) probes += mih_probes_of(mih_sub_bits(bits, j), a->sub_radius[j]);
  }
  a->first[kMihMaxSubs] = probes;
  a->probes = probes;
  return CMH_OK;
}

template <bool FILL>
void launch_mih(const MihArgs& a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(a.Q)), block(kMihThreads);
  switch ((a.bits + 31) / 32) {
    case 1: hipLaunchKernelGGL((mih_kernel<FILL, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((mih_kernel<FILL, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((mih_kernel<FILL, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((mih_kernel<FILL, 4>), grid, block, 0, st, a); break;
  }
}

// the shape checks of the k-nearest passes (r_cap < 0: the fill pass, which takes its radii per query), then the call's arguments
int mih_knn_args(const char* what, const uint32_t* q_sign, int Q, const uint32_t* db_sign, int64_t N, int bits, int64_t k, int r_cap,
                 const int32_t* order, const int32_t* starts, MihKnnArgs* a) {
  int rc = check_mih_queries(what, Q, N, bits);
  if (rc != CMH_OK) return rc;
  const int m = mih_subs(bits);
  if (r_cap >= 0) {
    CMH_CHECK_ARG(k >= 1 && k <= N, "%s: k=%lld outside [1, N=%lld]", what, static_cast<long long>(k), static_cast<long long>(N));
    CMH_CHECK_ARG(r_cap <= (CMH_MIH_SUB_RADIUS_MAX + 1) * m - 1,
                  "%s: r_cap=%d outside [0, %d] (%d substrings of %d bits, each probed within %d)", what, r_cap,
                  (CMH_MIH_SUB_RADIUS_MAX + 1) * m - 1, m, CMH_MIH_SUB_BITS, CMH_MIH_SUB_RADIUS_MAX);
  }
  rc = check_mih_rows(what, db_sign, bits);
  if (rc != CMH_OK) return rc;
  *a = MihKnnArgs{};
  a->q_sign = q_sign; a->db_sign = db_sign; a->order = order; a->starts = starts;
  a->N = N; a->Q = Q; a->bits = bits; a->m = m; a->k = static_cast<int>(k); a->r_cap = r_cap;
  return CMH_OK;
}

template <bool FILL>
void launch_mih_knn(const MihKnnArgs& a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(a.Q)), block(kMihThreads);
  switch ((a.bits + 31) / 32) {
    case 1: hipLaunchKernelGGL((mih_knn_kernel<FILL, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((mih_knn_kernel<FILL, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((mih_knn_kernel<FILL, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((mih_knn_kernel<FILL, 4>), grid, block, 0, st, a); break;
  }
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_mih_build_workspace_bytes(int64_t N, int32_t bits) {
  return N >= 1 && N <= 2147483647ll && bits >= 1 && bits <= CMH_BUCKET_BITS_MAX ? sort_plan(N, bits).bytes : 0;
}

extern "C" int cmh_mih_build(const uint32_t* sign, int64_t N, int32_t bits, int32_t* order, int32_t* starts, void* workspace,
                             size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(sign && order && starts, "mih_build: null pointer");
  const int rc = check_mih_table("mih_build", N, bits);
  if (rc != CMH_OK) return rc;
  const SortPlan p = sort_plan(N, bits);
  if (!workspace || workspace_bytes < p.bytes) return fail(CMH_ERR_WORKSPACE, "mih_build: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
  uint8_t* ws = aligned_ws(workspace);
  hipStream_t st = as_stream(stream);
  const int m = mih_subs(bits);
  for (int j = 0; j < m; ++j) {
    const int s = run_sort("mih_build", sign, N, bits, 2 * j, (mih_sub_bits(bits, j) + 7) / 8, p, ws, order + static_cast<size_t>(j) * N, st);
    if (s != CMH_OK) return s;
  }
  hipLaunchKernelGGL(mih_starts_kernel, dim3(kMihKeys / 256 + 1, m), dim3(256), 0, st, sign, order, N, p.W, bits, starts);
  CMH_CHECK_LAUNCH("mih_build (starts)");
  return CMH_OK;
}

extern "C" int cmh_mih_count(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t radius,
                             const int32_t* order, const int32_t* starts, int32_t* n_hits, void* stream) {
  CMH_CHECK_ARG(q_sign && db_sign && order && starts && n_hits, "mih_count: null pointer");
  MihArgs a;
  const int rc = mih_args("mih_count", q_sign, Q, db_sign, N, bits, radius, order, starts, &a);
  if (rc != CMH_OK) return rc;
  a.n_hits = n_hits;
  launch_mih<false>(a, as_stream(stream));
  CMH_CHECK_LAUNCH("mih_count");
  return CMH_OK;
}

extern "C" int cmh_mih_fill(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t radius,
                            const int32_t* order, const int32_t* starts, const int64_t* offsets, int64_t capacity, int32_t* idx,
                            int32_t* dist, void* stream) {
  CMH_CHECK_ARG(q_sign && db_sign && order && starts && offsets && idx && dist, "mih_fill: null pointer");
  MihArgs a;
  CMH_CHECK_ARG(capacity >= 1, "mih_fill: capacity=%lld below 1 (no hits: no call)", static_cast<long long>(capacity));
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0, "mih_fill: offsets holds 64-bit integers: aligned to 8 bytes");
  const int rc = mih_args("mih_fill", q_sign, Q, db_sign, N, bits, radius, order, starts, &a);
  if (rc != CMH_OK) return rc;
  a.offsets = reinterpret_cast<const long long*>(offsets); a.capacity = capacity; a.idx = idx; a.dist = dist;
  launch_mih<true>(a, as_stream(stream));
  CMH_CHECK_LAUNCH("mih_fill");
  return CMH_OK;
}

extern "C" int cmh_mih_knn_count(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits, int32_t k,
                                 int32_t r_cap, const int32_t* order, const int32_t* starts, int32_t* radius, int32_t* n_ball,
                                 int32_t* n_less, void* stream) {
  CMH_CHECK_ARG(q_sign && db_sign && order && starts && radius && n_ball && n_less, "mih_knn_count: null pointer");
  CMH_CHECK_ARG(r_cap >= 0, "mih_knn_count: r_cap=%d below 0", r_cap);
  MihKnnArgs a;
  const int rc = mih_knn_args("mih_knn_count", q_sign, Q, db_sign, N, bits, k, r_cap, order, starts, &a);
  if (rc != CMH_OK) return rc;
  a.radius = radius; a.n_ball = n_ball; a.n_less = n_less;
  launch_mih_knn<false>(a, as_stream(stream));
  CMH_CHECK_LAUNCH("mih_knn_count");
  return CMH_OK;
}

extern "C" int cmh_mih_knn_fill(const uint32_t* q_sign, int32_t Q, const uint32_t* db_sign, int64_t N, int32_t bits,
                                const int32_t* radius, const int32_t* order, const int32_t* starts, const int64_t* offsets,
                                int64_t capacity, int32_t* idx, int32_t* dist, void* stream) {
  CMH_CHECK_ARG(q_sign && db_sign && radius && order && starts && offsets && idx && dist, "mih_knn_fill: null pointer");
  MihKnnArgs a;
  CMH_CHECK_ARG(capacity >= 1, "mih_knn_fill: capacity=%lld below 1 (no hits: no call)", static_cast<long long>(capacity));
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0, "mih_knn_fill: offsets holds 64-bit integers: aligned to 8 bytes");
  const int rc = mih_knn_args("mih_knn_fill", q_sign, Q, db_sign, N, bits, 1, -1, order, starts, &a);
  if (rc != CMH_OK) return rc;
  a.walk_radius = radius; a.offsets = reinterpret_cast<const long long*>(offsets); a.capacity = capacity; a.idx = idx; a.dist = dist;
  launch_mih_knn<true>(a, as_stream(stream));
  CMH_CHECK_LAUNCH("mih_knn_fill");
  return CMH_OK;
}
