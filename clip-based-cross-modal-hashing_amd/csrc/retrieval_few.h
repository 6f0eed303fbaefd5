// The pipeline of the searches in which LANES OWN ITEMS (retrieval_few.hip: Hamming distance; retrieval_soft.hip: the weighted
// distance of a real-valued query), written once.  A translation unit supplies a RULE:
//   struct Rule {
//     using Out = ...;                                     the element type of the distance column
//     template <int W> struct Query { int hs; load(qa, qb, hstar, q, last); };      a query's wave-uniform words and its radius
//     template <int W> static int bin(const Item<W>&, const Query<W>&, int bits);   the integer distance, 0 <= bin < FewArgs::bins
//     static Out out(int bin);                             what the distance column holds for that bin
//     static Out pad();                                    ... and for a column behind a masked search's last admitted item
//   };
// and the pipeline is the stable counting sort over that integer:
//   few_pass<.., false>  per (chunk, group of <= FewArgs::group queries) the histogram of the bins, left in the workspace as
//                        img[chunk][q][bin]
//   few_total            tot[q][bin] = the sum over the chunks, and its exclusive prefixes over 32 PARTS of the chunk range
//   few_radius           per query the radius h* at which the cumulative count reaches k; tot becomes off[h], the exclusive prefix
//   few_base             for the bins <= h*: img[chunk][q][bin] = off[bin] + the items of that bin in earlier chunks
//   few_pass<.., true>   the walk again, 64 items at a time in index order: an item with bin <= h* takes column
//                        cursor[bin] + (lanes below it in the ballot of its bin); stored iff that column is < k
// A workgroup is ONE wave and owns one contiguous chunk, so the images are at wave granularity and the second walk needs nothing
// from other waves.  Histogram and cursors live in LDS as [query of the group][bin], 4 bytes each; the increments are LDS atomics
// on shared words.  Queries beyond a group go to further workgroups (grid.y) that read the same chunk again (from L2 / the
// Infinity Cache: the groups of a chunk are dispatched together).
// No atomics on the outputs: every (query, column < k) is written exactly once, so two calls give equal bytes.
// The FILTERED search (MASKED = true) is the same pipeline over the items an allow-mask admits: one 64-bit word per slab in the
// walk's `valid`, and a radius kernel that takes "fewer than k admitted" (found < k; it writes found and the pad columns).
#pragma once

#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kFewParts = 32;                        // parts of the chunk range in few_total / few_base
constexpr int kFewBinTile = 32;                      // bins per workgroup there (32 bins x 32 parts = 1024 threads)
constexpr int kFewSlabs = 4;                         // 64-item slabs a wave holds in registers at a time
constexpr size_t kFewImageCap = size_t(256) << 20;   // bytes of images, as kImageCap of retrieval.hip

struct FewArgs {      // (the operand planes are kernel parameters of their own: `__restrict__` there keeps the query words on the scalar unit)
  int Q, bits, W, bins, S, L, chunk, k;      // S chunks of `chunk` items (a multiple of 64), L = chunks per part
  int group;                                 // queries per workgroup: the LDS rows of one wave
  int64_t N;
  uint32_t* img;      // [S][Q][bins]  histograms -> bases
  uint32_t* tot;      // [Q][bins]     totals -> off
  uint32_t* ppre;     // [Q][bins][kFewParts]
  int32_t* hstar;     // [Q]
  int32_t* idx;       // [Q][k]
  void* dist;         // [Q][k] of Rule::Out
};

// The W words per plane of one item, in registers
template <int W>
struct Item {
  uint32_t s[W], n[W];
  __device__ __forceinline__ void load(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn, int64_t j) {
    const size_t at = static_cast<size_t>(j) * W;
    if constexpr (W == 4) {
      const uint4 a = *reinterpret_cast<const uint4*>(rs + at), b = *reinterpret_cast<const uint4*>(rn + at);
      s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
      n[0] = b.x; n[1] = b.y; n[2] = b.z; n[3] = b.w;
    } else if constexpr (W == 2) {
      const uint2 a = *reinterpret_cast<const uint2*>(rs + at), b = *reinterpret_cast<const uint2*>(rn + at);
      s[0] = a.x; s[1] = a.y;
      n[0] = b.x; n[1] = b.y;
    } else {
#pragma unroll
      for (int w = 0; w < W; ++w) { s[w] = rs[at + w]; n[w] = rn[at + w]; }
    }
  }
};

// ---- the walk of both passes: SELECT = false the histogram, true the stable counting sort of the items at bin <= h* ---------------
// MASKED: only the items an allow-mask admits are counted and placed.  allow u64 [ceil(N / 64)], bit j % 64 of word j / 64 = item j
// is admitted; a slab of 64 items starts at a multiple of 64 (chunks are multiples of 64 items, a step is 64 kFewSlabs), so its
// 64 bits are ONE wave-uniform word, requested with the slab's rows and ANDed into `valid`.  Bits at and behind N are cut by
// j < je as the lanes behind the last item are; a slab that starts at or behind je reads no word.
template <class Rule, int W, bool SELECT, bool MASKED>
__global__ __launch_bounds__(64) void few_pass_kernel(FewArgs a, const uint32_t* __restrict__ qa, const uint32_t* __restrict__ qb,
                                                      const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                      const int32_t* __restrict__ hstar, const uint64_t* __restrict__ allow) {
  using Query = typename Rule::template Query<W>;
  using Out = typename Rule::Out;
  extern __shared__ uint32_t col[];      // [nq][bins]: counters (histogram) or cursors (select)
  const int lane = threadIdx.x, c = blockIdx.x, q0 = blockIdx.y * a.group;
  const int nq = a.Q - q0 < a.group ? a.Q - q0 : a.group;
  uint32_t* image = a.img + (static_cast<size_t>(c) * a.Q + q0) * a.bins;      // the group's rows of this chunk: nq * bins words
  if (SELECT) {
    for (int qi = 0; qi < nq; ++qi) {
      const int hs = hstar[q0 + qi];
      for (int h = lane; h <= hs; h += 64) col[qi * a.bins + h] = image[qi * a.bins + h];
    }
  } else {
    for (int i = lane; i < nq * a.bins; i += 64) col[i] = 0u;
  }
  __syncthreads();
  const int64_t jb = static_cast<int64_t>(c) * a.chunk;
  const int64_t je = jb + a.chunk < a.N ? jb + a.chunk : a.N;
  const uint32_t last = (a.bits & 31) ? (1u << (a.bits & 31)) - 1u : 0xffffffffu;
  const uint64_t below = (uint64_t(1) << lane) - 1u;
  const uint32_t k = static_cast<uint32_t>(a.k);
  Out* dist = static_cast<Out*>(a.dist);
  // kFewSlabs x 64 items at a time: that many independent row loads per plane are in flight per lane (one wave per workgroup and two
  // workgroups per SIMD: nothing else hides the latency), and the next set is requested before this one is worked on.
  constexpr int kWords = MASKED ? kFewSlabs : 1;                             // (unmasked: never touched)
  Item<W> cur[kFewSlabs], nxt[kFewSlabs];
  uint64_t cura[kWords], nxta[kWords];
  auto fetch = [&](Item<W>(&it)[kFewSlabs], uint64_t(&aw)[kWords], int64_t base) {
#pragma unroll
    for (int u = 0; u < kFewSlabs; ++u) {
      const int64_t j = base + u * 64 + lane;
      it[u].load(rs, rn, j < je ? j : je - 1);                               // (lanes behind the last item read it once more)
      if constexpr (MASKED) aw[u] = base + u * 64 < je ? allow[(base + u * 64) >> 6] : uint64_t(0);
    }
  };
  fetch(cur, cura, jb);
  for (int64_t base = jb; base < je; base += 64 * kFewSlabs) {
    fetch(nxt, nxta, base + 64 * kFewSlabs);
    Query qc, qx;
    qc.load(qa, qb, hstar, q0, last);
    for (int qi = 0; qi < nq; ++qi) {
      qx.load(qa, qb, hstar, q0 + (qi + 1 < nq ? qi + 1 : qi), last);       // the next query's words fly during this one's work
#pragma unroll
      for (int u = 0; u < kFewSlabs; ++u) {                                   // in index order: slab u lies before slab u + 1
        const int64_t j = base + u * 64 + lane;
        bool valid = j < je;                                                  // lanes behind item N - 1 count and place nothing
        if constexpr (MASKED) valid = valid && ((cura[u] >> lane) & 1u);      // ... and items the mask does not admit
        const int h = Rule::template bin<W>(cur[u], qc, a.bits);
        if (!SELECT) {
          if (valid) atomicAdd(&col[qi * a.bins + h], 1u);
        } else {
          bool pend = valid && h <= qc.hs;
          uint64_t mask = __ballot(pend);
          while (mask) {                                                      // wave-uniform: one turn per distinct bin among the qualifiers
            const int hsel = __builtin_amdgcn_readlane(h, __ffsll(static_cast<unsigned long long>(mask)) - 1);
            const bool mine = pend && h == hsel;
            const uint64_t m = __ballot(mine);
            uint32_t* cursor = &col[qi * a.bins + hsel];
            const uint32_t at = *cursor;                                      // (same word for every lane)
            const uint32_t p = at + __popcll(m & below);
            if (mine && p < k) {
              const size_t o = static_cast<size_t>(q0 + qi) * k + p;
              a.idx[o] = static_cast<int32_t>(j);
              dist[o] = Rule::out(hsel);
            }
            *cursor = at + __popcll(m);
            pend = pend && !mine;
            mask &= ~m;
          }
        }
      }
      qc = qx;
    }
#pragma unroll
    for (int u = 0; u < kFewSlabs; ++u) cur[u] = nxt[u];
    if constexpr (MASKED) {
#pragma unroll
      for (int u = 0; u < kFewSlabs; ++u) cura[u] = nxta[u];
    }
  }
  if (!SELECT) {
    __syncthreads();
    for (int i = lane; i < nq * a.bins; i += 64) image[i] = col[i];
  }
}

// ---- one thread per (bin, part) of a query: its part's chunks summed; thread (bin, 0) then scans the parts -> ppre, tot --------------
__global__ __launch_bounds__(kFewParts * kFewBinTile) void few_total_kernel(FewArgs a) {
  __shared__ uint32_t sums[kFewParts][kFewBinTile + 1];
  const int b = threadIdx.x % kFewBinTile, p = threadIdx.x / kFewBinTile;
  const int bin = blockIdx.x * kFewBinTile + b, q = blockIdx.y;
  const size_t stride = static_cast<size_t>(a.Q) * a.bins, w = static_cast<size_t>(q) * a.bins + bin;
  uint32_t s = 0;
  if (bin < a.bins) {
    const int c1 = (p + 1) * a.L < a.S ? (p + 1) * a.L : a.S;
    for (int c = p * a.L; c < c1; ++c) s += a.img[c * stride + w];
  }
  sums[p][b] = s;
  __syncthreads();
  if (p == 0 && bin < a.bins) {
    uint32_t run = 0;
    for (int i = 0; i < kFewParts; ++i) {
      a.ppre[w * kFewParts + i] = run;
      run += sums[i][b];
    }
    a.tot[w] = run;
  }
}

// ---- one wave per query: tot becomes off (the exclusive prefix over the bins), hstar = the first bin whose cumulative count >= k ----
// -> h* of the wave's query, -1 when the query's bins hold fewer than k items (a masked search only); total = the sum of its bins
__device__ __forceinline__ int few_radius(const FewArgs& a, int lane, int q, uint32_t& total) {
  uint32_t* tot = a.tot + static_cast<size_t>(q) * a.bins;
  uint32_t carry = 0;
  int hs = -1;
  for (int h0 = 0; h0 < a.bins; h0 += 64) {
    const int h = h0 + lane;
    const uint32_t v = h < a.bins ? tot[h] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (h < a.bins) tot[h] = carry + x - v;
    const uint64_t m = __ballot(h < a.bins && carry + x >= static_cast<uint32_t>(a.k));
    if (hs < 0 && m) hs = h0 + __ffsll(static_cast<unsigned long long>(m)) - 1;
    carry += __shfl(x, 63, 64);
  }
  total = carry;
  return hs;
}

__global__ __launch_bounds__(64) void few_radius_kernel(FewArgs a) {
  uint32_t total;
  const int hs = few_radius(a, threadIdx.x, blockIdx.x, total);
  if (threadIdx.x == 0) a.hstar[blockIdx.x] = hs;      // (k <= N = the sum of a query's bins: always found)
}

// The masked search's: the bins hold the A admitted items, and A < k is legal.  Then h* = the last bin (everything admitted is
// placed, in columns 0..A-1), found = A, and the columns at and behind found are written HERE, once: idx = -1, dist = pad.
template <class Out>
__global__ __launch_bounds__(64) void few_radius_masked_kernel(FewArgs a, int32_t* __restrict__ found, Out pad) {
  const int lane = threadIdx.x, q = blockIdx.x;
  uint32_t total;
  const int hs = few_radius(a, lane, q, total);
  const int got = hs < 0 ? static_cast<int>(total) : a.k;
  if (lane == 0) {
    a.hstar[q] = hs < 0 ? a.bins - 1 : hs;
    found[q] = got;
  }
  Out* dist = static_cast<Out*>(a.dist);
  for (int c = got + lane; c < a.k; c += 64) {
    const size_t o = static_cast<size_t>(q) * a.k + c;
    a.idx[o] = -1;
    dist[o] = pad;
  }
}

// ---- one thread per (bin <= h*, part) of a query: every image of its part becomes the cursor base of its (chunk, bin) ---------------
__global__ __launch_bounds__(kFewParts * kFewBinTile) void few_base_kernel(FewArgs a) {
  const int b = threadIdx.x % kFewBinTile, p = threadIdx.x / kFewBinTile;
  const int bin = blockIdx.x * kFewBinTile + b, q = blockIdx.y;
  if (bin >= a.bins || bin > a.hstar[q]) return;
  const size_t stride = static_cast<size_t>(a.Q) * a.bins, w = static_cast<size_t>(q) * a.bins + bin;
  uint32_t base = a.tot[w] + a.ppre[w * kFewParts + p];
  const int c1 = (p + 1) * a.L < a.S ? (p + 1) * a.L : a.S;
  for (int c = p * a.L; c < c1; ++c) {
    const uint32_t v = a.img[c * stride + w];
    a.img[c * stride + w] = base;
    base += v;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// CUs of the device that is current at the first call, kept for the life of the process; 256 (MI355X) where none answers.  It only
// sizes the grid: the workspace query and the call compute the plan from the same number, and the result does not depend on how
// the database is cut, so a process that later runs on another device or stream is as correct, at worst filled less evenly.
int few_cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      return 256;      // (the workspace query also serves callers without a GPU)
    }
    return n;
  }();
  return cus;
}

// The database cut into chunks, one wave each: as many as fill `waves_per_cu` wave slots of every CU once (equal work per wave), none
// below `min_chunk` items, and no more than keep the images under kFewImageCap.
struct FewPlan {
  int W, bins, group, groups, S, L, chunk;
  size_t words(int Q) const {
    return static_cast<size_t>(S) * Q * bins + static_cast<size_t>(Q) * bins * (1 + kFewParts) + CMH_FEW_Q_MAX;
  }
  size_t bytes(int Q) const { return words(Q) * 4 + 256; }
};

FewPlan make_few_plan(int Q, int64_t N, int bits, int bins, int group, int waves_per_cu, int min_chunk) {
  FewPlan p;
  p.W = (bits + 31) / 32;
  p.bins = bins;
  p.group = group;
  p.groups = (Q + group - 1) / group;
  int64_t s = static_cast<int64_t>(few_cu_count()) * waves_per_cu / p.groups;
  const int64_t by_min = (N + min_chunk - 1) / min_chunk;
  const int64_t cap = static_cast<int64_t>(kFewImageCap / (static_cast<size_t>(Q) * p.bins * 4));
  s = s < by_min ? s : by_min;
  s = s < cap ? s : cap;
  s = s > 1 ? s : 1;
  p.chunk = static_cast<int>((((N + s - 1) / s) + 63) & ~int64_t(63));
  p.S = static_cast<int>((N + p.chunk - 1) / p.chunk);
  p.L = (p.S + kFewParts - 1) / kFewParts;
  return p;
}

int check_few_shape(const char* what, int Q, int64_t N, int bits) {
  auto bad = [&](const char* fmt, auto... v) -> int { return what ? fail(CMH_ERR_INVALID, fmt, what, v...) : CMH_ERR_INVALID; };
  if (Q < 1 || Q > CMH_FEW_Q_MAX) return bad("%s: Q=%d outside [1, %d]", Q, CMH_FEW_Q_MAX);
  if (N < 1 || N > INT32_MAX) return bad("%s: N=%lld outside [1, 2^31 - 1]", static_cast<long long>(N));
  if (bits < 1 || bits > CMH_FEW_BITS_MAX) return bad("%s: bits=%d outside [1, %d]", bits, CMH_FEW_BITS_MAX);
  return CMH_OK;
}

// The arguments of a call, its workspace carved: img, tot, ppre, hstar in that order behind a 256-byte boundary
FewArgs few_args(const FewPlan& p, int Q, int64_t N, int bits, int k, int32_t* idx, void* dist, void* workspace) {
  FewArgs a = {};
  a.Q = Q; a.bits = bits; a.W = p.W; a.bins = p.bins; a.S = p.S; a.L = p.L; a.chunk = p.chunk; a.k = k; a.group = p.group; a.N = N;
  a.img = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  a.tot = a.img + static_cast<size_t>(p.S) * Q * p.bins;
  a.ppre = a.tot + static_cast<size_t>(Q) * p.bins;
  a.hstar = reinterpret_cast<int32_t*>(a.ppre + static_cast<size_t>(Q) * p.bins * kFewParts);
  a.idx = idx; a.dist = dist;
  return a;
}

// a lane fetches its item's row with one load of W words: rows of 2 and 4 words are read as 8 and 16 bytes
int few_row_bytes(int W) { return W == 2 ? 8 : W == 4 ? 16 : 4; }

// allow / found: null = the plain search; both given = the masked one (the masked walk, the radius kernel that writes found and pads)
template <class Rule, int W, bool MASKED>
int run_few_w(const char* what, const FewArgs& a, const FewPlan& p, const uint32_t* qa, const uint32_t* qb, const uint32_t* rs,
              const uint32_t* rn, const uint64_t* allow, int32_t* found, hipStream_t st) {
  const int nq = a.Q < a.group ? a.Q : a.group;
  const size_t lds = static_cast<size_t>(nq) * a.bins * 4;
  const dim3 walk(p.S, p.groups), bins((a.bins + kFewBinTile - 1) / kFewBinTile, a.Q);
  char stage[96];
  auto launched = [&](const char* name) -> int {
    snprintf(stage, sizeof stage, "%s %s", what, name);
    CMH_CHECK_LAUNCH(stage);
    return CMH_OK;
  };
  int rc;
  hipLaunchKernelGGL((few_pass_kernel<Rule, W, false, MASKED>), walk, dim3(64), lds, st, a, qa, qb, rs, rn,
                     static_cast<const int32_t*>(nullptr), allow);
  if ((rc = launched("histogram")) != CMH_OK) return rc;
  hipLaunchKernelGGL(few_total_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, a);
  if ((rc = launched("totals")) != CMH_OK) return rc;
  if constexpr (MASKED)
    hipLaunchKernelGGL((few_radius_masked_kernel<typename Rule::Out>), dim3(a.Q), dim3(64), 0, st, a, found, Rule::pad());
  else
    hipLaunchKernelGGL(few_radius_kernel, dim3(a.Q), dim3(64), 0, st, a);
  if ((rc = launched("radius")) != CMH_OK) return rc;
  hipLaunchKernelGGL(few_base_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, a);
  if ((rc = launched("bases")) != CMH_OK) return rc;
  hipLaunchKernelGGL((few_pass_kernel<Rule, W, true, MASKED>), walk, dim3(64), lds, st, a, qa, qb, rs, rn,
                     static_cast<const int32_t*>(a.hstar), allow);
  return launched("select");
}

template <class Rule, bool MASKED>
int run_few_m(const char* what, const FewArgs& a, const FewPlan& p, const uint32_t* qa, const uint32_t* qb, const uint32_t* rs,
              const uint32_t* rn, const uint64_t* allow, int32_t* found, hipStream_t st) {
  return p.W == 1   ? run_few_w<Rule, 1, MASKED>(what, a, p, qa, qb, rs, rn, allow, found, st)
         : p.W == 2 ? run_few_w<Rule, 2, MASKED>(what, a, p, qa, qb, rs, rn, allow, found, st)
         : p.W == 3 ? run_few_w<Rule, 3, MASKED>(what, a, p, qa, qb, rs, rn, allow, found, st)
                    : run_few_w<Rule, 4, MASKED>(what, a, p, qa, qb, rs, rn, allow, found, st);
}

template <class Rule>
int run_few(const char* what, const FewArgs& a, const FewPlan& p, const uint32_t* qa, const uint32_t* qb, const uint32_t* rs,
            const uint32_t* rn, hipStream_t st, const uint64_t* allow = nullptr, int32_t* found = nullptr) {
  return allow ? run_few_m<Rule, true>(what, a, p, qa, qb, rs, rn, allow, found, st)
               : run_few_m<Rule, false>(what, a, p, qa, qb, rs, rn, nullptr, nullptr, st);
}

// What a masked call refuses beyond the plain one's checks
int check_few_mask(const char* what, const void* allow, const void* found) {
  if (!allow || !found) return fail(CMH_ERR_INVALID, "%s: null pointer (allow, found)", what);
  if (reinterpret_cast<uintptr_t>(allow) % 8) return fail(CMH_ERR_INVALID, "%s: the allow-mask holds 64-bit words: aligned to 8 bytes", what);
  return CMH_OK;
}

}  // namespace
}  // namespace cmh
