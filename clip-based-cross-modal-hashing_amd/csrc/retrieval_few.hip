// Top-k Hamming search for FEW queries (cmh_hamming_topk_few): the interactive case, one caption or one image against an index.
//
// The kernels of retrieval.hip let LANES OWN QUERIES: with one query 63 of a wave's 64 lanes repeat it, the grid stops at 256
// chunks and a database past 524 287 items costs a search per shard plus a merge.  Here LANES OWN ITEMS: a lane reads its item's
// W words per plane with one vector load (consecutive lanes, consecutive rows: coalesced), the query words are wave-uniform and
// arrive through the scalar cache, and the item words stay in registers while the wave loops over its queries.  Any database up to
// 2^31 - 1 items in one call: a chunk may hold any number of items (full 32-bit counters), row addresses are size_t.
//
// The result is cmh_hamming_topk's, bit for bit: the same distance arithmetic (h = bits - popc(nq & nr) + 2 popc((sq ^ sr) & nq &
// nr), the query's nz words cut to `bits` bits; Tile::half of retrieval.hip with the roles of the operands exchanged, which is
// why the text is not shared: there the query words are per lane and the item words uniform), the same stable counting sort:
//   few_pass<.., false>  per (chunk, group of <= 16 queries) the histogram of h, left in the workspace as img[chunk][q][bin]
//   few_total            tot[q][bin] = the sum over the chunks, and its exclusive prefixes over 32 PARTS of the chunk range
//   few_radius           per query the radius h* at which the cumulative count reaches k; tot becomes off[h], the exclusive prefix
//   few_base             for the bins <= h*: img[chunk][q][bin] = off[bin] + the items of that bin in earlier chunks
//   few_pass<.., true>   the walk again, 64 items at a time in index order: an item with h <= h* takes column
//                        cursor[h] + (lanes below it in the ballot of its h); stored iff that column is < k
// A workgroup is ONE wave and owns one contiguous chunk, so the images are at wave granularity and the second walk needs nothing
// from other waves.  Histogram and cursors live in LDS as [query of the group][bin], 4 bytes each: 16 queries x 257 bins = 16.1 KiB
// at 128 bit, 9 workgroups per CU by LDS, 8 by the wave slots the plan fills.  The private-column layout of retrieval.hip
// ([bin][lane], no same-address increments) would need 64 KiB PER QUERY here (lanes own items: every lane may hit every bin of
// every query), so the increments are LDS atomics on shared words and distances that cluster around K/2 serialise inside one
// instruction; 16-bit counters would halve the LDS but bound a chunk to 65 535 items, which 2^31 items in <= 2048 chunks exceed.
// Queries beyond 16 go to further workgroups (grid.y) that read the same chunk again (from L2 / the Infinity Cache: the groups of a
// chunk are dispatched together): the database is read once per 16 queries and pass, not once per query.
// No atomics on the outputs: every (query, column < k) is written exactly once, so two calls give equal bytes.
#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kFewGroup = 16;                        // queries per workgroup: the LDS rows of one wave
constexpr int kFewParts = 32;                        // parts of the chunk range in few_total / few_base
constexpr int kFewBinTile = 32;                      // bins per workgroup there (32 bins x 32 parts = 1024 threads)
constexpr int kFewSlabs = 4;                         // 64-item slabs a wave holds in registers at a time
constexpr int kFewWavesPerCu = 8;
constexpr size_t kFewImageCap = size_t(256) << 20;   // bytes of images, as kImageCap of retrieval.hip

struct FewArgs {      // (the operand planes are kernel parameters of their own: `__restrict__` there keeps the query words on the scalar unit)
  int Q, bits, W, bins, S, L, chunk, k;      // S chunks of `chunk` items (a multiple of 64), L = chunks per part
  int64_t N;
  uint32_t* img;      // [S][Q][bins]  histograms -> bases
  uint32_t* tot;      // [Q][bins]     totals -> off
  uint32_t* ppre;     // [Q][bins][kFewParts]
  int32_t* hstar;     // [Q]
  int32_t* idx;       // [Q][k]
  float* dist;        // [Q][k]
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
  // half-units of calc_hammingDist against a query (its words are wave-uniform, the nz words cut to `bits` bits)
  __device__ __forceinline__ int half(const uint32_t (&qs)[W], const uint32_t (&qn)[W], int bits) const {
    int both = 0, diff = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t nz = qn[w] & n[w];
      both += __popc(nz);
      diff += __popc((qs[w] ^ s[w]) & nz);
    }
    return bits - both + 2 * diff;
  }
};

// A query's words and its radius: wave-uniform, so they arrive through the scalar cache and stay in scalar registers
template <int W>
struct Query {
  uint32_t s[W], n[W];
  int hs;
  __device__ __forceinline__ void load(const uint32_t* __restrict__ qs, const uint32_t* __restrict__ qn, const int32_t* __restrict__ hstar,
                                       int q, uint32_t last) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
      s[w] = qs[q * W + w];
      n[w] = qn[q * W + w] & (w == W - 1 ? last : 0xffffffffu);
    }
    hs = hstar ? hstar[q] : 0;
  }
};

// ---- the walk of both passes: SELECT = false the histogram, true the stable counting sort of the items at h <= h* -----------------
template <int W, bool SELECT>
__global__ __launch_bounds__(64) void few_pass_kernel(FewArgs a, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ qn,
                                                      const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                      const int32_t* __restrict__ hstar) {
  extern __shared__ uint32_t col[];      // [nq][bins]: counters (histogram) or cursors (select)
  const int lane = threadIdx.x, c = blockIdx.x, q0 = blockIdx.y * kFewGroup;
  const int nq = a.Q - q0 < kFewGroup ? a.Q - q0 : kFewGroup;
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
  // kFewSlabs x 64 items at a time: that many independent row loads per plane are in flight per lane (one wave per workgroup and two
  // workgroups per SIMD: nothing else hides the latency), and the next set is requested before this one is worked on.
  Item<W> cur[kFewSlabs], nxt[kFewSlabs];
  auto fetch = [&](Item<W>(&it)[kFewSlabs], int64_t base) {
#pragma unroll
    for (int u = 0; u < kFewSlabs; ++u) {
      const int64_t j = base + u * 64 + lane;
      it[u].load(rs, rn, j < je ? j : je - 1);                               // (lanes behind the last item read it once more)
    }
  };
  fetch(cur, jb);
  for (int64_t base = jb; base < je; base += 64 * kFewSlabs) {
    fetch(nxt, base + 64 * kFewSlabs);
    Query<W> qc, qx;
    qc.load(qs, qn, hstar, q0, last);
    for (int qi = 0; qi < nq; ++qi) {
      qx.load(qs, qn, hstar, q0 + (qi + 1 < nq ? qi + 1 : qi), last);       // the next query's words fly during this one's work
#pragma unroll
      for (int u = 0; u < kFewSlabs; ++u) {                                   // in index order: slab u lies before slab u + 1
        const int64_t j = base + u * 64 + lane;
        const bool valid = j < je;                                            // lanes behind item N - 1 count and place nothing
        const int h = cur[u].half(qc.s, qc.n, a.bits);
        if (!SELECT) {
          if (valid) atomicAdd(&col[qi * a.bins + h], 1u);
        } else {
          bool pend = valid && h <= qc.hs;
          uint64_t mask = __ballot(pend);
          while (mask) {                                                      // wave-uniform: one turn per distinct h among the qualifiers
            const int hsel = __builtin_amdgcn_readlane(h, __ffsll(static_cast<unsigned long long>(mask)) - 1);
            const bool mine = pend && h == hsel;
            const uint64_t m = __ballot(mine);
            uint32_t* cursor = &col[qi * a.bins + hsel];
            const uint32_t at = *cursor;                                      // (same word for every lane)
            const uint32_t p = at + __popcll(m & below);
            if (mine && p < k) {
              const size_t o = static_cast<size_t>(q0 + qi) * k + p;
              a.idx[o] = static_cast<int32_t>(j);
              a.dist[o] = 0.5f * static_cast<float>(hsel);
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
__global__ __launch_bounds__(64) void few_radius_kernel(FewArgs a) {
  const int lane = threadIdx.x, q = blockIdx.x;
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
  if (lane == 0) a.hstar[q] = hs;      // (k <= N = the sum of a query's bins: always found)
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

// The database cut into chunks, one wave each: as many as fill the chip's wave slots once (equal work per wave), none below 256
// items (a small database is cut as cut_chunks of retrieval.hip cuts it), and no more than keep the images under kFewImageCap
// (at most 2048 / groups chunks of at most 64.25 KiB per chunk: 33 MiB, so the cap never binds on a 256-CU chip; it is what bounds
// the count on a larger one).
struct FewPlan {
  int W, bins, groups, S, L, chunk;
  size_t words(int Q) const {
    return static_cast<size_t>(S) * Q * bins + static_cast<size_t>(Q) * bins * (1 + kFewParts) + CMH_FEW_Q_MAX;
  }
  size_t bytes(int Q) const { return words(Q) * 4 + 256; }
};

FewPlan make_few_plan(int Q, int64_t N, int bits) {
  FewPlan p;
  p.W = (bits + 31) / 32;
  p.bins = 2 * bits + 1;
  p.groups = (Q + kFewGroup - 1) / kFewGroup;
  int64_t s = static_cast<int64_t>(few_cu_count()) * kFewWavesPerCu / p.groups;
  const int64_t by256 = (N + 255) / 256;
  const int64_t cap = static_cast<int64_t>(kFewImageCap / (static_cast<size_t>(Q) * p.bins * 4));
  s = s < by256 ? s : by256;
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

template <int W>
int run_few(const FewArgs& a, const FewPlan& p, const uint32_t* qs, const uint32_t* qn, const uint32_t* rs, const uint32_t* rn, hipStream_t st) {
  const int nq = a.Q < kFewGroup ? a.Q : kFewGroup;
  const size_t lds = static_cast<size_t>(nq) * a.bins * 4;
  const dim3 walk(p.S, p.groups), bins((a.bins + kFewBinTile - 1) / kFewBinTile, a.Q);
  hipLaunchKernelGGL((few_pass_kernel<W, false>), walk, dim3(64), lds, st, a, qs, qn, rs, rn, static_cast<const int32_t*>(nullptr));
  CMH_CHECK_LAUNCH("hamming_topk_few histogram");
  hipLaunchKernelGGL(few_total_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, a);
  CMH_CHECK_LAUNCH("hamming_topk_few totals");
  hipLaunchKernelGGL(few_radius_kernel, dim3(a.Q), dim3(64), 0, st, a);
  CMH_CHECK_LAUNCH("hamming_topk_few radius");
  hipLaunchKernelGGL(few_base_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, a);
  CMH_CHECK_LAUNCH("hamming_topk_few bases");
  hipLaunchKernelGGL((few_pass_kernel<W, true>), walk, dim3(64), lds, st, a, qs, qn, rs, rn, static_cast<const int32_t*>(a.hstar));
  CMH_CHECK_LAUNCH("hamming_topk_few select");
  return CMH_OK;
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_topk_few_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return check_few_shape(nullptr, Q, N, bits) == CMH_OK ? make_few_plan(Q, N, bits).bytes(Q) : 0;
}

extern "C" int cmh_hamming_topk_few(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q,
                                    int64_t N, int32_t bits, int32_t k, int32_t* idx, float* dist, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && idx && dist, "hamming_topk_few: null pointer");
  const int rc = check_few_shape("hamming_topk_few", Q, N, bits);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 1 && k <= CMH_FEW_K_MAX, "hamming_topk_few: k=%d outside [1, %d]", k, CMH_FEW_K_MAX);
  CMH_CHECK_ARG(k <= N, "hamming_topk_few: k=%d exceeds N=%lld", k, static_cast<long long>(N));
  const FewPlan p = make_few_plan(Q, N, bits);
  // a lane fetches its item's row with one load of W words: rows of 2 and 4 words are read as 8 and 16 bytes
  const uintptr_t row = p.W == 2 ? 8 : p.W == 4 ? 16 : 4;
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "hamming_topk_few: database planes of %d words per row must be aligned to %d bytes", p.W, static_cast<int>(row));
  if (!workspace || workspace_bytes < p.bytes(Q))
    return fail(CMH_ERR_WORKSPACE, "hamming_topk_few: workspace %zu < %zu bytes", workspace_bytes, p.bytes(Q));
  FewArgs a = {};
  a.Q = Q; a.bits = bits; a.W = p.W; a.bins = p.bins; a.S = p.S; a.L = p.L; a.chunk = p.chunk; a.k = k; a.N = N;
  a.img = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  a.tot = a.img + static_cast<size_t>(p.S) * Q * p.bins;
  a.ppre = a.tot + static_cast<size_t>(Q) * p.bins;
  a.hstar = reinterpret_cast<int32_t*>(a.ppre + static_cast<size_t>(Q) * p.bins * kFewParts);
  a.idx = idx; a.dist = dist;
  hipStream_t st = as_stream(stream);
  return p.W == 1 ? run_few<1>(a, p, q_sign, q_nz, r_sign, r_nz, st) : p.W == 2 ? run_few<2>(a, p, q_sign, q_nz, r_sign, r_nz, st)
         : p.W == 3 ? run_few<3>(a, p, q_sign, q_nz, r_sign, r_nz, st) : run_few<4>(a, p, q_sign, q_nz, r_sign, r_nz, st);
}
