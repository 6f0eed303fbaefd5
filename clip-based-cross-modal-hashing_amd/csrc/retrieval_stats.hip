// Code diagnostics (cmh_code_gram): gram[i][j] = sum over the N items of a_i(n) b_j(n) for two operands in cmh_pack_codes' planes,
// and the per-bit sums sum a_i, sum |a_i|, sum b_j, sum |b_j|: bit balance, bit correlation, the agreement of an item's image and
// caption code and the class / bit tables are all made of these integers (utils/code_stats.py).  Exact int64, from the packed
// planes, without a float copy of the codes, any N up to 2^31 - 1 in one call.
//
// A product of two bit COLUMNS over 64 items is two popcounts: with ZA, ZB the nz columns and SA, SB the sign columns (64-bit words,
// bit n = item n of the slab), t = ZA_i & ZB_j, sum = popc(t) - 2 popc(t & (SA_i ^ SB_j)).  The planes are stored by ROWS (an item's
// words are adjacent), so the kernel transposes 64 items at a time with the wave's own ballot: a lane loads its item's words, and
// __ballot(bit b of my word) IS column b of the slab, a wave-uniform 64-bit value.
//   B columns  LANES OWN COLUMNS: lane l keeps columns l, 64 + l, ... (CB of them) of both planes in registers; a ballot arrives in
//              its lane by a select.  Built once per slab.
//   A columns  stay wave-uniform (scalar registers), made right before their use, one bit at a time.
//   work       for bit i of the A tile and each of the lane's CB columns: 2 AND, 1 XOR and 2 popcounts on 64-bit values, into the
//              32-bit accumulator acc[i][column] - 32 x CB registers, indexed by unrolled loops only (no scratch).
// One wave per workgroup owns a contiguous CHUNK of items (grid.x); the A bits are tiled over grid.y, kGramTile = 32 bits (one word
// of a row) per tile, so the accumulators stay at <= 128 registers.  Every tile builds the B columns of its slabs again: that is
// the price of keeping the accumulators in registers.  (64-bit tiles halve the rebuilding but leave one wave per SIMD at 128 bit:
// measured 7 - 24 % slower there and 3 % faster at 64 bit)
// Bits at and above abits / bbits are never output (no masking is needed: a column is one output row or column).  Lanes behind the
// chunk's last item read that item once more (no row behind the end is read) and clear their nz words, so they add nothing.
//
// The end of a chunk: the 32-bit partials go, sign-extended, by 64-bit integer atomics into one of <= kGramSlabs int64 images of the
// outputs in the workspace (chunk c -> image c % G; a hipMemsetAsync zeroes them first), so that the chunks of a large database
// do not all queue on the same words; code_gram_sum_kernel then adds the images and WRITES every output element.  Integer sums do
// not depend on the order: two calls give equal bytes, on any stream.
#include "retrieval_few.h"      // few_cu_count

namespace cmh {
namespace {

constexpr int kGramSlabs = 8;             // int64 images of the outputs that the chunks' atomics are spread over
constexpr int kGramTile = 32;             // A bits per workgroup: one word of a row
constexpr int kGramWavesPerCu = 16;       // chunks x A tiles that the plan aims at, per CU
constexpr int kGramMinChunk = 256;        // a chunk's epilogue is 32 x CB atomic instructions: not per 64 items

struct GramArgs {
  int64_t N;
  int abits, bbits, WA, WB, chunk, G;
  long long* img;      // [G][tot]: gram [abits][bbits], a_pos [abits], a_abs [abits], b_pos [bbits], b_abs [bbits]
};

__host__ __device__ __forceinline__ size_t gram_tot(int abits, int bbits) {
  return static_cast<size_t>(abits) * bbits + 2 * static_cast<size_t>(abits) + 2 * static_cast<size_t>(bbits);
}

// the first NW words (NW even) of a row of W words; rows of an even W are read as 8-byte pairs (the entry point checked the
// alignment), words at and behind W read as 0
template <int NW>
__device__ __forceinline__ void load_words(const uint32_t* __restrict__ p, int64_t row, int W, uint32_t (&out)[NW]) {
  const uint32_t* r = p + static_cast<size_t>(row) * W;
  if ((W & 1) == 0) {
#pragma unroll
    for (int w = 0; w < NW; w += 2) {
      uint2 v = {0u, 0u};
      if (w < W) v = *reinterpret_cast<const uint2*>(r + w);
      out[w] = v.x;
      out[w + 1] = v.y;
    }
    return;
  }
#pragma unroll
  for (int w = 0; w < NW; ++w) out[w] = w < W ? r[w] : 0u;
}

__device__ __forceinline__ uint64_t column(uint32_t word, int b) { return __ballot((word >> b) & 1u); }

// CB: B columns per lane (64 CB >= bbits)
template <int CB>
__global__ __launch_bounds__(64) void code_gram_kernel(GramArgs g, const uint32_t* __restrict__ as, const uint32_t* __restrict__ an,
                                                       const uint32_t* __restrict__ bs, const uint32_t* __restrict__ bn) {
  constexpr int TA = kGramTile;
  const int lane = threadIdx.x, c = blockIdx.x, i0 = blockIdx.y * TA;
  const int na = g.abits - i0 < TA ? g.abits - i0 : TA;      // bits of this tile: >= 1
  const bool sums_b = blockIdx.y == 0;                       // the B sums are the first tile's
  const int64_t jb = static_cast<int64_t>(c) * g.chunk;
  const int64_t je = jb + g.chunk < g.N ? jb + g.chunk : g.N;
  // 32-bit accumulators.  |acc[i][k]| is the absolute value of a sum of products in {-1, 0, +1} over the items of ONE chunk that were
  // walked so far (each step adds popc(t) - 2 popc(t & x), the exact sum over a slab), so it is <= the chunk's items <=
  // CMH_GRAM_CHUNK_MAX = 2^20 < 2^31.  The sums below count items of one chunk as well: the same bound.
  int acc[TA][CB];
  int apos = 0, aabs = 0, bpos[CB], babs[CB];      // lane l: bit i0 + l of A (l < na); columns l + 64 k of B
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int k = 0; k < CB; ++k) acc[i][k] = 0;
#pragma unroll
  for (int k = 0; k < CB; ++k) bpos[k] = babs[k] = 0;

  uint32_t cas, can, cbs[2 * CB], cbn[2 * CB], nas, nan_, nbs[2 * CB], nbn[2 * CB];      // the tile's word of A, the words of B
  auto fetch = [&](uint32_t& xs, uint32_t& xn, uint32_t (&ys)[2 * CB], uint32_t (&yn)[2 * CB], int64_t base) {
    const int64_t j = base + lane;
    const int64_t row = j < je ? j : je - 1;      // (lanes behind the last item read it once more)
    xs = as[static_cast<size_t>(row) * g.WA + blockIdx.y];
    xn = an[static_cast<size_t>(row) * g.WA + blockIdx.y];
    load_words<2 * CB>(bs, row, g.WB, ys);
    load_words<2 * CB>(bn, row, g.WB, yn);
    if (j >= je) {                                // ... and hold no item: nothing is non-zero
      xn = 0u;
#pragma unroll
      for (int w = 0; w < 2 * CB; ++w) yn[w] = 0u;
    }
  };
  fetch(cas, can, cbs, cbn, jb);
  for (int64_t base = jb; base < je; base += 64) {
    if (base + 64 < je) fetch(nas, nan_, nbs, nbn, base + 64);      // the next slab's rows fly during this one's work
    // the lane's B columns of this slab
    uint64_t zb[CB], sb[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) {
      zb[k] = sb[k] = 0u;
#pragma unroll
      for (int b = 0; b < 64; ++b) {      // (a ballot is wave-uniform: lane b keeps it, a select on a constant lane mask)
        const uint64_t z = column(cbn[2 * k + b / 32], b & 31), s = column(cbs[2 * k + b / 32], b & 31);
        zb[k] = lane == b ? z : zb[k];
        sb[k] = lane == b ? s : sb[k];
      }
      if (sums_b) {
        babs[k] += __popcll(zb[k]);
        bpos[k] += __popcll(zb[k] & sb[k]);
      }
    }
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      if (i < na) {                                                 // wave-uniform
        const uint64_t za = column(can, i), sa = column(cas, i);
        if (lane == i) {
          aabs += __popcll(za);
          apos += __popcll(za & sa);
        }
#pragma unroll
        for (int k = 0; k < CB; ++k) {
          const uint64_t t = za & zb[k];
          acc[i][k] += __popcll(t) - 2 * __popcll(t & (sa ^ sb[k]));
        }
      }
    }
    if (base + 64 < je) {
      cas = nas;
      can = nan_;
#pragma unroll
      for (int w = 0; w < 2 * CB; ++w) { cbs[w] = nbs[w]; cbn[w] = nbn[w]; }
    }
  }

  // the chunk's partials into its image: lane l adds to 64 adjacent words of a gram row (512 contiguous bytes per instruction)
  unsigned long long* img = reinterpret_cast<unsigned long long*>(g.img) + static_cast<size_t>(c % g.G) * gram_tot(g.abits, g.bbits);
  auto add = [](unsigned long long* p, int v) { atomicAdd(p, static_cast<unsigned long long>(static_cast<long long>(v))); };
#pragma unroll
  for (int i = 0; i < TA; ++i) {
    if (i < na) {
#pragma unroll
      for (int k = 0; k < CB; ++k) {
        const int j = 64 * k + lane;
        if (j < g.bbits) add(img + static_cast<size_t>(i0 + i) * g.bbits + j, acc[i][k]);
      }
    }
  }
  unsigned long long* sums = img + static_cast<size_t>(g.abits) * g.bbits;
  if (lane < na) {
    add(sums + i0 + lane, apos);
    add(sums + g.abits + i0 + lane, aabs);
  }
  if (sums_b) {
#pragma unroll
    for (int k = 0; k < CB; ++k) {
      const int j = 64 * k + lane;
      if (j < g.bbits) {
        add(sums + 2 * g.abits + j, bpos[k]);
        add(sums + 2 * g.abits + g.bbits + j, babs[k]);
      }
    }
  }
}

// the images added; every output element is written here, once.  sum = (items at +1) - (items at -1) = 2 pos - abs
__global__ __launch_bounds__(256) void code_gram_sum_kernel(GramArgs g, long long* __restrict__ gram, long long* __restrict__ a_sum,
                                                            long long* __restrict__ a_abs, long long* __restrict__ b_sum,
                                                            long long* __restrict__ b_abs) {
  const size_t tot = gram_tot(g.abits, g.bbits), cells = static_cast<size_t>(g.abits) * g.bbits;
  const size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  auto total = [&](size_t at) {
    long long s = 0;
    for (int i = 0; i < g.G; ++i) s += g.img[i * tot + at];
    return s;
  };
  if (e < cells) {
    gram[e] = total(e);
    return;
  }
  const size_t r = e - cells;
  if (r < static_cast<size_t>(g.abits)) {
    const long long pos = total(cells + r), ab = total(cells + g.abits + r);
    if (a_sum) a_sum[r] = 2 * pos - ab;
    if (a_abs) a_abs[r] = ab;
  } else if (r < static_cast<size_t>(g.abits + g.bbits)) {
    const size_t j = r - g.abits;
    const long long pos = total(cells + 2 * g.abits + j), ab = total(cells + 2 * g.abits + g.bbits + j);
    if (b_sum) b_sum[j] = 2 * pos - ab;
    if (b_abs) b_abs[j] = ab;
  }
}

int check_gram_shape(const char* what, int64_t N, int abits, int bbits, int64_t chunk_items) {
  auto bad = [&](const char* fmt, auto... v) -> int { return what ? fail(CMH_ERR_INVALID, fmt, what, v...) : CMH_ERR_INVALID; };
  if (N < 1 || N > INT32_MAX) return bad("%s: N=%lld outside [1, 2^31 - 1]", static_cast<long long>(N));
  if (abits < 1 || abits > CMH_GRAM_BITS_MAX) return bad("%s: abits=%d outside [1, %d]", abits, CMH_GRAM_BITS_MAX);
  if (bbits < 1 || bbits > CMH_GRAM_BITS_MAX) return bad("%s: bbits=%d outside [1, %d]", bbits, CMH_GRAM_BITS_MAX);
  if (chunk_items < 0 || chunk_items % 64 != 0 || chunk_items > CMH_GRAM_CHUNK_MAX)
    return bad("%s: chunk_items=%lld is neither 0 nor a multiple of 64 up to %d", static_cast<long long>(chunk_items), CMH_GRAM_CHUNK_MAX);
  return CMH_OK;
}

// The items cut into chunks, one wave each: with the A tiles as many as fill kGramWavesPerCu wave slots of every CU once, none
// below kGramMinChunk items and none above CMH_GRAM_CHUNK_MAX; or the caller's chunk_items as it stands.
struct GramPlan {
  int CB, tiles, chunk, G;
  int64_t S;
  size_t bytes(int abits, int bbits) const { return static_cast<size_t>(G) * gram_tot(abits, bbits) * 8 + 256; }
};

GramPlan gram_plan(int64_t N, int abits, int bbits, int64_t chunk_items) {
  GramPlan p;
  p.CB = (bbits + 63) / 64;
  p.tiles = (abits + kGramTile - 1) / kGramTile;
  int64_t chunk = chunk_items;
  if (chunk == 0) {
    int64_t s = static_cast<int64_t>(few_cu_count()) * kGramWavesPerCu / p.tiles;
    const int64_t by_min = (N + kGramMinChunk - 1) / kGramMinChunk;
    s = s < by_min ? s : by_min;
    s = s > 1 ? s : 1;
    chunk = (((N + s - 1) / s) + 63) & ~int64_t(63);
    chunk = chunk < CMH_GRAM_CHUNK_MAX ? chunk : CMH_GRAM_CHUNK_MAX;
  }
  p.chunk = static_cast<int>(chunk);
  p.S = (N + chunk - 1) / chunk;      // <= 2^31 / 64: a legal grid.x
  p.G = p.S < kGramSlabs ? static_cast<int>(p.S) : kGramSlabs;
  return p;
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_code_gram_workspace_bytes(int64_t N, int32_t abits, int32_t bbits, int64_t chunk_items) {
  return check_gram_shape(nullptr, N, abits, bbits, chunk_items) == CMH_OK ? gram_plan(N, abits, bbits, chunk_items).bytes(abits, bbits) : 0;
}

extern "C" int cmh_code_gram(const uint32_t* a_sign, const uint32_t* a_nz, const uint32_t* b_sign, const uint32_t* b_nz, int64_t N,
                             int32_t abits, int32_t bbits, int64_t chunk_items, int64_t* gram, int64_t* a_sum, int64_t* a_abs,
                             int64_t* b_sum, int64_t* b_abs, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(a_sign && a_nz && b_sign && b_nz && gram, "code_gram: null pointer");
  const int rc = check_gram_shape("code_gram", N, abits, bbits, chunk_items);
  if (rc != CMH_OK) return rc;
  const GramPlan p = gram_plan(N, abits, bbits, chunk_items);
  const int WA = (abits + 31) / 32, WB = (bbits + 31) / 32;
  auto aligned = [](const void* q, int W) { return (W & 1) != 0 || reinterpret_cast<uintptr_t>(q) % 8 == 0; };
  CMH_CHECK_ARG(aligned(b_sign, WB) && aligned(b_nz, WB),      // (an A tile is one word of a row: read as such)
                "code_gram: B planes of an even number of words per row (%d) are read as 8-byte pairs: aligned to 8 bytes", WB);
  if (!workspace || workspace_bytes < p.bytes(abits, bbits))
    return fail(CMH_ERR_WORKSPACE, "code_gram: workspace %zu < %zu bytes", workspace_bytes, p.bytes(abits, bbits));
  GramArgs g = {};
  g.N = N; g.abits = abits; g.bbits = bbits; g.WA = WA; g.WB = WB; g.chunk = p.chunk; g.G = p.G;
  g.img = reinterpret_cast<long long*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  hipStream_t st = as_stream(stream);
  const size_t tot = gram_tot(abits, bbits);
  if (hipMemsetAsync(g.img, 0, static_cast<size_t>(p.G) * tot * 8, st) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMH_ERR_LAUNCH, "code_gram: clearing the workspace failed");
  }
  const dim3 grid(static_cast<unsigned>(p.S), static_cast<unsigned>(p.tiles));
  switch (p.CB) {
    case 1: hipLaunchKernelGGL(code_gram_kernel<1>, grid, dim3(64), 0, st, g, a_sign, a_nz, b_sign, b_nz); break;
    case 2: hipLaunchKernelGGL(code_gram_kernel<2>, grid, dim3(64), 0, st, g, a_sign, a_nz, b_sign, b_nz); break;
    case 3: hipLaunchKernelGGL(code_gram_kernel<3>, grid, dim3(64), 0, st, g, a_sign, a_nz, b_sign, b_nz); break;
    default: hipLaunchKernelGGL(code_gram_kernel<4>, grid, dim3(64), 0, st, g, a_sign, a_nz, b_sign, b_nz); break;
  }
  CMH_CHECK_LAUNCH("code_gram");
  const size_t outs = static_cast<size_t>(abits) * bbits + abits + bbits;
  hipLaunchKernelGGL(code_gram_sum_kernel, dim3(static_cast<unsigned>((outs + 255) / 256)), dim3(256), 0, st, g,
                     reinterpret_cast<long long*>(gram), reinterpret_cast<long long*>(a_sum), reinterpret_cast<long long*>(a_abs),
                     reinterpret_cast<long long*>(b_sum), reinterpret_cast<long long*>(b_abs));
  CMH_CHECK_LAUNCH("code_gram (sum)");
  return CMH_OK;
}
