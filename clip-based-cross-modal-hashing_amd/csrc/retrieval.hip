// Retrieval on packed codes: distance histograms by relevance and top-k search (the consumers of the codes that the reference leaves
// to an offline MATLAB step: the PR_cruve/*.mat files of train/base.py::save_mat exist to draw precision-recall and top-N curves).
//   calc_hammingDist :8-13   0.5*(K - q.r)   -> half-units h = K - q.r in [0, 2K], AND/XOR + popcount on the bit planes
//   calc_neighbor    :42-45  (la.lb^T > 0)   -> any(la & lb)
//
// A distance takes at most 2K+1 values, so both results come from counting, never from sorting:
//   cmh_hamming_hist  counts[q, h, rel]                                  (one pass over the database)
//   cmh_hamming_topk  the first k columns of torch.sort(hamm, stable=True): the histogram gives, per query, the radius h* at which
//                     the cumulative count reaches k and the exclusive prefix off[h] of every bin below it; a second pass over the
//                     database is a STABLE COUNTING SORT restricted to h <= h*: item j goes to column off[h] + (items of the same
//                     h before j), and is dropped when that column is >= k (only the tie group at h* loses members: its first
//                     k - count(< h*) items in index order stay).
//
// Mapping: LANES OWN QUERIES.  A 64-thread workgroup holds 64 queries (their code words in registers); database words are
// wave-uniform, so they arrive through the scalar cache and every item costs each lane 5 VALU operations per 32 bits.  Each lane
// has a private column of counters, word index = bin * 64 + lane: the 64 lanes of one LDS instruction hit 64 different words in 32
// banks, two lanes per bank in different 32-lane groups, so an increment never meets a same-address or a bank conflict however the
// distances cluster around K/2 (lanes that own database items would all increment the few bins around K/2 of one query).  The same
// column is what makes the second pass trivial: a lane walks the database in index order, so its private cursor per bin IS the
// stable rank, and the tie rule needs no extra code.
// The database is cut into S chunks (grid = query tiles x chunks) to fill the chip; a chunk holds <= 65 532 items, so one 32-bit
// word per (bin, lane) carries both counters of the pass (low half: all items, high half: the relevant ones).  Every workgroup
// leaves its column image [bin][lane] in the workspace; reduce_kernel adds the images up (no atomics on the output: counts are
// written once) and turns them into exclusive prefixes over the chunks, radius_kernel scans the bins per query.
// LDS per workgroup: (2K+1) * 256 bytes: 33 KiB at 64 bit (4 per CU), 64.25 KiB at 128 bit (2 per CU).  Wider codes (up to 2048 bit:
// 4097 bins = 1 MiB per tile) keep the columns in the workspace and increment them with global atomics: same code, same results,
// not fast.
//
// Graded relevance (NDCG / ACG / WAP count the labels a pair shares; calc_neighbor only asks whether there are any):
//   cmh_hamming_topk_graded  the same search; the select pass stores popcount(la & lb) where it stores the hit flag
//   cmh_label_overlap_hist   grade_counts[q, g] = database items that share exactly g labels with query q.  The mapping of the
//                            distance histogram with the grade as the bin: 64 queries per workgroup with their label words in
//                            registers (1 or 3 words) or staged in LDS, database label words wave-uniform, a private column
//                            [g][lane] of full 32-bit counters (a chunk may hold any number of items), images summed by
//                            grade_reduce_kernel.  LDS per workgroup: (C+1) * 256 bytes: 6.25 KiB at 24 classes, 20.25 KiB at 80,
//                            64 KiB at 255 (one byte per grade: C <= 255).
//
// mAP by counting (AP needs ranks, not the permutation; any database size, as shards):
//   cmh_hamming_ap_partial   per query the float64 sum of relrank / rank over the relevant items of one call's database, which may be
//                            one shard of a larger one: the histogram pass, three small kernels that turn its images into 32-bit
//                            bases per (chunk, bin, lane), and a second walk whose packed LDS cursor gives both positions of an item.
//   cmh_ap_finish            ap = sum / min(k, R), map = their f32 mean in query order.
//
// Radius search (every item within a Hamming radius, as ragged lists; any database size, as shards):
//   cmh_hamming_range        the select pass without a k: the histogram pass, three small kernels that turn its images into the
//                            32-bit in-row base of every (chunk, bin <= radius, lane), and a second walk that stores item j at
//                            row_off[q] + its base's cursor.  The caller sizes the rows from cmh_hamming_hist.
//
// Ranks of given targets (instance-level recall: where does the item that belongs to this query rank?; any database size, as shards):
//   cmh_hamming_rank         per (query, target) the three counts less / ties_before / ties of one walk over the database: no
//                            columns, a lane keeps its targets' distances and counters in registers; the counts of shards add.
//
// Written once, used by every entry point: Block (what a pass kernel starts from), walk2 (the software-pipelined walk over a chunk;
// select_kernel alone keeps a copy of both, for a measured reason given there),
// the images -> bases family total / scan / base (REL: with the relevant half, the mAP; without, the radius search), and on the host
// dispatch + launch_walk (run-time shape -> compile-time kernel form) and for_each_batch (query tiles in batches, the histogram pass).
#include <type_traits>

#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kRetMaxWords = 64;           // bits, classes <= 2048
constexpr int kRetMaxN = (1 << 19) - 1;    // as the ranking kernel
constexpr int kLdsBits = 128;              // columns in LDS up to this code length
constexpr int kChunkMax = 65532;           // items per chunk: two 16-bit counters per word (a multiple of the unroll)
constexpr int kGradeMax = 255;             // classes of the graded entry points: a grade is one byte
constexpr size_t kImageCap = size_t(256) << 20;   // bytes of column images per batch of query tiles

struct RetArgs {
  const uint32_t *qs, *qn, *ql;      // (the database planes are kernel parameters of their own: `__restrict__` there is what tells the
                                     // compiler that the select pass's stores never touch them, so their loads stay on the scalar unit)
  int Q, N, bits, W, LW, bins, tiles, S, chunk, k;
  uint32_t* img;      // [S][tiles][bins][64]
  uint32_t* off;      // [tiles][bins][64]
  int32_t* hstar;     // [tiles * 64]
  uint32_t* counts;   // [Q][bins][2] or null ([Q][bins], bins = classes + 1, in the label histogram)
  int32_t* idx;       // [Q][k]
  float* dist;        // [Q][k]
  uint8_t* rel;       // [Q][k] or null
};      // (what one kernel alone needs is a trailing parameter of that kernel: a larger RetArgs moves the argument offsets of every
        // pass, measured as +1.2 % on the plain search when the grade pointer was a member)

// Label words per item: LT > 0 = that many, in registers; LAB_NONE = no labels; LAB_ANY = any number, the query's staged in LDS.
enum { LAB_NONE = 0, LAB_ANY = -1 };

// A tile's query operands: WT > 0 = exactly WT code words per plane, in registers; WT = 0 = any number, staged in LDS as [word][lane].
template <int WT, int LT>
struct Tile {
  static constexpr int WR = WT > 0 ? WT : 1, LR = LT > 0 ? LT : 1;
  uint32_t s[WR], n[WR], l[LR];
  const uint32_t* st;      // staged words: sign [W][64], nz [W][64] (WT = 0), then label [LW][64] (LAB_ANY)
  int W, LW, bits, lane;

  __device__ __forceinline__ void load(const RetArgs& a, int q, int lane_, uint32_t* stage) {
    W = a.W; LW = a.LW; bits = a.bits; lane = lane_; st = stage;
    // the query's nz words are cut to `bits` bits: whatever the planes hold behind the code, 0 <= h <= 2 * bits (h indexes the column)
    const uint32_t last = (bits & 31) ? (1u << (bits & 31)) - 1u : 0xffffffffu;
    if (WT > 0) {
#pragma unroll
      for (int w = 0; w < WR; ++w) {
        s[w] = a.qs[static_cast<size_t>(q) * WT + w];
        n[w] = a.qn[static_cast<size_t>(q) * WT + w] & (w == WT - 1 ? last : 0xffffffffu);
      }
    } else {
      for (int w = 0; w < W; ++w) {
        stage[w * 64 + lane] = a.qs[static_cast<size_t>(q) * W + w];
        stage[(W + w) * 64 + lane] = a.qn[static_cast<size_t>(q) * W + w] & (w == W - 1 ? last : 0xffffffffu);
      }
    }
    if (LT > 0) {
#pragma unroll
      for (int w = 0; w < LR; ++w) l[w] = a.ql[static_cast<size_t>(q) * LT + w];
    }
    if (LT == LAB_ANY)
      for (int w = 0; w < LW; ++w) stage[((WT ? 0 : 2 * W) + w) * 64 + lane] = a.ql[static_cast<size_t>(q) * LW + w];
  }
  // half-units of calc_hammingDist against one database item (its words are wave-uniform)
  __device__ __forceinline__ int half(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn) const {
    int both = 0, diff = 0;
    if (WT > 0) {
#pragma unroll
      for (int w = 0; w < WR; ++w) {
        const uint32_t nz = n[w] & rn[w];
        both += __popc(nz);
        diff += __popc((s[w] ^ rs[w]) & nz);
      }
    } else {
      for (int w = 0; w < W; ++w) {
        const uint32_t nz = st[(W + w) * 64 + lane] & rn[w];
        both += __popc(nz);
        diff += __popc((st[w * 64 + lane] ^ rs[w]) & nz);
      }
    }
    return bits - both + 2 * diff;
  }
  __device__ __forceinline__ uint32_t relevant(const uint32_t* __restrict__ rl) const {
    if (LT == LAB_NONE) return 0u;
    uint32_t any = 0;
    if (LT > 0) {
#pragma unroll
      for (int w = 0; w < LR; ++w) any |= l[w] & rl[w];
    } else {
      for (int w = 0; w < LW; ++w) any |= st[((WT ? 0 : 2 * W) + w) * 64 + lane] & rl[w];
    }
    return any ? 1u : 0u;
  }
  // labels shared with one database item
  __device__ __forceinline__ uint32_t overlap(const uint32_t* __restrict__ rl) const {
    uint32_t g = 0;
    if (LT > 0) {
#pragma unroll
      for (int w = 0; w < LR; ++w) g += __popc(l[w] & rl[w]);
    } else if (LT == LAB_ANY) {
      for (int w = 0; w < LW; ++w) g += __popc(st[((WT ? 0 : 2 * W) + w) * 64 + lane] & rl[w]);
    }
    return g;
  }
};

__host__ __device__ inline size_t stage_words(int WT, int LT, int W, int LW) {
  return static_cast<size_t>((WT ? 0 : 2 * W) + (LT == LAB_ANY ? LW : 0)) * 64;
}

// The words of U consecutive database items, U * WT <= 16 per plane: constant offsets from one wave-uniform address, so each plane
// arrives in one or two wide scalar loads.  A scalar load can only be waited for together with everything else in flight on its
// counter, so per-word loads inside the item loop cost a full round trip each (a first version: ~840 cycles per item at 128 bit
// against ~110 of vector work): see walk2.
template <int WT, int LT>
struct Group {
  static constexpr int U = WT == 1 ? 16 : WT == 2 ? 8 : 4, NW = U * (WT > 0 ? WT : 1), NL = U * (LT > 0 ? LT : 1);
  uint32_t s[NW], n[NW], l[NL];
  __device__ __forceinline__ void load(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn, const uint32_t* __restrict__ rl,
                                       int j, bool labels) {
    const uint32_t* __restrict__ ps = rs + static_cast<size_t>(j) * WT;
    const uint32_t* __restrict__ pn = rn + static_cast<size_t>(j) * WT;
#pragma unroll
    for (int i = 0; i < NW; ++i) { s[i] = ps[i]; n[i] = pn[i]; }
    if (LT > 0 && labels) {
      const uint32_t* __restrict__ pl = rl + static_cast<size_t>(j) * LT;
#pragma unroll
      for (int i = 0; i < NL; ++i) l[i] = pl[i];
    }
  }
};

// The label words of U consecutive database items, as Group holds the code words: one or two wide scalar loads.
template <int LT>
struct LabelGroup {
  static constexpr int U = LT == 1 ? 16 : 4, NL = U * (LT > 0 ? LT : 1);
  uint32_t l[NL];
  __device__ __forceinline__ void load(const uint32_t* __restrict__ rl, int j) {
    const uint32_t* __restrict__ pl = rl + static_cast<size_t>(j) * LT;
#pragma unroll
    for (int i = 0; i < NL; ++i) l[i] = pl[i];
  }
};

// What every pass kernel starts from: its lane's query, its chunk [jb, je) of the database, its column image.
struct Block {
  int lane, tile, c, q, jb, je;
  bool valid;      // the lane has a query of its own
  size_t at;       // the image [bins][64] of (chunk, tile): its first word in a.img and in every array laid out like it
  __device__ __forceinline__ explicit Block(const RetArgs& a) : lane(threadIdx.x), tile(blockIdx.x), c(blockIdx.y) {
    const int qa = tile * 64 + lane;
    valid = qa < a.Q;
    q = valid ? qa : a.Q - 1;      // lanes behind the last query repeat it; nobody reads their column or sum
    at = (static_cast<size_t>(c) * a.tiles + tile) * a.bins * 64;
    jb = c * a.chunk;
    je = jb + a.chunk < a.N ? jb + a.chunk : a.N;
  }
};

// The walk over the items [jb, je) in groups of G::U: load(g, j) fetches the group that starts at item j, work(g, j0, u0, u1) handles
// its members u0 <= u < u1.  Two register sets, and the fetch of one is issued right BEHIND the first use of the other (where the
// wait for the scalar loads sits): it is in flight while the rest of that group is worked on.  -> the first item left over, for
// the caller's item-at-a-time tail (fewer than U items).
template <class G, class Load, class Work>
__device__ __forceinline__ int walk2(int jb, int je, Load load, Work work) {
  int j = jb;
  const int groups = (je - jb) / G::U;
  G ga, gb;                                                       // two register sets: one is fetched while the other is worked on
  int g = 0;
  if (groups > 0) load(ga, jb);
  for (; g + 2 <= groups; g += 2, j += 2 * G::U) {
    work(ga, j, 0, 1);                                           // the wait for ga's words (and for everything else in flight) sits here
    __builtin_amdgcn_sched_barrier(0);
    load(gb, j + G::U);                                          // ... so gb's fetch is issued behind it and flies during the rest of ga
    __builtin_amdgcn_sched_barrier(0);
    work(ga, j, 1, G::U);
    work(gb, j + G::U, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
    load(ga, g + 2 < groups ? j + 2 * G::U : j);                 // (behind the last pair: a group once more, no branch)
    __builtin_amdgcn_sched_barrier(0);
    work(gb, j + G::U, 1, G::U);
  }
  if (g < groups) { work(ga, j, 0, G::U); j += G::U; }
  return j;
}

// ---- pass 1: per (query tile, chunk) the column image: word [h][lane] = items at h | relevant items at h << 16 ------------------
template <int WT, int LT, bool GLOB>
__global__ __launch_bounds__(64) void hist_kernel(RetArgs a, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                  const uint32_t* __restrict__ rl) {
  extern __shared__ uint32_t smem[];
  const Block b(a);
  const int lane = b.lane;
  uint32_t* image = a.img + b.at;
  uint32_t* col = GLOB ? image : smem;
  Tile<WT, LT> t;
  t.load(a, b.q, lane, smem + (GLOB ? 0 : a.bins * 64));
  if (!GLOB)
    for (int h = 0; h < a.bins; ++h) col[h * 64 + lane] = 0u;
  __syncthreads();
  int j = b.jb;
  if (WT > 0) {
    using G = Group<WT, LT>;
    j = walk2<G>(
        b.jb, b.je, [&](G& g, int j0) { g.load(rs, rn, rl, j0, true); },
        [&](const G& g, int j0, int u0, int u1) {
#pragma unroll
          for (int u = u0; u < u1; ++u) {
            const int h = t.half(g.s + u * WT, g.n + u * WT);
            const uint32_t r = LT > 0 ? t.relevant(g.l + u * LT) : t.relevant(rl + static_cast<size_t>(j0 + u) * a.LW);
            atomicAdd(&col[h * 64 + lane], 1u + (r << 16));
          }
        });
  }
  for (; j < b.je; ++j) {
    const int h = t.half(rs + static_cast<size_t>(j) * a.W, rn + static_cast<size_t>(j) * a.W);
    const uint32_t r = t.relevant(rl + static_cast<size_t>(j) * a.LW);
    atomicAdd(&col[h * 64 + lane], 1u + (r << 16));
  }
  if (!GLOB) {
    __syncthreads();
    for (int h = 0; h < a.bins; ++h) image[h * 64 + lane] = col[h * 64 + lane];
  }
}

// ---- images -> counts and bases: one thread per word (tile, bin < used, lane) of a tile's images ------------------------------------
struct Word {
  size_t stride, w;      // words of one chunk's images; this thread's word in them
  int h, q;              // its bin, its query (clamped as in Block)
  bool live, valid;      // the thread has a word; the word has a query of its own
  __device__ __forceinline__ Word(const RetArgs& a, int used) : stride(static_cast<size_t>(a.tiles) * a.bins * 64) {
    const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    live = t < static_cast<size_t>(a.tiles) * used * 64;
    const int lane = static_cast<int>(t & 63);
    const size_t hb = t >> 6;
    h = static_cast<int>(hb % used);
    const int tile = static_cast<int>(hb / used), qa = tile * 64 + lane;
    valid = qa < a.Q;
    q = valid ? qa : a.Q - 1;
    w = (static_cast<size_t>(tile) * a.bins + h) * 64 + lane;
  }
};

// A word summed over the chunks.  packed: hist_kernel's word, items | relevant << 16 (else one full counter); prefix: every chunk's
// word becomes the items of the chunks before it.
struct Sum { uint32_t items, rel; };
__device__ __forceinline__ Sum sum_chunks(const RetArgs& a, const Word& x, bool packed, bool prefix) {
  Sum s = {0u, 0u};
  for (int c = 0; c < a.S; ++c) {
    const uint32_t v = a.img[c * x.stride + x.w];
    if (prefix) a.img[c * x.stride + x.w] = s.items;
    s.items += packed ? v & 0xffffu : v;
    if (packed) s.rel += v >> 16;
  }
  return s;
}

__device__ __forceinline__ void put_counts(const RetArgs& a, const Word& x, Sum s) {
  if (a.counts && x.valid) {
    uint32_t* o = a.counts + (static_cast<size_t>(x.q) * a.bins + x.h) * 2;
    o[0] = s.items - s.rel;
    o[1] = s.rel;
  }
}

// ---- the images of a tile summed over the chunks -> counts; with `select` also: each image becomes the exclusive prefix over the
//      chunks before it (items only) and off[tile][h][lane] = items at h
__global__ __launch_bounds__(256) void reduce_kernel(RetArgs a, int select) {
  const Word x(a, a.bins);
  if (!x.live) return;
  const Sum s = sum_chunks(a, x, true, select);
  put_counts(a, x, s);
  if (select) a.off[x.w] = s.items;
}

// ---- per query: off becomes the exclusive prefix over the bins up to the radius h* where the cumulative count reaches k ---------
__global__ __launch_bounds__(64) void radius_kernel(RetArgs a) {
  const int lane = threadIdx.x, tile = blockIdx.x;
  uint32_t* base = a.off + static_cast<size_t>(tile) * a.bins * 64 + lane;
  uint32_t run = 0;
  int hs = -1;
  for (int h0 = 0; h0 < a.bins && hs < 0; h0 += 8) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = h0 + u < a.bins ? base[static_cast<size_t>(h0 + u) * 64] : 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (h0 + u < a.bins && hs < 0) {
        base[static_cast<size_t>(h0 + u) * 64] = run;
        run += v[u];
        if (run >= static_cast<uint32_t>(a.k)) hs = h0 + u;
      }
    }
  }
  a.hstar[tile * 64 + lane] = tile * 64 + lane < a.Q ? hs : -1;      // (k <= N = the sum of a query's bins: always found)
}

// ---- pass 2: the stable counting sort of the items at h <= h* ---------------------------------------------------------------------
// GRADED: the grade of every placed item as well (grade [Q][k] of the batch, saturated at 255), the hit flag from it.
// Its own preamble and its own copy of walk2: with Block and walk2 the k = 100 search of 5000 x 190 834 x 128 bit measured 5.660 /
// 5.667 ms against 5.648 / 5.646 ms of this text (A B A B in one run), past the A-to-A spread; this text compiles to the code it was.
template <int WT, int LT, bool GLOB, bool GRADED = false>
__global__ __launch_bounds__(64) void select_kernel(RetArgs a, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                    const uint32_t* __restrict__ rl, uint8_t* __restrict__ grade) {
  extern __shared__ uint32_t smem[];
  const int lane = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
  const int qa = tile * 64 + lane, q = qa < a.Q ? qa : a.Q - 1;
  uint32_t* image = a.img + (static_cast<size_t>(c) * a.tiles + tile) * a.bins * 64;
  const uint32_t* off = a.off + static_cast<size_t>(tile) * a.bins * 64;
  uint32_t* cur = GLOB ? image : smem;
  Tile<WT, LT> t;
  t.load(a, q, lane, smem + (GLOB ? 0 : a.bins * 64));
  const int hs = a.hstar[tile * 64 + lane];        // -1 behind the last query: such a lane selects nothing
  int hmax = hs;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(hmax, o, 64);
    hmax = hmax > other ? hmax : other;
  }
  // cursor of bin h = items at smaller h (all chunks) + items at h in the chunks before this one
  for (int h = 0; h <= hmax; ++h) cur[h * 64 + lane] = off[h * 64 + lane] + image[h * 64 + lane];
  __syncthreads();
  const int jb = c * a.chunk, je = jb + a.chunk < a.N ? jb + a.chunk : a.N;
  const uint32_t k = static_cast<uint32_t>(a.k);
  auto place = [&](int j, int h) {
    if (h <= hs) {
      const uint32_t p = atomicAdd(&cur[h * 64 + lane], 1u);
      if (p < k) {
        const size_t o = static_cast<size_t>(q) * k + p;
        a.idx[o] = j;
        a.dist[o] = 0.5f * static_cast<float>(h);
        if (GRADED) {
          const uint32_t g = t.overlap(rl + static_cast<size_t>(j) * a.LW);
          grade[o] = static_cast<uint8_t>(g < 255u ? g : 255u);
          if (a.rel) a.rel[o] = g ? 1 : 0;
        } else if (a.rel) {
          a.rel[o] = static_cast<uint8_t>(t.relevant(rl + static_cast<size_t>(j) * a.LW));
        }
      }
    }
  };
  int j = jb;
  if (WT > 0) {
    using G = Group<WT, LT>;
    auto work = [&](const G& g, int j0, int u0, int u1) {
#pragma unroll
      for (int u = u0; u < u1; ++u) place(j0 + u, t.half(g.s + u * WT, g.n + u * WT));
    };
    const int groups = (je - jb) / G::U;
    G ga, gb;                                                       // (walk2, which see)
    int g = 0;
    if (groups > 0) ga.load(rs, rn, rl, jb, false);
    for (; g + 2 <= groups; g += 2, j += 2 * G::U) {
      work(ga, j, 0, 1);
      __builtin_amdgcn_sched_barrier(0);
      gb.load(rs, rn, rl, j + G::U, false);
      __builtin_amdgcn_sched_barrier(0);
      work(ga, j, 1, G::U);
      work(gb, j + G::U, 0, 1);
      __builtin_amdgcn_sched_barrier(0);
      ga.load(rs, rn, rl, g + 2 < groups ? j + 2 * G::U : j, false);
      __builtin_amdgcn_sched_barrier(0);
      work(gb, j + G::U, 1, G::U);
    }
    if (g < groups) { work(ga, j, 0, G::U); j += G::U; }
  }
  for (; j < je; ++j) place(j, t.half(rs + static_cast<size_t>(j) * a.W, rn + static_cast<size_t>(j) * a.W));
}

// ---- the label histogram: per (query tile, chunk) the column image: word [g][lane] = items of the chunk at grade g ----------------
template <int LT>
__global__ __launch_bounds__(64) void grade_kernel(RetArgs a, const uint32_t* __restrict__ rl) {
  extern __shared__ uint32_t smem[];
  const Block b(a);
  const int lane = b.lane;
  uint32_t* image = a.img + b.at;
  uint32_t* col = smem;
  uint32_t* stage = smem + a.bins * 64;
  Tile<0, LT> t;                                                     // no code words (a.W = 0): the label words only
  t.load(a, b.q, lane, stage);
  // the query's label words are cut to `classes` bits: whatever the words hold behind them, 0 <= g <= classes (g indexes the column)
  const int classes = a.bins - 1;
  const uint32_t last = (classes & 31) ? (1u << (classes & 31)) - 1u : 0xffffffffu;
  if (LT > 0) t.l[(LT > 0 ? LT : 1) - 1] &= last;
  else stage[(a.LW - 1) * 64 + lane] &= last;
  for (int g = 0; g < a.bins; ++g) col[g * 64 + lane] = 0u;
  __syncthreads();
  int j = b.jb;
  if (LT > 0) {
    using G = LabelGroup<LT>;
    j = walk2<G>(
        b.jb, b.je, [&](G& g, int j0) { g.load(rl, j0); },
        [&](const G& g, int, int u0, int u1) {
#pragma unroll
          for (int u = u0; u < u1; ++u) atomicAdd(&col[t.overlap(g.l + u * LT) * 64 + lane], 1u);
        });
  }
  for (; j < b.je; ++j) atomicAdd(&col[t.overlap(rl + static_cast<size_t>(j) * a.LW) * 64 + lane], 1u);
  __syncthreads();
  for (int g = 0; g < a.bins; ++g) image[g * 64 + lane] = col[g * 64 + lane];
}

// ---- the images of a tile summed over the chunks -> grade_counts[q][g]
__global__ __launch_bounds__(256) void grade_reduce_kernel(RetArgs a) {
  const Word x(a, a.bins);
  if (x.live && x.valid) a.counts[static_cast<size_t>(x.q) * a.bins + x.h] = sum_chunks(a, x, false, false).items;
}

// ---- images -> bases (cmh_hamming_ap_partial / cmh_hamming_range) -----------------------------------------------------------------
// mAP by counting.  AP needs ranks, not the permutation: for a relevant item j at bin h, with ties by ascending database index,
//   rank(j)    = #{items at h' < h} + #{items at h with index < j} + 1,   relrank(j) = the same over the relevant items,
//   AP = (1 / total) * sum_{relevant j, relrank(j) <= total} relrank(j) / rank(j),   total = min(k, R).
// Pass 1 is hist_kernel.  The three kernels below (REL) turn its images into the two BASES of every (chunk, bin, lane): items /
// relevant items at smaller h in the whole database + at h in earlier shards (`prior`) + at h in earlier chunks of this call.
// ap_kernel then walks its chunk in index order with the packed cursor of hist_kernel in LDS: the returning add gives both positions
// inside the chunk.  The database may be one shard of a larger one: `total` is then the histogram of all shards and `prior` that of
// the shards before.
// Radius search.  Every item at h <= hr, as a ragged list per query in the order (h, database index): the select pass without a k.
// An item j of this call at bin h goes to
//   row_off[q] + #{items of the whole database at h' < h} + #{items at h in earlier shards} + #{items of this call at h, index < j}.
// The same three kernels over the items alone (!REL): every image becomes the 32-bit in-row BASE of its (chunk, bin, lane), for the
// bins up to hr only; range_kernel then walks its chunk in index order with the bases as its private cursors and adds row_off as
// int64 at the store.  lim[q] = the whole database's items at h <= hr: a position at or behind it is never stored (it cannot arise
// from consistent histograms; an inconsistent `total` then loses entries and writes nothing outside the query's own rows).
struct BaseArgs {
  const uint32_t* total;   // [Q][bins][2] of the whole database, or null: this call's own
  const uint32_t* prior;   // [Q][bins][2] of the shards before this one, or null: none
  uint32_t* toti;          // [tiles][bins][64] this call's items per bin -> exclusive prefix over the bins of the whole database
  uint32_t* totr;          // ... the relevant ones (REL)
  uint32_t* brel;          // [S][tiles][bins][64] bases over the relevant items (REL; those over all items replace the images in a.img)
  uint32_t* lim;           // [tiles * 64] REL: min(k, R) per query; else the items of the whole database at h <= hr (0 behind the last query)
  double* part;            // [S][tiles][64] a workgroup's sums (mAP)
  double* ap_sum;          // [Q] (mAP)
  uint32_t k;              // (mAP)
  int hr;                  // the last bin that gets bases: the radius; bins - 1 in the mAP
};

// the images of a tile summed over the chunks -> toti, totr (and counts)
template <bool REL>
__global__ __launch_bounds__(256) void total_kernel(RetArgs a, BaseArgs p) {
  const Word x(a, a.bins);
  if (!x.live) return;
  const Sum s = sum_chunks(a, x, true, false);
  p.toti[x.w] = s.items;
  if (REL) p.totr[x.w] = s.rel;
  put_counts(a, x, s);
}

// per query: toti / totr become the exclusive prefixes over the bins <= hr of the whole database's histogram; lim = min(k, R) / the end
template <bool REL>
__global__ __launch_bounds__(64) void scan_kernel(RetArgs a, BaseArgs p) {
  const int lane = threadIdx.x, tile = blockIdx.x;
  const int qa = tile * 64 + lane, q = qa < a.Q ? qa : a.Q - 1;
  const size_t base = static_cast<size_t>(tile) * a.bins * 64 + lane;
  uint32_t ri = 0, rr = 0;
  for (int h = 0; h <= p.hr; ++h) {
    const size_t t = base + static_cast<size_t>(h) * 64;
    uint32_t ni, nr = 0;
    if (p.total) {
      const uint32_t* c = p.total + (static_cast<size_t>(q) * a.bins + h) * 2;
      nr = c[1];
      ni = c[0] + nr;
    } else {
      ni = p.toti[t];
      if (REL) nr = p.totr[t];
    }
    p.toti[t] = ri;
    if (REL) p.totr[t] = rr;
    ri += ni;
    rr += nr;
  }
  p.lim[tile * 64 + lane] = REL ? (rr < p.k ? rr : p.k) : (qa < a.Q ? ri : 0u);
}

// every image of a bin <= hr becomes the base over all items, brel the base over the relevant ones
template <bool REL>
__global__ __launch_bounds__(256) void base_kernel(RetArgs a, BaseArgs p) {
  const Word x(a, p.hr + 1);
  if (!x.live) return;
  uint32_t bi = p.toti[x.w], br = REL ? p.totr[x.w] : 0u;
  if (p.prior) {
    const uint32_t* c = p.prior + (static_cast<size_t>(x.q) * a.bins + x.h) * 2;
    bi += c[0] + c[1];
    br += c[1];
  }
  for (int c = 0; c < a.S; ++c) {
    const uint32_t v = a.img[c * x.stride + x.w];
    a.img[c * x.stride + x.w] = bi;
    if (REL) p.brel[c * x.stride + x.w] = br;
    bi += v & 0xffffu;
    br += v >> 16;
  }
}

// ---- pass 2 of the mAP: a workgroup's sum of relrank / rank over the relevant items of its chunk ----------------------------------
// Cursors in LDS (hist_kernel's packed word: the histogram pass's occupancy), the bases read from the workspace for relevant items
// only; lanes that meet the same bin read one line of [bin][lane].  GLOB: the bases themselves are the cursors, advanced with global
// atomics (a lane owns its words: the adds of one word come from one lane in index order).
template <int WT, int LT, bool GLOB>
__global__ __launch_bounds__(64) void ap_kernel(RetArgs a, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                const uint32_t* __restrict__ rl, uint32_t* brel_all, const uint32_t* __restrict__ kq,
                                                double* __restrict__ part) {
  extern __shared__ uint32_t smem[];
  const Block b(a);
  const int lane = b.lane;
  uint32_t* bitem = a.img + b.at;
  uint32_t* brel = brel_all + b.at;
  uint32_t* cur = smem;
  Tile<WT, LT> t;
  t.load(a, b.q, lane, smem + (GLOB ? 0 : a.bins * 64));
  if (!GLOB)
    for (int h = 0; h < a.bins; ++h) cur[h * 64 + lane] = 0u;
  __syncthreads();
  const uint32_t total = kq[b.tile * 64 + lane];
  double acc = 0.0;
  auto score = [&](int h, uint32_t r) {
    const int w = h * 64 + lane;
    if (GLOB) {
      const uint32_t pi = atomicAdd(&bitem[w], 1u);
      if (r) {
        const uint32_t pr = atomicAdd(&brel[w], 1u) + 1u;
        if (pr <= total) acc += static_cast<double>(__fdiv_rn(static_cast<float>(pr), static_cast<float>(pi + 1u)));
      }
    } else {
      const uint32_t old = atomicAdd(&cur[w], 1u + (r << 16));
      if (r) {
        const uint32_t pr = brel[w] + (old >> 16) + 1u;
        const uint32_t pi = bitem[w] + (old & 0xffffu) + 1u;
        if (pr <= total) acc += static_cast<double>(__fdiv_rn(static_cast<float>(pr), static_cast<float>(pi)));
      }
    }
  };
  int j = b.jb;
  if (WT > 0) {
    // A workgroup is one wave, and at 4 (2) workgroups per CU a SIMD holds one: nothing hides a wait, so an item at a time (the add's
    // return, then the bases, then the quotient) costs three round trips per item.  A group is therefore worked on in phases, each
    // a run of independent instructions: distances and relevance of its U items; the loads of the bases (they need only the bin);
    // the U returning adds; the quotients.  ONE register set, not walk2's two: the next group's fetch is issued behind the wait for
    // the adds' returns (both count on the same counter: a fetch in flight would be waited for with them) and flies during the
    // quotients.
    using G = Group<WT, LT>;
    const int groups = (b.je - b.jb) / G::U;
    G g;
    if (groups > 0) g.load(rs, rn, rl, b.jb, true);
    for (int gi = 0; gi < groups; ++gi, j += G::U) {
      int w[G::U];
      uint32_t r[G::U], old[G::U], bi[G::U], br[G::U];
#pragma unroll
      for (int u = 0; u < G::U; ++u) {
        w[u] = t.half(g.s + u * WT, g.n + u * WT) * 64 + lane;
        r[u] = LT > 0 ? t.relevant(g.l + u * LT) : t.relevant(rl + static_cast<size_t>(j + u) * a.LW);
      }
#pragma unroll
      for (int u = 0; u < G::U; ++u) {
        bi[u] = br[u] = 0u;
        if (r[u]) { bi[u] = bitem[w[u]]; br[u] = brel[w[u]]; }
      }
#pragma unroll
      for (int u = 0; u < G::U; ++u) old[u] = atomicAdd(&cur[w[u]], 1u + (r[u] << 16));
      asm volatile("" : "+v"(old[G::U - 1]));                       // the wait for the adds' returns sits here (they return in order)
      __builtin_amdgcn_sched_barrier(0);
      g.load(rs, rn, rl, gi + 1 < groups ? j + G::U : j, true);      // (behind the last group: it once more, no branch)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < G::U; ++u) {
        const uint32_t pr = br[u] + (old[u] >> 16) + 1u;
        if (r[u] && pr <= total)
          acc += static_cast<double>(__fdiv_rn(static_cast<float>(pr), static_cast<float>(bi[u] + (old[u] & 0xffffu) + 1u)));
      }
    }
  }
  for (; j < b.je; ++j)
    score(t.half(rs + static_cast<size_t>(j) * a.W, rn + static_cast<size_t>(j) * a.W), t.relevant(rl + static_cast<size_t>(j) * a.LW));
  part[(static_cast<size_t>(b.c) * a.tiles + b.tile) * 64 + lane] = acc;
}

// the chunks' sums added in chunk order
__global__ __launch_bounds__(64) void ap_sum_kernel(RetArgs a, BaseArgs p) {
  const int lane = threadIdx.x, tile = blockIdx.x, q = tile * 64 + lane;
  if (q >= a.Q) return;
  double s = 0.0;
  for (int c = 0; c < a.S; ++c) s += p.part[(static_cast<size_t>(c) * a.tiles + tile) * 64 + lane];
  p.ap_sum[q] = s;
}

// one wave per query: R from the histogram, ap = ap_sum / min(k, R) in float64, rounded to f32 once
__global__ __launch_bounds__(64) void ap_finish_kernel(const double* __restrict__ ap_sum, const uint32_t* __restrict__ counts, int bins,
                                                       uint32_t k, float* __restrict__ ap) {
  const size_t q = blockIdx.x;
  uint32_t r = 0;
  for (int h = threadIdx.x; h < bins; h += 64) r += counts[(q * bins + h) * 2 + 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
  if (threadIdx.x == 0) {
    const uint32_t total = r < k ? r : k;
    ap[q] = total ? static_cast<float>(ap_sum[q] / static_cast<double>(total)) : 0.f;
  }
}

// (((ap[0] + ap[1]) + ...) / Q) in f32 in query order: the mean of the ranking kernel of hamming_map.hip
__global__ __launch_bounds__(64) void ap_mean_kernel(const float* __restrict__ ap, int Q, float* __restrict__ out) {
  __shared__ float buf[1024];
  float acc = 0.f;
  for (int q0 = 0; q0 < Q; q0 += 1024) {
    const int n = Q - q0 < 1024 ? Q - q0 : 1024;
    for (int i = threadIdx.x; i < n; i += 64) buf[i] = ap[q0 + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) acc += buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = acc / static_cast<float>(Q);
}

// ---- pass 2 of the radius search: the stable counting sort of the items at h <= hr into the queries' rows -------------------------
// The cursors are the bases of the bins 0..hr: (hr + 1) * 256 bytes of LDS (GLOB: the bases themselves, advanced with global
// atomics; a lane owns its words).
template <int WT, int LT, bool GLOB>
__global__ __launch_bounds__(64) void range_kernel(RetArgs a, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                   const uint32_t* __restrict__ rl, const int64_t* __restrict__ row_off,
                                                   const uint32_t* __restrict__ ball, int hr, int idx_base) {
  extern __shared__ uint32_t smem[];
  const Block b(a);
  const int lane = b.lane;
  uint32_t* image = a.img + b.at;
  uint32_t* cur = GLOB ? image : smem;
  Tile<WT, LT> t;
  t.load(a, b.q, lane, smem + (GLOB ? 0 : (hr + 1) * 64));
  const int hq = b.valid ? hr : -1;                // a lane behind the last query places nothing
  if (!GLOB)
    for (int h = 0; h <= hr; ++h) cur[h * 64 + lane] = image[h * 64 + lane];
  __syncthreads();
  const int64_t row = row_off[b.q];
  const uint32_t end = ball[b.tile * 64 + lane];
  auto place = [&](int j, int h) {
    if (h <= hq) {
      const uint32_t p = atomicAdd(&cur[h * 64 + lane], 1u);
      if (p < end) {
        const int64_t o = row + static_cast<int64_t>(p);
        a.idx[o] = idx_base + j;
        a.dist[o] = 0.5f * static_cast<float>(h);
        if (a.rel) a.rel[o] = static_cast<uint8_t>(t.relevant(rl + static_cast<size_t>(j) * a.LW));
      }
    }
  };
  int j = b.jb;
  if (WT > 0) {
    using G = Group<WT, LT>;
    j = walk2<G>(
        b.jb, b.je, [&](G& g, int j0) { g.load(rs, rn, rl, j0, false); },
        [&](const G& g, int j0, int u0, int u1) {
#pragma unroll
          for (int u = u0; u < u1; ++u) place(j0 + u, t.half(g.s + u * WT, g.n + u * WT));
        });
  }
  for (; j < b.je; ++j) place(j, t.half(rs + static_cast<size_t>(j) * a.W, rn + static_cast<size_t>(j) * a.W));
}

// ---- ranks of given targets by counting (cmh_hamming_rank) ------------------------------------------------------------------------
// The 0-based position of target t in the stable ranking of query q is #{j : h(q, j) < h(q, t)} + #{j < t : h(q, j) = h(q, t)}: a
// count, so one walk over the database answers it, without columns, sort or list.  A lane holds, for each of its up to GT targets,
// the target's half-distance h_t (rank_target_kernel; -1 = the slot has no target: no distance is below or at it), its bound and
// three full 32-bit counters (a chunk may hold any number of items):
//   less += h < h_t,   ties += h == h_t,   ties_before += (h == h_t) & (j < bound).
// Every (chunk, tile) workgroup leaves its counters [g][3][lane] where the other passes leave their column image (a.bins = 3 * G);
// grade_reduce_kernel adds the chunks in ascending order and writes out[q][g][3] once.

// one thread per (q, g): h_t = Tile::half of query q against its g-th target (same arithmetic, same cut of the last word)
__global__ __launch_bounds__(256) void rank_target_kernel(RetArgs a, const uint32_t* __restrict__ ts, const uint32_t* __restrict__ tn,
                                                          const int32_t* __restrict__ bound, int G, int32_t* __restrict__ ht) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<size_t>(a.Q) * G) return;
  if (bound[i] < 0) { ht[i] = -1; return; }
  const size_t q = i / G;
  const uint32_t last = (a.bits & 31) ? (1u << (a.bits & 31)) - 1u : 0xffffffffu;
  int both = 0, diff = 0;
  for (int w = 0; w < a.W; ++w) {
    const uint32_t nz = a.qn[q * a.W + w] & (w == a.W - 1 ? last : 0xffffffffu) & tn[i * a.W + w];
    both += __popc(nz);
    diff += __popc((a.qs[q * a.W + w] ^ ts[i * a.W + w]) & nz);
  }
  ht[i] = a.bits - both + 2 * diff;
}

template <int WT, int GT>
__global__ __launch_bounds__(64) void rank_kernel(RetArgs a, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                  const int32_t* __restrict__ ht, const int32_t* __restrict__ bound, int G) {
  extern __shared__ uint32_t smem[];
  const Block b(a);
  const int lane = b.lane;
  Tile<WT, LAB_NONE> t;
  t.load(a, b.q, lane, smem);
  __syncthreads();
  int hq[GT], bd[GT];
  uint32_t less[GT], before[GT], ties[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {                 // (G < GT: the slots behind the call's targets are empty ones)
    const bool live = g < G;
    hq[g] = live ? ht[static_cast<size_t>(b.q) * G + g] : -1;
    bd[g] = live ? bound[static_cast<size_t>(b.q) * G + g] : -1;
    less[g] = before[g] = ties[g] = 0u;
  }
  auto count = [&](int j, int h) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const uint32_t eq = h == hq[g] ? 1u : 0u;
      less[g] += h < hq[g] ? 1u : 0u;
      ties[g] += eq;
      before[g] += eq & (j < bd[g] ? 1u : 0u);
    }
  };
  int j = b.jb;
  if (WT > 0) {
    using Gr = Group<WT, LAB_NONE>;
    j = walk2<Gr>(
        b.jb, b.je, [&](Gr& g, int j0) { g.load(rs, rn, nullptr, j0, false); },
        [&](const Gr& g, int j0, int u0, int u1) {
#pragma unroll
          for (int u = u0; u < u1; ++u) count(j0 + u, t.half(g.s + u * WT, g.n + u * WT));
        });
  }
  for (; j < b.je; ++j) count(j, t.half(rs + static_cast<size_t>(j) * a.W, rn + static_cast<size_t>(j) * a.W));
  uint32_t* image = a.img + b.at;
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    if (g < G) {
      image[(g * 3 + 0) * 64 + lane] = less[g];
      image[(g * 3 + 1) * 64 + lane] = before[g];
      image[(g * 3 + 2) * 64 + lane] = ties[g];
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// A call's operands as the entry points receive them (ql, rl: null without labels)
struct Problem {
  const uint32_t *qs, *qn, *ql, *rs, *rn, *rl;
  int Q;
  int64_t N;
  int bits, classes;
};

struct Plan {
  int bins, W, tiles, S, chunk, tb;      // tb = query tiles per batch (the images of one batch fit kImageCap)
  bool glob;
  size_t tile_words() const { return static_cast<size_t>(bins) * 64; }
  size_t bytes() const { return ((static_cast<size_t>(S) + 1) * tb * tile_words() + static_cast<size_t>(tb) * 64) * 4 + 256; }
};

template <class T>
T* aligned256(void* p) { return reinterpret_cast<T*>((reinterpret_cast<uintptr_t>(p) + 255) & ~static_cast<uintptr_t>(255)); }

// CUs of the current device; 256 (MI355X) where none answers (the workspace query also serves callers without a GPU)
int cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      return 256;
    }
    return n;
  }();
  return cus;
}

// The database cut into chunks for `tiles` query tiles whose workgroups hold `lds` bytes of columns (0: none): as many chunks as
// fill the chip's resident slots once (equal work per workgroup: a second, partly filled round would only wait for its last
// members), at least smin, at most smax, none below 256 items.  Resident per CU: what the columns leave of the 160 KiB of LDS.
// -> the number of chunks; *chunk = items per chunk, a multiple of 4.
int cut_chunks(int n, int tiles, size_t lds, int smin, int smax, int* chunk) {
  const int per_cu = lds == 0 ? 8 : static_cast<int>((160 * 1024) / lds) < 8 ? static_cast<int>((160 * 1024) / lds) : 8;
  int s = cu_count() * per_cu / tiles;
  const int by256 = (n + 255) / 256;
  s = s < by256 ? s : by256;
  s = s < smax ? s : smax;
  s = s > smin ? s : smin;
  s = s > 1 ? s : 1;
  *chunk = ((n + s - 1) / s + 3) & ~3;
  return (n + *chunk - 1) / *chunk;
}

// tb = the query tiles whose workspace of per_tile bytes each fits kImageCap
int batch_tiles(size_t per_tile, int tiles) {
  size_t tb = kImageCap / per_tile;
  tb = tb < 1 ? 1 : tb;
  return tb < static_cast<size_t>(tiles) ? static_cast<int>(tb) : tiles;
}

Plan make_plan(int Q, int64_t N, int bits) {
  Plan p;
  p.bins = 2 * bits + 1;
  p.W = (bits + 31) / 32;
  p.glob = bits > kLdsBits;
  p.tiles = (Q + 63) / 64;
  const int n = static_cast<int>(N);
  const int smin = (n + kChunkMax - 1) / kChunkMax;
  const size_t lds = p.glob ? 0 : static_cast<size_t>(p.bins) * 256;
  p.S = cut_chunks(n, p.tiles, lds, smin, p.glob ? 32 : 256, &p.chunk);      // (an image of the wide codes is up to 1 MiB per tile)
  p.tb = batch_tiles((static_cast<size_t>(p.S) + 1) * p.tile_words() * 4, p.tiles);
  return p;
}

// The run-time shape of a call -> the compile-time form of its pass kernels: f(WT, LT, GLOB) as integral constants.
//   GLOB (columns in the workspace): any number of code words, labels none or staged
//   else W in 1..4 code words in registers; label words none (where NONE allows it), 1 (<= 32 classes: MIRFlickr 24, NUS-WIDE 21)
//   or 3 (65..96 classes: MS-COCO 80) in registers, any other number staged.
template <int V>
using Int = std::integral_constant<int, V>;

template <bool NONE, class F>
int dispatch(bool glob, int W, int LW, std::bool_constant<NONE>, F f) {
  auto labels = [&](auto wt, auto gl) {
    if constexpr (NONE)
      if (LW == 0) return f(wt, Int<LAB_NONE>{}, gl);
    if constexpr (!decltype(gl)::value) {
      if (LW == 1) return f(wt, Int<1>{}, gl);
      if (LW == 3) return f(wt, Int<3>{}, gl);
    }
    return f(wt, Int<LAB_ANY>{}, gl);
  };
  if (glob) return labels(Int<0>{}, std::true_type{});
  if (W == 1) return labels(Int<1>{}, std::false_type{});
  if (W == 2) return labels(Int<2>{}, std::false_type{});
  if (W == 3) return labels(Int<3>{}, std::false_type{});
  return labels(Int<4>{}, std::false_type{});
}

// One pass kernel over (query tiles x chunks): lds_bins columns [bin][lane] in LDS plus the form's staged query words.
template <int WT, int LT, class... P, class... A>
int launch_walk(void (*kernel)(RetArgs, P...), int lds_bins, const char* what, const RetArgs& a, hipStream_t st, A... args) {
  const size_t lds = (static_cast<size_t>(lds_bins) * 64 + stage_words(WT, LT, a.W, a.LW)) * 4;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess)
    return fail(CMH_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS", what, lds);
  hipLaunchKernelGGL(kernel, dim3(a.tiles, a.S), dim3(64), lds, st, a, args...);
  CMH_CHECK_LAUNCH(what);
  return CMH_OK;
}

// The limits all entry points share: bits where `codes`, 0 < classes <= cmax where `labels`.  what = null: only the answer (the
// workspace queries leave no message).
int check_shape(const char* what, int Q, int64_t N, int bits, bool codes, int classes, bool labels, int cmax = 32 * kRetMaxWords) {
  auto bad = [&](const char* fmt, auto... v) -> int { return what ? fail(CMH_ERR_INVALID, fmt, what, v...) : CMH_ERR_INVALID; };
  if (Q <= 0 || Q > 65535 || N <= 0) return bad("%s: Q=%d N=%lld", Q, static_cast<long long>(N));
  if (N > kRetMaxN) return bad("%s: N=%lld exceeds %d", static_cast<long long>(N), kRetMaxN);
  if (codes && (bits <= 0 || bits > 32 * kRetMaxWords)) return bad("%s: bits=%d unsupported", bits);
  if (labels && (classes <= 0 || (classes > cmax && cmax != kGradeMax))) return bad("%s: classes=%d unsupported", classes);
  if (labels && classes > cmax) return bad("%s: classes=%d exceeds %d (a grade is one byte)", classes, cmax);
  return CMH_OK;
}

// The query tiles in batches of p.tb.  Per batch: the RetArgs of its queries (operands, images at the head of the workspace, counts),
// the zeroed images of the wide codes, the histogram pass; then body(a, q0, stride) with q0 = the batch's first query and stride =
// the words of one chunk's images, for what the caller makes of the images.
template <class Body>
int for_each_batch(const char* what, const Plan& p, const Problem& pb, uint32_t* counts, void* workspace, hipStream_t st, Body body) {
  RetArgs a = {};
  a.N = static_cast<int>(pb.N); a.bits = pb.bits; a.W = p.W; a.LW = pb.ql ? (pb.classes + 31) / 32 : 0; a.bins = p.bins;
  a.S = p.S; a.chunk = p.chunk;
  a.img = aligned256<uint32_t>(workspace);
  for (int t0 = 0; t0 < p.tiles; t0 += p.tb) {
    const int q0 = t0 * 64;
    a.tiles = p.tiles - t0 < p.tb ? p.tiles - t0 : p.tb;
    a.Q = pb.Q - q0 < a.tiles * 64 ? pb.Q - q0 : a.tiles * 64;
    a.qs = pb.qs + static_cast<size_t>(q0) * a.W;
    a.qn = pb.qn + static_cast<size_t>(q0) * a.W;
    a.ql = pb.ql ? pb.ql + static_cast<size_t>(q0) * a.LW : nullptr;
    a.counts = counts ? counts + static_cast<size_t>(q0) * a.bins * 2 : nullptr;
    const size_t stride = static_cast<size_t>(a.tiles) * p.tile_words();
    if (p.glob && hipMemsetAsync(a.img, 0, static_cast<size_t>(a.S) * stride * 4, st) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "%s: memset failed", what);
    int rc = dispatch(p.glob, a.W, a.LW, std::true_type{}, [&](auto WT, auto LT, auto GLOB) {
      return launch_walk<WT, LT>(hist_kernel<WT, LT, GLOB>, GLOB ? 0 : a.bins, "hamming_hist", a, st, pb.rs, pb.rn, pb.rl);
    });
    if (rc == CMH_OK) rc = body(a, q0, stride);
    if (rc != CMH_OK) return rc;
  }
  return CMH_OK;
}

// hist (k == 0) or hist + select (k > 0)
int run(const char* what, const Problem& pb, int k, int32_t* idx, float* dist, uint8_t* rel, uint8_t* grade, uint32_t* counts,
        void* workspace, size_t workspace_bytes, hipStream_t st) {
  const Plan p = make_plan(pb.Q, pb.N, pb.bits);
  if (!workspace || workspace_bytes < p.bytes()) return fail(CMH_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, p.bytes());
  return for_each_batch(what, p, pb, counts, workspace, st, [&](RetArgs& a, int q0, size_t stride) -> int {
    a.k = k;
    a.off = a.img + static_cast<size_t>(a.S) * stride;
    a.hstar = reinterpret_cast<int32_t*>(a.off + stride);
    a.idx = idx ? idx + static_cast<size_t>(q0) * k : nullptr;
    a.dist = dist ? dist + static_cast<size_t>(q0) * k : nullptr;
    a.rel = rel ? rel + static_cast<size_t>(q0) * k : nullptr;
    hipLaunchKernelGGL(reduce_kernel, dim3(static_cast<unsigned>((stride + 255) / 256)), dim3(256), 0, st, a, k > 0 ? 1 : 0);
    CMH_CHECK_LAUNCH("retrieval reduce");
    if (k <= 0) return CMH_OK;
    hipLaunchKernelGGL(radius_kernel, dim3(a.tiles), dim3(64), 0, st, a);
    CMH_CHECK_LAUNCH("retrieval radius");
    uint8_t* g = grade ? grade + static_cast<size_t>(q0) * k : nullptr;
    return dispatch(p.glob, a.W, a.LW, std::true_type{}, [&](auto WT, auto LT, auto GLOB) {
      constexpr bool kLabels = LT != LAB_NONE;      // (the graded select exists with labels only)
      if (g && !kLabels) return fail(CMH_ERR_INVALID, "retrieval: grades asked for without labels");
      return launch_walk<WT, LT>(g ? select_kernel<WT, LT, GLOB, kLabels> : select_kernel<WT, LT, GLOB>, GLOB ? 0 : a.bins,
                                 "hamming_topk select", a, st, pb.rs, pb.rn, pb.rl, g);
    });
  });
}

// The mAP's workspace per batch of tb query tiles: images (-> bases over the items) and bases over the relevant items [S] each,
// toti, totr, lim, the workgroups' float64 sums.  The batch is sized so that all of it fits kImageCap.
struct ApPlan : Plan {
  size_t per_tile() const { return (2 * static_cast<size_t>(S) + 2) * tile_words() * 4 + 64 * 4 + static_cast<size_t>(S) * 64 * 8; }
  size_t ap_bytes() const { return static_cast<size_t>(tb) * per_tile() + 512; }
};

ApPlan make_ap_plan(int Q, int64_t N, int bits) {
  ApPlan p;
  static_cast<Plan&>(p) = make_plan(Q, N, bits);
  p.tb = batch_tiles(p.per_tile(), p.tiles);
  return p;
}

// total, scan and base over the bins 0..b.hr of a batch: the images become bases
template <bool REL>
int launch_bases(const RetArgs& a, const BaseArgs& b, size_t stride, const char* what, hipStream_t st) {
  hipLaunchKernelGGL(total_kernel<REL>, dim3(static_cast<unsigned>((stride + 255) / 256)), dim3(256), 0, st, a, b);
  hipLaunchKernelGGL(scan_kernel<REL>, dim3(a.tiles), dim3(64), 0, st, a, b);
  const size_t used = static_cast<size_t>(a.tiles) * (b.hr + 1) * 64;
  hipLaunchKernelGGL(base_kernel<REL>, dim3(static_cast<unsigned>((used + 255) / 256)), dim3(256), 0, st, a, b);
  CMH_CHECK_LAUNCH(what);
  return CMH_OK;
}

// hist, the bases, the AP pass and the sum over the chunks
int run_ap(const Problem& pb, uint32_t k, const uint32_t* total, const uint32_t* prior, uint32_t* counts, double* ap_sum, void* workspace,
           hipStream_t st) {
  const ApPlan p = make_ap_plan(pb.Q, pb.N, pb.bits);
  return for_each_batch("hamming_ap_partial", p, pb, counts, workspace, st, [&](RetArgs& a, int q0, size_t stride) -> int {
    const size_t row = static_cast<size_t>(q0) * a.bins * 2;
    BaseArgs b = {};
    b.total = total ? total + row : nullptr;
    b.prior = prior ? prior + row : nullptr;
    b.brel = a.img + static_cast<size_t>(a.S) * stride;
    b.toti = b.brel + static_cast<size_t>(a.S) * stride;
    b.totr = b.toti + stride;
    b.lim = b.totr + stride;
    b.part = aligned256<double>(b.lim + static_cast<size_t>(a.tiles) * 64);
    b.ap_sum = ap_sum + q0;
    b.k = k;
    b.hr = a.bins - 1;
    int rc = launch_bases<true>(a, b, stride, "hamming_ap_partial bases", st);
    if (rc != CMH_OK) return rc;
    rc = dispatch(p.glob, a.W, a.LW, std::false_type{}, [&](auto WT, auto LT, auto GLOB) {
      return launch_walk<WT, LT>(ap_kernel<WT, LT, GLOB>, GLOB ? 0 : a.bins, "hamming_ap_partial", a, st, pb.rs, pb.rn, pb.rl, b.brel,
                                 b.lim, b.part);
    });
    if (rc != CMH_OK) return rc;
    hipLaunchKernelGGL(ap_sum_kernel, dim3(a.tiles), dim3(64), 0, st, a, b);
    CMH_CHECK_LAUNCH("hamming_ap_partial sum");
    return CMH_OK;
  });
}

// hist, the bases and the fill.  The workspace is that of run(): images [S], toti where run() keeps off, lim where it keeps hstar.
int run_range(const Problem& pb, int hr, const uint32_t* total, const uint32_t* prior, const int64_t* row_off, int idx_base, int32_t* idx,
              float* dist, uint8_t* rel, uint32_t* counts, void* workspace, hipStream_t st) {
  const Plan p = make_plan(pb.Q, pb.N, pb.bits);
  return for_each_batch("hamming_range", p, pb, counts, workspace, st, [&](RetArgs& a, int q0, size_t stride) -> int {
    a.idx = idx; a.dist = dist; a.rel = rel;      // (whole buffers: a query's rows start at its row_off)
    const size_t row = static_cast<size_t>(q0) * a.bins * 2;
    BaseArgs b = {};
    b.total = total ? total + row : nullptr;
    b.prior = prior ? prior + row : nullptr;
    b.toti = a.img + static_cast<size_t>(a.S) * stride;
    b.lim = b.toti + stride;
    b.hr = hr;
    const int rc = launch_bases<false>(a, b, stride, "hamming_range bases", st);
    if (rc != CMH_OK) return rc;
    return dispatch(p.glob, a.W, a.LW, std::true_type{}, [&](auto WT, auto LT, auto GLOB) {
      return launch_walk<WT, LT>(range_kernel<WT, LT, GLOB>, GLOB ? 0 : hr + 1, "hamming_range", a, st, pb.rs, pb.rn, pb.rl, row_off + q0,
                                 b.lim, hr, idx_base);
    });
  });
}

struct GradePlan {
  int bins, LW, tiles, S, chunk;
  size_t lds() const { return (static_cast<size_t>(bins) + (LW == 1 || LW == 3 ? 0 : LW)) * 256; }      // columns + staged query words
  size_t bytes() const { return static_cast<size_t>(S) * tiles * bins * 256 + 256; }
};

GradePlan make_grade_plan(int Q, int64_t N, int classes) {
  GradePlan p;
  p.bins = classes + 1;
  p.LW = (classes + 31) / 32;
  p.tiles = (Q + 63) / 64;
  p.S = cut_chunks(static_cast<int>(N), p.tiles, p.lds(), 1, 256, &p.chunk);      // 32-bit counters: no limit on a chunk's items
  return p;
}

constexpr int kRankTargets = 8;            // targets per query and call: the widest form of rank_kernel

// The rank pass keeps no columns, so a workgroup's LDS is the staged query words alone (none with 1..4 code words) and its image is
// the 3 * G counter rows: the chunks only have to fill the chip (32-bit counters: no limit on a chunk's items).
struct RankPlan {
  int W, tiles, S, chunk, G;
  bool staged() const { return W > 4; }
  size_t targets_bytes() const { return align_up(static_cast<size_t>(tiles) * 64 * G * 4, 256); }      // h_t [Q][G]
  size_t bytes() const { return 256 + targets_bytes() + static_cast<size_t>(S) * tiles * 3 * G * 256; }
};

RankPlan make_rank_plan(int Q, int64_t N, int bits, int G) {
  RankPlan p;
  p.W = (bits + 31) / 32;
  p.tiles = (Q + 63) / 64;
  p.G = G;
  p.S = cut_chunks(static_cast<int>(N), p.tiles, p.staged() ? static_cast<size_t>(2 * p.W) * 256 : 0, 1, 1024, &p.chunk);
  return p;
}

int check_rank_shape(const char* what, int Q, int64_t N, int bits, int G) {
  const int rc = check_shape(what, Q, N, bits, true, 0, false);
  if (rc != CMH_OK) return rc;
  if (G < 1 || G > kRankTargets) return what ? fail(CMH_ERR_INVALID, "%s: G=%d outside [1, %d]", what, G, kRankTargets) : CMH_ERR_INVALID;
  return CMH_OK;
}

// the preamble, the walk (WT: 1..4 words in registers, else staged; GT: one target, else eight slots) and the sum over the chunks
int run_rank(const Problem& pb, const uint32_t* ts, const uint32_t* tn, const int32_t* bound, int G, int32_t* out, void* workspace,
             hipStream_t st) {
  const RankPlan p = make_rank_plan(pb.Q, pb.N, pb.bits, G);
  RetArgs a = {};
  a.qs = pb.qs; a.qn = pb.qn;
  a.Q = pb.Q; a.N = static_cast<int>(pb.N); a.bits = pb.bits; a.W = p.W; a.bins = 3 * G; a.tiles = p.tiles; a.S = p.S; a.chunk = p.chunk;
  int32_t* ht = aligned256<int32_t>(workspace);
  a.img = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ht) + p.targets_bytes());
  a.counts = reinterpret_cast<uint32_t*>(out);
  const size_t pairs = static_cast<size_t>(pb.Q) * G;
  hipLaunchKernelGGL(rank_target_kernel, dim3(static_cast<unsigned>((pairs + 255) / 256)), dim3(256), 0, st, a, ts, tn, bound, G, ht);
  CMH_CHECK_LAUNCH("hamming_rank targets");
  const int32_t* hc = ht;
  auto walk = [&](auto WT, auto GT) {
    return launch_walk<WT, LAB_NONE>(rank_kernel<WT, GT>, 0, "hamming_rank", a, st, pb.rs, pb.rn, hc, bound, G);
  };
  auto targets = [&](auto WT) { return G == 1 ? walk(WT, Int<1>{}) : walk(WT, Int<kRankTargets>{}); };
  const int rc = p.staged() ? targets(Int<0>{}) : p.W == 1 ? targets(Int<1>{}) : p.W == 2 ? targets(Int<2>{}) : p.W == 3 ? targets(Int<3>{})
                                                                                                              : targets(Int<4>{});
  if (rc != CMH_OK) return rc;
  const size_t stride = static_cast<size_t>(p.tiles) * a.bins * 64;
  hipLaunchKernelGGL(grade_reduce_kernel, dim3(static_cast<unsigned>((stride + 255) / 256)), dim3(256), 0, st, a);
  CMH_CHECK_LAUNCH("hamming_rank reduce");
  return CMH_OK;
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_retrieval_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return check_shape(nullptr, Q, N, bits, true, 0, false) == CMH_OK ? make_plan(Q, N, bits).bytes() : 0;
}

extern "C" int cmh_hamming_hist(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                                const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                                uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && counts, "hamming_hist: null pointer");
  CMH_CHECK_ARG((q_label == nullptr) == (r_label == nullptr), "hamming_hist: labels on one side only");
  const int rc = check_shape("hamming_hist", Q, N, bits, true, classes, q_label != nullptr);
  if (rc != CMH_OK) return rc;
  return run("hamming_hist", {q_sign, q_nz, q_label, r_sign, r_nz, r_label, Q, N, bits, classes}, 0, nullptr, nullptr, nullptr, nullptr, counts,
             workspace, workspace_bytes, as_stream(stream));
}

extern "C" int cmh_hamming_topk(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                                const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                                int64_t k, int32_t* idx, float* dist, uint8_t* rel, uint32_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && idx && dist, "hamming_topk: null pointer");
  CMH_CHECK_ARG((q_label == nullptr) == (r_label == nullptr), "hamming_topk: labels on one side only");
  CMH_CHECK_ARG(!rel || q_label, "hamming_topk: hit flags asked for without labels");
  CMH_CHECK_ARG(k >= 1 && k <= CMH_TOPK_MAX, "hamming_topk: k=%lld outside [1, %d]", static_cast<long long>(k), CMH_TOPK_MAX);
  const int rc = check_shape("hamming_topk", Q, N, bits, true, classes, q_label != nullptr);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k <= N, "hamming_topk: k=%lld exceeds N=%lld", static_cast<long long>(k), static_cast<long long>(N));
  return run("hamming_topk", {q_sign, q_nz, q_label, r_sign, r_nz, r_label, Q, N, bits, classes}, static_cast<int>(k), idx, dist, rel,
             nullptr, counts, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int cmh_hamming_topk_graded(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                                       const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits,
                                       int32_t classes, int64_t k, int32_t* idx, float* dist, uint8_t* rel, uint8_t* grade,
                                       uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && idx && dist && grade, "hamming_topk_graded: null pointer");
  CMH_CHECK_ARG(q_label && r_label, "hamming_topk_graded: grades need the labels of both sides");
  CMH_CHECK_ARG(k >= 1 && k <= CMH_TOPK_MAX, "hamming_topk_graded: k=%lld outside [1, %d]", static_cast<long long>(k), CMH_TOPK_MAX);
  const int rc = check_shape("hamming_topk_graded", Q, N, bits, true, classes, true, kGradeMax);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k <= N, "hamming_topk_graded: k=%lld exceeds N=%lld", static_cast<long long>(k), static_cast<long long>(N));
  return run("hamming_topk_graded", {q_sign, q_nz, q_label, r_sign, r_nz, r_label, Q, N, bits, classes}, static_cast<int>(k), idx, dist,
             rel, grade, counts, workspace, workspace_bytes, as_stream(stream));
}

extern "C" size_t cmh_map_count_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return check_shape(nullptr, Q, N, bits, true, 0, false) == CMH_OK ? make_ap_plan(Q, N, bits).ap_bytes() : 0;
}

extern "C" int cmh_hamming_ap_partial(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                                      const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits,
                                      int32_t classes, int64_t topk, const uint32_t* total_counts, const uint32_t* prior_counts,
                                      uint32_t* counts_out, double* ap_sum, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && ap_sum, "hamming_ap_partial: null pointer");
  CMH_CHECK_ARG(q_label && r_label, "hamming_ap_partial: AP needs the labels of both sides");
  const int rc = check_shape("hamming_ap_partial", Q, N, bits, true, classes, true);
  if (rc != CMH_OK) return rc;
  const size_t need = make_ap_plan(Q, N, bits).ap_bytes();
  CMH_CHECK_ARG(workspace && workspace_bytes >= need, "hamming_ap_partial: workspace %zu < %zu bytes", workspace_bytes, need);
  const uint32_t k = topk <= 0 || topk > INT32_MAX ? static_cast<uint32_t>(INT32_MAX) : static_cast<uint32_t>(topk);      // (R <= 2^31 - 1)
  return run_ap({q_sign, q_nz, q_label, r_sign, r_nz, r_label, Q, N, bits, classes}, k, total_counts, prior_counts, counts_out, ap_sum,
                workspace, as_stream(stream));
}

extern "C" int cmh_ap_finish(const double* ap_sum, const uint32_t* total_counts, int32_t Q, int32_t bits, int64_t topk, float* ap,
                             float* map, void* stream) {
  CMH_CHECK_ARG(ap_sum && total_counts && ap && map, "ap_finish: null pointer");
  CMH_CHECK_ARG(Q > 0, "ap_finish: Q=%d", Q);
  CMH_CHECK_ARG(bits > 0 && bits <= 32 * kRetMaxWords, "ap_finish: bits=%d unsupported", bits);
  const uint32_t k = topk <= 0 || topk > INT32_MAX ? static_cast<uint32_t>(INT32_MAX) : static_cast<uint32_t>(topk);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ap_finish_kernel, dim3(Q), dim3(64), 0, st, ap_sum, total_counts, 2 * bits + 1, k, ap);
  CMH_CHECK_LAUNCH("ap_finish");
  hipLaunchKernelGGL(ap_mean_kernel, dim3(1), dim3(64), 0, st, ap, Q, map);
  CMH_CHECK_LAUNCH("ap_finish mean");
  return CMH_OK;
}

extern "C" size_t cmh_range_workspace_bytes(int32_t Q, int64_t N, int32_t bits) { return cmh_retrieval_workspace_bytes(Q, N, bits); }

extern "C" int cmh_hamming_range(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* q_label, const uint32_t* r_sign,
                                 const uint32_t* r_nz, const uint32_t* r_label, int32_t Q, int64_t N, int32_t bits, int32_t classes,
                                 int32_t radius_h, const uint32_t* total_counts, const uint32_t* prior_counts, const int64_t* row_off,
                                 int32_t idx_base, int32_t* idx, float* dist, uint8_t* rel, uint32_t* counts_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && row_off && idx && dist, "hamming_range: null pointer");
  CMH_CHECK_ARG((q_label == nullptr) == (r_label == nullptr), "hamming_range: labels on one side only");
  CMH_CHECK_ARG(!rel || q_label, "hamming_range: hit flags asked for without labels");
  const int rc = check_shape("hamming_range", Q, N, bits, true, classes, q_label != nullptr);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(radius_h >= 0 && radius_h <= 2 * bits, "hamming_range: radius_h=%d outside [0, %d]", radius_h, 2 * bits);
  CMH_CHECK_ARG(idx_base >= 0 && idx_base <= INT32_MAX - static_cast<int32_t>(N), "hamming_range: idx_base=%d with N=%lld passes 2^31 - 1",
                idx_base, static_cast<long long>(N));
  const size_t need = make_plan(Q, N, bits).bytes();
  CMH_CHECK_ARG(workspace && workspace_bytes >= need, "hamming_range: workspace %zu < %zu bytes", workspace_bytes, need);
  return run_range({q_sign, q_nz, q_label, r_sign, r_nz, r_label, Q, N, bits, classes}, radius_h, total_counts, prior_counts, row_off,
                   idx_base, idx, dist, rel, counts_out, workspace, as_stream(stream));
}

extern "C" size_t cmh_rank_workspace_bytes(int32_t Q, int64_t N, int32_t bits, int32_t G) {
  return check_rank_shape(nullptr, Q, N, bits, G) == CMH_OK ? make_rank_plan(Q, N, bits, G).bytes() : 0;
}

extern "C" int cmh_hamming_rank(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q,
                                int64_t N, int32_t bits, const uint32_t* t_sign, const uint32_t* t_nz, const int32_t* bound, int32_t G,
                                int32_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && t_sign && t_nz && bound && out, "hamming_rank: null pointer");
  const int rc = check_rank_shape("hamming_rank", Q, N, bits, G);
  if (rc != CMH_OK) return rc;
  const size_t need = make_rank_plan(Q, N, bits, G).bytes();
  CMH_CHECK_ARG(workspace && workspace_bytes >= need, "hamming_rank: workspace %zu < %zu bytes", workspace_bytes, need);
  return run_rank({q_sign, q_nz, nullptr, r_sign, r_nz, nullptr, Q, N, bits, 0}, t_sign, t_nz, bound, G, out, workspace, as_stream(stream));
}

extern "C" size_t cmh_label_overlap_workspace_bytes(int32_t Q, int64_t N, int32_t classes) {
  return check_shape(nullptr, Q, N, 0, false, classes, true, kGradeMax) == CMH_OK ? make_grade_plan(Q, N, classes).bytes() : 0;
}

extern "C" int cmh_label_overlap_hist(const uint32_t* q_label, const uint32_t* r_label, int32_t Q, int64_t N, int32_t classes,
                                      uint32_t* grade_counts, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_label && r_label && grade_counts, "label_overlap_hist: null pointer");
  int rc = check_shape("label_overlap_hist", Q, N, 0, false, classes, true, kGradeMax);
  if (rc != CMH_OK) return rc;
  const GradePlan p = make_grade_plan(Q, N, classes);
  if (!workspace || workspace_bytes < p.bytes())
    return fail(CMH_ERR_WORKSPACE, "label_overlap_hist: workspace %zu < %zu bytes", workspace_bytes, p.bytes());
  hipStream_t st = as_stream(stream);
  RetArgs a = {};
  a.ql = q_label;
  a.Q = Q; a.N = static_cast<int>(N); a.bits = 32; a.W = 0; a.LW = p.LW; a.bins = p.bins; a.tiles = p.tiles; a.S = p.S; a.chunk = p.chunk;
  a.img = aligned256<uint32_t>(workspace);
  a.counts = grade_counts;
  const char* what = "label_overlap_hist";
  rc = p.LW == 1   ? launch_walk<0, 1>(grade_kernel<1>, a.bins, what, a, st, r_label)
       : p.LW == 3 ? launch_walk<0, 3>(grade_kernel<3>, a.bins, what, a, st, r_label)
                   : launch_walk<0, LAB_ANY>(grade_kernel<LAB_ANY>, a.bins, what, a, st, r_label);
  if (rc != CMH_OK) return rc;
  const size_t stride = static_cast<size_t>(p.tiles) * p.bins * 64;
  hipLaunchKernelGGL(grade_reduce_kernel, dim3(static_cast<unsigned>((stride + 255) / 256)), dim3(256), 0, st, a);
  CMH_CHECK_LAUNCH("label_overlap_hist reduce");
  return CMH_OK;
}
