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
// why the text is not shared: there the query words are per lane and the item words uniform), the same stable counting sort
// (written in retrieval_few.h, which retrieval_soft.hip runs with another distance; this file supplies HammingRule):
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
// cmh_hamming_topk_few_masked is the same search over the items an allow-mask admits (retrieval_few.h: MASKED).
#include "retrieval_few.h"

namespace cmh {
namespace {

constexpr int kFewGroup = 16;                        // queries per workgroup: the LDS rows of one wave
constexpr int kFewWavesPerCu = 8;

// calc_hammingDist in half-units as the rule of the pipeline (retrieval_few.h)
struct HammingRule {
  using Out = float;
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
  // half-units of calc_hammingDist against a query (its words are wave-uniform, the nz words cut to `bits` bits)
  template <int W>
  static __device__ __forceinline__ int bin(const Item<W>& r, const Query<W>& q, int bits) {
    int both = 0, diff = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t nz = q.n[w] & r.n[w];
      both += __popc(nz);
      diff += __popc((q.s[w] ^ r.s[w]) & nz);
    }
    return bits - both + 2 * diff;
  }
  static __device__ __forceinline__ float out(int h) { return 0.5f * static_cast<float>(h); }
  static float pad() { return __builtin_inff(); }
};

// As many chunks as fill the chip's wave slots once, none below 256 items (a small database is cut as cut_chunks of retrieval.hip
// cuts it); at most 2048 / groups chunks of at most 64.25 KiB per chunk: 33 MiB, so the image cap never binds on a 256-CU chip; it
// is what bounds the count on a larger one.
FewPlan hamming_plan(int Q, int64_t N, int bits) { return make_few_plan(Q, N, bits, 2 * bits + 1, kFewGroup, kFewWavesPerCu, 256); }

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" size_t cmh_topk_few_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return check_few_shape(nullptr, Q, N, bits) == CMH_OK ? hamming_plan(Q, N, bits).bytes(Q) : 0;
}

extern "C" int cmh_hamming_topk_few(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q,
                                    int64_t N, int32_t bits, int32_t k, int32_t* idx, float* dist, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && idx && dist, "hamming_topk_few: null pointer");
  const int rc = check_few_shape("hamming_topk_few", Q, N, bits);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 1 && k <= CMH_FEW_K_MAX, "hamming_topk_few: k=%d outside [1, %d]", k, CMH_FEW_K_MAX);
  CMH_CHECK_ARG(k <= N, "hamming_topk_few: k=%d exceeds N=%lld", k, static_cast<long long>(N));
  const FewPlan p = hamming_plan(Q, N, bits);
  const uintptr_t row = few_row_bytes(p.W);
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "hamming_topk_few: database planes of %d words per row must be aligned to %d bytes", p.W, static_cast<int>(row));
  if (!workspace || workspace_bytes < p.bytes(Q))
    return fail(CMH_ERR_WORKSPACE, "hamming_topk_few: workspace %zu < %zu bytes", workspace_bytes, p.bytes(Q));
  const FewArgs a = few_args(p, Q, N, bits, k, idx, dist, workspace);
  return run_few<HammingRule>("hamming_topk_few", a, p, q_sign, q_nz, r_sign, r_nz, as_stream(stream));
}

extern "C" size_t cmh_topk_few_masked_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return cmh_topk_few_workspace_bytes(Q, N, bits);      // (the filter adds nothing to the workspace: one plan for both)
}

extern "C" int cmh_hamming_topk_few_masked(const uint32_t* q_sign, const uint32_t* q_nz, const uint32_t* r_sign, const uint32_t* r_nz,
                                           const uint64_t* allow, int32_t Q, int64_t N, int32_t bits, int32_t k, int32_t* idx, float* dist,
                                           int32_t* found, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_nz && r_sign && r_nz && idx && dist, "hamming_topk_few_masked: null pointer");
  int rc = check_few_mask("hamming_topk_few_masked", allow, found);
  if (rc != CMH_OK) return rc;
  if ((rc = check_few_shape("hamming_topk_few_masked", Q, N, bits)) != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 1 && k <= CMH_FEW_K_MAX, "hamming_topk_few_masked: k=%d outside [1, %d]", k, CMH_FEW_K_MAX);
  CMH_CHECK_ARG(k <= N, "hamming_topk_few_masked: k=%d exceeds N=%lld", k, static_cast<long long>(N));
  const FewPlan p = hamming_plan(Q, N, bits);
  const uintptr_t row = few_row_bytes(p.W);
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "hamming_topk_few_masked: database planes of %d words per row must be aligned to %d bytes", p.W, static_cast<int>(row));
  if (!workspace || workspace_bytes < p.bytes(Q))
    return fail(CMH_ERR_WORKSPACE, "hamming_topk_few_masked: workspace %zu < %zu bytes", workspace_bytes, p.bytes(Q));
  const FewArgs a = few_args(p, Q, N, bits, k, idx, dist, workspace);
  return run_few<HammingRule>("hamming_topk_few_masked", a, p, q_sign, q_nz, r_sign, r_nz, as_stream(stream), allow, found);
}
