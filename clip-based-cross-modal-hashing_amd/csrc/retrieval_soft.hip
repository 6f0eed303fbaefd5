// Soft-query search (cmh_soft_query_planes, cmh_soft_topk): the packed database ranked by the head's REAL-VALUED output instead of
// its sign.  calc_hammingDist = 0.5 (K - q . r) (utils/calc_utils.py:8-13) is defined for any real q; on the head's output u it is
// the asymmetric distance of the hashing literature: a bit the head was unsure about costs little when it disagrees, a confident
// one a lot.  Nothing is stored per item: the database stays the sign / nz planes of cmh_pack_codes.
//
// The query is quantised to integer weights w_i = rint(u_i / max|u| * 15) in [-15, 15] (three f32 operations, each rounded once),
// held as a sign plane and the four bit planes P_0..P_3 of |w|.  Against an item r in {-1, 0, +1}^K
//   wdist = sum |w_i| - sum w_i r_i = sum_{r_i = 0} |w_i| + 2 sum_{r_i != 0, sign differs} |w_i|
//         = sum_b 2^b (popc(P_b & ~r_nz) + 2 popc(P_b & r_nz & (q_sign ^ r_sign)))      per word,
// an integer in [0, 30 bits]: pure VALU on wave-uniform query words, and the stable counting sort of retrieval_few.h (lanes own
// items; histogram -> radius -> bases -> placement) carries over with 30 bits + 1 bins in place of 2 bits + 1.  Exact, independent
// of any summation order, bit-reproducible.
//
// A query's histogram row is 4 (30 bits + 1) bytes of LDS: 15 KiB at 128 bit against the Hamming search's 1 KiB, so fewer queries
// share a workgroup (soft_group: as many as fit kSoftLdsBudget: 1 at 128 bit, 2 at 64 bit, 4 at 32 bit, 8 at 16 bit), and a chunk
// holds at least kSoftMinChunk items against the Hamming search's 256: the image a chunk leaves in the workspace is that much
// larger, and zeroing, storing and summing it is paid per chunk.
//
// Behind the search, in the second half of this file: cmh_soft_ap, the mAP, relevant counts and rank sums of soft queries over the
// whole database by counting (two counters per bin on the same pipeline).
#include <cstdlib>

#include "retrieval_few.h"

namespace cmh {
namespace {

constexpr int kSoftPlanes = 4;                       // bit planes of |w| <= CMH_SOFT_LEVELS = 15
constexpr int kSoftLdsBudget = 16 << 10;             // bytes of histogram rows per workgroup (measured: DESIGN.md 9.7)
constexpr int kSoftMinChunk = 1024;                  // the fewest items of a chunk (measured there too)
constexpr int kSoftLdsMax = 64 << 10;                // what a launch takes without asking for more
constexpr int kSoftGroupMax = 16;
constexpr int kLdsPerCu = 160 << 10;
static_assert(CMH_SOFT_LEVELS == (1 << kSoftPlanes) - 1, "the planes hold |w| <= CMH_SOFT_LEVELS");

int soft_bins(int bits) { return 2 * CMH_SOFT_LEVELS * bits + 1; }

// Two diagnostic pins for the A/B of tools/retrieval_bench.py --soft (results never depend on either): CMH_SOFT_GROUP = queries per
// workgroup, CMH_SOFT_MIN_CHUNK = the fewest items of a chunk.  0 / unset: the plan's own choice.
int soft_pin(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : 0;
}

// Queries per workgroup: as many histogram rows as fit kSoftLdsBudget, within what one workgroup's LDS holds
int soft_group(int bits) {
  static const int pinned = soft_pin("CMH_SOFT_GROUP");
  const int row = soft_bins(bits) * 4, most = kSoftLdsMax / row < kSoftGroupMax ? kSoftLdsMax / row : kSoftGroupMax;
  int g = pinned > 0 ? pinned : kSoftLdsBudget / row;
  g = g < most ? g : most;
  return g > 1 ? g : 1;
}

FewPlan soft_plan(int Q, int64_t N, int bits) {
  static const int pinned = soft_pin("CMH_SOFT_MIN_CHUNK");
  const int bins = soft_bins(bits), group = soft_group(bits);
  const int by_lds = kLdsPerCu / (group * bins * 4);
  return make_few_plan(Q, N, bits, bins, group, by_lds < 8 ? by_lds : 8, pinned > 0 ? pinned : kSoftMinChunk);
}

struct SoftRule {
  using Out = int32_t;
  // A query's sign words, the planes of |w| cut to `bits` bits, and its radius: wave-uniform, in scalar registers
  template <int W>
  struct Query {
    uint32_t s[W], m[kSoftPlanes][W];
    int hs;
    __device__ __forceinline__ void load(const uint32_t* __restrict__ qs, const uint32_t* __restrict__ qm, const int32_t* __restrict__ hstar,
                                         int q, uint32_t last) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        s[w] = qs[q * W + w];
#pragma unroll
        for (int b = 0; b < kSoftPlanes; ++b) m[b][w] = qm[(q * kSoftPlanes + b) * W + w] & (w == W - 1 ? last : 0xffffffffu);
      }
      hs = hstar ? hstar[q] : 0;
    }
  };
  template <int W>
  static __device__ __forceinline__ int bin(const Item<W>& r, const Query<W>& q, int) {
    int zero[kSoftPlanes] = {}, flip[kSoftPlanes] = {};
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t off = ~r.n[w], x = (q.s[w] ^ r.s[w]) & r.n[w];
#pragma unroll
      for (int b = 0; b < kSoftPlanes; ++b) {
        zero[b] += __popc(q.m[b][w] & off);
        flip[b] += __popc(q.m[b][w] & x);
      }
    }
    int d = 0;
#pragma unroll
    for (int b = 0; b < kSoftPlanes; ++b) d += (zero[b] + 2 * flip[b]) << b;
    return d;
  }
  static __device__ __forceinline__ int32_t out(int d) { return d; }
  static int32_t pad() { return INT32_MAX; }
};

// ---- the quantiser: one wave per query row, lane l holds entries l and l + 64 ---------------------------------------------------------
__global__ __launch_bounds__(64) void soft_query_planes_kernel(const float* __restrict__ u, int bits, int W, uint32_t* __restrict__ q_sign,
                                                               uint32_t* __restrict__ q_mag, int32_t* __restrict__ wsum,
                                                               float* __restrict__ scale, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x, q = blockIdx.x;
  const float* row = u + static_cast<size_t>(q) * bits;
  float v[2];
  bool finite = true;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = lane + 64 * t;
    v[t] = i < bits ? row[i] : 0.f;
    finite = finite && fabsf(v[t]) <= 3.402823466e+38f;      // false for NaN and +-Inf
    s = fmaxf(s, fabsf(v[t]));
  }
  finite = __ballot(!finite) == 0;                            // the row's: a row with a bad entry gets zero weights
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = fmaxf(s, __shfl_xor(s, o, 64));      // (a maximum: no rounding, no order)
  int sum = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    int w = 0;
    if (finite && s > 0.f) w = static_cast<int>(rintf(__fmul_rn(__fdiv_rn(v[t], s), static_cast<float>(CMH_SOFT_LEVELS))));
    const int mag = w < 0 ? -w : w;
    sum += mag;
    const uint64_t pos = __ballot(w > 0);
    uint64_t plane[kSoftPlanes];
#pragma unroll
    for (int b = 0; b < kSoftPlanes; ++b) plane[b] = __ballot((mag >> b) & 1);
    // lane 0 / 1 write the two words of this half (entries 64 t .. 64 t + 63) that lie inside the row's W words
    if (lane < 2 && 2 * t + lane < W) {
      const int word = 2 * t + lane, sh = 32 * lane;
      q_sign[q * W + word] = static_cast<uint32_t>(pos >> sh);
#pragma unroll
      for (int b = 0; b < kSoftPlanes; ++b) q_mag[(q * kSoftPlanes + b) * W + word] = static_cast<uint32_t>(plane[b] >> sh);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) {
    wsum[q] = sum;
    scale[q] = finite ? s : 0.f;
    if (!finite) *bad = 1;
  }
}

int check_soft_topk(const char* what, int Q, int64_t N, int bits) {
  static_assert(CMH_SOFT_Q_MAX == CMH_FEW_Q_MAX && CMH_SOFT_BITS_MAX == CMH_FEW_BITS_MAX, "the limits of the shared pipeline");
  return check_few_shape(what, Q, N, bits);
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" int cmh_soft_query_planes(const float* u, int32_t Q, int32_t bits, uint32_t* q_sign, uint32_t* q_mag, int32_t* wsum,
                                     float* scale, int32_t* bad, void* stream) {
  CMH_CHECK_ARG(u && q_sign && q_mag && wsum && scale && bad, "soft_query_planes: null pointer");
  CMH_CHECK_ARG(Q >= 1 && Q <= 65535, "soft_query_planes: Q=%d outside [1, 65535]", Q);
  CMH_CHECK_ARG(bits >= 1 && bits <= CMH_SOFT_BITS_MAX, "soft_query_planes: bits=%d outside [1, %d]", bits, CMH_SOFT_BITS_MAX);
  hipLaunchKernelGGL(soft_query_planes_kernel, dim3(Q), dim3(64), 0, as_stream(stream), u, bits, (bits + 31) / 32, q_sign, q_mag, wsum,
                     scale, bad);
  CMH_CHECK_LAUNCH("soft_query_planes");
  return CMH_OK;
}

extern "C" size_t cmh_soft_topk_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return check_soft_topk(nullptr, Q, N, bits) == CMH_OK ? soft_plan(Q, N, bits).bytes(Q) : 0;
}

extern "C" int cmh_soft_topk(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz, int32_t Q,
                             int64_t N, int32_t bits, int32_t k, int32_t* idx, int32_t* wdist, void* workspace, size_t workspace_bytes,
                             void* stream) {
  CMH_CHECK_ARG(q_sign && q_mag && r_sign && r_nz && idx && wdist, "soft_topk: null pointer");
  const int rc = check_soft_topk("soft_topk", Q, N, bits);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 1 && k <= CMH_SOFT_K_MAX, "soft_topk: k=%d outside [1, %d]", k, CMH_SOFT_K_MAX);
  CMH_CHECK_ARG(k <= N, "soft_topk: k=%d exceeds N=%lld", k, static_cast<long long>(N));
  const FewPlan p = soft_plan(Q, N, bits);
  const uintptr_t row = few_row_bytes(p.W);
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "soft_topk: database planes of %d words per row must be aligned to %d bytes", p.W, static_cast<int>(row));
  if (!workspace || workspace_bytes < p.bytes(Q))
    return fail(CMH_ERR_WORKSPACE, "soft_topk: workspace %zu < %zu bytes", workspace_bytes, p.bytes(Q));
  const FewArgs a = few_args(p, Q, N, bits, k, idx, wdist, workspace);
  return run_few<SoftRule>("soft_topk", a, p, q_sign, q_mag, r_sign, r_nz, as_stream(stream));
}

extern "C" size_t cmh_soft_topk_masked_workspace_bytes(int32_t Q, int64_t N, int32_t bits) {
  return cmh_soft_topk_workspace_bytes(Q, N, bits);      // (the filter adds nothing to the workspace: one plan for both)
}

extern "C" int cmh_soft_topk_masked(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz,
                                    const uint64_t* allow, int32_t Q, int64_t N, int32_t bits, int32_t k, int32_t* idx, int32_t* wdist,
                                    int32_t* found, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(q_sign && q_mag && r_sign && r_nz && idx && wdist, "soft_topk_masked: null pointer");
  int rc = check_few_mask("soft_topk_masked", allow, found);
  if (rc != CMH_OK) return rc;
  if ((rc = check_soft_topk("soft_topk_masked", Q, N, bits)) != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 1 && k <= CMH_SOFT_K_MAX, "soft_topk_masked: k=%d outside [1, %d]", k, CMH_SOFT_K_MAX);
  CMH_CHECK_ARG(k <= N, "soft_topk_masked: k=%d exceeds N=%lld", k, static_cast<long long>(N));
  const FewPlan p = soft_plan(Q, N, bits);
  const uintptr_t row = few_row_bytes(p.W);
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "soft_topk_masked: database planes of %d words per row must be aligned to %d bytes", p.W, static_cast<int>(row));
  if (!workspace || workspace_bytes < p.bytes(Q))
    return fail(CMH_ERR_WORKSPACE, "soft_topk_masked: workspace %zu < %zu bytes", workspace_bytes, p.bytes(Q));
  const FewArgs a = few_args(p, Q, N, bits, k, idx, wdist, workspace);
  return run_few<SoftRule>("soft_topk_masked", a, p, q_sign, q_mag, r_sign, r_nz, as_stream(stream), allow, found);
}

// ==== mAP, R and the rank sum of soft queries over the WHOLE database, by counting (cmh_soft_ap) =====================
// AP needs the rank of every relevant item and its rank among the relevant ones, not a permutation.  In (wdist, database index)
// order both are counts:
//   rank(j)    = items in lower bins + items of j's bin in earlier chunks + ... in earlier slabs of j's chunk + ... on lower lanes + 1
//   relrank(j) = the same over the relevant items
// so the pipeline is retrieval_few.h's with TWO counters per bin (all items, relevant items), kept as two histogram rows per query:
// the kernels few_total / few_base and the prefix of few_radius run over 2 Q rows unchanged.
//   soft_ap_rel       rel[j] = one 64-bit word per item, bit q = item j shares a label with query q of this call (the lanes load their
//                     items' label words, the queries' are wave-uniform): every later walk reads 8 bytes per item whatever the
//                     number of classes, and a (chunk, group) never touches label words again
//   soft_ap_pass<0>   the histograms img[chunk][q][all | relevant][bin]
//   few_total, soft_ap_prefix (tot -> exclusive prefixes over the bins, R = the relevant row's sum), few_base
//   soft_ap_pass<1>   the walk again in index order with the bases as cursors.  Only RELEVANT lanes need positions, and a lane that
//                     is alone in its bin within its 64-item slab (the cursor moves by 1 under the slab's order-free LDS adds) reads
//                     them off the cursors as they stood before the slab.  Lanes that share a bin take one wave-uniform turn per
//                     distinct shared bin; the turn ballots the valid lanes of that bin (rank) and the relevant ones (relrank).  A
//                     lane adds its own terms, in index order, to its own float64 / int64 slot in LDS; a fixed xor tree over the
//                     lanes closes the chunk -> psum, prank [chunk][q]
//   soft_ap_finish    the chunks added in chunk order; ap = sum / min(k, R) in float64, rounded to f32 once
// No atomics on any output and no order that depends on timing: two calls give equal bytes.
namespace cmh {
namespace {

constexpr int kApLdsBudget = 32 << 10;      // bytes of counter rows per workgroup: kSoftLdsBudget's queries, two rows each

struct ApArgs {
  FewArgs f;                 // over 2 Q rows: f.Q = 2 Q, f.group = 2 (queries per workgroup); row 2 q = all items, 2 q + 1 = relevant
  int Q, k;
  const uint64_t* rel;       // [N]
  uint32_t* R;               // [Q]
  double* psum;              // [S][Q]
  long long* prank;          // [S][Q]
};

struct ApPlan {
  FewPlan p;                 // of the 2 Q rows
  int group;                 // queries per workgroup
  size_t words(int Q) const {
    return static_cast<size_t>(p.S) * 2 * Q * p.bins + static_cast<size_t>(2 * Q) * p.bins * (1 + kFewParts) + 3 * CMH_SOFT_Q_MAX;
  }
  size_t bytes(int Q, int64_t N) const {
    return words(Q) * 4 + static_cast<size_t>(p.S) * Q * 16 + static_cast<size_t>(N) * 8 + 3 * 256;
  }
};

ApPlan soft_ap_plan(int Q, int64_t N, int bits) {
  const int bins = soft_bins(bits), row = bins * 8;
  int g = kApLdsBudget / row < kSoftGroupMax ? kApLdsBudget / row : kSoftGroupMax;
  g = g > 1 ? g : 1;
  const int lds = g * (row + 64 * 16), by_lds = kLdsPerCu / lds;
  ApPlan a;
  a.group = g;
  a.p = make_few_plan(2 * Q, N, bits, bins, 2 * g, by_lds < 8 ? by_lds : 8, kSoftMinChunk);
  return a;
}

template <class T>
T* ap_aligned(void* p) {
  return reinterpret_cast<T*>((reinterpret_cast<uintptr_t>(p) + 255) & ~static_cast<uintptr_t>(255));
}

ApArgs soft_ap_args(const ApPlan& pl, int Q, int64_t N, int bits, int k, void* workspace) {
  const FewPlan& p = pl.p;
  ApArgs a = {};
  FewArgs& f = a.f;
  f.Q = 2 * Q; f.bits = bits; f.W = p.W; f.bins = p.bins; f.S = p.S; f.L = p.L; f.chunk = p.chunk; f.k = k; f.group = p.group; f.N = N;
  f.img = ap_aligned<uint32_t>(workspace);
  f.tot = f.img + static_cast<size_t>(p.S) * 2 * Q * p.bins;
  f.ppre = f.tot + static_cast<size_t>(2 * Q) * p.bins;
  f.hstar = reinterpret_cast<int32_t*>(f.ppre + static_cast<size_t>(2 * Q) * p.bins * kFewParts);      // [2 Q]
  a.R = reinterpret_cast<uint32_t*>(f.hstar + 2 * CMH_SOFT_Q_MAX);                                        // [Q]
  a.psum = ap_aligned<double>(a.R + CMH_SOFT_Q_MAX);
  a.prank = reinterpret_cast<long long*>(a.psum + static_cast<size_t>(p.S) * Q);
  a.rel = ap_aligned<uint64_t>(a.prank + static_cast<size_t>(p.S) * Q);
  a.Q = Q; a.k = k;
  return a;
}

// ---- one thread per item: the 64 relevance bits of its label words against the call's queries ---------------------------------------
__global__ __launch_bounds__(256) void soft_ap_rel_kernel(const uint32_t* __restrict__ q_lab, const uint32_t* __restrict__ r_lab, int LW,
                                                          int Q, int64_t N, uint64_t* __restrict__ rel) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (j >= N) return;
  uint64_t bits = 0;
  for (int w = 0; w < LW; ++w) {
    const uint32_t mine = r_lab[static_cast<size_t>(j) * LW + w];
    for (int q = 0; q < Q; ++q) bits |= static_cast<uint64_t>((mine & q_lab[q * LW + w]) != 0u) << q;      // (q_lab: wave-uniform)
  }
  rel[j] = bits;
}

// ---- the walk of both passes: SECOND = false the two histograms, true ranks and relranks of the relevant items -----------------------
template <int W, bool SECOND>
__global__ __launch_bounds__(64) void soft_ap_pass_kernel(ApArgs a, const uint32_t* __restrict__ qa, const uint32_t* __restrict__ qb,
                                                          const uint32_t* __restrict__ rs, const uint32_t* __restrict__ rn,
                                                          const uint64_t* __restrict__ rel) {
  using Query = SoftRule::Query<W>;
  extern __shared__ uint32_t col[];      // [nq][2][bins]: counters (histogram) or cursors; SECOND: + double [nq][64], int64 [nq][64]
  const FewArgs& f = a.f;
  const int lane = threadIdx.x, c = blockIdx.x, group = f.group / 2, q0 = blockIdx.y * group, bins = f.bins;
  const int nq = a.Q - q0 < group ? a.Q - q0 : group;
  uint32_t* image = f.img + (static_cast<size_t>(c) * f.Q + 2 * q0) * bins;      // the group's rows of this chunk: 2 nq bins words
  double* dacc = reinterpret_cast<double*>(col + static_cast<size_t>(2) * group * bins);
  long long* racc = reinterpret_cast<long long*>(dacc + group * 64);
  if (SECOND) {
    for (int i = lane; i < 2 * nq * bins; i += 64) col[i] = image[i];
    for (int qi = 0; qi < nq; ++qi) {
      dacc[qi * 64 + lane] = 0.0;
      racc[qi * 64 + lane] = 0;
    }
  } else {
    for (int i = lane; i < 2 * nq * bins; i += 64) col[i] = 0u;
  }
  __syncthreads();
  const int64_t jb = static_cast<int64_t>(c) * f.chunk;
  const int64_t je = jb + f.chunk < f.N ? jb + f.chunk : f.N;
  const uint32_t last = (f.bits & 31) ? (1u << (f.bits & 31)) - 1u : 0xffffffffu;
  const uint64_t below = (uint64_t(1) << lane) - 1u;
  Item<W> cur[kFewSlabs], nxt[kFewSlabs];
  uint64_t curl[kFewSlabs], nxtl[kFewSlabs];
  auto fetch = [&](Item<W>(&it)[kFewSlabs], uint64_t(&lw)[kFewSlabs], int64_t base) {
#pragma unroll
    for (int u = 0; u < kFewSlabs; ++u) {
      const int64_t j = base + u * 64 + lane, at = j < je ? j : je - 1;      // (lanes behind the last item read it once more)
      it[u].load(rs, rn, at);
      lw[u] = rel[at];
    }
  };
  fetch(cur, curl, jb);
  for (int64_t base = jb; base < je; base += 64 * kFewSlabs) {
    fetch(nxt, nxtl, base + 64 * kFewSlabs);
    Query qc, qx;
    qc.load(qa, qb, nullptr, q0, last);
    for (int qi = 0; qi < nq; ++qi) {
      qx.load(qa, qb, nullptr, q0 + (qi + 1 < nq ? qi + 1 : qi), last);
      uint32_t* all = col + static_cast<size_t>(2 * qi) * bins;
      uint32_t* hit = all + bins;
      uint32_t total = 0;
      if (SECOND) {
        const uint32_t R = a.R[q0 + qi], k = static_cast<uint32_t>(a.k);
        total = R < k ? R : k;
      }
#pragma unroll
      for (int u = 0; u < kFewSlabs; ++u) {                                   // in index order: slab u lies before slab u + 1
        const int64_t j = base + u * 64 + lane;
        const bool valid = j < je;
        const bool relevant = valid && ((curl[u] >> (q0 + qi)) & 1u);
        const int h = SoftRule::bin<W>(cur[u], qc, f.bits);
        if (!SECOND) {
          if (valid) atomicAdd(&all[h], 1u);
          if (relevant) atomicAdd(&hit[h], 1u);
        } else {
          // The cursors of the lane's OWN bin as they stood before this slab, then every lane's add, then the first cursor again:
          // it has moved by the valid lanes of this slab in that bin.  A relevant lane ALONE in its bin (nearly all of them, with
          // 30 bits + 1 bins) has its ranks at once; the others take one wave-uniform turn per distinct shared bin, which ballots
          // the valid lanes of that bin for rank and the relevant ones for relrank.  (One wave: its LDS operations run in order.)
          const uint32_t a0 = *reinterpret_cast<volatile uint32_t*>(all + h), r0 = *reinterpret_cast<volatile uint32_t*>(hit + h);
          if (valid) atomicAdd(&all[h], 1u);
          if (relevant) atomicAdd(&hit[h], 1u);
          const uint32_t a1 = *reinterpret_cast<volatile uint32_t*>(all + h);
          uint32_t pi = a0 + 1u, pr = r0 + 1u;
          bool pend = relevant && a1 - a0 > 1u;
          uint64_t mask = __ballot(pend);
          while (mask) {
            const int hsel = __builtin_amdgcn_readlane(h, __ffsll(static_cast<unsigned long long>(mask)) - 1);
            const uint64_t m_all = __ballot(valid && h == hsel);
            const bool mine = pend && h == hsel;
            const uint64_t m_rel = __ballot(mine);                            // (every relevant lane of a shared bin is pending)
            if (mine) {
              pi = a0 + __popcll(m_all & below) + 1u;
              pr = r0 + __popcll(m_rel & below) + 1u;
            }
            pend = pend && !mine;
            mask &= ~m_rel;
          }
          if (relevant) {                                                     // a lane's own slots: its terms meet in index order
            if (pr <= total) dacc[qi * 64 + lane] += static_cast<double>(__fdiv_rn(static_cast<float>(pr), static_cast<float>(pi)));
            racc[qi * 64 + lane] += pi;
          }
        }
      }
      qc = qx;
    }
#pragma unroll
    for (int u = 0; u < kFewSlabs; ++u) {
      cur[u] = nxt[u];
      curl[u] = nxtl[u];
    }
  }
  __syncthreads();
  if (SECOND) {
    for (int qi = 0; qi < nq; ++qi) {
      double s = dacc[qi * 64 + lane];
      long long r = racc[qi * 64 + lane];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {                                      // a fixed tree: the same sum for the same terms
        s += __shfl_xor(s, o, 64);
        r += __shfl_xor(r, o, 64);
      }
      if (lane == 0) {
        a.psum[static_cast<size_t>(c) * a.Q + q0 + qi] = s;
        a.prank[static_cast<size_t>(c) * a.Q + q0 + qi] = r;
      }
    }
  } else {
    for (int i = lane; i < 2 * nq * bins; i += 64) image[i] = col[i];
  }
}

// ---- one wave per row: tot -> the exclusive prefix over the bins (few_radius); every bin gets a base; R from the relevant rows ------
__global__ __launch_bounds__(64) void soft_ap_prefix_kernel(ApArgs a) {
  const int row = blockIdx.x;
  uint32_t total;
  (void)few_radius(a.f, threadIdx.x, row, total);
  if (threadIdx.x == 0) {
    a.f.hstar[row] = a.f.bins - 1;
    if (row & 1) a.R[row >> 1] = total;
  }
}

// ---- one thread per query: the chunks in chunk order ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void soft_ap_finish_kernel(ApArgs a, float* __restrict__ ap, int32_t* __restrict__ relevant,
                                                            long long* __restrict__ rank_sum) {
  const int q = threadIdx.x;
  if (q >= a.Q) return;
  double s = 0.0;
  long long r = 0;
  for (int c = 0; c < a.f.S; ++c) {
    s += a.psum[static_cast<size_t>(c) * a.Q + q];
    r += a.prank[static_cast<size_t>(c) * a.Q + q];
  }
  const uint32_t R = a.R[q], k = static_cast<uint32_t>(a.k), total = R < k ? R : k;
  ap[q] = total ? static_cast<float>(s / static_cast<double>(total)) : 0.f;
  relevant[q] = static_cast<int32_t>(R);
  rank_sum[q] = r;
}

template <int W>
int run_soft_ap_w(const ApArgs& a, const ApPlan& pl, const uint32_t* qs, const uint32_t* qm, const uint32_t* rs, const uint32_t* rn,
                  const uint32_t* q_lab, const uint32_t* r_lab, int LW, float* ap, int32_t* relevant, long long* rank_sum,
                  hipStream_t st) {
  const FewArgs& f = a.f;
  const int nq = a.Q < pl.group ? a.Q : pl.group;
  const size_t rows = static_cast<size_t>(2) * pl.group * f.bins * 4, lds1 = static_cast<size_t>(2) * nq * f.bins * 4,
               lds2 = rows + static_cast<size_t>(pl.group) * 64 * 16;
  const dim3 walk(pl.p.S, pl.p.groups), bins((f.bins + kFewBinTile - 1) / kFewBinTile, f.Q);
  uint64_t* rel = const_cast<uint64_t*>(a.rel);
  hipLaunchKernelGGL(soft_ap_rel_kernel, dim3(static_cast<unsigned>((f.N + 255) / 256)), dim3(256), 0, st, q_lab, r_lab, LW, a.Q, f.N, rel);
  CMH_CHECK_LAUNCH("soft_ap relevance");
  hipLaunchKernelGGL((soft_ap_pass_kernel<W, false>), walk, dim3(64), lds1, st, a, qs, qm, rs, rn, a.rel);
  CMH_CHECK_LAUNCH("soft_ap histogram");
  hipLaunchKernelGGL(few_total_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, f);
  CMH_CHECK_LAUNCH("soft_ap totals");
  hipLaunchKernelGGL(soft_ap_prefix_kernel, dim3(f.Q), dim3(64), 0, st, a);
  CMH_CHECK_LAUNCH("soft_ap prefixes");
  hipLaunchKernelGGL(few_base_kernel, bins, dim3(kFewParts * kFewBinTile), 0, st, f);
  CMH_CHECK_LAUNCH("soft_ap bases");
  hipLaunchKernelGGL((soft_ap_pass_kernel<W, true>), walk, dim3(64), lds2, st, a, qs, qm, rs, rn, a.rel);
  CMH_CHECK_LAUNCH("soft_ap ranks");
  hipLaunchKernelGGL(soft_ap_finish_kernel, dim3(1), dim3(64), 0, st, a, ap, relevant, rank_sum);
  CMH_CHECK_LAUNCH("soft_ap finish");
  return CMH_OK;
}

int check_soft_ap(const char* what, int Q, int64_t N, int bits, int label_words) {
  const int rc = check_few_shape(what, Q, N, bits);
  if (rc != CMH_OK) return rc;
  if (label_words < 1) return what ? fail(CMH_ERR_INVALID, "%s: label_words=%d below 1", what, label_words) : CMH_ERR_INVALID;
  return CMH_OK;
}

}  // namespace
}  // namespace cmh

extern "C" size_t cmh_soft_ap_workspace_bytes(int32_t Q, int64_t N, int32_t bits, int32_t label_words) {
  return check_soft_ap(nullptr, Q, N, bits, label_words) == CMH_OK ? soft_ap_plan(Q, N, bits).bytes(Q, N) : 0;
}

extern "C" int cmh_soft_ap(const uint32_t* q_sign, const uint32_t* q_mag, const uint32_t* r_sign, const uint32_t* r_nz,
                           const uint32_t* q_lab, const uint32_t* r_lab, int32_t label_words, int32_t Q, int64_t N, int32_t bits,
                           int32_t k, float* ap, int32_t* relevant, int64_t* rank_sum, void* workspace, size_t workspace_bytes,
                           void* stream) {
  CMH_CHECK_ARG(q_sign && q_mag && r_sign && r_nz && q_lab && r_lab && ap && relevant && rank_sum, "soft_ap: null pointer");
  const int rc = check_soft_ap("soft_ap", Q, N, bits, label_words);
  if (rc != CMH_OK) return rc;
  CMH_CHECK_ARG(k >= 0 && k <= N, "soft_ap: k=%d outside [1, N=%lld] (0 = N)", k, static_cast<long long>(N));
  const ApPlan pl = soft_ap_plan(Q, N, bits);
  const uintptr_t row = few_row_bytes(pl.p.W);
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(r_sign) % row == 0 && reinterpret_cast<uintptr_t>(r_nz) % row == 0,
                "soft_ap: database planes of %d words per row must be aligned to %d bytes", pl.p.W, static_cast<int>(row));
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(rank_sum) % 8 == 0, "soft_ap: rank_sum holds 64-bit integers: aligned to 8 bytes");
  if (!workspace || workspace_bytes < pl.bytes(Q, N))
    return fail(CMH_ERR_WORKSPACE, "soft_ap: workspace %zu < %zu bytes", workspace_bytes, pl.bytes(Q, N));
  const ApArgs a = soft_ap_args(pl, Q, N, bits, k ? k : static_cast<int>(N), workspace);
  long long* rsum = reinterpret_cast<long long*>(rank_sum);
  const hipStream_t st = as_stream(stream);
  return pl.p.W == 1   ? run_soft_ap_w<1>(a, pl, q_sign, q_mag, r_sign, r_nz, q_lab, r_lab, label_words, ap, relevant, rsum, st)
         : pl.p.W == 2 ? run_soft_ap_w<2>(a, pl, q_sign, q_mag, r_sign, r_nz, q_lab, r_lab, label_words, ap, relevant, rsum, st)
         : pl.p.W == 3 ? run_soft_ap_w<3>(a, pl, q_sign, q_mag, r_sign, r_nz, q_lab, r_lab, label_words, ap, relevant, rsum, st)
                       : run_soft_ap_w<4>(a, pl, q_sign, q_mag, r_sign, r_nz, q_lab, r_lab, label_words, ap, relevant, rsum, st);
}
