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
