// Allow-masks of the filtered search (cmh_hamming_topk_few_masked, cmh_soft_topk_masked): u64 [ceil(N / 64)], bit j % 64 of word
// j / 64 set = database item j is admitted.  Two ways to make one on the GPU, without a trip through the host:
//   cmh_mask_from_labels  a condition on the packed label words of every item.  One lane per item; the ballot of a wave IS the
//                         64-bit word of its 64 items, so every word is written once, by one lane, with the bits at and behind
//                         N zero.  No atomics.
//   cmh_mask_from_ids     an allow list (value 1) or a deny list (value 0) applied to an existing mask.  One thread per id; ids
//                         may repeat and several may fall into one word, so the bits go in by atomicOr / atomicAnd on the word: the
//                         result does not depend on the order.  An id outside [0, N) changes nothing and sets *bad.
#include "cmh_common.h"

namespace cmh {
namespace {

constexpr int kMaskBlock = 256;      // four waves, four words

__global__ __launch_bounds__(kMaskBlock) void mask_from_labels_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ need,
                                                                      int mode, int64_t N, int LW, uint64_t* __restrict__ allow) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kMaskBlock + threadIdx.x;
  bool any = false, all = true;
  if (j < N) {
    const uint32_t* row = lab + static_cast<size_t>(j) * LW;
    for (int w = 0; w < LW; ++w) {
      const uint32_t nd = need[w], both = row[w] & nd;
      any = any || both != 0u;
      all = all && both == nd;
    }
  }
  const bool ok = j < N && (mode == CMH_MASK_ANY ? any : mode == CMH_MASK_ALL ? all : !any);
  const uint64_t word = __ballot(ok);
  const int64_t first = j - (threadIdx.x & 63);      // the wave's first item: a multiple of 64
  if ((threadIdx.x & 63) == 0 && first < N) allow[first >> 6] = word;
}

__global__ __launch_bounds__(kMaskBlock) void mask_from_ids_kernel(const int32_t* __restrict__ ids, int64_t M, int64_t N, int value,
                                                                   unsigned long long* __restrict__ allow, int32_t* __restrict__ bad) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMaskBlock + threadIdx.x;
  if (i >= M) return;
  const int64_t id = ids[i];
  if (id < 0 || id >= N) {
    *bad = 1;
    return;
  }
  const unsigned long long bit = 1ull << (id & 63);
  if (value) atomicOr(&allow[id >> 6], bit);
  else atomicAnd(&allow[id >> 6], ~bit);
}

}  // namespace
}  // namespace cmh

using namespace cmh;

extern "C" int cmh_mask_from_labels(const uint32_t* r_label, const uint32_t* need, int32_t mode, int64_t N, int32_t classes,
                                    uint64_t* allow, void* stream) {
  CMH_CHECK_ARG(r_label && need && allow, "mask_from_labels: null pointer");
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(allow) % 8 == 0, "mask_from_labels: the allow-mask holds 64-bit words: aligned to 8 bytes");
  CMH_CHECK_ARG(mode == CMH_MASK_ANY || mode == CMH_MASK_ALL || mode == CMH_MASK_NONE, "mask_from_labels: mode=%d is none of any, all, none", mode);
  CMH_CHECK_ARG(N >= 1 && N <= INT32_MAX, "mask_from_labels: N=%lld outside [1, 2^31 - 1]", static_cast<long long>(N));
  CMH_CHECK_ARG(classes >= 1, "mask_from_labels: classes=%d below 1", classes);
  const int64_t blocks = (N + kMaskBlock - 1) / kMaskBlock;
  hipLaunchKernelGGL(mask_from_labels_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kMaskBlock), 0, as_stream(stream), r_label, need,
                     mode, N, (classes + 31) / 32, allow);
  CMH_CHECK_LAUNCH("mask_from_labels");
  return CMH_OK;
}

extern "C" int cmh_mask_from_ids(const int32_t* ids, int64_t M, int64_t N, int32_t value, uint64_t* allow, int32_t* bad, void* stream) {
  CMH_CHECK_ARG(allow && bad && (ids || M == 0), "mask_from_ids: null pointer");
  CMH_CHECK_ARG(reinterpret_cast<uintptr_t>(allow) % 8 == 0, "mask_from_ids: the allow-mask holds 64-bit words: aligned to 8 bytes");
  CMH_CHECK_ARG(value == 0 || value == 1, "mask_from_ids: value=%d is neither 0 (clear) nor 1 (set)", value);
  CMH_CHECK_ARG(N >= 1 && N <= INT32_MAX, "mask_from_ids: N=%lld outside [1, 2^31 - 1]", static_cast<long long>(N));
  CMH_CHECK_ARG(M >= 0 && M <= INT32_MAX, "mask_from_ids: M=%lld outside [0, 2^31 - 1]", static_cast<long long>(M));
  if (M == 0) return CMH_OK;
  const int64_t blocks = (M + kMaskBlock - 1) / kMaskBlock;
  hipLaunchKernelGGL(mask_from_ids_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kMaskBlock), 0, as_stream(stream), ids, M, N, value,
                     reinterpret_cast<unsigned long long*>(allow), bad);
  CMH_CHECK_LAUNCH("mask_from_ids");
  return CMH_OK;
}
