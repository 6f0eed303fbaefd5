// conv1 of the image tower as an implicit GEMM: patch_out[B g^2, d] f32 = patches[B g^2, 3p^2] . conv1_w[d, 3p^2]^T with the patch matrix
// never written.  The two-launch stem (norm_embed.hip: patchify_kernel, then launch_gemm) reads the f32 image, writes its bf16
// re-layout and reads that back three times (one per column tile); nothing else in inference reads the patch matrix.  Here the loader
// waves of a loader / consumer kernel (gemm_lc.hip's 12-wave 160-row form: 4 staging + 8 MFMA waves, 160 x 256 tile, three LDS stages
// of 52 KB) build the A tile straight from the image:
//  - W (the conv1 weight [d, 3p^2] bf16) arrives by LDS-DMA exactly as in gemm_lc3_kernel: 8 pieces of 1 KiB per loader wave and
//    stage, XOR swizzle on the source chunk.
//  - A: a K-step of 64 k is, for one channel c, 64 / p consecutive patch rows py - for a tile row (b, gy, gx) that is 64 / p runs of p
//    floats of the image.  A loader lane owns logical chunk ch = lane % 8 (k = 8 ch .. 8 ch + 7 of the K-step: 8 consecutive floats
//    of one run, p % 8 == 0) of tile rows 8 (5 wid + i) + lane / 8, i < 5: ten 16-byte global loads per lane and stage.  It rounds
//    them to f32_to_bf16's bits - patchify_kernel's function, so the operand is the patch matrix's (C1_ROUND below: how) - and writes
//    five packed 16-byte chunks to LDS at physical chunk ch ^ (row & 7): the image the LDS-DMA path leaves and the MFMA side reads.
//  - two register stages (named registers ra* / rb*): while stage n is being rounded, the loads of stage n + 1 are in flight; with
//    the three LDS stages the image loads are issued five K-steps ahead of their MFMAs.
//  - row -> (b, gy, gx) and the row's image pointer (first or second image tensor: the split batch of cmh_clip_encode_pair2) are
//    formed once per tile; inside the K loop one uniform offset (c R^2 + py0 R) moves.
// Barrier protocol per loader iteration s (barrier s stands in front of the MFMA waves' reads of stage s + 1):
//    vmcnt(18): W(s + 1) and the image loads of A(s + 3) have landed (W(s + 2): 8 and A(s + 4): 10 entries may fly)
//    round A(s + 3) into 20 registers; lgkmcnt(0): A(s + 2)'s LDS writes are done; s_barrier
//    behind it nobody reads buffer s % 3: write A(s + 3) there, issue W(s + 3)'s DMA into it, issue A(s + 5)'s image loads.
// MFMA side: gemm_lc3_kernel's K-step without its parked stores and residual fetch - the same v_mfma_f32_16x16x32_bf16, the same
// fragment-to-accumulator assignment (W rows = A operand: a lane owns 4 consecutive n), K-steps in sequence, k = 64 kt + 32 ks + 8 fq + j
// inside: per output element the chain of the wide kernel that runs conv1 in the two-launch stem - the same bits.  The epilogue is
// plain: 20 16-byte f32 stores per lane, rows past M skipped.
// The deal is LcSchedule's (cmh_common.h: deal_share / deal_count): n-fastest tiles, an XCD owns a contiguous eighth, so the column
// tiles of a row tile run at the same time on one XCD and the second and third read of an image row find it in that XCD's L2.
#include <cstdlib>
#include <cstring>

#include "cmh_common.h"

#include <hip/hip_ext.h>

namespace cmh {

typedef __attribute__((ext_vector_type(8))) __bf16 c1_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float c1_f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t c1_u32x4_t;
typedef const __attribute__((address_space(1))) void* c1_gptr_t;
typedef __attribute__((address_space(3))) void* c1_lptr_t;
typedef __attribute__((address_space(3))) c1_u32x4_t* c1_lds_u4p;

constexpr int c1BM = 160, c1BN = 256;
constexpr int c1RowBytes = 128;                      // one K-step of one row: 64 bf16
constexpr int c1WBytes = c1BN * c1RowBytes;          // 32 KB
constexpr int c1STG = c1WBytes + c1BM * c1RowBytes;  // 52 KB per stage, three stages = 156 KB of LDS
constexpr int c1WPieces = 8, c1ALoads = 10;          // a loader wave's vmcnt entries per stage: W DMA pieces, image loads

struct Conv1Args {
  const float* image;      // rows of the first batch_a images
  const float* image_b;    // ... of the rest (== image - batch_a images when the batch is one tensor: the host folds the offset in)
  const char* W;           // [N, K] bf16
  float* out;              // [M, N] f32
  int batch_a, M, N, K;    // M = B g^2, N = d, K = 3 p^2
  int R, p, g;
};

__device__ __forceinline__ int c1_swz(int row, int chunk) { return row * c1RowBytes + ((chunk ^ (row & 7)) << 4); }
__device__ __forceinline__ c1_u32x4_t c1_lds_read(uint32_t addr) {
  return *reinterpret_cast<const __attribute__((address_space(3))) c1_u32x4_t*>(static_cast<size_t>(addr));
}
__device__ __forceinline__ c1_f32x4_t c1_mfma(const c1_u32x4_t& w, const c1_u32x4_t& x, const c1_f32x4_t& cin) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(c1_bf16x8_t, w), __builtin_bit_cast(c1_bf16x8_t, x), cin, 0, 0, 0);
}
__device__ __forceinline__ uint32_t c1_round2(float a, float b) {
  return static_cast<uint32_t>(f32_to_bf16(a)) | (static_cast<uint32_t>(f32_to_bf16(b)) << 16);
}
// 8 consecutive floats -> one 16-byte chunk of the A tile
__device__ __forceinline__ c1_u32x4_t c1_round8(const c1_f32x4_t& lo, const c1_f32x4_t& hi) {
  return c1_u32x4_t{c1_round2(lo[0], lo[1]), c1_round2(lo[2], lo[3]), c1_round2(hi[0], hi[1]), c1_round2(hi[2], hi[3])};
}
// the same for values known not to be NaN: v_cvt_pk_bf16_f32, round-to-nearest-even
__device__ __forceinline__ c1_u32x4_t c1_cvt8(const c1_f32x4_t& lo, const c1_f32x4_t& hi) {
  return c1_u32x4_t{pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3])};
}
#define C1_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define C1_LGKM0() __builtin_amdgcn_s_waitcnt(0xC07F)      // lgkmcnt(0), vmcnt / expcnt untouched

__global__ __launch_bounds__(768) void conv1_stem_kernel(Conv1Args g) {
  __shared__ __attribute__((aligned(1024))) char lds[3 * c1STG];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

  // the deal (LcSchedule's statement for one problem)
  const int M = g.M, N = g.N, K = g.K;
  const int tiles_n = N / c1BN;
  const int total = tiles_n * ((M + c1BM - 1) / c1BM);
  const int slot = blockIdx.x >> 3, per = gridDim.x >> 3;
  const DealShare sh = deal_share(total, blockIdx.x & 7);
  const int my_tiles = deal_count(sh.len, slot, per);
  if (my_tiles == 0) return;
  const int nk = K / 64;
  const int S = my_tiles * nk;      // K-steps of this workgroup = barriers after the prologue's
  auto tile_of = [&](int ti, int& m0, int& n0) {
    const int logical = sh.lo + slot + ti * per;
    const int tm = logical / tiles_n;
    m0 = tm * c1BM;
    n0 = (logical - tm * tiles_n) * c1BN;
  };

  if (wid < 4) {
    // ---- loader waves ----
    const int sub = lane >> 3, ch = lane & 7;
    const int R = g.R, p = g.p, gg = g.g, g2 = gg * gg;
    // W side: lc_loader_wave's
    const uint32_t rs = static_cast<uint32_t>(K) * 2;
    uint32_t offW[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = (wid * 8 + i) * 8 + sub;
      offW[i] = static_cast<uint32_t>(row) * rs + ((ch ^ (row & 7)) << 4);
    }
    const char* Wt = nullptr;
    int w_kt = 0, w_tile = 0, w_buf = 0;
    auto set_w_tile = [&](int ti) {
      int m0, n0;
      tile_of(ti, m0, n0);
      Wt = g.W + static_cast<size_t>(n0) * rs;
    };
    set_w_tile(0);
    auto issue_w = [&]() __attribute__((always_inline)) {
      char* base = lds + w_buf * c1STG;
      const uint32_t koff = static_cast<uint32_t>(w_kt) * c1RowBytes;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        __builtin_amdgcn_global_load_lds((c1_gptr_t)(Wt + koff + offW[i]), (c1_lptr_t)(base + (wid * 8 + i) * 1024), 16, 0, 0);
      w_buf = w_buf == 2 ? 0 : w_buf + 1;
      if (++w_kt == nk) {
        w_kt = 0;
        if (++w_tile < my_tiles) set_w_tile(w_tile);
      }
    };
    // A side.  This lane's 8 floats of a K-step sit (8 ch) / p image rows below the K-step's first and (8 ch) % p floats into the run
    const size_t plane = static_cast<size_t>(R) * R;
    const int lane_off = (ch * 8 / p) * R + (ch * 8) % p;
    const int step_rows = (64 / p) * R;                       // one K-step further inside a channel: 64 / p image rows
    const int chan_steps = p * p / 64;                        // K-steps per channel
    const int chan_skip = static_cast<int>(plane) - p * R;    // ... and from a channel's last K-step to the next channel's first
    const float *ap0 = nullptr, *ap1 = nullptr, *ap2 = nullptr, *ap3 = nullptr, *ap4 = nullptr;      // this lane's five rows of the tile
    int a_j = 0, a_kt = 0, a_tile = 0, a_kb = 0;              // K-step inside the channel / the tile, tile, float offset of the K-step
    auto row_ptr = [&](int m0, int i) __attribute__((always_inline)) {
      int r = m0 + (wid * 5 + i) * 8 + sub;
      r = r < M ? r : M - 1;                                  // rows past M are computed on duplicated data and never stored
      const int b = r / g2, q = r - b * g2, gy = q / gg, gx = q - gy * gg;
      const float* img = b < g.batch_a ? g.image : g.image_b;
      return img + static_cast<size_t>(b) * 3 * plane + static_cast<size_t>(gy * p) * R + gx * p + lane_off;
    };
    auto set_a_tile = [&](int ti) __attribute__((always_inline)) {
      int m0, n0;
      tile_of(ti, m0, n0);
      ap0 = row_ptr(m0, 0); ap1 = row_ptr(m0, 1); ap2 = row_ptr(m0, 2); ap3 = row_ptr(m0, 3); ap4 = row_ptr(m0, 4);
    };
    set_a_tile(0);
    auto next_a = [&]() __attribute__((always_inline)) {
      a_kb += step_rows;
      if (++a_j == chan_steps) { a_j = 0; a_kb += chan_skip; }
      if (++a_kt == nk) {
        a_kt = 0; a_j = 0; a_kb = 0;
        if (++a_tile < my_tiles) set_a_tile(a_tile);
      }
    };
    c1_f32x4_t ra0, ra1, ra2, ra3, ra4, ra5, ra6, ra7, ra8, ra9;      // the two register stages of image loads
    c1_f32x4_t rb0, rb1, rb2, rb3, rb4, rb5, rb6, rb7, rb8, rb9;
    c1_u32x4_t q0, q1, q2, q3, q4;                                    // a rounded stage on its way to LDS
    char* const a_dst = lds + c1WBytes + wid * 5 * 1024 + sub * c1RowBytes + ((ch ^ sub) << 4);      // (row & 7 == sub)
// The image loads are written out and hand-counted: a wave with LDS-DMA in flight makes hipcc place `s_waitcnt vmcnt(0)` in front of
// every use of a loaded register (a pending FLAT-encoded LDS access: the conservative rule), which would drain both stages in flight
// at every K-step.  Nothing but C1_WAIT may touch a stage's registers between its C1_LOAD and that wait.
#define C1_LD2(lo, hi, ptr)                                                                                    \
  do {                                                                                                         \
    const float* p_ = (ptr) + a_kb;                                                                            \
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(lo) : "v"(p_) : "memory");                           \
    asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(hi) : "v"(p_) : "memory");                 \
  } while (0)
#define C1_LOAD(r)                                                                                             \
  do {                                                                                                         \
    C1_LD2(r##0, r##1, ap0); C1_LD2(r##2, r##3, ap1); C1_LD2(r##4, r##5, ap2); C1_LD2(r##6, r##7, ap3);        \
    C1_LD2(r##8, r##9, ap4);                                                                                   \
    next_a();                                                                                                  \
  } while (0)
// stage r has landed; n younger entries of this wave's vmcnt queue may fly
#define C1_WAIT(n, r)                                                                                          \
  asm volatile("s_waitcnt vmcnt(%10)"                                                                          \
               : "+v"(r##0), "+v"(r##1), "+v"(r##2), "+v"(r##3), "+v"(r##4), "+v"(r##5), "+v"(r##6), "+v"(r##7), "+v"(r##8), "+v"(r##9) \
               : "n"(n)                                                                                        \
               : "memory")
// Rounding a stage.  f32_to_bf16 inlines to a masked two-way path per value (13 instructions: 520 per stage, about a K-step's whole
// MFMA time on the same SIMD); v_cvt_pk_bf16_f32 (pack_bf16x2) rounds two values in one.  Both are round-to-nearest-even, so for every
// value that is not a NaN they give the same bits by definition (denormals are kept: the kernel runs with f32 / 16-bit denormals on);
// only a NaN's payload is each one's own choice.  So: the sum of the stage's 40 values is a NaN iff one of them is (or an inf - inf
// false alarm); a wave without one takes the one-instruction conversion, any other rounds the stage with f32_to_bf16 itself.
#define C1_ROUND(r)                                                                                            \
  do {                                                                                                         \
    const c1_f32x4_t t_ = (((r##0 + r##1) + (r##2 + r##3)) + ((r##4 + r##5) + (r##6 + r##7))) + (r##8 + r##9); \
    const float u_ = (t_[0] + t_[1]) + (t_[2] + t_[3]);                                                        \
    if (__builtin_amdgcn_ballot_w64(u_ != u_) == 0) {                                                          \
      q0 = c1_cvt8(r##0, r##1); q1 = c1_cvt8(r##2, r##3); q2 = c1_cvt8(r##4, r##5);                            \
      q3 = c1_cvt8(r##6, r##7); q4 = c1_cvt8(r##8, r##9);                                                      \
    } else {                                                                                                   \
      q0 = c1_round8(r##0, r##1); q1 = c1_round8(r##2, r##3); q2 = c1_round8(r##4, r##5);                      \
      q3 = c1_round8(r##6, r##7); q4 = c1_round8(r##8, r##9);                                                  \
    }                                                                                                          \
  } while (0)
#define C1_WRITE(buf)                                                                                          \
  do {                                                                                                         \
    char* d_ = a_dst + (buf) * c1STG;                                                                          \
    *(c1_lds_u4p)(d_) = q0; *(c1_lds_u4p)(d_ + 1024) = q1; *(c1_lds_u4p)(d_ + 2048) = q2;                      \
    *(c1_lds_u4p)(d_ + 3072) = q3; *(c1_lds_u4p)(d_ + 4096) = q4;                                              \
  } while (0)
    // prologue (S >= 6, even: the host's rule): stages 0..2 into the ring, the image loads of stages 3 and 4 into the two register
    // stages.  W(2) is issued between A(3) and A(4), so that the queue ends as every loop iteration's does: A(s + 3), W, A(s + 4)
    issue_w();
    issue_w();
    C1_LOAD(ra);
    C1_LOAD(rb);
    C1_WAIT(c1ALoads, ra); C1_ROUND(ra); C1_WRITE(0);      // (W(0) and W(1) are older: landed with it)
    C1_LOAD(ra);
    C1_WAIT(c1ALoads, rb); C1_ROUND(rb); C1_WRITE(1);
    C1_LOAD(rb);
    C1_WAIT(c1ALoads, ra); C1_ROUND(ra); C1_WRITE(2);
    issue_w();
    C1_LOAD(ra);
    C1_LGKM0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int a_buf = 0;                                  // s % 3
    // iteration s; r: the register stage that holds A(s + 3) (stage n lives in ra for even n).  FULL: A(s + 5) exists and takes r
    // over.  In front of barrier s W(s + 1) and A(s + 3) have landed - W(s + 2) and A(s + 4), 18 entries, may fly.  The last six
    // iterations drain: whatever is left has landed, what does not exist is not issued
#define C1_BARRIER()                                                                                           \
  do {                                                                                                         \
    C1_LGKM0();                                                                                                \
    __builtin_amdgcn_s_barrier();                                                                              \
    asm volatile("" ::: "memory");                                                                             \
  } while (0)
#define C1_FULL(r)                                                                                             \
  do {                                                                                                         \
    C1_WAIT(c1WPieces + c1ALoads, r);                                                                          \
    C1_ROUND(r);                                                                                               \
    C1_BARRIER();                                                                                              \
    C1_WRITE(a_buf);                                                                                           \
    issue_w();                                                                                                 \
    C1_LOAD(r);                                                                                                \
    a_buf = a_buf == 2 ? 0 : a_buf + 1;                                                                        \
  } while (0)
#define C1_TAIL(r)                                                                                             \
  do {                                                                                                         \
    C1_WAIT(0, r);                                                                                             \
    C1_ROUND(r);                                                                                               \
    C1_BARRIER();                                                                                              \
    C1_WRITE(a_buf);                                                                                           \
    issue_w();                                                                                                 \
    a_buf = a_buf == 2 ? 0 : a_buf + 1;                                                                        \
  } while (0)
    for (int s = 0; s + 6 < S; s += 2) {
      C1_FULL(rb);
      C1_FULL(ra);
    }
    C1_FULL(rb);                                    // s = S - 6: A(S - 1) is the last stage there is
    C1_TAIL(ra);                                    // s = S - 5
    C1_TAIL(rb);                                    // s = S - 4
    C1_VMCNT(0);                                    // W(S - 1)
    C1_BARRIER();                                   // s = S - 3 .. S - 1: nothing left to stage
    C1_BARRIER();
    C1_BARRIER();
#undef C1_WAIT
#undef C1_LD2
#undef C1_TAIL
#undef C1_FULL
#undef C1_BARRIER
#undef C1_WRITE
#undef C1_ROUND
#undef C1_LOAD
    return;
  }

  // ---- MFMA waves: 2 (m) x 4 (n) waves of 80 x 64, gemm_lc3_kernel's K-step ----
  const int c = wid - 4;
  const int wm = c >> 2, wn = c & 3;
  const int frow = lane & 15, fq = lane >> 4;
  const uint32_t lds_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((c1_lptr_t)lds));
  const uint32_t aW = lds_base + c1_swz(wn * 64 + frow, fq);
  const uint32_t aX = lds_base + c1WBytes + c1_swz(wm * 80 + frow, fq);      // (80 rows = 10 x 8: the swizzle's row & 7 is frow & 7)

  c1_f32x4_t acc[4][5];                            // [n-fragment][m-fragment]
  c1_u32x4_t fw[4], fx[5];

  __builtin_amdgcn_s_barrier();                    // stage 0 has landed
  asm volatile("" ::: "memory");
#pragma unroll
  for (int b = 0; b < 5; ++b) fx[b] = c1_lds_read(aX + b * 2048);
#pragma unroll
  for (int a = 0; a < 4; ++a) fw[a] = c1_lds_read(aW + a * 2048);

  // One half-step: group a = fw[a] x fx[0..4], W-outer; fw[a] refilled from (wsrc) after its group, fx[b] from (xsrc) after MFMA (3, b)
  // and fw[3] last
#define C1_GROUP(a)                                                                                    \
  do {                                                                                                 \
    acc[a][0] = c1_mfma(fw[a], fx[0], acc[a][0]);                                                      \
    acc[a][1] = c1_mfma(fw[a], fx[1], acc[a][1]);                                                      \
    acc[a][2] = c1_mfma(fw[a], fx[2], acc[a][2]);                                                      \
    acc[a][3] = c1_mfma(fw[a], fx[3], acc[a][3]);                                                      \
    acc[a][4] = c1_mfma(fw[a], fx[4], acc[a][4]);                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)
#define C1_LAST_ONE(b, xsrc)                                                                           \
  do {                                                                                                 \
    acc[3][b] = c1_mfma(fw[3], fx[b], acc[3][b]);                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    fx[b] = c1_lds_read((xsrc) + (b) * 2048);                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)
#define C1_LAST(wsrc, xsrc)                                                                            \
  do {                                                                                                 \
    C1_LAST_ONE(0, xsrc); C1_LAST_ONE(1, xsrc); C1_LAST_ONE(2, xsrc); C1_LAST_ONE(3, xsrc);            \
    acc[3][4] = c1_mfma(fw[3], fx[4], acc[3][4]);                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    fx[4] = c1_lds_read((xsrc) + 8192);                                                                \
    fw[3] = c1_lds_read((wsrc) + 6144);                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)
#define C1_REFILL_W(a, wsrc)                                                                           \
  do {                                                                                                 \
    fw[a] = c1_lds_read((wsrc) + (a) * 2048);                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)

  int cur = 0;
  for (int ti = 0; ti < my_tiles; ++ti) {
    int m0, n0;
    tile_of(ti, m0, n0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 5; ++b) acc[a][b] = c1_f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("" : "+s"(kt));
      const uint32_t bo = static_cast<uint32_t>(cur) * c1STG;
      const uint32_t w1 = (aW + bo) ^ 64u, x1 = (aX + bo) ^ 64u;      // k 32..63 of this stage
      // ---------------- half 0 ----------------
      C1_GROUP(0); C1_REFILL_W(0, w1);
      C1_GROUP(1); C1_REFILL_W(1, w1);
      C1_GROUP(2); C1_REFILL_W(2, w1);
      C1_LAST(w1, x1);
      // ---------------- half 1 ----------------
      const int nxt = cur == 2 ? 0 : cur + 1;
      const uint32_t bn = static_cast<uint32_t>(nxt) * c1STG;
      const uint32_t w0 = aW + bn, x0 = aX + bn;      // k 0..31 of the next stage
      C1_GROUP(0);
      C1_GROUP(1);
      C1_LGKM0();                                    // every fragment of this stage is in registers ...
      __builtin_amdgcn_s_barrier();                  // ... in every MFMA wave; the next stage has landed
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      C1_REFILL_W(0, w0); C1_REFILL_W(1, w0);
      C1_GROUP(2); C1_REFILL_W(2, w0);
      C1_LAST(w0, x0);
      cur = nxt;
    }
    // epilogue: lane (frow, fq) holds rows wm 80 + 16 b + frow, columns wn 64 + 16 a + 4 fq .. + 3 of the tile
    float* const orow = g.out + static_cast<size_t>(m0 + wm * 80 + frow) * N + n0 + wn * 64 + fq * 4;
    const int rows_left = M - (m0 + wm * 80 + frow);
#pragma unroll
    for (int b = 0; b < 5; ++b)
      if (b * 16 < rows_left) {
#pragma unroll
        for (int a = 0; a < 4; ++a) *reinterpret_cast<c1_f32x4_t*>(orow + static_cast<size_t>(b) * 16 * N + a * 16) = acc[a][b];
      }
  }
#undef C1_GROUP
#undef C1_LAST_ONE
#undef C1_LAST
#undef C1_REFILL_W
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int g_conv1_fused = -1;      // cmh_set_conv1_fused: -1 = environment (CMH_CONV1_FUSED=0 switches the fused stem off)
bool conv1_fused_enabled() {
  static const bool env_on = []() { const char* e = getenv("CMH_CONV1_FUSED"); return !(e && !strcmp(e, "0")); }();
  return g_conv1_fused < 0 ? env_on : g_conv1_fused != 0;
}

// the shapes conv1_stem_kernel is built for: bf16 operands, a K-step of whole image runs (64 % p == 0, p % 4 == 0) without K padding,
// an even number >= 6 of K-steps (the loader's prologue and its two register stages) - together p = 16, 32, 64 - 16-byte aligned
// runs, whole column tiles
bool conv1_fused_takes(int dt, int p, int R, int d) {
  if (!(dt == CMH_BF16 && p > 0 && 64 % p == 0 && p % 4 == 0 && R % 4 == 0 && R % p == 0 && d % c1BN == 0 && conv1_k(p, dt) == 3 * p * p))
    return false;
  const int nk = 3 * p * p / 64;
  return nk >= 6 && nk % 2 == 0;
}

int launch_conv1_fused(const float* image, const float* image_b, int batch_a, int B, int R, int p, const void* W, float* out, int d,
                       hipStream_t st) {
  CMH_CHECK_ARG(image && W && out && B > 0, "conv1 (fused): null pointer or empty batch");
  CMH_CHECK_ARG(conv1_fused_takes(CMH_BF16, p, R, d), "conv1 (fused): resolution %d / patch %d / width %d unsupported", R, p, d);
  CMH_CHECK_ARG(!image_b || (batch_a > 0 && batch_a < B), "conv1 (fused): split batch %d of %d", batch_a, B);
  CMH_CHECK_ARG(((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(image_b) | reinterpret_cast<uintptr_t>(W) |
                  reinterpret_cast<uintptr_t>(out)) & 15) == 0, "conv1 (fused): operands must be 16-byte aligned");
  const int g = R / p, K = 3 * p * p;
  const long long rows = static_cast<long long>(B) * g * g;
  CMH_CHECK_ARG(rows < (1ll << 31) - c1BM && static_cast<size_t>(d) * K * 2 < (1ull << 32), "conv1 (fused): %lld rows / weight of %d x %d exceed the index range", rows, d, K);
  Conv1Args a;
  a.image = image;
  // one tensor: every image b takes the first base; two: image b >= batch_a is image b - batch_a of the second
  a.batch_a = image_b ? batch_a : B;
  a.image_b = image_b ? image_b - static_cast<size_t>(batch_a) * 3 * R * R : image;
  a.W = static_cast<const char*>(W);
  a.out = out;
  a.M = static_cast<int>(rows); a.N = d; a.K = K; a.R = R; a.p = p; a.g = g;
  const int total = (d / c1BN) * ((a.M + c1BM - 1) / c1BM), cus = gemm_cus();
  const int grid = total < cus ? ((total + 7) & ~7) : cus;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const bool timed = gemm_prof_open_conv1(&ev0, &ev1);
  if (timed) hipExtLaunchKernelGGL(conv1_stem_kernel, dim3(grid), dim3(768), 0, st, ev0, ev1, 0, a);
  else hipLaunchKernelGGL(conv1_stem_kernel, dim3(grid), dim3(768), 0, st, a);
  CMH_CHECK_LAUNCH("conv1 (fused)");
  if (timed) gemm_prof_close_conv1(a.M, d, K);
  return CMH_OK;
}

}  // namespace cmh

extern "C" int cmh_set_conv1_fused(int32_t on) {
  CMH_CHECK_ARG(on >= -1 && on <= 1, "set_conv1_fused: %d (-1 environment, 0 off, 1 on)", on);
  cmh::g_conv1_fused = on;
  return CMH_OK;
}
