// DScPH proxy-fusion (CPF) loss and the step's quantisation term: reference train/DScPH/CPF_loss.py:24-54 `CPF.forward(image, text, labels)`
// and train/DScPH/hash_train.py:64-70 (bit_var_loss of the rotated, normalised head outputs), forward and backward, both modalities in
// one call.
//
//   n(x) = x / max(|x|, 1e-12) per row (F.normalize);  c = n(h) n(W)^T  [B, C], per modality                                  (:27-28)
//   tp = 2 sum max(c, 0) Y + b                                                                                                (:30-31)
//   lp = sum (1 - c) exp((1 - c) sp) Y,   ln = sum_{c > tau} (c - psi) exp((c - mu) sn) (1 - Y)     (the exponentials detached, :36-49)
//   L  = 1 - tp / (tp + lp + ln);   CPF = L(image) + L(text)                                                                  (:51-54)
//   q  = mean(sigma(z) (1 - sigma(z))) over the B K elements of z = n(h).  The reference takes z = n(rot(h^T)^T) with a HouseHolder
//        whose weights are the identity and are in no optimiser group (hash_train.py:35-45): rot(X) = -X exactly, and the summand is
//        even in z, so the rotation is not built
//   loss = L_img + L_txt + quant_weight (q_img + q_txt)
//   d L / d c = -(lp + ln) / D^2 2 Y [c >= 0] + tp / D^2 (-exp((1 - c) sp) Y + [c > tau] exp((c - mu) sn) (1 - Y)),  D = tp + lp + ln >= b
//   d n(h) = G n(W),  d n(W) = G_img^T n(h_img) + G_txt^T n(h_txt),  dx = (g - n (n . g)) / max(|x|, 1e-12) for rows of h and of W
//
// Forward: normalize_rows for hi, ht and W (the unit rows and divisors stay on the tape), then workgroup (row block, modality) keeps its
// kCpfRows unit rows in LDS and walks the unit proxies through LDS kCpfChunk classes at a time, k-major with a pad column (staging store
// and reads meet every bank once per 32 lanes); thread (ry, cx) owns class cx of the chunk for rows ry, ry + 4, ry + 8, ry + 12, each
// cosine one k-ascending fmaf chain.  The cosines go to `cos`; the element terms are f32 as the reference's are and are added in f64:
// per thread in walk order, per workgroup left to right, and one workgroup then adds the row blocks in ascending order and leaves the
// four terms, the loss and the six sums (tp, lp, ln per modality) on the tape.  Backward, ONE launch: workgroup (block, side) owns 16
// rows of d_hi (side 0), d_ht (1) or d_proxies (2).  It reads the decisions' cosines back from `cos` (the very values the forward
// compared), builds its 16 coefficient rows a slice of kCpfSlice partners at a time in LDS and adds the partners' unit rows in ascending
// order, one fmaf chain per output element - for the proxies the image rows first, then the text rows; the q term's gradient and the
// normaliser's backward finish the rows in the same launch.  No atomics, no workgroup waits on another, nothing is read back: two calls
// give the same bits.  Launches: forward 5 (three normalisers, row blocks, fold), backward 1.
#include "head_common.h"

namespace cmh {

constexpr int kCpfMaxB = 1024, kCpfMaxK = 128, kCpfMaxC = 1024;
constexpr int kCpfRows = 16;                                 // rows per workgroup, forward and backward
constexpr int kCpfChunk = 64;                                // classes per staged proxy tile (forward)
constexpr int kCpfSlice = 256;                               // partners per coefficient slice (backward)
constexpr int kCpfHead = 16;                                 // floats at the head of the tape: the six f64 sums, padded to 64 bytes

struct CpfScalars { float tau, psi, sp, sn, mu, b; };

// sigma(z) (1 - sigma(z)) with the reference's sigma (FAST_HPP.py:7-10)
__device__ __forceinline__ float cpf_bit_var(float z, float* sig) {
  const float s = 1.f / (1.f + expf(-z));
  *sig = s;
  return s * (1.f - s);
}

// grid (row blocks, 2).  unit [2, B, K]; uw [C, K]; cos [2, B, C]; part [2, row blocks, 4]: sum max(c, 0) Y, lp, ln, sum of the q summand
__global__ __launch_bounds__(256) void cpf_rows_kernel(const float* __restrict__ unit, const float* __restrict__ uw, const float* __restrict__ y,
                                                       int B, int K, int C, CpfScalars s, float* __restrict__ cos, double* __restrict__ part) {
  __shared__ float sh[kCpfRows][kCpfMaxK];
  __shared__ float sw[kCpfMaxK][kCpfChunk + 1];
  __shared__ double red[4];
  const int m = blockIdx.y, r0 = blockIdx.x * kCpfRows, tid = threadIdx.x, cx = tid & 63, ry = tid >> 6;
  const float* u = unit + static_cast<size_t>(m) * B * K;
  float* cm = cos + static_cast<size_t>(m) * B * C;
  for (int e = tid; e < kCpfRows * K; e += 256) {
    const int r = e / K, k = e - r * K;
    sh[r][k] = r0 + r < B ? u[static_cast<size_t>(r0 + r) * K + k] : 0.f;
  }
  __syncthreads();
  double q = 0.0, tp = 0.0, lp = 0.0, ln = 0.0;
  for (int e = tid; e < kCpfRows * K; e += 256) {
    const int r = e / K, k = e - r * K;
    float sig;
    if (r0 + r < B) q += static_cast<double>(cpf_bit_var(sh[r][k], &sig));
  }
  const int sk = tid & 31, sc = tid >> 5;                    // staging: 32 consecutive k of class sc, sc + 8, ...
  for (int c0 = 0; c0 < C; c0 += kCpfChunk) {
    __syncthreads();                                         // the previous chunk has been read
    for (int k0 = 0; k0 < K; k0 += 32) {
      const int k = k0 + sk;
      if (k >= K) continue;
#pragma unroll
      for (int j = 0; j < kCpfChunk / 8; ++j) {
        const int c = sc + 8 * j;
        sw[k][c] = c0 + c < C ? uw[static_cast<size_t>(c0 + c) * K + k] : 0.f;
      }
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
      const float w = sw[k][cx];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(sh[ry + 4 * j][k], w, acc[j]);
    }
    const int cl = c0 + cx;
    if (cl >= C) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = r0 + ry + 4 * j;
      if (row >= B) continue;
      const size_t e = static_cast<size_t>(row) * C + cl;
      const float c = acc[j], yv = y[e], omc = 1.f - c;
      cm[e] = c;
      tp += static_cast<double>(fmaxf(c, 0.f) * yv);
      lp += static_cast<double>(omc * expf(omc * s.sp) * yv);
      if (c > s.tau) ln += static_cast<double>((c - s.psi) * expf((c - s.mu) * s.sn) * (1.f - yv));
    }
  }
  tp = block_sum_ltr(tp, red);
  lp = block_sum_ltr(lp, red);
  ln = block_sum_ltr(ln, red);
  q = block_sum_ltr(q, red);
  if (tid == 0) {
    double* out = part + (static_cast<size_t>(m) * gridDim.x + blockIdx.x) * 4;
    out[0] = tp; out[1] = lp; out[2] = ln; out[3] = q;
  }
}

// one workgroup: thread t < 8 adds quantity t & 3 of modality t >> 2 over the row blocks in ascending order; thread 0 makes the terms.
// sums [6] (the tape): tp (with 2 x and + b), lp, ln of the image side, then of the text side
__global__ __launch_bounds__(64) void cpf_fold_kernel(const double* __restrict__ part, int blocks, int B, int K, CpfScalars s, float qw,
                                                      float* __restrict__ terms, float* __restrict__ loss, double* __restrict__ sums) {
  __shared__ double tot[8];
  const int t = threadIdx.x;
  if (t < 8) {
    double a = 0.0;
    for (int i = 0; i < blocks; ++i) a += part[(static_cast<size_t>(t >> 2) * blocks + i) * 4 + (t & 3)];
    tot[t] = a;
  }
  __syncthreads();
  if (t != 0) return;
  float out[4];
  for (int m = 0; m < 2; ++m) {
    const double tp = 2.0 * tot[4 * m] + static_cast<double>(s.b), lp = tot[4 * m + 1], ln = tot[4 * m + 2];
    sums[3 * m] = tp; sums[3 * m + 1] = lp; sums[3 * m + 2] = ln;
    out[m] = static_cast<float>(1.0 - tp / (tp + lp + ln));
    out[2 + m] = static_cast<float>(tot[4 * m + 3] / (static_cast<double>(B) * static_cast<double>(K)));
  }
  for (int j = 0; j < 4; ++j) terms[j] = out[j];
  loss[0] = (out[0] + out[1]) + qw * (out[2] + out[3]);
}

// d L / d c of one element; a = -2 (lp + ln) / D^2 dloss, t = tp / D^2 dloss
__device__ __forceinline__ float cpf_coef(float c, float yv, float a, float t, const CpfScalars& s) {
  float e = -expf((1.f - c) * s.sp) * yv;
  if (c > s.tau) e = fmaf(expf((c - s.mu) * s.sn), 1.f - yv, e);
  return fmaf(t, e, c >= 0.f ? a * yv : 0.f);
}

// grid (max(row blocks of B, row blocks of C), 3).  side 0 / 1: rows of d_hi / d_ht, partners the C unit proxies; side 2: rows of
// d_proxies, partners the B unit image rows, then the B unit text rows.  div [2B + C]: the divisors of hi, ht and the proxies
__global__ __launch_bounds__(256) void cpf_backward_kernel(const float* __restrict__ unit, const float* __restrict__ uw,
                                                           const float* __restrict__ div, const float* __restrict__ y,
                                                           const float* __restrict__ cos, const double* __restrict__ sums,
                                                           const float* __restrict__ dloss, int B, int K, int C, CpfScalars s, float qw,
                                                           float* __restrict__ d_hi, float* __restrict__ d_ht, float* __restrict__ d_w) {
  __shared__ float sg[kCpfRows][kCpfSlice + 1];              // the pad column: side 2 stores 16 rows of one partner at a time
  __shared__ float gs[kCpfRows][kCpfMaxK];
  const int side = blockIdx.y, r0 = blockIdx.x * kCpfRows, tid = threadIdx.x, k = tid & 127, half = tid >> 7;
  const int R = side < 2 ? B : C, J = side < 2 ? C : B;
  if (r0 >= R) return;                                       // uniform over the workgroup
  const float dl = dloss[0];
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < (side < 2 ? 1 : 2); ++pass) {
    const int m = side < 2 ? side : pass;
    const float* other = side < 2 ? uw : unit + static_cast<size_t>(m) * B * K;
    const float* cm = cos + static_cast<size_t>(m) * B * C;
    const double tp = sums[3 * m], rest = sums[3 * m + 1] + sums[3 * m + 2], D = tp + rest;
    const float a = static_cast<float>(-2.0 * rest / (D * D) * static_cast<double>(dl));
    const float t = static_cast<float>(tp / (D * D) * static_cast<double>(dl));
    for (int j0 = 0; j0 < J; j0 += kCpfSlice) {
      __syncthreads();                                       // the previous slice has been read
      for (int e = tid; e < kCpfRows * kCpfSlice; e += 256) {
        // side 0 / 1: a row's classes are contiguous; side 2: the 16 classes of one batch row are
        const int r = side < 2 ? e / kCpfSlice : e % kCpfRows, j = side < 2 ? e % kCpfSlice : e / kCpfRows;
        float g = 0.f;
        if (r0 + r < R && j0 + j < J) {
          const size_t idx = side < 2 ? static_cast<size_t>(r0 + r) * C + j0 + j : static_cast<size_t>(j0 + j) * C + r0 + r;
          g = cpf_coef(cm[idx], y[idx], a, t, s);
        }
        sg[r][j] = g;
      }
      __syncthreads();
      const int jn = min(kCpfSlice, J - j0);
      if (k < K)
        for (int j = 0; j < jn; ++j) {
          const float o = other[static_cast<size_t>(j0 + j) * K + k];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = fmaf(sg[half * 8 + i][j], o, acc[i]);
        }
    }
  }
  const float* own = side < 2 ? unit + static_cast<size_t>(side) * B * K : uw;
  const float* n_own = div + (side < 2 ? side * B : 2 * B);
  float* out = side == 0 ? d_hi : side == 1 ? d_ht : d_w;
  const float qc = qw * dl / (static_cast<float>(B) * static_cast<float>(K));
  if (k < K) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = half * 8 + i;
      float g = acc[i];
      if (side < 2 && r0 + r < R) {
        // d / dz of sigma (1 - sigma) = sigma (1 - sigma) (1 - 2 sigma) = -t (1 - t^2) / 4 with t = tanh(z / 2): 1 - 2 sigma formed from
        // sigma near 1 / 2 would lose |z| / 2^-23 of its digits, and the normaliser's projection below removes most of what is left
        const float t = tanhf(0.5f * own[static_cast<size_t>(r0 + r) * K + k]);
        g = fmaf(qc, -0.25f * t * fmaf(-t, t, 1.f), g);
      }
      gs[r][k] = g;
    }
  }
  __syncthreads();
  // the normaliser's backward (l2norm_bwd_kernel's arithmetic): wave w finishes rows w, w + 4, ...; below the eps clamp u = x / eps is linear
  const int lane = tid & 63, w = tid >> 6, k_lo = lane, k_hi = lane + 64;
  for (int r = w; r < kCpfRows; r += 4) {
    const int row = r0 + r;                                  // uniform over the wave
    if (row >= R) break;
    const float g0 = k_lo < K ? gs[r][k_lo] : 0.f, g1 = k_hi < K ? gs[r][k_hi] : 0.f;
    const float u0 = k_lo < K ? own[static_cast<size_t>(row) * K + k_lo] : 0.f, u1 = k_hi < K ? own[static_cast<size_t>(row) * K + k_hi] : 0.f;
    const float dot = wave_sum(fmaf(u1, g1, u0 * g0)), nrm = n_own[row];
    const float proj = nrm > 1e-12f ? dot : 0.f;
    if (k_lo < K) out[static_cast<size_t>(row) * K + k_lo] = (g0 - u0 * proj) / nrm;
    if (k_hi < K) out[static_cast<size_t>(row) * K + k_hi] = (g1 - u1 * proj) / nrm;
  }
}

}  // namespace cmh

using namespace cmh;

// tape f32 [kCpfHead + 2BK + CK + 2B + C]: the six f64 sums, the unit rows of hi and ht, the unit proxies, the divisors of the three
struct CpfTape { double* sums; float* unit; float* uw; float* div; size_t floats; };
static CpfTape carve_cpf_tape(float* tape, size_t B, size_t K, size_t C) {
  Carver c(tape);
  return {c.take<double>(kCpfHead * sizeof(float), 4), c.f32(2 * B * K * sizeof(float), 4), c.f32(C * K * sizeof(float), 4),
          c.f32((2 * B + C) * sizeof(float), 4), c.total() / sizeof(float)};
}
// part [2, row blocks, 4] f64, then a tape's worth for a forward without one
struct CpfWs { double* part; float* tape; size_t total; };
static CpfWs carve_cpf(void* ws, size_t B, size_t K, size_t C) {
  Carver c(ws);
  const size_t blocks = (B + kCpfRows - 1) / kCpfRows;
  return {c.take<double>(2 * blocks * 4 * sizeof(double)), c.f32(carve_cpf_tape(nullptr, B, K, C).floats * sizeof(float)), c.total()};
}
static bool cpf_in_range(int B, int K, int C) { return B >= 1 && B <= kCpfMaxB && K >= 1 && K <= kCpfMaxK && C >= 1 && C <= kCpfMaxC; }

extern "C" size_t cmh_cpf_workspace_bytes(int32_t B, int32_t K, int32_t C) { return cpf_in_range(B, K, C) ? carve_cpf(nullptr, B, K, C).total : 0; }
extern "C" size_t cmh_cpf_tape_bytes(int32_t B, int32_t K, int32_t C) {
  return cpf_in_range(B, K, C) ? carve_cpf_tape(nullptr, B, K, C).floats * sizeof(float) : 0;
}

static int cpf_shape(const char* what, int B, int K, int C) {
  CMH_CHECK_ARG(cpf_in_range(B, K, C), "%s: B=%d (1 .. %d) K=%d (1 .. %d) C=%d (1 .. %d)", what, B, kCpfMaxB, K, kCpfMaxK, C, kCpfMaxC);
  return CMH_OK;
}

extern "C" int cmh_cpf_loss(const float* hi, const float* ht, const float* labels, const float* proxies, int32_t B, int32_t K, int32_t C,
                            float tau, float psi, float sp, float sn, float mu, float b, float quant_weight, float* terms, float* loss,
                            float* cos, float* tape, void* workspace, size_t workspace_bytes, void* stream) {
  CMH_CHECK_ARG(hi && ht && labels && proxies && terms && loss && cos, "cpf_loss: null pointer");
  int rc = cpf_shape("cpf_loss", B, K, C);
  if (rc) return rc;
  if ((rc = open_ws("cpf_loss", workspace, workspace_bytes, carve_cpf(nullptr, B, K, C).total, CMH_ERR_INVALID))) return rc;
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "cpf_loss: workspace is not 256-byte aligned");
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(tape) & 7) == 0, "cpf_loss: tape is not 8-byte aligned");
  const CpfWs w = carve_cpf(workspace, B, K, C);
  const CpfTape tp = carve_cpf_tape(tape ? tape : w.tape, B, K, C);
  const CpfScalars s{tau, psi, sp, sn, mu, b};
  hipStream_t st = as_stream(stream);
  const unsigned blocks = (B + kCpfRows - 1) / kCpfRows;
  launch_normalize_rows(hi, tp.unit, tp.div, B, K, 1e-12f, nullptr, st);
  launch_normalize_rows(ht, tp.unit + static_cast<size_t>(B) * K, tp.div + B, B, K, 1e-12f, nullptr, st);
  launch_normalize_rows(proxies, tp.uw, tp.div + 2 * B, C, K, 1e-12f, nullptr, st);
  hipLaunchKernelGGL(cpf_rows_kernel, dim3(blocks, 2), dim3(256), 0, st, tp.unit, tp.uw, labels, B, K, C, s, cos, w.part);
  hipLaunchKernelGGL(cpf_fold_kernel, dim3(1), dim3(64), 0, st, w.part, static_cast<int>(blocks), B, K, s, quant_weight, terms, loss, tp.sums);
  CMH_CHECK_LAUNCH("cpf_loss");
  return CMH_OK;
}

extern "C" int cmh_cpf_loss_backward(const float* labels, const float* cos, const float* tape, int32_t B, int32_t K, int32_t C, float tau,
                                     float sp, float sn, float mu, float quant_weight, const float* dloss, float* d_hi, float* d_ht,
                                     float* d_proxies, void* stream) {
  CMH_CHECK_ARG(labels && cos && tape && dloss && d_hi && d_ht && d_proxies, "cpf_loss_backward: null pointer");
  int rc = cpf_shape("cpf_loss_backward", B, K, C);
  if (rc) return rc;
  CMH_CHECK_ARG((reinterpret_cast<uintptr_t>(tape) & 7) == 0, "cpf_loss_backward: tape is not 8-byte aligned");
  const CpfTape tp = carve_cpf_tape(const_cast<float*>(tape), B, K, C);
  const CpfScalars s{tau, 0.f, sp, sn, mu, 0.f};
  const unsigned blocks = (static_cast<unsigned>(B > C ? B : C) + kCpfRows - 1) / kCpfRows;
  hipLaunchKernelGGL(cpf_backward_kernel, dim3(blocks, 3), dim3(256), 0, as_stream(stream), tp.unit, tp.uw, tp.div, labels, cos, tp.sums, dloss,
                     B, K, C, s, quant_weight, d_hi, d_ht, d_proxies);
  CMH_CHECK_LAUNCH("cpf_loss_backward");
  return CMH_OK;
}
