// GEMM dispatch for the CLIP towers:  out[M,N] = epi( X[M,K] . W[N,K]^T )
//
// Replaces every nn.Linear / in_proj / conv1-as-GEMM of the reference's transformer blocks
// (model/base/model.py:171-196 ResidualAttentionBlock, :215 conv1, :250 proj, :370 text_projection).
//
// This file DECIDES every launch - plan_gemm: validation, kernel family, tile rows, grid, tile order, deferred QuickGELU, residual
// form, one grouped launch or two plain ones - and carries the measurement hook (cmh_prof_gemm_*).  The kernel files hold the
// kernels and a launcher that picks the template instance the finished plan names.  In the order plan_gemm asks:
//   M <= 2048 rows (pooled tail, projections)             -> gemm_rows_kernel   (gemm_rows.hip: 64 x 64 tiles, the wide kernel's bits)
//   N % 256 == 0 (every encoder GEMM)                     -> gemm_wide_kernel   (gemm_wide.hip: 160/128/96 x 256 persistent tiles)
//   ... bf16 block launches, by cmh_set_gemm_lc's mode    -> gemm_lc*_kernel    (gemm_lc.hip: loader / consumer forms, the same bits;
//       modes 1-3 the 8-wave kernel for every launch it has the epilogue for (mode 2: not the QuickGELU ones), 4 / 9 the 12-wave
//       128- / 160-row form, 7 the e4m3 form, 8 (default) the 160-row form where its replayed cost is below the wide kernel's -
//       never the 128-row form, never a residual launch)
//   N % 128 == 0 only (test-sized towers, width 128/384)  -> gemm_glds_kernel   (gemm_glds.hip: 128 x 128 LDS-DMA tiles)
// Round 1's register-staged 128 x 128 kernel (CMH_GEMM_IMPL=regstage) and round 3's two measured-slower experiments (the 256 x 256
// "big" tile, the LayerNorm fold inside the wide kernel) left the tree in round 4; DESIGN.md 4.3 keeps their numbers, git history
// (commit 20b80d8 and before) their code.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cmh_common.h"

#include <array>
#include <map>

namespace cmh {

constexpr int kTile = 128;             // N granule of the smallest tile any GEMM kernel of the library has
constexpr int kWideN = 256;            // tile columns of the wide kernel and of every loader / consumer form

// ---- the process-wide switches of the plan (cmh_set_gemm_lc's mode and cmh_set_gemm_rows' switch sit with their predicates) -------
// CMH_GEMM_WIDE=0 (A/B against round 1's 128 x 128 kernels): launches that do not need the wide kernel's epilogues avoid it
bool gemm_wide_enabled() {
  static const bool wide = []() { const char* e = getenv("CMH_GEMM_WIDE"); return !(e && !strcmp(e, "0")); }();
  return wide;
}
static int g_grouped = -1;   // cmh_set_gemm_grouped: -1 = environment (CMH_GEMM_GROUPED=0 switches grouping off)
static bool grouping_enabled() {
  static const bool env_on = []() { const char* e = getenv("CMH_GEMM_GROUPED"); return !(e && !strcmp(e, "0")); }();
  return g_grouped < 0 ? env_on : g_grouped != 0;
}
// Tuning overrides (cmh_gemm_tuning; initial values from CMH_GEMM_BM / CMH_GEMM_ORDER): -1 = decided per launch.  A pinned tile
// height names the wide kernel's own variants: no launch leaves for a loader / consumer form then.
static int g_force_rows = []() { const char* e = getenv("CMH_GEMM_BM"); return e ? atoi(e) : -1; }();
static int g_force_order = []() { const char* e = getenv("CMH_GEMM_ORDER"); return e ? atoi(e) : -1; }();

int gemm_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus < 8) cus = 256;
    cus &= ~7;   // whole groups of 8: blockIdx % 8 names the XCD share
  }
  return cus;
}

// n-panels per group of the wide kernel's tile order (see tile_coords in the kernel); 0 = the n-fastest order
int gemm_order_group(int N) {
  // Round 2 (tools/gemm_bench2.py + bench.py A/B on one box): GROUPS of 3-4 panels inside each XCD's band of m-tiles (ordG 1..64) are
  // +6 % on a back-to-back chain of a block's four GEMMs but -6 ... -10 % on the QKV / c_fc launches INSIDE the encoder (an X tile
  // is re-read once per group, after the outputs have passed through the L2): never the default.
  // Round 4: panel BLOCKS outermost (ordG >= 100, see tile_coords): 2 blocks for 4..11 panels, 3 from 12 on.  Fabric reads per launch
  // 116 -> 90 MB (QKV, N = 2304) and 185 -> 114 MB (c_fc, N = 3072), L2 hit rate 68-72 -> 76 % - and the SAME launch duration to
  // +-1 % (profiles/r04_d_gemm_nblocked_order_ab.txt, r04_d_gemm_nblocked_order_traffic.txt): the K loop does not wait on L2 misses.
  // It is the default for the traffic it saves the other tower's kernels (+0.4 % on the two-stream step, A/B/A/B on one box).
  const int tn = N / kWideN;
  auto blocked = [&](int nb) { return tn >= 2 * nb ? 100 + (tn + nb - 1) / nb : 0; };
  if (g_force_order <= -2) return blocked(-g_force_order);     // -NB: the n-blocked order with NB panel blocks
  if (g_force_order >= 0) return g_force_order;                 // 0: plain n-fastest; 1..64: round 2's panel groups
  return tn >= 12 ? blocked(3) : (tn >= 4 ? blocked(2) : 0);
}

// Deferred QuickGELU (the wide kernel's template parameter DGE): which launches take it, and what the activation costs a tile switch
// in the cost model below, in K-steps (tools/gemm_tile_cost.py: switch 1.70 / 1.77 / 2.19 us with a bias epilogue, 3.02 / 3.40 /
// 5.04 us with QuickGELU at 96 / 128 / 160 rows, K-steps of 0.68 / 0.80 / 0.96 us).  CMH_GEMM_DGE=0 turns the variant off (A/B runs).
static bool dge_applies(int dt, int epi, int mf, int kmin) {   // kmin: the shortest K of the launch - a tile's 8 pieces need 8 K-steps of the next
  static const bool off = []() { const char* e = getenv("CMH_GEMM_DGE"); return e && e[0] == '0'; }();
  return !off && dt == CMH_BF16 && mf == 4 && kmin >= 8 * 64 && (epi & EPI_QUICKGELU) && (epi & (EPI_OUT_BF16 | EPI_OUT_F16)) &&
         !(epi & ~(EPI_BIAS | EPI_QUICKGELU | EPI_OUT_BF16 | EPI_OUT_F16 | EPI_SAVE_PRE)) && (!(epi & EPI_SAVE_PRE) || (epi & EPI_OUT_BF16));
}
static int gelu_ksteps(int dt, int epi, int mf, int kmin) {
  if (!(epi & EPI_QUICKGELU) || dge_applies(dt, epi, mf, kmin)) return 0;
  return mf == 5 ? 3 : 2;
}

// ---- the cost model: one replay of the kernels' static tile assignment -------------------------------------------------------------
static int k_step(int dt) { return dt == CMH_F32 ? 32 : (dt == CMH_FP8 ? 128 : 64); }
static int tiles_of(int M, int N, int rows) { return (N / kWideN) * ((M + rows - 1) / rows); }
static int likely_rows(const GemmProblem& g) { return g.m_dev && g.m_hint > 0 && g.m_hint <= g.M ? g.m_hint : g.M; }   // a hint above M is ignored
// sized for the upper bounds of the row counts: workgroups beyond the real tile count exit at once
static int grid_of(const GemmProblem& a, const GemmProblem* b, int rows) {
  const int total = tiles_of(a.M, a.N, rows) + (b ? tiles_of(b->M, b->N, rows) : 0), cus = gemm_cus();
  return total < cus ? ((total + 7) & ~7) : cus;
}
// What a launch costs on `rows`-row tiles, for the wide kernel and the loader / consumer forms alike: the WORST workgroup of the
// persistent grid - a's tiles, then b's, dealt to 8 XCD shares x grid / 8 workgroup slots as the kernels deal them, for the likely
// row counts - in K-steps + 4 per tile (+ ge for an activation that is not deferred), x (rows + the per-K-step cost that does not
// shrink with the tile: W fragment reads, barrier).  One problem: slot 0 of the fullest share is the worst, ceil(tiles / CUs)
// rounds, which is the plain launches' cost of rounds 2-5 (tests/golden/gemm_plan.json pins that the two agree).
static long long tile_cost(int dt, const GemmProblem& a, const GemmProblem* b, int rows, int ge) {
  const int per = grid_of(a, b, rows) >> 3;
  const int t0 = tiles_of(likely_rows(a), a.N, rows), t1 = b ? tiles_of(likely_rows(*b), b->N, rows) : 0;
  const int c0 = a.K / k_step(dt) + 4 + ge, c1 = b ? b->K / k_step(dt) + 4 + ge : 0;
  long long worst = 0;
  for (int x = 0; x < 8; ++x) {
    const int len0 = deal_share(t0, x).len, len1 = deal_share(t1, x).len;
    for (int sl = 0; sl < (b ? per : 1); ++sl) {
      const int n0 = deal_count(len0, sl, per), nall = deal_count(len0 + len1, sl, per);
      const long long c = static_cast<long long>(n0) * c0 + static_cast<long long>(nall - n0) * c1;
      worst = c > worst ? c : worst;
    }
  }
  return worst * (10 * (rows / 32) + 6);
}

// The wide kernel's tile rows: 160, 128 or 96, whichever costs this launch least (ties go to the taller tile); *cost: that cost.
// M = 12 800 / 19 712 (the dense towers) take 160; the packed text rows (M ~ 10 k) take 128 at N = 1536 / 2048 and 96 at N = 512,
// where one round of 220 tiles keeps 86 % of the CUs busy instead of 65 % (166 tiles of 128 rows).
// fp8: 160 rows by default only with e4m3 OUTPUT (the c_fc launches).  The 160-row variant needs 56 fragment registers live across the epilogue
// (both 16-byte halves of the next K-step's operands, as aligned 8-register MFMA operands) next to 80 accumulators and the pending
// stores; left alone hipcc spills inside the K loop (scratch reloads with vmcnt(0) drain the LDS-DMA pipeline: measured 64 us
// against bf16's 46 on QKV).  With the epilogue paths fp8 never takes compiled out, the residual loads in two groups and - for the
// 16-bit outputs - only 4 of the 10 stores deferred, the K loops of the e4m3- and 16-bit-output variants are free of scratch
// (tools/asm_loop_scratch.py: every variant a launch can select must show no scratch at loop depth 2).
// (the f32-output fp8 variant still spills in its K loop; the 16-bit-output one is loop-clean but pays 28 scratch instructions per
// tile in its epilogue: serialized GEMM time of an fp8 step -1.3 %, the overlapped step -1.5 % in pairs/s, A/B/A/B on one box - so
// it is taken only on request, CMH_GEMM_BM=160 / cmh_gemm_tuning, and by plain launches alone)
static int wide_tile_rows(int dt, const GemmProblem& a, const GemmProblem* b, int epi, long long* cost) {
  const int kmin = b && b->K < a.K ? b->K : a.K;
  auto cost_of = [&](int mf) { return tile_cost(dt, a, b, 32 * mf, gelu_ksteps(dt, epi, mf, kmin)); };
  int mf = dt == CMH_FP8 && !(epi & EPI_OUT_FP8) ? 4 : 5;
  long long best = cost_of(mf);
  for (int m = mf - 1; m >= 3; --m) {
    const long long c = cost_of(m);
    if (c < best) { best = c; mf = m; }
  }
  *cost = best;
  return 32 * mf;
}
static int forced_tile_rows(int dt, bool grouped, int epi, int rows) {
  const bool fp8_160 = epi & (grouped ? EPI_OUT_FP8 : EPI_OUT_FP8 | EPI_OUT_BF16 | EPI_OUT_F16);
  const int forced = g_force_rows;
  return forced == 96 || forced == 128 || (forced == 160 && (dt != CMH_FP8 || fp8_160)) ? forced : rows;
}

// the wide kernel's residual-first rule (gemm_wide.hip, res_first), per GEMM: a short K without an activation starts from the residual
static bool res_first(int epi, int K) { return (epi & EPI_RESIDUAL) && !(epi & (EPI_QUICKGELU | EPI_GELU | EPI_RELU)) && K / 64 <= 16; }

// Which loader / consumer form takes a launch the wide kernel could run (b: the second problem of a grouped launch): 0 none, 1 the
// 8-wave kernel, 2 the 12-wave form on 128-row tiles (lc2), 3 on 160-row tiles (lc3).  Both problems must be the form's, with the
// same residual form.  Mode 8 (the default) prices the 160-row form against the wide kernel (`wide_cost`), both by tile_cost.
static int lc_route(int dt, const GemmProblem& a, const GemmProblem* b, int epi, long long wide_cost) {
  const int mode = gemm_lc_mode();
  if (mode == 0 || mode == 7 || g_force_rows > 0 || (mode == 2 && (epi & EPI_QUICKGELU))) return 0;
  if (!gemm_lc_takes(dt, a.N, a.K, epi)) return 0;
  if (b && (!gemm_lc_takes(dt, b->N, b->K, epi) || res_first(epi, a.K) != res_first(epi, b->K))) return 0;
  if (mode >= 1 && mode <= 3) return 1;
  if (mode == 4) return 2;
  if (mode == 9) return 3;
  if (mode != 8) return 0;
  // The 160-row form against the wide kernel: its K-step priced at 56/64 of the wide kernel's (83 % MFMA issue against 65-72 %), its
  // tiles by the same static assignment.  It never takes a residual launch: its residual forms spill 27-28 scratch instructions per
  // tile in the epilogue (none in the K loop) and measured 1.02-1.5 x the wide kernel on all six (profiles/r06_a_lc_per_shape.txt).
  // The 128-row form (lc2) is not routed: with its reads compiler-counted it measured 1.08 x on grouped out_proj, the one block launch
  // where the hand-counted form had won (0.93; profiles/r06_d_route_ab.txt), and it stays an opt-in (mode 4).
  if (epi & EPI_RESIDUAL) return 0;
  return tile_cost(dt, a, b, 160, 0) * 56 / 64 < wide_cost ? 3 : 0;
}

// A launch the wide kernel can run: the loader / consumer form the route names, the e4m3 form (mode 7), or the wide kernel itself.
// who: "gemm" / "gemm (grouped)", for the message.
static int plan_wide_side(const char* who, int dt, const GemmProblem& a, const GemmProblem* b, int epi, GemmPlan* p) {
  long long wide_cost;
  const int rows = wide_tile_rows(dt, a, b, epi, &wide_cost);
  const int form = lc_route(dt, a, b, epi, wide_cost);
  if (form) {
    p->family = GEMM_LC + form - 1;
    p->rows = form == 3 ? 160 : 128;
  } else if (dt == CMH_FP8 && !b && g_force_rows <= 0 && gemm_lc2q_takes(a.N, a.K, epi)) {
    p->family = GEMM_LC2Q;
    p->rows = 128;
  } else {
    p->family = GEMM_WIDE;
    p->rows = forced_tile_rows(dt, b != nullptr, epi, rows);
    p->order = b ? 0 : gemm_order_group(a.N);
    p->dge = dge_applies(dt, epi, p->rows / 32, b && b->K < a.K ? b->K : a.K);
  }
  p->grid = grid_of(a, b, p->rows);
  const size_t esz = dt == CMH_F32 ? 4 : (dt == CMH_FP8 ? 1 : 2);
  for (const GemmProblem* g : {&a, b}) {
    if (!g || (static_cast<size_t>(g->M) * g->K * esz < (1ull << 32) && static_cast<size_t>(kWideN) * g->K * esz < (1ull << 32))) continue;
    if (p->family == GEMM_WIDE)
      return fail(CMH_ERR_INVALID, "%s: operand of %zu bytes exceeds the 32-bit offset range of the wide kernel", who,
                  static_cast<size_t>(g->M) * g->K * esz);
    return fail(CMH_ERR_INVALID, "gemm (lc): operand of %zu bytes exceeds the 32-bit offset range", static_cast<size_t>(g->M) * g->K * esz);
  }
  return CMH_OK;
}

// Does ONE grouped launch beat two plain ones?  tile_cost of the pair against the two plain launches' (each at its best tile height),
// plus a fixed ~8 K-steps per LAUNCH (first stage landing on every CU at once, last epilogue's store drain:
// profiles/r02_a_gemm_launch_timeline.txt).  Measured at batch 256 (profiles/r04_b_grouped_per_shape.txt): QKV 74.5 -> 68.8 us,
// out_proj 41.8 -> 36.9, c_fc 104.8 -> 96.4 grouped - but c_proj 92.0 -> 98.3: one 48-K-step image tile per workgroup plus a
// 32-K-step text tile on every second one is a worse packing than two launches; the model reproduces all four.
static bool grouping_pays(int dt, const GemmProblem& a, const GemmProblem& b, int epi) {
  static const bool always = []() { const char* e = getenv("CMH_GEMM_GROUPED"); return e && !strcmp(e, "always"); }();
  if (always || g_force_rows > 0) return true;            // (a forced tile height: A/B runs and the tests that walk every variant)
  const long long fixed = 8 * 56;
  long long both, ca, cb;
  (void)wide_tile_rows(dt, a, &b, epi, &both);
  (void)wide_tile_rows(dt, a, nullptr, epi, &ca);
  (void)wide_tile_rows(dt, b, nullptr, epi, &cb);
  return both + fixed <= ca + cb + 2 * fixed;
}

static const char* const kNeedsDq = "gemm: EPI_MUL_DQGELU needs aux in the residual slot, N %% 256 == 0 (N=%d), no residual / fp16 output";
static const char* const kNeedsPre = "gemm: EPI_SAVE_PRE needs the second output in the residual slot, bf16 operands and output, N %% 256 == 0 (N=%d)";

// THE decision of a launch: everything about it that does not need the operands' addresses is checked and chosen here, on the host,
// before anything is recorded or launched (cmh_gemm_plan asks without launching).  epi: as the caller passes it (fp8: EPI_SCALE is
// implied).  b: a grouped request - the same layer of both towers as ONE launch when the wide kernel or a loader / consumer form can
// take both problems and the cost model expects one launch to be faster; two plain launches otherwise (p->launches = 2; identical
// results either way).
int plan_gemm(int dt, const GemmProblem& a, const GemmProblem* b, int epi, GemmPlan* p) {
  const bool fp8 = dt == CMH_FP8;
  if (fp8) epi |= EPI_SCALE;
  *p = GemmPlan{1, GEMM_WIDE, 0, 0, 0, !(epi & EPI_RESIDUAL) ? 0 : (res_first(epi, a.K) ? 1 : 2), false, false};
  const bool wide = gemm_wide_enabled();
  const int M = a.M, N = a.N, K = a.K;
  if (b) {
    auto fits = [&](const GemmProblem& g) {
      return g.M > 0 && g.K > 0 && gemm_wide_supported(g.N) && g.K % k_step(dt) == 0 && (g.m_dev || !gemm_rows_takes(g.M, g.N, g.K, epi));
    };
    const bool groupable = (fp8 || dt == CMH_F32 || dt == CMH_BF16) && grouping_enabled() && wide && fits(a) && fits(*b) && !(epi & (EPI_MUL_DQGELU | EPI_SAVE_PRE)) &&
                           (fp8 ? (epi & (EPI_OUT_BF16 | EPI_OUT_F16 | EPI_OUT_FP8)) != 0
                                : (dt == CMH_BF16) == ((epi & (EPI_OUT_BF16 | EPI_OUT_F16)) != 0));
    p->swap = a.K < b->K;      // the longer K first: its tiles are the long jobs of the static schedule
    const GemmProblem &first = p->swap ? *b : a, &second = p->swap ? a : *b;
    if (!groupable || !grouping_pays(dt, first, second, epi)) {
      p->launches = 2;
      return CMH_OK;
    }
    p->res = !(epi & EPI_RESIDUAL) ? 0 : (res_first(epi, first.K) ? 1 : 2);
    return plan_wide_side("gemm (grouped)", dt, first, &second, epi, p);
  }
  if (fp8) {
    CMH_CHECK_ARG(M > 0 && N > 0 && K > 0, "gemm_fp8: empty problem M=%d N=%d K=%d", M, N, K);
    CMH_CHECK_ARG(gemm_wide_supported(N) && K % 128 == 0, "gemm_fp8: N=%d must be a multiple of 256 and K=%d of 128", N, K);
    CMH_CHECK_ARG(!(epi & EPI_MUL_DQGELU), "gemm_fp8: forward epilogues only");
    const int okinds = ((epi & EPI_OUT_BF16) ? 1 : 0) + ((epi & EPI_OUT_F16) ? 1 : 0) + ((epi & EPI_OUT_FP8) ? 1 : 0);
    CMH_CHECK_ARG(okinds <= 1, "gemm_fp8: one output type at a time");
  } else {
    CMH_CHECK_ARG(dt == CMH_F32 || dt == CMH_BF16, "gemm: bad dtype %d", dt);
    CMH_CHECK_ARG(M > 0 && N > 0 && K > 0, "gemm: empty problem M=%d N=%d K=%d", M, N, K);
    CMH_CHECK_ARG(N % kTile == 0, "gemm: N=%d must be a multiple of %d", N, kTile);
    CMH_CHECK_ARG(K % k_step(dt) == 0, "gemm: K=%d must be a multiple of %d", K, k_step(dt));
    CMH_CHECK_ARG(!(epi & (EPI_RES_F16 | EPI_OUT_F16)) || (gemm_wide_supported(N) && !(epi & EPI_OUT_BF16)),
                  "gemm: fp16 residual / output needs N %% 256 == 0 (N=%d) and excludes EPI_OUT_BF16", N);
    CMH_CHECK_ARG(!(epi & EPI_MUL_DQGELU) || (gemm_wide_supported(N) && !(epi & (EPI_RESIDUAL | EPI_OUT_F16))), kNeedsDq, N);
    CMH_CHECK_ARG(!(epi & EPI_SAVE_PRE) || (dt == CMH_BF16 && (epi & EPI_OUT_BF16) && gemm_wide_supported(N) &&
                                            !(epi & (EPI_RESIDUAL | EPI_MUL_DQGELU | EPI_OUT_F16))), kNeedsPre, N);
  }
  if (wide && !a.m_dev && gemm_rows_takes(M, N, K, epi)) {      // few rows: 64 x 64 tiles (the wide kernel's bits: off with it)
    p->family = GEMM_ROWS;
    p->rows = 64;
    p->grid = (N / 64) * ((M + 63) / 64);
  } else if (fp8 || (wide && gemm_wide_supported(N)) || (epi & (EPI_RES_F16 | EPI_OUT_F16 | EPI_MUL_DQGELU | EPI_SAVE_PRE))) {
    return plan_wide_side("gemm", dt, a, nullptr, epi, p);
  } else {
    CMH_CHECK_ARG(!a.m_dev, "gemm: a device-side row count needs the wide kernel (N %% 256 == 0, N=%d)", N);
    static const int order = []() { const char* e = getenv("CMH_GEMM_ORDER"); return e ? atoi(e) : 0; }();
    p->family = GEMM_FALLBACK;
    p->rows = kTile;
    p->grid = (N / kTile) * ((M + kTile - 1) / kTile);
    p->order = order;
  }
  return CMH_OK;
}

// ---- optional launch timing (bench.py roofline): HIP events around every GEMM launch on its own stream ----
struct GemmProf {
  bool on = false;
  std::vector<hipEvent_t> ev;     // pairs
  std::vector<double> flops;
  std::vector<std::array<int, 4>> dims;   // M, N, K, epi of each timed launch (CMH_GEMM_PROF_DUMP breakdown)
  std::vector<int> kind;                  // name each timed launch is counted under: see kind_of
  // device-side row counts (packed text): copied, asynchronously, into a pinned slot at launch time and turned into FLOPs by _end()
  // - the hook itself never waits for the stream, so a profiled region keeps the launch queue of an unprofiled one
  struct Pending { size_t launch; int slot; int Mub; double flops_per_row; };
  std::vector<Pending> pending;
  std::map<const int32_t*, int> slot_of;  // one copy per device word and session: every launch that names the word shares its slot
  int32_t* rows_pinned = nullptr;
  size_t rows_cap = 0, rows_used = 0;
  size_t used = 0;
};
static GemmProf g_prof;

// The three names cmh_prof_gemm_by_kernel (and bench.py's roofline) counts launches under: [0] "gemm_wide_kernel" is the wide kernel
// AND every loader / consumer form (lc, lc2, lc3, lc2q: other schedules of its arithmetic on the same launches), [1]
// "gemm_rows_kernel" the few-row kernel, [2] "fallback" the 128 x 128 kernel.
static int kind_of(int family) { return family == GEMM_ROWS ? 1 : (family == GEMM_FALLBACK ? 2 : 0); }
constexpr int kKindConv1 = 3;      // a fourth name, outside the three: the fused conv1 stem (conv1_stem.hip; cmh_prof_gemm_conv1_fused)

// the measurement hook counts algorithmic FLOPs on REAL rows: FLOPs of `flops_per_row` x the rows of launch `launch` (the entry
// g_prof.flops[launch] is created by the caller with the upper bound's FLOPs and corrected by _end() once the count has arrived)
static void prof_rows_later(size_t launch, int Mub, const int32_t* m_dev, double flops_per_row, hipStream_t st) {
  if (!m_dev || !g_prof.rows_pinned) return;
  // (a copy per LAUNCH would put ~46 four-byte copies of 4-5 us each into every profiled step of the single-stream pair mode; the
  // word is read once per profiling session - a session measures repetitions of one batch - by the first launch that names it)
  auto it = g_prof.slot_of.find(m_dev);
  int slot;
  if (it != g_prof.slot_of.end()) {
    slot = it->second;
  } else {
    if (g_prof.rows_used >= g_prof.rows_cap) return;
    slot = static_cast<int>(g_prof.rows_used);
    g_prof.rows_pinned[slot] = -1;
    if (hipMemcpyAsync(g_prof.rows_pinned + slot, m_dev, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return;
    ++g_prof.rows_used;
    g_prof.slot_of[m_dev] = slot;
  }
  g_prof.pending.push_back({launch, slot, Mub, flops_per_row});
}

// The hook of a launch.  Every kernel but the 128 x 128 one launches through hipExtLaunchKernelGGL, which stamps the pair handed to
// its launcher with the DISPATCH's own begin / end (what rocprofv3's kernel trace reports); the 128 x 128 kernel - and, under
// CMH_GEMM_PROF_BRACKET=1 (round 1-2's method, for comparison), every launch - is bracketed by two recorded events instead, which
// adds the marker packets' gaps.  Outside a session both events stay null and nothing is recorded.
struct GemmTimer { bool timed; hipEvent_t ev0, ev1; };
static GemmTimer prof_open(const GemmPlan& p, hipStream_t st) {
  const bool timed = g_prof.on && g_prof.used + 2 <= g_prof.ev.size();
  if (!timed) return {false, nullptr, nullptr};
  static const bool bracket = []() { const char* e = getenv("CMH_GEMM_PROF_BRACKET"); return e && e[0] == '1'; }();
  if (p.family != GEMM_FALLBACK && !bracket) return {true, g_prof.ev[g_prof.used], g_prof.ev[g_prof.used + 1]};
  (void)hipEventRecord(g_prof.ev[g_prof.used], st);
  return {true, nullptr, nullptr};
}
static void prof_close(const GemmTimer& t, const GemmPlan& p, const GemmProblem& a, const GemmProblem* b, int epi, hipStream_t st) {
  if (!t.timed) return;
  if (!t.ev0) (void)hipEventRecord(g_prof.ev[g_prof.used + 1], st);
  double flops = 0.0;                                   // algorithmic FLOPs (real rows only: corrected by _end)
  for (const GemmProblem* g : {&a, b}) if (g) flops += 2.0 * g->M * static_cast<double>(g->N) * g->K;
  g_prof.flops.push_back(flops);
  for (const GemmProblem* g : {&a, b}) if (g) prof_rows_later(g_prof.flops.size() - 1, g->M, g->m_dev, 2.0 * static_cast<double>(g->N) * g->K, st);
  if (b) g_prof.dims.push_back({a.M + b->M, a.N + b->N, a.K, epi | (1 << 20)});   // (1 << 20: a grouped launch; rows / columns summed)
  else g_prof.dims.push_back({a.M, a.N, a.K, epi});
  g_prof.kind.push_back(kind_of(p.family));
  g_prof.used += 2;
}

// The same hook for the one GEMM that launches outside run_gemm (conv1_stem.hip: it stamps the pair through hipExtLaunchKernelGGL)
bool gemm_prof_open_conv1(hipEvent_t* ev0, hipEvent_t* ev1) {
  if (!g_prof.on || g_prof.used + 2 > g_prof.ev.size()) return false;
  *ev0 = g_prof.ev[g_prof.used];
  *ev1 = g_prof.ev[g_prof.used + 1];
  return true;
}
void gemm_prof_close_conv1(int M, int N, int K) {
  g_prof.flops.push_back(2.0 * M * static_cast<double>(N) * K);
  g_prof.dims.push_back({M, N, K, 0});
  g_prof.kind.push_back(kKindConv1);
  g_prof.used += 2;
}

// ---- the one launch path: plan, check the operands, launch what the plan names -------------------------------------------------------
static int check_operands(const char* who, int dt, const GemmProblem& g, int epi, bool grouped) {
  CMH_CHECK_ARG(g.A && g.W && g.out && (grouped || dt != CMH_FP8 || g.colscale), "%s: null pointer", who);
  CMH_CHECK_ARG(dt != CMH_FP8 || g.colscale, "%s: fp8 operands without weight scales", who);
  CMH_CHECK_ARG(!(epi & EPI_BIAS) || g.bias, "%s: EPI_BIAS without bias", who);
  CMH_CHECK_ARG(!(epi & EPI_RESIDUAL) || g.residual, "%s: EPI_RESIDUAL without residual", who);
  CMH_CHECK_ARG(!(epi & EPI_MUL_DQGELU) || g.residual, kNeedsDq, g.N);
  CMH_CHECK_ARG(!(epi & EPI_SAVE_PRE) || g.residual, kNeedsPre, g.N);
  return CMH_OK;
}

static int run_gemm(const char* who, int dt, const GemmProblem& a, const GemmProblem* b, int epi, hipStream_t st) {
  GemmPlan p;
  if (const int rc = plan_gemm(dt, a, b, epi, &p)) return rc;
  if (p.launches == 2) {
    for (const GemmProblem* g : {&a, b})
      if (const int rc = run_gemm(dt == CMH_FP8 ? "gemm_fp8" : "gemm", dt, *g, nullptr, epi, st)) return rc;
    return CMH_OK;
  }
  for (const GemmProblem* g : {&a, b})
    if (g)
      if (const int rc = check_operands(who, dt, *g, epi, b != nullptr)) return rc;
  const int kepi = dt == CMH_FP8 ? epi | EPI_SCALE : epi;
  const GemmProblem& first = p.swap ? *b : a;
  const GemmProblem* second = !b ? nullptr : (p.swap ? &a : b);
  const GemmTimer t = prof_open(p, st);
  int rc;
  switch (p.family) {
    case GEMM_ROWS: rc = launch_gemm_rows(dt, a, kepi, p, st, t.ev0, t.ev1); break;
    case GEMM_FALLBACK: rc = launch_gemm_glds(dt, a, kepi, p, st); break;
    case GEMM_WIDE: rc = launch_gemm_wide(dt, first, second, kepi, p, st, t.ev0, t.ev1); break;
    case GEMM_LC2Q: rc = launch_gemm_lc2q(a, kepi, p, st, t.ev0, t.ev1); break;
    default: rc = launch_gemm_lc(first, second, kepi, p, st, t.ev0, t.ev1); break;
  }
  if (rc) return rc;
  prof_close(t, p, a, b, b ? epi : kepi, st);
  CMH_CHECK_LAUNCH(who);
  return CMH_OK;
}

int launch_gemm(int dt, const void* A, const void* W, const float* bias, const float* residual, void* out,
                int M, int N, int K, int epi, hipStream_t st, const int32_t* m_dev, int m_hint) {
  return run_gemm("gemm", dt, GemmProblem{A, W, bias, residual, out, M, N, K, m_dev, m_hint, nullptr, 1.f, 1.f}, nullptr, epi, st);
}

int launch_gemm_fp8(const void* A8, const void* W8, const float* colscale, float alpha, const float* bias, const float* residual,
                    void* out, float oscale, int M, int N, int K, int epi, hipStream_t st, const int32_t* m_dev, int m_hint) {
  return run_gemm("gemm_fp8", CMH_FP8, GemmProblem{A8, W8, bias, residual, out, M, N, K, m_dev, m_hint, colscale, alpha, oscale}, nullptr,
                  epi, st);
}

// The same layer of both towers: ONE launch when plan_gemm says so, two plain ones otherwise (identical results either way)
int launch_gemm_grouped(int dt, const GemmProblem& a, const GemmProblem& b, int epi, hipStream_t st) {
  return run_gemm("gemm (grouped)", dt, a, &b, epi, st);
}

}  // namespace cmh

extern "C" int cmh_set_gemm_grouped(int32_t on) { cmh::g_grouped = on < 0 ? -1 : (on ? 1 : 0); return CMH_OK; }

extern "C" int cmh_gemm_tuning(int32_t tile_rows, int32_t order_group) {
  using namespace cmh;
  CMH_CHECK_ARG(tile_rows == -1 || tile_rows == 96 || tile_rows == 128 || tile_rows == 160, "gemm_tuning: tile_rows %d (-1, 96, 128, 160)", tile_rows);
  CMH_CHECK_ARG(order_group >= -8 && order_group <= 64, "gemm_tuning: order_group %d (-8..-2: n-blocked, -1: default, 0: n-fastest, > 0: panel groups)", order_group);
  g_force_rows = tile_rows;
  g_force_order = order_group;
  return CMH_OK;
}

extern "C" int cmh_gemm_route(int32_t dt, int32_t Ma, int32_t Na, int32_t Ka, int32_t Mb, int32_t Nb, int32_t Kb, int32_t epi) {
  using namespace cmh;
  CMH_CHECK_ARG(Ma > 0 && Na > 0 && Ka > 0 && Mb >= 0, "gemm_route: shape %d x %d x %d / %d rows", Ma, Na, Ka, Mb);
  const GemmProblem a{nullptr, nullptr, nullptr, nullptr, nullptr, Ma, Na, Ka, nullptr, 0, nullptr, 1.f, 1.f};
  const GemmProblem b{nullptr, nullptr, nullptr, nullptr, nullptr, Mb, Nb, Kb, nullptr, 0, nullptr, 1.f, 1.f};
  long long wide_cost;
  (void)wide_tile_rows(dt, a, Mb > 0 ? &b : nullptr, epi, &wide_cost);
  return lc_route(dt, a, Mb > 0 ? &b : nullptr, epi, wide_cost);
}

extern "C" int cmh_gemm_plan(int32_t dt, int32_t epi, const int32_t* a5, const int32_t* b5, int32_t* out16) {
  using namespace cmh;
  CMH_CHECK_ARG(a5 && out16, "gemm_plan: null pointer");
  static const int32_t rows_word = 0;      // stands for a device word: the plan never reads it
  auto problem = [&](const int32_t* s) {
    return GemmProblem{nullptr, nullptr, nullptr, nullptr, nullptr, s[0], s[1], s[2], s[3] ? &rows_word : nullptr, s[4], nullptr, 1.f, 1.f};
  };
  auto put = [](const GemmPlan& p, bool grouped, int32_t* o) {
    o[0] = p.family; o[1] = p.rows; o[2] = p.grid; o[3] = p.order; o[4] = p.dge; o[5] = p.res; o[6] = grouped;
  };
  for (int i = 0; i < 16; ++i) out16[i] = 0;
  const GemmProblem a = problem(a5), b = problem(b5 ? b5 : a5);
  out16[1] = cmh_gemm_route(dt, a.M, a.N, a.K, b5 ? b.M : 0, b.N, b.K, dt == CMH_FP8 ? epi | EPI_SCALE : epi);
  if (out16[1] < 0) return out16[1];
  GemmPlan p;
  if (const int rc = plan_gemm(dt, a, b5 ? &b : nullptr, epi, &p)) return rc;
  out16[0] = p.launches;
  if (p.launches == 1) {
    put(p, b5 != nullptr, out16 + 2);
    return CMH_OK;
  }
  for (int i = 0; i < 2; ++i) {
    if (const int rc = plan_gemm(dt, i ? b : a, nullptr, epi, &p)) return rc;
    put(p, false, out16 + 2 + 7 * i);
  }
  return CMH_OK;
}

extern "C" int cmh_prof_gemm_begin(int32_t max_launches) {
  using namespace cmh;
  CMH_CHECK_ARG(max_launches > 0 && max_launches <= (1 << 20), "prof_gemm_begin: bad max_launches");
  while (g_prof.ev.size() < static_cast<size_t>(max_launches) * 2) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return fail(CMH_ERR_LAUNCH, "prof_gemm_begin: hipEventCreate failed");
    g_prof.ev.push_back(e);
  }
  if (g_prof.rows_cap < static_cast<size_t>(max_launches) * 2) {      // (profiling only: the product path never allocates here)
    if (g_prof.rows_pinned) (void)hipHostFree(g_prof.rows_pinned);
    g_prof.rows_pinned = nullptr;
    g_prof.rows_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&g_prof.rows_pinned), static_cast<size_t>(max_launches) * 2 * 4, hipHostMallocDefault) == hipSuccess)
      g_prof.rows_cap = static_cast<size_t>(max_launches) * 2;
    else
      g_prof.rows_pinned = nullptr;
  }
  g_prof.rows_used = 0;
  g_prof.pending.clear();
  g_prof.slot_of.clear();
  g_prof.used = 0;
  g_prof.flops.clear();
  g_prof.dims.clear();
  g_prof.kind.clear();
  g_prof.on = true;
  return CMH_OK;
}

extern "C" int cmh_prof_gemm_by_kernel(double* ms3, double* flops3, int64_t* launches3) {
  using namespace cmh;
  CMH_CHECK_ARG(ms3 && flops3 && launches3, "prof_gemm_by_kernel: null pointer");
  CMH_CHECK_ARG(!g_prof.on, "prof_gemm_by_kernel: call cmh_prof_gemm_end first");
  for (int k = 0; k < 3; ++k) { ms3[k] = 0.0; flops3[k] = 0.0; launches3[k] = 0; }
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "prof_gemm_by_kernel: hipEventElapsedTime failed");
    const int k = g_prof.kind[i / 2];
    if (k == kKindConv1) continue;      // (cmh_prof_gemm_conv1_fused's)
    ms3[k] += t; flops3[k] += g_prof.flops[i / 2]; launches3[k] += 1;
  }
  return CMH_OK;
}

extern "C" int cmh_prof_gemm_conv1_fused(double* ms, double* flops, int64_t* launches) {
  using namespace cmh;
  CMH_CHECK_ARG(ms && flops && launches, "prof_gemm_conv1_fused: null pointer");
  CMH_CHECK_ARG(!g_prof.on, "prof_gemm_conv1_fused: call cmh_prof_gemm_end first");
  *ms = 0.0; *flops = 0.0; *launches = 0;
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    if (g_prof.kind[i / 2] != kKindConv1) continue;
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "prof_gemm_conv1_fused: hipEventElapsedTime failed");
    *ms += t; *flops += g_prof.flops[i / 2]; *launches += 1;
  }
  return CMH_OK;
}

extern "C" int cmh_prof_gemm_end(double* total_ms, double* total_flops, int64_t* launches) {
  using namespace cmh;
  CMH_CHECK_ARG(total_ms && total_flops && launches, "prof_gemm_end: null pointer");
  g_prof.on = false;
  if (hipDeviceSynchronize() != hipSuccess) return fail(CMH_ERR_LAUNCH, "prof_gemm_end: device synchronisation failed");   // (the row-count copies too)
  double ms = 0.0, fl = 0.0;
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    if (hipEventSynchronize(g_prof.ev[i + 1]) != hipSuccess) return fail(CMH_ERR_LAUNCH, "prof_gemm_end: event sync failed");
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess)
      return fail(CMH_ERR_LAUNCH, "prof_gemm_end: hipEventElapsedTime failed");
    ms += t;
  }
  // every event has completed, so has every row-count copy queued before it: real rows instead of the upper bounds
  for (const auto& p : g_prof.pending) {
    const int got = g_prof.rows_pinned[p.slot];
    if (got > 0 && got < p.Mub) {
      g_prof.flops[p.launch] -= static_cast<double>(p.Mub - got) * p.flops_per_row;
      g_prof.dims[p.launch][0] -= p.Mub - got;
    }
  }
  g_prof.pending.clear();
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) fl += g_prof.flops[i / 2];
  if (getenv("CMH_GEMM_PROF_DUMP")) {   // per-shape breakdown of the timed launches, to stderr
    std::map<std::array<int, 4>, std::array<double, 3>> by;   // dims -> {ms, flops, launches}
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
      float t = 0.f;
      (void)hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]);
      auto& e = by[g_prof.dims[i / 2]];
      e[0] += t; e[1] += g_prof.flops[i / 2]; e[2] += 1;
    }
    for (const auto& kv : by)
      fprintf(stderr, "gemm M=%6d N=%5d K=%5d epi=%3d  launches %5.0f  avg %8.2f us  %7.1f TF/s  share %5.1f%%\n", kv.first[0],
              kv.first[1], kv.first[2], kv.first[3], kv.second[2], kv.second[0] * 1e3 / kv.second[2],
              kv.second[1] / (kv.second[0] * 1e-3) / 1e12, 100.0 * kv.second[0] / ms);
  }
  *total_ms = ms;
  *total_flops = fl;
  *launches = static_cast<int64_t>(g_prof.used / 2);
  return CMH_OK;
}
