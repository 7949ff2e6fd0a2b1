// Which kernel runs a bf16 GEMM problem (csrc/gemm.hip): one pure host function, plan_gemm, from the problem,
// the CU count and the knobs to a GemmPlan.  dtc_gemm launches from the plan; dtc_gemm_plan and the planning
// queries (split-K factors, part counts, "this dgrad takes its own launch") read the same plan, so they cannot
// drift from what launches.  No HIP header: this file compiles with a plain C++ compiler.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>

namespace gp {

// epilogue codes of common.h (gemm.hip asserts they agree)
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_GELU = 2, EPI_DGELU = 3, EPI_LMHEAD = 4, EPI_LMHEAD_EVAL = 7 };
constexpr int BIG = 256;  // tile edge of the 256^2 kernels

// Kernel families, as recorded by the launch sites (dtc_gemm_last_launch) and planned here.
enum {
  FAM_NONE = 0,
  FAM_REG = 1,       // gemm_kernel, register-staged; sub = BK (32 / 64)
  FAM_DMA64 = 2,     // gemm_dma_kernel 64^2 NT; sub = stages
  FAM_DMAW = 3,      // gemm_dmaw_kernel; sub = stages, aux = wave grid WGM * 10 + WGN
  FAM_BIG = 4,       // gemm8p_kernel; sub = CB (4 = 256^2, 3 = the 256 x 192 plan)
  FAM_R8 = 5,        // gemm8r_kernel; sub = CB2, aux = n_split (columns on 256^2 tiles)
  FAM_N8 = 6,        // gemm8n_kernel; sub = CB
  FAM_PAIR = 7,      // gemm_pair_kernel; bm / bn = dgrad / weight-gradient tile, split = the weight gradient's
  FAM_WGROUP = 8,    // gemm8p_group_kernel; split = tail split, sub = tail tiles, aux = all tiles
  FAM_CE_DGRAD = 9,  // ce_dgrad256_kernel
  FAM_LN = 10,       // gemm_dmaw_kernel with a LayerNorm epilogue; sub = 1 backward, 0 forward
  FAM_COUNT = 11,
};

// ---- knobs ---------------------------------------------------------------------------------------------
// Every environment switch of the bf16 GEMM dispatch, read once (gemm.hip keeps the one instance; the
// dtc_gemm_set_* entry points write into it).  docs/KNOBS.md describes them.
struct Knobs {
  int dma_fwd64 = 1;           // DTC_GEMM_DMA: LDS-DMA variant of the 64^2 forward tiles (0: register-staged everywhere)
  int wgrad_blocks_128 = 256;  // DTC_WGRAD_BLOCKS sets both: the block count the split-K of a weight gradient
  int wgrad_blocks_64 = 512;   //   aims at, on 128^2 tiles and on 64^2 tiles
  int wide_gm = 3;             // DTC_WIDE_GM: tile-group height for grids with many N-tiles (0 = tiles_m)
  int wgrad_cs256 = 1;         // DTC_WGRAD_CS256=0: bias gradients of the 256^2 weight gradients as a separate column sum
  int wgrad256 = 1;            // DTC_WGRAD256: layer weight gradients split-K on the 256^2 kernel
  int gemm256 = 7;             // DTC_GEMM256: bit mask of layouts allowed the 256^2 kernel (1 fwd, 2 dgrad, 4 wgrad)
  int big_min_tiles = 512;     // DTC_BIG_MIN_TILES: whole 256^2 tiles from this many
  int big_tail = 64;           // DTC_BIG_TAIL: ... or forwards whose last round holds at most this many
  int big_cb3 = 1;             // DTC_BIG_CB3: the 256 x 192 split-K plan
  int r8_mask = 5;             // DTC_GEMM8R: 1 NT bf16, 2 also fp32 outputs, 4 also NN, 0 off
  int r8_ilv = 1;              // DTC_R8_ILV: interleaved gemm8r block order
  int n8_mask = 3;             // DTC_GEMM8N: 1 layout 0, 2 layout 1, 4 also multi-round problems
  int n8_cb = 0;               // DTC_N8_CB: only this gemm8n tile width (3 / 4; 0 = 3 then 4)
  int n8_mink = 1024;          // DTC_N8_MINK: smallest K of a one-round gemm8n problem
  int w8_mode = 1;             // DTC_GEMM_W8: 1 measured winners, 2 every 8-wave config, 4 128x64 fp32 dgrads
  int wg_nfast = 1;            // DTC_WG_NFAST=0: grouped weight gradients M-tiles fastest everywhere
};

// an integer switch: the variable's value, or the default when it is unset
inline int env_int(const char* value, int dflt) { return value ? atoi(value) : dflt; }

inline Knobs knobs_from_env() {
  Knobs k;
  k.dma_fwd64 = env_int(getenv("DTC_GEMM_DMA"), k.dma_fwd64);
  k.wgrad_blocks_128 = env_int(getenv("DTC_WGRAD_BLOCKS"), k.wgrad_blocks_128);
  k.wgrad_blocks_64 = env_int(getenv("DTC_WGRAD_BLOCKS"), k.wgrad_blocks_64);
  k.wide_gm = env_int(getenv("DTC_WIDE_GM"), k.wide_gm);
  k.wgrad_cs256 = env_int(getenv("DTC_WGRAD_CS256"), k.wgrad_cs256);
  k.wgrad256 = env_int(getenv("DTC_WGRAD256"), k.wgrad256);
  k.gemm256 = env_int(getenv("DTC_GEMM256"), k.gemm256);
  k.big_min_tiles = env_int(getenv("DTC_BIG_MIN_TILES"), k.big_min_tiles);
  k.big_tail = env_int(getenv("DTC_BIG_TAIL"), k.big_tail);
  k.big_cb3 = env_int(getenv("DTC_BIG_CB3"), k.big_cb3);
  k.r8_mask = env_int(getenv("DTC_GEMM8R"), k.r8_mask);
  k.r8_ilv = env_int(getenv("DTC_R8_ILV"), k.r8_ilv);
  k.n8_mask = env_int(getenv("DTC_GEMM8N"), k.n8_mask);
  k.n8_cb = env_int(getenv("DTC_N8_CB"), k.n8_cb);
  k.n8_mink = env_int(getenv("DTC_N8_MINK"), k.n8_mink);
  k.w8_mode = env_int(getenv("DTC_GEMM_W8"), k.w8_mode);
  k.wg_nfast = env_int(getenv("DTC_WG_NFAST"), k.wg_nfast);
  return k;
}

// ---- the problem and its plan ----------------------------------------------------------------------------
struct Problem {
  int layout, M, N, K;
  int epi;              // as the caller gave it (EPI_LMHEAD_EVAL plans as EPI_LMHEAD)
  bool f32;             // fp32 output asked for
  bool has_bias, has_colsum;
  bool unit_ab;         // alpha == 1 and beta == 0
  bool eval_ok;         // EPI_LMHEAD_EVAL: its label / part / arg-max buffers are all there
  long ws_bytes;        // split-K workspace the caller holds (LONG_MAX: plan as if it were ample)
};

struct GemmPlan {
  int err = 0;          // the code dtc_gemm returns instead of launching (0: it launches).  The fields below then
                        // say what would have run, as far as the plan got: the queries read them
  int family = FAM_NONE;
  int bm = 0, bn = 0;   // tile
  int bk = 64;
  int split = 1;        // split-K
  int sub = 0, aux = 0; // sub-variant, as in the launch record: BK / stages / CB / CB2, wave grid / n_split
  int epi = 0;          // the instantiated epilogue and output type: what the (layout, epi, fp32) table is asked
  bool f32 = false;     //   for.  Not always the caller's: see the notes in plan_gemm
};

// ---- register-staged tiles (gemm_kernel / gemm_dma_kernel) -----------------------------------------------
// allow_split: 1 = small-grid split (wgrad), 2 = huge-K only (dgrad through the lm_head)
inline GemmPlan reg_plan(int M, int N, int K, int allow_split, const Knobs& k) {
  GemmPlan p;
  p.family = FAM_REG;
  p.bm = p.bn = 128;
  if (K % 64) {  // K a multiple of 32 only (e.g. a TP shard of d_model=768): BK=32, small tiles
    p.bm = p.bn = 64;
    p.bk = 32;
    return p;
  }
  const int nk = K / 64;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (allow_split && K >= 8192 && t128 >= 32) {  // e.g. dH = dlogits . W_lm (K = vocab)
    p.split = (int)std::max(1L, std::min((long)nk / 64, (512 + t128 - 1) / t128));
    return p;
  }
  // weight gradients: 128^2 tiles + split-K (A/B: 5.99 vs 6.05 ms on 64^2 tiles)
  if (allow_split == 1 && t128 < 256) {
    while (t128 * p.split < k.wgrad_blocks_128 && nk / (p.split * 2) >= 8) p.split *= 2;
    return p;
  }
  if (t128 >= 256) return p;
  p.bm = p.bn = 64;
  const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64);
  // weight gradients run on the backward side stream next to the dgrad chain: a grid that
  // fills every CU starves the critical path, so their split-K targets DTC_WGRAD_BLOCKS blocks
  if (allow_split == 1)
    while (t64 * p.split < k.wgrad_blocks_64 && nk / (p.split * 2) >= 4) p.split *= 2;
  return p;
}

// the (layout, epilogue, output) combinations instantiated on the register-staged kernels; the lm_head
// epilogues on 128^2 tiles only (reg_has_tile64)
constexpr bool reg_has(int layout, int epi, bool f32) {
  return layout == 0   ? (f32 ? (epi == EPI_STORE || epi == EPI_RESID)
                              : (epi == EPI_STORE || epi == EPI_GELU || epi == EPI_DGELU || epi == EPI_LMHEAD ||
                                 epi == EPI_LMHEAD_EVAL))
         : layout == 1 ? (epi == EPI_STORE || (epi == EPI_DGELU && !f32))
                       : (layout == 2 && epi == EPI_STORE && f32);
}
constexpr bool reg_has_tile64(int epi) { return epi != EPI_LMHEAD && epi != EPI_LMHEAD_EVAL; }

// ---- 256^2 tiles (gemm8p_kernel) -------------------------------------------------------------------------
// The 256^2 kernel pays on lm_head-sized problems.  Returns the split-K factor (0 = use the
// 128/64 kernels).  layout 0 (fwd): whole tiles; layout 1 (dgrad through the lm_head, K = vocab):
// split so ~256 blocks run (so does layout 0 at K >= 16384: the same dgrad as an NT GEMM on a
// transposed lm_head weight, ~25% faster main loop with both operands K-major); layout 2 (wgrad): no split (a 103 MB fp32 output; extra slab passes
// cost more than the last partial wave of tiles).
inline int big_split(int layout, int M, int N, int K, const Knobs& k) {
  if (!(k.gemm256 & (1 << layout)) || K % 64) return 0;
  if (layout != 0 && N % 8) return 0;              // MN-major B extent (dgrad / wgrad)
  if (layout == 2 && M % 8) return 0;              // MN-major A extent (wgrad)
  const long t = (long)((M + BIG - 1) / BIG) * ((N + BIG - 1) / BIG);
  if (layout == 2) {
    if (t >= 256 && K >= 1024) return 1;
    // DTC_WGRAD256=1 (default; in-step 14.30 -> 14.23 ms): layer weight gradients (K = tokens, a few dozen 256^2 tiles) split-K across
    // ~256 blocks of >= 8 K-steps on this kernel, fp32 slabs summed by the caller's reducer
    // K >= 8192 tokens: at the reference model's 4096 the split pieces are 4-8 K-steps and the grid half
    // empty (whole step 4.65 -> 5.04 ms with it, profiles/r3_ab_ref_regress.log)
    if (!k.wgrad256 || t < 8 || K < 8192) return 0;
    int split = (int)std::max(1L, 256 / t);
    while (split > 1 && (K / 64) / split < 8) --split;
    // fp32 slabs of one problem <= 96 MB (a layer's four weight gradients share the reducer's window)
    while (split > 1 && (long)split * M * N * 4 > (96L << 20)) --split;
    return split > 1 ? split : 0;
  }
  // ordinary K: whole tiles, when there are enough of them, or when the last round of 256^2 tiles is
  // nearly empty anyway (GPT-2 small qkv forward: 288 tiles = 1.125 rounds, 54.7 -> 47.7 us;
  // fc1's 384 = 1.5 rounds stays on the 128^2 kernel: 76 vs 85 us, profiles/r3_gemm_bench_gpt2s*.log)
  if (K < 16384) return (t >= k.big_min_tiles || (layout == 0 && t >= 256 && t % 256 <= k.big_tail)) ? 1 : 0;
  if (t > 256) return 0;                           // dgrad through the vocab (NN, or NT on W^T): split-K
  int split = (int)std::max(1L, 256 / t);
  while (split > 1 && (K / 64) / split < 8) --split;
  return split;
}

constexpr bool big_has(int layout, int epi, bool f32) { return reg_has(layout, epi, f32); }

// The 256^2 plan of a problem big_split took with split-K factor `split`.
// DTC_BIG_CB3 (default on: GPT-2 small lm_head dgrad 553 -> 502 us, step 11.01-11.04 vs 11.04-11.09 ms,
// profiles/r4_ab_big_cb3.log): fp32-store split-K problems whose 256^2 grid leaves CUs idle (96 tiles x split 2
// = 192 blocks) run 256 x 192 tiles when that grid is exactly one block per CU (128 x 2 = 256)
inline GemmPlan big_plan(const Problem& q, int epi, bool f32, int split, int cus, const Knobs& k) {
  GemmPlan p;
  p.family = FAM_BIG;
  p.bm = p.bn = BIG;
  p.sub = 4;
  p.split = split;
  p.epi = epi;
  p.f32 = f32;
  if (split > 1 && (q.ws_bytes < (long)split * q.M * q.N * 4 || q.N % 4)) p.err = 1005;
  const int tiles_m = (q.M + BIG - 1) / BIG, tiles_n = (q.N + BIG - 1) / BIG, tn3 = q.N / 192;
  if (epi == EPI_STORE && f32 && k.big_cb3 && split > 1 && q.N % 192 == 0 && tiles_m * tiles_n * split < cus &&
      tiles_m * tn3 * split == cus) {
    p.bn = 192;
    p.sub = 3;
  }
  return p;
}

// ---- gemm8r plans (layer GEMMs on 256-row tiles of two widths, one launch) ---------------------------
// DTC_GEMM8R: 1 (default) = use the plan for NT problems (forwards, dgrads on transposed weights) with a bf16
// staged epilogue (plain + bias, GELU pair, dGELU) whose 256^2 grid is not whole rounds; 2 = also fp32
// outputs (measured slower: out_proj f32 21 -> 29 us); 4 = also NN problems (dgrads on the row-major weight:
// the fc2 dgrad + dGELU); 0 = off.  HBM-cold, GPT-2 small (profiles/r5_gemm8r.md):
// qkv fwd 44.5 -> 41.6 us, fc1 fwd + GELU 67.3 -> 54.9, fc2 NT dgrad + dGELU 73.7 -> 61.3; step 10.89 -> 10.74 ms
// NN added (default 5): fc2 dgrad + dGELU on the row-major weight 74.3 -> 62.3 us cold, step 10.84 -> 10.74 ms
// (profiles/r5_gemm8r.md), level with the NT form on a transposed copy (DTC_DGRAD_NT_FC2=1: 10.76 ms)
struct R8Plan {
  int n_split = -1, cb2 = 0;
};

inline R8Plan r8_plan(int layout, int M, int N, int K, int epi, bool f32, int cus, const Knobs& k) {
  R8Plan r;
  if (!k.r8_mask || !(layout == 0 || (layout == 1 && (k.r8_mask & 4))) || M % BIG || N % 64 || K % 64 || K < 256 ||
      K > 4096 || N > 16384)
    return r;
  if (!(epi == EPI_STORE || epi == EPI_GELU || epi == EPI_DGELU)) return r;
  if (f32 && (epi != EPI_STORE || !(k.r8_mask & 2))) return r;
  const int tm = M / BIG, q = N / BIG;
  if ((long)tm * q % cus == 0 && q > 0 && N % BIG == 0) return r;  // whole rounds of 256^2 tiles: the 256^2 kernel
  int c1 = q;
  while (c1 > 0 && ((long)tm * c1) % cus) --c1;  // whole rounds of 256^2 tiles
  const int u = (N - BIG * c1) / 64;
  int best = 0;
  long best_cost = 0;
  for (int cb : {4, 2, 1}) {
    if (u % cb) continue;
    const long blocks = (long)tm * (u / cb);
    const long cost = ((blocks + cus - 1) / cus) * cb;  // rounds x tile width
    if (!best || cost < best_cost) {
      best = cb;
      best_cost = cost;
    }
  }
  if (!best) return r;
  r.n_split = BIG * c1;
  r.cb2 = best;
  return r;
}

constexpr bool r8_has(int layout, int epi, bool f32) {
  return layout == 0   ? (epi == EPI_STORE || ((epi == EPI_GELU || epi == EPI_DGELU) && !f32))
         : layout == 1 ? ((epi == EPI_STORE || epi == EPI_DGELU) && !f32)
                       : false;
}

// ---- gemm8n_kernel plans (layer GEMMs, 128 x 64*CB tiles) ----------------------------------------
// DTC_GEMM8N bit mask: 1 = forwards and NT dgrads (layout 0), 2 = NN dgrads (layout 1), 4 = also
// multi-round problems.  A problem takes it when its tile count on 128x192 (CB 3) or 128x256 (CB 4)
// tiles is exactly one round of 256 (the d_model-wide outputs of GPT-2 small / medium at 8192 tokens:
// out_proj / fc2 forwards, qkv / fc1 / out_proj dgrads).  Measured (profiles/r3_gemm8n.md): one round
// wins (fc1 NT dgrad 60.8 -> 44.9 us, fc2 forward 63.5 -> 49.5 us); 3-4 rounds lose to the 128^2 /
// 256^2 kernels (fc1 forward 75.6 -> 85.6 us: each round pays its own prologue fill and epilogue at
// one block per CU), and so does a vocab-sized K (the lm_head dgrad keeps its split-K 256^2 kernel).
// DTC_N8_MINK: smallest K of a one-round problem (default 1024; 768 = also the out_proj forward /
// dgrad, whose plain stores take the overlapped epilogue since the residual add moved to the LayerNorm)
inline int n8_cb(int layout, int M, int N, int K, int epi, const Knobs& k) {
  // K >= 1024: at K = 768 (out_proj forward, 12 K-steps) the one-block-per-CU epilogue (fp32 residual
  // in + out, nothing to hide it under) costs more than the main loop gains (29.2 vs 26.6 us)
  if (layout > 1 || !(k.n8_mask & (1 << layout)) || K % 64 || K < 768 || K > 8192 || M < 128) return 0;
  if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_GELU && epi != EPI_DGELU) return 0;
  const long tm = (M + 127) / 128;
  for (int cb : {3, 4}) {
    if (k.n8_cb && cb != k.n8_cb) continue;
    const int bn = 64 * cb;
    if (N % bn) continue;
    const long t = tm * (N / bn);
    if ((t == 256 && K >= k.n8_mink) || ((k.n8_mask & 4) && t > 256 && t % 256 == 0)) return cb;
  }
  return 0;
}

// the (layout, epilogue, output) combinations the layer GEMMs use
constexpr bool n8_has(int layout, int epi, bool f32) {
  return layout == 0   ? (epi == EPI_STORE || (epi == EPI_RESID && f32) || ((epi == EPI_GELU || epi == EPI_DGELU) && !f32))
         : layout == 1 ? (epi == EPI_STORE || (epi == EPI_DGELU && !f32))
                       : false;
}

// ---- 8-wave DMA plans (gemm_dmaw_kernel) for the layer-GEMM shapes ------------------------------
// Main loop only, L2-hot and back to back (benchmarks/gemm_dma8_micro.hip) the 8-wave configs beat the
// 4-wave kernels on every layer shape (e.g. fc1 fwd 10.9 -> 8.8 us, fc1 dgrad 26 -> 18 us), but in the
// step (rocprofv3, profiles/r2_gemm_w8_instep.md) only two keep a gain once their epilogues and
// in-step operand traffic are counted: the fp32 residual forwards (out_proj, fc2: 128x64 tiles, 16.1
// -> 14.4 us per call) and the bias-free small weight gradient (out_proj: 64x128, split 8, 11.4 ->
// 10.8 us).  The 256x128 bf16 forwards tie (14.4 vs 14.7, 22.9 vs 22.6 us: the all-CU epilogue
// dominates), the dgrads lose (fc1 dgrad 26.5 -> 34-36 us) and unpairing the fc2 / qkv
// dgrad+weight-gradient launches loses (37.9 -> 49.6, 36.1 -> 43.4 us).  Those configs stay
// selectable for experiments (DTC_GEMM_W8=2) but are off in the default plan.
enum { W_NONE = -1, W_256x128 = 0, W_128x64 = 1, W_64x128 = 2, W_128x128 = 3 };

struct WPlan {
  int cfg, split;
};

// The 8-wave config (and split-K) of a problem, or W_NONE.  Layer-sized problems only (the lm_head
// GEMMs keep the 256^2 kernel); weight gradients that fuse their bias column sums (has_colsum) stay
// on the register-staged kernel, which reads dY through registers.
inline WPlan dmaw_plan(int layout, int M, int N, int K, int epi, bool f32, bool has_colsum, const Knobs& k) {
  WPlan w{W_NONE, 1};
  const int mode = k.w8_mode;
  if (!(mode & 7) || K % 64 || M % 8 || N % 8) return w;
  const bool all = (mode & 2) != 0;
  auto tiles = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  if (layout == 0) {
    if (all && !f32 && (epi == EPI_STORE || epi == EPI_GELU) && K <= 1024 && tiles(256, 128) >= 128 &&
        tiles(256, 128) <= 512)
      w.cfg = W_256x128;
    else if ((f32 ? (epi == EPI_RESID || epi == EPI_STORE) : epi == EPI_STORE) && K <= 4096 && tiles(128, 64) >= 192 &&
             tiles(128, 64) <= 512)
      w.cfg = W_128x64;
  } else if (layout == 1) {
    if (all && !f32 && epi == EPI_DGELU && K <= 1024 && tiles(256, 128) >= 128 && tiles(256, 128) <= 512)
      w.cfg = W_256x128;
    else if (all && epi == EPI_STORE && K <= 4096 && tiles(64, 128) >= 192 && tiles(64, 128) <= 512)
      w.cfg = W_64x128;
    else if ((mode & 4) && epi == EPI_STORE && f32 && K <= 4096 && tiles(128, 64) >= 192 && tiles(128, 64) <= 512)
      w.cfg = W_128x64;
  } else if (layout == 2 && epi == EPI_STORE && f32 && !has_colsum && tiles(128, 128) <= 256 &&
             (all || tiles(128, 128) <= 48)) {
    // (<= 48 tiles: also GPT-2's [768 x 768] out_proj weight gradient, 53.4 -> 38.3 us)
    // weight gradient (K = tokens): split-K towards 256 blocks of >= 8 k-steps
    const int nk = K / 64;
    const int cfg = tiles(128, 128) >= 32 ? W_128x128 : W_64x128;
    const long t = cfg == W_128x128 ? tiles(128, 128) : tiles(64, 128);
    int split = 1;
    while (t * split * 2 <= 256 && nk / (split * 2) >= 8) split *= 2;
    w.cfg = cfg;
    w.split = split;
  }
  return w;
}

// the (layout, epilogue, output) combinations that ask for an 8-wave config at all, and, of those, the ones
// instantiated on each config: only what dmaw_plan can return (a disagreement is error 1101)
constexpr bool dmaw_has(int layout, int epi, bool f32) {
  return layout == 0   ? (epi == EPI_STORE || (epi == EPI_GELU && !f32) || (epi == EPI_RESID && f32))
         : layout == 1 ? (epi == EPI_STORE || (epi == EPI_DGELU && !f32))
                       : (layout == 2 && epi == EPI_STORE && f32);
}
constexpr bool dmaw_cfg_has(int cfg, int layout, int epi, bool f32) {
  const bool ak = layout != 2, bkm = layout == 0;
  return !dmaw_has(layout, epi, f32) ? false
         : cfg == W_256x128  ? (!f32 && (epi == EPI_STORE || epi == EPI_GELU || epi == EPI_DGELU) && ak && (bkm || epi == EPI_DGELU))
         : cfg == W_128x64  ? (ak && ((f32 && (epi == EPI_STORE || (bkm && epi == EPI_RESID))) || (bkm && !f32 && epi == EPI_STORE)))
         : cfg == W_64x128  ? (epi == EPI_STORE && ((ak && !bkm) || (!ak && !bkm && f32)))
         : cfg == W_128x128 ? (!ak && !bkm && f32 && epi == EPI_STORE)
                            : false;
}

struct WTile {
  int bm, bn, stages, wgm, wgn;
};
constexpr WTile W_TILES[4] = {{256, 128, 2, 4, 2}, {128, 64, 4, 4, 2}, {64, 128, 4, 2, 4}, {128, 128, 4, 4, 2}};

// ---- the plan ----------------------------------------------------------------------------------------------
// The first family, in this order, that claims the problem and has its (layout, epilogue, output) combination
// instantiated: gemm8r (unless gemm8n claims the shape), gemm8n, the 8-wave DMA kernel, the 256^2 kernel, the
// register-staged kernels (64^2 forward tiles on the LDS-DMA variant).
inline GemmPlan plan_gemm(const Problem& q, int cus, const Knobs& k) {
  const int layout = q.layout, M = q.M, N = q.N, K = q.K;
  const bool eval = q.epi == EPI_LMHEAD_EVAL;
  // the evaluation head plans as the training head (same kernel family, tile and part count)
  const int epi = eval ? (int)EPI_LMHEAD : q.epi;
  const bool f32 = q.f32;
  auto refused = [](int err) {
    GemmPlan p;
    p.err = err;
    return p;
  };
  auto variant = [&](GemmPlan p, int e, bool f) {
    p.epi = e;
    p.f32 = f;
    if (p.family == FAM_REG) p.sub = p.bk;
    return p;
  };
  if (eval && (layout != 0 || f32 || !q.eval_ok)) return refused(1011);

  if (layout <= 1 && !q.has_colsum && q.unit_ab) {  // the layer kernels know no alpha / beta / column sums
    const int cb = n8_cb(layout, M, N, K, epi, k);
    if (!cb) {
      const R8Plan r = r8_plan(layout, M, N, K, epi, f32, cus, k);
      if (r.cb2 && r8_has(layout, epi, f32)) {
        GemmPlan p;
        p.family = FAM_R8;
        p.bm = BIG; p.bn = 64 * r.cb2; p.sub = r.cb2; p.aux = r.n_split;
        return variant(p, epi, f32);
      }
    } else if (n8_has(layout, epi, f32)) {
      GemmPlan p;
      p.family = FAM_N8;
      p.bm = 128; p.bn = 64 * cb; p.sub = cb;
      return variant(p, epi, f32);
    }
  }

  if (layout >= 0 && layout <= 2 && !(layout == 2 && (q.has_bias || big_split(2, M, N, K, k)))) {
    const WPlan w = dmaw_plan(layout, M, N, K, epi, f32, q.has_colsum, k);
    if (w.cfg != W_NONE && dmaw_has(layout, epi, f32)) {
      if (!dmaw_cfg_has(w.cfg, layout, epi, f32)) return refused(1101);  // dmaw_plan and the table disagree
      const WTile t = W_TILES[w.cfg];
      GemmPlan p;
      p.family = FAM_DMAW;
      p.bm = t.bm; p.bn = t.bn; p.split = w.split; p.sub = t.stages; p.aux = t.wgm * 10 + t.wgn;
      if (w.split > 1 && q.ws_bytes < (long)w.split * M * N * 4) p.err = 1005;
      return variant(p, epi, f32);
    }
  }

  // Output types below follow the epilogue where the caller's flag was never looked at: a GELU, dGELU-on-NN or
  // lm_head problem gets the bf16 kernel and a RESID problem the fp32 one whatever c_f32 says.
  if (layout == 0) {
    const int bs = big_split(0, M, N, K, k);
    const bool out32 = epi == EPI_RESID || (epi == EPI_STORE && f32);
    if (!reg_has(0, q.epi, out32) || (epi == EPI_DGELU && f32)) return refused(1003);
    if (bs > 1 && epi == EPI_STORE && f32) {
      // the split-K slabs hold bare accumulators and splitk_reduce knows no bias: refuse it, do not drop it
      if (q.has_bias) return refused(1010);
      return big_plan(q, epi, true, bs, cus, k);
    }
    if (bs == 1) return big_plan(q, q.epi, out32, 1, cus, k);
    GemmPlan p = reg_plan(M, N, K, 0, k);
    if (epi == EPI_LMHEAD) {
      p.bm = p.bn = 128;
      if (p.bk != 64) p.err = 1008;
    }
    if (p.bm == 64 && p.bk == 64 && k.dma_fwd64) {
      p.family = FAM_DMA64;
      p.sub = 4;  // stages
    }
    return variant(p, q.epi, out32);
  }
  if (layout == 1) {
    const int bs = big_split(1, M, N, K, k);  // 0 when N % 8
    const bool out32 = epi == EPI_STORE && f32;
    if (bs > 1 && out32) return big_plan(q, epi, true, bs, cus, k);
    if (bs == 1 && K < 16384 && (epi == EPI_DGELU || epi == EPI_STORE)) return big_plan(q, epi, out32, 1, cus, k);
    GemmPlan p = reg_plan(M, N, K, out32 ? 2 : 0, k);
    if (N % 8) p.err = 1004;
    else if (p.split > 1 && q.ws_bytes < (long)p.split * M * N * 4) p.err = 1005;
    else if (epi != EPI_DGELU && epi != EPI_STORE) p.err = 1003;
    return variant(p, epi, out32);
  }
  if (layout == 2) {
    int err = 0;
    if (M % 8 || N % 8) err = 1004;
    else if (epi != EPI_STORE || !f32 || q.has_bias) err = 1003;
    const int bs = big_split(2, M, N, K, k);
    // gemm8p_kernel sums the bias gradient with its MFMAs (DTC_WGRAD_CS256); the register-staged kernel always can
    if (!err && q.has_colsum && bs && !k.wgrad_cs256) err = 1009;
    GemmPlan p = bs ? big_plan(q, EPI_STORE, true, bs, cus, k) : reg_plan(M, N, K, 1, k);
    if (!bs && p.split > 1 && q.ws_bytes < (long)p.split * M * N * 4) p.err = 1005;
    if (err) p.err = err;
    return variant(p, EPI_STORE, true);
  }
  return refused(1006);
}

}  // namespace gp
