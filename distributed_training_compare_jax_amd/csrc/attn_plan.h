// Which kernels run a bf16 attention call (csrc/attention.hip): two pure host functions, plan_attn_fwd and
// plan_attn_bwd, from the problem, the flags, the CU count and the knobs to an AttnPlan -- the path, the ordered
// launches with their grids and blocks, and the block order.  dtc_attn_fwd / dtc_attn_bwd launch from the plan,
// dtc_attn_plan answers from the same plan, and dtc_attn_last_launch reports what ran.  No HIP header: this file
// compiles with a plain C++ compiler (the few helpers the kernels share carry ATTN_PLAN_HD).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#if defined(__HIPCC__)
#define ATTN_PLAN_HD __host__ __device__
#else
#define ATTN_PLAN_HD
#endif

// The CU-balanced block order, a kernel argument of attn_fwd5 (fw_order below fills it).  It stays in the
// unnamed namespace, where attention.hip's kernels live: the scope of a parameter type is part of a kernel's
// symbol name.
constexpr int FW_ORDER_MAX = 256;
namespace {
struct FwOrder {
  int n;  // 0: heavy-first; else per XCD block k runs query block q[k] of the XCD's (b, h) number j[k]
  unsigned char q[FW_ORDER_MAX], j[FW_ORDER_MAX];
};
}  // namespace

namespace ap {

using ::FwOrder;
using ::FW_ORDER_MAX;

// ---- knobs ---------------------------------------------------------------------------------------------
// Every environment switch of the dispatch, read once per process (attention.hip keeps the one instance).
// docs/KNOBS.md describes them.  DTC_ATTN_XCD_PAIR and DTC_ATTN_STAMPS are compile-time defines of attention.hip.
struct AttnKnobs {
  int resident = 1;    // DTC_ATTN_RESIDENT=0: never the LDS-resident head_dim 32 kernels
  int chunk = 1;       // DTC_ATTN_CHUNK=0: the 256-thread tiled kernels at head_dim 32 / 64
  int fused = 1;       // DTC_ATTN_FUSED=0: the two-round resident backward instead of the fused single round
  int merged = 1;      // DTC_ATTN_MERGED=0: the two-round resident backward as two launches
  int bwd_merged = 1;  // DTC_ATTN_BWD_MERGED=0: head_dim 64 dQ and dK/dV as two launches (BWD_FORCE_MERGED overrides)
};

inline int env_int(const char* value, int dflt) { return value ? atoi(value) : dflt; }

inline AttnKnobs attn_knobs_from_env() {
  AttnKnobs k;
  k.resident = env_int(getenv("DTC_ATTN_RESIDENT"), k.resident);
  k.chunk = env_int(getenv("DTC_ATTN_CHUNK"), k.chunk);
  k.fused = env_int(getenv("DTC_ATTN_FUSED"), k.fused);
  k.merged = env_int(getenv("DTC_ATTN_MERGED"), k.merged);
  k.bwd_merged = env_int(getenv("DTC_ATTN_BWD_MERGED"), k.bwd_merged);
  return k;
}

// ---- flags (A/B switches of one call; ops/attention.py mirrors them as FwdFlags / BwdFlags) --------------
enum FwdFlags {
  FWD_PLAIN_WAVES = 1 << 0,  // resident kernel: plain wave -> query-group order instead of the SIMD-balanced one
  FWD_CHUNK16 = 1 << 2,      // head_dim 64: the 16-row chunk kernel
  FWD_ROUND4 = 1 << 4,       // head_dim 64: the round-4 32-row kernel (attn_fwd32) instead of the round-5 pipeline
  FWD_WPS2 = 1 << 5,         // head_dim 64: the round-5 pipeline at two waves per SIMD (heavy-first, no order)
  FWD_HEAVY_FIRST = 1 << 6,  // head_dim 64: the round-5 pipeline in heavy-first block order, not CU-balanced
};
enum BwdFlags {
  BWD_TWO_ROUND = 1 << 0,     // resident: the two-round kernels instead of the fused single round
  BWD_CHUNK16 = 1 << 2,       // head_dim 64: the 16-row chunk kernels
  BWD_FORCE_MERGED = 1 << 3,  // head_dim 64: the merged dK/dV + dQ launch even with DTC_ATTN_BWD_MERGED=0
};

// ---- paths and kernels ---------------------------------------------------------------------------------
enum Dir { DIR_NONE = 0, DIR_FWD = 1, DIR_BWD = 2 };
enum Path {
  PATH_NONE = 0,
  FWD_RESIDENT,      // attn_fwd_res<32>: K and V of one (b, h) resident in LDS
  FWD_PIPE3,         // attn_fwd5<64, 3>: the round-5 pipeline, three waves per SIMD, takes a block order
  FWD_PIPE2,         // attn_fwd5<64, 2>
  FWD_ROWS32,        // attn_fwd32<64 / 128>: 32 query rows per wave
  FWD_CHUNK,         // attn_fwd_chunk<32 / 64>: 16 query rows per wave
  FWD_TILED,         // attn_fwd<32 / 64>: the 256-thread tiled kernel
  BWD_RES_FUSED,     // attn_bwd_fused<32>: one round
  BWD_RES_SPLIT,     // attn_bwd_dkdv_res<32>, attn_bwd_dq_res<32>
  BWD_RES_MERGED,    // attn_bwd_res<32>: both rounds in one launch
  BWD_ROWS32_128,    // delta, attn_bwd_dkdv32<128>, attn_bwd_dq32<128, true>
  BWD_ROWS32_MERGED, // delta, attn_bwd_merged32<64>
  BWD_ROWS32_SPLIT,  // attn_bwd_dq32<64> (writes delta), attn_bwd_dkdv32<64>
  BWD_CHUNK,         // attn_bwd_dq_chunk (writes delta), attn_bwd_dkdv_chunk, <32 / 64>
  BWD_TILED,         // delta, attn_bwd_dkdv, attn_bwd_dq, <32 / 64>
  // document-masked attention (plan_attn_fwd_doc / plan_attn_bwd_doc): the 32-row family with per-row bounds
  FWD_ROWS32_DOC,        // attn_fwd32_doc<64 / 128>
  BWD_ROWS32_DOC_128,    // delta, attn_bwd_dkdv32_doc<128>, attn_bwd_dq32_doc<128>
  BWD_ROWS32_DOC_MERGED, // delta, attn_bwd_merged32_doc<64>
  PATH_COUNT,
};

// One id per instantiated kernel; KERNEL_NAMES[id] is the launch site's kernel expression without spaces and
// parentheses (tests/attn_plan_dump.hip holds every launch to it).  The 32 / 64 pairs are adjacent: by_hd().
enum Kernel {
  K_NONE = 0,
  K_DELTA_32, K_DELTA_64, K_DELTA_128,
  K_FWD_TILED_32, K_FWD_TILED_64,
  K_FWD_RES_32,
  K_FWD_CHUNK_32, K_FWD_CHUNK_64,
  K_FWD32_64, K_FWD32_128,
  K_FWD5_64_2, K_FWD5_64_3,
  K_BWD_DKDV_TILED_32, K_BWD_DKDV_TILED_64,
  K_BWD_DQ_TILED_32, K_BWD_DQ_TILED_64,
  K_BWD_FUSED_32,
  K_BWD_DKDV_RES_32, K_BWD_DQ_RES_32, K_BWD_RES_32,
  K_BWD_DQ_CHUNK_32, K_BWD_DQ_CHUNK_64,
  K_BWD_DKDV_CHUNK_32, K_BWD_DKDV_CHUNK_64,
  K_BWD_DQ32_64, K_BWD_DQ32_128_DELTA_IN,
  K_BWD_DKDV32_64, K_BWD_DKDV32_128,
  K_BWD_MERGED32_64,
  K_FWD32_DOC_64, K_FWD32_DOC_128,
  K_BWD_DQ32_DOC_128, K_BWD_DKDV32_DOC_128,
  K_BWD_MERGED32_DOC_64,
  K_COUNT,
};
constexpr const char* KERNEL_NAMES[] = {
    "none",
    "attn_delta_kernel<32>", "attn_delta_kernel<64>", "attn_delta_kernel<128>",
    "attn_fwd_kernel<32>", "attn_fwd_kernel<64>",
    "attn_fwd_res_kernel<32>",
    "attn_fwd_chunk_kernel<32>", "attn_fwd_chunk_kernel<64>",
    "attn_fwd32_kernel<64>", "attn_fwd32_kernel<128>",
    "attn_fwd5_kernel<64,2>", "attn_fwd5_kernel<64,3>",
    "attn_bwd_dkdv_kernel<32>", "attn_bwd_dkdv_kernel<64>",
    "attn_bwd_dq_kernel<32>", "attn_bwd_dq_kernel<64>",
    "attn_bwd_fused_kernel<32>",
    "attn_bwd_dkdv_res_kernel<32>", "attn_bwd_dq_res_kernel<32>", "attn_bwd_res_kernel<32>",
    "attn_bwd_dq_chunk_kernel<32>", "attn_bwd_dq_chunk_kernel<64>",
    "attn_bwd_dkdv_chunk_kernel<32>", "attn_bwd_dkdv_chunk_kernel<64>",
    "attn_bwd_dq32_kernel<64>", "attn_bwd_dq32_kernel<128,true>",
    "attn_bwd_dkdv32_kernel<64>", "attn_bwd_dkdv32_kernel<128>",
    "attn_bwd_merged32_kernel<64>",
    "attn_fwd32_doc_kernel<64>", "attn_fwd32_doc_kernel<128>",
    "attn_bwd_dq32_doc_kernel<128>", "attn_bwd_dkdv32_doc_kernel<128>",
    "attn_bwd_merged32_doc_kernel<64>",
};
static_assert(sizeof(KERNEL_NAMES) / sizeof(KERNEL_NAMES[0]) == K_COUNT, "one name per kernel id");

// ---- launch geometry the kernels and the plan share ------------------------------------------------------
constexpr int RES_THREADS = 1024;
constexpr int RES_MAXT = 512;  // 16 waves x 2 blocks x 16 rows
constexpr int FB_THREADS = 1024;
constexpr int CH_THREADS = 1024, CH_QROWS = 256;
constexpr int CHB_THREADS = 512, CHB_KROWS = CHB_THREADS / 4;
constexpr int FW_THREADS = 256, FW_QROWS = 128;
constexpr int TILED_THREADS = 256, TILED_ROWS = 64;
constexpr int RES_KLD = 80;  // AttnLds<32>::KLD (attention.hip asserts it)
constexpr long LDS_MAX = 160 * 1024;

// Q / dO and K / V panel rows of the fused resident backward
ATTN_PLAN_HD constexpr int fb_rows_q(int T) { return (T + 15) / 16 * 16 + 64; }
ATTN_PLAN_HD constexpr int fb_rows_k(int T) { return (T + 63) / 64 * 64; }
constexpr long fb_lds_bytes(int T) {
  return (long)(2 * fb_rows_q(T) + 2 * fb_rows_k(T)) * 32 * 2 + (long)2 * fb_rows_q(T) * 4;
}
// LDS bytes of the resident kernels
constexpr long res_lds_fwd(int T, int HD) { return (long)((T + 63) / 64 * 64) * (RES_KLD + HD + 16) * 2; }
constexpr long res_lds_dkdv(int T, int HD) { return 2 * (long)((T + 63) / 64 * 64 + 64) * (HD + 16) * 2 + (long)((T + 63) / 64 * 64 + 64) * 8; }
constexpr long res_lds_dq(int T, int HD) { return 2 * (long)((T + 63) / 64 * 64) * (HD + 16) * 2; }

// the sequence fits the resident kernels (otherwise the chunk or tiled ones run)
inline bool use_resident(int T, int HD, const AttnKnobs& k) {
  return k.resident && HD == 32 && T % 4 == 0 && T <= RES_MAXT && res_lds_fwd(T, HD) <= LDS_MAX &&
         res_lds_dkdv(T, HD) <= LDS_MAX && res_lds_dq(T, HD) <= LDS_MAX;
}

constexpr long bwd_workspace_bytes(int B, int T, int H) { return (long)B * H * T * 4; }  // delta, fp32 [B, H, T]

// ---- the CU-balanced block order of attn_fwd5<64, 3> -------------------------------------------------------
enum OrderKind { ORDER_NONE = 0, ORDER_HEAVY_FIRST = 1, ORDER_BALANCED = 2 };

// Blocks per XCD of the balanced order, or 0 when the grid of nqb query blocks x nbh (b, h) is not exactly one
// round of 8 equal XCDs at wps blocks per CU (then the kernel runs heavy-first).  cus = 0: the query failed.
inline int fw_order_n(int nqb, int nbh, int wps, int cus) {
  const int C = cus / 8, per_xcd = nbh / 8 * nqb;
  const bool one_round = cus % 8 == 0 && nbh % 8 == 0 && C > 0 && per_xcd == C * wps && per_xcd <= FW_ORDER_MAX &&
                         nqb <= 255 && nbh / 8 <= 255;
  return one_round ? per_xcd : 0;
}

// Longest-processing-time-first per XCD: the query blocks, heaviest first, each to the least-loaded CU with a
// free slot; CU c's s-th block becomes k = s * C + c.
inline FwOrder fw_order(int nqb, int nbh, int wps, int cus) {
  FwOrder ord{};
  ord.n = fw_order_n(nqb, nbh, wps, cus);
  if (!ord.n) return ord;
  const int C = cus / 8;
  std::vector<int> load(C, 0), cnt(C, 0), used(nqb, 0);
  for (int q = nqb - 1; q >= 0; --q)
    for (int i = 0; i < nbh / 8; ++i) {
      int c = -1;
      for (int t = 0; t < C; ++t)
        if (cnt[t] < wps && (c < 0 || load[t] < load[c])) c = t;
      const int k = cnt[c] * C + c;
      ord.q[k] = (unsigned char)q;
      ord.j[k] = (unsigned char)used[q]++;
      load[c] += q + 1;
      ++cnt[c];
    }
  return ord;
}

// ---- the plan ------------------------------------------------------------------------------------------
struct Launch {
  int kernel = K_NONE, grid = 0, block = 0;
  int lds = 0;  // dynamic LDS bytes: set here for the resident kernels, whose size decides the path; the others'
                // come from the kernels' device layout structs and are filled in next to them (attention.hip)
};
constexpr int MAX_LAUNCHES = 3;

struct AttnPlan {
  int err = 0;  // the code the entry point returns instead of launching: 4001 head_dim, 4002 workspace,
                // 4005 head_dim of a document-masked call (ERR_DOC_HEAD_DIM)
  int dir = DIR_NONE, path = PATH_NONE;
  int order = ORDER_NONE;  // the block order asked of attn_fwd5<64, 3>
  int order_n = 0;         // ORDER_BALANCED: blocks per XCD of the order; 0 = not one round, runs heavy-first
  int nlaunch = 0;
  Launch launch[MAX_LAUNCHES];

  void add(int kernel, long grid, int block, long lds = 0) {
    launch[nlaunch++] = Launch{kernel, (int)grid, block, (int)lds};
  }
};

// the record of a plan: dir, path, order, order_n, nlaunch, then kernel, grid, block, lds of each launch slot
constexpr int REC_INTS = 5 + 4 * MAX_LAUNCHES;
inline void to_record(const AttnPlan& p, int out[REC_INTS]) {
  const bool ran = p.err == 0;  // a refused call records nothing
  out[0] = ran ? p.dir : 0; out[1] = ran ? p.path : 0; out[2] = ran ? p.order : 0; out[3] = ran ? p.order_n : 0;
  out[4] = ran ? p.nlaunch : 0;
  for (int i = 0; i < MAX_LAUNCHES; ++i) {
    const Launch l = ran && i < p.nlaunch ? p.launch[i] : Launch{};
    out[5 + 4 * i] = l.kernel; out[6 + 4 * i] = l.grid; out[7 + 4 * i] = l.block; out[8 + 4 * i] = l.lds;
  }
}

constexpr long cdiv(long a, long b) { return (a + b - 1) / b; }
inline int by_hd(int kernel32, int HD) { return kernel32 + (HD == 64); }  // the <64> twin of a <32> kernel id
inline AttnPlan refused(int dir, int err) {
  AttnPlan p;
  p.dir = dir;
  p.err = err;
  return p;
}

// The forward ladder, first match wins.  Its quirks, all kept:
//  - the resident kernel is tried before anything else, so at head_dim 32 with T % 4 == 0 and T <= 512 no flag but
//    FWD_PLAIN_WAVES means anything; without it (T % 4 != 0, longer T, DTC_ATTN_RESIDENT=0) head_dim 32 has one
//    chunk and one tiled kernel and every forward flag is ignored;
//  - head_dim 128 has one kernel and ignores every flag and DTC_ATTN_CHUNK;
//  - at head_dim 64 FWD_CHUNK16 beats FWD_ROUND4 beats FWD_WPS2, and FWD_HEAVY_FIRST only matters to the
//    three-waves pipeline (FWD_WPS2 always runs heavy-first, with an empty order);
//  - DTC_ATTN_CHUNK=0 turns off every head_dim 64 variant at once, whatever the flags say;
//  - an unsupported head_dim is only found out at the bottom: 4001, nothing launched.
inline AttnPlan plan_attn_fwd(int B, int T, int H, int HD, int flags, int cus, const AttnKnobs& k) {
  AttnPlan p;
  p.dir = DIR_FWD;
  const long bh = (long)B * H, g32 = bh * cdiv(T, FW_QROWS);
  if (use_resident(T, HD, k)) {
    p.path = FWD_RESIDENT;
    p.add(K_FWD_RES_32, bh * 2, RES_THREADS, res_lds_fwd(T, HD));
  } else if (HD == 128) {
    p.path = FWD_ROWS32;
    p.add(K_FWD32_128, g32, FW_THREADS);
  } else if (HD == 64 && k.chunk && !(flags & FWD_CHUNK16) && !(flags & FWD_ROUND4)) {
    if (flags & FWD_WPS2) {
      p.path = FWD_PIPE2;
      p.add(K_FWD5_64_2, g32, FW_THREADS);
    } else {
      p.path = FWD_PIPE3;
      p.order = (flags & FWD_HEAVY_FIRST) ? ORDER_HEAVY_FIRST : ORDER_BALANCED;
      if (p.order == ORDER_BALANCED) p.order_n = fw_order_n((int)cdiv(T, FW_QROWS), (int)bh, 3, cus);
      p.add(K_FWD5_64_3, g32, FW_THREADS);
    }
  } else if (HD == 64 && k.chunk && !(flags & FWD_CHUNK16)) {
    p.path = FWD_ROWS32;
    p.add(K_FWD32_64, g32, FW_THREADS);
  } else if (HD != 32 && HD != 64) {
    return refused(DIR_FWD, 4001);
  } else if (k.chunk) {
    p.path = FWD_CHUNK;
    p.add(by_hd(K_FWD_CHUNK_32, HD), bh * cdiv(T, CH_QROWS), CH_THREADS);
  } else {
    p.path = FWD_TILED;
    p.add(by_hd(K_FWD_TILED_32, HD), bh * cdiv(T, TILED_ROWS), TILED_THREADS);
  }
  return p;
}

// The backward ladder, first match wins.  Its quirks, all kept:
//  - the workspace is checked before the head_dim: a short one is 4002 even at an unsupported head_dim (4001);
//  - the resident kernels come first (head_dim 32 only): fused unless BWD_TWO_ROUND, DTC_ATTN_FUSED=0 or its
//    LDS does not fit; then DTC_ATTN_MERGED=0 splits the two rounds into two launches of B*H*2, otherwise one
//    launch of B*H*4 with the larger of the two LDS sizes.  BWD_CHUNK16 and BWD_FORCE_MERGED mean nothing there;
//  - head_dim 128 has one path and ignores every flag and DTC_ATTN_CHUNK;
//  - non-resident head_dim 32 always takes the chunk pair, whatever the flags;
//  - at head_dim 64 BWD_CHUNK16 beats BWD_FORCE_MERGED, which beats DTC_ATTN_BWD_MERGED=0;
//  - the chunk and the split 32-row pairs launch dQ first (it writes delta); the paths with a delta pass
//    launch dK/dV before dQ, except the merged kernel, which is one launch on twice the 32-row grid.
inline AttnPlan plan_attn_bwd(int B, int T, int H, int HD, int flags, long ws_bytes, int cus, const AttnKnobs& k) {
  (void)cus;  // no backward kernel is planned by CU count yet
  if (ws_bytes < bwd_workspace_bytes(B, T, H)) return refused(DIR_BWD, 4002);
  AttnPlan p;
  p.dir = DIR_BWD;
  const long bh = (long)B * H, g32 = bh * cdiv(T, FW_QROWS);
  const long delta_grid = cdiv(bh * T * (HD / 8), 256);
  if (use_resident(T, HD, k)) {
    if (k.fused && !(flags & BWD_TWO_ROUND) && fb_lds_bytes(T) <= LDS_MAX) {
      p.path = BWD_RES_FUSED;
      p.add(K_BWD_FUSED_32, bh * 2, FB_THREADS, fb_lds_bytes(T));
    } else if (!k.merged) {
      p.path = BWD_RES_SPLIT;
      p.add(K_BWD_DKDV_RES_32, bh * 2, RES_THREADS, res_lds_dkdv(T, HD));
      p.add(K_BWD_DQ_RES_32, bh * 2, RES_THREADS, res_lds_dq(T, HD));
    } else {
      p.path = BWD_RES_MERGED;
      p.add(K_BWD_RES_32, bh * 4, RES_THREADS, std::max(res_lds_dkdv(T, HD), res_lds_dq(T, HD)));
    }
  } else if (HD == 128) {
    p.path = BWD_ROWS32_128;
    p.add(K_DELTA_128, delta_grid, 256);
    p.add(K_BWD_DKDV32_128, g32, FW_THREADS);
    p.add(K_BWD_DQ32_128_DELTA_IN, g32, FW_THREADS);
  } else if (HD != 32 && HD != 64) {
    return refused(DIR_BWD, 4001);
  } else if (!k.chunk) {
    p.path = BWD_TILED;
    p.add(by_hd(K_DELTA_32, HD), delta_grid, 256);
    p.add(by_hd(K_BWD_DKDV_TILED_32, HD), bh * cdiv(T, TILED_ROWS), TILED_THREADS);
    p.add(by_hd(K_BWD_DQ_TILED_32, HD), bh * cdiv(T, TILED_ROWS), TILED_THREADS);
  } else if (HD == 32 || (flags & BWD_CHUNK16)) {
    p.path = BWD_CHUNK;
    p.add(by_hd(K_BWD_DQ_CHUNK_32, HD), bh * cdiv(T, CH_QROWS), CH_THREADS);
    p.add(by_hd(K_BWD_DKDV_CHUNK_32, HD), bh * cdiv(T, CHB_KROWS), CHB_THREADS);
  } else if (k.bwd_merged || (flags & BWD_FORCE_MERGED)) {
    p.path = BWD_ROWS32_MERGED;
    p.add(K_DELTA_64, delta_grid, 256);
    p.add(K_BWD_MERGED32_64, 2 * g32, FW_THREADS);
  } else {
    p.path = BWD_ROWS32_SPLIT;
    p.add(K_BWD_DQ32_64, g32, FW_THREADS);
    p.add(K_BWD_DKDV32_64, g32, FW_THREADS);
  }
  return p;
}

// ---- document-masked attention ----------------------------------------------------------------------------
// Causal attention that stops at document boundaries (doc_start / doc_end per row, csrc/elementwise.hip
// dtc_doc_bounds) runs the doc instantiations of the 32-row family at head_dim 64 and 128, whatever the flags and
// the knobs say: one forward kernel; backward as the unmasked twin's structure (head_dim 64: delta pass + the merged
// dK/dV + dQ launch, head_dim 128: delta, dK/dV, dQ).  Block order heavy-first by query / key block, as the twins.
// Any other head_dim (32 included) is refused with ERR_DOC_HEAD_DIM before the workspace is looked at.
constexpr int ERR_DOC_HEAD_DIM = 4005;

inline AttnPlan plan_attn_fwd_doc(int B, int T, int H, int HD, int flags, int cus, const AttnKnobs& k) {
  (void)flags; (void)cus; (void)k;
  if (HD != 64 && HD != 128) return refused(DIR_FWD, ERR_DOC_HEAD_DIM);
  AttnPlan p;
  p.dir = DIR_FWD;
  p.path = FWD_ROWS32_DOC;
  p.add(HD == 128 ? K_FWD32_DOC_128 : K_FWD32_DOC_64, (long)B * H * cdiv(T, FW_QROWS), FW_THREADS);
  return p;
}

inline AttnPlan plan_attn_bwd_doc(int B, int T, int H, int HD, int flags, long ws_bytes, int cus, const AttnKnobs& k) {
  (void)flags; (void)cus; (void)k;
  if (HD != 64 && HD != 128) return refused(DIR_BWD, ERR_DOC_HEAD_DIM);
  if (ws_bytes < bwd_workspace_bytes(B, T, H)) return refused(DIR_BWD, 4002);
  AttnPlan p;
  p.dir = DIR_BWD;
  const long bh = (long)B * H, g32 = bh * cdiv(T, FW_QROWS);
  const long delta_grid = cdiv(bh * T * (HD / 8), 256);
  if (HD == 128) {
    p.path = BWD_ROWS32_DOC_128;
    p.add(K_DELTA_128, delta_grid, 256);
    p.add(K_BWD_DKDV32_DOC_128, g32, FW_THREADS);
    p.add(K_BWD_DQ32_DOC_128, g32, FW_THREADS);
  } else {
    p.path = BWD_ROWS32_DOC_MERGED;
    p.add(K_DELTA_64, delta_grid, 256);
    p.add(K_BWD_MERGED32_DOC_64, 2 * g32, FW_THREADS);
  }
  return p;
}

}  // namespace ap
