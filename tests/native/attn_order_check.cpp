// Properties of the CU-balanced block order (csrc/attn_plan.h fw_order), checked over every grid that meets its
// one-round precondition with up to FW_ORDER_MAX blocks per XCD, and a sweep of the two plan functions.  Plain
// C++: includes only attn_plan.h.  tests/test_attn_plan_cpu.py builds it twice, once with
// -fsanitize=address,undefined: fw_order indexes fixed arrays of FW_ORDER_MAX by a computed k.
//
// For every (nqb, nbh, wps, cus) with n > 0:
//   - k -> (q[k], j[k]) is a bijection from [0, n) onto nqb x nbh / 8;
//   - CU c of an XCD runs blocks c, c + C, c + 2C, ...: exactly wps of them;
//   - no CU's load (sum of q + 1, the function's own weight) exceeds the lightest CU's by more than nqb, the
//     heaviest single block.  This is the greedy assignment's own bound: a block only ever goes to the least-
//     loaded CU with a free slot, heaviest blocks first, so while all CUs have free slots the spread stays within
//     the last block placed; slots run out on the heavier CUs first, and the rest fill with lighter blocks.
// Where a precondition fails (CUs not a multiple of 8 or 0, (b, h) not a multiple of 8, blocks != CUs x wps, more
// than FW_ORDER_MAX blocks per XCD), n == 0.
#include "attn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

long g_checked = 0;

[[noreturn]] void fail(const char* what, int nqb, int nbh, int wps, int cus) {
  printf("FAIL %s: nqb %d nbh %d wps %d cus %d\n", what, nqb, nbh, wps, cus);
  exit(1);
}

void check_order(int nqb, int nbh, int wps, int cus) {
  const ap::FwOrder o = ap::fw_order(nqb, nbh, wps, cus);
  const int C = cus / 8, per_xcd = nbh / 8 * nqb;
  const bool one_round = cus > 0 && cus % 8 == 0 && nbh % 8 == 0 && per_xcd == C * wps && per_xcd <= ap::FW_ORDER_MAX;
  if (o.n != ap::fw_order_n(nqb, nbh, wps, cus)) fail("fw_order_n disagrees with fw_order", nqb, nbh, wps, cus);
  if (!one_round) {
    if (o.n != 0) fail("an order outside the one-round precondition", nqb, nbh, wps, cus);
    return;
  }
  if (o.n != per_xcd) fail("n is not the blocks per XCD", nqb, nbh, wps, cus);
  std::vector<int> hit(nqb * (nbh / 8), 0), load(C, 0), cnt(C, 0);
  for (int k = 0; k < o.n; ++k) {
    if (o.q[k] >= nqb || o.j[k] >= nbh / 8) fail("(q, j) out of range", nqb, nbh, wps, cus);
    if (hit[o.q[k] * (nbh / 8) + o.j[k]]++) fail("a (q, j) twice", nqb, nbh, wps, cus);
    load[k % C] += o.q[k] + 1;
    ++cnt[k % C];
  }
  int lo = load[0], hi = load[0];
  for (int c = 0; c < C; ++c) {
    if (cnt[c] != wps) fail("a CU without exactly wps blocks", nqb, nbh, wps, cus);
    lo = std::min(lo, load[c]);
    hi = std::max(hi, load[c]);
  }
  if (hi - lo > nqb) fail("CU loads further apart than the heaviest block", nqb, nbh, wps, cus);
  ++g_checked;
}

}  // namespace

int main() {
  // every one-round grid, and its neighbours on each side of every precondition
  for (int wps = 1; wps <= 4; ++wps)
    for (int nqb = 1; nqb <= 64; ++nqb)
      for (int j = 1; j <= 64; ++j) {
        if (nqb * j % wps) continue;
        const int C = nqb * j / wps, nbh = 8 * j, cus = 8 * C;
        check_order(nqb, nbh, wps, cus);  // n > 0 up to FW_ORDER_MAX blocks per XCD, 0 beyond
        for (int d : {-8, -1, 1, 8}) check_order(nqb, nbh, wps, cus + d);
        for (int d : {-1, 1, 4}) check_order(nqb, nbh + d, wps, cus);
        check_order(nqb + 1, nbh, wps, cus);
        check_order(nqb, nbh, wps + 1, cus);
        check_order(nqb, nbh, wps, 0);
      }
  // the shapes the GPU tests and the benchmark balance: GPT-2 small at 256 CUs, three blocks per CU
  if (ap::fw_order(8, 96, 3, 256).n != 96) fail("GPT-2 small", 8, 96, 3, 256);
  if (ap::fw_order(8, 96, 3, 304).n != 0) fail("GPT-2 small at 304 CUs", 8, 96, 3, 304);

  // the plan functions over a grid of problems, flags and knob settings: launch counts and records in range
  long plans = 0;
  for (int knobs = 0; knobs < 32; ++knobs) {
    ap::AttnKnobs k;
    k.resident = knobs & 1; k.chunk = (knobs >> 1) & 1; k.fused = (knobs >> 2) & 1; k.merged = (knobs >> 3) & 1;
    k.bwd_merged = (knobs >> 4) & 1;
    for (int HD : {32, 64, 128, 48, 96})
      for (int T : {1, 4, 63, 64, 200, 203, 512, 516, 777, 1024, 4096})
        for (int B : {1, 8})
          for (int H : {1, 3, 12, 16})
            for (int cus : {0, 64, 256, 304})
              for (int flags = 0; flags < 128; ++flags) {
                int rec[ap::REC_INTS];
                const ap::AttnPlan f = ap::plan_attn_fwd(B, T, H, HD, flags, cus, k);
                ap::to_record(f, rec);
                const long need = ap::bwd_workspace_bytes(B, T, H);
                const ap::AttnPlan b = ap::plan_attn_bwd(B, T, H, HD, flags & 15, need - (flags >> 6 & 1), cus, k);
                ap::to_record(b, rec);
                for (const ap::AttnPlan& p : {f, b}) {
                  const bool ok = p.err ? p.nlaunch == 0 : p.nlaunch >= 1 && p.nlaunch <= ap::MAX_LAUNCHES;
                  if (!ok) fail("launch count", T, B * H, HD, flags);
                  for (int i = 0; i < p.nlaunch; ++i)
                    if (p.launch[i].kernel <= 0 || p.launch[i].kernel >= ap::K_COUNT || p.launch[i].grid <= 0)
                      fail("launch", T, B * H, HD, flags);
                }
                plans += 2;
              }
  }
  printf("ok: %ld orders, %ld plans\n", g_checked, plans);
  return 0;
}
