// The document-masked plans of csrc/attn_plan.h (plan_attn_fwd_doc / plan_attn_bwd_doc) over a sweep of
// (B, T, H, HD, flags, knobs, CUs), and what adding them must not have changed.  Plain C++: includes only
// attn_plan.h.  tests/test_attn_doc_cpu.py builds it twice, once with -fsanitize=address,undefined.
//   - head_dim 64 / 128: the doc kernels of the 32-row family on the 32-row grids, whatever the flags, the knobs
//     and the CU count say: one forward launch; backward = delta pass + the merged launch on twice the grid
//     (head_dim 64) or delta, dK/dV, dQ (head_dim 128); a short workspace is 4002;
//   - any other head_dim (32 included) is refused with ERR_DOC_HEAD_DIM = 4005, nothing planned, an all-zero
//     record, even with a short workspace;
//   - the doc paths and kernel ids are appended: every id that existed keeps its number.  The doc plans are
//     functions of their own, so plan_attn_fwd / plan_attn_bwd keep the one call form they had and there is no
//     second form to compare them with field by field: what is checked here is that they never name a doc path
//     or kernel; that every unmasked problem still plans what it planned is tests/test_attn_plan_cpu.py's
//     comparison with the parent's listing.
#include "attn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

static_assert(ap::BWD_TILED == 14 && ap::FWD_ROWS32_DOC == 15 && ap::BWD_ROWS32_DOC_128 == 16 &&
                  ap::BWD_ROWS32_DOC_MERGED == 17 && ap::PATH_COUNT == 18, "doc paths are appended");
static_assert(ap::K_BWD_MERGED32_64 == 29 && ap::K_FWD32_DOC_64 == 30 && ap::K_FWD32_DOC_128 == 31 &&
                  ap::K_BWD_DQ32_DOC_128 == 32 && ap::K_BWD_DKDV32_DOC_128 == 33 && ap::K_BWD_MERGED32_DOC_64 == 34 &&
                  ap::K_COUNT == 35, "doc kernel ids are appended");
static_assert(ap::ERR_DOC_HEAD_DIM == 4005, "next to 4001 / 4002 (4003 / 4004 belong to attention.hip)");

[[noreturn]] void fail(const char* what, int B, int T, int H, int HD, int flags) {
  printf("FAIL %s: B %d T %d H %d HD %d flags %d\n", what, B, T, H, HD, flags);
  exit(1);
}

bool is(const ap::Launch& l, int kernel, long grid, int block) {
  return l.kernel == kernel && l.grid == grid && l.block == block && l.lds == 0;
}

}  // namespace

int main() {
  if (strcmp(ap::KERNEL_NAMES[ap::K_FWD32_DOC_64], "attn_fwd32_doc_kernel<64>") ||
      strcmp(ap::KERNEL_NAMES[ap::K_FWD32_DOC_128], "attn_fwd32_doc_kernel<128>") ||
      strcmp(ap::KERNEL_NAMES[ap::K_BWD_DQ32_DOC_128], "attn_bwd_dq32_doc_kernel<128>") ||
      strcmp(ap::KERNEL_NAMES[ap::K_BWD_DKDV32_DOC_128], "attn_bwd_dkdv32_doc_kernel<128>") ||
      strcmp(ap::KERNEL_NAMES[ap::K_BWD_MERGED32_DOC_64], "attn_bwd_merged32_doc_kernel<64>") ||
      strcmp(ap::KERNEL_NAMES[ap::K_BWD_MERGED32_64], "attn_bwd_merged32_kernel<64>"))
    fail("kernel names", 0, 0, 0, 0, 0);
  long plans = 0;
  for (int knobs = 0; knobs < 32; ++knobs) {
    ap::AttnKnobs k;
    k.resident = knobs & 1; k.chunk = (knobs >> 1) & 1; k.fused = (knobs >> 2) & 1; k.merged = (knobs >> 3) & 1;
    k.bwd_merged = (knobs >> 4) & 1;
    for (int HD : {32, 64, 128, 48, 96, 256})
      for (int T : {1, 63, 128, 129, 777, 2048})
        for (int B : {1, 8})
          for (int H : {1, 12})
            for (int cus : {0, 64, 256, 304})
              for (int flags = 0; flags < 128; ++flags) {
                const long need = ap::bwd_workspace_bytes(B, T, H), g32 = (long)B * H * ((T + 127) / 128);
                const bool short_ws = flags >> 6 & 1;
                const ap::AttnPlan f = ap::plan_attn_fwd_doc(B, T, H, HD, flags, cus, k);
                const ap::AttnPlan b = ap::plan_attn_bwd_doc(B, T, H, HD, flags & 15, need - short_ws, cus, k);
                int rec[ap::REC_INTS];
                if (HD != 64 && HD != 128) {
                  for (const ap::AttnPlan& p : {f, b}) {
                    if (p.err != 4005 || p.nlaunch != 0 || p.path != ap::PATH_NONE) fail("refusal", B, T, H, HD, flags);
                    ap::to_record(p, rec);
                    for (int v : rec)
                      if (v) fail("a refused plan leaves a record", B, T, H, HD, flags);
                  }
                } else {
                  if (f.err || f.dir != ap::DIR_FWD || f.path != ap::FWD_ROWS32_DOC || f.nlaunch != 1 || f.order ||
                      f.order_n || !is(f.launch[0], HD == 64 ? ap::K_FWD32_DOC_64 : ap::K_FWD32_DOC_128, g32, 256))
                    fail("forward doc plan", B, T, H, HD, flags);
                  const long dg = ((long)B * H * T * (HD / 8) + 255) / 256;
                  if (short_ws) {
                    if (b.err != 4002 || b.nlaunch) fail("short workspace", B, T, H, HD, flags);
                  } else if (HD == 64) {
                    if (b.err || b.dir != ap::DIR_BWD || b.path != ap::BWD_ROWS32_DOC_MERGED || b.nlaunch != 2 ||
                        !is(b.launch[0], ap::K_DELTA_64, dg, 256) ||
                        !is(b.launch[1], ap::K_BWD_MERGED32_DOC_64, 2 * g32, 256))
                      fail("backward doc plan, head_dim 64", B, T, H, HD, flags);
                  } else {
                    if (b.err || b.dir != ap::DIR_BWD || b.path != ap::BWD_ROWS32_DOC_128 || b.nlaunch != 3 ||
                        !is(b.launch[0], ap::K_DELTA_128, dg, 256) ||
                        !is(b.launch[1], ap::K_BWD_DKDV32_DOC_128, g32, 256) ||
                        !is(b.launch[2], ap::K_BWD_DQ32_DOC_128, g32, 256))
                      fail("backward doc plan, head_dim 128", B, T, H, HD, flags);
                  }
                  ap::to_record(f, rec);
                  if (rec[0] != ap::DIR_FWD || rec[1] != ap::FWD_ROWS32_DOC || rec[4] != 1 || rec[5] != f.launch[0].kernel)
                    fail("forward doc record", B, T, H, HD, flags);
                }
                // the old call form: no doc path, no doc kernel
                const ap::AttnPlan f0 = ap::plan_attn_fwd(B, T, H, HD, flags, cus, k);
                const ap::AttnPlan b0 = ap::plan_attn_bwd(B, T, H, HD, flags & 15, need - short_ws, cus, k);
                for (const ap::AttnPlan& p : {f0, b0}) {
                  if (p.path >= ap::FWD_ROWS32_DOC) fail("a doc path from the unmasked plan", B, T, H, HD, flags);
                  for (int i = 0; i < ap::MAX_LAUNCHES; ++i)
                    if (p.launch[i].kernel >= ap::K_FWD32_DOC_64) fail("a doc kernel from the unmasked plan", B, T, H, HD, flags);
                }
                plans += 4;
              }
  }
  printf("ok: %ld plans\n", plans);
  return 0;
}
