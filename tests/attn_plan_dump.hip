// Host-only dump of the bf16 attention dispatch (csrc/attention.hip): for every row of a case table, the
// return code of dtc_attn_fwd / dtc_attn_bwd and, per launch, the kernel, grid, block, dynamic LDS bytes and
// block order.  No kernel runs and no GPU is needed: the launch macro is replaced by a call that writes down
// the kernel expression and the launch geometry, and the device query answers a CU count chosen on the
// command line.  tests/test_attn_plan_cpu.py builds it with
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -I <csrc> tests/attn_plan_dump.hip
// and compares its output with tests/golden/attn_plan_parent.txt.
//
//   attn_plan_dump [brief|digest|full] [CUs]      (CUs: default 256, the MI355X's; 0 = the query fails)
// `brief` (the test's run with default knobs) lists the shapes of the GPU tests and folds the rest into one
// digest per section; `digest` (its knob and CU-count runs) prints only the digests; `full` prints every row.
// A shape prints one line per distinct outcome over its flag values.
//
// The text comes from dtc_attn_last_launch.  Every row also checks (exit 3) that the record is what the
// launch sites did: as many launches, each with the kernel expression the record's kernel id is named after
// (`HD` inside a templated helper stands for the row's head_dim), the same grid, block and LDS bytes, an LDS
// opt-in of that size before every launch with dynamic LDS, and the block order fw_order gives for the
// record's n.  -DPLAN_CHECK: every row also asks dtc_attn_plan and exits 3 unless it returns exactly that
// return code and record.
//
// -DATTN_PLAN_PARENT is how the golden file was recorded, against the attention.hip of the commit before
// the plan existed (no record, no query: the text comes from the launch macro alone).  That build takes an
// ordinary `hipcc --offload-arch=gfx950` compile, because the old allow_lds took kernels as arguments.
#include "common.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace harness {

typedef unsigned long long u64;

struct Digest {
  u64 h = 1469598103934665603ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  void add(const std::string& s) { add(s.data(), s.size()); }
};

struct Seen {
  std::string expr;  // the kernel expression at the launch site, spaces and parentheses stripped
  long grid, block, lds;
  bool has_order = false;
  int n = 0;
  u64 order = 0;  // digest of q[0..n) and j[0..n)
  std::vector<unsigned char> q, j;
};
std::vector<Seen> g_seen;
struct Allowed {
  std::string expr;
  long bytes;
};
std::vector<Allowed> g_allowed;
int g_cus = 256;

std::string strip(const char* s) {
  std::string r;
  for (; *s; ++s)
    if (*s != ' ' && *s != '(' && *s != ')') r += *s;
  return r;
}

// an argument with q[], j[] and n is the block order (FwOrder); anything else is not looked at
template <typename T>
auto note_arg(Seen& s, const T& v, int) -> decltype(v.q[0], v.j[0], v.n, void()) {
  s.has_order = true;
  s.n = v.n;
  s.q.assign(v.q, v.q + v.n);
  s.j.assign(v.j, v.j + v.n);
  Digest d;
  d.add(v.q, (size_t)v.n);
  d.add(v.j, (size_t)v.n);
  s.order = d.h;
}
template <typename T>
void note_arg(Seen&, const T&, long) {}

template <typename... A>
void seen(const char* expr, unsigned grid, unsigned block, long lds, const A&... args) {
  Seen s;
  s.expr = strip(expr);
  s.grid = grid; s.block = block; s.lds = lds;
  (note_arg(s, args, 0), ...);
  g_seen.push_back(s);
}
inline void allowed(const char* expr, long bytes) { g_allowed.push_back({strip(expr), bytes}); }

inline hipError_t get_device(int* dev) {
  *dev = 0;
  return g_cus > 0 ? hipSuccess : hipErrorNoDevice;
}
inline hipError_t get_cus(int* v) {
  *v = g_cus;
  return hipSuccess;
}

}  // namespace harness

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, st, ...) harness::seen(#k, (g).x, (b).x, (long)(l), __VA_ARGS__)
#undef DTC_CHECK_LAUNCH
#define DTC_CHECK_LAUNCH() ((void)0)
#define hipGetDevice(p) harness::get_device(p)
#define hipDeviceGetAttribute(p, attr, dev) harness::get_cus(p)
#ifdef ATTN_PLAN_PARENT
#define hipFuncSetAttribute(...) hipSuccess
#else
#define ATTN_ALLOW_LDS(kernel, bytes) harness::allowed(#kernel, (long)(bytes))
#endif
#include "attention.hip"

namespace {

using namespace harness;

bf16* const PTR = (bf16*)0x10000;  // never dereferenced: nothing launches
float* const FPTR = (float*)0x10000;
const long AMPLE = 1L << 42;

int g_min_level = 1;  // full 0, brief 1, digest 2
Digest g_folded;
long g_nfolded = 0;

void emit(int level, const std::string& line) {
  if (level >= g_min_level) {
    puts(line.c_str());
  } else {
    g_folded.add(line);
    ++g_nfolded;
  }
}
void end_section(const char* name) {
  printf("# %s: %ld more lines, digest %016llx\n", name, g_nfolded, g_folded.h);
  g_folded = Digest();
  g_nfolded = 0;
}

std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

[[noreturn]] void fail(const std::string& row, const std::string& why) {
  printf("MISMATCH %s\n  %s\n", row.c_str(), why.c_str());
  exit(3);
}

// `HD` in an expression from inside a templated helper is the row's head_dim
std::string with_hd(std::string expr, int HD) {
  for (size_t p; (p = expr.find("HD")) != std::string::npos;) expr.replace(p, 2, std::to_string(HD));
  return expr;
}

std::string show_launch(const std::string& name, long grid, long block, long lds, const Seen& s) {
  const std::string ord = s.has_order ? fmt("n%d:%016llx", s.n, s.order) : std::string("-");
  return fmt(" | %s %ld %ld %ld %s", name.c_str(), grid, block, lds, ord.c_str());
}

// One call: "rc R | kernel grid block lds order | ...".  bwd: 0 forward, 1 backward.
std::string run(int bwd, int B, int T, int H, int HD, int flags, long ws_bytes) {
  const std::string row = fmt("%s %d %d %d %d flags %d ws %ld", bwd ? "B" : "F", B, T, H, HD, flags, ws_bytes);
  g_seen.clear();
  g_allowed.clear();
#ifndef ATTN_PLAN_PARENT
  g_attn_last = ap::AttnPlan{};  // an entry point that refuses leaves the record alone: start from "none"
#endif
  const int rc = bwd ? dtc_attn_bwd(PTR, PTR, FPTR, PTR, PTR, flags, B, T, H, HD, 0.125f, FPTR, ws_bytes, nullptr)
                     : dtc_attn_fwd(PTR, PTR, FPTR, B, T, H, HD, flags, 0.125f, nullptr);
  std::string out = fmt("rc %d", rc);
#ifdef ATTN_PLAN_PARENT
  for (const Seen& s : g_seen) out += show_launch(with_hd(s.expr, HD), s.grid, s.block, s.lds, s);
#else
  int rec[ap::REC_INTS];
  dtc_attn_last_launch(rec);
  const int nl = rec[4];
  if (rc ? (nl != 0 || rec[0] != 0 || !g_seen.empty()) : (rec[0] != (bwd ? ap::DIR_BWD : ap::DIR_FWD)))
    fail(row, fmt("rc %d with direction %d, %d launches recorded, %zu seen", rc, rec[0], nl, g_seen.size()));
  if ((size_t)nl != g_seen.size()) fail(row, fmt("%d launches recorded, %zu seen", nl, g_seen.size()));
  for (int i = 0; i < nl; ++i) {
    const int* l = rec + 5 + 4 * i;
    const Seen& s = g_seen[i];
    if (l[0] <= 0 || l[0] >= ap::K_COUNT) fail(row, fmt("launch %d: kernel id %d", i, l[0]));
    const std::string name = ap::KERNEL_NAMES[l[0]];
    if (name != with_hd(s.expr, HD) || l[1] != s.grid || l[2] != s.block || l[3] != s.lds)
      fail(row, fmt("launch %d: recorded %s %d %d %d, launched %s %ld %ld %ld", i, name.c_str(), l[1], l[2], l[3],
                    s.expr.c_str(), s.grid, s.block, s.lds));
    bool opted = s.lds == 0;
    for (const Allowed& a : g_allowed) opted = opted || (a.expr == s.expr && a.bytes == s.lds);
    if (!opted) fail(row, fmt("launch %d: %s takes %ld bytes of LDS without the opt-in", i, s.expr.c_str(), s.lds));
    if (s.has_order) {
      // the order travels with the one forward kernel that takes it; its n is the record's
      const int want_n = rec[2] == ap::ORDER_BALANCED ? rec[3] : 0;
      if (s.n != want_n || (rec[2] != ap::ORDER_BALANCED && rec[3] != 0))
        fail(row, fmt("order kind %d n %d recorded, n %d launched", rec[2], rec[3], s.n));
      if (s.n > 0) {
        const ap::FwOrder o = ap::fw_order((T + 127) / 128, B * H, 3, g_cus);
        if (o.n != s.n || memcmp(o.q, s.q.data(), s.n) || memcmp(o.j, s.j.data(), s.n))
          fail(row, "the launched order is not fw_order's");
      }
    }
    out += show_launch(name, l[1], l[2], l[3], s);
  }
  if (nl && !g_seen.back().has_order && (rec[2] == ap::ORDER_BALANCED || rec[3] != 0))
    fail(row, fmt("order kind %d n %d recorded on a kernel that takes none", rec[2], rec[3]));
#ifdef PLAN_CHECK
  int plan[ap::REC_INTS];
  const int prc = dtc_attn_plan(bwd ? ap::DIR_BWD : ap::DIR_FWD, B, T, H, HD, flags, ws_bytes, plan);
  if (prc != rc || memcmp(plan, rec, sizeof rec)) {
    std::string a, b;
    for (int i = 0; i < ap::REC_INTS; ++i) a += fmt(" %d", rec[i]), b += fmt(" %d", plan[i]);
    fail(row, fmt("launched rc %d rec%s\n  planned  rc %d rec%s", rc, a.c_str(), prc, b.c_str()));
  }
  if (g_seen.size() != (size_t)nl) fail(row, "dtc_attn_plan launched something");
#endif
#endif
  return out;
}

long ws_need(int B, int T, int H, int HD) { return dtc_attn_bwd_workspace_bytes(B, T, H, HD); }

// one shape under every forward flag value 0..127 and every backward value 0..15
void dump_shape(int level, int B, int T, int H, int HD) {
  for (int bwd = 0; bwd < 2; ++bwd) {
    // one line per distinct outcome, in order of its lowest flag value: that value, how many values share the
    // outcome, and which (bit f of the 128-bit hex mask = flag value f)
    struct Group {
      std::string outcome;
      int first, count;
      u64 mask[2];
    };
    std::vector<Group> groups;
    for (int f = 0; f < (bwd ? 16 : 128); ++f) {
      const std::string o = run(bwd, B, T, H, HD, f, AMPLE);
      size_t g = 0;
      while (g < groups.size() && groups[g].outcome != o) ++g;
      if (g == groups.size()) groups.push_back({o, f, 0, {0, 0}});
      ++groups[g].count;
      groups[g].mask[f / 64] |= 1ull << (f % 64);
    }
    for (const Group& g : groups)
      emit(level, fmt("%s %d %d %d %d flags %d x%d %016llx%016llx %s", bwd ? "B" : "F", B, T, H, HD, g.first, g.count,
                      g.mask[1], g.mask[0], g.outcome.c_str()));
  }
}

void test_shapes() {
  // every bf16 attention shape of tests/*_gpu.py (the hd128 and fp32-floor files' shapes included)
  const int shapes[][4] = {
      {2, 512, 4, 32}, {1, 256, 2, 64}, {2, 128, 3, 32}, {2, 200, 3, 32}, {1, 520, 2, 32}, {1, 1024, 2, 64},
      {1, 1000, 2, 64}, {1, 700, 3, 32}, {2, 1024, 3, 64}, {1, 777, 2, 64}, {8, 1024, 12, 64}, {1, 200, 3, 32},
      {2, 64, 2, 32}, {1, 512, 2, 32}, {1, 508, 3, 32}, {1, 1024, 2, 32}, {1, 1000, 2, 32}, {1, 203, 3, 32},
      {1, 777, 3, 64}, {1, 72, 1, 128}, {2, 200, 2, 128}, {1, 777, 3, 128}, {1, 1024, 2, 128}, {1, 200, 2, 128},
      {1, 777, 2, 128}, {1, 256, 2, 128}, {1, 64, 2, 64}, {2, 192, 2, 64}, {1, 64, 2, 96},
  };
  for (const auto& s : shapes) dump_shape(1, s[0], s[1], s[2], s[3]);
  // a workspace one byte short, and exactly enough
  for (int HD : {32, 64, 128, 96}) {
    const long need = ws_need(2, 200, 3, HD);
    emit(1, fmt("B 2 200 3 %d short ws %s", HD, run(1, 2, 200, 3, HD, 0, need - 1).c_str()));
    emit(1, fmt("B 2 200 3 %d exact ws %s", HD, run(1, 2, 200, 3, HD, 0, need).c_str()));
  }
  end_section("test shapes");
}

void grid() {
  const int Ts[] = {4, 63, 64, 128, 200, 203, 256, 508, 512, 516, 520, 700, 777, 1000, 1024, 2048, 4096};
  const int BH[][2] = {{1, 2}, {1, 3}, {2, 4}, {8, 12}, {4, 16}, {1, 8}};
  const int HDs[] = {32, 64, 128, 48, 96};
  for (int HD : HDs)
    for (int T : Ts)
      for (const auto& bh : BH) dump_shape(0, bh[0], T, bh[1], HD);
  end_section("grid");
}

u64 g_rng = 0x9E3779B97F4A7C15ull;
u64 rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
int pick(int n) { return (int)(rnd() % (u64)n); }

void sweep() {
  Digest d;
  const int HDs[] = {32, 64, 128, 32, 64, 128, 48, 96, 16, 256};
  for (int i = 1; i <= 6000; ++i) {
    const int HD = HDs[pick(10)];
    // grids around one round of 256 / 304 / 64 CUs at 3 blocks each, and anything
    const int B = pick(3) ? 1 + pick(16) : 8, H = pick(3) ? 1 + pick(24) : 4 * (1 + pick(6));
    int T;
    switch (pick(6)) {
      case 0: T = 1 + pick(640); break;
      case 1: T = 4 * (1 + pick(160)); break;
      case 2: T = 128 * (1 + pick(32)); break;
      case 3: T = 1024 + pick(3) - 1; break;
      default: T = 1 + pick(4096); break;
    }
    const int bwd = pick(2), flags = pick(bwd ? 16 : 128);
    const long need = ws_need(B, T, H, HD);
    const long ws = bwd && pick(8) == 0 ? need - 1 - pick(64) : pick(2) ? need : AMPLE;
    d.add(fmt("%d %d %d %d %d %d %d ", bwd, B, T, H, HD, flags, ws == AMPLE ? 2 : ws == need));
    d.add(run(bwd, B, T, H, HD, flags, ws));
    if (i % 1000 == 0) printf("sweep %5d %016llx\n", i, d.h);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) g_min_level = !strcmp(argv[1], "digest") ? 2 : !strcmp(argv[1], "full") ? 0 : 1;
  if (argc > 2) harness::g_cus = atoi(argv[2]);
  test_shapes();
  grid();
  sweep();
  return 0;
}
