// Host-only dump of the bf16 GEMM dispatch (csrc/gemm.hip): which kernel family, tile and split-K every
// problem lands on, and what the planning queries answer for it.  No kernel runs: the launch macros are
// replaced by no-ops, so the program needs no GPU (without one the CU count falls back to 256, the
// MI355X's, so the table is the GPU's table).  tests/test_gemm_plan_cpu.py builds it with
//   hipcc --offload-arch=gfx950 --cuda-host-only -O1 -I <csrc> tests/gemm_plan_dump.hip
// and compares its output with tests/golden/gemm_plan_parent.txt, recorded before the dispatch was
// rewritten around one plan function.
//
//   gemm_plan_dump [brief|digest|full]
// Every line has a level.  By default the featured sizes (the test tables, the K and ragged cases, two presets
// at 8192 tokens) print in full and the rest folds into one digest per section; `brief` (the test's run with
// default knobs) prints one digest line per featured size; `digest` (its knob runs) only the section and sweep
// digests; `full` prints everything.  The golden file holds brief and digest runs: to read a difference, build
// this program against both trees and compare their `full` listings.
//
// -DPLAN_CHECK: every dtc_gemm row also asks dtc_gemm_plan and aborts unless it returns exactly the
// return code and the record the stubbed launch wrote.
#include "common.h"
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)0)
#undef DTC_CHECK_LAUNCH
#define DTC_CHECK_LAUNCH() ((void)0)
#include "gemm.hip"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace {

typedef unsigned long long u64;

void* const PTR = (void*)0x10000;  // never dereferenced: nothing launches
const long AMPLE = 1L << 42;

struct Digest {
  u64 h = 1469598103934665603ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  void add(long v) { add(&v, sizeof v); }
  void add(const std::string& s) { add(s.data(), s.size()); }
};

int g_min_level = 1;  // full 0, default 1, brief 2, digest 3
Digest g_folded;  // lines not printed in full
long g_nfolded = 0;

// level 2: always printed; 1: printed unless brief; 0: only printed by `full`; the rest folds into the section digest
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

long round8(long v) { return (v + 7) / 8 * 8; }

const int EPIS[6] = {EPI_STORE, EPI_RESID, EPI_GELU, EPI_DGELU, EPI_LMHEAD, EPI_LMHEAD_EVAL};

GemmArgs make_args(int layout, int M, int N, int K, int epi, bool f32, bool bias, bool colsum, bool acc, bool ws,
                   bool defer) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  a.layout = layout; a.M = M; a.N = N; a.K = K;
  a.A = PTR; a.B = PTR; a.C = PTR;
  // leading dimensions padded to the 16-byte rows the entry points require, so ragged sizes reach the plan
  a.lda = round8(layout == 2 ? M : K);
  a.ldb = round8(layout == 0 ? K : N);
  a.ldc = round8(N);
  a.c_f32 = f32; a.epi = epi;
  a.bias = bias ? (const float*)PTR : nullptr;
  a.aux = PTR; a.ldaux = a.ldc; a.aux_out = PTR;
  a.alpha = 1.f; a.beta = acc ? 1.f : 0.f;
  a.labels = (const int*)PTR; a.n_valid = N;
  a.part = (float*)PTR; a.label_out = (float*)PTR; a.part_arg = (int*)PTR;
  a.workspace = PTR; a.ws_bytes = ws ? AMPLE : 0;
  a.defer_reduce = defer;
  a.colsum = colsum ? (float*)PTR : nullptr;
  return a;
}

struct Outcome {
  int rc;
  int rec[8];
  bool operator==(const Outcome& o) const { return rc == o.rc && !memcmp(rec, o.rec, sizeof rec); }
};

std::string show(const Outcome& o) {
  return fmt("rc %d rec %d %d %d %d %d %d %d %d", o.rc, o.rec[0], o.rec[1], o.rec[2], o.rec[3], o.rec[4], o.rec[5],
             o.rec[6], o.rec[7]);
}

Outcome read_record(int rc) {
  Outcome o;
  o.rc = rc;
  dtc_gemm_last_launch(o.rec);
  return o;
}

Outcome run_gemm(const GemmArgs& a) {
  g_last = LastLaunch{};  // an entry point that refuses leaves the record alone: start from "none"
  const Outcome o = read_record(dtc_gemm(&a, nullptr));
#ifdef PLAN_CHECK
  Outcome p;
  p.rc = dtc_gemm_plan(&a, p.rec);
  if (!(p == o)) {
    printf("PLAN MISMATCH layout %d M %d N %d K %d epi %d f32 %d bias %d colsum %d beta %g ws %ld defer %d\n  launched %s\n  planned  %s\n",
           a.layout, a.M, a.N, a.K, a.epi, a.c_f32, a.bias != nullptr, a.colsum != nullptr, a.beta, a.ws_bytes,
           a.defer_reduce, show(o).c_str(), show(p).c_str());
    exit(3);
  }
#endif
  return o;
}

std::string queries(int layout, int M, int N, int K) {
  return fmt("ws %ld wsplit %d %d fuses %d nparts %d", dtc_gemm_workspace_bytes(layout, M, N, K),
             dtc_gemm_wgrad_split(M, N, K, 0), dtc_gemm_wgrad_split(M, N, K, 1), dtc_gemm_wgrad_fuses_colsum(M, N, K),
             dtc_lmhead_nparts(M, N, K));
}

// One problem size under one layout, crossed with epilogue x output x beta x colsum x bias x workspace x defer
// (384 combinations, in that nesting order).  Runs of consecutive combinations with the same outcome print as
// one line "first-index count outcome" (one level below the size's own line, which carries their digest), so
// the listing is complete and short.
void dump_cross(int level, int layout, int M, int N, int K) {
  std::vector<std::string> rows;
  Digest d;
  Outcome prev{};
  int start = 0, idx = 0;
  auto flush = [&](int end) {
    if (end > start) rows.push_back(fmt("  %d %d %s", start, end - start, show(prev).c_str()));
  };
  for (int e = 0; e < 6; ++e)
    for (int f32 = 0; f32 < 2; ++f32)
      for (int acc = 0; acc < 2; ++acc)
        for (int cs = 0; cs < 2; ++cs)
          for (int bias = 0; bias < 2; ++bias)
            for (int ws = 0; ws < 2; ++ws)
              for (int defer = 0; defer < 2; ++defer, ++idx) {
                const Outcome o = run_gemm(make_args(layout, M, N, K, EPIS[e], f32, bias, cs, acc, ws, defer));
                d.add(&o, sizeof o);
                if (idx && !(o == prev)) {
                  flush(idx);
                  start = idx;
                }
                prev = o;
              }
  flush(idx);
  emit(level, fmt("P L%d %d %d %d %s all %016llx", layout, M, N, K, queries(layout, M, N, K).c_str(), d.h));
  for (const std::string& r : rows) emit(level - 1, r);
}

typedef std::tuple<int, int, int> Shape;  // M, N, K of C[M][N] = sum over K

struct Preset {
  const char* name;
  int d, ff;
};
const Preset PRESETS[5] = {{"reference", 512, 2048}, {"gpt2_small", 768, 3072}, {"gpt2_medium", 1024, 4096},
                           {"gpt_1p3b", 2048, 8192}, {"tiny", 64, 256}};
const int VOCAB = 50304;
const int TOKENS[4] = {1024, 4096, 8192, 16384};
const int SHARDS[3] = {1, 2, 4};

struct Dense {
  int out, in;
  bool bias;
};

// the Dense layers of a preset under tensor parallelism `tp` (column-parallel qkv / fc1 / lm_head shard
// `out`, row-parallel out_proj / fc2 shard `in`); the lm_head last
std::vector<Dense> layers(const Preset& p, int tp) {
  return {{3 * p.d / tp, p.d, true}, {p.d, p.d / tp, true}, {p.ff / tp, p.d, true}, {p.d, p.ff / tp, true},
          {VOCAB / tp, p.d, false}};
}

void named_shapes() {
  // forward (T, out, in), dgrad (T, in, out) and weight gradient (out, in, T) of every Dense
  std::set<Shape> all, featured;
  for (const Preset& p : PRESETS)
    for (int t : TOKENS)
      for (int tp : SHARDS)
        for (const Dense& d : layers(p, tp)) {
          const Shape s[3] = {Shape(t, d.out, d.in), Shape(t, d.in, d.out), Shape(d.out, d.in, t)};
          for (const Shape& x : s) {
            all.insert(x);
            if (tp == 1 && t == 8192 && (p.d == 768 || p.d == 512)) featured.insert(x);
          }
        }
  // the case tables of tests/test_gemm_floor_gpu.py and tests/test_gemm_n8_gpu.py
  const int cases[][3] = {
      {200, 136, 96}, {512, 768, 256}, {200, 136, 64}, {4000, 1024, 512}, {1024, 1536, 128}, {1000, 1544, 192},
      {4096, 4096, 64}, {2048, 16384, 64}, {2000, 16400, 128}, {256, 256, 16384}, {200, 264, 16384},
      {4096, 1536, 16384}, {256, 64, 256}, {256, 128, 256}, {256, 256, 256}, {256, 320, 256}, {8192, 768, 256},
      {2048, 7936, 256}, {8192, 2304, 256}, {8192, 768, 1024}, {8100, 768, 1024}, {4096, 1536, 1024},
      {8192, 1024, 1024}, {256, 64, 96}, {256, 128, 64}, {300, 136, 64}, {136, 200, 96}, {512, 512, 4096},
      {256, 256, 1024}, {256, 256, 8192}, {768, 768, 1024}, {768, 768, 8192}, {4096, 4096, 1024},
      {8192, 2304, 768}, {8192, 768, 768}, {8192, 3072, 768}, {8192, 768, 3072}, {8100, 768, 768},
      {8192, 4096, 1024}, {8192, 1024, 4096}, {2304, 768, 8192}, {3072, 768, 8192}, {768, 3072, 8192},
      {4096, 3072, 1024},
      // K in {32, 96, 16384, 50304}
      {512, 512, 32}, {4096, 768, 32}, {512, 512, 96}, {4096, 768, 96}, {512, 512, 16384}, {4096, 768, 16384},
      {8192, 768, 16384}, {512, 512, 50304}, {4096, 768, 50304}, {8192, 1024, 50304}, {16384, 2048, 50304},
      // one ragged M and one ragged N per family (register / DMA 64^2, 8-wave, 256^2, gemm8r, gemm8n)
      {1001, 768, 256}, {1024, 766, 256}, {1000, 1536, 128}, {1024, 1540, 128}, {4090, 4096, 64}, {4096, 4100, 64},
      {8190, 2304, 768}, {8192, 2300, 768}, {8100, 1024, 1024}, {8192, 1020, 1024},
  };
  for (const auto& c : cases) {
    all.insert(Shape(c[0], c[1], c[2]));
    featured.insert(Shape(c[0], c[1], c[2]));
  }
  printf("# named shapes: %zu sizes x 3 layouts x 384 combinations\n", all.size());
  for (const Shape& s : all)
    for (int layout = 0; layout < 3; ++layout)
      dump_cross(featured.count(s) ? 2 : 0, layout, std::get<0>(s), std::get<1>(s), std::get<2>(s));
  end_section("named shapes");
}

void pairs() {
  for (const Preset& p : PRESETS)
    for (int t : TOKENS)
      for (int tp : SHARDS) {
        const std::vector<Dense> ls = layers(p, tp);
        for (size_t li = 0; li < ls.size(); ++li)
          for (int nt = 0; nt < 2; ++nt)
            for (int e = 0; e < 3; ++e)  // dgrad: bf16 store, fp32 store, bf16 dGELU
              for (int cs = 0; cs < 2; ++cs) {
                const Dense& d = ls[li];
                GemmArgs a1 = make_args(nt ? 0 : 1, t, d.in, d.out, e == 2 ? EPI_DGELU : EPI_STORE, e == 1, false,
                                        false, false, true, false);
                GemmArgs a2 = make_args(2, d.out, d.in, t, EPI_STORE, true, false, cs, false, true, true);
                g_last = LastLaunch{};
                const Outcome o = read_record(dtc_gemm_pair(&a1, &a2, nullptr));
                emit(tp != 1 ? 0 : (p.d == 768 && t == 8192) ? 2 : 1, fmt("pair %s t %d tp %d layer %zu nt %d epi %d cs %d %s", p.name, t,
                                                        tp, li, nt, e, cs, show(o).c_str()));
              }
      }
  end_section("pairs");
}

void groups() {
  for (const Preset& p : PRESETS)
    for (int t : TOKENS)
      for (int tp : SHARDS) {
        static WgBatch b;
        memset(&b, 0, sizeof b);
        for (const Dense& d : layers(p, tp)) {
          WgEntry& w = b.e[b.n++];
          w.A = (const bf16*)PTR; w.B = (const bf16*)PTR; w.C = (float*)PTR;
          w.cs = d.bias ? (float*)PTR : nullptr;
          w.M = d.out; w.N = d.in;
        }
        b.K = t;
        for (int ts = 0; ts < 3; ++ts) {  // tail split off, auto, forced 3
          b.tail_split = ts == 2 ? 3 : ts;
          b.tail_slab = (float*)PTR;
          b.tail_cap = AMPLE;
          g_last = LastLaunch{};
          const Outcome o = read_record(dtc_wgrad_group(&b, nullptr));
          emit(p.d == 768 && tp == 1 ? 2 : 1, fmt("group %s t %d tp %d tail %d %s", p.name, t, tp, b.tail_split, show(o).c_str()));
        }
      }
  end_section("groups");
}

void ce_dgrads() {
  for (const Preset& p : PRESETS)
    for (int t : TOKENS)
      for (int tp : SHARDS)
        for (int ws = 0; ws < 2; ++ws) {
          const int M = t, N = p.d, K = VOCAB / tp;
          g_last = LastLaunch{};
          const Outcome o = read_record(dtc_ce_dgrad((const bf16*)PTR, K, (const float*)PTR, (const int*)PTR, 0, K, 1.f,
                                                     (const bf16*)PTR, N, (bf16*)PTR, K, (float*)PTR, (float*)PTR, M, N,
                                                     K, (float*)PTR, ws ? AMPLE : 0, nullptr));
          emit(p.d == 768 ? 2 : 1, fmt("ce %s t %d tp %d ws %d bytes %ld colpart %d %s", p.name, t, tp, ws,
                      dtc_ce_dgrad_workspace_bytes(M, N, K), dtc_ce_dgrad_colpart_rows(M), show(o).c_str()));
        }
  end_section("ce dgrads");
}

// ---- seeded sweep ------------------------------------------------------------------------------------
u64 g_rng = 0x9E3779B97F4A7C15ull;
u64 rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
int pick(int n) { return (int)(rnd() % (u64)n); }

// a size in [1, hi]: mostly multiples of 256 / 192 / 64 / 8, sometimes anything
int size(int hi) {
  const int unit[6] = {256, 256, 192, 64, 8, 1};
  const int u = unit[pick(6)];
  return (1 + pick(hi / u)) * u;
}
int depth() {
  switch (pick(8)) {
    case 0: return 32 * (1 + pick(64));             // multiples of 32 only
    case 1: return 64 * (1 + pick(1024));           // up to 65536
    case 2: return 1 + pick(4096);                  // mostly refused
    case 3: return 8192 << pick(3);                 // 8192 / 16384 / 32768
    case 4: return 50304 / (1 << pick(3));
    default: return 64 * (1 + pick(128));           // layer-sized
  }
}

void sweep() {
  Digest d;
  for (int i = 1; i <= 20000; ++i) {
    const int layout = pick(16) == 0 ? 3 : pick(3);
    const int M = size(pick(4) ? 16384 : 1024), N = size(pick(8) ? 8192 : 50304), K = depth();
    const int epi = pick(24) == 0 ? EPI_RESID_LN : EPIS[pick(6)];
    const unsigned bits = (unsigned)rnd();
    GemmArgs a = make_args(layout, M, N, K, epi, bits & 1, bits & 2, bits & 4, bits & 8, (bits & 48) != 0, bits & 64);
    if ((bits & 0xF00) == 0) a.alpha = 0.5f;
    if ((bits & 0xF000) == 0) a.part_arg = nullptr;
    if ((bits & 0x30000) == 0) a.ws_bytes = (long)M * N * 8;  // enough for split 2 only
    const Outcome o = run_gemm(a);
    d.add(o.rc);
    for (int v : o.rec) d.add(v);
    d.add(dtc_gemm_workspace_bytes(layout, M, N, K));
    d.add(dtc_gemm_wgrad_split(M, N, K, 0));
    d.add(dtc_gemm_wgrad_split(M, N, K, 1));
    d.add(dtc_gemm_wgrad_fuses_colsum(M, N, K));
    d.add(dtc_lmhead_nparts(M, N, K));
    d.add(dtc_ce_dgrad_workspace_bytes(M, N, K));
    if (layout <= 1 && K % 8 == 0) {  // the same Dense's dgrad + weight gradient as a pair
      GemmArgs a2 = make_args(2, K, N, M, EPI_STORE, true, false, bits & 128, false, (bits & 48) != 0, !(bits & 64));
      g_last = LastLaunch{};
      const Outcome po = read_record(dtc_gemm_pair(&a, &a2, nullptr));
      d.add(po.rc);
      for (int v : po.rec) d.add(v);
    }
    if (i % 1000 == 0) printf("sweep %5d %016llx\n", i, d.h);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1)
    g_min_level = !strcmp(argv[1], "digest") ? 3 : !strcmp(argv[1], "brief") ? 2 : !strcmp(argv[1], "full") ? 0 : 1;
  named_shapes();
  pairs();
  groups();
  ce_dgrads();
  sweep();
  return 0;
}
