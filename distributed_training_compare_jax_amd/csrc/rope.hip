// Rotary position embeddings (RoPE), rotate-half pairing (Llama / GPT-NeoX), applied in place to the Q and K
// heads of a packed activation x[rows = B*T][ld = (H + 2 Hkv) * hd] between the qkv GEMM and the attention
// (forward), and as the transposed rotation to dQ | dK after the attention backward (INVERSE).
//
//   lo' = lo * cos[t, i] - hi * sin[t, i]        lo = head[i], hi = head[i + hd/2], i < hd/2, t = row % T
//   hi' = hi * cos[t, i] + lo * sin[t, i]        INVERSE: sin -> -sin (the exact transpose)
//
// fp32 math, one rounding to T (round-to-nearest-even).  cos / sin come from a host-built float2 table
// tab[tab_rows][hd/2] (ops/rope.py rope_table): no transcendental function here.  The V columns are never touched.
//
// Work split, as embed_fwd_kernel (csrc/elementwise.hip): one wave per token row, four rows per 256-thread block, so
// the position and the table row are wave-uniform.  A lane owns one 16-byte vector of a head's low half and the
// matching vector of its high half (bf16: 8 pairs, hd/16 lanes per head; fp32: 4 pairs, hd/8 lanes per head); the
// wave covers 64 / lanes_per_head heads per pass and loops over passes.  The lane's 8 (4) table entries are loaded
// once per row, before the head loop, and reused for every head.  Both 16-byte loads of a pass are issued before its
// math; stores are 16 bytes.  A head count that does not fill the last pass masks lanes (the same code path).  No
// LDS, no atomics, no scratch; registers and occupancy of every instantiation: profiles/rope.md.
// Minimal traffic: 2 * rows * (H + Hkv) * hd * sizeof(T) bytes; the table (T * hd * 4 bytes) stays in L2.
//
// Out of scope here: fusing the rotation into the qkv GEMM epilogue or the attention loads, the interleaved
// (GPT-J) pairing, partial rotary dimensions, position offsets (KV-cache decode), NTK / YaRN scaling.
#include "common.h"

namespace {

template <typename T> struct RopeVec;
template <> struct RopeVec<bf16> { typedef bf16x8 type; };
template <> struct RopeVec<float> { typedef f32x4 type; };

template <typename T, int HD, bool INVERSE>
__global__ void __launch_bounds__(256) rope_kernel(T* __restrict__ x, const f32x2* __restrict__ tab, int rows, int seq,
                                                   int nrot, long ld) {
  using V = typename RopeVec<T>::type;
  constexpr int N = 16 / sizeof(T);  // pairs per lane
  constexpr int LPH = HD / 2 / N;    // lanes per head
  constexpr int HPP = 64 / LPH;      // heads per pass
  static_assert(LPH >= 1 && 64 % LPH == 0, "head_dim");
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int t = row % seq;
  const int hl = lane / LPH, i0 = (lane % LPH) * N;
  // (cos, sin) of this lane's N pairs: N/2 vectors of two float2 entries
  f32x4 cs[N / 2];
  const f32x4* tp = (const f32x4*)(tab + (long)t * (HD / 2) + i0);
#pragma unroll
  for (int k = 0; k < N / 2; ++k) cs[k] = tp[k];
  T* xr = x + (long)row * ld + i0;
  for (int h0 = 0; h0 < nrot; h0 += HPP) {
    const int h = h0 + hl;
    if (h >= nrot) continue;  // partly filled last pass
    DTC_ASSERT((long)h * HD + i0 + HD / 2 + N <= ld);
    V* plo = (V*)(xr + (long)h * HD);
    V* phi = (V*)(xr + (long)h * HD + HD / 2);
    const V lo = *plo, hi = *phi;
    V olo, ohi;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float c = cs[e >> 1][2 * (e & 1)];
      const float s = INVERSE ? -cs[e >> 1][2 * (e & 1) + 1] : cs[e >> 1][2 * (e & 1) + 1];
      const float a = (float)lo[e], b = (float)hi[e];
      olo[e] = (T)(a * c - b * s);
      ohi[e] = (T)(b * c + a * s);
    }
    *plo = olo;
    *phi = ohi;
  }
}

template <typename T, int HD>
int rope_launch(void* x, const void* tab, int rows, int seq, int nrot, long ld, int inverse, hipStream_t st) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (inverse)
    hipLaunchKernelGGL((rope_kernel<T, HD, true>), grid, block, 0, st, (T*)x, (const f32x2*)tab, rows, seq, nrot, ld);
  else
    hipLaunchKernelGGL((rope_kernel<T, HD, false>), grid, block, 0, st, (T*)x, (const f32x2*)tab, rows, seq, nrot, ld);
  DTC_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int rope_dispatch(void* x, const void* tab, int rows, int seq, int nrot, long ld, int head_dim, int inverse,
                  hipStream_t st) {
  switch (head_dim) {
    case 32: return rope_launch<T, 32>(x, tab, rows, seq, nrot, ld, inverse, st);
    case 64: return rope_launch<T, 64>(x, tab, rows, seq, nrot, ld, inverse, st);
    default: return rope_launch<T, 128>(x, tab, rows, seq, nrot, ld, inverse, st);
  }
}

}  // namespace

extern "C" {

// x: bf16 (dtype 0) or fp32 (dtype 1) [B*T][(H + 2 Hkv) * head_dim], rotated in place over its first (H + Hkv) *
// head_dim columns; tab: float2 [tab_rows][head_dim / 2] of (cos, sin).  Refusals launch nothing (codes of this
// file: 500x).
int dtc_rope(void* x, const void* tab, int B, int T, int H, int Hkv, int head_dim, int tab_rows, int dtype,
             int inverse, hipStream_t st) {
  if (head_dim != 32 && head_dim != 64 && head_dim != 128) return 5001;
  if (Hkv < 1 || H < 1 || H % Hkv) return 5002;
  if (T < 1 || T > tab_rows) return 5003;
  if (((uintptr_t)x | (uintptr_t)tab) & 15) return 5004;
  if (dtype != 0 && dtype != 1) return 5005;
  if (B < 1 || (long)B * T > 0x7fffffffL - 4) return 5006;
  const int rows = B * T, nrot = H + Hkv;
  const long ld = (long)(H + 2 * Hkv) * head_dim;
  return dtype ? rope_dispatch<float>(x, tab, rows, T, nrot, ld, head_dim, inverse, st)
               : rope_dispatch<bf16>(x, tab, rows, T, nrot, ld, head_dim, inverse, st);
}

}  // extern "C"
