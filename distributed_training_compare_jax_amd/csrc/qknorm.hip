// QK-norm (ModelConfig.qk_norm: rmsnorm) fused with the rotary embedding: an RMSNorm over head_dim of every query and
// key head of the packed activation x[rows = B*T][ld = (H + 2 Hkv) * hd], a learned gain shared by the heads of a
// kind (gq [hd] for the H query heads, gk [hd] for the Hkv key heads), then the rotation of csrc/rope.hip -- all in the
// one in-place pass over the Q | K columns that RoPE already pays for, between the qkv GEMM and the attention.
//
//   forward   rstd = rsqrt(mean_i(x_i^2) + eps)    xh = x * rstd    z = xh * g    y = rope(z)   (no table: y = z)
//   backward  dz = rope^T(dy)  (or dy)             dxh = dz * g
//             dx = rstd * (dxh - xh * mean_i(dxh_i * xh_i))
//             dg[i] = beta * dg[i] + sum_rows sum_heads dz_i * xh_i        (query heads -> dgq, key heads -> dgk)
//
// fp32 math, one rounding to T.  The V columns are never touched.  The table is the float2 (cos, sin) table of
// ops/rope.py; a null table means no rotation (pos_emb: learned) and compiles to kernels without the table loads.
//
// Work split: rope_kernel's.  One wave per token row (position and table row wave-uniform); a lane owns one 16-byte
// vector of a head's low half and the matching vector of its high half (bf16: 8 + 8 elements, LPH = hd/16 lanes per
// head; fp32: 4 + 4, LPH = hd/8), so a rotation pair never leaves its lane and a head is LPH ADJACENT lanes: the
// per-head sums (sum x^2 forward, sum dxh * xh backward) are log2(LPH) xor-shuffles, no LDS.  The wave covers
// 64 / LPH heads per pass; a pass that straddles the Q / K boundary picks the gain (and, backward, the accumulator)
// per head with selects, and a partly filled last pass masks its loads and stores while every lane still takes part
// in the shuffles.  The lane's slice of gq and gk and its table entries are loaded once per row, before the head loop.
//
// Forward, one launch: reads the raw Q | K columns once; writes y in place, the raw columns again as the compact
// qk_raw[rows][(H + Hkv) * hd] (activation dtype, bit-equal to the input) and rstd[rows][H + Hkv] (fp32).
// The raw copy is deliberate: the backward needs xh, and recovering it from y would mean dividing by the gain, which
// is ill-conditioned near g = 0 (and g = 0 is a legitimate value of a learned gain).  It costs
// rows * (H + Hkv) * hd * sizeof(T) + rows * (H + Hkv) * 4 bytes of saved activation per layer: at gpt-1.3b GQA
// (H 16, Hkv 4, hd 128, T 2048, bf16) 10.6 MB per sequence and layer next to the 12.6 MB of qkv itself.
// Minimal traffic: read n, write 2 n + rstd, n = rows * (H + Hkv) * hd * sizeof(T).
//
// Backward, in place on the Q | K columns of dqkv: reads dy, qk_raw, rstd, writes dx.  A block of 4 waves walks
// QKN_BWD_ROWS rows; each lane keeps fp32 accumulators of ITS columns (2 x 16-byte vectors wide) for gq and for gk
// across every head and row it visits.  At the end the lanes that hold the same columns (same lane % LPH) are summed
// by xor-shuffles in a fixed order, the 4 waves meet in 4 x 2 x hd floats of LDS and are summed in a fixed order, and
// the block writes one [2][hd] partial into part[blocks][2][hd].  The slab is finished by the ordered reduction
// below -- the TALL arithmetic of reduce_tasks_kernel (csrc/norm_reduce.hip), as rms_slab_reduce (csrc/rmsnorm.hip) --
// or left for GradReducer.add_tall: bitwise the same.  No float atomics, no scratch.
// Minimal traffic: read 2 n + rstd, write n.
// Registers, LDS and occupancy of every instantiation: profiles/qknorm.md.
//
// Out of scope here: per-head (unshared) gains, a LayerNorm-style norm with bias, fusing the pass into the qkv GEMM
// epilogue or the attention loads, tensor parallelism (each rank's partials cover its own heads only).
#include "common.h"

namespace {

constexpr int QKN_BWD_ROWS = 32;  // rows per backward block (8 per wave): the partial slab has ceil(rows / 32) entries

template <typename T> struct QknVec;
template <> struct QknVec<bf16> { typedef bf16x8 type; };
template <> struct QknVec<float> { typedef f32x4 type; };

// sum over the LPH adjacent lanes of a head (LPH a power of two, groups aligned): every lane of the wave takes part
template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int o = LPH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// this lane's N (cos, sin) entries of table row t, or (1, 0) without a table
template <int N, int HD, bool TAB>
__device__ __forceinline__ void load_cs(const f32x2* tab, int t, int i0, float (&c)[N], float (&s)[N]) {
  if constexpr (TAB) {
    const f32x4* tp = (const f32x4*)(tab + (long)t * (HD / 2) + i0);
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
      const f32x4 v = tp[k];
      c[2 * k] = v[0], s[2 * k] = v[1], c[2 * k + 1] = v[2], s[2 * k + 1] = v[3];
    }
  }
}

// g[i0 .. i0 + N) and g[HD/2 + i0 .. HD/2 + i0 + N) of a gain vector
template <int N, int HD>
__device__ __forceinline__ void load_gain(const float* __restrict__ g, int i0, float (&lo)[N], float (&hi)[N]) {
#pragma unroll
  for (int k = 0; k < N / 4; ++k) {
    const f32x4 a = *(const f32x4*)(g + i0 + 4 * k), b = *(const f32x4*)(g + HD / 2 + i0 + 4 * k);
#pragma unroll
    for (int e = 0; e < 4; ++e) lo[4 * k + e] = a[e], hi[4 * k + e] = b[e];
  }
}

template <typename T, int HD, bool TAB>
__global__ void __launch_bounds__(256) qknorm_fwd_kernel(T* __restrict__ x, const f32x2* __restrict__ tab,
                                                         const float* __restrict__ gq, const float* __restrict__ gk,
                                                         T* __restrict__ raw, float* __restrict__ rstd_out, int rows,
                                                         int seq, int nq, int nrot, long ld, float eps) {
  using V = typename QknVec<T>::type;
  constexpr int N = 16 / sizeof(T);  // elements per vector: the lane holds N of the low half and N of the high half
  constexpr int LPH = HD / 2 / N;    // lanes per head
  constexpr int HPP = 64 / LPH;      // heads per pass
  static_assert(LPH >= 1 && 64 % LPH == 0 && N % 4 == 0, "head_dim");
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int hl = lane / LPH, i0 = (lane % LPH) * N;
  float c[N], s[N], gql[N], gqh[N], gkl[N], gkh[N];
  load_cs<N, HD, TAB>(tab, row % seq, i0, c, s);
  load_gain<N, HD>(gq, i0, gql, gqh);
  load_gain<N, HD>(gk, i0, gkl, gkh);
  T* xr = x + (long)row * ld + i0;
  T* rr = raw + (long)row * nrot * HD + i0;
  for (int h0 = 0; h0 < nrot; h0 += HPP) {
    const int h = h0 + hl;
    const bool ok = h < nrot;           // partly filled last pass: load head nrot - 1 again, store nothing
    const int hc = ok ? h : nrot - 1;
    DTC_ASSERT((long)hc * HD + i0 + HD / 2 + N <= ld);
    V* plo = (V*)(xr + (long)hc * HD);
    V* phi = (V*)(xr + (long)hc * HD + HD / 2);
    const V lo = *plo, hi = *phi;
    float a[N], b[N], ss = 0.f;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      a[e] = (float)lo[e], b[e] = (float)hi[e];
      ss += a[e] * a[e] + b[e] * b[e];
    }
    const float rs = rsqrtf(head_sum<LPH>(ss) / HD + eps);
    const bool isq = h < nq;
    V olo, ohi;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float za = a[e] * rs * (isq ? gql[e] : gkl[e]), zb = b[e] * rs * (isq ? gqh[e] : gkh[e]);
      if constexpr (TAB) {
        olo[e] = (T)(za * c[e] - zb * s[e]);
        ohi[e] = (T)(zb * c[e] + za * s[e]);
      } else {
        olo[e] = (T)za;
        ohi[e] = (T)zb;
      }
    }
    if (ok) {
      *(V*)(rr + (long)h * HD) = lo;
      *(V*)(rr + (long)h * HD + HD / 2) = hi;
      *plo = olo;
      *phi = ohi;
      if (lane % LPH == 0) rstd_out[(long)row * nrot + h] = rs;
    }
  }
}

template <typename T, int HD, bool TAB>
__global__ void __launch_bounds__(256) qknorm_bwd_kernel(T* __restrict__ dy, const f32x2* __restrict__ tab,
                                                         const T* __restrict__ raw, const float* __restrict__ rstd,
                                                         const float* __restrict__ gq, const float* __restrict__ gk,
                                                         float* __restrict__ part, int rows, int seq, int nq, int nrot,
                                                         long ld) {
  using V = typename QknVec<T>::type;
  constexpr int N = 16 / sizeof(T);
  constexpr int LPH = HD / 2 / N;
  constexpr int HPP = 64 / LPH;
  static_assert(LPH >= 1 && 64 % LPH == 0 && N % 4 == 0, "head_dim");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hl = lane / LPH, i0 = (lane % LPH) * N;
  DTC_ASSERT((long)blockIdx.x * QKN_BWD_ROWS < rows);
  float gql[N], gqh[N], gkl[N], gkh[N];
  load_gain<N, HD>(gq, i0, gql, gqh);
  load_gain<N, HD>(gk, i0, gkl, gkh);
  // column accumulators of this lane's 2 N columns: [0] query heads, [1] key heads
  float al[2][N], ah[2][N];
#pragma unroll
  for (int e = 0; e < N; ++e) al[0][e] = al[1][e] = ah[0][e] = ah[1][e] = 0.f;
  const int rend = min(rows, (int)(blockIdx.x + 1) * QKN_BWD_ROWS);
  for (int row = blockIdx.x * QKN_BWD_ROWS + wave; row < rend; row += 4) {  // wave-uniform
    float c[N], s[N];
    load_cs<N, HD, TAB>(tab, row % seq, i0, c, s);
    T* dr = dy + (long)row * ld + i0;
    const T* rr = raw + (long)row * nrot * HD + i0;
    const float* rsr = rstd + (long)row * nrot;
    for (int h0 = 0; h0 < nrot; h0 += HPP) {
      const int h = h0 + hl;
      const bool ok = h < nrot;  // a head past the end re-reads head nrot - 1 and counts as zeros
      const int hc = ok ? h : nrot - 1;
      DTC_ASSERT((long)hc * HD + i0 + HD / 2 + N <= ld);
      V* plo = (V*)(dr + (long)hc * HD);
      V* phi = (V*)(dr + (long)hc * HD + HD / 2);
      const V dlo = *plo, dhi = *phi;
      const V xlo = *(const V*)(rr + (long)hc * HD), xhi = *(const V*)(rr + (long)hc * HD + HD / 2);
      const float rs = ok ? rsr[hc] : 0.f;  // rs = 0: xh = 0, so the masked head adds nothing anywhere
      const bool isq = h < nq;
      float dza[N], dzb[N], xa[N], xb[N], dot = 0.f;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float a = (float)dlo[e], b = (float)dhi[e];
        if constexpr (TAB) {  // the transposed rotation: sin -> -sin
          dza[e] = a * c[e] + b * s[e];
          dzb[e] = b * c[e] - a * s[e];
        } else {
          dza[e] = a, dzb[e] = b;
        }
        xa[e] = (float)xlo[e] * rs, xb[e] = (float)xhi[e] * rs;
        const float pa = dza[e] * xa[e], pb = dzb[e] * xb[e];  // dz * xh: the gain gradient's summand
        al[0][e] += isq ? pa : 0.f, al[1][e] += isq ? 0.f : pa;
        ah[0][e] += isq ? pb : 0.f, ah[1][e] += isq ? 0.f : pb;
        dza[e] *= isq ? gql[e] : gkl[e];  // dxh = dz * g
        dzb[e] *= isq ? gqh[e] : gkh[e];
        dot += dza[e] * xa[e] + dzb[e] * xb[e];
      }
      const float m = head_sum<LPH>(dot) / HD;
      V olo, ohi;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        olo[e] = (T)(rs * (dza[e] - xa[e] * m));
        ohi[e] = (T)(rs * (dzb[e] - xb[e] * m));
      }
      if (ok) {
        *plo = olo;
        *phi = ohi;
      }
    }
  }
  // lanes with the same lane % LPH hold the same columns: fixed xor order LPH, 2 LPH, .. 32
  __shared__ __attribute__((aligned(16))) float red[4][2][HD];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
      float u = al[k][e], v = ah[k][e];
#pragma unroll
      for (int o = LPH; o < 64; o <<= 1) u += __shfl_xor(u, o, 64), v += __shfl_xor(v, o, 64);
      if (lane < LPH) red[wave][k][i0 + e] = u, red[wave][k][HD / 2 + i0 + e] = v;
    }
  }
  __syncthreads();
  // the 4 waves in a fixed order; thread j owns element j of the block's [2][HD] partial (2 HD <= 256)
  if ((int)threadIdx.x < 2 * HD) {
    const float* r0 = &red[0][0][0];
    const int j = threadIdx.x;
    part[(long)blockIdx.x * 2 * HD + j] = (r0[j] + r0[2 * HD + j]) + (r0[4 * HD + j] + r0[6 * HD + j]);
  }
}

// out[c] (beta*out[c] +)= sum_p part[(p * 2 + k) * D + c], slab k = blockIdx.y -> o0 / o1: 32 columns x 8 partial groups
// per block, p ascending within a group, the groups added in order -- the TALL arithmetic of reduce_tasks_kernel
// (the copy of rms_slab_reduce, csrc/rmsnorm.hip), so the deferred path gives the same bits.
constexpr int QS_COLS = 32, QS_GROUPS = 256 / QS_COLS;
__global__ void __launch_bounds__(256) qkn_slab_reduce(const float* __restrict__ part, int P, int D,
                                                       float* __restrict__ o0, float* __restrict__ o1, float beta) {
  const int tx = threadIdx.x % QS_COLS, ty = threadIdx.x / QS_COLS;
  const int c = blockIdx.x * QS_COLS + tx;
  DTC_ASSERT(P >= 1 && (int)blockIdx.y < 2 && (long)blockIdx.x * QS_COLS < D);
  const float* src = part + (long)blockIdx.y * D;
  const long pstride = 2L * D;
  float s = 0.f;
  if (c < D) {
#pragma unroll 8
    for (int p = ty; p < P; p += QS_GROUPS) s += src[(long)p * pstride + c];
  }
  __shared__ float red[QS_GROUPS][QS_COLS];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < D) {
    float u = 0.f;
#pragma unroll
    for (int gi = 0; gi < QS_GROUPS; ++gi) u += red[gi][tx];
    float* o = blockIdx.y == 0 ? o0 : o1;
    o[c] = beta != 0.f ? beta * o[c] + u : u;
  }
}

struct QknArgs {
  void* x;
  const void* tab;
  const float *gq, *gk;
  void* raw;      // forward: written; backward: read
  float* rstd;    // forward: written; backward: read
  float* part;    // backward only
  int rows, seq, nq, nrot;
  long ld;
  float eps;
};

template <typename T, int HD, bool TAB>
void qkn_launch(const QknArgs& a, bool bwd, hipStream_t st) {
  if (bwd)
    hipLaunchKernelGGL((qknorm_bwd_kernel<T, HD, TAB>), dim3((a.rows + QKN_BWD_ROWS - 1) / QKN_BWD_ROWS), dim3(256), 0, st,
                       (T*)a.x, (const f32x2*)a.tab, (const T*)a.raw, (const float*)a.rstd, a.gq, a.gk, a.part, a.rows,
                       a.seq, a.nq, a.nrot, a.ld);
  else
    hipLaunchKernelGGL((qknorm_fwd_kernel<T, HD, TAB>), dim3((a.rows + 3) / 4), dim3(256), 0, st, (T*)a.x,
                       (const f32x2*)a.tab, a.gq, a.gk, (T*)a.raw, a.rstd, a.rows, a.seq, a.nq, a.nrot, a.ld, a.eps);
}

template <typename T, int HD>
void qkn_tab(const QknArgs& a, bool bwd, hipStream_t st) {
  if (a.tab) qkn_launch<T, HD, true>(a, bwd, st);
  else qkn_launch<T, HD, false>(a, bwd, st);
}

template <typename T>
void qkn_dispatch(const QknArgs& a, int head_dim, bool bwd, hipStream_t st) {
  switch (head_dim) {
    case 32: return qkn_tab<T, 32>(a, bwd, st);
    case 64: return qkn_tab<T, 64>(a, bwd, st);
    default: return qkn_tab<T, 128>(a, bwd, st);
  }
}

// the refusals shared by both entry points: nothing is launched (codes of this file: 600x)
int qkn_refuse(const void* x, const void* tab, const void* gq, const void* gk, const void* raw, const void* rstd, int B,
               int T, int H, int Hkv, int head_dim, int tab_rows, int dtype) {
  if (head_dim != 32 && head_dim != 64 && head_dim != 128) return 6001;
  if (Hkv < 1 || H < 1 || H % Hkv) return 6002;
  if (T < 1 || (tab && T > tab_rows)) return 6003;
  if (((uintptr_t)x | (uintptr_t)tab | (uintptr_t)gq | (uintptr_t)gk | (uintptr_t)raw) & 15 || ((uintptr_t)rstd & 3))
    return 6004;
  if (dtype != 0 && dtype != 1) return 6005;
  if (B < 1 || (long)B * T > 0x7fffffffL - QKN_BWD_ROWS) return 6006;
  if (!x || !gq || !gk || !raw || !rstd) return 6007;
  return 0;
}

}  // namespace

extern "C" {

// x: bf16 (dtype 0) or fp32 (dtype 1) [B*T][(H + 2 Hkv) * head_dim]; its first (H + Hkv) * head_dim columns are
// normalised per head, scaled by gq / gk (fp32 [head_dim]) and rotated by tab (float2 [tab_rows][head_dim / 2] of
// (cos, sin); null: no rotation) in place.  qk_raw [B*T][(H + Hkv) * head_dim] (dtype of x) receives the raw columns,
// rstd [B*T][H + Hkv] (fp32) the statistics.  Refusals launch nothing and leave every tensor as it is.
int dtc_qknorm_fwd(void* x, const void* tab, const float* gq, const float* gk, void* qk_raw, float* rstd, int B, int T,
                   int H, int Hkv, int head_dim, int tab_rows, float eps, int dtype, hipStream_t st) {
  if (const int e = qkn_refuse(x, tab, gq, gk, qk_raw, rstd, B, T, H, Hkv, head_dim, tab_rows, dtype)) return e;
  const QknArgs a{x, tab, gq, gk, qk_raw, rstd, nullptr, B * T, T, H, H + Hkv, (long)(H + 2 * Hkv) * head_dim, eps};
  if (dtype) qkn_dispatch<float>(a, head_dim, false, st);
  else qkn_dispatch<bf16>(a, head_dim, false, st);
  DTC_CHECK_LAUNCH();
  return 0;
}

// the backward's partial slab: [ceil(rows / QKN_BWD_ROWS)][2][head_dim] floats
long dtc_qknorm_bwd_workspace_bytes(int rows, int head_dim) {
  return (long)((rows + QKN_BWD_ROWS - 1) / QKN_BWD_ROWS) * 2 * head_dim * 4;
}

// dy: the Q | K columns of dqkv [B*T][(H + 2 Hkv) * head_dim] are replaced in place by dx; dgq / dgk (fp32
// [head_dim]) = (accumulate ? dg : 0) + sum_rows sum_heads dz * xh.  defer: the partials stay in ws as
// [blocks][2][head_dim] (slab 0: dgq, slab 1: dgk) for the caller's reducer.
int dtc_qknorm_bwd(void* dy, const void* tab, const void* qk_raw, const float* rstd, const float* gq, const float* gk,
                   float* dgq, float* dgk, int B, int T, int H, int Hkv, int head_dim, int tab_rows, int dtype,
                   int accumulate, float* ws, long ws_bytes, int defer, hipStream_t st) {
  if (const int e = qkn_refuse(dy, tab, gq, gk, qk_raw, rstd, B, T, H, Hkv, head_dim, tab_rows, dtype)) return e;
  const int rows = B * T;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < dtc_qknorm_bwd_workspace_bytes(rows, head_dim)) return 6008;
  if (!dgq || !dgk) return 6007;
  const QknArgs a{dy, tab, gq, gk, (void*)qk_raw, (float*)rstd, ws, rows, T, H, H + Hkv, (long)(H + 2 * Hkv) * head_dim,
                  0.f};
  if (dtype) qkn_dispatch<float>(a, head_dim, true, st);
  else qkn_dispatch<bf16>(a, head_dim, true, st);
  DTC_CHECK_LAUNCH();
  if (defer) return 0;
  const int blocks = (rows + QKN_BWD_ROWS - 1) / QKN_BWD_ROWS;
  hipLaunchKernelGGL(qkn_slab_reduce, dim3((head_dim + QS_COLS - 1) / QS_COLS, 2), dim3(256), 0, st, ws, blocks, head_dim,
                     dgq, dgk, accumulate ? 1.f : 0.f);
  DTC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
