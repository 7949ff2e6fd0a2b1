// RMSNorm forward / backward (ModelConfig.norm: rmsnorm), fp32 math on the fp32 residual stream:
//
//   rstd = rsqrt(mean(x^2) + eps)      xh = x * rstd      y = xh * gamma          (y bf16, or fp32 in dtype: fp32)
//   c  = mean(gamma * dy * xh)         dx = rstd * (gamma * dy - xh * c) [+ dres]
//   dgamma = sum_rows dy * xh          dbias = sum_rows dx  (optional: the out_proj / fc2 bias gradient)
//
// One row statistic, no mean, no beta: what a lane holds is the row, gamma and (backward) two column accumulators,
// so the budgets are not the LayerNorm kernels' (csrc/norm_reduce.hip) and neither are the cut-offs below.
//
// Work split.  A lane owns 16-byte chunks (f32x4 / bf16x4) of a row; every global load of a row group is issued
// before the first reduction.
//   narrow: one wave64 per row, chunk lane + 64 i, i < NV.  Forward: one pass over registers, one warp_sum per row.
//           Backward: RMS_BWD_ROWS rows per block walked by 4 waves, the column accumulators of the 4 waves meet in
//           LDS ONE SLAB AT A TIME (4 x D floats, the buffer reused for the second slab), summed in a fixed order.
//   wide:   a row spread over the W waves of a block, wave w owning the contiguous chunks [w NV 64, (w + 1) NV 64).
//           The one row sum crosses the waves through R x W floats of LDS in a fixed pairwise order (one barrier per
//           row group, the buffer alternating between groups); the column partials are exclusive to the owning wave
//           and go straight to the slab: no block reduction.
// Column partials: part[blocks][nslab][D], slab 0 = dgamma, slab 1 (optional) = sum dx; finished by the ordered
// reduction below (the arithmetic of reduce_tasks_kernel's TALL mode, csrc/norm_reduce.hip, so the deferred path
// through GradReducer.add_tall is bitwise the direct one).  No float atomics.
// Registers, LDS, occupancy of every instantiation and the measured times: profiles/rmsnorm.md.
#include "common.h"

namespace {

constexpr int RMS_MAX_D = 8192;
// Cut-offs, from the registers each instantiation compiles to (profiles/rmsnorm.md).
// Forward: a wave holds the row and gamma, 8 NV VGPRs (LayerNorm: row, gamma, beta = 12 NV).  NV = 16 (D = 4096) compiles
// to 151 VGPRs with fp32 x and 208 with bf16 x: three / two waves per SIMD, each lane with 16 (+ 16) loads of 16 bytes in
// flight.  Twice that width would not fit 256 VGPRs, so rows wider than 4096 go to the wide kernel.
constexpr int RMS_FWD_NARROW_D = 4096;
// Backward: xh, dy, dres of the row (12 NV) + gamma and two accumulators (12 NV), and 4 x D floats of LDS for the
// slab-at-a-time block reduction.  NV = 6 (D = 1536) compiles to 230 VGPRs, two waves per SIMD, 24 KB of LDS; NV = 8
// needs 300 (AGPR copies, one wave per SIMD), so 1536 is the limit (LayerNorm: 1024, with 230 VGPRs and 48 KB there).
constexpr int RMS_BWD_NARROW_D = 1536;
constexpr int RMS_BWD_ROWS = 16;  // rows per block of every backward kernel: the partial slab has ceil(M / 16) rows

// 16-byte chunk c of the row at element offset off.  The row address is wave-uniform (scalar registers) and the lane's
// part a 32-bit byte offset: one VGPR per chunk shared by every stream, not a 64-bit address per load.
__device__ __forceinline__ f32x4 ld4(const void* p, long off, int c, bool bf) {
  if (bf) {
    const bf16x4 t = *(const bf16x4*)((const char*)p + off * 2 + (unsigned)c * 8u);
    return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
  }
  return *(const f32x4*)((const char*)p + off * 4 + (unsigned)c * 16u);
}
// chunk c of a row of D4 chunks, zeros past the end.  The load itself is unconditional on a clamped (in-bounds) chunk and
// the mask a select: straight-line code, so every load of a row group issues back to back (a branch per load cost
// 100+ VGPRs at NV = 6 and 8)
__device__ __forceinline__ f32x4 ld4m(const void* p, long off, int c, int D4, bool bf, bool ok = true) {
  const f32x4 t = ld4(p, off, min(c, D4 - 1), bf);
  return ok && c < D4 ? t : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void st4(void* p, long off, int c, bool f32, const f32x4& o) {
  if (f32) *(f32x4*)((char*)p + off * 4 + (unsigned)c * 16u) = o;
  else *(bf16x4*)((char*)p + off * 2 + (unsigned)c * 8u) = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
}
__device__ __forceinline__ float sum4(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// sum over the block's W waves of R per-wave values; buf is [R][W] floats of LDS, fixed pairwise order
template <int R, int W>
__device__ __forceinline__ void rms_block_sum(float (&v)[R], float* buf, int lane, int wave) {
  static_assert(W == 4 || W == 8, "pairwise order below");
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < R; ++q) buf[q * W + wave] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const float* p = buf + q * W;
    float t = (p[0] + p[1]) + (p[2] + p[3]);
    if constexpr (W == 8) t += (p[4] + p[5]) + (p[6] + p[7]);
    v[q] = t;
  }
}

// ---- forward, narrow: one wave per row ----
// resid (optional): the row is x + resid, written to x_out (may alias x unless XB) before it is normalised.
// XB: x is bf16 (a bf16 GEMM output).
template <int NV, bool XB>
__global__ void __launch_bounds__(256) rms_fwd_kernel(const void* x, const float* __restrict__ resid, float* x_out,
                                                      const float* __restrict__ g, void* __restrict__ y,
                                                      float* __restrict__ rstd_out, int M, int D, float eps, int out_f32) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= M) return;
  DTC_ASSERT(D % 4 == 0 && D / 4 <= NV * 64);
  const int D4 = D / 4;
  const long off = (long)row * D;
  f32x4 v[NV], gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = ld4m(x, off, c, D4, XB);
  }
  if (resid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += ld4m(resid, off, lane + 64 * i, D4, false);
  }
  // gamma is issued with the row loads: its latency hides under the reduction
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    gv[i] = ld4m(g, 0, c, D4, false);
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) ss += sum4(v[i] * v[i]);
  const float rstd = rsqrtf(warp_sum(ss) / D + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      if (x_out) st4(x_out, off, c, true, v[i]);
      st4(y, off, c, out_f32, v[i] * rstd * gv[i]);
    }
  }
}

// ---- forward, wide: R rows per block of W waves ----
template <int NV, int W, bool XB>
__global__ void __launch_bounds__(64 * W) rms_fwd_wide_kernel(const void* x, const float* __restrict__ resid, float* x_out,
                                                              const float* __restrict__ g, void* __restrict__ y,
                                                              float* __restrict__ rstd_out, int M, int D, float eps,
                                                              int out_f32) {
  constexpr int R = 4;  // 4 NV (x 2 with resid) loads of 16 bytes in flight per lane; 16 NV + 4 NV floats held
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = blockIdx.x * R;
  const int D4 = D / 4, cbase = wave * NV * 64 + lane;
  DTC_ASSERT(D % 4 == 0 && D4 <= NV * 64 * W && row0 < M && wave < W);
  __shared__ float xs[R * W];
  f32x4 v[R][NV], gv[NV];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const long off = (long)min(row0 + q, M - 1) * D;  // a row past M re-reads row M - 1 and stores nothing
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = cbase + 64 * i;
      v[q][i] = ld4m(x, off, c, D4, XB);
    }
    if (resid) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[q][i] += ld4m(resid, off, cbase + 64 * i, D4, false);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    gv[i] = ld4m(g, 0, c, D4, false);
  }
  float ss[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) t += sum4(v[q][i] * v[q][i]);
    ss[q] = warp_sum(t);
  }
  rms_block_sum<R, W>(ss, xs, lane, wave);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int row = row0 + q;
    if (row >= M) continue;
    const float rstd = rsqrtf(ss[q] / D + eps);
    const long off = (long)row * D;
    if (threadIdx.x == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = cbase + 64 * i;
      if (c < D4) {
        if (x_out) st4(x_out, off, c, true, v[q][i]);
        st4(y, off, c, out_f32, v[q][i] * rstd * gv[i]);
      }
    }
  }
}

// one row's loads of the backward: xh = x * rstd, dy, the residual gradient (zeros past M or past D)
template <int NV, bool DYF, bool RES>
__device__ __forceinline__ void rms_bwd_load(const void* dy, const float* x, const float* rstd, const float* dres,
                                             int row, int M, int D, int D4, int cbase, f32x4 (&xh)[NV], f32x4 (&d)[NV],
                                             f32x4 (&rv)[NV], float& rs) {
  const bool ok = row < M;  // a row past M reads row M - 1 and counts as zeros
  const long off = (long)min(row, M - 1) * D;
  rs = ok ? rstd[min(row, M - 1)] : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    xh[i] = ld4m(x, off, c, D4, false, ok) * rs;
    d[i] = ld4m(dy, off, c, D4, !DYF, ok);
    rv[i] = RES ? ld4m(dres, off, c, D4, false, ok) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// the row's dx from its finished sum; stores, and adds into the sum-dx accumulator
template <int NV>
__device__ __forceinline__ void rms_bwd_store(float cm, float rs, const f32x4 (&xh)[NV], const f32x4 (&d)[NV],
                                              const f32x4 (&rv)[NV], const f32x4 (&gv)[NV], float* dx, bf16* dx_c, long off,
                                              int D4, int cbase, f32x4 (&ao)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    if (c < D4) {
      const f32x4 o = (d[i] * gv[i] - xh[i] * cm) * rs + rv[i];
      st4(dx, off, c, true, o);
      if (dx_c) st4(dx_c, off, c, false, o);
      ao[i] += o;
    }
  }
}

// ---- backward, narrow: RMS_BWD_ROWS rows per block, one wave per row, R rows of a wave loaded together ----
// DYF: dy is fp32 (else bf16); RES: dres is given
template <int NV, bool DYF, bool RES>
__global__ void __launch_bounds__(256) rms_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ g, const float* __restrict__ rstd,
                                                      const float* dres, float* dx,
                                                      bf16* __restrict__ dx_c, float* __restrict__ part, int nslab, int M,
                                                      int D) {
  constexpr int R = NV <= 3 ? 2 : 1;  // rows in flight per wave: 3 R NV loads of 16 bytes per lane, 6 .. 24
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int D4 = D / 4;
  DTC_ASSERT(D % 4 == 0 && D4 <= NV * 64 && (long)blockIdx.x * RMS_BWD_ROWS < M && nslab >= 1 && nslab <= 2);
  f32x4 ag[NV], ao[NV], gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    ag[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    ao[i] = ag[i];
    gv[i] = ld4m(g, 0, c, D4, false);
  }
  for (int it = 0; it < RMS_BWD_ROWS / (4 * R); ++it) {
    const int r0 = blockIdx.x * RMS_BWD_ROWS + (it * 4 + wave) * R;
    f32x4 xh[R][NV], d[R][NV], rv[R][NV];
    float rs[R], s[R];
#pragma unroll
    for (int q = 0; q < R; ++q) rms_bwd_load<NV, DYF, RES>(dy, x, rstd, dres, r0 + q, M, D, D4, lane, xh[q], d[q], rv[q], rs[q]);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const f32x4 dxh = d[q][i] * xh[q][i];
        t += sum4(dxh * gv[i]);
        ag[i] += dxh;
      }
      s[q] = t;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float cm = warp_sum(s[q]) / D;
      if (r0 + q < M) rms_bwd_store<NV>(cm, rs[q], xh[q], d[q], rv[q], gv, dx, dx_c, (long)(r0 + q) * D, D4, lane, ao);
    }
  }
  // block reduce of the column partials over the 4 waves, one slab at a time through the same 4 x D floats
  __shared__ __attribute__((aligned(16))) float red[4][NV * 256];
  float* pb = part + (long)blockIdx.x * nslab * D;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s >= nslab) break;
    if (s) __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) ((f32x4*)red[wave])[lane + 64 * i] = s ? ao[i] : ag[i];
    __syncthreads();
    for (int c = threadIdx.x; c < D4; c += 256) {
      const f32x4 t = (((const f32x4*)red[0])[c] + ((const f32x4*)red[1])[c]) +
                      (((const f32x4*)red[2])[c] + ((const f32x4*)red[3])[c]);
      ((f32x4*)(pb + (long)s * D))[c] = t;
    }
  }
}

// ---- backward, wide: RMS_BWD_ROWS rows per block in groups of R, a row over the W waves ----
template <int NV, int W, bool DYF, bool RES>
__global__ void __launch_bounds__(64 * W) rms_bwd_wide_kernel(const void* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ g,
                                                              const float* __restrict__ rstd, const float* dres,
                                                              float* __restrict__ dx, bf16* __restrict__ dx_c,
                                                              float* __restrict__ part, int nslab, int M, int D) {
  constexpr int R = NV <= 2 ? 4 : NV == 3 ? 2 : 1;  // 3 R NV = 24, 18, 12 loads of 16 bytes in flight per lane
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int D4 = D / 4, cbase = wave * NV * 64 + lane;
  DTC_ASSERT(D % 4 == 0 && D4 <= NV * 64 * W && wave < W && nslab >= 1 && nslab <= 2 && (long)blockIdx.x * RMS_BWD_ROWS < M);
  __shared__ float xs[2][R * W];
  f32x4 ag[NV], ao[NV], gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    ag[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    ao[i] = ag[i];
    gv[i] = ld4m(g, 0, c, D4, false);
  }
  for (int it = 0; it < RMS_BWD_ROWS / R; ++it) {
    const int r0 = blockIdx.x * RMS_BWD_ROWS + it * R;  // block-uniform: every wave reaches the barrier below
    f32x4 xh[R][NV], d[R][NV], rv[R][NV];
    float rs[R], s[R];
#pragma unroll
    for (int q = 0; q < R; ++q) rms_bwd_load<NV, DYF, RES>(dy, x, rstd, dres, r0 + q, M, D, D4, cbase, xh[q], d[q], rv[q], rs[q]);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const f32x4 dxh = d[q][i] * xh[q][i];
        t += sum4(dxh * gv[i]);
        ag[i] += dxh;
      }
      s[q] = warp_sum(t);
    }
    rms_block_sum<R, W>(s, xs[it & 1], lane, wave);
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (r0 + q < M) rms_bwd_store<NV>(s[q] / D, rs[q], xh[q], d[q], rv[q], gv, dx, dx_c, (long)(r0 + q) * D, D4, cbase, ao);
  }
  // this wave's columns of the block's partial row
  float* pb = part + (long)blockIdx.x * nslab * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    if (c < D4) {
      ((f32x4*)pb)[c] = ag[i];
      if (nslab > 1) ((f32x4*)(pb + D))[c] = ao[i];
    }
  }
}

// out[c] (beta*out[c] +)= sum_p part[(p * nslab + s) * D + c], slab s = blockIdx.y -> o0 / o1: 32 columns x 8 partial
// groups per block, p ascending within a group, the groups added in order -- the TALL arithmetic of
// reduce_tasks_kernel, so the deferred path gives the same bits.
constexpr int RS_COLS = 32, RS_GROUPS = 256 / RS_COLS;
__global__ void __launch_bounds__(256) rms_slab_reduce(const float* __restrict__ part, int P, int D, int nslab,
                                                       float* __restrict__ o0, float* __restrict__ o1, float beta) {
  const int tx = threadIdx.x % RS_COLS, ty = threadIdx.x / RS_COLS;
  const int c = blockIdx.x * RS_COLS + tx;
  DTC_ASSERT(P >= 1 && (int)blockIdx.y < nslab && (long)blockIdx.x * RS_COLS < D);
  const float* src = part + (long)blockIdx.y * D;
  const long pstride = (long)nslab * D;
  float s = 0.f;
  if (c < D) {
#pragma unroll 8
    for (int p = ty; p < P; p += RS_GROUPS) s += src[(long)p * pstride + c];
  }
  __shared__ float red[RS_GROUPS][RS_COLS];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < D) {
    float u = 0.f;
#pragma unroll
    for (int gq = 0; gq < RS_GROUPS; ++gq) u += red[gq][tx];
    float* o = blockIdx.y == 0 ? o0 : o1;
    o[c] = beta != 0.f ? beta * o[c] + u : u;
  }
}

}  // namespace

#define RMS_NV_CASE(N_, ...) case N_: { constexpr int NVC = N_; __VA_ARGS__; } break;
// narrow forward: NV = ceil(D / 256) rounded up to an instantiated class, 1 .. 16
#define RMS_FWD_NV_SWITCH(NV_, ...)                                                                \
  switch ((NV_) <= 4 ? (NV_) : (NV_) <= 6 ? 6 : (NV_) <= 8 ? 8 : (NV_) <= 12 ? 12 : 16) {          \
    RMS_NV_CASE(1, __VA_ARGS__) RMS_NV_CASE(2, __VA_ARGS__) RMS_NV_CASE(3, __VA_ARGS__)            \
    RMS_NV_CASE(4, __VA_ARGS__) RMS_NV_CASE(6, __VA_ARGS__) RMS_NV_CASE(8, __VA_ARGS__)            \
    RMS_NV_CASE(12, __VA_ARGS__) RMS_NV_CASE(16, __VA_ARGS__)                                      \
    default: return 2001;                                                                          \
  }
#define RMS_BWD_NV_SWITCH(NV_, ...)                                                                \
  switch ((NV_) <= 4 ? (NV_) : 6) {                                                                \
    RMS_NV_CASE(1, __VA_ARGS__) RMS_NV_CASE(2, __VA_ARGS__) RMS_NV_CASE(3, __VA_ARGS__)            \
    RMS_NV_CASE(4, __VA_ARGS__) RMS_NV_CASE(6, __VA_ARGS__)                                        \
    default: return 2001;                                                                          \
  }

// D % 4 == 0 (16-byte chunks) and D <= 8192: the codes of the LayerNorm entry points
static inline int rms_width_error(int D) { return D <= 0 || D % 4 ? 2002 : (D > RMS_MAX_D ? 2001 : 0); }

template <bool XB>
static int rms_fwd_launch(const void* x, const float* resid, float* x_out, const float* g, void* y, float* rstd, int M,
                          int D, float eps, int out_f32, hipStream_t st) {
  if (const int e = rms_width_error(D)) return e;
  DTC_HOST_CHECK(M >= 1 && x && g && y && rstd && !(((uintptr_t)x | (uintptr_t)resid | (uintptr_t)x_out | (uintptr_t)g |
                                                      (uintptr_t)y) & 15));
  if (D <= RMS_FWD_NARROW_D) {
    const int nv = (D / 4 + 63) / 64;
    RMS_FWD_NV_SWITCH(nv, hipLaunchKernelGGL((rms_fwd_kernel<NVC, XB>), dim3((M + 3) / 4), dim3(256), 0, st, x, resid, x_out,
                                             g, y, rstd, M, D, eps, out_f32));
  } else {  // 8 waves, NV = ceil(D / 2048) = 3 or 4 chunks per lane, 4 rows per block
    const dim3 grid((M + 3) / 4), block(512);
    if (D <= 6144)
      hipLaunchKernelGGL((rms_fwd_wide_kernel<3, 8, XB>), grid, block, 0, st, x, resid, x_out, g, y, rstd, M, D, eps, out_f32);
    else
      hipLaunchKernelGGL((rms_fwd_wide_kernel<4, 8, XB>), grid, block, 0, st, x, resid, x_out, g, y, rstd, M, D, eps, out_f32);
  }
  DTC_CHECK_LAUNCH();
  return 0;
}

extern "C" {

// y = RMSNorm(x) * gamma (bf16, or fp32 with out_f32), rstd[M]
int dtc_rmsnorm_fwd(const float* x, const float* g, void* y, float* rstd, int M, int D, float eps, int out_f32,
                    hipStream_t st) {
  return rms_fwd_launch<false>(x, nullptr, nullptr, g, y, rstd, M, D, eps, out_f32, st);
}

// x_out = x + resid (fp32; x_out may alias x), then the above on x_out
int dtc_add_rmsnorm_fwd(const float* x, const float* resid, float* x_out, const float* g, void* y, float* rstd, int M,
                        int D, float eps, int out_f32, hipStream_t st) {
  if (const int e = rms_width_error(D)) return e;
  DTC_HOST_CHECK(resid && x_out);
  return rms_fwd_launch<false>(x, resid, x_out, g, y, rstd, M, D, eps, out_f32, st);
}

// x_out = float(d) + resid with d bf16 (a bf16 out_proj / fc2 output); x_out must not alias d
int dtc_add_rmsnorm_fwd_bf16(const bf16* d, const float* resid, float* x_out, const float* g, void* y, float* rstd, int M,
                             int D, float eps, int out_f32, hipStream_t st) {
  if (const int e = rms_width_error(D)) return e;
  DTC_HOST_CHECK(resid && x_out && (const void*)d != (const void*)x_out);
  return rms_fwd_launch<true>(d, resid, x_out, g, y, rstd, M, D, eps, out_f32, st);
}

// two slabs are always provided for, so the size does not depend on dbias
long dtc_rmsnorm_bwd_workspace_bytes(int M, int D) {
  return (long)((M + RMS_BWD_ROWS - 1) / RMS_BWD_ROWS) * 2 * D * 4;
}

// dx (fp32, may alias dres) [, dx_c bf16]; dg = (accumulate ? dg : 0) + sum_rows dy * xh; dbias (optional) likewise
// sum_rows dx.  defer: the partials stay in ws as [blocks][nslab][D], nslab = dbias ? 2 : 1, for the caller's reducer.
int dtc_rmsnorm_bwd(const void* dy, int dy_f32, const float* x, const float* g, const float* rstd, const float* dres,
                    float* dx, bf16* dx_c, float* dg, float* dbias, int M, int D, int accumulate, float* ws,
                    long ws_bytes, int defer, hipStream_t st) {
  if (const int e = rms_width_error(D)) return e;
  if (ws_bytes < dtc_rmsnorm_bwd_workspace_bytes(M, D)) return 2003;
  DTC_HOST_CHECK(M >= 1 && dy && x && g && rstd && dx && dg && ws &&
                 !(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)g | (uintptr_t)dres | (uintptr_t)dx | (uintptr_t)dx_c |
                    (uintptr_t)ws) & 15));
  const int blocks = (M + RMS_BWD_ROWS - 1) / RMS_BWD_ROWS;
  const int nslab = dbias ? 2 : 1;
  // the dy type and the presence of dres are compile-time: a run-time test per load breaks the load sequence up
#define RMS_BWD_GO(K_, T_, ...) \
  hipLaunchKernelGGL((K_<__VA_ARGS__>), dim3(blocks), dim3(T_), 0, st, dy, x, g, rstd, dres, dx, dx_c, ws, nslab, M, D)
#define RMS_BWD_TYPES(K_, T_, ...)                                                  \
  do {                                                                              \
    if (dy_f32) { if (dres) RMS_BWD_GO(K_, T_, __VA_ARGS__, true, true); else RMS_BWD_GO(K_, T_, __VA_ARGS__, true, false); } \
    else { if (dres) RMS_BWD_GO(K_, T_, __VA_ARGS__, false, true); else RMS_BWD_GO(K_, T_, __VA_ARGS__, false, false); }      \
  } while (0)
  if (D <= RMS_BWD_NARROW_D) {
    const int nv = (D / 4 + 63) / 64;
    RMS_BWD_NV_SWITCH(nv, RMS_BWD_TYPES(rms_bwd_kernel, 256, NVC));
  } else {
#define RMS_BWD_WIDE(NV_, W_) RMS_BWD_TYPES(rms_bwd_wide_kernel, 64 * W_, NV_, W_)
    // 4 waves up to 3072, 8 above; NV = ceil(D / (256 W)) = 2 .. 4 chunks per lane
    if (D <= 2048) RMS_BWD_WIDE(2, 4);
    else if (D <= 3072) RMS_BWD_WIDE(3, 4);
    else if (D <= 4096) RMS_BWD_WIDE(2, 8);
    else if (D <= 6144) RMS_BWD_WIDE(3, 8);
    else RMS_BWD_WIDE(4, 8);
#undef RMS_BWD_WIDE
  }
#undef RMS_BWD_TYPES
#undef RMS_BWD_GO
  DTC_CHECK_LAUNCH();
  if (defer) return 0;
  hipLaunchKernelGGL(rms_slab_reduce, dim3((D + RS_COLS - 1) / RS_COLS, nslab), dim3(256), 0, st, ws, blocks, D, nslab, dg,
                     dbias, accumulate ? 1.f : 0.f);
  DTC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
