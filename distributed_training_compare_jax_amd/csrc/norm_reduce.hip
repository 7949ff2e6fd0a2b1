// LayerNorm fwd/bwd and deterministic column reductions (bias grads, dgamma/dbeta).
//
// LayerNorm (flax nn.LayerNorm, eps 1e-6): one wave64 per row, the row held in registers as
// float4 chunks (16-byte loads), two-pass mean/variance in fp32, output in the GEMM operand
// dtype.  Backward fuses the residual-gradient add and writes a bf16 copy of dx for the next
// dgrad/wgrad GEMM; dgamma/dbeta go through per-block partial slabs + an ordered reduce (no
// float atomics -> bitwise reproducible).  Rows wider than a wave can hold (forward D > 2048, backward
// D > 1024, up to 8192) are spread over the waves of a block: the ln_*_wide kernels below.
#include "common.h"
#include "fp8_quant.h"
#include <cstdlib>

namespace {

// RPW rows per wave, every row's loads issued before the first reduction (as the backward): with one
// row per wave a wave had 3 x 16 B in flight per lane and the kernel ran at ~4 TB/s
// resid (optional): the row is x + resid (the residual add of the producing layer, moved here from its
// GEMM epilogue), written to x_out (may alias x) before it is normalised.
// XB: x is bf16 (a bf16 GEMM output; the sum x + resid is fp32 in x_out, which must not alias x)
// MX (bf16 y, D % 32 == 0; mq / msc are unused without it): the MXFP8 form of the bf16 y that is stored goes to mq / msc, the
// same bytes as the stand-alone quantiser gives on y (csrc/gemm_fp8.hip mx_quant_tasks_kernel).  A lane holds
// columns 4 (lane + 64 i) .. + 3, so a 32-column block is 8 consecutive lanes of one i (all inside or all outside
// the row: D / 4 is a multiple of 8): three xor-shuffles, one 4-byte store per lane, one scale byte per 8 lanes.
template <int NV, int RPW, bool XB = false, bool MX = false>
__global__ void __launch_bounds__(256) ln_fwd_kernel(const void* x, const float* __restrict__ resid, float* x_out,
                                                     const float* __restrict__ g,
                                                     const float* __restrict__ b, void* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     int M, int D, float eps, int out_f32, uint8_t* mq, uint8_t* msc) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (row0 >= M) return;
  DTC_ASSERT(D % 4 == 0 && D / 4 <= NV * 64);
  const int D4 = D / 4;
  f32x4 v[RPW][NV], gv[NV], bv[NV];
  // gamma/beta are issued with the row loads so their latency hides under the row reductions
#pragma unroll
  for (int q = 0; q < RPW; ++q) {
    const int row = row0 + q;
    if constexpr (XB) {
      const bf16x4* xr = (const bf16x4*)((const bf16*)x + (long)min(row, M - 1) * D);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = lane + 64 * i;
        if (c < D4) {
          const bf16x4 t = xr[c];
          v[q][i] = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
        } else {
          v[q][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    } else {
      const f32x4* xr = (const f32x4*)((const float*)x + (long)min(row, M - 1) * D);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = lane + 64 * i;
        v[q][i] = c < D4 ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (resid) {
      const f32x4* rr = (const f32x4*)(resid + (long)min(row, M - 1) * D);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = lane + 64 * i;
        if (c < D4) v[q][i] += rr[c];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    int c = lane + 64 * i;
    gv[i] = c < D4 ? ((const f32x4*)g)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    bv[i] = c < D4 ? ((const f32x4*)b)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int q = 0; q < RPW; ++q) {
    const int row = row0 + q;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += v[q][i][0] + v[q][i][1] + v[q][i][2] + v[q][i][3];
    const float mean = warp_sum(s) / D;
    float qs = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int c = lane + 64 * i;
      if (c < D4) {
        f32x4 d = v[q][i] - mean;
        qs += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
      }
    }
    const float rstd = rsqrtf(warp_sum(qs) / D + eps);
    if (row >= M) continue;
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    if (x_out) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = lane + 64 * i;
        if (c < D4) ((f32x4*)(x_out + (long)row * D))[c] = v[q][i];
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int c = lane + 64 * i;
      if (c < D4) {
        f32x4 o = (v[q][i] - mean) * rstd * gv[i] + bv[i];
        if constexpr (MX) {
          const bf16x4 ob = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
          ((bf16x4*)((bf16*)y + (long)row * D))[c] = ob;
          const float r0 = (float)ob[0], r1 = (float)ob[1], r2 = (float)ob[2], r3 = (float)ob[3];
          uint32_t mx = max(max(__float_as_uint(r0) & 0x7fffffffu, __float_as_uint(r1) & 0x7fffffffu),
                            max(__float_as_uint(r2) & 0x7fffffffu, __float_as_uint(r3) & 0x7fffffffu));
          mx = amax_xor(amax_xor(amax_xor(mx, 1), 2), 4);
          const int se = se_of_amax(mx);
          const float s = pow2_f(se);
          ((uint32_t*)(mq + (long)row * D))[c] = e4m3_pk4(r0 * s, r1 * s, r2 * s, r3 * s);
          if ((lane & 7) == 0) msc[(long)row * (D >> 5) + (c >> 3)] = (uint8_t)(127 - se);
        } else {
          if (out_f32) ((f32x4*)((float*)y + (long)row * D))[c] = o;
          else ((bf16x4*)((bf16*)y + (long)row * D))[c] = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
        }
      }
    }
  }
}

#ifndef DTC_LN_RPW
#define DTC_LN_RPW 2  // rows per wave in the LayerNorm backward (all loaded before the first use)
#endif
constexpr int LN_RPW = DTC_LN_RPW;
constexpr int LN_BWD_ROWS = 4 * LN_RPW;  // rows per block (4 waves): 512 blocks at M=4096 with 2 rows per wave

// LayerNorm backward, 2 rows per wave with all loads issued before the two row reductions (ILP),
// fused residual-gradient add, bf16 copy of dx, and per-block column partials of
//   slab 0: sum dy*xhat (dgamma)   slab 1: sum dy (dbeta)   slab 2: sum dx (the bias grad of the
//   layer whose OUTPUT gradient dx is: out_proj.b / fc2.b — saves a separate colsum pass)
template <int NV>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const void* __restrict__ dy, int dy_f32, const float* __restrict__ x,
                                                     const float* __restrict__ g, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dres,
                                                     float* __restrict__ dx, bf16* __restrict__ dx_c,
                                                     float* __restrict__ part, int nslab, int M, int D, int iters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D4 = D / 4;
  f32x4 ag[NV], ab[NV], ao[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { ag[i] = f32x4{0.f, 0.f, 0.f, 0.f}; ab[i] = ag[i]; ao[i] = ag[i]; }
  DTC_ASSERT(D % 4 == 0 && D / 4 <= NV * 64 && (long)blockIdx.x * LN_BWD_ROWS * iters < M + LN_BWD_ROWS * iters);
  f32x4 gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    gv[i] = c < D4 ? ((const f32x4*)g)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // iters row groups per block (one partial row per block: fewer partials for the column reduction)
  for (int it = 0; it < iters; ++it) {
  const int r0 = (blockIdx.x * iters + it) * LN_BWD_ROWS + wave * LN_RPW;
  f32x4 xh[LN_RPW][NV], d[LN_RPW][NV], rv[LN_RPW][NV];
  float s1[LN_RPW] = {}, s2[LN_RPW] = {}, rsv[LN_RPW] = {};
  // every global load of the row group (x, dy, the residual gradient) is issued before the first
  // use: the residual-gradient read used to sit after the row reductions, fully exposed
#pragma unroll
  for (int q = 0; q < LN_RPW; ++q) {
    const int row = r0 + q;
    const bool ok = row < M;
    const float mu = ok ? mean[row] : 0.f;
    rsv[q] = ok ? rstd[row] : 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f}, rr = {0.f, 0.f, 0.f, 0.f};
      if (ok && c < D4) {
        xv = ((const f32x4*)(x + (long)row * D))[c];
        if (dy_f32) dv = ((const f32x4*)((const float*)dy + (long)row * D))[c];
        else { bf16x4 t = ((const bf16x4*)((const bf16*)dy + (long)row * D))[c]; dv = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]}; }
        if (dres) rr = ((const f32x4*)(dres + (long)row * D))[c];
      }
      xh[q][i] = (xv - mu) * rsv[q];
      d[q][i] = dv;
      rv[q][i] = rr;
    }
  }
#pragma unroll
  for (int q = 0; q < LN_RPW; ++q)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) {
        f32x4 gd = d[q][i] * gv[i];
        s1[q] += gd[0] + gd[1] + gd[2] + gd[3];
        f32x4 t2 = gd * xh[q][i];
        s2[q] += t2[0] + t2[1] + t2[2] + t2[3];
        ag[i] += d[q][i] * xh[q][i];
        ab[i] += d[q][i];
      }
    }
#pragma unroll
  for (int q = 0; q < LN_RPW; ++q) {
    const int row = r0 + q;
    const float c1 = warp_sum(s1[q]) / D, c2 = warp_sum(s2[q]) / D;
    if (row >= M) continue;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) {
        f32x4 gd = d[q][i] * gv[i];
        f32x4 o = (gd - c1 - xh[q][i] * c2) * rsv[q];
        if (dres) o += rv[q][i];
        ((f32x4*)(dx + (long)row * D))[c] = o;
        if (dx_c) ((bf16x4*)(dx_c + (long)row * D))[c] = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
        ao[i] += o;
      }
    }
  }
  }  // row groups
  // block reduce of the column partials over the 4 waves (fixed order); part[block][nslab][D]
  __shared__ __attribute__((aligned(16))) float red[4][3][NV * 256];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    ((f32x4*)red[wave][0])[c] = ag[i];
    ((f32x4*)red[wave][1])[c] = ab[i];
    ((f32x4*)red[wave][2])[c] = ao[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (s >= nslab) break;
      const float v = (red[0][s][c] + red[1][s][c]) + (red[2][s][c] + red[3][s][c]);
      part[((long)blockIdx.x * nslab + s) * D + c] = v;
    }
  }
}

// ---- wide rows: forward 2048 < D <= 8192, backward 1024 < D <= 8192 ----
// A row no longer fits one wave's registers next to gamma / the column accumulators, so the W waves of a
// block (4 up to D 4096, 8 above: at most 4 f32x4 per lane either way) each own a contiguous 1/W of the
// columns (NV f32x4 per lane, chunk wave*NV*64 + lane + 64*i, NV = ceil(D / (256 W))) and walk the SAME rows.
// Row sums: each wave reduces its share (warp_sum), the W wave sums meet in a few floats of LDS and every
// wave adds them in one fixed pairwise order: one barrier per exchange, the LDS buffer alternating between
// row groups so no second barrier is needed.  The column partials of the backward are exclusive to the
// owning wave and go straight to the slab: no block reduction, no LDS beyond the exchange (<= 512 B).
constexpr int LNW_MAX_D = 8192;
// rows per group: a lane has 6-8 (fwd) / 18-24 (bwd) 16-byte loads in flight per group, as the narrow kernels
// have at their widest
__host__ __device__ constexpr int lnw_rows(int NV) { return NV <= 2 ? 4 : 2; }

// sum over the block's W waves of a per-wave value, R values at once; buf is [R][W] floats of LDS
template <int R, int W>
__device__ __forceinline__ void lnw_block_sum(float (&v)[R], float* buf, int lane, int wave) {
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

// one group of R rows per block; same two-pass statistics, residual add and outputs as ln_fwd_kernel
template <int NV, int W, bool XB>
__global__ void __launch_bounds__(64 * W) ln_fwd_wide_kernel(const void* x, const float* __restrict__ resid, float* x_out,
                                                          const float* __restrict__ g, const float* __restrict__ b,
                                                          void* __restrict__ y, float* __restrict__ mean_out,
                                                          float* __restrict__ rstd_out, int M, int D, float eps,
                                                          int out_f32) {
  constexpr int R = lnw_rows(NV);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * R;
  const int D4 = D / 4, cbase = wave * NV * 64 + lane;
  DTC_ASSERT(D % 4 == 0 && D4 <= NV * 64 * W && row0 < M && wave < W && cbase + 64 * (NV - 1) < NV * 64 * W);
  __shared__ float xs[2][R * W];
  f32x4 v[R][NV], gv[NV], bv[NV];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const long off = (long)min(row0 + q, M - 1) * D;  // a row past M re-reads row M-1 and stores nothing
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = cbase + 64 * i;
      if (c < D4) {
        if constexpr (XB) {
          const bf16x4 t = ((const bf16x4*)((const bf16*)x + off))[c];
          v[q][i] = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
        } else {
          v[q][i] = ((const f32x4*)((const float*)x + off))[c];
        }
      } else {
        v[q][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (resid) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = cbase + 64 * i;
        if (c < D4) v[q][i] += ((const f32x4*)(resid + off))[c];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    gv[i] = c < D4 ? ((const f32x4*)g)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    bv[i] = c < D4 ? ((const f32x4*)b)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float s[R], qs[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) t += v[q][i][0] + v[q][i][1] + v[q][i][2] + v[q][i][3];
    s[q] = warp_sum(t);
  }
  lnw_block_sum<R, W>(s, xs[0], lane, wave);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    s[q] = s[q] / D;  // the mean
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (cbase + 64 * i < D4) {
        f32x4 d = v[q][i] - s[q];
        t += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
      }
    }
    qs[q] = warp_sum(t);
  }
  lnw_block_sum<R, W>(qs, xs[1], lane, wave);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int row = row0 + q;
    const float mean = s[q], rstd = rsqrtf(qs[q] / D + eps);
    if (row >= M) continue;
    if (threadIdx.x == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    if (x_out) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = cbase + 64 * i;
        if (c < D4) ((f32x4*)(x_out + (long)row * D))[c] = v[q][i];
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = cbase + 64 * i;
      if (c < D4) {
        f32x4 o = (v[q][i] - mean) * rstd * gv[i] + bv[i];
        if (out_f32) ((f32x4*)((float*)y + (long)row * D))[c] = o;
        else ((bf16x4*)((bf16*)y + (long)row * D))[c] = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
      }
    }
  }
}

// `groups` row groups of R rows per block (R * groups = the narrow kernel's rows per block, so the partial
// slab has the same [blocks][nslab][D] shape); same slabs and outputs as ln_bwd_kernel
template <int NV, int W>
__global__ void __launch_bounds__(64 * W) ln_bwd_wide_kernel(const void* __restrict__ dy, int dy_f32, const float* __restrict__ x,
                                                          const float* __restrict__ g, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ dres,
                                                          float* __restrict__ dx, bf16* __restrict__ dx_c,
                                                          float* __restrict__ part, int nslab, int M, int D, int groups) {
  constexpr int R = lnw_rows(NV);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D4 = D / 4, cbase = wave * NV * 64 + lane;
  DTC_ASSERT(D % 4 == 0 && D4 <= NV * 64 * W && wave < W && cbase + 64 * (NV - 1) < NV * 64 * W && nslab >= 2 && nslab <= 3 &&
             (long)blockIdx.x * R * groups < M);
  __shared__ float xs[2][2 * R * W];
  f32x4 ag[NV], ab[NV], ao[NV], gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ag[i] = f32x4{0.f, 0.f, 0.f, 0.f}; ab[i] = ag[i]; ao[i] = ag[i];
    const int c = cbase + 64 * i;
    gv[i] = c < D4 ? ((const f32x4*)g)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int it = 0; it < groups; ++it) {
    const int r0 = (blockIdx.x * groups + it) * R;  // block-uniform: every wave reaches the barrier below
    f32x4 xh[R][NV], d[R][NV], rv[R][NV];
    float ss[2 * R], rsv[R];
    // every global load of the row group is issued before the first reduction
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = r0 + q;
      const bool ok = row < M;
      const float mu = ok ? mean[row] : 0.f;
      rsv[q] = ok ? rstd[row] : 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = cbase + 64 * i;
        f32x4 xv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f}, rr = {0.f, 0.f, 0.f, 0.f};
        if (ok && c < D4) {
          xv = ((const f32x4*)(x + (long)row * D))[c];
          if (dy_f32) dv = ((const f32x4*)((const float*)dy + (long)row * D))[c];
          else { bf16x4 t = ((const bf16x4*)((const bf16*)dy + (long)row * D))[c]; dv = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]}; }
          if (dres) rr = ((const f32x4*)(dres + (long)row * D))[c];
        }
        xh[q][i] = (xv - mu) * rsv[q];
        d[q][i] = dv;
        rv[q][i] = rr;
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (cbase + 64 * i < D4) {
          f32x4 gd = d[q][i] * gv[i];
          s1 += gd[0] + gd[1] + gd[2] + gd[3];
          f32x4 t2 = gd * xh[q][i];
          s2 += t2[0] + t2[1] + t2[2] + t2[3];
          ag[i] += d[q][i] * xh[q][i];
          ab[i] += d[q][i];
        }
      }
      ss[2 * q] = warp_sum(s1);
      ss[2 * q + 1] = warp_sum(s2);
    }
    lnw_block_sum<2 * R, W>(ss, xs[it & 1], lane, wave);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = r0 + q;
      const float c1 = ss[2 * q] / D, c2 = ss[2 * q + 1] / D;
      if (row >= M) continue;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = cbase + 64 * i;
        if (c < D4) {
          f32x4 gd = d[q][i] * gv[i];
          f32x4 o = (gd - c1 - xh[q][i] * c2) * rsv[q];
          if (dres) o += rv[q][i];
          ((f32x4*)(dx + (long)row * D))[c] = o;
          if (dx_c) ((bf16x4*)(dx_c + (long)row * D))[c] = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
          ao[i] += o;
        }
      }
    }
  }  // row groups
  // this wave's columns of the block's partial row: part[block][nslab][D]
  float* pb = part + (long)blockIdx.x * nslab * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = cbase + 64 * i;
    if (c < D4) {
      ((f32x4*)pb)[c] = ag[i];
      ((f32x4*)(pb + D))[c] = ab[i];
      if (nslab > 2) ((f32x4*)(pb + 2 * (long)D))[c] = ao[i];
    }
  }
}

// out (beta*out +)= sum_p part[p*C + c], c in [0, C), the C columns cut into segments of `seg`
// columns routed to o0 / o1 / o2.  Block = 32 columns x 8 partial groups (whole 128-B row segments; 16
// columns read half lines), LDS tree over the groups — deterministic order, P/8 loads per thread, 8 in
// flight.  The batched TALL reduction (reduce_tasks_kernel) uses the same scheme: both paths stay bitwise
// equal.
constexpr int SR_COLS = 32, SR_GROUPS = 256 / SR_COLS;
__global__ void __launch_bounds__(256) slab_reduce(const float* __restrict__ part, int P, int C, float* __restrict__ o0,
                                                   float* __restrict__ o1, float* __restrict__ o2, int seg, float beta) {
  const int tx = threadIdx.x % SR_COLS, ty = threadIdx.x / SR_COLS;
  const int c = blockIdx.x * SR_COLS + tx;
  DTC_ASSERT(P >= 1 && ty < SR_GROUPS && (long)blockIdx.x * SR_COLS < C);
  float s = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int p = ty; p < P; p += SR_GROUPS) s += part[(long)p * C + c];
  }
  __shared__ float red[SR_GROUPS][SR_COLS];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int gq = 0; gq < SR_GROUPS; ++gq) t += red[gq][tx];
    const int which = c / seg, col = c % seg;
    float* o = which == 0 ? o0 : (which == 1 ? o1 : o2);
    o[col] = beta != 0.f ? beta * o[col] + t : t;
  }
}

constexpr int CS_ROWS = 32;  // rows per stage-1 slab

// stage 1: part[slab][n] = sum over the slab's rows.  Block = 64 column-threads (4 columns each,
// vector loads) x 4 row groups of CS_ROWS/4 rows, LDS combine of the groups.
__global__ void __launch_bounds__(256) colsum_stage1(const void* __restrict__ dy, int is_f32, int M, int N, long ld,
                                                     float* __restrict__ part) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int n = (blockIdx.x * 64 + tx) * 4;
  const int r0 = blockIdx.y * CS_ROWS + ty * (CS_ROWS / 4);
  DTC_ASSERT((long)blockIdx.y * CS_ROWS < M && ld >= N && ld % 4 == 0);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (n < N) {
    if (n + 4 <= N) {
#pragma unroll
      for (int i = 0; i < CS_ROWS / 4; ++i) {
        const int r = r0 + i;
        if (r < M) {
          if (is_f32) s += *(const f32x4*)((const float*)dy + (long)r * ld + n);
          else { bf16x4 t = *(const bf16x4*)((const bf16*)dy + (long)r * ld + n); s += f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]}; }
        }
      }
    } else {
      for (int i = 0; i < CS_ROWS / 4; ++i) {
        const int r = r0 + i;
        if (r < M)
          for (int j = 0; j < 4 && n + j < N; ++j)
            s[j] += is_f32 ? ((const float*)dy)[(long)r * ld + n + j] : (float)((const bf16*)dy)[(long)r * ld + n + j];
      }
    }
  }
  __shared__ f32x4 red[4][64];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && n < N) {
    f32x4 t = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    float* o = part + (long)blockIdx.y * N + n;
    if (n + 4 <= N) *(f32x4*)o = t;
    else for (int j = 0; j < 4 && n + j < N; ++j) o[j] = t[j];
  }
}

// One launch for a whole backward layer's deferred reductions (split-K weight-gradient slabs,
// LayerNorm dgamma/dbeta partials, bias column partials) and grad-norm partials.  Each per-op
// reduce kernel it replaces is tiny, so its cost was the ~5 us per-launch floor of a replayed
// graph node, paid ~9 times per layer.  Every output element is summed by one thread in a fixed
// partial order (p ascending), so results are bitwise reproducible and equal the per-op path.
//  WIDE  (few partials, many columns; split-K slabs): 1024 columns per block, f32x4 per thread.
//  TALL  (many partials, few columns; LN / colsum partials): 32 columns x 8 partial groups per
//        block, fixed-order LDS combine (the slab_reduce scheme).
//  SUMSQ (grad-norm chunk): part[b] = weight * sum x^2 over a grid-stride share of the range.
__global__ void __launch_bounds__(256) reduce_tasks_kernel(RedBatch batch) {
  // task of this block: binary search over the ascending blk0 (a linear scan cost up to 47 dependent scalar
  // loads of the kernel argument per block: 18 us for a launch of 48 one-block norm chunks)
  int t = 0, hi = batch.ntasks - 1;
  while (t < hi) {
    const int mid = (t + hi + 1) >> 1;
    if ((int)blockIdx.x >= batch.t[mid].blk0) t = mid;
    else hi = mid - 1;
  }
  const RedTask& T = batch.t[t];
  const int b = blockIdx.x - T.blk0;
  DTC_ASSERT(t < batch.ntasks && b >= 0 && b < T.nblk && (int)blockIdx.x < batch.nblocks);
  DTC_ASSERT(T.mode == RED_SUMSQ ? (T.part != nullptr) : (T.dst != nullptr && T.P >= 1));
  const int tid = threadIdx.x;
  if (T.mode == RED_WIDE) {
    const long c = ((long)b * 256 + tid) * 4;
    if (c >= T.C) return;
    if (c + 4 <= T.C) {
      f32x4 s = *(const f32x4*)(T.src + c);
      for (int p = 1; p < T.P; ++p) s += *(const f32x4*)(T.src + (long)p * T.pstride + c);
      f32x4* o = (f32x4*)(T.dst + c);
      if (T.beta != 0.f) s += T.beta * *o;
      *o = s;
    } else {
      for (long cc = c; cc < T.C; ++cc) {
        float s = T.src[cc];
        for (int p = 1; p < T.P; ++p) s += T.src[(long)p * T.pstride + cc];
        T.dst[cc] = T.beta != 0.f ? T.beta * T.dst[cc] + s : s;
      }
    }
  } else if (T.mode == RED_TALL) {
    const int tx = tid % SR_COLS, ty = tid / SR_COLS;
    const long c = (long)b * SR_COLS + tx;
    float s = 0.f;
    if (c < T.C) {
#pragma unroll 8
      for (int p = ty; p < T.P; p += SR_GROUPS) s += T.src[(long)p * T.pstride + c];
    }
    __shared__ float red[SR_GROUPS][SR_COLS];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < T.C) {
      float u = 0.f;
#pragma unroll
      for (int gq = 0; gq < SR_GROUPS; ++gq) u += red[gq][tx];
      T.dst[c] = T.beta != 0.f ? T.beta * T.dst[c] + u : u;
    }
  } else {
    float acc = 0.f;
    const long n4 = T.C / 4, stride = (long)T.nblk * 256;
    const f32x4* x4 = (const f32x4*)T.src;
    long i = (long)b * 256 + tid;
    for (; i + 3 * stride < n4; i += 4 * stride) {  // 4 independent 16-B loads in flight
      f32x4 v0 = x4[i], v1 = x4[i + stride], v2 = x4[i + 2 * stride], v3 = x4[i + 3 * stride];
      f32x4 q = v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
      acc += (q[0] + q[1]) + (q[2] + q[3]);
    }
    for (; i < n4; i += stride) { f32x4 v = x4[i] * x4[i]; acc += (v[0] + v[1]) + (v[2] + v[3]); }
    if (b == 0)
      for (long i = n4 * 4 + tid; i < T.C; i += 256) acc += T.src[i] * T.src[i];
    acc = warp_sum(acc);
    __shared__ float wred[4];
    if ((tid & 63) == 0) wred[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) T.part[b] = T.weight * ((wred[0] + wred[1]) + (wred[2] + wred[3]));
  }
}

}  // namespace

#define DTC_NV_SWITCH(NV_, ...)                                              \
  switch (NV_) {                                                             \
    case 1: { constexpr int NVC = 1; __VA_ARGS__; } break;                   \
    case 2: { constexpr int NVC = 2; __VA_ARGS__; } break;                   \
    case 3: { constexpr int NVC = 3; __VA_ARGS__; } break;                   \
    case 4: { constexpr int NVC = 4; __VA_ARGS__; } break;                   \
    case 5: case 6: { constexpr int NVC = 6; __VA_ARGS__; } break;           \
    case 7: case 8: { constexpr int NVC = 8; __VA_ARGS__; } break;           \
    default: return 2001;                                                    \
  }

// the wide kernels: W waves per block and NV = ceil(D / (256 W)) f32x4 per lane, 2..4
#define DTC_NVW_SWITCH(D_, ...)                                                                   \
  if ((D_) <= 4096) {                                                                             \
    constexpr int WC = 4;                                                                         \
    switch (((D_) + 1023) / 1024) {                                                               \
      case 2: { constexpr int NVC = 2; __VA_ARGS__; } break;                                      \
      case 3: { constexpr int NVC = 3; __VA_ARGS__; } break;                                      \
      case 4: { constexpr int NVC = 4; __VA_ARGS__; } break;                                      \
      default: return 2001;                                                                       \
    }                                                                                             \
  } else {                                                                                        \
    constexpr int WC = 8;                                                                         \
    switch (((D_) + 2047) / 2048) {                                                               \
      case 3: { constexpr int NVC = 3; __VA_ARGS__; } break;                                      \
      case 4: { constexpr int NVC = 4; __VA_ARGS__; } break;                                      \
      default: return 2001;                                                                       \
    }                                                                                             \
  }

// LayerNorm widths: D % 4 == 0 (16-byte chunks) and D <= 8192.  The forward keeps a row per wave up to 2048
// and the backward up to 1024 (its block reduction holds 3 x 4 x D floats of LDS); wider rows take the
// kernels that spread a row over the block's waves.
constexpr int LN_FWD_NARROW_D = 2048, LN_BWD_NARROW_D = 1024;
static inline int ln_width_error(int D) { return D <= 0 || D % 4 ? 2002 : (D > LNW_MAX_D ? 2001 : 0); }

template <bool XB>
static int ln_fwd_wide_launch(const void* x, const float* resid, float* x_out, const float* g, const float* b, void* y,
                              float* mean, float* rstd, int M, int D, float eps, int out_f32, hipStream_t st) {
  DTC_NVW_SWITCH(D, hipLaunchKernelGGL((ln_fwd_wide_kernel<NVC, WC, XB>), dim3((M + lnw_rows(NVC) - 1) / lnw_rows(NVC)),
                                       dim3(64 * WC), 0, st, x, resid, x_out, g, b, y, mean, rstd, M, D, eps, out_f32));
  DTC_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int dtc_add_layernorm_fwd(const float* x, const float* resid, float* x_out, const float* g, const float* b, void* y,
                          float* mean, float* rstd, int M, int D, float eps, int out_f32, hipStream_t st) {
  if (const int e = ln_width_error(D)) return e;
  if (D > LN_FWD_NARROW_D) return ln_fwd_wide_launch<false>(x, resid, x_out, g, b, y, mean, rstd, M, D, eps, out_f32, st);
  int nv = (D / 4 + 63) / 64;
  // one row per wave (two rows per wave measured neutral on GPT-2 small, round 3: removed)
  dim3 grid((M + 3) / 4);
  DTC_NV_SWITCH(nv, hipLaunchKernelGGL((ln_fwd_kernel<NVC, 1>), grid, dim3(256), 0, st, x, resid, x_out, g, b, y, mean,
                                       rstd, M, D, eps, out_f32, (uint8_t*)nullptr, (uint8_t*)nullptr));
  DTC_CHECK_LAUNCH();
  return 0;
}

// x_out = (fp32) d + resid with d bf16 (a bf16 out_proj / fc2 output, DTC_FWD_BF16), then LayerNorm(x_out)
int dtc_add_layernorm_fwd_bf16(const bf16* d, const float* resid, float* x_out, const float* g, const float* b,
                               void* y, float* mean, float* rstd, int M, int D, float eps, int out_f32, hipStream_t st) {
  if (const int e = ln_width_error(D)) return e;
  DTC_HOST_CHECK(d && resid && x_out && (const void*)d != (const void*)x_out);
  if (D > LN_FWD_NARROW_D) return ln_fwd_wide_launch<true>(d, resid, x_out, g, b, y, mean, rstd, M, D, eps, out_f32, st);
  int nv = (D / 4 + 63) / 64;
  dim3 grid((M + 3) / 4);
  DTC_NV_SWITCH(nv, hipLaunchKernelGGL((ln_fwd_kernel<NVC, 1, true>), grid, dim3(256), 0, st, d, resid, x_out, g, b, y,
                                       mean, rstd, M, D, eps, out_f32, (uint8_t*)nullptr, (uint8_t*)nullptr));
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_layernorm_fwd(const float* x, const float* g, const float* b, void* y, float* mean, float* rstd, int M, int D,
                      float eps, int out_f32, hipStream_t st) {
  return dtc_add_layernorm_fwd(x, nullptr, nullptr, g, b, y, mean, rstd, M, D, eps, out_f32, st);
}

// The narrow forward with the MXFP8 form of its bf16 y as a further output (mq e4m3 [M][D], msc E8M0 [M][D / 32]).
// x_bf16 = 0: x fp32, resid / x_out optional (x_out may alias x); 1: x bf16, resid and x_out required (the bf16
// branch of the add-LayerNorm).  D % 32 == 0 and D <= 2048: wider rows have no fused form (error 2003).
int dtc_layernorm_fwd_mx(const void* x, int x_bf16, const float* resid, float* x_out, const float* g, const float* b,
                         void* y, float* mean, float* rstd, int M, int D, float eps, uint8_t* mq, uint8_t* msc,
                         hipStream_t st) {
  if (const int e = ln_width_error(D)) return e;
  if (D > LN_FWD_NARROW_D || D % 32) return 2003;
  DTC_HOST_CHECK(M >= 1 && x && y && mq && msc && ((uintptr_t)mq & 3) == 0);
  DTC_HOST_CHECK(!x_bf16 || (resid && x_out && (const void*)x != (const void*)x_out));
  int nv = (D / 4 + 63) / 64;
  dim3 grid((M + 3) / 4);
  if (x_bf16) {
    DTC_NV_SWITCH(nv, hipLaunchKernelGGL((ln_fwd_kernel<NVC, 1, true, true>), grid, dim3(256), 0, st, x, resid, x_out, g,
                                         b, y, mean, rstd, M, D, eps, 0, mq, msc));
  } else {
    DTC_NV_SWITCH(nv, hipLaunchKernelGGL((ln_fwd_kernel<NVC, 1, false, true>), grid, dim3(256), 0, st, x, resid, x_out,
                                         g, b, y, mean, rstd, M, D, eps, 0, mq, msc));
  }
  DTC_CHECK_LAUNCH();
  return 0;
}

// DTC_LN_BWD_ITER: row groups of LN_BWD_ROWS per block.  2 (512 blocks at 8192 rows): half the partial
// rows for the batched column reduction -- GPT-2 small step 11.22-11.24 vs 11.31-11.34 ms with 1,
// 11.25-11.29 with 4 (profiles/r4_ab_ln_bwd_iter.log)
static int ln_bwd_iters() {
  static const int v = [] { const char* e = getenv("DTC_LN_BWD_ITER"); return e ? std::max(1, atoi(e)) : 2; }();
  return v;
}

long dtc_layernorm_bwd_workspace_bytes(int M, int D) {
  const int rows = LN_BWD_ROWS * ln_bwd_iters();
  long blocks = (M + rows - 1) / rows;
  return blocks * 3 * D * 4;
}

int dtc_layernorm_bwd(const void* dy, int dy_f32, const float* x, const float* g, const float* mean, const float* rstd,
                      const float* dres, float* dx, bf16* dx_c, float* dg, float* db, float* dbias, int M, int D,
                      int accumulate, float* ws, long ws_bytes, int defer, hipStream_t st) {
  if (const int e = ln_width_error(D)) return e;  // D % 4 == 0 and D <= 8192 (see ln_width_error)
  const int iters = ln_bwd_iters();
  int blocks = (M + LN_BWD_ROWS * iters - 1) / (LN_BWD_ROWS * iters);
  if (ws_bytes < dtc_layernorm_bwd_workspace_bytes(M, D)) return 2003;
  const int nslab = dbias ? 3 : 2;
  if (D > LN_BWD_NARROW_D) {
    // same rows per block as the narrow kernel (LN_BWD_ROWS * iters, a multiple of every lnw_rows), so the
    // partials are [blocks][nslab][D] with the same `blocks` and dtc_layernorm_bwd_workspace_bytes holds
    static_assert(LN_BWD_ROWS % 4 == 0, "lnw_rows must divide the rows per block");
    DTC_HOST_CHECK(((uintptr_t)ws & 15) == 0);  // the partial rows are stored as f32x4
    DTC_NVW_SWITCH(D, hipLaunchKernelGGL((ln_bwd_wide_kernel<NVC, WC>), dim3(blocks), dim3(64 * WC), 0, st, dy, dy_f32, x, g,
                                         mean, rstd, dres, dx, dx_c, ws, nslab, M, D, LN_BWD_ROWS * iters / lnw_rows(NVC)));
  } else {
    int nv = (D / 4 + 63) / 64;
    DTC_NV_SWITCH(nv, hipLaunchKernelGGL(ln_bwd_kernel<NVC>, dim3(blocks), dim3(256), 0, st, dy, dy_f32, x, g, mean, rstd,
                                         dres, dx, dx_c, ws, nslab, M, D, iters));
  }
  DTC_CHECK_LAUNCH();
  if (defer) return 0;  // partials stay in ws: [blocks][nslab][D] (a RED_TALL task per slab)
  hipLaunchKernelGGL(slab_reduce, dim3((nslab * D + SR_COLS - 1) / SR_COLS), dim3(256), 0, st, ws, blocks, nslab * D, dg, db, dbias,
                     D, accumulate ? 1.f : 0.f);
  DTC_CHECK_LAUNCH();
  return 0;
}

long dtc_colsum_workspace_bytes(int M, int N) { return (long)((M + CS_ROWS - 1) / CS_ROWS) * N * 4; }

int dtc_colsum(const void* dy, int is_f32, int M, int N, long ld, float* out, float beta, float* ws, long ws_bytes,
               int defer, hipStream_t st) {
  int P = (M + CS_ROWS - 1) / CS_ROWS;
  if (ws_bytes < dtc_colsum_workspace_bytes(M, N)) return 2004;
  if (ld % 4) return 2005;
  dim3 g1((N + 255) / 256, P);
  hipLaunchKernelGGL(colsum_stage1, g1, dim3(256), 0, st, dy, is_f32, M, N, ld, ws);
  DTC_CHECK_LAUNCH();
  if (defer) return 0;  // partials stay in ws: [P][N]
  hipLaunchKernelGGL(slab_reduce, dim3((N + SR_COLS - 1) / SR_COLS), dim3(256), 0, st, ws, P, N, out, out, out, N, beta);
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_red_max_tasks() { return RED_MAX_TASKS; }
int dtc_red_task_bytes() { return (int)sizeof(RedTask); }

int dtc_reduce_tasks(const RedBatch* b, hipStream_t st) {
  if (b->ntasks <= 0) return 0;
  if (b->ntasks > RED_MAX_TASKS) return 2010;
  hipLaunchKernelGGL(reduce_tasks_kernel, dim3(b->nblocks), dim3(256), 0, st, *b);
  DTC_CHECK_LAUNCH();
  return 0;
}

// generic ordered reduction of fp32 partial slabs: out (beta*out +) sum_p part[p][c]
int dtc_slab_reduce(const float* part, int P, int C, float* out, float beta, hipStream_t st) {
  hipLaunchKernelGGL(slab_reduce, dim3((C + SR_COLS - 1) / SR_COLS), dim3(256), 0, st, part, P, C, out, out, out, C, beta);
  DTC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
