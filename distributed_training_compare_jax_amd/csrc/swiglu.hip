// SwiGLU MLP (ModelConfig.mlp: swiglu) for gfx950: the gated fc1 forward and the fc2 dgrad with the gate backward,
// each one bf16 MFMA GEMM launch, plus the elementwise pair that serves what the fused kernels do not take.
//
//   forward   g = x.Wg^T + bg,  u = x.Wu^T + bu,  h = silu(g) * u          fc1.w = [Wg ; Wu] is [2F, D]
//   backward  dh = dy.W2,  dg = dh * u * s (1 + g (1 - s)),  du = dh * g * s,  s = sigmoid(g)
//
// glu_fwd_kernel / glu_bwd_kernel share one body (glu_body<BWD>):
//  * A block of 256 threads (4 waves, 2x2) owns BM = 128 token rows and TWO panels of BH = 64 weight rows.  Forward:
//    the panels are rows [n0, n0+64) and [F+n0, F+n0+64) of fc1.w, the gate and the up projection of the SAME 64
//    hidden units, so g and u of an element meet in one lane and h needs no second pass.  Backward: rows
//    [n0, n0+64) and [n0+64, n0+128) of the transposed fc2 mirror [F, D], 128 hidden units of dh.
//  * A wave holds 64 rows x 32 hidden units of both panels: two sets of 2x4 accumulators (16x16x32 bf16 MFMAs, fp32).
//    Per 32-k chunk it reads 4 A fragments and 2 + 2 B fragments from LDS and issues 16 MFMAs: every A fragment
//    feeds both panels.  As in gemm.hip the MFMA's first operand is the weight side, so a lane's 4 accumulator
//    registers are 4 CONSECUTIVE hidden units of one token row: 8-byte bf16 stores, one float4 of bias.
//  * LDS: two stages of [128 A rows | 64 + 64 B rows] x 64 k, 32 KB a stage, rows of 128 B with NO padding.  The
//    16-byte chunk c (8 k) of row r sits at chunk slot c ^ ((r >> 1) & 7).  64 banks x 4 B: a row is 32 banks, so
//    row parity picks the bank half and the slot picks 4 banks inside it.
//      - fragment read (ds_read_b128, served 16 lanes at a time): the 16 lanes are rows r0..r0+15 (r0 % 16 == 0) at
//        one chunk c: (r & 1, c ^ (r >> 1 & 7)) takes all 16 (half, slot) pairs, each bank exactly once;
//      - staging write (ds_write_b128): 16 consecutive threads are the 8 chunks of rows 2q and 2q + 1, the same
//        (r >> 1), so the 8 slots c ^ const are distinct in each half, each bank exactly once.
//    Lane group g = lane >> 4 reads chunk 4 kk + g for BOTH operands, so element j of group g is k = 8 (4 kk + g) + j
//    on either side: the products pair up whatever order the MFMA sums them in.
//  * Register-staged double buffer: the global loads (buffer loads: rows past the operand read as 0, no branch) of
//    k-step t+2 are issued before the MFMAs of step t, written to the other stage at the top of step t+1, one
//    barrier per k-step.
//  * Backward epilogue operands g, u (bf16, the accumulator layout): loaded BEFORE the main loop, guarded, into 64
//    VGPRs.  The block count per CU is set by LDS (2 x 64 KB), which leaves 256 VGPRs a lane; the forward compiles
//    to 155, the backward with them to 213, so the registers are free and the loads have the whole loop to land -- a load issued before the last
//    k-steps would need a peeled loop tail for the same effect.
//  * XCD-aware tile order (xcd_remap), M-tiles fastest: the blocks that share a weight panel share an L2.
// No atomics, no scratch, no inline assembly.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BM = 128, BH = 64, BK = 64;
constexpr int A_ELEMS = BM * BK, B_ELEMS = 2 * BH * BK, STAGE = A_ELEMS + B_ELEMS;
constexpr int PT = BM * BK / 8 / NT;  // 16-byte chunks per thread and operand (A and B tiles are both 128 rows)
static_assert(PT == 4 && 2 * BH == BM, "the staging loops assume 128-row A and B tiles");

struct GluArgs {
  const bf16* A; long lda; unsigned a_bytes;  // [M, K] activations (fwd: y2, bwd: dy)
  const bf16* B; long ldb; unsigned b_bytes;  // fwd: fc1.w [2F, K]; bwd: transposed fc2 mirror [F, K]
  int M, F, K;
  const float* bias;  // fwd: [2F] or null
  bf16* gu;           // fwd out / bwd in: [M, 2F] biased pre-activations, gate | up
  bf16* out;          // fwd: h [M, F]; bwd: dgu [M, 2F]
  int tiles_m, tiles_n;
};

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3); }

__device__ __forceinline__ float sigmoid_f(float g) {  // one v_exp_f32 + one v_rcp_f32; exp2 -> inf gives 0, -> 0 gives 1
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
}
__device__ __forceinline__ float swiglu_f(float g, float u) { return g * sigmoid_f(g) * u; }
__device__ __forceinline__ void swiglu_grad_f(float dh, float g, float u, float& dg, float& du) {
  const float s = sigmoid_f(g), gs = g * s;
  dg = dh * u * fmaf(gs, 1.f - s, s);  // s (1 + g (1 - s))
  du = dh * gs;
}

template <bool BWD>
__device__ __forceinline__ void glu_body(const GluArgs& a, bf16* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 15, lg = lane >> 4;
  const int lid = xcd_remap(blockIdx.x, a.tiles_m * a.tiles_n);
  const int m0 = (lid % a.tiles_m) * BM;
  const int n0 = (lid / a.tiles_m) * (BWD ? 2 * BH : BH);
  const int rb0 = n0, rb1 = BWD ? n0 + BH : a.F + n0;  // first weight row of the two panels
  const int nk = a.K / BK;
  DTC_ASSERT(m0 < a.M && n0 < a.F);

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, (short)0, a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)a.B, (short)0, a.b_bytes, 0x00020000);
  // thread's chunk i: tile row (tid >> 3) + 32 i, k-chunk tid & 7
  const int srow = tid >> 3, sch = tid & 7;
  int offA[PT], offB[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int r = srow + 32 * i;
    offA[i] = (int)(((long)(m0 + r) * a.lda + sch * 8) * 2);
    offB[i] = (int)(((long)((r < BH ? rb0 : rb1 - BH) + r) * a.ldb + sch * 8) * 2);
  }
  u32x4 ra[PT], rb[PT];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      ra[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, offA[i] + kt * (BK * 2), 0, 0));
      rb[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, offB[i] + kt * (BK * 2), 0, 0));
    }
  };
  auto store = [&](bf16* st) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int o = lds_off(srow + 32 * i, sch);
      *(u32x4*)(st + o) = ra[i];
      *(u32x4*)(st + A_ELEMS + o) = rb[i];
    }
  };

  f32x4 acc[2][2][4];  // [panel][hidden 16-tile][row 16-tile]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[p][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](const bf16* st) {
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 fa[4], fb[2][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) fa[j] = *(const bf16x8*)(st + lds_off(wm * 64 + j * 16 + li, kk * 4 + lg));
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          fb[p][i] = *(const bf16x8*)(st + A_ELEMS + lds_off(p * BH + wn * 32 + i * 16 + li, kk * 4 + lg));
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[p][i], fa[j], acc[p][i][j], 0, 0, 0);
    }
  };

  // lane's outputs: token row m(j), 4 consecutive hidden units from n(p, i)
  const int mrow = m0 + wm * 64 + li, ncol = n0 + wn * 32 + 4 * lg;
  const long ld2 = 2L * a.F;
  bf16x4 gpre[BWD ? 2 : 1][2][4], upre[BWD ? 2 : 1][2][4];
  f32x4 bg[2], bu[2];
  if constexpr (BWD) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = mrow + j * 16, n = ncol + p * BH + i * 16;
          const bool ok = m < a.M && n < a.F;
          const bf16* src = a.gu + (long)m * ld2 + n;
          gpre[p][i][j] = ok ? *(const bf16x4*)src : bf16x4{};
          upre[p][i][j] = ok ? *(const bf16x4*)(src + a.F) : bf16x4{};
        }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bg[i] = a.bias ? *(const f32x4*)(a.bias + ncol + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
      bu[i] = a.bias ? *(const f32x4*)(a.bias + a.F + ncol + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  bf16* const s0 = smem;
  bf16* const s1 = smem + STAGE;
  load(0);
  store(s0);
  if (nk > 1) load(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    bf16* cur = (kt & 1) ? s1 : s0;
    if (kt + 1 < nk) {
      store((kt & 1) ? s0 : s1);  // last read before the previous barrier
      if (kt + 2 < nk) load(kt + 2);
    }
    compute(cur);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = mrow + j * 16;
      if (m >= a.M) continue;
      if constexpr (!BWD) {
        const int n = ncol + i * 16;
        bf16x4 og, ou, oh;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = acc[0][i][j][r] + bg[i][r], u = acc[1][i][j][r] + bu[i][r];
          og[r] = f2bf(g);
          ou[r] = f2bf(u);
          oh[r] = f2bf(swiglu_f(g, u));
        }
        bf16* dst = a.gu + (long)m * ld2 + n;
        *(bf16x4*)dst = og;
        *(bf16x4*)(dst + a.F) = ou;
        *(bf16x4*)(a.out + (long)m * a.F + n) = oh;
      } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int n = ncol + p * BH + i * 16;
          if (n >= a.F) continue;  // F % 64 == 0: a panel past F is dropped whole
          bf16x4 og, ou;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float dg, du;
            swiglu_grad_f(acc[p][i][j][r], (float)gpre[p][i][j][r], (float)upre[p][i][j][r], dg, du);
            og[r] = f2bf(dg);
            ou[r] = f2bf(du);
          }
          bf16* dst = a.out + (long)m * ld2 + n;
          *(bf16x4*)dst = og;
          *(bf16x4*)(dst + a.F) = ou;
        }
      }
    }
}

__global__ void __launch_bounds__(NT, 2) glu_fwd_kernel(GluArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * STAGE];
  glu_body<false>(a, smem);
}
__global__ void __launch_bounds__(NT, 2) glu_bwd_kernel(GluArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * STAGE];
  glu_body<true>(a, smem);
}

// ---------------------------------------------------------------- elementwise pair (the unfused path)
template <typename T>
struct Vec4;
template <>
struct Vec4<float> { typedef f32x4 type; };
template <>
struct Vec4<bf16> { typedef bf16x4 type; };

// h = silu(g) * u over gu [M, 2F] (gate | up); 4 hidden units a thread (fp32: 16-byte loads and stores).  gu_out
// (optional): gu rounded to TO, what a bf16 model saves for the backward when its fc1 GEMM wrote fp32.
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) swiglu_fwd_kernel(const TI* __restrict__ gu, TO* __restrict__ gu_out,
                                                         TO* __restrict__ h, int M, int F) {
  typedef typename Vec4<TI>::type VI;
  typedef typename Vec4<TO>::type VO;
  const int fq = F >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * fq) return;
  const long m = idx / fq;
  const int n = (int)(idx - m * fq) << 2;
  const TI* src = gu + m * 2 * F + n;
  const VI g = *(const VI*)src, u = *(const VI*)(src + F);
  VO og, ou, oh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    og[r] = (TO)g[r];
    ou[r] = (TO)u[r];
    oh[r] = (TO)swiglu_f((float)g[r], (float)u[r]);
  }
  if (gu_out) {
    *(VO*)(gu_out + m * 2 * F + n) = og;
    *(VO*)(gu_out + m * 2 * F + F + n) = ou;
  }
  *(VO*)(h + m * F + n) = oh;
}

// dgu [M, 2F] from fp32 dh [M, F] and the saved gu
template <typename T>
__global__ void __launch_bounds__(256) swiglu_bwd_kernel(const float* __restrict__ dh, const T* __restrict__ gu,
                                                         T* __restrict__ dgu, int M, int F) {
  typedef typename Vec4<T>::type V;
  const int fq = F >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * fq) return;
  const long m = idx / fq;
  const int n = (int)(idx - m * fq) << 2;
  const f32x4 d = *(const f32x4*)(dh + m * F + n);
  const V g = *(const V*)(gu + m * 2 * F + n), u = *(const V*)(gu + m * 2 * F + F + n);
  V og, ou;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float dg, du;
    swiglu_grad_f(d[r], (float)g[r], (float)u[r], dg, du);
    og[r] = (T)dg;
    ou[r] = (T)du;
  }
  *(V*)(dgu + m * 2 * F + n) = og;
  *(V*)(dgu + m * 2 * F + F + n) = ou;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the fused pair's support contract (ops/swiglu.py routes everything else to the unfused path): bf16, M >= 1,
// F % BH == 0, K % 64 == 0, 16-byte aligned rows, operands whose 32-bit buffer offsets cannot wrap
int glu_fill(GluArgs& a, const void* A, long lda, const void* B, long ldb, int b_rows, int M, int F, int K, bool bwd) {
  DTC_HOST_CHECK(M >= 1 && F >= BH && F % BH == 0 && K >= BK && K % BK == 0);
  DTC_HOST_CHECK(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0 && aligned16(A) && aligned16(B));
  a.tiles_m = (M + BM - 1) / BM;
  a.tiles_n = bwd ? (F + 2 * BH - 1) / (2 * BH) : F / BH;
  // every offset the kernel forms, rows past the extent included, stays below 2^31
  DTC_HOST_CHECK((long)a.tiles_m * BM * lda * 2 < (1L << 31) && ((long)b_rows + 2 * BH) * ldb * 2 < (1L << 31));
  DTC_HOST_CHECK((long)a.tiles_m * a.tiles_n < (1L << 31));
  a.A = (const bf16*)A; a.lda = lda; a.a_bytes = (unsigned)((((long)M - 1) * lda + K) * 2);
  a.B = (const bf16*)B; a.ldb = ldb; a.b_bytes = (unsigned)((((long)b_rows - 1) * ldb + K) * 2);
  a.M = M; a.F = F; a.K = K;
  return 0;
}

}  // namespace

extern "C" {

// gu [M, 2F] = x.W^T + b (bf16), h [M, F] = silu(g) * u; x [M, K] (lda), w [2F, K] (ldb), bias fp32 [2F] or null
int dtc_glu_fwd(const void* x, long lda, const void* w, long ldb, const float* bias, void* gu, void* h, int M, int F,
                int K, void* stream) {
  GluArgs a{};
  if (int rc = glu_fill(a, x, lda, w, ldb, 2 * F, M, F, K, false)) return rc;
  DTC_HOST_CHECK(aligned16(gu) && aligned16(h) && (bias == nullptr || aligned16(bias)));
  a.bias = bias; a.gu = (bf16*)gu; a.out = (bf16*)h;
  hipLaunchKernelGGL(glu_fwd_kernel, dim3(a.tiles_m * a.tiles_n), dim3(NT), 0, (hipStream_t)stream, a);
  DTC_CHECK_LAUNCH();
  return 0;
}

// dgu [M, 2F] = silu-gate backward of dh = dy.W2; dy [M, K] (lda), w2t [F, K] (ldb) the transposed fc2 weight
int dtc_glu_bwd(const void* dy, long lda, const void* w2t, long ldb, const void* gu, void* dgu, int M, int F, int K,
                void* stream) {
  GluArgs a{};
  if (int rc = glu_fill(a, dy, lda, w2t, ldb, F, M, F, K, true)) return rc;
  DTC_HOST_CHECK(aligned16(gu) && aligned16(dgu));
  a.bias = nullptr; a.gu = (bf16*)gu; a.out = (bf16*)dgu;
  hipLaunchKernelGGL(glu_bwd_kernel, dim3(a.tiles_m * a.tiles_n), dim3(NT), 0, (hipStream_t)stream, a);
  DTC_CHECK_LAUNCH();
  return 0;
}

// mode 0: bf16 gu -> bf16 h; 1: fp32 gu -> fp32 h; 2: fp32 gu -> bf16 gu_out and bf16 h
int dtc_swiglu_fwd(const void* gu, void* gu_out, void* h, int mode, int M, int F, void* stream) {
  DTC_HOST_CHECK(M >= 1 && F >= 4 && F % 4 == 0 && aligned16(gu) && aligned16(h) && mode >= 0 && mode <= 2);
  DTC_HOST_CHECK(mode == 2 ? (gu_out != nullptr && aligned16(gu_out)) : gu_out == nullptr);
  const long n = (long)M * (F / 4);
  DTC_HOST_CHECK((n + 255) / 256 < (1L << 31));
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL((swiglu_fwd_kernel<bf16, bf16>), grid, blk, 0, s, (const bf16*)gu, (bf16*)nullptr, (bf16*)h, M, F);
  else if (mode == 1)
    hipLaunchKernelGGL((swiglu_fwd_kernel<float, float>), grid, blk, 0, s, (const float*)gu, (float*)nullptr, (float*)h, M, F);
  else
    hipLaunchKernelGGL((swiglu_fwd_kernel<float, bf16>), grid, blk, 0, s, (const float*)gu, (bf16*)gu_out, (bf16*)h, M, F);
  DTC_CHECK_LAUNCH();
  return 0;
}

// dgu (the dtype of gu: f32 = 1 fp32, 0 bf16) from fp32 dh [M, F] and gu [M, 2F]
int dtc_swiglu_bwd(const float* dh, const void* gu, void* dgu, int f32, int M, int F, void* stream) {
  DTC_HOST_CHECK(M >= 1 && F >= 4 && F % 4 == 0 && aligned16(dh) && aligned16(gu) && aligned16(dgu));
  const long n = (long)M * (F / 4);
  DTC_HOST_CHECK((n + 255) / 256 < (1L << 31));
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  hipStream_t s = (hipStream_t)stream;
  if (f32) hipLaunchKernelGGL((swiglu_bwd_kernel<float>), grid, blk, 0, s, dh, (const float*)gu, (float*)dgu, M, F);
  else hipLaunchKernelGGL((swiglu_bwd_kernel<bf16>), grid, blk, 0, s, dh, (const bf16*)gu, (bf16*)dgu, M, F);
  DTC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
