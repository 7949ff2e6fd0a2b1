// FP8 (OCP e4m3fn) forward path for gfx950: the per-tensor power-of-two quantiser and the NT GEMM on the
// block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, E8M0 scale operands fixed at 2^0).
//
//   quantiser   amax = max|x| (integer atomicMax on the bit pattern of |x|: order-independent, so bitwise
//               deterministic), s = 2^(8-e) or 2^(7-e) with e = floor(log2(amax)) so that amax*s is in (224, 448],
//               q = RNE_e4m3(x*s).  amax, s and 1/s stay on the device (docs/NUMERICS.md "FP8 forward").
//   GEMM        C[M,N] = (Aq[M,K] . Bq[N,K]^T) * (1/sa) * (1/sb) (+ epilogue), both operands K-major e4m3,
//               fp32 accumulation; K % 128 == 0, N % 16 == 0, any M >= 1.
#include "common.h"
#include "fp8_quant.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------ quantiser
// One task per tensor; blocks [blk0, blk0 + nblk) of a launch work on task t (tasks sorted by blk0), as
// reduce_tasks_kernel does.  st = {amax bit pattern, scale, 1 / scale} (uint32 / fp32 / fp32).
struct QuantTask {
  const void* src;
  uint8_t* q;
  uint32_t* st;
  long n;
  int blk0, nblk;
  int f32;  // source dtype: 0 bf16, 1 fp32
  int pad;
};
constexpr int QT_MAX = 64;  // QuantBatch is a kernel argument: 8 + 64 x 48 B < 4 KB
struct QuantBatch {
  int ntasks, nblocks;
  QuantTask t[QT_MAX];
};

__device__ __forceinline__ int quant_task_of(const QuantBatch& b, int blk) {
  int ti = 0;
  while (ti + 1 < b.ntasks && b.t[ti + 1].blk0 <= blk) ++ti;
  return ti;
}

// The scale from amax's bit pattern.  e = biased exponent - 127; amax * 2^(8-e) = 256 * mantissa is above 448
// exactly when the mantissa is above 1.75 (fraction bits > 0x600000).  The exponent of s is clamped to
// [-126, 126] so that s and 1/s are normal fp32; a subnormal amax (e < -126) lands on the upper clamp.
// (se_of_amax in csrc/fp8_quant.h is the same rule returning the exponent, for the MX quantisers.)
__device__ __forceinline__ void scale_of_amax(uint32_t bits, float& s, float& inv) {
  const int ef = (int)(bits >> 23);
  int se = 0;
  if (bits != 0u) {
    se = ef == 0 ? 126 : ((bits & 0x7fffffu) > 0x600000u ? 7 : 8) - (ef - 127);
    se = se < -126 ? -126 : (se > 126 ? 126 : se);
  }
  s = __uint_as_float((uint32_t)(127 + se) << 23);
  inv = __uint_as_float((uint32_t)(127 - se) << 23);
}

__device__ __forceinline__ void load8(const QuantTask& t, long v, float (&x)[8]) {
  if (t.f32) {
    const f32x4 a = ((const f32x4*)t.src)[2 * v], c = ((const f32x4*)t.src)[2 * v + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = a[i]; x[4 + i] = c[i]; }
  } else {
    const u32x4 a = ((const u32x4*)t.src)[v];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(a[i] << 16);
      x[2 * i + 1] = __uint_as_float(a[i] & 0xffff0000u);
    }
  }
}
__device__ __forceinline__ float load1(const QuantTask& t, long i) {
  return t.f32 ? ((const float*)t.src)[i] : (float)((const bf16*)t.src)[i];
}

__global__ void __launch_bounds__(256) amax_tasks_kernel(QuantBatch b) {
  __shared__ uint32_t red[4];
  const QuantTask& t = b.t[quant_task_of(b, blockIdx.x)];
  const int lb = blockIdx.x - t.blk0, tid = threadIdx.x;
  DTC_ASSERT(lb >= 0 && lb < t.nblk);
  const long nvec = t.n >> 3;
  uint32_t mx = 0u;
  for (long v = (long)lb * 256 + tid; v < nvec; v += (long)t.nblk * 256) {
    float x[8];
    load8(t, v, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) mx = max(mx, __float_as_uint(x[i]) & 0x7fffffffu);
  }
  if (lb == 0)
    for (long i = nvec * 8 + tid; i < t.n; i += 256) mx = max(mx, __float_as_uint(load1(t, i)) & 0x7fffffffu);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    if (mx) atomicMax(t.st, mx);  // integer max of |x| bit patterns: the order of arrival does not matter
  }
}

__global__ void __launch_bounds__(256) quant_tasks_kernel(QuantBatch b) {
  const QuantTask& t = b.t[quant_task_of(b, blockIdx.x)];
  const int lb = blockIdx.x - t.blk0, tid = threadIdx.x;
  DTC_ASSERT(lb >= 0 && lb < t.nblk);
  float s, inv;
  scale_of_amax(t.st[0], s, inv);
  if (lb == 0 && tid == 0) {
    ((float*)t.st)[1] = s;
    ((float*)t.st)[2] = inv;
  }
  const long nvec = t.n >> 3;
  for (long v = (long)lb * 256 + tid; v < nvec; v += (long)t.nblk * 256) {
    float x[8];
    load8(t, v, x);
    u32x2 o;
    o[0] = e4m3_pk2(x[0] * s, x[1] * s) | (e4m3_pk2(x[2] * s, x[3] * s) << 16);
    o[1] = e4m3_pk2(x[4] * s, x[5] * s) | (e4m3_pk2(x[6] * s, x[7] * s) << 16);
    ((u32x2*)t.q)[v] = o;
  }
  if (lb == 0)
    for (long i = nvec * 8 + tid; i < t.n; i += 256) t.q[i] = (uint8_t)(e4m3_pk2(load1(t, i) * s, 0.f) & 0xffu);
}

// ------------------------------------------------------------------------------------------------ MX quantiser
// MXFP8 (OCP microscaling): e4m3 bytes plus one E8M0 scale byte per 32 consecutive elements of a row.  A row-major
// [M, K] tensor with K % 32 == 0 is a flat run of n32 = M K / 32 blocks, block b = elements [32 b, 32 b + 32), its
// scale byte at sc[b].  Per block the per-tensor rule above: se = se_of_amax(max|x|), q = RNE_e4m3(x 2^se), stored
// scale 127 - se (the E8M0 code of the dequantisation scale 2^-se).  One pass, no state: a lane holds 8
// consecutive elements, the four lanes of a block reduce amax with two xor-shuffles.
struct MxQuantTask {
  const void* src;
  uint8_t* q;
  uint8_t* sc;
  long n32;  // blocks of 32 elements
  int blk0, nblk;
  int f32;   // source dtype: 0 bf16, 1 fp32
  int pad;
};
struct MxQuantBatch {
  int ntasks, nblocks;
  MxQuantTask t[QT_MAX];
};

__global__ void __launch_bounds__(256) mx_quant_tasks_kernel(MxQuantBatch b) {
  int ti = 0;
  while (ti + 1 < b.ntasks && b.t[ti + 1].blk0 <= (int)blockIdx.x) ++ti;
  const MxQuantTask& t = b.t[ti];
  const int lb = blockIdx.x - t.blk0, tid = threadIdx.x;
  DTC_ASSERT(lb >= 0 && lb < t.nblk);
  const long nvec = t.n32 * 4;  // a multiple of 4: the four lanes of a block are all inside or all outside
  for (long v = (long)lb * 256 + tid; v < nvec; v += (long)t.nblk * 256) {
    float x[8];
    if (t.f32) {
      const f32x4 a = ((const f32x4*)t.src)[2 * v], c = ((const f32x4*)t.src)[2 * v + 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[i] = a[i]; x[4 + i] = c[i]; }
    } else {
      const u32x4 a = ((const u32x4*)t.src)[v];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[2 * i] = __uint_as_float(a[i] << 16);
        x[2 * i + 1] = __uint_as_float(a[i] & 0xffff0000u);
      }
    }
    uint32_t mx = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) mx = max(mx, __float_as_uint(x[i]) & 0x7fffffffu);
    mx = amax_xor(amax_xor(mx, 1), 2);
    const int se = se_of_amax(mx);
    const float s = pow2_f(se);
    u32x2 o;
    o[0] = e4m3_pk4(x[0] * s, x[1] * s, x[2] * s, x[3] * s);
    o[1] = e4m3_pk4(x[4] * s, x[5] * s, x[6] * s, x[7] * s);
    ((u32x2*)t.q)[v] = o;
    if ((v & 3) == 0) t.sc[v >> 2] = (uint8_t)(127 - se);
  }
}

// ------------------------------------------------------------------------------------------------ GEMM
// Mirror of ops/fp8.py Fp8GemmArgs (keep field order and types identical).
struct Fp8GemmArgs {
  int M, N, K;
  const uint8_t* A; long lda;  // e4m3 [M][K]
  const uint8_t* B; long ldb;  // e4m3 [N][K]
  void* C; long ldc;
  int c_f32;
  int epi;                     // EPI_STORE / EPI_RESID / EPI_GELU
  const float* bias;           // fp32 [N] or null
  const float* aux; long ldaux;  // EPI_RESID: fp32 residual
  void* aux_out;               // EPI_GELU: gelu(u) (bf16, ldc)
  const float* inv_sa;         // device scalars 1/sa, 1/sb (powers of two)
  const float* inv_sb;
};

// Tile (32 TM) x 128, 256 threads = 2 x 2 waves of (16 TM) x 64, one k-step = 128 e4m3 = one 128-B row piece.
// Register-staged, two LDS buffers, one barrier per k-step: the loads of step t+1 are issued before the MFMAs of
// step t and written to the other buffer after them.
//
// LDS image: row r of a tile is 128 B = eight 16-B slots, slot c stored at c ^ ((r >> 1) & 7): the 16 rows
// of a fragment read with ds_read_b128 cover all 16 slots of two 256-B bank rows.
//
// A/B operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands, established with an exact-integer
// single-instruction probe (benchmarks/mfma_f8_map_probe.hip: A one-hot in k, B small integers that identify k and
// the column, 0 mismatches over 3 x 128 cases): lane l holds row / column l & 15, and byte j (0..31) of its eight
// dwords is k = 32 (l >> 4) + j, for A and B alike.  So a lane's fragment is the 32 contiguous bytes at k-offset
// 32 (l >> 4) of its row of a K-major operand.  That pairing is all the per-tensor kernel needs (its scales are
// equal); which k and which scale block the instruction assigns to a byte is stated at f8_frag below.  The scale
// operands must be set in every lane.
//
// How the instruction sums (benchmarks/mfma_f8_sum_probe.hip, docs/NUMERICS.md): within a 32-element block the
// products are aligned to the block's largest product exponent and cut toward zero 13 bits below it; different
// blocks do not cut each other.  Small-integer data is exact (tests B1), real data errs about 1e-5 |A|.|B| at
// K = 128, falling as 1 / sqrt(K): far above fp32 accumulation, far below the e4m3 quantisation itself (2^-4).
//
// The MFMA is issued with the operands swapped (B fragment first): D = B_tile . A_tile^T, so a lane's four
// accumulator registers are four CONSECUTIVE n of one m (C/D map: column = lane & 15 = m, row = 4 (lane >> 4)
// + reg = n) and the stores are 16 B (fp32) / 8 B (bf16) wide.
constexpr int F8_BN = 128;

template <int ROWS>
__device__ __forceinline__ void f8_load(const uint8_t* __restrict__ g, long ld, int row0, int nrows, int k0, int tid,
                                        u32x4 (&r)[ROWS / 32]) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int c = tid + 256 * i, row = c >> 3, slot = c & 7;
    const int gr = min(row0 + row, nrows - 1);  // rows past the edge re-read the last row (never stored)
    r[i] = *(const u32x4*)(g + (long)gr * ld + k0 + slot * 16);
  }
}
template <int ROWS>
__device__ __forceinline__ void f8_write(uint8_t* lds, int tid, const u32x4 (&r)[ROWS / 32]) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int c = tid + 256 * i, row = c >> 3, slot = c & 7;
    DTC_ASSERT(row < ROWS);
    *(u32x4*)(lds + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4)) = r[i];
  }
}
// MXK = false: a lane's fragment is the 32 contiguous bytes (16-B slots 2 g, 2 g + 1) of its row.  With equal
// scales any pairing of A bytes with the same B bytes gives the same products, which is all the map probe above
// can see.  Unequal block scales show which k the instruction itself assigns to a byte (the scale-block cases of
// benchmarks/mfma_f8_map_probe.hip, the mx family of benchmarks/mfma_f8_sum_probe.hip): dwords 0..3 of lane l
// are k = 16 (l >> 4) + 0..15 and dwords 4..7 are k = 64 + 16 (l >> 4) + 0..15, and the scale of the 32-element
// block b = k / 32 of row l & 15 is the byte supplied by lane 16 b + (l & 15).  MXK = true gathers in that order
// (slots g and 4 + g), so that the instruction's k is the k of the K-major operand in memory and lane l supplies
// the scale byte of block l >> 4 of its row.
template <bool MXK>
__device__ __forceinline__ i32x8 f8_frag(const uint8_t* lds, int row, int g) {
  const int sw = (row >> 1) & 7;
  const uint8_t* p = lds + row * 128;
  const u32x4 lo = *(const u32x4*)(p + (((MXK ? g : 2 * g) ^ sw) << 4));
  const u32x4 hi = *(const u32x4*)(p + (((MXK ? 4 + g : 2 * g + 1) ^ sw) << 4));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// MX (block-scaled operands, ops/mxfp8.py): lane l feeds the instruction the E8M0 scale byte of block l >> 4 of
// its fragment row for this k-step, byte kt * 4 + (l >> 4) of the row's scale row, fetched one k-step ahead like
// the operands and replicated into the four bytes of the scale register (opsel i selects byte i, opsel 0 is used:
// benchmarks/mfma_f8_map_probe.hip; the replication keeps the kernel independent of that); the epilogue's
// 1/sa 1/sb multiply drops out.
// FQ (MX, EPI_GELU, N % 32 == 0): the epilogue also emits the MX form of the bf16 gelu(u) it stores.
struct MxGemmExtra {
  const uint8_t* sa; long ldsa;  // E8M0 [M][K / 32]
  const uint8_t* sb; long ldsb;  // E8M0 [N][K / 32]
  uint8_t* gq;                   // FQ: e4m3 [M][N] of gelu(u)
  uint8_t* gsc;                  // FQ: E8M0 [M][N / 32]
};

template <int TM, int EPI, bool OUTF32, bool MX = false, bool FQ = false>
__global__ void __launch_bounds__(256) gemm_fp8_kernel(Fp8GemmArgs a, int mt, int nwg, MxGemmExtra x) {
  static_assert(!FQ || (MX && EPI == EPI_GELU && !OUTF32), "the fused MX output belongs to the MX GELU-pair epilogue");
  constexpr int BM = 32 * TM;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][(BM + F8_BN) * 128];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int mb = (id % mt) * BM, nb = (id / mt) * F8_BN;  // neighbouring ids share the weight tile
  const int M = a.M, N = a.N, nk = a.K >> 7;
  DTC_ASSERT(mb < M && nb < N);

  f32x4 acc[TM][4];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[BM / 32], rb[F8_BN / 32];
  f8_load<BM>(a.A, a.lda, mb, M, 0, tid, ra);
  f8_load<F8_BN>(a.B, a.ldb, nb, N, 0, tid, rb);
  f8_write<BM>(lds[0], tid, ra);
  f8_write<F8_BN>(lds[0] + BM * 128, tid, rb);
  __syncthreads();

  const int fr = lane & 15, fg = lane >> 4;
  // MX: the scale bytes of this lane's fragment rows (rows past the edge clamp, as the operand loads do)
  const uint8_t* psa[MX ? TM : 1];
  const uint8_t* psb[MX ? 4 : 1];
  int sca[MX ? TM : 1], scb[MX ? 4 : 1];
  if constexpr (MX) {
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      psa[m] = x.sa + (long)min(mb + wr * 16 * TM + m * 16 + fr, M - 1) * x.ldsa + fg;
      sca[m] = psa[m][0];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      psb[n] = x.sb + (long)min(nb + wc * 64 + n * 16 + fr, N - 1) * x.ldsb + fg;
      scb[n] = psb[n][0];
    }
  }
  for (int kt = 0; kt < nk; ++kt) {
    const uint8_t* cur = lds[kt & 1];
    const bool more = kt + 1 < nk;
    if (more) {
      f8_load<BM>(a.A, a.lda, mb, M, (kt + 1) << 7, tid, ra);
      f8_load<F8_BN>(a.B, a.ldb, nb, N, (kt + 1) << 7, tid, rb);
    }
    int nsa[MX ? TM : 1], nsb[MX ? 4 : 1];
    if constexpr (MX) {
      const int ko = more ? (kt + 1) * 4 : kt * 4;  // the last step re-reads its own bytes (in bounds)
#pragma unroll
      for (int m = 0; m < TM; ++m) nsa[m] = psa[m][ko];
#pragma unroll
      for (int n = 0; n < 4; ++n) nsb[n] = psb[n][ko];
    }
    i32x8 fa[TM], fb[4];
#pragma unroll
    for (int m = 0; m < TM; ++m) fa[m] = f8_frag<MX>(cur, wr * 16 * TM + m * 16 + fr, fg);
#pragma unroll
    for (int n = 0; n < 4; ++n) fb[n] = f8_frag<MX>(cur + BM * 128, wc * 64 + n * 16 + fr, fg);
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if constexpr (MX)
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[n], fa[m], acc[m][n], 0, 0, 0,
                                                                       scb[n] * 0x01010101, 0, sca[m] * 0x01010101);
        else
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[n], fa[m], acc[m][n], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                       0x7f7f7f7f);
      }
    if constexpr (MX) {
#pragma unroll
      for (int m = 0; m < TM; ++m) sca[m] = nsa[m];
#pragma unroll
      for (int n = 0; n < 4; ++n) scb[n] = nsb[n];
    }
    if (more) {
      uint8_t* nxt = lds[(kt + 1) & 1];
      f8_write<BM>(nxt, tid, ra);
      f8_write<F8_BN>(nxt + BM * 128, tid, rb);
    }
    __syncthreads();
  }

  // epilogue: lane = row m (lane & 15), four consecutive columns n = 4 (lane >> 4) + 0..3 of each 16 x 16 fragment
  float isa = 1.f, isb = 1.f;
  if constexpr (!MX) { isa = *a.inv_sa; isb = *a.inv_sb; }
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    const int row = mb + wr * 16 * TM + m * 16 + fr;
    float gq[FQ ? 4 : 1][4];  // FQ: the bf16-rounded gelu(u) of this lane's four fragments (0 where not stored)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = nb + wc * 64 + n * 16 + fg * 4;
      if constexpr (FQ) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gq[n][r] = 0.f;
      }
      if (row >= M || col >= N) continue;  // N % 16 == 0: a fragment's columns are all in or all out
      DTC_ASSERT(col + 4 <= N);
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MX) o[r] = acc[m][n][r];
        else o[r] = acc[m][n][r] * isa * isb;  // powers of two: exact
      }
      if (a.bias) {
        const f32x4 bb = *(const f32x4*)(a.bias + col);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += bb[r];
      }
      if constexpr (EPI == EPI_RESID) {
        const f32x4 rr = *(const f32x4*)(a.aux + (long)row * a.ldaux + col);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += rr[r];
      }
      if constexpr (OUTF32) {
        *(f32x4*)((float*)a.C + (long)row * a.ldc + col) = f32x4{o[0], o[1], o[2], o[3]};
      } else {
        bf16x4 gb;
        if constexpr (EPI == EPI_GELU) {  // C = gelu'(u), aux_out = gelu(u) (as csrc/gemm.hip epilogue_store)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float gv, dgv;
            gelu_tanh_and_grad_f(o[r], gv, dgv);
            o[r] = dgv;
            gb[r] = f2bf(gv);
            if constexpr (FQ) gq[n][r] = (float)gb[r];
          }
          *(bf16x4*)((bf16*)a.aux_out + (long)row * a.ldc + col) = gb;
        }
        *(bf16x4*)((bf16*)a.C + (long)row * a.ldc + col) = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
      }
    }
    if constexpr (FQ) {
      // fragments 2 h and 2 h + 1 of the four lanes l & 15, l >> 4 = 0..3 are one 32-column block of row
      // l & 15 (N % 32 == 0: a block is all in or all out); every lane takes part in the shuffles
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint32_t mx = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          mx = max(mx, max(__float_as_uint(gq[2 * h][r]) & 0x7fffffffu, __float_as_uint(gq[2 * h + 1][r]) & 0x7fffffffu));
        mx = amax_xor(amax_xor(mx, 16), 32);
        const int se = se_of_amax(mx);
        const float s = pow2_f(se);
        const int col0 = nb + wc * 64 + h * 32;
        if (row < M && col0 < N) {
          DTC_ASSERT(col0 + 32 <= N);
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            const float* g4 = gq[2 * h + f];
            *(uint32_t*)(x.gq + (long)row * N + col0 + f * 16 + fg * 4) =
                e4m3_pk4(g4[0] * s, g4[1] * s, g4[2] * s, g4[3] * s);
          }
          if (fg == 0) x.gsc[(long)row * (N >> 5) + (col0 >> 5)] = (uint8_t)(127 - se);
        }
      }
    }
  }
}


// Record of the last FP8 GEMM launch, written by the launch site (as note_launch in csrc/gemm.hip).
struct LastLaunchFp8 {
  int bm, bn, tm, epi, c_f32, blocks;
  int mx = 0;  // 0 per-tensor scales, 1 MX block scales, 2 MX with the fused MX output of gelu(u)
};
static LastLaunchFp8 g_last_fp8{};

static int fp8_cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
    return v;
  }();
  return n;
}

template <int TM, int EPI, bool OUTF32>
static int launch_fp8(const Fp8GemmArgs& a, hipStream_t st) {
  constexpr int BM = 32 * TM;
  const int mt = (a.M + BM - 1) / BM, nt = (a.N + F8_BN - 1) / F8_BN;
  const int nwg = mt * nt;
  hipLaunchKernelGGL((gemm_fp8_kernel<TM, EPI, OUTF32>), dim3(nwg), dim3(256), 0, st, a, mt, nwg, MxGemmExtra{});
  DTC_CHECK_LAUNCH();
  g_last_fp8 = LastLaunchFp8{BM, F8_BN, TM, EPI, OUTF32 ? 1 : 0, nwg};
  return 0;
}

template <int TM>
static int launch_fp8_epi(const Fp8GemmArgs& a, hipStream_t st) {
  if (a.epi == EPI_STORE) return a.c_f32 ? launch_fp8<TM, EPI_STORE, true>(a, st) : launch_fp8<TM, EPI_STORE, false>(a, st);
  if (a.epi == EPI_RESID) return launch_fp8<TM, EPI_RESID, true>(a, st);
  return launch_fp8<TM, EPI_GELU, false>(a, st);
}

template <int TM, int EPI, bool OUTF32, bool FQ>
static int launch_mxfp8(const Fp8GemmArgs& a, const MxGemmExtra& x, hipStream_t st) {
  constexpr int BM = 32 * TM;
  const int mt = (a.M + BM - 1) / BM, nt = (a.N + F8_BN - 1) / F8_BN;
  const int nwg = mt * nt;
  hipLaunchKernelGGL((gemm_fp8_kernel<TM, EPI, OUTF32, true, FQ>), dim3(nwg), dim3(256), 0, st, a, mt, nwg, x);
  DTC_CHECK_LAUNCH();
  g_last_fp8 = LastLaunchFp8{BM, F8_BN, TM, EPI, OUTF32 ? 1 : 0, nwg, FQ ? 2 : 1};
  return 0;
}

template <int TM>
static int launch_mxfp8_epi(const Fp8GemmArgs& a, const MxGemmExtra& x, hipStream_t st) {
  if (a.epi == EPI_STORE)
    return a.c_f32 ? launch_mxfp8<TM, EPI_STORE, true, false>(a, x, st) : launch_mxfp8<TM, EPI_STORE, false, false>(a, x, st);
  if (a.epi == EPI_RESID) return launch_mxfp8<TM, EPI_RESID, true, false>(a, x, st);
  return x.gq ? launch_mxfp8<TM, EPI_GELU, false, true>(a, x, st) : launch_mxfp8<TM, EPI_GELU, false, false>(a, x, st);
}

static int g_fp8_force_tm = 0;  // ops/fp8.py set_tile_m: 0 = by grid size, 64 / 128 = that tile height (A/B, tests)

extern "C" {

int dtc_qt_max() { return QT_MAX; }
int dtc_qt_task_bytes() { return (int)sizeof(QuantTask); }
int dtc_qt_batch_bytes() { return (int)sizeof(QuantBatch); }

// amax + quantise of every task: one memset of the tasks' amax words (the caller lays the st blocks of a batch
// out contiguously: st_base, st_bytes), one amax launch, one quantise launch.  Stream-ordered, capturable.
int dtc_quant_e4m3_tasks(const QuantBatch* b, void* st_base, long st_bytes, hipStream_t st) {
  DTC_HOST_CHECK(b->ntasks >= 1 && b->ntasks <= QT_MAX && b->nblocks >= b->ntasks);
  for (int i = 0; i < b->ntasks; ++i) {
    const QuantTask& t = b->t[i];
    DTC_HOST_CHECK(t.n >= 1 && t.nblk >= 1 && t.src && t.q && t.st);
    DTC_HOST_CHECK(((uintptr_t)t.src & 15) == 0 && ((uintptr_t)t.q & 7) == 0 && ((uintptr_t)t.st & 3) == 0);
    DTC_HOST_CHECK(t.blk0 == (i ? b->t[i - 1].blk0 + b->t[i - 1].nblk : 0));
    DTC_HOST_CHECK((const char*)t.st >= (const char*)st_base && (const char*)t.st + 12 <= (const char*)st_base + st_bytes);
  }
  DTC_HOST_CHECK(b->t[b->ntasks - 1].blk0 + b->t[b->ntasks - 1].nblk == b->nblocks);
  hipError_t e = hipMemsetAsync(st_base, 0, (size_t)st_bytes, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(amax_tasks_kernel, dim3(b->nblocks), dim3(256), 0, st, *b);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(quant_tasks_kernel, dim3(b->nblocks), dim3(256), 0, st, *b);
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_gemm_fp8_set_tile_m(int bm) {
  g_fp8_force_tm = bm == 128 ? 4 : (bm == 64 ? 2 : 0);
  return 0;
}

int dtc_gemm_fp8(const Fp8GemmArgs* a, hipStream_t st) {
  DTC_HOST_CHECK(a->M >= 1 && a->N >= 16 && a->K >= 128 && a->K % 128 == 0 && a->N % 16 == 0);
  DTC_HOST_CHECK(a->lda >= a->K && a->ldb >= a->K && a->lda % 16 == 0 && a->ldb % 16 == 0 && a->ldc >= a->N);
  DTC_HOST_CHECK(((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->B & 15) == 0 && ((uintptr_t)a->C & 15) == 0);
  DTC_HOST_CHECK(a->ldc % 4 == 0 && a->inv_sa && a->inv_sb);
  DTC_HOST_CHECK(a->epi == EPI_STORE || a->epi == EPI_RESID || a->epi == EPI_GELU);
  DTC_HOST_CHECK(a->epi != EPI_RESID || (a->c_f32 && a->aux && a->ldaux >= a->N && a->ldaux % 4 == 0 &&
                                         ((uintptr_t)a->aux & 15) == 0));
  DTC_HOST_CHECK(a->epi != EPI_GELU || (!a->c_f32 && a->aux_out && ((uintptr_t)a->aux_out & 7) == 0));
  DTC_HOST_CHECK(!a->bias || ((uintptr_t)a->bias & 15) == 0);
  // 128-row tiles once they fill every CU; below that 64-row tiles give twice the blocks
  const long t128 = (long)((a->M + 127) / 128) * ((a->N + F8_BN - 1) / F8_BN);
  const int tm = g_fp8_force_tm ? g_fp8_force_tm : (t128 >= fp8_cu_count() ? 4 : 2);
  return tm == 4 ? launch_fp8_epi<4>(*a, st) : launch_fp8_epi<2>(*a, st);
}

int dtc_gemm_fp8_last_launch(int* out) {
  out[0] = g_last_fp8.bm; out[1] = g_last_fp8.bn; out[2] = g_last_fp8.tm; out[3] = g_last_fp8.epi;
  out[4] = g_last_fp8.c_f32; out[5] = g_last_fp8.blocks; out[6] = g_last_fp8.mx; out[7] = 0;
  return 0;
}

int dtc_mxqt_task_bytes() { return (int)sizeof(MxQuantTask); }
int dtc_mxqt_batch_bytes() { return (int)sizeof(MxQuantBatch); }

// MX quantiser over a task table: one launch, no state.  Stream-ordered, capturable.
int dtc_quant_mxfp8_tasks(const MxQuantBatch* b, hipStream_t st) {
  DTC_HOST_CHECK(b->ntasks >= 1 && b->ntasks <= QT_MAX && b->nblocks >= b->ntasks);
  for (int i = 0; i < b->ntasks; ++i) {
    const MxQuantTask& t = b->t[i];
    DTC_HOST_CHECK(t.n32 >= 1 && t.nblk >= 1 && t.src && t.q && t.sc);
    DTC_HOST_CHECK(((uintptr_t)t.src & 15) == 0 && ((uintptr_t)t.q & 7) == 0);
    DTC_HOST_CHECK(t.blk0 == (i ? b->t[i - 1].blk0 + b->t[i - 1].nblk : 0));
  }
  DTC_HOST_CHECK(b->t[b->ntasks - 1].blk0 + b->t[b->ntasks - 1].nblk == b->nblocks);
  hipLaunchKernelGGL(mx_quant_tasks_kernel, dim3(b->nblocks), dim3(256), 0, st, *b);
  DTC_CHECK_LAUNCH();
  return 0;
}

// The MX GEMM: a's inv_sa / inv_sb are unused; x carries the operands' scale bytes and, for EPI_GELU with
// N % 32 == 0, optionally the MX output of gelu(u) (gq and gsc both set, or neither).
int dtc_gemm_mxfp8(const Fp8GemmArgs* a, const MxGemmExtra* x, hipStream_t st) {
  DTC_HOST_CHECK(a->M >= 1 && a->N >= 16 && a->K >= 128 && a->K % 128 == 0 && a->N % 16 == 0);
  DTC_HOST_CHECK(a->lda >= a->K && a->ldb >= a->K && a->lda % 16 == 0 && a->ldb % 16 == 0 && a->ldc >= a->N);
  DTC_HOST_CHECK(((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->B & 15) == 0 && ((uintptr_t)a->C & 15) == 0);
  DTC_HOST_CHECK(a->ldc % 4 == 0 && x->sa && x->sb && x->ldsa >= a->K / 32 && x->ldsb >= a->K / 32);
  DTC_HOST_CHECK(a->epi == EPI_STORE || a->epi == EPI_RESID || a->epi == EPI_GELU);
  DTC_HOST_CHECK(a->epi != EPI_RESID || (a->c_f32 && a->aux && a->ldaux >= a->N && a->ldaux % 4 == 0 &&
                                         ((uintptr_t)a->aux & 15) == 0));
  DTC_HOST_CHECK(a->epi != EPI_GELU || (!a->c_f32 && a->aux_out && ((uintptr_t)a->aux_out & 7) == 0));
  DTC_HOST_CHECK(!a->bias || ((uintptr_t)a->bias & 15) == 0);
  DTC_HOST_CHECK((x->gq != nullptr) == (x->gsc != nullptr));
  DTC_HOST_CHECK(!x->gq || (a->epi == EPI_GELU && a->N % 32 == 0 && ((uintptr_t)x->gq & 3) == 0));
  const long t128 = (long)((a->M + 127) / 128) * ((a->N + F8_BN - 1) / F8_BN);
  const int tm = g_fp8_force_tm ? g_fp8_force_tm : (t128 >= fp8_cu_count() ? 4 : 2);
  return tm == 4 ? launch_mxfp8_epi<4>(*a, *x, st) : launch_mxfp8_epi<2>(*a, *x, st);
}

}  // extern "C"
