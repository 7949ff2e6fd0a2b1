// Exact-integer probe of the A/B operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands
// (cbsz = blgp = 0, E8M0 scales 2^0).  One wave, one MFMA per case.
//
// Hypothesis H: lane l holds row i = l & 15 of A (column j = l & 15 of B), and byte b (0..31) of its eight
// dwords is k = 32 (l >> 4) + b, for A and B alike; D follows the 16x16 C/D map (column = lane & 15,
// row = 4 (lane >> 4) + reg).
//
// For every (i0, k0), A is one-hot at (i0, k0) under H and B[k][j] under H is, in three passes,
// (k & 15) - 8, (k >> 4) - 4 and j - 8: all exact in e4m3.  Under H, D[i0][j] must be that value at k = k0 and
// every other row 0; the three passes together pin k0 (both nibbles) and j, so any other pairing of A bytes with
// B bytes, or another row / column placement, fails.  Prints the mismatch count (0 = H holds).
//
//   hipcc -O2 --offload-arch=gfx950 benchmarks/mfma_f8_map_probe.hip -o mfma_f8_map_probe && ./mfma_f8_map_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// e4m3 code of a small integer v in [-8, 8]
__host__ __device__ inline uint8_t e4m3_int(int v) {
  if (v == 0) return 0;
  const uint8_t s = v < 0 ? 0x80 : 0;
  int a = v < 0 ? -v : v, e = 0;
  while ((a >> (e + 1)) != 0) ++e;                          // a = 2^e * (1 + m / 8)
  const int m = ((a << 3) >> e) & 7;
  return (uint8_t)(s | ((e + 7) << 3) | m);
}

__device__ inline int bval(int pass, int k, int j) { return pass == 0 ? (k & 15) - 8 : (pass == 1 ? (k >> 4) - 4 : j - 8); }

__global__ void probe(int* bad, float* sample) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  int nbad = 0;
  for (int pass = 0; pass < 3; ++pass)
    for (int k0 = 0; k0 < 128; ++k0) {
      const int i0 = (k0 * 7 + pass) & 15;
      uint8_t ab[32], bb[32];
      for (int b = 0; b < 32; ++b) {
        const int k = 32 * g + b;
        ab[b] = (r == i0 && k == k0) ? 0x38 /* 1.0 */ : 0;
        bb[b] = e4m3_int(bval(pass, k, r));
      }
      i32x8 a, bq;
      for (int d = 0; d < 8; ++d) {
        a[d] = ab[4 * d] | (ab[4 * d + 1] << 8) | (ab[4 * d + 2] << 16) | (ab[4 * d + 3] << 24);
        bq[d] = bb[4 * d] | (bb[4 * d + 1] << 8) | (bb[4 * d + 2] << 16) | (bb[4 * d + 3] << 24);
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, bq, acc, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      for (int q = 0; q < 4; ++q) {
        const int row = 4 * g + q, col = r;
        const float want = row == i0 ? (float)bval(pass, k0, col) : 0.f;
        if (acc[q] != want) ++nbad;
        if (pass == 0 && k0 == 37) sample[row * 16 + col] = acc[q];
      }
    }
  atomicAdd(bad, nbad);
}

// Which byte of the 32-bit scale operand the instruction applies, per opsel value 0..3 (the builtin's sixth and
// eighth arguments) and per 32-element block: A one-hot 1.0 at (row 0, k0), B 1.0 at (k0, column 0), the probed
// operand's scale register 0x8281807f in every lane (bytes 0..3 = 2^0, 2^1, 2^2, 2^3), the other operand's 2^0.
// D[0][0] is then 2^(index of the byte used).  out[which * 16 + blk * 4 + opsel], which = 0 for A's scale, 1 for B's.
template <int OPSEL, bool ON_B>
__device__ float scale_byte_case(int lane, int blk) {
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
  if ((lane & 15) == 0 && (lane >> 4) == blk) { a[0] = 0x38; b[0] = 0x38; }  // k0 = 32 blk
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int probed = (int)0x8281807fu, one = 0x7f7f7f7f;
  if constexpr (ON_B) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, one, OPSEL, probed);
  else acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, OPSEL, probed, 0, one);
  return acc[0];  // lane 0: row 0, column 0
}
__global__ void scale_byte_probe(float* out) {
  const int lane = threadIdx.x;
  for (int blk = 0; blk < 4; ++blk) {
    const float r[8] = {scale_byte_case<0, false>(lane, blk), scale_byte_case<1, false>(lane, blk),
                        scale_byte_case<2, false>(lane, blk), scale_byte_case<3, false>(lane, blk),
                        scale_byte_case<0, true>(lane, blk),  scale_byte_case<1, true>(lane, blk),
                        scale_byte_case<2, true>(lane, blk),  scale_byte_case<3, true>(lane, blk)};
    // every lane stores (its own slot): the MFMAs stay outside any single-lane EXEC mask
    for (int i = 0; i < 8; ++i) out[lane * 32 + (i >> 2) * 16 + blk * 4 + (i & 3)] = r[i];
  }
}

// Which lane group's scale the instruction applies to a given operand byte: A one-hot 1.0 at byte j of lane group
// g (row 0), B 1.0 in the same place (column 0), A's scale register 2^q in lane group q (all four bytes), B's 2^0.
// D[0][0] = 2^q names the lane group q whose scale was used, i.e. the 32-element scale block the byte belongs to.
// out[lane * 32 + g * 8 + jj], jj indexing j in {0, 7, 15, 16, 24, 31, 3, 19}.
__global__ void scale_block_probe(float* out) {
  const int lane = threadIdx.x, grp = lane >> 4;
  const int js[8] = {0, 7, 15, 16, 24, 31, 3, 19};
  const int sa = (0x7f + grp) * 0x01010101, one = 0x7f7f7f7f;
  for (int g = 0; g < 4; ++g)
    for (int jj = 0; jj < 8; ++jj) {
      const int j = js[jj];
      i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
      if ((lane & 15) == 0 && grp == g) {
        for (int d = 0; d < 8; ++d)
          if (d == (j >> 2)) { a[d] = 0x38 << (8 * (j & 3)); b[d] = a[d]; }
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, sa, 0, one);
      out[lane * 32 + g * 8 + jj] = acc[0];
    }
}

static void run_scale_block_probe() {
  float* out;
  if (hipMalloc(&out, 64 * 32 * 4) != hipSuccess) return;
  (void)hipMemset(out, 0, 64 * 32 * 4);
  hipLaunchKernelGGL(scale_block_probe, dim3(1), dim3(64), 0, 0, out);
  float h[32];
  if (hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;  // lane 0's slots
  const int js[8] = {0, 7, 15, 16, 24, 31, 3, 19};
  for (int g = 0; g < 4; ++g) {
    printf("scale block probe: byte j of lane group %d ->", g);
    for (int jj = 0; jj < 8; ++jj) printf(" j=%d: 2^%d", js[jj], h[g * 8 + jj] > 0 ? (int)log2f(h[g * 8 + jj]) : -1);
    printf("   (2^q = the scale of lane group q was applied)\n");
  }
  (void)hipFree(out);
}

static void run_scale_byte_probe() {
  float* out;
  if (hipMalloc(&out, 64 * 32 * 4) != hipSuccess) return;
  (void)hipMemset(out, 0, 64 * 32 * 4);
  hipLaunchKernelGGL(scale_byte_probe, dim3(1), dim3(64), 0, 0, out);
  float h[32];
  if (hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;  // lane 0's slots
  for (int w = 0; w < 2; ++w)
    for (int blk = 0; blk < 4; ++blk) {
      printf("scale byte probe: %c scale, one-hot in block %d, opsel 0..3 ->", w ? 'B' : 'A', blk);
      for (int o = 0; o < 4; ++o) printf(" %g", h[w * 16 + blk * 4 + o]);
      printf("   (2^i = byte i of the scale register)\n");
    }
  (void)hipFree(out);
}

int main() {
  run_scale_byte_probe();
  run_scale_block_probe();
  int* bad;
  float* sample;
  if (hipMalloc(&bad, 4) != hipSuccess || hipMalloc(&sample, 1024) != hipSuccess) return 2;
  (void)hipMemset(bad, 0, 4);
  (void)hipMemset(sample, 0, 1024);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, bad, sample);
  int h = -1;
  float hs[256];
  if (hipMemcpy(&h, bad, 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  (void)hipMemcpy(hs, sample, 1024, hipMemcpyDeviceToHost);
  printf("mfma_scale_f32_16x16x128_f8f6f4 e4m3 map probe: %d mismatches over 3 x 128 cases (0 = hypothesis holds)\n", h);
  printf("sample (pass 0, k0 = 37, i0 = %d): row i0 =", (37 * 7) & 15);
  for (int j = 0; j < 16; ++j) printf(" %g", hs[((37 * 7) & 15) * 16 + j]);
  printf("\n");
  return h == 0 ? 0 : 1;
}
