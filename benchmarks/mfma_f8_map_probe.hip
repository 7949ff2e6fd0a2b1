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

int main() {
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
