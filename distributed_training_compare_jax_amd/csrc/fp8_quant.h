// Device helpers shared by the e4m3 quantisers (csrc/gemm_fp8.hip) and the producers that emit MXFP8 output
// beside their bf16 output (csrc/norm_reduce.hip): the power-of-two scale exponent of an amax and the e4m3 rounding.
#pragma once
#include "common.h"

// Scale exponent se from amax's bit pattern: s = 2^se.  e = biased exponent - 127; amax * 2^(8-e) = 256 * mantissa
// is above 448 exactly when the mantissa is above 1.75 (fraction bits > 0x600000).  se is clamped to [-126, 126] so
// that 2^se and 2^-se are normal fp32 (and 127 - se is an E8M0 byte in 1..253); a subnormal amax (e < -126) lands
// on the upper clamp; amax == 0 gives 0.
__device__ __forceinline__ int se_of_amax(uint32_t bits) {
  const int ef = (int)(bits >> 23);
  int se = 0;
  if (bits != 0u) {
    se = ef == 0 ? 126 : ((bits & 0x7fffffu) > 0x600000u ? 7 : 8) - (ef - 127);
    se = se < -126 ? -126 : (se > 126 ? 126 : se);
  }
  return se;
}
__device__ __forceinline__ float pow2_f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }

// Two fp32 values -> two e4m3 bytes (low 16 bits), round to nearest even.  The hardware convert handles the
// normal range (|v| >= 2^-6); the e4m3 subnormal range is rounded here as an integer count of 2^-9 steps
// (0..8, where 8 is the encoding of 2^-6 itself), so the result does not depend on how the convert treats it.
__device__ __forceinline__ uint32_t e4m3_sub(float v) {
  return ((__float_as_uint(v) >> 24) & 0x80u) | (uint32_t)(int)rintf(fabsf(v) * 512.f);
}
__device__ __forceinline__ uint32_t e4m3_pk2(float v0, float v1) {
  uint32_t p = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false) & 0xffffu;
  if (fabsf(v0) < 0.015625f) p = (p & 0xff00u) | e4m3_sub(v0);
  if (fabsf(v1) < 0.015625f) p = (p & 0x00ffu) | (e4m3_sub(v1) << 8);
  return p;
}
__device__ __forceinline__ uint32_t e4m3_pk4(float v0, float v1, float v2, float v3) {
  return e4m3_pk2(v0, v1) | (e4m3_pk2(v2, v3) << 16);
}

// max over the lanes l ^ o of the |x| bit patterns (an integer max: exact and order-independent)
__device__ __forceinline__ uint32_t amax_xor(uint32_t mx, int o) { return max(mx, (uint32_t)__shfl_xor((int)mx, o, 64)); }
