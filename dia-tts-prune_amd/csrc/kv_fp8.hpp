// FP8 (OCP e4m3) K/V caches with one power-of-two scale per key and head (dia_hip.h "FP8 cross K/V", "FP8 self K/V"): the
// quantisation rule and the fragment conversion, ONE definition for the decode step's kernels (attn.hip) and the batched prompt
// prefill (prefill.hip) — a prompted key must be quantised exactly like a generated one.
#pragma once
#include "common.hpp"

// A K / V fragment is 8 bytes instead of 16 and is expanded to bf16x8 in registers (v_cvt_scalef32_pk_bf16_fp8 at scale 1, exact:
// every e4m3 value is a bf16 value)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
__device__ __forceinline__ bf16x8 expand_e4m3(uint2 d) {      // (gemm_mx.hip Fp8::frag at scale 1)
  const bf16x2 r0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d.x, 1.0f, false);
  const bf16x2 r1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d.x, 1.0f, true);
  const bf16x2 r2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d.y, 1.0f, false);
  const bf16x2 r3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d.y, 1.0f, true);
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  const bf16x4 lo = __builtin_shufflevector(r0, r1, 0, 1, 2, 3), hi = __builtin_shufflevector(r2, r3, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// OCP e4m3 (bias 7, subnormal step 2^-9, finite max 448 = 0x7E) of a finite x with |x| <= 448, rounded to nearest even
__device__ __forceinline__ unsigned e4m3_rne(float x) {
  unsigned u = __float_as_uint(x);
  const unsigned s = (u >> 24) & 0x80u;
  u &= 0x7fffffffu;
  if (u < 0x3c800000u) return s | (unsigned)rintf(__uint_as_float(u) * 512.f);     // below 2^-6: multiples of 2^-9 (8 = the first normal)
  u += 0x7ffffu + ((u >> 20) & 1u);          // three mantissa bits stay
  return s | ((u >> 20) - (120u << 3));
}
// kv_scale_bits for an fp32 amax bit pattern: 448 = 1.75 * 2^8, so e = exponent - 8, one more when the significand is above 1.75
__device__ __forceinline__ unsigned kv_scale_bits_f32(unsigned amax) {
  if (amax == 0) return 0x3f800000u;
  const int se = (int)(amax >> 23) - 8 + ((amax & 0x7fffffu) > 0x600000u ? 1 : 0);
  return (unsigned)min(max(se, 1), 254) << 23;
}
__device__ __forceinline__ unsigned e4m3_finite(float x) {      // e4m3_rne, a non-finite or oversized input held to +-448
  const unsigned b = e4m3_rne(x);
  return (b & 0x80u) | min(b & 0x7fu, 0x7eu);
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
