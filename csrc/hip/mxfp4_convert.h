// mxfp4_convert.h — the two device converts every MXFP4 kernel shares
// (linear_mxfp4.hip, moe.hip): an e8m0 scale byte to a float, and eight e2m1
// codes times that float to the eight bf16 of one MFMA operand.
#pragma once
#include "hip_common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// e8m0 byte -> 2^(byte - 127): the byte is the exponent field
__device__ __forceinline__ float e8m0_to_f32(uint32_t b) {
  union { uint32_t i; float f; } c;
  c.i = b << 23;
  return c.f;
}

// 8 e2m1 codes (one dword, k ascending from the low nibble of byte 0) times
// sc -> the 8 bf16 of one MFMA operand. The convert puts the low nibble of
// the selected byte in the low half of its result.
__device__ __forceinline__ short8 fp4x8_to_bf16(uint32_t v, float sc) {
  union { bf16x2 h[4]; short8 s; } u;
  u.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 0);
  u.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 1);
  u.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 2);
  u.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 3);
  return u.s;
}
