// fp8_convert.h — the device convert every weight-only fp8 kernel shares
// (linear_fp8.hip, moe.hip): eight OCP e4m3 bytes to the eight bf16 of one
// MFMA operand.
#pragma once
#include "hip_common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// 8 e4m3 bytes (two dwords) -> the 8 bf16 of one MFMA operand, in byte order.
// e4m3 is exact in bf16: the convert with scale 1 unpacks two bytes.
__device__ __forceinline__ short8 fp8x8_to_bf16(uint32_t lo, uint32_t hi) {
  union { bf16x2 h[4]; short8 s; } u;
  u.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  u.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  u.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  u.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return u.s;
}
