// fp8_tile.h — the LDS-staged fp8 operand tile shared by the W8A8 GEMMs
// (linear_fp8_a8.hip, moe_fp8_a8.hip, linear_fp8_block.hip,
// moe_fp8_block.hip): the swizzled
// tile address, a thread's staging registers, the MFMA operand read and the
// slab loop, and the eight-element steps of the activation quantisers. The
// layout and its derivation are in the header of linear_fp8_a8.hip.
#pragma once
#include "hip_common.h"
#include "launchers.h"

// Built without packed fp32 arithmetic, as the kernels it is inlined into
// are (linear_fp8.hip gives the reason).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fp8_tile {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(8))) int i32x8;
constexpr int A8_THREADS = 256;
constexpr int A8_WAVES = A8_THREADS / WAVE;
constexpr int BK = LINEAR_FP8_A8_BK;     // bytes of K a slab
constexpr int CHUNKS = BK / 16;          // 16-byte chunks of a tile row
constexpr int E8M0_ONE = 0x7F7F7F7F;     // scale 2^0 in every byte

// ---- quantiser steps -------------------------------------------------------

__device__ __forceinline__ float absmax8(short8 v, float m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(bf16_to_f32(v[j])));
  return m;
}

// 8 bf16 -> 8 e4m3 codes of x / sx, clamped to +-448, in element order
__device__ __forceinline__ u32x2 quant8(short8 v, float sx) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float q = __fdiv_rn(bf16_to_f32(v[j]), sx);
    f[j] = q > FP8_E4M3_MAX ? FP8_E4M3_MAX
                            : (q < -FP8_E4M3_MAX ? -FP8_E4M3_MAX : q);
  }
  u32x2 o = {0u, 0u};
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], o[0], false);
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], o[0], true);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], o[1], false);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], o[1], true);
  return o;
}

// ---- operand tile ----------------------------------------------------------

// the single LDS address function of an operand tile: byte offset of the
// 16-byte chunk c of row r
__host__ __device__ constexpr int tile_off(int r, int c) {
  return r * BK + ((c ^ ((r >> 1) & (CHUNKS - 1))) << 4);
}

constexpr bool tile_off_conflict_free() {
  // operand read: 16 consecutive rows at one chunk; staging write: two rows
  // with all 8 chunks. Both must cover the 16 slots of a 256-byte line.
  for (int r0 = 0; r0 < 32; r0 += 16)
    for (int c = 0; c < CHUNKS; ++c) {
      unsigned seen = 0;
      for (int r = r0; r < r0 + 16; ++r) seen |= 1u << ((tile_off(r, c) >> 4) & 15);
      if (seen != 0xFFFFu) return false;
    }
  for (int r0 = 0; r0 < 16; r0 += 2) {
    unsigned seen = 0;
    for (int q = 0; q < 16; ++q)
      seen |= 1u << ((tile_off(r0 + (q >> 3), q & 7) >> 4) & 15);
    if (seen != 0xFFFFu) return false;
  }
  return true;
}
static_assert(tile_off_conflict_free(), "a pass of 16 lanes covers 16 slots");

// This thread's chunks of one operand's slab: R rows of 32 apart.
template <int R>
struct Staging {
  const unsigned char* src[R];  // global address of the chunk in slab 0
  int dst[R];                   // tile_off of the chunk
  u32x4 v[R];

  // tile row r is row row_of(r) of a [., in] matrix: any in-bounds row
  template <class F>
  __device__ __forceinline__ void init_rows(const unsigned char* base, int in,
                                            F&& row_of) {
    const int r = threadIdx.x >> 3, c = threadIdx.x & (CHUNKS - 1);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      src[i] = base + (int64_t)row_of(r + 32 * i) * in + c * 16;
      dst[i] = tile_off(r + 32 * i, c);
    }
  }
  // rows row0 + (tid >> 3) + 32 i of a [n_rows, in] matrix, clamped
  __device__ __forceinline__ void init(const unsigned char* base, int row0,
                                       int n_rows, int in) {
    init_rows(base, in, [=](int r) { return min(row0 + r, n_rows - 1); });
  }
  // in_slab: this thread's chunk of the slab lies below `in`
  __device__ __forceinline__ void load(int slab, bool in_slab) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      v[i] = in_slab ? *(const u32x4*)(src[i] + (int64_t)slab * BK)
                     : u32x4{0u, 0u, 0u, 0u};
  }
  __device__ __forceinline__ void store(unsigned char* tile) const {
#pragma unroll
    for (int i = 0; i < R; ++i) *(u32x4*)(tile + dst[i]) = v[i];
  }
};

// the 32 operand bytes of this lane for the block whose first row is `row0`
__device__ __forceinline__ i32x8 read_operand(const unsigned char* tile,
                                              int row0) {
  const int lane = threadIdx.x % WAVE;
  const int r = row0 + (lane & 15), c = (lane >> 4) * 2;
  union { u32x4 h[2]; i32x8 v; } u;
  u.h[0] = *(const u32x4*)(tile + tile_off(r, c));
  u.h[1] = *(const u32x4*)(tile + tile_off(r, c + 1));
  return u.v;
}

// What gemm_slabs does with an instruction's result. NoPromotion: the MFMA
// adds into the running sum itself, one scale pair for the whole of K
// (linear_fp8_a8.hip, moe_fp8_a8.hip). A promoting policy (BlockScales of
// linear_fp8_block.hip, GatheredScales of moe_fp8_block.hip) has per-slab
// scales: the MFMA goes into a zeroed partial and acc += partial *
// row_scales(mb, nb)[j]. It provides
//   fetch(slab)          issue the loads of a slab's scales (no wait)
//   advance()            the scales fetched last become the current ones;
//                        called before the barrier that publishes their slab
//   row_scales(mb, nb)   the current scale of this lane's D rows j of row
//                        block mb against column block nb (the dense kernel
//                        has one weight scale a workgroup and ignores nb)
struct NoPromotion {
  static constexpr bool promoted = false;
};

// acc += A · Bᵀ over the ceil(in / 128) slabs of K, for a workgroup of four
// waves 2 x 2 whose wave owns WM x WN blocks of 16 x 16 at rows wm of the A
// tile (32 WM rows) and rows wn of the B tile (32 WN rows). lds holds two
// stages of (A tile, B tile). The loads of slab s + 1 (and its scales, under
// a promoting policy) are issued before the MFMAs of slab s and written to
// the other stage behind them: one barrier a slab, and every wave is past
// the last read of lds when this returns.
template <int WM, int WN, class P>
__device__ __forceinline__ void gemm_slabs(Staging<WM>& sa, Staging<WN>& sb,
                                           unsigned char* lds,
                                           f32x4 (&acc)[WM][WN], int wm,
                                           int wn, int in, P& p) {
  constexpr int A_BYTES = 32 * WM * BK, STAGE = 32 * (WM + WN) * BK;
  const int kc = (threadIdx.x & (CHUNKS - 1)) * 16;  // chunk's k in a slab
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int nb = 0; nb < WN; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_slabs = (in + BK - 1) / BK;
  sa.load(0, kc < in);
  sb.load(0, kc < in);
  if constexpr (P::promoted) p.fetch(0);
  sa.store(lds);
  sb.store(lds + A_BYTES);
  if constexpr (P::promoted) p.advance();
  __syncthreads();
  for (int s = 0; s < n_slabs; ++s) {
    const unsigned char* cur = lds + (s & 1) * STAGE;
    unsigned char* nxt = lds + ((s + 1) & 1) * STAGE;
    const bool more = s + 1 < n_slabs;
    if (more) {
      const bool in_slab = (s + 1) * BK + kc < in;
      sa.load(s + 1, in_slab);
      sb.load(s + 1, in_slab);
      if constexpr (P::promoted) p.fetch(s + 1);
    }
    i32x8 b[WN];
#pragma unroll
    for (int nb = 0; nb < WN; ++nb)
      b[nb] = read_operand(cur + A_BYTES, wn + nb * 16);
#pragma unroll
    for (int mb = 0; mb < WM; ++mb) {
      const i32x8 a = read_operand(cur, wm + mb * 16);
      if constexpr (P::promoted) {
        f32x4 part[WN];
#pragma unroll
        for (int nb = 0; nb < WN; ++nb)
          part[nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a, b[nb], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, E8M0_ONE, 0,
              E8M0_ONE);
#pragma unroll
        for (int nb = 0; nb < WN; ++nb) {
          const f32x4 rs = p.row_scales(mb, nb);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[mb][nb][j] =
                __builtin_fmaf(part[nb][j], rs[j], acc[mb][nb][j]);
        }
      } else {
#pragma unroll
        for (int nb = 0; nb < WN; ++nb)
          acc[mb][nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a, b[nb], acc[mb][nb], 0, 0, 0, E8M0_ONE, 0, E8M0_ONE);
      }
    }
    if (more) {
      sa.store(nxt);
      sb.store(nxt + A_BYTES);
      if constexpr (P::promoted) p.advance();
    }
    // slab s + 1 is visible, and slab s is free for the loads of s + 2
    __syncthreads();
  }
}

template <int WM, int WN>
__device__ __forceinline__ void gemm_slabs(Staging<WM>& sa, Staging<WN>& sb,
                                           unsigned char* lds,
                                           f32x4 (&acc)[WM][WN], int wm,
                                           int wn, int in) {
  NoPromotion p;
  gemm_slabs<WM, WN, NoPromotion>(sa, sb, lds, acc, wm, wn, in, p);
}

}  // namespace fp8_tile

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
