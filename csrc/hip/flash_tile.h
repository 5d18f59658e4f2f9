// flash_tile.h — the attention math shared by the two flash-prefill kernels
// (flash_prefill.hip, flash_prefill_glds.hip): row geometry, Q fragments,
// the 32-token sub-tile body and the epilogue. The kernels differ only in
// how a K/V sub-tile reaches LDS; everything they compute lives here.
// This header declares no __shared__ storage (the glds kernel must keep
// all LDS in one object); the functions only take pointers.
//
// Layout choice ("swapped QK^T"): compute S^T = K.Q^T on
// v_mfma_f32_32x32x16_bf16 so each lane owns ONE query row (col = lane&31)
// across all its accumulator registers — the online-softmax row reduction
// is in-lane fmax/adds plus a single cross-half shuffle, the O-rescale is
// a per-lane scalar, and S never leaves registers.
//
// Work decomposition:
//   grid.x = row tiles (128 "virtual rows" = (position, q-head-in-group)
//            pairs, v = p*QPG + g), grid.y = kv_head
//   workgroup = 4 waves; wave w owns v-rows [vrow0+32w, vrow0+32w+32)
// GQA: q-heads of one group share the kv_head's K/V tiles; causal masking
// is per-lane compares (kv <= prior + p), no divergence.
#pragma once
#include <hip/hip_runtime.h>

#include "hip_common.h"

namespace flash {

constexpr int D = 128;       // head_dim
constexpr int NW = 4;        // waves per workgroup
constexpr int QROWS = 32;    // q virtual-rows per wave
constexpr int SUBTILE = 32;  // kv tokens per attend_subtile (one mfma tile)
constexpr float NEG = -1e30f;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

// A K or V sub-tile in LDS is [SUBTILE tokens][256 B] row-major, with the
// 16-B chunks of row r XORed by swz4(r).
//
// Bank swizzle swz4(row): swap the two 2-bit halves of row&15. Chosen from
// the CDNA4 LDS bank model: the K ds_read_b128 only needs it bijective on
// row&15 (its 16-lane groups cover all 16 values of qcol&15, so any
// bijection spreads the 16 slots); the V ds_read_b64_tr_b16 (32-lane
// groups) additionally needs kv0&3 steered into address bits [7:6] so the
// 8-byte granule index (dt | g | r) ^ (swz4 << 1) is injective over the
// group's (g, kv0, r) — the plain XOR by row&15 left granule bits [4:3]
// untouched and put FOUR lanes on every granule (47% of LDS-active cycles
// were conflicts, profiles/r01_pmc_final.md; 0 after, profiles/r02_notes.md).
__host__ __device__ constexpr int swz4(int row) {
  return ((row & 3) << 2) | ((row >> 2) & 3);
}

constexpr bool swz4_is_involution_on_16() {
  unsigned seen = 0;
  for (int r = 0; r < 16; ++r) {
    if (swz4(swz4(r)) != r) return false;
    seen |= 1u << swz4(r);
  }
  return seen == 0xFFFFu;  // bijection on 0..15
}
static_assert(swz4_is_involution_on_16(), "swz4 permutes 0..15, self-inverse");

// the single LDS address function: byte offset of (row, byte_off) in a tile
__host__ __device__ constexpr int swz_off(int row, int byte_off) {
  return row * 256 + (byte_off ^ (swz4(row) << 4));
}

__device__ __forceinline__ unsigned int pack_bf16(float a, float b) {
  return ((unsigned int)(unsigned short)f32_to_bf16(b) << 16) |
         (unsigned int)(unsigned short)f32_to_bf16(a);
}

// This lane's query row and the causal KV extents of its wave / workgroup.
struct RowGeom {
  int seq, seq_start, chunk, prior, ctx;
  bool active;        // lane owns a real (position, head) row
  int p, g, qh;       // position in chunk (-1 if inactive), head in group
  int n_q_heads;
  int64_t q_row;      // row of q/out, clamped to a valid row for loads
  int kv_end_wg, kv_end_w;  // causal horizon of the workgroup / this wave
};

template <int QPG>
__device__ __forceinline__ RowGeom row_geom(
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ seq_meta,
    int kvh) {
  RowGeom r;
  const int kh = blockIdx.y;
  const int wave = threadIdx.x / WAVE;
  r.seq = tiles[2 * blockIdx.x];
  const int vrow0 = tiles[2 * blockIdx.x + 1];
  r.seq_start = seq_meta[3 * r.seq];
  r.chunk = seq_meta[3 * r.seq + 1];
  r.prior = seq_meta[3 * r.seq + 2];
  r.ctx = r.prior + r.chunk;
  r.n_q_heads = kvh * QPG;

  const int vrow = vrow0 + wave * QROWS + (threadIdx.x & 31);
  r.active = vrow < r.chunk * QPG;
  r.p = r.active ? vrow / QPG : -1;
  r.g = r.active ? vrow % QPG : 0;
  const int p_c = r.active ? r.p : r.chunk - 1;  // clamped for loads
  r.qh = kh * QPG + r.g;
  r.q_row = (int64_t)(r.seq_start + p_c) * r.n_q_heads + r.qh;

  const int p_max_wg = min(
      (min(vrow0 + NW * QROWS, r.chunk * QPG) - 1) / QPG, r.chunk - 1);
  const int p_max_w = min(
      (min(vrow0 + (wave + 1) * QROWS, r.chunk * QPG) - 1) / QPG,
      r.chunk - 1);
  r.kv_end_wg = min(r.ctx, r.prior + p_max_wg + 1);
  r.kv_end_w = r.prior + p_max_w + 1;
  return r;
}

// Q^T B-fragments: q_frag[kk] covers head dims [16kk + 8hi, 16kk + 8hi+8)
__device__ __forceinline__ void load_q_frags(const short* __restrict__ q,
                                             const RowGeom& r,
                                             bf16x8 (&q_frag)[D / 16]) {
  const int hi = (threadIdx.x % WAVE) >> 5;
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk)
    q_frag[kk] = *(const bf16x8*)(q + r.q_row * D + kk * 16 + hi * 8);
}

// One 32-token sub-tile: S^T = K.Q^T, mask, online softmax, O^T += V^T.P^T.
// k_lds / v_lds point at a swizzled [SUBTILE][D] bf16 sub-tile whose first
// token is sub0; m_run / l_run / acc_o are this lane's running state.
__device__ __forceinline__ void attend_subtile(
    const short* k_lds, const short* v_lds, int sub0, const RowGeom& r,
    const bf16x8 (&q_frag)[D / 16], float scale, float& m_run, float& l_run,
    f32x16 (&acc_o)[D / 32]) {
  const int lane = threadIdx.x % WAVE;
  const int qcol = lane & 31;
  const int hi = lane >> 5;

  // ---- S^T = K . Q^T : acc rows = kv tokens, cols = q rows ----
  f32x16 acc_s = (f32x16)(0.f);
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk) {
    const bf16x8 k_frag = *(const bf16x8*)(
        (const char*)k_lds + swz_off(qcol, (kk * 16 + hi * 8) * 2));
    acc_s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag, q_frag[kk],
                                                    acc_s, 0, 0, 0);
  }

  // ---- per-lane online softmax over this sub-tile's 32 kv tokens ----
  float s[16];
  float tmax = NEG;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int kv = sub0 + (i & 3) + 8 * (i >> 2) + 4 * hi;
    const bool valid = r.active && kv <= r.prior + r.p;
    s[i] = valid ? acc_s[i] * scale : NEG;
    tmax = fmaxf(tmax, s[i]);
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
  const float m_new = fmaxf(m_run, tmax);
  // MFMA reads operand registers from ALL 64 lanes regardless of EXEC,
  // so the PV block below must run wave-uniformly: lanes with no valid
  // element yet (m_new still NEG) contribute zero P columns instead of
  // branching around the matrix op (a per-lane `if` here corrupts the
  // shared A/B operands with uninitialized registers — measured).
  const bool has = m_new > NEG * 0.5f;
  if (!__any(has)) return;
  const float m_eff = has ? m_new : 0.f;
  const float alpha = (m_run <= NEG * 0.5f) ? 0.f : __expf(m_run - m_eff);
  float tsum = 0.f;
  float pr[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    pr[i] = (s[i] <= NEG * 0.5f) ? 0.f : __expf(s[i] - m_eff);
    tsum += pr[i];
  }
  tsum += __shfl_xor(tsum, 32, WAVE);
  l_run = l_run * alpha + tsum;
  if (has) m_run = m_new;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc_o[dt][e] *= alpha;

  // ---- pack P^T into B fragments (cross-half exchange) ----
  unsigned int w[8], x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    w[i] = pack_bf16(pr[2 * i], pr[2 * i + 1]);
    x[i] = __shfl_xor((int)w[i], 32, WAVE);
  }
  uint4v f0 = hi ? (uint4v){x[2], x[3], w[2], w[3]}
                 : (uint4v){w[0], w[1], x[0], x[1]};
  uint4v f1 = hi ? (uint4v){x[6], x[7], w[6], w[7]}
                 : (uint4v){w[4], w[5], x[4], x[5]};
  const bf16x8 p_frag0 = __builtin_bit_cast(bf16x8, f0);
  const bf16x8 p_frag1 = __builtin_bit_cast(bf16x8, f1);

  // ---- O^T += V^T . P^T ----
  // V stays ROW-MAJOR in LDS; the A-operand (V^T fragments) is gathered by
  // the gfx950 hardware transpose read ds_read_b64_tr_b16: within each
  // fixed 16-lane group, lane i's element j comes from the group's
  // combined 64-short window at [i + 16*j] — pointing lane i at
  // &V[kv0 + i/4][d0 + (i%4)*4] delivers exactly A[dim=d0+i][kv=kv0+j]
  // (layout verified empirically, tools/tr16_probe.hip). This removed the
  // per-element b16 scatter-transpose staging that dominated
  // SQ_LDS_BANK_CONFLICT (profiles/r01_pmc_counters.md).
  typedef __attribute__((address_space(3))) short4v lds_short4v;
  const int i16 = lane % 16;
  const int d_grp = 16 * ((lane & 31) >> 4);  // group's dim base
  const int dim_col = d_grp + (i16 % 4) * 4;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kv0 = ks * 16 + hi * 8 + i16 / 4;
      const int dc = (dt * 32 + dim_col) * 2;
      short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_short4v*)((const char*)v_lds + swz_off(kv0, dc)));
      short4v hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_short4v*)((const char*)v_lds + swz_off(kv0 + 4, dc)));
      short8 vfrag8 = {lo[0], lo[1], lo[2], lo[3],
                       hi4[0], hi4[1], hi4[2], hi4[3]};
      acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          __builtin_bit_cast(bf16x8, vfrag8), ks == 0 ? p_frag0 : p_frag1,
          acc_o[dt], 0, 0, 0);
    }
  }
}

// ---- epilogue: out[seq_start+p][qh][dim] = acc_o / l ----
__device__ __forceinline__ void store_out(short* __restrict__ out,
                                          const RowGeom& r, float l_run,
                                          const f32x16 (&acc_o)[D / 32]) {
  if (!(r.active && l_run > 0.f)) return;
  const int hi = (threadIdx.x % WAVE) >> 5;
  const float inv_l = 1.f / l_run;
  const int64_t out_row =
      ((int64_t)(r.seq_start + r.p) * r.n_q_heads + r.qh) * D;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {   // reg quads: dims 4-contiguous
      const int dim = dt * 32 + 8 * rq + 4 * hi;
      unsigned int lo = pack_bf16(acc_o[dt][4 * rq] * inv_l,
                                  acc_o[dt][4 * rq + 1] * inv_l);
      unsigned int hi2 = pack_bf16(acc_o[dt][4 * rq + 2] * inv_l,
                                   acc_o[dt][4 * rq + 3] * inv_l);
      *(uint2*)(out + out_row + dim) = make_uint2(lo, hi2);
    }
  }
}

}  // namespace flash
