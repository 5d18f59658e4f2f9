// flash_prefill.hip — fused causal varlen GQA prefill attention over the
// paged KV pool, MFMA-tiled for gfx950 (CDNA4): the convert-on-stage
// kernel. It serves fp8 KV (converted to bf16 on the way into LDS) and
// bf16 KV whose block table is too wide for the glds ring
// (flash_prefill_glds.hip).
//
// Replaces the composed einsum+softmax prefill path (materialized S matrix,
// ~6 HBM passes) with a flash-style kernel: per Q-tile, iterate KV tiles
// computing QK^T -> online softmax -> P.V entirely on matrix cores, S never
// leaving registers. The attention math, fragment layouts and the LDS
// swizzle are in flash_tile.h; this file is staging + loop + launcher.
//
// KV loop: 64-token tiles (two 32-token sub-tiles) loaded through VGPRs
// and stored swizzled to LDS between a __syncthreads() pair, rows beyond
// ctx zero-filled; each wave then attends the sub-tiles below its causal
// horizon.
#include "flash_tile.h"
#include "launchers.h"

namespace {

using namespace flash;

constexpr int KVBLK = 2 * SUBTILE;  // tokens per staged KV tile

// SCALED: the cache is fp8 with per-head scales. It is a template flag, not
// a run-time test, so that the unscaled instantiations stay the code they
// were: with the scale loads present the compiler schedules the fp8 kernel
// onto 186 VGPRs (2 workgroups per CU where it had 3). The scaled
// instantiation asks for 3 in its launch bounds and gets 168, no scratch.
template <int QPG, typename CT, bool SCALED>
__global__ __launch_bounds__(NW * WAVE, SCALED ? 3 : 2)
void flash_prefill_kernel(
    const short* __restrict__ q,        // [T, QH, D]
    const CT* __restrict__ k_cache,     // [NB, KVH, BS, D] bf16|fp8
    const CT* __restrict__ v_cache,     // [NB, KVH, BS, D] bf16|fp8
    const int32_t* __restrict__ block_tables,  // [S, max_blocks]
    const int32_t* __restrict__ seq_meta,      // [S, 3] start, chunk, prior
    const int32_t* __restrict__ tiles,         // [n_tiles, 2] seq, vrow0
    short* __restrict__ out,                   // [T, QH, D]
    const float* __restrict__ k_scale,  // [KVH] fp8 dequant scale | null
    const float* __restrict__ v_scale,  // [KVH] fp8 dequant scale | null
    int kvh, int bs, int max_blocks, float scale) {
  const int kh = blockIdx.y;
  // scaled fp8 cache: k = byte * k_scale[kh] folds into the softmax scale
  if (SCALED && k_scale != nullptr) scale *= k_scale[kh];
  const int tid = threadIdx.x;
  const RowGeom r = row_geom<QPG>(tiles, seq_meta, kvh);
  const int32_t* bt = block_tables + (int64_t)r.seq * max_blocks;

  // K tile and V tile: [KVBLK tokens][256 B] row-major, chunks swizzled
  __shared__ short k_lds[KVBLK * D];
  __shared__ short v_lds[KVBLK * D];
  static_assert(KVBLK * 16 % (NW * WAVE) == 0, "staging divides evenly");

  bf16x8 q_frag[D / 16];
  load_q_frags(q, r, q_frag);

  // online-softmax state (per lane = per q-row) and O^T accumulators
  float m_run = NEG, l_run = 0.f;
  f32x16 acc_o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc_o[dt] = (f32x16)(0.f);

  for (int tile0 = 0; tile0 < r.kv_end_wg; tile0 += KVBLK) {
    // ---- stage K and V (swizzled) into LDS ----
    __syncthreads();  // previous tile's reads complete before overwrite
#pragma unroll
    for (int rep = 0; rep < KVBLK * 16 / (NW * WAVE); ++rep) {
      const int ch = tid + rep * (NW * WAVE);
      const int row = ch / 16, c16 = ch % 16;
      const int t = tile0 + row;
      short8 piece = {0, 0, 0, 0, 0, 0, 0, 0};
      short8 vpiece = {0, 0, 0, 0, 0, 0, 0, 0};
      if (t < r.ctx) {
        const int64_t base =
            (((int64_t)bt[t / bs] * kvh + kh) * bs + t % bs) * D;
        piece = load_kv8_bf16(k_cache + base + c16 * 8);
        vpiece = load_kv8_bf16(v_cache + base + c16 * 8);
      }
      *(short8*)((char*)k_lds + swz_off(row, c16 * 16)) = piece;
      *(short8*)((char*)v_lds + swz_off(row, c16 * 16)) = vpiece;
    }
    __syncthreads();

    if (tile0 >= r.kv_end_w) continue;  // beyond this wave's causal horizon

#pragma unroll 1
    for (int half = 0; half < KVBLK / SUBTILE; ++half) {
      const int sub0 = tile0 + SUBTILE * half;
      if (sub0 >= r.kv_end_w) break;
      attend_subtile(k_lds + half * SUBTILE * D, v_lds + half * SUBTILE * D,
                     sub0, r, q_frag, scale, m_run, l_run, acc_o);
    }
  }

  // v = byte * v_scale[kh]: applied once to the finished output row
  if (SCALED && v_scale != nullptr) {
    const float vs = v_scale[kh];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) acc_o[dt] *= vs;
  }
  store_out(out, r, l_run, acc_o);
}

}  // namespace

hipError_t lds_flash_prefill(const AttnArgs& a, hipStream_t stream) {
  if (a.n_tiles == 0) return hipSuccess;
  if (a.head_dim != D) return hipErrorInvalidValue;
  if (!a.kv_fp8 && (a.k_scale || a.v_scale)) return hipErrorInvalidValue;
  dim3 grid(a.n_tiles, a.kvh), block(NW * WAVE);
  const bool ok = dispatch_qpg(a.n_q_heads / a.kvh, [&](auto Q) {
    // ct: a value of the cache element type; scaled: std::true_type to
    // read the scales
    auto launch = [&](auto ct, auto scaled) {
      typedef decltype(ct) CT;
      hipLaunchKernelGGL(
          (flash_prefill_kernel<decltype(Q)::value, CT,
                                decltype(scaled)::value>),
          grid, block, 0, stream, (const short*)a.q, (const CT*)a.k_cache,
          (const CT*)a.v_cache, a.block_tables, a.seq_meta, a.tiles,
          (short*)a.out, a.k_scale, a.v_scale, a.kvh, a.bs, a.max_blocks,
          a.scale);
    };
    if (!a.kv_fp8) launch((short)0, std::false_type{});
    else if (a.k_scale || a.v_scale)
      launch((unsigned char)0, std::true_type{});
    else launch((unsigned char)0, std::false_type{});
  });
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK_LAST();
  return hipSuccess;
}
