// flash_prefill_glds.hip — the bf16-KV variant of the fused MFMA prefill
// attention with a glds staging pipeline (guide §5 "glds with >1 tile in
// flight"): K/V tiles are DMA'd straight to LDS (`global_load_lds`) into a
// 3-deep ring, one tile ahead, with COUNTED `s_waitcnt vmcnt(N)` and raw
// `s_barrier` (a `__syncthreads()` would drain the in-flight DMA; hipcc
// also drains glds at any ordinary in-loop global load, so the block table
// is staged into LDS up front and the hot loop touches global memory ONLY
// through glds). The LDS image stays lane-linear (a glds constraint); the
// XOR bank swizzle is applied by permuting the per-lane SOURCE addresses.
//
// Ring safety: iteration order is [counted vmcnt][raw barrier]
// [compute tile n][issue tile n+2] — barrier C_n separates every wave's
// last read of buffer (n-1)%3 (its compute at iteration n-1, before C_n)
// from the buffer's rewrite for tile n+2 (after C_n in every wave).
//
// fp8 KV cannot ride glds (raw byte copy, no conversion point), so the
// fp8 path keeps the convert-on-stage kernel in flash_prefill.hip; the
// launcher in ops.hip picks per cache dtype. The attention math, fragment
// layouts and the swizzle are shared with that kernel (flash_tile.h); this
// file is staging + ring loop + launcher.
#include "flash_tile.h"
#include "launchers.h"

namespace {

using namespace flash;

constexpr int KVBLK = SUBTILE;  // tokens per KV tile (ring granularity)
constexpr int NBUF = 3;
constexpr int BT_CAP = FLASH_GLDS_BT_CAP;  // staged block-table entries

constexpr int TILE_SHORTS = KVBLK * D;           // 4096 shorts = 8 KB
constexpr int GLDS_PER_WAVE = KVBLK * 16 / 64 / NW;  // K instrs/wave (=2)

__device__ __forceinline__ void raw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

template <int QPG>
__global__ __launch_bounds__(NW * WAVE, 2) void flash_prefill_glds_kernel(
    const short* __restrict__ q, const short* __restrict__ k_cache,
    const short* __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,
    const int32_t* __restrict__ seq_meta, const int32_t* __restrict__ tiles,
    short* __restrict__ out, int kvh, int bs, int max_blocks, float scale) {
  const int kh = blockIdx.y;
  const RowGeom r = row_geom<QPG>(tiles, seq_meta, kvh);
  const int ctx = r.ctx;

  // ONE shared object (a second __shared__ symbol makes hipcc emit
  // vmcnt(0) before every ds_read — guide §5 trap (a))
  __shared__ __align__(16) char lds_raw[BT_CAP * 4 +
                                        NBUF * 2 * TILE_SHORTS * 2];
  int32_t* bt_lds = (int32_t*)lds_raw;
  auto kbuf = [&](int b) -> short* {
    return (short*)(lds_raw + BT_CAP * 4) + b * 2 * TILE_SHORTS;
  };
  auto vbuf = [&](int b) -> short* { return kbuf(b) + TILE_SHORTS; };

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int n_kv_tiles = (r.kv_end_wg + KVBLK - 1) / KVBLK;

  // ---- prologue: Q fragments + block table; every ordinary global load
  //      completes before the first glds issues ----
  bf16x8 q_frag[D / 16];
  load_q_frags(q, r, q_frag);
  // stage enough entries to cover the final tile's clamped pad rows
  // (t = min(tile0+row, ctx-1) can reach up to kv_end_wg + KVBLK - 1)
  const int n_bt = min(max_blocks,
                       (min(r.kv_end_wg + KVBLK, ctx) + bs - 1) / bs);
  for (int i = tid; i < n_bt; i += NW * WAVE)
    bt_lds[i] = block_tables[(int64_t)r.seq * max_blocks + i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // publish bt_lds (no glds in flight yet)

  auto stage_tile = [&](int n) {
    const int tile0 = n * KVBLK;
    const int buf = n % NBUF;
#pragma unroll
    for (int j = 0; j < GLDS_PER_WAVE; ++j) {
      const int piece = (wave * GLDS_PER_WAVE + j) * 64 + lane;
      const int row = piece / 16, c16 = piece % 16;
      const int src16 = c16 ^ swz4(row);        // source-side swizzle
      const int t = min(tile0 + row, ctx - 1);  // clamp: no garbage bf16
      const int64_t base =
          (((int64_t)bt_lds[t / bs] * kvh + kh) * bs + t % bs) * D;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              k_cache + base + src16 * 8),
          (__attribute__((address_space(3))) unsigned int*)(
              (char*)kbuf(buf) + (wave * GLDS_PER_WAVE + j) * 1024),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              v_cache + base + src16 * 8),
          (__attribute__((address_space(3))) unsigned int*)(
              (char*)vbuf(buf) + (wave * GLDS_PER_WAVE + j) * 1024),
          16, 0, 0);
    }
  };

  float m_run = NEG, l_run = 0.f;
  f32x16 acc_o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) acc_o[dt] = (f32x16)(0.f);

  stage_tile(0);
  if (n_kv_tiles > 1) stage_tile(1);

  for (int n = 0; n < n_kv_tiles; ++n) {
    const int tile0 = n * KVBLK;
    const int buf = n % NBUF;
    // tile n has landed when at most the NEXT tile's DMA remains in
    // flight (counted per-wave wait; vmcnt retires in order)
    if (n + 1 < n_kv_tiles)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * GLDS_PER_WAVE)
                   : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    raw_barrier();

    if (tile0 < r.kv_end_w)
      attend_subtile(kbuf(buf), vbuf(buf), tile0, r, q_frag, scale, m_run,
                     l_run, acc_o);
    if (n + 2 < n_kv_tiles) stage_tile(n + 2);
  }

  store_out(out, r, l_run, acc_o);
}

}  // namespace

hipError_t lds_flash_prefill_glds(const AttnArgs& a, hipStream_t stream) {
  if (a.n_tiles == 0) return hipSuccess;
  if (a.head_dim != D || a.max_blocks > BT_CAP || a.kv_fp8)
    return hipErrorInvalidValue;
  dim3 grid(a.n_tiles, a.kvh), block(NW * WAVE);
  const bool ok = dispatch_qpg(a.n_q_heads / a.kvh, [&](auto Q) {
    hipLaunchKernelGGL((flash_prefill_glds_kernel<decltype(Q)::value>), grid,
                       block, 0, stream, (const short*)a.q,
                       (const short*)a.k_cache, (const short*)a.v_cache,
                       a.block_tables, a.seq_meta, a.tiles, (short*)a.out,
                       a.kvh, a.bs, a.max_blocks, a.scale);
  });
  if (!ok) return hipErrorInvalidValue;
  HIP_CHECK_LAST();
  return hipSuccess;
}
