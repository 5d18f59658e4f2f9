// linear_fp8_block.hip — block-scaled fp8 linears on the fp8 matrix
// instruction of gfx950 (the recipe of the public DeepSeek-V3 / Qwen3-FP8
// checkpoints): e4m3 weights with one fp32 scale per 128 x 128 block, e4m3
// activations with one dynamic fp32 scale per token and 128-wide group of K.
//   xq[m, k], sx[m, g] = the codes and group scales of x[m, :]
//   y[m, n] = bf16(sum_g sx[m, g] * scale[n / 128, g] *
//                  sum_{k in g} float(xq[m, k]) * float(wq[n, k]))
//
// x [T, in] bf16; wq [out, in] OCP e4m3, K contiguous; scale [NBk, G] fp32,
// NBk = ceil(out / 128), G = ceil(in / 128); y [T, out] bf16. in % 64 == 0
// (the last group may be 64 wide), out % 16 == 0, T >= 1 here.
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 consumes exactly one group, so the
// scale promotion needs no bookkeeping below an instruction: every MFMA goes
// into a zeroed partial, and acc = fma(partial, sx[m, g] * scale[nb, g],
// acc) in fp32 VALU. The instruction's own e8m0 scale operands stay at 1:
// these scales are arbitrary fp32 values.
//
//   quantize_groups_fp8_kernel    grid (T, ceil(in / 4096))
//     A group is 256 bytes of bf16: 16 lanes x 16 bytes, so a wave owns four
//     groups a load and a workgroup 16. A thread keeps QG_HELD = 2 chunks:
//     the group absmax is a 16-lane xor-shuffle reduction (no LDS), and the
//     codes come from the registers that fed it, so every element is read
//     from memory once whatever `in` is, and a wide row spreads over several
//     workgroups. True fp32 division on scale and elements: the bytes of
//     ops.ref.quantize_groups_fp8. The scales go to sx[g * Tp + m]
//     (launchers.h gives the layout's reason).
//
//   linear_fp8_block_kernel<WM, WN>    grid (column tiles, row tiles)
//     linear_fp8_a8_kernel with the promotion: the swizzled LDS tile, the
//     staging and the double-buffered slab loop are those of fp8_tile.h, a
//     slab is a group. Tile origins are multiples of the tile edge (64 or
//     128), which divides 128, so the weight scale is one value a workgroup
//     and slab; the row scales of a lane's D rows, (lane >> 4) * 4 + j of
//     each row block, are one 16-byte load a row block. Both are fetched
//     with the loads of the slab in flight, before the MFMAs of the current
//     one, and multiplied together when their slab is consumed. The epilogue
//     is that of linear_fp8_a8_kernel without the two multiplies.
//
//   linear_fp8_block_skinny_kernel<MB, NB>   grid (column block, 64-row tile,
//                                                  K split)
//     The decode-sized kernel, registers only, in the spirit of
//     linear_fp8.hip: a workgroup of four waves owns BN = 16 NB columns and
//     16 MB rows over one K split, and its waves take the split's groups
//     round-robin. Per group a lane loads the 32 weight bytes
//     [32 (lane >> 4), +32) of row lane & 15 of each column block and the
//     same 32 bytes of each row block's codes, straight into the operand
//     registers of one MFMA per (row block, column block); lanes past `in`
//     in the 64-wide tail group hold zeros. BN divides 128 and n0 is a
//     multiple of BN, so again one weight scale a workgroup and group. A
//     ring of DEPTH stages (operands and scales) stays in flight over the
//     MFMAs. The partial is one column block at a time, MB x 4 registers.
//     The four waves' accumulators are summed through LDS in wave order.
//   linear_fp8_block_reduce_kernel   only when K is split across workgroups
//     (linear_fp8_block_k_splits): sums the fp32 partials in split order.
//
// Determinism: no atomics. In the tiled kernel an element is one
// accumulator over the groups in order. In the skinny kernel the split
// count and the group -> (split, wave) assignment depend on (in, out)
// alone, and the wave and split sums run in a fixed order. MFMA rows and
// columns never mix, and the k a lane feeds to an instruction depends on
// the group alone. So within either kernel a row's bits do not depend on T,
// on the row's index, on the other rows of the launch or on the tile / MB /
// BN choice. The two kernels sum the groups in different orders: a row's
// bits may differ between batch sizes that linear_fp8_block_kernel_for sends
// to different kernels.
#include "hip_common.h"
#include "launchers.h"
#include "fp8_tile.h"

// Built without packed fp32 arithmetic, as linear_fp8.hip is and for the
// reason given there.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using namespace fp8_tile;
constexpr int GROUP = LINEAR_FP8_BLOCK_GROUP;
static_assert(GROUP == BK, "a slab of the tiled kernel is one group");

// ---- quantiser -----------------------------------------------------------

constexpr int QG_HELD = 2;   // chunks a thread: 256 * 2 * 8 = 4096 k a workgroup

__global__ __launch_bounds__(A8_THREADS) void quantize_groups_fp8_kernel(
    const short* __restrict__ x, unsigned char* __restrict__ xq,
    float* __restrict__ sx, int Tp, int in) {
  const int row = blockIdx.x;
  const int n_chunks = in / 8;   // a multiple of 8: half a group
  const short8* xr = (const short8*)(x + (int64_t)row * in);
  u32x2* qr = (u32x2*)(xq + (int64_t)row * in);

  short8 held[QG_HELD];
  float amax[QG_HELD];
#pragma unroll
  for (int i = 0; i < QG_HELD; ++i) {
    const int c = (blockIdx.y * QG_HELD + i) * A8_THREADS + threadIdx.x;
    amax[i] = 0.f;
    if (c < n_chunks) {
      held[i] = xr[c];
      amax[i] = absmax8(held[i], 0.f);
    }
  }
  // the 16 lanes of a group; lanes past `in` (the upper half of a 64-wide
  // tail group) take part with 0
#pragma unroll
  for (int i = 0; i < QG_HELD; ++i) {
    amax[i] = fmaxf(amax[i], __shfl_xor(amax[i], 8, 16));
    amax[i] = fmaxf(amax[i], __shfl_xor(amax[i], 4, 16));
    amax[i] = fmaxf(amax[i], __shfl_xor(amax[i], 2, 16));
    amax[i] = fmaxf(amax[i], __shfl_xor(amax[i], 1, 16));
  }
#pragma unroll
  for (int i = 0; i < QG_HELD; ++i) {
    const int c = (blockIdx.y * QG_HELD + i) * A8_THREADS + threadIdx.x;
    if (c < n_chunks) {
      const float s =
          amax[i] > 0.f ? __fdiv_rn(amax[i], FP8_E4M3_MAX) : 1.f;
      if ((threadIdx.x & 15) == 0) sx[(int64_t)(c >> 4) * Tp + row] = s;
      qr[c] = quant8(held[i], s);
    }
  }
}

// ---- tiled GEMM ----------------------------------------------------------

// The promoting policy of gemm_slabs: the scales of this lane's D rows and
// of the workgroup's weight block, one slab ahead.
template <int WM>
struct BlockScales {
  static constexpr bool promoted = true;
  const float* sx[WM];   // the lane's row quad of row block mb, group 0
  const float* ws;       // the workgroup's row of scale: [G]
  int Tp;
  f32x4 cur_r[WM], nxt_r[WM];
  float cur_w, nxt_w;

  __device__ __forceinline__ void fetch(int slab) {
#pragma unroll
    for (int mb = 0; mb < WM; ++mb)
      nxt_r[mb] = *(const f32x4*)(sx[mb] + (int64_t)slab * Tp);
    nxt_w = ws[slab];
  }
  __device__ __forceinline__ void advance() {
#pragma unroll
    for (int mb = 0; mb < WM; ++mb) cur_r[mb] = nxt_r[mb];
    cur_w = nxt_w;
  }
  __device__ __forceinline__ f32x4 row_scales(int mb, int /*nb*/) const {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = cur_r[mb][j] * cur_w;
    return r;
  }
};

template <int WM, int WN>
__global__ __launch_bounds__(A8_THREADS) void linear_fp8_block_kernel(
    const unsigned char* __restrict__ xq, const float* __restrict__ sx,
    const unsigned char* __restrict__ wq, const float* __restrict__ scale,
    short* __restrict__ y, int T, int in, int out) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int STAGE = (BM + BN) * BK;
  constexpr int PITCH = BN + 8;  // shorts: rows of the y tile stay 16-byte aligned
  static_assert(GROUP % BN == 0, "a tile lies in one 128-row weight block");
  static_assert(BM * PITCH * 2 <= 2 * STAGE, "the y tile fits the slab buffers");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = (wave >> 1) * WM * 16, wn = (wave & 1) * WN * 16;
  const int G = (in + GROUP - 1) / GROUP, Tp = linear_fp8_block_tp(T);

  Staging<WM> sa;
  Staging<WN> sb;
  sa.init(xq, m0, T, in);
  sb.init(wq, n0, out, in);
  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j. Row
  // quads past T read the last quad instead and are never stored.
  BlockScales<WM> p;
  p.Tp = Tp;
  p.ws = scale + (int64_t)(n0 / GROUP) * G;
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
    p.sx[mb] = sx + min(m0 + wm + mb * 16 + (lane >> 4) * 4, Tp - 4);
  f32x4 acc[WM][WN];
  gemm_slabs<WM, WN>(sa, sb, lds, acc, wm, wn, in, p);

  short* yt = (short*)lds;
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm + mb * 16 + (lane >> 4) * 4 + j;
#pragma unroll
      for (int nb = 0; nb < WN; ++nb)
        yt[r * PITCH + wn + nb * 16 + (lane & 15)] =
            f32_to_bf16(acc[mb][nb][j]);
    }
  __syncthreads();
  for (int q = threadIdx.x; q < BM * (BN / 8); q += A8_THREADS) {
    const int r = q / (BN / 8), c = (q % (BN / 8)) * 8;
    if (m0 + r < T && n0 + c < out)
      *(short8*)(y + (int64_t)(m0 + r) * out + n0 + c) =
          *(const short8*)(yt + r * PITCH + c);
  }
}

template <int WM, int WN>
void launch_tiled(const LinearFp8BlockArgs& a, hipStream_t stream) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  const dim3 grid((uint32_t)((a.out + BN - 1) / BN),
                  (uint32_t)((a.T + BM - 1) / BM));
  hipLaunchKernelGGL((linear_fp8_block_kernel<WM, WN>), grid,
                     dim3(A8_THREADS), 0, stream, (const unsigned char*)a.xq,
                     a.sx, (const unsigned char*)a.wq, a.scale, (short*)a.y,
                     a.T, a.in, a.out);
}

// ---- skinny GEMM ---------------------------------------------------------

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / WAVE;
constexpr int SK_ROWS = 64;   // rows of a grid.y tile

// One ring stage: a group's weight bytes (32 a column block) and codes (32 a
// row block) of this lane, the scales of its D rows and the weight scale.
template <int MB, int NB>
struct SkStage {
  u32x4 w[NB][2];
  u32x4 x[MB][2];
  f32x4 sx[MB];
  float ws;
};

// What a lane reads of every group: operand rows at its 32-byte column kq,
// its row quads of sx, the workgroup's row of scale.
template <int MB, int NB>
struct SkSource {
  const unsigned char* wp[NB];
  const unsigned char* xp[MB];
  const float* sxp[MB];
  const float* ws;
  int kq, in, Tp;
};

template <int MB, int NB>
__device__ __forceinline__ void sk_load(SkStage<MB, NB>& s,
                                        const SkSource<MB, NB>& src, int g) {
  const int64_t k = (int64_t)g * GROUP;
  // in % 64 == 0: a lane's 32 bytes are below `in` or past it together
  const bool live = g * GROUP + src.kq < src.in;
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    s.w[nb][0] = live ? *(const u32x4*)(src.wp[nb] + k) : zero;
    s.w[nb][1] = live ? *(const u32x4*)(src.wp[nb] + k + 16) : zero;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    s.x[mb][0] = live ? *(const u32x4*)(src.xp[mb] + k) : zero;
    s.x[mb][1] = live ? *(const u32x4*)(src.xp[mb] + k + 16) : zero;
    s.sx[mb] = *(const f32x4*)(src.sxp[mb] + (int64_t)g * src.Tp);
  }
  s.ws = src.ws[g];
}

__device__ __forceinline__ i32x8 sk_operand(const u32x4 (&h)[2]) {
  union { u32x4 h[2]; i32x8 v; } u;
  u.h[0] = h[0];
  u.h[1] = h[1];
  return u.v;
}

// One turn of the ring, as in linear_fp8.hip: stages i .. i + DEPTH - 1 go
// through the matrix core, and each slot is refilled with the stage DEPTH
// later once its MFMAs have read it. TAIL checks every stage against n_it.
template <int MB, int NB, int DEPTH, bool TAIL>
__device__ __forceinline__ void sk_round(SkStage<MB, NB> (&ring)[DEPTH],
                                         f32x4 (&acc)[MB][NB],
                                         const SkSource<MB, NB>& src, int g0,
                                         int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
    i32x8 a[MB];
    f32x4 rs[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      a[mb] = sk_operand(ring[d].x[mb]);
#pragma unroll
      for (int j = 0; j < 4; ++j) rs[mb][j] = ring[d].sx[mb][j] * ring[d].ws;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const i32x8 b = sk_operand(ring[d].w[nb]);
      f32x4 part[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        part[mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a[mb], b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, E8M0_ONE, 0,
            E8M0_ONE);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[mb][nb][j] =
              __builtin_fmaf(part[mb][j], rs[mb][j], acc[mb][nb][j]);
    }
    if (!TAIL || i + d + DEPTH < n_it)
      sk_load(ring[d], src, g0 + (i + d + DEPTH) * SK_WAVES);
    // a stage's MFMAs and adds stay in front of the next stage's wait
    __builtin_amdgcn_sched_barrier(0);
  }
}

// part == null: y = bf16(sum); else part[split, T, out] = sum.
template <int MB, int NB, int DEPTH>
__global__ __launch_bounds__(SK_THREADS) void linear_fp8_block_skinny_kernel(
    const unsigned char* __restrict__ xq, const float* __restrict__ sx,
    const unsigned char* __restrict__ wq, const float* __restrict__ scale,
    short* __restrict__ y, float* __restrict__ part, int T, int in, int out,
    int g_per_split) {
  constexpr int BN = NB * 16;
  static_assert(GROUP % BN == 0, "a column block lies in one weight block");
  __shared__ float red[SK_WAVES][MB][NB][4][WAVE];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * BN, row0 = blockIdx.y * SK_ROWS;
  const int split = blockIdx.z;
  const int r = lane & 15;
  const int G = (in + GROUP - 1) / GROUP;

  // Rows and columns past the end read a valid row instead (T >= 1, n0 <
  // out and out % 16 == 0): MFMA rows and columns never mix, and the
  // epilogue stores nothing for them.
  SkSource<MB, NB> src;
  src.kq = (lane >> 4) * 32;
  src.in = in;
  src.Tp = linear_fp8_block_tp(T);
  src.ws = scale + (int64_t)(n0 / GROUP) * G;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = n0 + nb * 16 + r;
    src.wp[nb] = wq + (int64_t)(n < out ? n : n0 + r) * in + src.kq;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    src.xp[mb] = xq + (int64_t)min(row0 + mb * 16 + r, T - 1) * in + src.kq;
    src.sxp[mb] = sx + min(row0 + mb * 16 + (lane >> 4) * 4, src.Tp - 4);
  }

  f32x4 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this wave's groups: g0, g0 + 4, ... below g_end
  const int g_end = min(G, (split + 1) * g_per_split);
  const int g0 = split * g_per_split + wave;
  const int n_it = (g_end - g0 + SK_WAVES - 1) / SK_WAVES;  // may be <= 0

  SkStage<MB, NB> ring[DEPTH];
  int i = 0;
  if (n_it >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      sk_load(ring[d], src, g0 + d * SK_WAVES);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_it; i += DEPTH)
      sk_round<MB, NB, DEPTH, false>(ring, acc, src, g0, i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it) sk_load(ring[d], src, g0 + d * SK_WAVES);
  }
  for (; i < n_it; i += DEPTH)
    sk_round<MB, NB, DEPTH, true>(ring, acc, src, g0, i, n_it);

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][mb][nb][j][lane] = acc[mb][nb][j];
  __syncthreads();
  const int rows = min(MB * 16, T - row0);
  for (int q = threadIdx.x; q < rows * (BN / 4); q += SK_THREADS) {
    const int m = q / (BN / 4), c = (q % (BN / 4)) * 4;
    const int n = n0 + c;
    if (n >= out) continue;  // out % 16 == 0: four columns are in or out
    const int l0 = ((m & 15) >> 2) * 16 + (c & 15);
    f32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = red[0][m >> 4][c >> 4][m & 3][l0 + e];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w)
        v += red[w][m >> 4][c >> 4][m & 3][l0 + e];
      s[e] = v;
    }
    if (part != nullptr) {
      *(f32x4*)(part + ((int64_t)split * T + row0 + m) * out + n) = s;
    } else {
      short4v o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f32_to_bf16(s[e]);
      *(short4v*)(y + (int64_t)(row0 + m) * out + n) = o;
    }
  }
}

// y = bf16(sum over splits, in split order), four columns a thread.
__global__ __launch_bounds__(SK_THREADS) void linear_fp8_block_reduce_kernel(
    const float* __restrict__ part, short* __restrict__ y, int64_t n_quads,
    int n_split) {
  const int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (i >= n_quads) return;
  f32x4 s = *(const f32x4*)(part + i * 4);
  for (int sp = 1; sp < n_split; ++sp) {
    const f32x4 p = *(const f32x4*)(part + (sp * n_quads + i) * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += p[e];
  }
  short4v o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f32_to_bf16(s[e]);
  *(short4v*)(y + i * 4) = o;
}

template <int MB, int NB>
void launch_skinny(const LinearFp8BlockArgs& a, float* part,
                   hipStream_t stream) {
  // ring depth by registers: a stage holds 2 (NB + MB) 16-byte loads and
  // 4 MB + 1 scales a lane
  constexpr int DEPTH = MB == 4 ? 2 : MB == 2 ? 3 : 4;
  const int G = linear_fp8_block_groups(a.in);
  const dim3 grid((uint32_t)((a.out + NB * 16 - 1) / (NB * 16)),
                  (uint32_t)((a.T + SK_ROWS - 1) / SK_ROWS),
                  (uint32_t)a.n_split);
  hipLaunchKernelGGL((linear_fp8_block_skinny_kernel<MB, NB, DEPTH>), grid,
                     dim3(SK_THREADS), 0, stream, (const unsigned char*)a.xq,
                     a.sx, (const unsigned char*)a.wq, a.scale, (short*)a.y,
                     part, a.T, a.in, a.out,
                     (G + a.n_split - 1) / a.n_split);
}

}  // namespace

hipError_t lds_quantize_groups_fp8(const void* x, void* xq, float* sx, int T,
                                   int in, hipStream_t stream) {
  if (T == 0 || in == 0) return hipSuccess;
  const int per_wg = QG_HELD * A8_THREADS * 8;
  hipLaunchKernelGGL(quantize_groups_fp8_kernel,
                     dim3((uint32_t)T, (uint32_t)((in + per_wg - 1) / per_wg)),
                     dim3(A8_THREADS), 0, stream, (const short*)x,
                     (unsigned char*)xq, sx, linear_fp8_block_tp(T), in);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_linear_fp8_block(const LinearFp8BlockArgs& a,
                                hipStream_t stream) {
  if (a.T == 0 || a.out == 0) return hipSuccess;
  float* part = a.n_split > 1 ? a.part : nullptr;
  switch (a.kernel) {
    case LINEAR_FP8_BLOCK_SKINNY:
      // BN 32 up to 16 rows, 64 beyond, as linear_fp8_bn: x comes from L2
      // once per column block
      if (a.T <= 16) launch_skinny<1, 2>(a, part, stream);
      else if (a.T <= 32) launch_skinny<2, 4>(a, part, stream);
      else launch_skinny<4, 4>(a, part, stream);
      HIP_CHECK_LAST();
      if (part != nullptr) {
        const int64_t n_quads = (int64_t)a.T * a.out / 4;
        hipLaunchKernelGGL(linear_fp8_block_reduce_kernel,
                           dim3((uint32_t)((n_quads + SK_THREADS - 1) /
                                           SK_THREADS)),
                           dim3(SK_THREADS), 0, stream, part, (short*)a.y,
                           n_quads, a.n_split);
      }
      break;
    case 64: launch_tiled<2, 2>(a, stream); break;
    case 128: launch_tiled<4, 4>(a, stream); break;
    default: return hipErrorInvalidValue;
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
