// moe_fp8_a8.hip — the expert FFN of an MoE layer with fp8 experts and fp8
// activations on the native fp8 matrix instruction of gfx950 (W8A8, dynamic
// per-row scales), as LDS-staged tiled grouped GEMMs for prefill-sized
// batches. A pair is p = t k + j with e = ids[t, j]:
//   (xq, sx) = quantize_rows_fp8(x)                 per token
//   g = (sum_k xq[t, k] w13q[e, n, k]) * sx[t] * w13s[e, n], u the same on
//       row I + n;  act[p, n] = bf16(silu(g) * u)
//   (aq, sa) = quantize_rows_fp8(act)               per pair
//   y2[p, n] = (sum_k aq[p, k] w2q[e, n, k]) * sa[p] * w2s[e, n] * w[t, j]
//   y[t] = bf16(sum_j y2[t k + j])                  moe_combine_kernel
//
// x [T, H] bf16; w13q [E, 2 I, H], w2q [E, H, I] OCP e4m3, K contiguous;
// w13s [E, 2 I], w2s [E, H] fp32. H % 64 == 0, I % 64 == 0, T >= 1 here.
// The work list (tiles, n_tiles, perm) is that of moe.hip (moe_align_kernel)
// with tile heights 64 and 128; both quantiser passes are
// quantize_rows_fp8_kernel of linear_fp8_a8.hip. act, aq, sa and y2 live by
// pair, not by sorted position: the second quantiser pass runs over exactly
// the T k rows gate-up wrote, and no padded row is ever quantised or read.
// That pass is not fused into the gate-up epilogue: a row's absmax spans the
// column workgroups of the row. The GEMM grids are launched at the
// host-known bound moe_tile_bound; a workgroup whose tile index is >=
// n_tiles returns at once, and nothing is read back by the host.
//
// Both GEMM kernels are linear_fp8_a8_kernel as a grouped kernel and share
// its tile code (fp8_tile.h): four waves 2 x 2, a wave owns WM x WN blocks of
// v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 both sides, unit e8m0 scales),
// 128-byte K slabs through double-buffered swizzled LDS with one barrier a
// slab, chunks past K written as zeros (K = 64 mod 128 has no tail loop).
// <2, 2> is the 64-row tile, <4, 4> the 128-row one (moe_fp8_a8_tile).
//
//   moe_gate_up_fp8_a8_kernel<WM, WN>   grid (I / (16 WN), tile bound)
//     A: tile row r is row perm[start + min(r, count - 1)] / k of xq, a
//     gather of whole 128-byte rows of a slab. B: 32 WN rows of w13q[e], of
//     which 16 WN are gate rows n0 .. and 16 WN the up rows I + n0 .. of the
//     same columns. They are laid out in LDS by wave: the 16 WN B-tile rows
//     of wave column h are gate columns n0 + 8 WN h .. + 8 WN - 1, then the
//     up rows of those columns, so blocks nb and WN / 2 + nb of a wave are
//     gate and up of one column block, and silu(g) * u happens in registers
//     with no exchange between waves. Epilogue: (acc * sx[t]) * w13s, silu,
//     the product, one bf16 rounding into an LDS tile (the slab buffers are
//     free by then), stored 16 bytes a thread to act[pair, n0 ..], rows past
//     count masked. I % 64 == 0: every column tile is whole.
//   moe_down_fp8_a8_kernel<WM, WN>      grid (ceil(H / (32 WN)), tile bound)
//     A: tile row r is row perm[start + min(r, count - 1)] of aq. B: rows
//     n0 .. of w2q[e], clamped at H - 1. Epilogue: ((acc * sa[p]) * w2s[e, n])
//     * w[p], stored fp32 to y2[p, n], 16 lanes a 64-byte run, rows past
//     count and columns past H masked (H = 192 leaves the second 128-column
//     tile half masked).
//   The pair, row scale and routing weight of a tile row are fetched before
//   the slab loop and parked in the slab buffers behind it.
//
// Determinism: no atomic touches floating-point data and K is never split.
// Every element is summed by one accumulator over the slabs in order, and the
// k a lane feeds to an instruction depends on the slab alone. The bits of a
// pair depend on its x row, its expert and its routing weight only: not on
// T, on the tile height, on the pair's position in its segment or on the
// other rows of the launch. The tile height decides who computes an element,
// never its bits.
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

// What a kernel knows of its work-list tile.
struct Tile { int start, count, expert; };

__device__ __forceinline__ Tile read_tile(const int32_t* __restrict__ tiles,
                                          int tile) {
  return {tiles[tile * 3], tiles[tile * 3 + 1], tiles[tile * 3 + 2]};
}

template <int WM, int WN>
__global__ __launch_bounds__(A8_THREADS) void moe_gate_up_fp8_a8_kernel(
    const unsigned char* __restrict__ xq, const float* __restrict__ sx,
    const unsigned char* __restrict__ w13q, const float* __restrict__ w13s,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, short* __restrict__ act, int H, int I,
    int k) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int HALF = BN / 2;    // act columns of the workgroup
  constexpr int WH = WN * 8;      // act columns of a wave
  constexpr int STAGE = (BM + BN) * BK;
  constexpr int PITCH = HALF + 8;  // shorts: rows of the act tile stay 16-byte aligned
  constexpr int ROWS_OFF = BM * PITCH * 2;  // row_pair, row_sx behind the tile
  static_assert(WN % 2 == 0, "a wave holds gate and up blocks in pairs");
  static_assert(BM <= A8_THREADS, "one thread a tile row");
  static_assert(ROWS_OFF % 16 == 0 && ROWS_OFF + BM * 8 <= 2 * STAGE,
                "the act tile and the row table fit the slab buffers");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

  if ((int)blockIdx.y >= *n_tiles) return;
  const Tile t = read_tile(tiles, blockIdx.y);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * HALF;
  const int wm = (wave >> 1) * WM * 16, wn = (wave & 1) * WN * 16;

  // Rows past count read the last live row instead (count >= 1): MFMA rows
  // never mix, and nothing of theirs is stored.
  const auto pair_of = [&](int r) { return perm[t.start + min(r, t.count - 1)]; };
  const int my_pair = pair_of(min((int)threadIdx.x, BM - 1));
  const float my_sx = sx[my_pair / k];

  Staging<WM> sa;
  Staging<WN> sb;
  sa.init_rows(xq, H, [&](int r) { return pair_of(r) / k; });
  sb.init_rows(w13q, H, [&](int b) {
    const int q = b % (2 * WH);
    const int col = n0 + (b / (2 * WH)) * WH + q % WH;
    return t.expert * 2 * I + col + (q >= WH ? I : 0);
  });
  f32x4 acc[WM][WN];
  gemm_slabs<WM, WN>(sa, sb, lds, acc, wm, wn, H);

  short* at = (short*)lds;
  int* row_pair = (int*)(lds + ROWS_OFF);
  float* row_sx = (float*)(lds + ROWS_OFF + BM * 4);
  if (threadIdx.x < BM) {
    row_pair[threadIdx.x] = my_pair;
    row_sx[threadIdx.x] = my_sx;
  }
  __syncthreads();

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
  const int wc = (wave & 1) * WH + (lane & 15);  // act column in the tile
  const float* sc = w13s + (int64_t)t.expert * 2 * I + n0 + wc;
  float sg[WN / 2], su[WN / 2];
#pragma unroll
  for (int nb = 0; nb < WN / 2; ++nb) {
    sg[nb] = sc[nb * 16];
    su[nb] = sc[I + nb * 16];
  }
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm + mb * 16 + (lane >> 4) * 4 + j;
      const float sr = row_sx[r];
#pragma unroll
      for (int nb = 0; nb < WN / 2; ++nb) {
        const float g = (acc[mb][nb][j] * sr) * sg[nb];
        const float u = (acc[mb][WN / 2 + nb][j] * sr) * su[nb];
        at[r * PITCH + wc + nb * 16] =
            f32_to_bf16(g / (1.f + expf(-g)) * u);
      }
    }
  __syncthreads();
  for (int q = threadIdx.x; q < BM * (HALF / 8); q += A8_THREADS) {
    const int r = q / (HALF / 8), c = (q % (HALF / 8)) * 8;
    if (r < t.count)
      *(short8*)(act + (int64_t)row_pair[r] * I + n0 + c) =
          *(const short8*)(at + r * PITCH + c);
  }
}

template <int WM, int WN>
__global__ __launch_bounds__(A8_THREADS) void moe_down_fp8_a8_kernel(
    const unsigned char* __restrict__ aq, const float* __restrict__ sa_rows,
    const unsigned char* __restrict__ w2q, const float* __restrict__ w2s,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, const float* __restrict__ w,
    float* __restrict__ y2, int H, int I) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int STAGE = (BM + BN) * BK;
  static_assert(BM <= A8_THREADS, "one thread a tile row");
  static_assert(BM * 12 <= 2 * STAGE, "the row table fits the slab buffers");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

  if ((int)blockIdx.y >= *n_tiles) return;
  const Tile t = read_tile(tiles, blockIdx.y);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * BN;
  const int wm = (wave >> 1) * WM * 16, wn = (wave & 1) * WN * 16;

  const auto pair_of = [&](int r) { return perm[t.start + min(r, t.count - 1)]; };
  const int my_pair = pair_of(min((int)threadIdx.x, BM - 1));
  const float my_sa = sa_rows[my_pair], my_w = w[my_pair];

  Staging<WM> sa;
  Staging<WN> sb;
  sa.init_rows(aq, I, pair_of);
  // columns past H read row H - 1 instead and are never stored
  sb.init_rows(w2q, I,
               [&](int b) { return t.expert * H + min(n0 + b, H - 1); });
  f32x4 acc[WM][WN];
  gemm_slabs<WM, WN>(sa, sb, lds, acc, wm, wn, I);

  int* row_pair = (int*)lds;
  float* row_sa = (float*)(lds + BM * 4);
  float* row_w = (float*)(lds + BM * 8);
  if (threadIdx.x < BM) {
    row_pair[threadIdx.x] = my_pair;
    row_sa[threadIdx.x] = my_sa;
    row_w[threadIdx.x] = my_w;
  }
  __syncthreads();

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
  const int n = n0 + wn + (lane & 15);
  float sc[WN];
#pragma unroll
  for (int nb = 0; nb < WN; ++nb)
    sc[nb] = w2s[(int64_t)t.expert * H + min(n + nb * 16, H - 1)];
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm + mb * 16 + (lane >> 4) * 4 + j;
      if (r >= t.count) continue;
      const float sr = row_sa[r], wt = row_w[r];
      float* yr = y2 + (int64_t)row_pair[r] * H;
#pragma unroll
      for (int nb = 0; nb < WN; ++nb)
        if (n + nb * 16 < H)
          yr[n + nb * 16] = ((acc[mb][nb][j] * sr) * sc[nb]) * wt;
    }
}

template <int WM, int WN>
void launch_gate_up(const MoeFfnFp8A8Args& a, uint32_t n_tiles,
                  hipStream_t stream) {
  constexpr int BN = 32 * WN;
  hipLaunchKernelGGL((moe_gate_up_fp8_a8_kernel<WM, WN>),
                     dim3((uint32_t)(a.I / (BN / 2)), n_tiles),
                     dim3(A8_THREADS), 0, stream, (const unsigned char*)a.xq,
                     a.sx, (const unsigned char*)a.w13q, a.w13s, a.tiles,
                     a.n_tiles, a.perm, (short*)a.act, a.H, a.I, a.k);
}

template <int WM, int WN>
void launch_down(const MoeFfnFp8A8Args& a, uint32_t n_tiles,
                 hipStream_t stream) {
  constexpr int BN = 32 * WN;
  hipLaunchKernelGGL((moe_down_fp8_a8_kernel<WM, WN>),
                     dim3((uint32_t)((a.H + BN - 1) / BN), n_tiles),
                     dim3(A8_THREADS), 0, stream, (const unsigned char*)a.aq,
                     a.sa, (const unsigned char*)a.w2q, a.w2s, a.tiles,
                     a.n_tiles, a.perm, a.w, a.y2, a.H, a.I);
}

}  // namespace

hipError_t lds_moe_ffn_fp8_a8(const MoeFfnFp8A8Args& a, hipStream_t stream) {
  if (a.T == 0) return hipSuccess;
  if (a.tile != 64 && a.tile != 128) return hipErrorInvalidValue;
  const bool tall = a.tile == 128;
  const int64_t P = (int64_t)a.T * a.k;
  const uint32_t n_tiles = (uint32_t)moe_tile_bound(P, a.E, a.tile / 16);
  hipError_t err = lds_quantize_rows_fp8(a.x, a.xq, a.sx, a.T, a.H, stream);
  if (err != hipSuccess) return err;
  err = lds_moe_align(a.ids, a.tiles, a.n_tiles, a.perm, P, a.E, a.tile,
                      stream);
  if (err != hipSuccess) return err;
  if (tall) launch_gate_up<4, 4>(a, n_tiles, stream);
  else launch_gate_up<2, 2>(a, n_tiles, stream);
  HIP_CHECK_LAST();
  err = lds_quantize_rows_fp8(a.act, a.aq, a.sa, (int)P, a.I, stream);
  if (err != hipSuccess) return err;
  if (tall) launch_down<4, 4>(a, n_tiles, stream);
  else launch_down<2, 2>(a, n_tiles, stream);
  HIP_CHECK_LAST();
  return lds_moe_combine(a.y2, a.y, a.T, a.H, a.k, stream);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
