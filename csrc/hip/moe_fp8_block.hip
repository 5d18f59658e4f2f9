// moe_fp8_block.hip — the expert FFN of an MoE layer on block-scaled fp8
// experts (the recipe of the public DeepSeek-V3 / Qwen3-FP8 checkpoints):
// e4m3 weights with one fp32 scale per expert and 128 x 128 block, e4m3
// activations with one dynamic fp32 scale per row and 128-wide group of K,
// on the fp8 matrix instruction of gfx950. A pair is p = t k + j with
// e = ids[t, j]; sums over groups g of K, in order:
//   (xq, sx) = quantize_groups_fp8(x)                   per token and group
//   g = sum_g sx[t, g] * w13s[e, n / 128, g] * sum_{k in g} xq[t, k]
//       w13q[e, n, k], u the same on row I + n with the scale of the up
//       half, w13s[e, NBI + n / 128, g];  act[p, n] = bf16(silu(g) * u)
//   (aq, sa) = quantize_groups_fp8(act)                 per pair and group
//   y2[p, n] = (sum_g sa[p, g] * w2s[e, n / 128, g] * sum_{k in g} aq[p, k]
//              w2q[e, n, k]) * w[t, j]
//   y[t] = bf16(sum_j y2[t k + j])                      moe_combine_kernel
//
// x [T, H] bf16; w13q [E, 2 I, H], w2q [E, H, I] OCP e4m3, K contiguous;
// w13s [E, 2 NBI, G_H], w2s [E, NBH, G_I] fp32 with NBI = ceil(I / 128), NBH
// = ceil(H / 128), G_K = ceil(K / 128). The gate rows [0, I) and the up rows
// [I, 2 I) of w13 each start a grid of 128-row blocks of their own, as the
// checkpoints store gate_proj and up_proj. H % 64 == 0, I % 64 == 0 (the
// last group of either K may be 64 wide), T >= 1 here.
//
// The launch sequence is that of moe_fp8_a8.hip with the group quantiser of
// linear_fp8_block.hip in both places: quantise x, moe_align_kernel at the
// tile height, gate-up, quantise act over the P = T k pair rows, down,
// moe_combine_kernel. act, aq, sa and y2 live by pair. The second quantiser
// stays a pass of its own: a 128-wide group of act spans two to eight column
// workgroups of gate-up. The scales are stored group-major, sx [G_H, Tp] and
// sa [G_I, Pp] (launchers.h). The GEMM grids are launched at moe_tile_bound;
// a workgroup whose tile index is >= n_tiles returns at once, and nothing is
// read back by the host.
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 consumes exactly one group, so the
// promotion is one MFMA into a zeroed partial and acc = fma(partial, row
// scale * weight scale, acc) in fp32, as in linear_fp8_block.hip; the
// instruction's own e8m0 operands stay at 1. Two kernel families:
//
//   moe_gate_up_fp8_block_kernel, moe_down_fp8_block_kernel   64-row tiles
//     The <2, 2> kernels of moe_fp8_a8.hip (LDS-staged, fp8_tile.h) with the
//     promoting policy GatheredScales. Two things are theirs alone.
//     Gathered row scales: tile row r is token perm[start + r] / k in
//     gate-up and pair perm[start + r] in down, so a lane's four D rows are
//     four unrelated rows of sx and the dense kernel's one 16-byte load is
//     gone. Instead each of the first 64 threads owns one tile row, whose
//     row index it fetched once before the slab loop: it loads that row's
//     scale of slab s + 1 together with the operand loads of that slab and
//     parks it in a 64-float column behind the two operand stages, double
//     buffered like them. Past the slab's barrier a lane reads its four
//     scales with one 16-byte LDS read a row block.
//     Two weight scales a slab in gate-up: a wave's blocks nb < WN / 2 are
//     gate columns and the rest the up rows of the same columns, in
//     different halves of w13s. The workgroup's 32 act columns start at a
//     multiple of 32, so each half lies in one 128-row block: one gate and
//     one up scale a workgroup and slab, scalar loads one slab ahead, chosen
//     by nb in row_scales(mb, nb).
//     The epilogues are those of moe_fp8_a8.hip without the scale
//     multiplies. No 128-row tile is built: on the dense kernel the 128 tile
//     with promotion trailed the 64 tile at every measured shape
//     (profiles/linear_fp8_block.md), and nothing here makes the promotion
//     cheaper.
//
//   moe_skinny_fp8_block_kernel<GATE, NB, DEPTH>   16-row tiles, registers only
//     For decode-sized batches, after linear_fp8_block_skinny_kernel<1, NB>:
//     a workgroup of four waves owns one work-list tile of at most 16 pairs
//     and NB column blocks, and its waves take the groups of K round-robin.
//     Per group a lane loads the 32 bytes [32 (lane >> 4), +32) of row
//     lane & 15 of each weight block and of the gathered activation row,
//     straight into the MFMA operand registers; lanes past K in a 64-wide
//     tail hold zeros; rows past count read the last live row. A ring of
//     DEPTH stages (operands, the four D-row scales sx[g * Tp + row_j] and
//     the weight scale or scales) stays in flight over the MFMAs. The four
//     waves' accumulators are summed through LDS in wave order. In gate-up
//     the NB blocks are NB / 2 gate blocks and the up blocks of the same
//     columns, with two weight scales a stage, and silu(g) * u happens after
//     the wave sum. K is not split across workgroups: with one tile per
//     routed expert the grids already fill the machine (a Qwen3-30B-A3B
//     layer at T = 1: 8 tiles x 48 column blocks in gate-up, 8 x 64 in
//     down). The ring is written here, not shared with the dense kernel,
//     whose code stays as it is.
//
// Determinism: no atomic touches floating-point data and K is never split
// across workgroups. In the tiled kernels an element is one accumulator over
// the groups in order. In the skinny kernels the group -> wave assignment
// depends on K alone and the wave sum runs in wave order. MFMA rows and
// columns never mix, and the k a lane feeds to an instruction depends on the
// group alone. So within a kernel family the bits of a pair depend on its x
// row, its expert and its routing weight only: not on T, on the pair's place
// in its segment or on the other rows of the launch. The two families sum
// the groups in different orders: a row's bits may differ between batch
// sizes that moe_fp8_block_tile serves with different families, as for
// linear_fp8_block.
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
static_assert(GROUP == BK, "a slab of the tiled kernels is one group");

// What a kernel knows of its work-list tile.
struct Tile { int start, count, expert; };

__device__ __forceinline__ Tile read_tile(const int32_t* __restrict__ tiles,
                                          int tile) {
  return {tiles[tile * 3], tiles[tile * 3 + 1], tiles[tile * 3 + 2]};
}

__device__ __forceinline__ float silu_mul(float g, float u) {
  return g / (1.f + expf(-g)) * u;
}

// ---- 64-row tiles ----------------------------------------------------------

// The promoting policy of gemm_slabs for gathered rows. Thread r < BM owns
// tile row r: row is that row's scale column (sx + its row index), and its
// scale of the slab in flight goes to col[stage][r] in LDS when the slab's
// operands do. Column blocks nb < SPLIT use weight scale 0, the rest 1
// (SPLIT == WN: one scale).
template <int BM, int WN, int SPLIT>
struct GatheredScales {
  static constexpr bool promoted = true;
  const float* row;      // this thread's tile row, group 0 (threads < BM)
  const float* ws[2];    // the workgroup's row(s) of the weight scales: [G]
  float* col;            // LDS, [2][BM]
  int stride;            // Tp
  int rd, wr;            // stage the MFMA lanes read, stage written next
  float nxt_r, nxt_w[2], cur_w[2];

  __device__ __forceinline__ void fetch(int slab) {
    if (threadIdx.x < BM) nxt_r = row[(int64_t)slab * stride];
    nxt_w[0] = ws[0][slab];
    if constexpr (SPLIT < WN) nxt_w[1] = ws[1][slab];
  }
  __device__ __forceinline__ void advance() {
    if (threadIdx.x < BM) col[wr * BM + threadIdx.x] = nxt_r;
    cur_w[0] = nxt_w[0];
    if constexpr (SPLIT < WN) cur_w[1] = nxt_w[1];
    rd = wr;
    wr ^= 1;
  }
  // D rows (lane >> 4) * 4 + j of the row block at tile row wm + 16 mb
  __device__ __forceinline__ f32x4 row_scales(int mb, int nb) const {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int r = (wave >> 1) * (BM / 2) + mb * 16 + (lane >> 4) * 4;
    const f32x4 s = *(const f32x4*)(col + rd * BM + r);
    const float w = cur_w[SPLIT < WN && nb >= SPLIT ? 1 : 0];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = s[j] * w;
    return o;
  }
};

template <int WM, int WN>
__global__ __launch_bounds__(A8_THREADS) void moe_gate_up_fp8_block_kernel(
    const unsigned char* __restrict__ xq, const float* __restrict__ sx,
    const unsigned char* __restrict__ w13q, const float* __restrict__ w13s,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, short* __restrict__ act, int Tp, int H,
    int I, int k) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int HALF = BN / 2;    // act columns of the workgroup
  constexpr int WH = WN * 8;      // act columns of a wave
  constexpr int STAGE = (BM + BN) * BK;
  constexpr int PITCH = HALF + 8;  // shorts: rows of the act tile stay 16-byte aligned
  constexpr int ROWS_OFF = BM * PITCH * 2;  // row_pair behind the act tile
  static_assert(WN % 2 == 0, "a wave holds gate and up blocks in pairs");
  static_assert(BM <= A8_THREADS, "one thread a tile row");
  static_assert(GROUP % HALF == 0, "each half lies in one 128-row block");
  static_assert(ROWS_OFF % 16 == 0 && ROWS_OFF + BM * 4 <= 2 * STAGE,
                "the act tile and the row table fit the slab buffers");
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[2 * STAGE + 2 * BM * 4];

  if ((int)blockIdx.y >= *n_tiles) return;
  const Tile t = read_tile(tiles, blockIdx.y);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * HALF;
  const int wm = (wave >> 1) * WM * 16, wn = (wave & 1) * WN * 16;
  const int G = (H + GROUP - 1) / GROUP, NBI = (I + GROUP - 1) / GROUP;

  // Rows past count read the last live row instead (count >= 1): MFMA rows
  // never mix, and nothing of theirs is stored.
  const auto pair_of = [&](int r) { return perm[t.start + min(r, t.count - 1)]; };
  const int my_pair = pair_of(min((int)threadIdx.x, BM - 1));

  Staging<WM> sa;
  Staging<WN> sb;
  sa.init_rows(xq, H, [&](int r) { return pair_of(r) / k; });
  sb.init_rows(w13q, H, [&](int b) {
    const int q = b % (2 * WH);
    const int col = n0 + (b / (2 * WH)) * WH + q % WH;
    return t.expert * 2 * I + col + (q >= WH ? I : 0);
  });
  GatheredScales<BM, WN, WN / 2> p;
  p.row = sx + my_pair / k;
  p.ws[0] = w13s + ((int64_t)t.expert * 2 * NBI + n0 / GROUP) * G;
  p.ws[1] = p.ws[0] + (int64_t)NBI * G;
  p.col = (float*)(lds + 2 * STAGE);
  p.stride = Tp;
  p.rd = p.wr = 0;
  f32x4 acc[WM][WN];
  gemm_slabs<WM, WN>(sa, sb, lds, acc, wm, wn, H, p);

  short* at = (short*)lds;
  int* row_pair = (int*)(lds + ROWS_OFF);
  if (threadIdx.x < BM) row_pair[threadIdx.x] = my_pair;

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
  const int wc = (wave & 1) * WH + (lane & 15);  // act column in the tile
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm + mb * 16 + (lane >> 4) * 4 + j;
#pragma unroll
      for (int nb = 0; nb < WN / 2; ++nb)
        at[r * PITCH + wc + nb * 16] = f32_to_bf16(
            silu_mul(acc[mb][nb][j], acc[mb][WN / 2 + nb][j]));
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
__global__ __launch_bounds__(A8_THREADS) void moe_down_fp8_block_kernel(
    const unsigned char* __restrict__ aq, const float* __restrict__ sa_rows,
    const unsigned char* __restrict__ w2q, const float* __restrict__ w2s,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, const float* __restrict__ w,
    float* __restrict__ y2, int Pp, int H, int I) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int STAGE = (BM + BN) * BK;
  static_assert(BM <= A8_THREADS, "one thread a tile row");
  static_assert(GROUP % BN == 0, "a tile lies in one 128-row weight block");
  static_assert(BM * 8 <= 2 * STAGE, "the row table fits the slab buffers");
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[2 * STAGE + 2 * BM * 4];

  if ((int)blockIdx.y >= *n_tiles) return;
  const Tile t = read_tile(tiles, blockIdx.y);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * BN;
  const int wm = (wave >> 1) * WM * 16, wn = (wave & 1) * WN * 16;
  const int G = (I + GROUP - 1) / GROUP, NBH = (H + GROUP - 1) / GROUP;

  const auto pair_of = [&](int r) { return perm[t.start + min(r, t.count - 1)]; };
  const int my_pair = pair_of(min((int)threadIdx.x, BM - 1));
  const float my_w = w[my_pair];

  Staging<WM> sa;
  Staging<WN> sb;
  sa.init_rows(aq, I, pair_of);
  // columns past H read row H - 1 instead and are never stored
  sb.init_rows(w2q, I,
               [&](int b) { return t.expert * H + min(n0 + b, H - 1); });
  GatheredScales<BM, WN, WN> p;
  p.row = sa_rows + my_pair;
  p.ws[0] = p.ws[1] = w2s + ((int64_t)t.expert * NBH + n0 / GROUP) * G;
  p.col = (float*)(lds + 2 * STAGE);
  p.stride = Pp;
  p.rd = p.wr = 0;
  f32x4 acc[WM][WN];
  gemm_slabs<WM, WN>(sa, sb, lds, acc, wm, wn, I, p);

  int* row_pair = (int*)lds;
  float* row_w = (float*)(lds + BM * 4);
  if (threadIdx.x < BM) {
    row_pair[threadIdx.x] = my_pair;
    row_w[threadIdx.x] = my_w;
  }
  __syncthreads();

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
  const int n = n0 + wn + (lane & 15);
#pragma unroll
  for (int mb = 0; mb < WM; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm + mb * 16 + (lane >> 4) * 4 + j;
      if (r >= t.count) continue;
      const float wt = row_w[r];
      float* yr = y2 + (int64_t)row_pair[r] * H;
#pragma unroll
      for (int nb = 0; nb < WN; ++nb)
        if (n + nb * 16 < H) yr[n + nb * 16] = acc[mb][nb][j] * wt;
    }
}

// ---- 16-row skinny kernels -------------------------------------------------

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / WAVE;
constexpr int SK_TILE = 16;   // rows of a work-list tile: one MFMA row block

// Column blocks of a skinny workgroup, both kernels. By registers and
// reasoning, not by a sweep: a ring stage holds 2 (NB + 1) 16-byte loads, the
// four row scales and the weight scales of a lane, 30 registers at NB = 2. NB
// = 4 would read the gathered rows half as often but halve the workgroups of
// a decode step, which at one short tile per routed expert is what fills the
// machine (8 x 48 and 8 x 64 workgroups on a Qwen3-30B-A3B layer at T = 1).
constexpr int SK_NB = 2;
// Stages in flight. By the compiler's register count, not measured against
// other depths: at 4 stages (the depth of linear_fp8_block_skinny_kernel<1,
// 2>) both kernels take more than 256 registers a lane and one wave a SIMD;
// at 3 they stay within 256 and two workgroups share a SIMD, six groups in
// flight there instead of four.
constexpr int SK_DEPTH = 3;

// One ring stage: a group's weight bytes (32 a column block) and codes of this
// lane, the scales of its four D rows and the weight scale(s).
template <int NB>
struct SkStage {
  u32x4 w[NB][2];
  u32x4 x[2];
  float sx[4];
  float ws[2];
};

// What a lane reads of every group: operand rows at its 32-byte column kq,
// the scale columns of its four D rows, the workgroup's row(s) of the weight
// scales.
template <int NB>
struct SkSource {
  const unsigned char* wp[NB];
  const unsigned char* xp;
  const float* sxp[4];
  const float* ws[2];
  int kq, in, stride;
};

template <bool GATE, int NB>
__device__ __forceinline__ void sk_load(SkStage<NB>& s, const SkSource<NB>& src,
                                        int g) {
  const int64_t k = (int64_t)g * GROUP;
  // K % 64 == 0: a lane's 32 bytes are below K or past it together
  const bool live = g * GROUP + src.kq < src.in;
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    s.w[nb][0] = live ? *(const u32x4*)(src.wp[nb] + k) : zero;
    s.w[nb][1] = live ? *(const u32x4*)(src.wp[nb] + k + 16) : zero;
  }
  s.x[0] = live ? *(const u32x4*)(src.xp + k) : zero;
  s.x[1] = live ? *(const u32x4*)(src.xp + k + 16) : zero;
#pragma unroll
  for (int j = 0; j < 4; ++j) s.sx[j] = src.sxp[j][(int64_t)g * src.stride];
  s.ws[0] = src.ws[0][g];
  s.ws[1] = GATE ? src.ws[1][g] : s.ws[0];
}

__device__ __forceinline__ i32x8 sk_operand(const u32x4 (&h)[2]) {
  union { u32x4 h[2]; i32x8 v; } u;
  u.h[0] = h[0];
  u.h[1] = h[1];
  return u.v;
}

// One turn of the ring: stages i .. i + DEPTH - 1 go through the matrix core,
// and each slot is refilled with the stage DEPTH later once its MFMAs have
// read it. TAIL checks every stage against n_it.
template <bool GATE, int NB, int DEPTH, bool TAIL>
__device__ __forceinline__ void sk_round(SkStage<NB> (&ring)[DEPTH],
                                         f32x4 (&acc)[NB],
                                         const SkSource<NB>& src, int g0,
                                         int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
    const i32x8 a = sk_operand(ring[d].x);
    f32x4 part[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      part[nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          a, sk_operand(ring[d].w[nb]), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0,
          E8M0_ONE, 0, E8M0_ONE);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float ws = ring[d].ws[GATE && nb >= NB / 2 ? 1 : 0];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[nb][j] =
            __builtin_fmaf(part[nb][j], ring[d].sx[j] * ws, acc[nb][j]);
    }
    if (!TAIL || i + d + DEPTH < n_it)
      sk_load<GATE>(ring[d], src, g0 + (i + d + DEPTH) * SK_WAVES);
    // a stage's MFMAs and adds stay in front of the next stage's wait
    __builtin_amdgcn_sched_barrier(0);
  }
}

// GATE: rows of xq gathered by perm[.] / k against NB / 2 gate blocks and the
// up blocks of the same columns of w13q[e]; out = act [P, I] bf16, N = I.
// Else: rows of aq gathered by perm[.] against NB blocks of w2q[e]; out = y2
// [P, H] fp32 times w[pair], N = H. K is the depth (H or I), stride the
// padded row count of the activation scales.
template <bool GATE, int NB, int DEPTH>
__global__ __launch_bounds__(SK_THREADS) void moe_skinny_fp8_block_kernel(
    const unsigned char* __restrict__ xq, const float* __restrict__ sx,
    const unsigned char* __restrict__ wq, const float* __restrict__ wscale,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, const float* __restrict__ w,
    void* __restrict__ out, int stride, int K, int N, int k) {
  constexpr int BN = (GATE ? NB / 2 : NB) * 16;   // output columns
  static_assert(!GATE || NB % 2 == 0, "gate and up blocks come in pairs");
  static_assert(GROUP % BN == 0, "a column block lies in one weight block");
  __shared__ float red[SK_WAVES][NB][4][WAVE];
  __shared__ int row_pair[SK_TILE];

  if ((int)blockIdx.y >= *n_tiles) return;
  const Tile t = read_tile(tiles, blockIdx.y);
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * BN;
  const int r = lane & 15;
  const int G = (K + GROUP - 1) / GROUP, NBN = (N + GROUP - 1) / GROUP;

  // Rows past count read the last live row instead (count >= 1): MFMA rows
  // never mix, and nothing of theirs is stored. N % BN == 0: every column
  // block is whole.
  const auto pair_of = [&](int m) { return perm[t.start + min(m, t.count - 1)]; };
  const auto row_of = [&](int m) { return GATE ? pair_of(m) / k : pair_of(m); };
  if (threadIdx.x < SK_TILE) row_pair[threadIdx.x] = pair_of(threadIdx.x);

  SkSource<NB> src;
  src.kq = (lane >> 4) * 32;
  src.in = K;
  src.stride = stride;
  src.xp = xq + (int64_t)row_of(r) * K + src.kq;
#pragma unroll
  for (int j = 0; j < 4; ++j) src.sxp[j] = sx + row_of((lane >> 4) * 4 + j);
  if (GATE) {
    src.ws[0] = wscale + ((int64_t)t.expert * 2 * NBN + n0 / GROUP) * G;
    src.ws[1] = src.ws[0] + (int64_t)NBN * G;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int row = (nb >= NB / 2 ? N : 0) + n0 + (nb % (NB / 2)) * 16 + r;
      src.wp[nb] = wq + ((int64_t)t.expert * 2 * N + row) * K + src.kq;
    }
  } else {
    src.ws[0] = src.ws[1] =
        wscale + ((int64_t)t.expert * NBN + n0 / GROUP) * G;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      src.wp[nb] =
          wq + ((int64_t)t.expert * N + n0 + nb * 16 + r) * K + src.kq;
  }

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this wave's groups: wave, wave + 4, ... below G
  const int g0 = wave;
  const int n_it = (G - g0 + SK_WAVES - 1) / SK_WAVES;  // may be 0

  SkStage<NB> ring[DEPTH];
  int i = 0;
  if (n_it >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      sk_load<GATE>(ring[d], src, g0 + d * SK_WAVES);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_it; i += DEPTH)
      sk_round<GATE, NB, DEPTH, false>(ring, acc, src, g0, i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it) sk_load<GATE>(ring[d], src, g0 + d * SK_WAVES);
  }
  for (; i < n_it; i += DEPTH)
    sk_round<GATE, NB, DEPTH, true>(ring, acc, src, g0, i, n_it);

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wave][nb][j][lane] = acc[nb][j];
  __syncthreads();
  // element (m, block nb, column c of the block), summed in wave order
  const auto total = [&](int m, int nb, int c) {
    const int l = (m >> 2) * 16 + c;
    float v = red[0][nb][m & 3][l];
#pragma unroll
    for (int wv = 1; wv < SK_WAVES; ++wv) v += red[wv][nb][m & 3][l];
    return v;
  };
  if (GATE) {
    short* act = (short*)out;
    for (int q = threadIdx.x; q < t.count * BN; q += SK_THREADS) {
      const int m = q / BN, c = q % BN;
      act[(int64_t)row_pair[m] * N + n0 + c] = f32_to_bf16(silu_mul(
          total(m, c >> 4, c & 15), total(m, NB / 2 + (c >> 4), c & 15)));
    }
  } else {
    float* y2 = (float*)out;
    for (int q = threadIdx.x; q < t.count * (BN / 4); q += SK_THREADS) {
      const int m = q / (BN / 4), c = (q % (BN / 4)) * 4;
      const int p = row_pair[m];
      const float wt = w[p];
      f32x4 s;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        s[e] = total(m, c >> 4, (c & 15) + e) * wt;
      *(f32x4*)(y2 + (int64_t)p * N + n0 + c) = s;
    }
  }
}

void launch_tiled(const MoeFfnFp8BlockArgs& a, uint32_t n_tiles, bool gate,
                  hipStream_t stream) {
  if (gate)
    hipLaunchKernelGGL((moe_gate_up_fp8_block_kernel<2, 2>),
                       dim3((uint32_t)(a.I / 32), n_tiles), dim3(A8_THREADS),
                       0, stream, (const unsigned char*)a.xq, a.sx,
                       (const unsigned char*)a.w13q, a.w13s, a.tiles,
                       a.n_tiles, a.perm, (short*)a.act,
                       linear_fp8_block_tp(a.T), a.H, a.I, a.k);
  else
    hipLaunchKernelGGL((moe_down_fp8_block_kernel<2, 2>),
                       dim3((uint32_t)((a.H + 63) / 64), n_tiles),
                       dim3(A8_THREADS), 0, stream,
                       (const unsigned char*)a.aq, a.sa,
                       (const unsigned char*)a.w2q, a.w2s, a.tiles, a.n_tiles,
                       a.perm, a.w, a.y2, linear_fp8_block_tp(a.T * a.k), a.H,
                       a.I);
}

void launch_skinny(const MoeFfnFp8BlockArgs& a, uint32_t n_tiles, bool gate,
                   hipStream_t stream) {
  if (gate)
    hipLaunchKernelGGL(
        (moe_skinny_fp8_block_kernel<true, SK_NB, SK_DEPTH>),
        dim3((uint32_t)(a.I / (SK_NB * 8)), n_tiles), dim3(SK_THREADS), 0,
        stream, (const unsigned char*)a.xq, a.sx,
        (const unsigned char*)a.w13q, a.w13s, a.tiles, a.n_tiles, a.perm, a.w,
        a.act, linear_fp8_block_tp(a.T), a.H, a.I, a.k);
  else
    hipLaunchKernelGGL(
        (moe_skinny_fp8_block_kernel<false, SK_NB, SK_DEPTH>),
        dim3((uint32_t)(a.H / (SK_NB * 16)), n_tiles), dim3(SK_THREADS), 0,
        stream, (const unsigned char*)a.aq, a.sa,
        (const unsigned char*)a.w2q, a.w2s, a.tiles, a.n_tiles, a.perm, a.w,
        (void*)a.y2, linear_fp8_block_tp(a.T * a.k), a.I, a.H, a.k);
}

}  // namespace

hipError_t lds_moe_ffn_fp8_block(const MoeFfnFp8BlockArgs& a,
                                 hipStream_t stream) {
  if (a.T == 0) return hipSuccess;
  if (a.tile != SK_TILE && a.tile != 64) return hipErrorInvalidValue;
  const bool skinny = a.tile == SK_TILE;
  const int64_t P = (int64_t)a.T * a.k;
  const uint32_t n_tiles = (uint32_t)moe_tile_bound(P, a.E, a.tile / 16);
  hipError_t err = lds_quantize_groups_fp8(a.x, a.xq, a.sx, a.T, a.H, stream);
  if (err != hipSuccess) return err;
  err = lds_moe_align(a.ids, a.tiles, a.n_tiles, a.perm, P, a.E, a.tile,
                      stream);
  if (err != hipSuccess) return err;
  if (skinny) launch_skinny(a, n_tiles, true, stream);
  else launch_tiled(a, n_tiles, true, stream);
  HIP_CHECK_LAST();
  err = lds_quantize_groups_fp8(a.act, a.aq, a.sa, (int)P, a.I, stream);
  if (err != hipSuccess) return err;
  if (skinny) launch_skinny(a, n_tiles, false, stream);
  else launch_tiled(a, n_tiles, false, stream);
  HIP_CHECK_LAST();
  return lds_moe_combine(a.y2, a.y, a.T, a.H, a.k, stream);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
