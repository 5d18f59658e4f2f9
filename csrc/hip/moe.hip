// moe.hip — mixture-of-experts FFN for gfx950, bf16:
//   ids, w = top-k of softmax(x · routerᵀ)                      (moe_route)
//   y[t] = bf16(sum_j w[t, j] * (bf16(silu(x[t] Wg_e) * (x[t] Wu_e)) W2_e)),
//          e = ids[t, j]                                         (moe_ffn)
//
// x [T, H]; router [E, H]; w13 [E, 2 I, H] (gate rows 0..I-1, up rows
// I..2I-1); w2 [E, H, I]: every matrix operand is K contiguous, so the eight
// consecutive k a lane feeds mfma_f32_16x16x32_bf16 are one 16-byte load
// straight from global memory. Routing, the work list and both GEMMs stay on
// the device: nothing here is read back by the host.
//
//   moe_route_kernel        one workgroup per 16 tokens. Token on the MFMA
//     row, expert on the column. The four waves take the 16-expert column
//     blocks round-robin, each over the whole K (a logit is one wave's sum),
//     up to four blocks a wave at once so x is loaded once per K step. Logits
//     go to LDS [16][E]; each wave then takes four tokens: wave max and sum,
//     k rounds of wave arg-max ordered by (value, -index), renormalise.
//   moe_align_kernel        one workgroup. LDS histogram of the P = T k
//     (token, slot) pairs over experts, exclusive scan with every count
//     padded to the tile height TM = 16 MB, then tiles [n, 3] = (start,
//     count <= TM, expert), n_tiles, and perm: sorted position -> pair. A
//     pair's place inside its expert's segment comes from an LDS integer
//     atomic and may differ from run to run (see Determinism).
//   moe_gate_up_kernel<MB>  grid (column block of I, tile). A workgroup owns
//     32 gate columns and the same 32 up columns of one expert for the
//     tile's rows, gathered through perm[.] / k.
//   moe_down_kernel<MB>     grid (column block of H, tile). act rows (by
//     sorted position, contiguous) times w2[e]; the epilogue multiplies by
//     the pair's routing weight and stores fp32 y2[pair, H].
//   moe_combine_kernel      y[t] = bf16(sum_j y2[t k + j]) in slot order.
//
// Both GEMM kernels share gemm_core, the skeleton of linear_fp8_kernel: the
// waves take 32-wide K steps round-robin, a register ring keeps the loads of
// the next DEPTH steps in flight over the current MFMAs, and the four waves'
// accumulators are summed through LDS in wave order. K is never split across
// workgroups: tiles x column blocks fill the chip at MoE shapes. The GEMM
// grids are launched at the host-known bound moe_tile_bound; a workgroup
// whose tile index is >= n_tiles returns at once.
//
// MXFP4 experts (moe_ffn_mxfp4): w13q [E, 2 I, H / 2] and w2q [E, H, I / 2]
// uint8, two e2m1 codes a byte with k = 2j in the low nibble, and w13s
// [E, 2 I, H / 32], w2s [E, H, I / 32] uint8, one e8m0 exponent per 32 k: the
// pair of ops.ref.quantize_weight_mxfp4 per expert. x, act, y2 and y are as
// above, and so are the work list, the tiles, the epilogues and the combine.
//   moe_gate_up_mxfp4_kernel<MB>, moe_down_mxfp4_kernel<MB>   the same grids.
//     What changes is the K loop (mx_gemm_core): its unit is that of
//     linear_mxfp4_kernel. A stage is a 128-wide K block; lane group
//     g = lane >> 4 owns MX group g of it. One 16-byte load is the 32 codes
//     of weight row lane & 15 in that group, one byte load is their scale,
//     and four 16-byte loads are the lane's x row at the same 32 k. Dword q
//     of the codes goes through four v_cvt_scalef32_pk_bf16_fp4 with the
//     scale as operand and is the B operand of MFMA q; the MFMA sums over its
//     four lane groups whatever k each brings, so a lane only multiplies k of
//     its own group and the scale costs no instruction. The waves take the K
//     blocks round-robin, a register ring keeps the next DEPTH blocks in
//     flight, and the accumulators meet in LDS as above.
//   K tail. K % 32 == 0 is all that is asked (gpt-oss: 2880 = 22 * 128 + 64).
//     The last K block may hold one to three groups: a lane group past K
//     issues no load and feeds zeros on both operands.
//   Tile height. A stage is 5 NW + 16 MB registers a lane: 36 and 52 for
//     gate-up (NW 4) at MB 1 and 2, 26 and 42 for down. At MB 4 a stage would
//     be 84: no ring fits next to 64 accumulators. So the MXFP4 work list is
//     built with MB <= 2 (moe_mxfp4_mb): a taller segment walks more tiles,
//     and its weights come from L2 after the first. A pair's bits do not
//     depend on that choice either.
//
// fp8 experts (moe_ffn_fp8): w13q [E, 2 I, H] and w2q [E, H, I] OCP e4m3, and
// w13s [E, 2 I], w2s [E, H] fp32, one scale per expert and output channel:
// the pair of ops.ref.quantize_weight_fp8 per expert. Everything else is as
// for bf16 experts, tile heights (moe_mb) and scratch included.
//   moe_gate_up_fp8_kernel<MB>, moe_down_fp8_kernel<MB>   the same grids.
//     What changes is the K loop (fp8_gemm_core): its unit is that of
//     linear_fp8_kernel. A stage is a 64-wide K block; lane group
//     g = lane >> 4 owns k = 64 b + 16 g .. + 15 of it. One 16-byte load is
//     those 16 bytes of weight row lane & 15, two 16-byte loads are the
//     lane's x row at the same k. Bytes 0..7 and 8..15 go through
//     v_cvt_scalef32_pk_bf16_fp8 with scale 1, which is exact, and are the B
//     operands of two MFMAs; x is read in the same order, so the k order
//     inside a step is permuted alike on both operands. The waves take the K
//     blocks round-robin, a register ring keeps the next DEPTH blocks in
//     flight, and the accumulators meet in LDS as above. Every weight byte is
//     read once, as fp8, by the one wave that uses it.
//   K tail. K % 16 == 0 is all that is asked (H % 32 and I % 16, as for bf16
//     experts). The last K block may hold one to three lane groups: a lane
//     group past K issues no load and feeds zeros on both operands. The
//     straight-line turns of the ring cover whole blocks only and carry no
//     predicate.
//   Scales. In the epilogues only, in this order. Gate-up: the fp32 sums of
//     gate column n and up column n times w13s[e, n] and w13s[e, I + n], then
//     silu(g) * u and the one bf16 rounding of act. Down: the fp32 sum times
//     w2s[e, n], then times the pair's routing weight, stored fp32 in y2.
//   Tile height. A stage is 4 NW + 8 MB registers a lane: 24 / 32 / 48 for
//     gate-up at MB 1 / 2 / 4, 16 / 24 / 40 for down. MB 4 fits next to 64
//     accumulators with a ring of two stages (three for down), without
//     scratch, so nothing is capped. The depths are register arithmetic, not
//     swept.
//
// Determinism: no atomic touches floating-point data. The bits of a pair
// depend on its x row, its expert and its routing weight only: MFMA rows and
// columns never mix, the K step -> wave assignment depends on K alone and
// every reduction runs in a fixed order. They do not depend on T, on MB, on
// the pair's position in its segment or on the other rows of the launch.
#include "hip_common.h"
#include "launchers.h"
#include "fp8_convert.h"
#include "mxfp4_convert.h"

// Built without packed fp32 arithmetic, as linear_fp8.hip is and for the
// reason given there.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int MOE_THREADS = 256;
constexpr int MOE_WAVES = MOE_THREADS / WAVE;
constexpr int MOE_KSTEP = 32;    // k of one MFMA
constexpr int MOE_NB = 2;        // 16-column blocks of a GEMM workgroup
constexpr int MOE_BN = MOE_NB * 16;

__device__ __forceinline__ short8 load8_or_zero(const short* p, bool ok) {
  short8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *(const short8*)p : z;
}

// ---- routing -------------------------------------------------------------

constexpr int ROUTE_CB = MOE_MAX_EXPERTS / 16 / MOE_WAVES;  // blocks a wave
constexpr int ROUTE_EPL = MOE_MAX_EXPERTS / WAVE;           // experts a lane
constexpr int ROUTE_UNROLL = 4;                             // K steps a turn

__global__ __launch_bounds__(MOE_THREADS) void moe_route_kernel(
    const short* __restrict__ x, const short* __restrict__ router,
    int32_t* __restrict__ ids, float* __restrict__ w, int T, int H, int E,
    int k, int renorm) {
  __shared__ float logit[MOE_ROUTE_TOKENS][MOE_MAX_EXPERTS];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int t0 = blockIdx.x * MOE_ROUTE_TOKENS;
  const int r = lane & 15, kq = (lane >> 4) * 8;
  const int n_cb = (E + 15) / 16;

  // Tokens past T and experts past E read a valid row instead: MFMA rows and
  // columns never mix, and nothing of theirs is stored.
  const short* xp = x + (int64_t)min(t0 + r, T - 1) * H + kq;
  const short* rp[ROUTE_CB];
#pragma unroll
  for (int c = 0; c < ROUTE_CB; ++c)
    rp[c] = router +
            (int64_t)min((wave + c * MOE_WAVES) * 16 + r, E - 1) * H + kq;
  f32x4 acc[ROUTE_CB];
#pragma unroll
  for (int c = 0; c < ROUTE_CB; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // ROUTE_UNROLL K steps a turn, every load ahead of the first MFMA: at
  // T <= 16 one workgroup streams the whole router, and what it waits for is
  // the latency of each load. The k order of a logit's sum does not change.
  int kk = 0;
  for (; kk + ROUTE_UNROLL * MOE_KSTEP <= H; kk += ROUTE_UNROLL * MOE_KSTEP) {
    short8 a[ROUTE_UNROLL], b[ROUTE_CB][ROUTE_UNROLL];
#pragma unroll
    for (int u = 0; u < ROUTE_UNROLL; ++u)
      a[u] = *(const short8*)(xp + kk + u * MOE_KSTEP);
#pragma unroll
    for (int c = 0; c < ROUTE_CB; ++c)
      if (wave + c * MOE_WAVES < n_cb) {
#pragma unroll
        for (int u = 0; u < ROUTE_UNROLL; ++u)
          b[c][u] = *(const short8*)(rp[c] + kk + u * MOE_KSTEP);
      }
#pragma unroll
    for (int u = 0; u < ROUTE_UNROLL; ++u)
#pragma unroll
      for (int c = 0; c < ROUTE_CB; ++c)
        if (wave + c * MOE_WAVES < n_cb)
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[c][u],
                                                           acc[c], 0, 0, 0);
  }
  for (; kk < H; kk += MOE_KSTEP) {
    const short8 a = *(const short8*)(xp + kk);
#pragma unroll
    for (int c = 0; c < ROUTE_CB; ++c) {
      if (wave + c * MOE_WAVES < n_cb) {  // wave-uniform
        const short8 b = *(const short8*)(rp[c] + kk);
        acc[c] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[c], 0, 0, 0);
      }
    }
  }
  // D of the MFMA: column (expert) = lane & 15, row (token) = (lane >> 4) * 4 + j
#pragma unroll
  for (int c = 0; c < ROUTE_CB; ++c) {
    const int e = (wave + c * MOE_WAVES) * 16 + r;
    if (e < E)
#pragma unroll
      for (int j = 0; j < 4; ++j) logit[(lane >> 4) * 4 + j][e] = acc[c][j];
  }
  __syncthreads();

  for (int i = 0; i < MOE_ROUTE_TOKENS / MOE_WAVES; ++i) {
    const int tl = wave * (MOE_ROUTE_TOKENS / MOE_WAVES) + i;
    const int t = t0 + tl;
    if (t >= T) break;  // wave-uniform
    // this lane's experts: lane, lane + 64, ...; -inf past E
    float v[ROUTE_EPL];
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < ROUTE_EPL; ++q) {
      const int e = lane + q * WAVE;
      v[q] = e < E ? logit[tl][e] : -INFINITY;
      mx = fmaxf(mx, v[q]);
    }
    mx = wave_reduce_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < ROUTE_EPL; ++q)
      sum += lane + q * WAVE < E ? expf(v[q] - mx) : 0.f;
    sum = wave_reduce_sum(sum);

    unsigned taken = 0;   // bit q: this lane's expert q is already chosen
    int sel_e[MOE_MAX_TOPK];
    float sel_w[MOE_MAX_TOPK];
    float chosen = 0.f;
#pragma unroll
    for (int j = 0; j < MOE_MAX_TOPK; ++j) {
      if (j >= k) continue;
      // best of this lane, then of the wave: larger value, then lower index.
      // be < 0: no candidate. k <= E, so the wave always has one.
      float bv = -INFINITY;
      int be = -1;
#pragma unroll
      for (int q = 0; q < ROUTE_EPL; ++q) {
        const int e = lane + q * WAVE;
        if (e < E && !(taken >> q & 1) && (be < 0 || v[q] > bv)) {
          bv = v[q];
          be = e;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, WAVE);
        const int oe = __shfl_xor(be, off, WAVE);
        if (oe >= 0 && (be < 0 || ov > bv || (ov == bv && oe < be))) {
          bv = ov;
          be = oe;
        }
      }
      // one answer for the wave even where a NaN logit breaks the ordering
      bv = __shfl(bv, 0, WAVE);
      be = __shfl(be, 0, WAVE);
      if ((be & (WAVE - 1)) == lane) taken |= 1u << (be / WAVE);
      sel_e[j] = be;
      sel_w[j] = expf(bv - mx) / sum;
      chosen += sel_w[j];
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < MOE_MAX_TOPK; ++j) {
        if (j >= k) continue;
        ids[(int64_t)t * k + j] = sel_e[j];
        w[(int64_t)t * k + j] = renorm ? sel_w[j] / chosen : sel_w[j];
      }
    }
  }
}

// ---- work list -----------------------------------------------------------

__device__ __forceinline__ int clamp_expert(int e, int E) {
  return min(max(e, 0), E - 1);
}

// One workgroup of MOE_MAX_EXPERTS threads: thread e owns expert e.
__global__ __launch_bounds__(MOE_MAX_EXPERTS) void moe_align_kernel(
    const int32_t* __restrict__ ids, int32_t* __restrict__ tiles,
    int32_t* __restrict__ n_tiles, int32_t* __restrict__ perm, int P, int E,
    int TM) {
  __shared__ int cnt[MOE_MAX_EXPERTS];     // pairs of the expert
  __shared__ int seg[MOE_MAX_EXPERTS];     // start of its padded segment
  __shared__ int cursor[MOE_MAX_EXPERTS];  // pairs placed so far
  __shared__ int wave_sum[MOE_MAX_EXPERTS / WAVE];
  const int e = threadIdx.x, wave = e / WAVE, lane = e % WAVE;
  cnt[e] = 0;
  cursor[e] = 0;
  __syncthreads();
  for (int p = e; p < P; p += MOE_MAX_EXPERTS)
    atomicAdd(&cnt[clamp_expert(ids[p], E)], 1);
  __syncthreads();
  // exclusive scan of the padded counts: inside a wave, then across waves
  const int c = e < E ? cnt[e] : 0;
  const int padded = (c + TM - 1) / TM * TM;
  int incl = padded;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int o = __shfl_up(incl, off, WAVE);
    if (lane >= off) incl += o;
  }
  if (lane == WAVE - 1) wave_sum[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < wave; ++i) base += wave_sum[i];
  const int start = base + incl - padded;
  seg[e] = start;
  for (int i = 0; i * TM < c; ++i) {
    int32_t* tp = tiles + (int64_t)(start / TM + i) * 3;
    tp[0] = start + i * TM;
    tp[1] = min(TM, c - i * TM);
    tp[2] = e;
  }
  if (e == MOE_MAX_EXPERTS - 1) *n_tiles = (start + padded) / TM;
  __syncthreads();
  for (int p = e; p < P; p += MOE_MAX_EXPERTS) {
    const int ex = clamp_expert(ids[p], E);
    perm[seg[ex] + atomicAdd(&cursor[ex], 1)] = p;
  }
}

// ---- the two expert GEMMs ------------------------------------------------

// One ring stage: a K step's NW weight rows and MB x rows of this lane.
template <int MB, int NW>
struct Stage {
  short8 w[NW];
  short8 x[MB];
};

// KPRED: K is a multiple of 16 only, and the lanes of the last step whose k
// is past it feed zeros on both operands. Otherwise K % 32 == 0.
template <int MB, int NW, bool KPRED>
__device__ __forceinline__ void load_stage(
    Stage<MB, NW>& s, const short* const (&wp)[NW],
    const short* const (&xp)[MB], int step, int k_left) {
  const int k = step * MOE_KSTEP;
  const bool ok = !KPRED || k < k_left;
#pragma unroll
  for (int n = 0; n < NW; ++n) s.w[n] = load8_or_zero(wp[n] + k, ok);
#pragma unroll
  for (int m = 0; m < MB; ++m) s.x[m] = load8_or_zero(xp[m] + k, ok);
}

// One turn of the ring, as in linear_fp8.hip: stages i .. i + DEPTH - 1 go
// through the matrix core and each slot is refilled with the stage DEPTH
// later. TAIL = false is straight-line code; the last turns check every
// stage against n_it.
template <int MB, int NW, int DEPTH, bool KPRED, bool TAIL>
__device__ __forceinline__ void ring_round(
    Stage<MB, NW> (&ring)[DEPTH], f32x4 (&acc)[MB][NW],
    const short* const (&wp)[NW], const short* const (&xp)[MB], int wave,
    int k_left, int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int m = 0; m < MB; ++m)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ring[d].x[m], ring[d].w[n], acc[m][n], 0, 0, 0);
    if (!TAIL || i + d + DEPTH < n_it)
      load_stage<MB, NW, KPRED>(ring[d], wp, xp,
                                wave + (i + d + DEPTH) * MOE_WAVES, k_left);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// acc += x rows · weight rowsᵀ over this wave's K steps (wave, wave + 4, ...
// below ceil(K / 32)), then all four waves' accumulators into red. wp and xp
// point at this lane's k = kq of each row; k_left = K - kq.
template <int MB, int NW, int DEPTH, bool KPRED>
__device__ __forceinline__ void gemm_core(
    float (&red)[MOE_WAVES][MB][NW][4][WAVE], const short* const (&wp)[NW],
    const short* const (&xp)[MB], int K, int k_left) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  f32x4 acc[MB][NW];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_steps = (K + MOE_KSTEP - 1) / MOE_KSTEP;
  const int n_it = (n_steps - wave + MOE_WAVES - 1) / MOE_WAVES;  // may be 0
  Stage<MB, NW> ring[DEPTH];
  int i = 0;
  if (n_it >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      load_stage<MB, NW, KPRED>(ring[d], wp, xp, wave + d * MOE_WAVES, k_left);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_it; i += DEPTH)
      ring_round<MB, NW, DEPTH, KPRED, false>(ring, acc, wp, xp, wave, k_left,
                                              i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it)
        load_stage<MB, NW, KPRED>(ring[d], wp, xp, wave + d * MOE_WAVES,
                                  k_left);
  }
  for (; i < n_it; i += DEPTH)
    ring_round<MB, NW, DEPTH, KPRED, true>(ring, acc, wp, xp, wave, k_left, i,
                                           n_it);

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][m][n][j][lane] = acc[m][n][j];
  __syncthreads();
}

// Element (row m, column block nb, columns c .. c + 3 of it) summed over the
// waves in wave order.
template <int MB, int NW>
__device__ __forceinline__ f32x4 red_sum(
    const float (&red)[MOE_WAVES][MB][NW][4][WAVE], int m, int nb, int c) {
  const int l0 = ((m & 15) >> 2) * 16 + c;
  f32x4 s;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = red[0][m >> 4][nb][m & 3][l0 + e];
#pragma unroll
    for (int w = 1; w < MOE_WAVES; ++w) v += red[w][m >> 4][nb][m & 3][l0 + e];
    s[e] = v;
  }
  return s;
}

// The epilogues, shared by the bf16, the MXFP4 and the fp8 kernels. Gate-up:
// act = bf16(silu(gate) * up) for the tile's live rows, by sorted position.
// SCALED (fp8 experts): sc is the expert's row of w13s, and the fp32 sums of
// gate column n and up column n are multiplied by sc[n] and sc[I + n] first.
template <int MB, bool SCALED = false>
__device__ __forceinline__ void gate_up_epilogue(
    const float (&red)[MOE_WAVES][MB][2 * MOE_NB][4][WAVE],
    short* __restrict__ act, int start, int count, int n0, int I,
    const float* __restrict__ sc = nullptr) {
  constexpr int NW = 2 * MOE_NB;
  for (int i = threadIdx.x; i < count * (MOE_BN / 4); i += MOE_THREADS) {
    const int m = i / (MOE_BN / 4), c = (i % (MOE_BN / 4)) * 4;
    const int n = n0 + c;
    if (n >= I) continue;  // I % 16 == 0: four columns are in or out
    f32x4 g = red_sum<MB, NW>(red, m, c >> 4, c & 15);
    f32x4 u = red_sum<MB, NW>(red, m, MOE_NB + (c >> 4), c & 15);
    if (SCALED) {
      const f32x4 sg = *(const f32x4*)(sc + n);
      const f32x4 su = *(const f32x4*)(sc + I + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g[e] *= sg[e];
        u[e] *= su[e];
      }
    }
    short4v o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = f32_to_bf16(g[e] / (1.f + expf(-g[e])) * u[e]);
    *(short4v*)(act + (int64_t)(start + m) * I + n) = o;
  }
}

// Down: y2[pair] = the pair's routing weight times its row, fp32. SCALED (fp8
// experts): sc is the expert's row of w2s, and the fp32 sum of column n is
// multiplied by sc[n] first, then by the routing weight.
template <int MB, bool SCALED = false>
__device__ __forceinline__ void down_epilogue(
    const float (&red)[MOE_WAVES][MB][MOE_NB][4][WAVE],
    const int32_t* __restrict__ perm, const float* __restrict__ w,
    float* __restrict__ y2, int start, int count, int n0, int H,
    const float* __restrict__ sc = nullptr) {
  for (int i = threadIdx.x; i < count * (MOE_BN / 4); i += MOE_THREADS) {
    const int m = i / (MOE_BN / 4), c = (i % (MOE_BN / 4)) * 4;
    const int n = n0 + c;
    if (n >= H) continue;  // H % 32 == 0
    const int pair = perm[start + m];
    const float wt = w[pair];
    f32x4 s = red_sum<MB, MOE_NB>(red, m, c >> 4, c & 15);
    if (SCALED) {
      const f32x4 sn = *(const f32x4*)(sc + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] *= sn[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] *= wt;
    *(f32x4*)(y2 + (int64_t)pair * H + n) = s;
  }
}

// ring depth by registers: a stage holds NW + MB 16-byte loads a lane
template <int MB>
constexpr int gate_up_depth() { return MB == 4 ? 3 : 4; }
template <int MB>
constexpr int down_depth() { return 4; }

template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_gate_up_kernel(
    const short* __restrict__ x, const short* __restrict__ w13,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, short* __restrict__ act, int H, int I,
    int k) {
  constexpr int NW = 2 * MOE_NB;   // gate blocks, then up blocks
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, kq = (lane >> 4) * 8;
  const int n0 = blockIdx.x * MOE_BN;

  // Rows past count and column blocks past I read a valid row instead
  // (count >= 1, n0 < I): the epilogue stores nothing for them.
  const short* wp[NW];
#pragma unroll
  for (int nb = 0; nb < MOE_NB; ++nb) {
    const int n = n0 + nb * 16 < I ? n0 + nb * 16 + r : n0 + r;
    wp[nb] = w13 + ((int64_t)expert * 2 * I + n) * H + kq;
    wp[MOE_NB + nb] = wp[nb] + (int64_t)I * H;
  }
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    const int pair = perm[start + (m < count ? m : 0)];
    xp[mb] = x + (int64_t)(pair / k) * H + kq;
  }
  gemm_core<MB, NW, gate_up_depth<MB>(), false>(red, wp, xp, H, H - kq);

  gate_up_epilogue<MB>(red, act, start, count, n0, I);
}

template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_down_kernel(
    const short* __restrict__ act, const short* __restrict__ w2,
    const int32_t* __restrict__ tiles, const int32_t* __restrict__ n_tiles,
    const int32_t* __restrict__ perm, const float* __restrict__ w,
    float* __restrict__ y2, int H, int I) {
  constexpr int NW = MOE_NB;
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, kq = (lane >> 4) * 8;
  const int n0 = blockIdx.x * MOE_BN;

  const short* wp[NW];
#pragma unroll
  for (int nb = 0; nb < NW; ++nb) {
    const int n = n0 + nb * 16 < H ? n0 + nb * 16 + r : n0 + r;
    wp[nb] = w2 + ((int64_t)expert * H + n) * I + kq;
  }
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    xp[mb] = act + (int64_t)(start + (m < count ? m : 0)) * I + kq;
  }
  gemm_core<MB, NW, down_depth<MB>(), true>(red, wp, xp, I, I - kq);

  down_epilogue<MB>(red, perm, w, y2, start, count, n0, H);
}

// eight columns a thread: k reads of 32 bytes, one 16-byte write
__global__ __launch_bounds__(MOE_THREADS) void moe_combine_kernel(
    const float* __restrict__ y2, short* __restrict__ y, int64_t n_oct, int H,
    int k) {
  const int64_t i = (int64_t)blockIdx.x * MOE_THREADS + threadIdx.x;
  if (i >= n_oct) return;
  const int64_t t = i / (H / 8);
  const int c = (int)(i % (H / 8)) * 8;
  const float* p = y2 + t * k * H + c;
  f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
  for (int j = 1; j < k; ++j) {
    p += H;
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo[e] += a[e];
      hi[e] += b[e];
    }
  }
  short8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = f32_to_bf16(lo[e]);
    o[4 + e] = f32_to_bf16(hi[e]);
  }
  *(short8*)(y + t * H + c) = o;
}

// ---- the two expert GEMMs on MXFP4 experts ---------------------------------

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MX_GROUP = 32;     // k that share one e8m0 scale
constexpr int MX_KBLOCK = 128;   // k of one stage: a group a lane group

// One ring stage of this lane: per weight row block one MX group (16 bytes
// of codes, one scale byte), per x row block the 32 x of the same k.
template <int MB, int NW>
struct MxStage {
  u32x4 w[NW];
  uint32_t s[NW];
  short8 x[MB][4];
};

// K block kb of this lane's group. groups_left = K / 32 - (lane >> 4): a
// lane group whose k is past K issues no load and feeds zeros on both
// operands (code 0 is +0 under any scale).
template <int MB, int NW>
__device__ __forceinline__ void mx_load_stage(
    MxStage<MB, NW>& s, const unsigned char* const (&wp)[NW],
    const unsigned char* const (&sp)[NW], const short* const (&xp)[MB],
    int kb, int groups_left) {
  const bool ok = kb * (MX_KBLOCK / MX_GROUP) < groups_left;
  const u32x4 zw = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int n = 0; n < NW; ++n) {
    s.w[n] = ok ? *(const u32x4*)(wp[n] + kb * (MX_KBLOCK / 2)) : zw;
    s.s[n] = ok ? sp[n][kb * (MX_KBLOCK / MX_GROUP)] : 127u;
  }
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int d = 0; d < 4; ++d)
      s.x[m][d] = load8_or_zero(xp[m] + kb * MX_KBLOCK + d * 8, ok);
}

// One turn of the ring, as ring_round: dword q of a stage's group is the B
// operand of MFMA q, converted with the group's scale, against the lane's x
// at the same eight k.
template <int MB, int NW, int DEPTH, bool TAIL>
__device__ __forceinline__ void mx_ring_round(
    MxStage<MB, NW> (&ring)[DEPTH], f32x4 (&acc)[MB][NW],
    const unsigned char* const (&wp)[NW],
    const unsigned char* const (&sp)[NW], const short* const (&xp)[MB],
    int wave, int groups_left, int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
#pragma unroll
    for (int n = 0; n < NW; ++n) {
      const float sc = e8m0_to_f32(ring[d].s[n]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const short8 b = fp4x8_to_bf16(ring[d].w[n][q], sc);
#pragma unroll
        for (int m = 0; m < MB; ++m)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ring[d].x[m][q], b, acc[m][n], 0, 0, 0);
      }
    }
    if (!TAIL || i + d + DEPTH < n_it)
      mx_load_stage(ring[d], wp, sp, xp, wave + (i + d + DEPTH) * MOE_WAVES,
                    groups_left);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// gemm_core for MXFP4 weight rows: this wave's 128-wide K blocks (wave,
// wave + 4, ... below ceil(K / 128)), then all four waves' accumulators into
// red. wp, sp and xp point at this lane's group of K block 0 of each row.
// K % 32 == 0; the last block may hold one to three groups.
template <int MB, int NW, int DEPTH>
__device__ __forceinline__ void mx_gemm_core(
    float (&red)[MOE_WAVES][MB][NW][4][WAVE],
    const unsigned char* const (&wp)[NW],
    const unsigned char* const (&sp)[NW], const short* const (&xp)[MB],
    int K) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int groups_left = K / MX_GROUP - (lane >> 4);
  f32x4 acc[MB][NW];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_kb = (K + MX_KBLOCK - 1) / MX_KBLOCK;
  const int n_it = (n_kb - wave + MOE_WAVES - 1) / MOE_WAVES;  // may be 0
  MxStage<MB, NW> ring[DEPTH];
  int i = 0;
  if (n_it >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      mx_load_stage(ring[d], wp, sp, xp, wave + d * MOE_WAVES, groups_left);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_it; i += DEPTH)
      mx_ring_round<MB, NW, DEPTH, false>(ring, acc, wp, sp, xp, wave,
                                          groups_left, i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it)
        mx_load_stage(ring[d], wp, sp, xp, wave + d * MOE_WAVES, groups_left);
  }
  for (; i < n_it; i += DEPTH)
    mx_ring_round<MB, NW, DEPTH, true>(ring, acc, wp, sp, xp, wave,
                                       groups_left, i, n_it);

#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][m][n][j][lane] = acc[m][n][j];
  __syncthreads();
}

// ring depth by registers: a stage holds 5 NW + 16 MB a lane. Gate-up
// (NW 4): 36 at MB 1, 52 at MB 2; down (NW 2): 26 and 42. MB 4 would be 84
// and 74 a stage, no room for a ring: MOE_MXFP4_MAX_MB caps the tiles at 2.
template <int MB>
constexpr int mx_gate_up_depth() { return MB == 1 ? 4 : 3; }
template <int MB>
constexpr int mx_down_depth() { return 4; }

// As moe_gate_up_kernel, on w13q [E, 2 I, H / 2] and w13s [E, 2 I, H / 32].
// I % 32 == 0: every column block is whole.
template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_gate_up_mxfp4_kernel(
    const short* __restrict__ x, const unsigned char* __restrict__ w13q,
    const unsigned char* __restrict__ w13s, const int32_t* __restrict__ tiles,
    const int32_t* __restrict__ n_tiles, const int32_t* __restrict__ perm,
    short* __restrict__ act, int H, int I, int k) {
  constexpr int NW = 2 * MOE_NB;   // gate blocks, then up blocks
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * MOE_BN;

  const unsigned char* wp[NW];
  const unsigned char* sp[NW];
#pragma unroll
  for (int nb = 0; nb < MOE_NB; ++nb) {
    const int64_t row = (int64_t)expert * 2 * I + n0 + nb * 16 + r;
    wp[nb] = w13q + row * (H / 2) + g * (MX_GROUP / 2);
    sp[nb] = w13s + row * (H / MX_GROUP) + g;
    wp[MOE_NB + nb] = wp[nb] + (int64_t)I * (H / 2);
    sp[MOE_NB + nb] = sp[nb] + (int64_t)I * (H / MX_GROUP);
  }
  // Rows past count read a valid row instead (count >= 1): the epilogue
  // stores nothing for them.
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    const int pair = perm[start + (m < count ? m : 0)];
    xp[mb] = x + (int64_t)(pair / k) * H + g * MX_GROUP;
  }
  mx_gemm_core<MB, NW, mx_gate_up_depth<MB>()>(red, wp, sp, xp, H);
  gate_up_epilogue<MB>(red, act, start, count, n0, I);
}

// As moe_down_kernel, on w2q [E, H, I / 2] and w2s [E, H, I / 32].
template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_down_mxfp4_kernel(
    const short* __restrict__ act, const unsigned char* __restrict__ w2q,
    const unsigned char* __restrict__ w2s, const int32_t* __restrict__ tiles,
    const int32_t* __restrict__ n_tiles, const int32_t* __restrict__ perm,
    const float* __restrict__ w, float* __restrict__ y2, int H, int I) {
  constexpr int NW = MOE_NB;
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * MOE_BN;

  const unsigned char* wp[NW];
  const unsigned char* sp[NW];
#pragma unroll
  for (int nb = 0; nb < NW; ++nb) {   // H % 32 == 0: the block is whole
    const int64_t row = (int64_t)expert * H + n0 + nb * 16 + r;
    wp[nb] = w2q + row * (I / 2) + g * (MX_GROUP / 2);
    sp[nb] = w2s + row * (I / MX_GROUP) + g;
  }
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    xp[mb] = act + (int64_t)(start + (m < count ? m : 0)) * I + g * MX_GROUP;
  }
  mx_gemm_core<MB, NW, mx_down_depth<MB>()>(red, wp, sp, xp, I);
  down_epilogue<MB>(red, perm, w, y2, start, count, n0, H);
}

// ---- the two expert GEMMs on fp8 experts -----------------------------------

constexpr int F8_GROUP = 16;     // k of one lane group: a 16-byte weight load
constexpr int F8_KBLOCK = 64;    // k of one stage: a group a lane group

// One ring stage of this lane: per weight row block 16 e4m3 bytes, per x row
// block the 16 bf16 of the same k.
template <int MB, int NW>
struct F8Stage {
  u32x4 w[NW];
  short8 x[MB][2];
};

// K block kb of this lane's group. KPRED: groups_left = K / 16 - (lane >> 4),
// and a lane group whose k is past K issues no load and feeds zeros on both
// operands (byte 0 is +0). Otherwise the block is whole.
template <int MB, int NW, bool KPRED>
__device__ __forceinline__ void f8_load_stage(
    F8Stage<MB, NW>& s, const unsigned char* const (&wp)[NW],
    const short* const (&xp)[MB], int kb, int groups_left) {
  const bool ok = !KPRED || kb * (F8_KBLOCK / F8_GROUP) < groups_left;
  const u32x4 zw = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int n = 0; n < NW; ++n)
    s.w[n] = ok ? *(const u32x4*)(wp[n] + kb * F8_KBLOCK) : zw;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    s.x[m][0] = load8_or_zero(xp[m] + kb * F8_KBLOCK, ok);
    s.x[m][1] = load8_or_zero(xp[m] + kb * F8_KBLOCK + 8, ok);
  }
}

// One turn of the ring, as ring_round: bytes 0..7 of a stage's weights are
// the B operand of one MFMA and bytes 8..15 of the next, against the lane's x
// at the same k. TAIL = false runs on whole K blocks only: neither the stage
// count nor K is checked.
template <int MB, int NW, int DEPTH, bool TAIL>
__device__ __forceinline__ void f8_ring_round(
    F8Stage<MB, NW> (&ring)[DEPTH], f32x4 (&acc)[MB][NW],
    const unsigned char* const (&wp)[NW], const short* const (&xp)[MB],
    int wave, int groups_left, int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
#pragma unroll
    for (int n = 0; n < NW; ++n) {
      const short8 b0 = fp8x8_to_bf16(ring[d].w[n][0], ring[d].w[n][1]);
      const short8 b1 = fp8x8_to_bf16(ring[d].w[n][2], ring[d].w[n][3]);
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ring[d].x[m][0], b0, acc[m][n], 0, 0, 0);
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ring[d].x[m][1], b1, acc[m][n], 0, 0, 0);
      }
    }
    if (!TAIL || i + d + DEPTH < n_it)
      f8_load_stage<MB, NW, TAIL>(ring[d], wp, xp,
                                  wave + (i + d + DEPTH) * MOE_WAVES,
                                  groups_left);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// gemm_core for e4m3 weight rows: this wave's 64-wide K blocks (wave,
// wave + 4, ... below ceil(K / 64)), then all four waves' accumulators into
// red. wp and xp point at this lane's group of K block 0 of each row.
// K % 16 == 0; the last block may hold one to three groups. n_full counts
// this wave's blocks below floor(K / 64): the straight-line turns stay inside
// them, so only the last turns carry the K predicate.
template <int MB, int NW, int DEPTH>
__device__ __forceinline__ void fp8_gemm_core(
    float (&red)[MOE_WAVES][MB][NW][4][WAVE],
    const unsigned char* const (&wp)[NW], const short* const (&xp)[MB],
    int K) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int groups_left = K / F8_GROUP - (lane >> 4);
  f32x4 acc[MB][NW];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_kb = (K + F8_KBLOCK - 1) / F8_KBLOCK;
  const int n_it = (n_kb - wave + MOE_WAVES - 1) / MOE_WAVES;  // may be 0
  const int n_full = (K / F8_KBLOCK - wave + MOE_WAVES - 1) / MOE_WAVES;
  F8Stage<MB, NW> ring[DEPTH];
  int i = 0;
  if (n_full >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      f8_load_stage<MB, NW, false>(ring[d], wp, xp, wave + d * MOE_WAVES,
                                   groups_left);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_full; i += DEPTH)
      f8_ring_round<MB, NW, DEPTH, false>(ring, acc, wp, xp, wave,
                                          groups_left, i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it)
        f8_load_stage<MB, NW, true>(ring[d], wp, xp, wave + d * MOE_WAVES,
                                    groups_left);
  }
  for (; i < n_it; i += DEPTH)
    f8_ring_round<MB, NW, DEPTH, true>(ring, acc, wp, xp, wave, groups_left,
                                       i, n_it);

#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][m][n][j][lane] = acc[m][n][j];
  __syncthreads();
}

// ring depth by registers: a stage holds 4 NW + 8 MB a lane. Gate-up (NW 4):
// 24 / 32 / 48 at MB 1 / 2 / 4 next to 16 MB accumulators; down (NW 2):
// 16 / 24 / 40 next to 8 MB. Chosen by that arithmetic, not swept.
template <int MB>
constexpr int f8_gate_up_depth() { return MB == 1 ? 4 : MB == 2 ? 3 : 2; }
template <int MB>
constexpr int f8_down_depth() { return MB == 4 ? 3 : 4; }

// As moe_gate_up_kernel, on w13q [E, 2 I, H] e4m3 and w13s [E, 2 I] fp32.
template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_gate_up_fp8_kernel(
    const short* __restrict__ x, const unsigned char* __restrict__ w13q,
    const float* __restrict__ w13s, const int32_t* __restrict__ tiles,
    const int32_t* __restrict__ n_tiles, const int32_t* __restrict__ perm,
    short* __restrict__ act, int H, int I, int k) {
  constexpr int NW = 2 * MOE_NB;   // gate blocks, then up blocks
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, kq = (lane >> 4) * F8_GROUP;
  const int n0 = blockIdx.x * MOE_BN;

  // Rows past count and column blocks past I read a valid row instead
  // (count >= 1, n0 < I): the epilogue stores nothing for them.
  const unsigned char* wp[NW];
#pragma unroll
  for (int nb = 0; nb < MOE_NB; ++nb) {
    const int n = n0 + nb * 16 < I ? n0 + nb * 16 + r : n0 + r;
    wp[nb] = w13q + ((int64_t)expert * 2 * I + n) * H + kq;
    wp[MOE_NB + nb] = wp[nb] + (int64_t)I * H;
  }
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    const int pair = perm[start + (m < count ? m : 0)];
    xp[mb] = x + (int64_t)(pair / k) * H + kq;
  }
  fp8_gemm_core<MB, NW, f8_gate_up_depth<MB>()>(red, wp, xp, H);
  gate_up_epilogue<MB, true>(red, act, start, count, n0, I,
                             w13s + (int64_t)expert * 2 * I);
}

// As moe_down_kernel, on w2q [E, H, I] e4m3 and w2s [E, H] fp32.
template <int MB>
__global__ __launch_bounds__(MOE_THREADS) void moe_down_fp8_kernel(
    const short* __restrict__ act, const unsigned char* __restrict__ w2q,
    const float* __restrict__ w2s, const int32_t* __restrict__ tiles,
    const int32_t* __restrict__ n_tiles, const int32_t* __restrict__ perm,
    const float* __restrict__ w, float* __restrict__ y2, int H, int I) {
  constexpr int NW = MOE_NB;
  __shared__ float red[MOE_WAVES][MB][NW][4][WAVE];
  const int tile = blockIdx.y;
  if (tile >= *n_tiles) return;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int expert = tiles[tile * 3 + 2];
  const int lane = threadIdx.x % WAVE;
  const int r = lane & 15, kq = (lane >> 4) * F8_GROUP;
  const int n0 = blockIdx.x * MOE_BN;

  const unsigned char* wp[NW];
#pragma unroll
  for (int nb = 0; nb < NW; ++nb)   // H % 32 == 0: the block is whole
    wp[nb] = w2q + ((int64_t)expert * H + n0 + nb * 16 + r) * I + kq;
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + r;
    xp[mb] = act + (int64_t)(start + (m < count ? m : 0)) * I + kq;
  }
  fp8_gemm_core<MB, NW, f8_down_depth<MB>()>(red, wp, xp, I);
  down_epilogue<MB, true>(red, perm, w, y2, start, count, n0, H,
                          w2s + (int64_t)expert * H);
}

template <int MB>
void launch_gemms_fp8(const MoeFfnFp8Args& a, uint32_t n_tiles,
                      hipStream_t stream) {
  hipLaunchKernelGGL(moe_gate_up_fp8_kernel<MB>,
                     dim3((uint32_t)((a.I + MOE_BN - 1) / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.x,
                     (const unsigned char*)a.w13q, a.w13s, a.tiles, a.n_tiles,
                     a.perm, (short*)a.act, a.H, a.I, a.k);
  hipLaunchKernelGGL(moe_down_fp8_kernel<MB>,
                     dim3((uint32_t)(a.H / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.act,
                     (const unsigned char*)a.w2q, a.w2s, a.tiles, a.n_tiles,
                     a.perm, a.w, a.y2, a.H, a.I);
}

template <int MB>
void launch_gemms_mxfp4(const MoeFfnMxfp4Args& a, uint32_t n_tiles,
                        hipStream_t stream) {
  hipLaunchKernelGGL(moe_gate_up_mxfp4_kernel<MB>,
                     dim3((uint32_t)(a.I / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.x,
                     (const unsigned char*)a.w13q,
                     (const unsigned char*)a.w13s, a.tiles, a.n_tiles, a.perm,
                     (short*)a.act, a.H, a.I, a.k);
  hipLaunchKernelGGL(moe_down_mxfp4_kernel<MB>,
                     dim3((uint32_t)(a.H / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.act,
                     (const unsigned char*)a.w2q, (const unsigned char*)a.w2s,
                     a.tiles, a.n_tiles, a.perm, a.w, a.y2, a.H, a.I);
}

template <int MB>
void launch_gemms(const MoeFfnArgs& a, uint32_t n_tiles, hipStream_t stream) {
  hipLaunchKernelGGL(moe_gate_up_kernel<MB>,
                     dim3((uint32_t)((a.I + MOE_BN - 1) / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.x,
                     (const short*)a.w13, a.tiles, a.n_tiles, a.perm,
                     (short*)a.act, a.H, a.I, a.k);
  hipLaunchKernelGGL(moe_down_kernel<MB>,
                     dim3((uint32_t)((a.H + MOE_BN - 1) / MOE_BN), n_tiles),
                     dim3(MOE_THREADS), 0, stream, (const short*)a.act,
                     (const short*)a.w2, a.tiles, a.n_tiles, a.perm, a.w,
                     a.y2, a.H, a.I);
}

}  // namespace

hipError_t lds_moe_route(const MoeRouteArgs& a, hipStream_t stream) {
  if (a.T == 0) return hipSuccess;
  const uint32_t grid =
      (uint32_t)((a.T + MOE_ROUTE_TOKENS - 1) / MOE_ROUTE_TOKENS);
  hipLaunchKernelGGL(moe_route_kernel, dim3(grid), dim3(MOE_THREADS), 0,
                     stream, (const short*)a.x, (const short*)a.router, a.ids,
                     a.w, a.T, a.H, a.E, a.k, a.renorm);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_moe_align(const int32_t* ids, int32_t* tiles, int32_t* n_tiles,
                         int32_t* perm, int64_t P, int E, int TM,
                         hipStream_t stream) {
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(MOE_MAX_EXPERTS), 0,
                     stream, ids, tiles, n_tiles, perm, (int)P, E, TM);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_moe_combine(const float* y2, void* y, int T, int H, int k,
                           hipStream_t stream) {
  const int64_t n_oct = (int64_t)T * H / 8;
  hipLaunchKernelGGL(moe_combine_kernel,
                     dim3((uint32_t)((n_oct + MOE_THREADS - 1) / MOE_THREADS)),
                     dim3(MOE_THREADS), 0, stream, y2, (short*)y, n_oct, H, k);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// The work list in front of the two GEMMs and the slot sum behind them, for
// any weight format: A is MoeFfnArgs, MoeFfnMxfp4Args or MoeFfnFp8Args.
template <class A, class F>
hipError_t moe_ffn_launch(const A& a, F&& gemms, hipStream_t stream) {
  if (a.T == 0) return hipSuccess;
  const int64_t P = (int64_t)a.T * a.k;
  const uint32_t n_tiles = (uint32_t)moe_tile_bound(P, a.E, a.mb);
  hipError_t err = lds_moe_align(a.ids, a.tiles, a.n_tiles, a.perm, P, a.E,
                                 16 * a.mb, stream);
  if (err != hipSuccess) return err;
  if (!gemms(n_tiles)) return hipErrorInvalidValue;
  HIP_CHECK_LAST();
  return lds_moe_combine(a.y2, a.y, a.T, a.H, a.k, stream);
}

hipError_t lds_moe_ffn(const MoeFfnArgs& a, hipStream_t stream) {
  return moe_ffn_launch(a, [&](uint32_t n_tiles) {
    switch (a.mb) {
      case 1: launch_gemms<1>(a, n_tiles, stream); return true;
      case 2: launch_gemms<2>(a, n_tiles, stream); return true;
      case 4: launch_gemms<4>(a, n_tiles, stream); return true;
      default: return false;
    }
  }, stream);
}

hipError_t lds_moe_ffn_mxfp4(const MoeFfnMxfp4Args& a, hipStream_t stream) {
  return moe_ffn_launch(a, [&](uint32_t n_tiles) {
    switch (a.mb) {
      case 1: launch_gemms_mxfp4<1>(a, n_tiles, stream); return true;
      case 2: launch_gemms_mxfp4<2>(a, n_tiles, stream); return true;
      default: return false;
    }
  }, stream);
}

hipError_t lds_moe_ffn_fp8(const MoeFfnFp8Args& a, hipStream_t stream) {
  return moe_ffn_launch(a, [&](uint32_t n_tiles) {
    switch (a.mb) {
      case 1: launch_gemms_fp8<1>(a, n_tiles, stream); return true;
      case 2: launch_gemms_fp8<2>(a, n_tiles, stream); return true;
      case 4: launch_gemms_fp8<4>(a, n_tiles, stream); return true;
      default: return false;
    }
  }, stream);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
