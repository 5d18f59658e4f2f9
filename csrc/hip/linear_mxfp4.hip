// linear_mxfp4.hip — weight-only MXFP4 linear for skinny batches on gfx950:
//   y[m, n] = sum_k x[m, k] * e2m1(wq[n, k]) * 2^(scale[n, k / 32] - 127)
//
// x [T, in] bf16; wq [out, in / 2] uint8, two e2m1 codes a byte, K contiguous,
// k = 2j in the low nibble of byte j; scale [out, in / 32] uint8, one e8m0
// exponent per 32 k; y [T, out] bf16. in % 128 == 0, out % 16 == 0. The
// format is in DEVELOPMENT.md "MXFP4 weights". Decode is bound by the weight
// stream: half a byte per weight, read once, straight into the registers of
// the one lane that uses it.
//
//   linear_mxfp4_kernel<MB, NB>  grid (column block, 32-row tile, K split)
//     A workgroup of four waves owns BN = NB * 16 output columns and MB * 16
//     rows (MB = 1 up to 16 rows, 2 beyond; grid.y walks 32-row tiles) over
//     one K split. Its waves take the split's 128-wide K blocks round-robin.
//     The unit of the format is the unit of the kernel: one 16-byte load of a
//     lane is one MX group, the 32 codes of output row lane & 15 for
//     k = 32 * (lane >> 4) .. + 32 of the K block. Dword d of the load is the
//     B operand of MFMA d: four v_cvt_scalef32_pk_bf16_fp4 turn its eight
//     codes times the group's scale into eight bf16, and the A operand is the
//     lane's x row at the same eight k (four 16-byte loads, 64 contiguous
//     bytes). mfma_f32_16x16x32_bf16 sums over its four lane groups whatever
//     k each of them brings, as long as A and B bring the same, so a lane only
//     ever multiplies k of its own group: the scale is one operand of a
//     convert that is needed anyway, applied before the matrix core, exactly
//     (e2m1 times a power of two is a bf16), at no instruction.
//   Scale bytes. A lane needs one byte per K block and column block: it is
//     fetched as that, one byte load next to each 16-byte weight load, in
//     the same ring stage. The four lane groups of a row read four contiguous
//     bytes, so a wave touches 16 short runs the weights' rows already
//     opened; the cost is one more load issue per 17 bytes. Sharing a dword
//     between consecutive K blocks was not taken: a wave's blocks are four
//     apart (round-robin, which keeps the four waves on neighbouring lines),
//     and a byte picked by a run-time index costs the shift the convert's
//     scale operand otherwise saves. The byte becomes a float by a shift
//     into the exponent field; 2 <= byte <= 252 keeps every product normal.
//   Ring. Loads for the next DEPTH K blocks are in flight over the current
//     MFMAs, weights, scales and x in one register ring (loads return in
//     order). A stage is 5 * NB + 16 * MB registers a lane: 26 at MB 1, NB 2
//     (DEPTH 4, 104 registers), 52 at MB 2, NB 4 (DEPTH 3, 156 registers,
//     next to 32 accumulators). MB = 4 would be 84 a stage and leaves no
//     room for a ring under 256 registers, so the row blocks are capped at 2
//     and taller batches walk grid.y; the weights of a column block are then
//     read once per 32 rows, from L2 after the first.
//   Nothing goes through LDS until the end: the four waves' accumulators are
//     summed there in wave order and stored as bf16, four columns a thread.
//   linear_mxfp4_reduce_kernel   only when K is split across workgroups: the
//     epilogue stores fp32 partials part[split, T, out] instead, and this
//     kernel sums them in split order and rounds.
//   dequant_mxfp4_weight_kernel  W[k, n] as [in, out] bf16 for the hipBLASLt
//     path of prefill-sized batches: tiles of 64 n x 128 k, a thread reads
//     one group (16 bytes) and its scale byte, converts with the same
//     instruction, transposes through LDS and writes 16 bytes along n.
//
// BN by T (linear_mxfp4_bn): 32 up to 16 rows, where more workgroups keep
// more loads in flight, 64 beyond, where x (read from L2 once per column
// block) would otherwise outweigh the weights. K split
// (linear_mxfp4_k_splits): doubled while the launch has fewer than 512
// workgroups and a split keeps 2048 k, 16 K blocks, four a wave.
//
// Determinism: no atomics. The split count and the K block -> wave
// assignment depend on (in, out) alone, MFMA rows and columns never mix, and
// both reductions run in a fixed order: a row's bits do not depend on T (BN
// and MB only choose who computes an element), on the row's index or on the
// other rows of the launch.
#include "hip_common.h"
#include "launchers.h"
#include "mxfp4_convert.h"

// Built without packed fp32 arithmetic, for the reason given in
// linear_fp8.hip: the fp32 work here is three adds per output element.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MX_THREADS = 256;
constexpr int MX_WAVES = MX_THREADS / WAVE;
constexpr int MX_ROWS = 32;    // rows of a grid.y tile
constexpr int MX_GROUP = 32;   // k that share one e8m0 scale

// One ring stage of this lane: per column block one MX group (16 bytes of
// codes, one scale byte), per row block the 32 x of the same k.
template <int MB, int NB>
struct Stage {
  u32x4 w[NB];
  uint32_t s[NB];
  short8 x[MB][4];
};

template <int MB, int NB>
__device__ __forceinline__ void load_stage(
    Stage<MB, NB>& s, const unsigned char* const (&wp)[NB],
    const unsigned char* const (&sp)[NB], const short* const (&xp)[MB],
    int kb) {
  const int64_t k = (int64_t)kb * LINEAR_MXFP4_KBLOCK;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    s.w[nb] = *(const u32x4*)(wp[nb] + k / 2);
    s.s[nb] = sp[nb][k / MX_GROUP];
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int d = 0; d < 4; ++d)
      s.x[mb][d] = *(const short8*)(xp[mb] + k + d * 8);
}

// One turn of the ring: stages i .. i + DEPTH - 1 go through the matrix
// core, and each slot is refilled with the stage DEPTH later once its MFMAs
// have read it. With TAIL = false every stage and every refill exists
// (straight-line code, exact load counts); the last turns check each against
// n_it.
template <int MB, int NB, int DEPTH, bool TAIL>
__device__ __forceinline__ void ring_round(
    Stage<MB, NB> (&ring)[DEPTH], f32x4 (&acc)[MB][NB],
    const unsigned char* const (&wp)[NB],
    const unsigned char* const (&sp)[NB], const short* const (&xp)[MB],
    int kb0, int i, int n_it) {
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (TAIL && i + d >= n_it) break;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float sc = e8m0_to_f32(ring[d].s[nb]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const short8 b = fp4x8_to_bf16(ring[d].w[nb][q], sc);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ring[d].x[mb][q], b, acc[mb][nb], 0, 0, 0);
      }
    }
    if (!TAIL || i + d + DEPTH < n_it)
      load_stage(ring[d], wp, sp, xp, kb0 + (i + d + DEPTH) * MX_WAVES);
    // a stage's converts and MFMAs stay in front of the next stage's wait
    __builtin_amdgcn_sched_barrier(0);
  }
}

// part == null: y = bf16(sum); else part[split, T, out] = sum.
template <int MB, int NB, int DEPTH>
__global__ __launch_bounds__(MX_THREADS) void linear_mxfp4_kernel(
    const short* __restrict__ x, const unsigned char* __restrict__ wq,
    const unsigned char* __restrict__ scale, short* __restrict__ y,
    float* __restrict__ part, int T, int in, int out, int kb_per_split) {
  constexpr int BN = NB * 16;
  __shared__ float red[MX_WAVES][MB][NB][4][WAVE];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int n0 = blockIdx.x * BN, row0 = blockIdx.y * MX_ROWS;
  const int split = blockIdx.z;
  const int r = lane & 15, g = lane >> 4;

  // Rows and columns past the end read a valid row instead (T >= 1 and
  // n0 < out): MFMA rows and columns never mix, and the epilogue stores
  // nothing for them.
  const unsigned char* wp[NB];
  const unsigned char* sp[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = n0 + nb * 16 + r;
    const int64_t row = n < out ? n : n0 + r;
    wp[nb] = wq + row * (in / 2) + g * (MX_GROUP / 2);
    sp[nb] = scale + row * (in / MX_GROUP) + g;
  }
  const short* xp[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
    xp[mb] = x + (int64_t)min(row0 + mb * 16 + r, T - 1) * in + g * MX_GROUP;

  f32x4 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this wave's K blocks: kb0, kb0 + 4, ... below kb_end
  const int kb_end =
      min(in / LINEAR_MXFP4_KBLOCK, (split + 1) * kb_per_split);
  const int kb0 = split * kb_per_split + wave;
  const int n_it = (kb_end - kb0 + MX_WAVES - 1) / MX_WAVES;  // may be <= 0

  // The bulk loop sits right behind an unconditional fill of the ring, so
  // that the load order is known where its waits are placed. A wave with no
  // more than DEPTH blocks has all of them in flight at once.
  Stage<MB, NB> ring[DEPTH];
  int i = 0;
  if (n_it >= 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      load_stage(ring[d], wp, sp, xp, kb0 + d * MX_WAVES);
      __builtin_amdgcn_sched_barrier(0);  // issue the stages in ring order
    }
    for (; i + 2 * DEPTH <= n_it; i += DEPTH)
      ring_round<MB, NB, DEPTH, false>(ring, acc, wp, sp, xp, kb0, i, n_it);
  } else {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < n_it) load_stage(ring[d], wp, sp, xp, kb0 + d * MX_WAVES);
  }
  for (; i < n_it; i += DEPTH)
    ring_round<MB, NB, DEPTH, true>(ring, acc, wp, sp, xp, kb0, i, n_it);

  // D of the MFMA: column n = lane & 15, row m = (lane >> 4) * 4 + j
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][mb][nb][j][lane] = acc[mb][nb][j];
  __syncthreads();
  const int rows = min(MB * 16, T - row0);
  for (int e0 = threadIdx.x; e0 < rows * (BN / 4); e0 += MX_THREADS) {
    const int m = e0 / (BN / 4), c = (e0 % (BN / 4)) * 4;
    const int n = n0 + c;
    if (n >= out) continue;  // out % 16 == 0: four columns are in or out
    const int l0 = ((m & 15) >> 2) * 16 + (c & 15);
    f32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = red[0][m >> 4][c >> 4][m & 3][l0 + e];
#pragma unroll
      for (int w = 1; w < MX_WAVES; ++w)
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
__global__ __launch_bounds__(MX_THREADS) void linear_mxfp4_reduce_kernel(
    const float* __restrict__ part, short* __restrict__ y, int64_t n_quads,
    int n_split) {
  const int64_t i = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x;
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

constexpr int DQ_N = 64;             // output columns of a tile
constexpr int DQ_K = LINEAR_MXFP4_KBLOCK;
constexpr int DQ_PITCH = DQ_N + 8;   // shorts: rows stay 16-byte aligned

// grid (in / 128, ceil(out / 64)). Read: thread -> one group (32 k) of one wq
// row. Write: thread -> 8 n of one W row, four times.
__global__ __launch_bounds__(MX_THREADS) void dequant_mxfp4_weight_kernel(
    const unsigned char* __restrict__ wq,
    const unsigned char* __restrict__ scale, short* __restrict__ W, int in,
    int out) {
  __shared__ __attribute__((aligned(16))) short tile[DQ_K][DQ_PITCH];
  const int k0 = blockIdx.x * DQ_K, n0 = blockIdx.y * DQ_N;
  {
    const int rn = threadIdx.x / 4, g = threadIdx.x % 4;
    if (n0 + rn < out) {
      const int64_t n = n0 + rn;
      const u32x4 v =
          *(const u32x4*)(wq + n * (in / 2) + k0 / 2 + g * (MX_GROUP / 2));
      const float sc =
          e8m0_to_f32(scale[n * (in / MX_GROUP) + k0 / MX_GROUP + g]);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const short8 b = fp4x8_to_bf16(v[d], sc);
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[g * MX_GROUP + d * 8 + e][rn] = b[e];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < DQ_K * (DQ_N / 8) / MX_THREADS; ++h) {
    const int c = threadIdx.x + h * MX_THREADS;
    const int rk = c / (DQ_N / 8), cn = (c % (DQ_N / 8)) * 8;
    if (n0 + cn < out)  // out % 16 == 0: eight columns are in or out
      *(short8*)(W + (int64_t)(k0 + rk) * out + n0 + cn) =
          *(const short8*)&tile[rk][cn];
  }
}

template <int MB, int NB>
void launch_linear(const LinearMxfp4Args& a, float* part,
                   hipStream_t stream) {
  // ring depth by registers: a stage holds 5 * NB + 16 * MB a lane
  constexpr int DEPTH = MB == 1 ? 4 : 3;
  const int kb = a.in / LINEAR_MXFP4_KBLOCK;
  const dim3 grid((uint32_t)((a.out + NB * 16 - 1) / (NB * 16)),
                  (uint32_t)((a.T + MX_ROWS - 1) / MX_ROWS),
                  (uint32_t)a.n_split);
  hipLaunchKernelGGL((linear_mxfp4_kernel<MB, NB, DEPTH>), grid,
                     dim3(MX_THREADS), 0, stream, (const short*)a.x,
                     (const unsigned char*)a.wq,
                     (const unsigned char*)a.scale, (short*)a.y, part, a.T,
                     a.in, a.out, (kb + a.n_split - 1) / a.n_split);
}

template <int NB>
void launch_linear_rows(const LinearMxfp4Args& a, float* part,
                        hipStream_t stream) {
  if (a.T <= 16) launch_linear<1, NB>(a, part, stream);
  else launch_linear<2, NB>(a, part, stream);
}

}  // namespace

hipError_t lds_linear_mxfp4(const LinearMxfp4Args& a, hipStream_t stream) {
  if (a.T == 0 || a.out == 0) return hipSuccess;
  float* part = a.n_split > 1 ? a.part : nullptr;
  switch (a.bn) {
    case 16: launch_linear_rows<1>(a, part, stream); break;
    case 32: launch_linear_rows<2>(a, part, stream); break;
    case 64: launch_linear_rows<4>(a, part, stream); break;
    default: return hipErrorInvalidValue;
  }
  HIP_CHECK_LAST();
  if (part != nullptr) {
    const int64_t n_quads = (int64_t)a.T * a.out / 4;
    hipLaunchKernelGGL(linear_mxfp4_reduce_kernel,
                       dim3((uint32_t)((n_quads + MX_THREADS - 1) /
                                       MX_THREADS)),
                       dim3(MX_THREADS), 0, stream, part, (short*)a.y,
                       n_quads, a.n_split);
    HIP_CHECK_LAST();
  }
  return hipSuccess;
}

hipError_t lds_dequant_mxfp4_weight(const void* wq, const void* scale,
                                    void* W, int in, int out,
                                    hipStream_t stream) {
  if (in == 0 || out == 0) return hipSuccess;
  const dim3 grid((uint32_t)(in / DQ_K), (uint32_t)((out + DQ_N - 1) / DQ_N));
  hipLaunchKernelGGL(dequant_mxfp4_weight_kernel, grid, dim3(MX_THREADS), 0,
                     stream, (const unsigned char*)wq,
                     (const unsigned char*)scale, (short*)W, in, out);
  HIP_CHECK_LAST();
  return hipSuccess;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
