// lora.hip — batched multi-adapter LoRA add for gfx950:
//   y[row] += (x[row] · A[slot]ᵀ) · B[slot]ᵀ      for every row in `perm`
//
// Slot pools: A [S, R, in] bf16 and B [S, out, R] bf16 (alpha / rank folded
// into B), R a multiple of 16 in 16..64. The host work list groups adapter
// rows by slot: perm holds their row indices and tiles [n_tiles, 3] holds
// (start in perm, count <= 16, slot). Rows with no adapter are in neither and
// are never read or written.
//
// Two kernels, both on mfma_f32_16x16x32_bf16 with operands straight from
// global memory: with these layouts the eight consecutive k a lane feeds the
// matrix core are one 16-byte load, for the shrink (k along `in`) and for the
// expand (k along R) alike, so nothing is staged through LDS.
//
//   shrink  grid (tile, K split). A split is LORA_KCHUNK columns of `in`, so
//           the split count depends on `in` alone. The four waves take the
//           split's 32-wide k-steps round-robin; their accumulators are
//           summed in wave order through LDS and written as one fp32 partial
//           part[split, tile*16 + m, R].
//   expand  grid (tile, column block of LORA_NBLOCK). Sums the partials in
//           split order, rounds to bf16 and multiplies by B[slot]. It
//           computes the transposed product (out column on the MFMA row,
//           token on the MFMA column), so a lane ends up with four
//           consecutive columns of one y row: an 8-byte read-add-round-write.
//           One workgroup owns a (tile, column block): no two write the same
//           element and there are no atomics.
//
// The bits a row receives depend on its x row and its adapter only: a row's
// sums never mix with another row's, and their order is fixed by `in` and R.
#include "hip_common.h"
#include "launchers.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int LORA_THREADS = 256;  // 4 waves
constexpr int LORA_WAVES = LORA_THREADS / WAVE;

// The lane's 8 bf16 of an operand row as one 16-byte load, or zeros.
__device__ __forceinline__ short8 load8_or_zero(const short* p, bool ok) {
  short8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *(const short8*)p : z;
}

// RB = R / 16 accumulator blocks per wave.
template <int RB>
__global__ __launch_bounds__(LORA_THREADS) void lora_shrink_kernel(
    const short* __restrict__ x, const short* __restrict__ A,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ tiles,
    float* __restrict__ part, int n_tiles, int in) {
  constexpr int R = RB * 16;
  __shared__ float red[LORA_WAVES][RB][WAVE][4];
  const int tile = blockIdx.x, split = blockIdx.y;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int slot = tiles[tile * 3 + 2];
  const int m = lane & 15, kq = (lane >> 4) * 8;

  const bool row_ok = m < count;
  const int64_t row = row_ok ? perm[start + m] : 0;
  const short* xrow = x + row * in + kq;
  const short* arow = A + ((int64_t)slot * R + m) * in + kq;

  const int k_begin = split * LORA_KCHUNK;
  const int k_end = min(in, k_begin + LORA_KCHUNK);
  f32x4 acc[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int k = k_begin + wave * 32; k < k_end; k += LORA_WAVES * 32) {
    const short8 a = load8_or_zero(xrow + k, row_ok);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const short8 b = *(const short8*)(arow + (int64_t)rb * 16 * in + k);
      acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wave][rb][lane][j] = acc[rb][j];
  __syncthreads();
  // D of the MFMA: column (rank index) = lane & 15, row = (lane >> 4) * 4 + j
  float* dst = part + ((int64_t)split * n_tiles + tile) * 16 * R;
  for (int i = threadIdx.x; i < RB * WAVE * 4; i += LORA_THREADS) {
    const int j = i & 3, l = (i >> 2) % WAVE, rb = i / (WAVE * 4);
    float s = red[0][rb][l][j];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) s += red[w][rb][l][j];
    dst[((l >> 4) * 4 + j) * R + rb * 16 + (l & 15)] = s;
  }
}

// KS = ceil(R / 32) MFMA k-steps; with R = 16 or 48 the upper half of the
// last step is zero in both operands.
template <int RB>
__global__ __launch_bounds__(LORA_THREADS) void lora_expand_kernel(
    short* __restrict__ y, const short* __restrict__ B,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ tiles,
    const float* __restrict__ part, int n_tiles, int n_split, int out) {
  constexpr int R = RB * 16;
  constexpr int KS = (R + 31) / 32;
  const int tile = blockIdx.x;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int start = tiles[tile * 3], count = tiles[tile * 3 + 1];
  const int slot = tiles[tile * 3 + 2];
  const int m = lane & 15, kq = (lane >> 4) * 8;

  // this lane's token (MFMA column) and its tmp fragment, summed over the
  // K splits in split order and rounded to bf16
  const bool row_ok = m < count;
  short8 t[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int r0 = s * 32 + kq;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row_ok && r0 < R) {
      const float* p = part + ((int64_t)tile * 16 + m) * R + r0;
      for (int sp = 0; sp < n_split; ++sp) {
        const f32x4 lo = *(const f32x4*)p;
        const f32x4 hi = *(const f32x4*)(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[j] += lo[j];
          f[4 + j] += hi[j];
        }
        p += (int64_t)n_tiles * 16 * R;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) t[s][j] = f32_to_bf16(f[j]);
  }

  const int64_t yrow = row_ok ? perm[start + m] : 0;
  const int n_base = blockIdx.y * LORA_NBLOCK + wave * (LORA_NBLOCK / LORA_WAVES);
#pragma unroll
  for (int nb = 0; nb < LORA_NBLOCK / LORA_WAVES / 16; ++nb) {
    const int n0 = n_base + nb * 16;
    if (n0 >= out) break;  // out % 16 == 0: a column block is whole or absent
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const short* brow = B + ((int64_t)slot * out + n0 + m) * R;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int r0 = s * 32 + kq;
      const short8 b = load8_or_zero(brow + r0, r0 < R);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, t[s], acc, 0, 0, 0);
    }
    // D: column (token) = lane & 15, rows (out columns) n0 + (lane >> 4) * 4 + j
    if (row_ok) {
      short4v* yp = (short4v*)(y + yrow * out + n0 + (lane >> 4) * 4);
      short4v v = *yp;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = f32_to_bf16(bf16_to_f32(v[j]) + acc[j]);
      *yp = v;
    }
  }
}

}  // namespace

hipError_t lds_lora_shrink(const LoraArgs& a, hipStream_t stream) {
  if (a.n_tiles == 0) return hipSuccess;
  const dim3 grid((uint32_t)a.n_tiles, (uint32_t)lora_k_splits(a.in));
#define LORA_SHRINK(RB)                                                     \
  hipLaunchKernelGGL(lora_shrink_kernel<RB>, grid, dim3(LORA_THREADS), 0,   \
                     stream, (const short*)a.x, (const short*)a.A, a.perm,  \
                     a.tiles, a.part, a.n_tiles, a.in)
  switch (a.R) {
    case 16: LORA_SHRINK(1); break;
    case 32: LORA_SHRINK(2); break;
    case 48: LORA_SHRINK(3); break;
    case 64: LORA_SHRINK(4); break;
    default: return hipErrorInvalidValue;
  }
#undef LORA_SHRINK
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_lora_expand(const LoraArgs& a, hipStream_t stream) {
  if (a.n_tiles == 0) return hipSuccess;
  const dim3 grid((uint32_t)a.n_tiles,
                  (uint32_t)((a.out + LORA_NBLOCK - 1) / LORA_NBLOCK));
#define LORA_EXPAND(RB)                                                     \
  hipLaunchKernelGGL(lora_expand_kernel<RB>, grid, dim3(LORA_THREADS), 0,   \
                     stream, (short*)a.y, (const short*)a.B, a.perm,        \
                     a.tiles, a.part, a.n_tiles, lora_k_splits(a.in), a.out)
  switch (a.R) {
    case 16: LORA_EXPAND(1); break;
    case 32: LORA_EXPAND(2); break;
    case 48: LORA_EXPAND(3); break;
    case 64: LORA_EXPAND(4); break;
    default: return hipErrorInvalidValue;
  }
#undef LORA_EXPAND
  HIP_CHECK_LAST();
  return hipSuccess;
}
