// sampler.hip — fused on-device token sampler for gfx950: temperature,
// top-k, top-p, per-request Philox seed and the sampled token's logprob in
// one launch over the whole batch (contract: DEVELOPMENT.md "Sampling").
//
// One workgroup of 1024 threads owns one row of logits. Nothing is sorted
// and no [B, V] temporary exists: the row is streamed a handful of times
// (the first pass from HBM, the rest from L2/MALL) —
//   1. online max / sum-exp of the raw logits + argmax      (logsumexp)
//   2. top-k: radix select on the order-preserving integer key of the raw
//      logit, one 8-bit digit per pass (2 passes bf16, 4 passes fp32)
//   3. top-p over what top-k kept: the same radix walk, on LDS histograms
//      that hold a count and a mass per bin
//   4. Gumbel-max draw over the kept set, Philox4x32-10 keyed by the
//      request's seed and counted by (vocabulary index, token position)
// Passes 2 and 3 are skipped per row when the filter is off; T <= 0 rows
// stop after pass 1.
//
// Masses are accumulated as 2^-32 fixed point in 64-bit LDS atomics:
// integer adds commute, so a row's result does not depend on the order in
// which waves reach the histogram (nor on batch position or batch size).
#include "hip_common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int SAMPLER_THREADS = 1024;
constexpr int SAMPLER_WAVES = SAMPLER_THREADS / WAVE;
constexpr float MASS_SCALE = 4294967296.f;                  // 2^32
constexpr float U_SCALE = 5.9604644775390625e-08f;          // 2^-24
constexpr float U_MAX = 0.999999940395355224609375f;        // 1 - 2^-24

typedef unsigned long long u64;

__device__ __forceinline__ float raw_to_f32(short v) { return bf16_to_f32(v); }
__device__ __forceinline__ float raw_to_f32(float v) { return v; }

// order-preserving unsigned key of a raw logit: a < b  <=>  key(a) < key(b)
__device__ __forceinline__ uint32_t key_of(short v) {
  const uint32_t u = (uint16_t)v;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <typename T>
__device__ __forceinline__ float key_to_f32(uint32_t key);
template <>
__device__ __forceinline__ float key_to_f32<short>(uint32_t key) {
  const uint32_t u = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xFFFFu);
  return bf16_to_f32((short)(uint16_t)u);
}
template <>
__device__ __forceinline__ float key_to_f32<float>(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  return __uint_as_float(u);
}

template <typename T> struct RowVec;
template <> struct RowVec<short> { typedef short8 type; };
template <> struct RowVec<float> { typedef float4v type; };

// Calls f(index, raw element) for every element of one row, each exactly
// once across the workgroup. 16-byte loads cover the part of the row that
// is aligned for them; a row starts at element r*V, so for odd V in bf16
// the elements before the first 16-byte boundary and after the last whole
// vector are read one by one.
template <typename T, typename F>
__device__ __forceinline__ void for_row(const T* __restrict__ row, int V,
                                        F&& f) {
  typedef typename RowVec<T>::type vec_t;
  constexpr int VEC = 16 / (int)sizeof(T);
  const int tid = threadIdx.x;
  int head = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) /
                   sizeof(T));
  if (head > V) head = V;
  if (tid < head) f(tid, row[tid]);
  const int nvec = (V - head) / VEC;
  const vec_t* rv = (const vec_t*)(row + head);
  for (int c = tid; c < nvec; c += SAMPLER_THREADS) {
    const vec_t v = rv[c];
    const int base = head + c * VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) f(base + j, (T)v[j]);
  }
  const int t = head + nvec * VEC + tid;
  if (t < V) f(t, row[t]);
}

// ---- workgroup reductions (every thread calls; result to all threads) ----

__device__ __forceinline__ float block_sum_f32(float v, float* scratch) {
  v = wave_reduce_sum(v);
  if (threadIdx.x % WAVE == 0) scratch[threadIdx.x / WAVE] = v;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < SAMPLER_WAVES; ++w) total += scratch[w];
  __syncthreads();
  return total;
}

__device__ __forceinline__ int block_sum_i32(int v, int* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  if (threadIdx.x % WAVE == 0) scratch[threadIdx.x / WAVE] = v;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < SAMPLER_WAVES; ++w) total += scratch[w];
  __syncthreads();
  return total;
}

// (value, index) -> the largest value, lowest index among equals
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov,
                                             int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void block_argmax(float& v, int& i, float* sf,
                                             int* si) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, WAVE);
    const int oi = __shfl_xor(i, off, WAVE);
    argmax_merge(v, i, ov, oi);
  }
  if (threadIdx.x % WAVE == 0) {
    sf[threadIdx.x / WAVE] = v;
    si[threadIdx.x / WAVE] = i;
  }
  __syncthreads();
  v = sf[0];
  i = si[0];
#pragma unroll
  for (int w = 1; w < SAMPLER_WAVES; ++w) argmax_merge(v, i, sf[w], si[w]);
  __syncthreads();
}

// Inclusive suffix sum over the 256 histogram bins: thread t < 256 passes
// bin t and gets sum{bin b : b >= t}. Every thread of the block calls.
template <typename S>
__device__ __forceinline__ S suffix_sum256(S v, S* wave_tot) {
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const S o = __shfl_down(v, off, WAVE);
    if (lane + off < WAVE) v += o;
  }
  if (lane == 0 && wave < 4) wave_tot[wave] = v;
  __syncthreads();
  if (wave < 4)
    for (int w = wave + 1; w < 4; ++w) v += wave_tot[w];
  __syncthreads();
  return v;
}

struct Hist {
  int cnt[256];
  u64 mass[256];
  int sfx_cnt[257];
  u64 sfx_mass[257];
  int wtot_i[4];
  u64 wtot_m[4];
  int sel;
};

__device__ __forceinline__ void hist_clear(Hist& h) {
  const int tid = threadIdx.x;
  if (tid < 256) { h.cnt[tid] = 0; h.mass[tid] = 0; }
  if (tid == 0) { h.sel = 0; h.sfx_cnt[256] = 0; h.sfx_mass[256] = 0; }
  __syncthreads();
}

// Bin holding the k_rem-th largest element of the histogram; `above`
// receives the count in the bins over it.
__device__ __forceinline__ int select_by_count(Hist& h, int k_rem,
                                               int& above) {
  const int tid = threadIdx.x;
  __syncthreads();                       // histogram complete
  const int c = tid < 256 ? h.cnt[tid] : 0;
  const int s = suffix_sum256<int>(c, h.wtot_i);
  if (tid < 256) {
    h.sfx_cnt[tid] = s;
    if (c > 0 && s >= k_rem) atomicMax(&h.sel, tid);
  }
  __syncthreads();
  const int b = h.sel;
  above = h.sfx_cnt[b + 1];
  __syncthreads();
  return b;
}

// Highest non-empty bin at which the mass from the top (`above` + the
// histogram's suffix) reaches `target`; `above` is advanced past the bins
// over it. Masses are integers, so the sub-bins of a chosen bin add up to
// it exactly and a bin always qualifies.
__device__ __forceinline__ int select_by_mass(Hist& h, double target,
                                              u64& above) {
  const int tid = threadIdx.x;
  __syncthreads();
  const int c = tid < 256 ? h.cnt[tid] : 0;
  const u64 m = tid < 256 ? h.mass[tid] : 0;
  const u64 s = suffix_sum256<u64>(m, h.wtot_m);
  if (tid < 256) {
    h.sfx_mass[tid] = s;
    if (c > 0 && (double)(above + s) >= target) atomicMax(&h.sel, tid);
  }
  __syncthreads();
  const int b = h.sel;
  above += h.sfx_mass[b + 1];
  __syncthreads();
  return b;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1,
                                              uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1,
                                              uint32_t& o0, uint32_t& o1,
                                              uint32_t& o2, uint32_t& o3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o0 = c0; o1 = c1; o2 = c2; o3 = c3;
}

template <typename T>
__global__ __launch_bounds__(SAMPLER_THREADS) void sample_kernel(
    const T* __restrict__ logits, const float* __restrict__ temperature,
    const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
    const int64_t* __restrict__ seed, const int32_t* __restrict__ pos, int V,
    int64_t* __restrict__ tokens, float* __restrict__ logprobs,
    int32_t* __restrict__ n_kept, float* __restrict__ threshold) {
  constexpr int KEYBITS = 8 * (int)sizeof(T);
  constexpr int NDIG = (int)sizeof(T);
  __shared__ Hist h;
  __shared__ float red_f[SAMPLER_WAVES];
  __shared__ int red_i[SAMPLER_WAVES];

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const T* row = logits + (int64_t)r * V;

  // ---- pass 1: raw max (lowest index), online sum of exp(l - max) ----
  float m_t = -FLT_MAX, s_t = 0.f;
  int i_t = 0x7FFFFFFF;
  for_row(row, V, [&](int i, T raw) {
    const float l = raw_to_f32(raw);
    if (l > m_t) {
      s_t = s_t * expf(m_t - l) + 1.f;
      m_t = l;
      i_t = i;
    } else {
      s_t += expf(l - m_t);
      if (l == m_t && i < i_t) i_t = i;
    }
  });
  float M = m_t;
  int arg = i_t;
  block_argmax(M, arg, red_f, red_i);
  if ((uint32_t)arg >= (uint32_t)V) arg = 0;     // an all-NaN row
  const float S = block_sum_f32(s_t * expf(m_t - M), red_f);
  const float lse = M + logf(S);

  const float T_ = temperature[r];
  if (!(T_ > 0.f)) {
    if (tid == 0) {
      tokens[r] = arg;
      logprobs[r] = M - lse;
      n_kept[r] = V;
      threshold[r] = -INFINITY;
    }
    return;
  }
  const float inv = 1.0f / T_;
  const float mz = __fmul_rn(M, inv);
  const int k = top_k[r];
  const float p = top_p[r];

  // ---- top-k: the k-th largest raw key, one digit per pass ----
  float tau = -INFINITY;
  if (k > 0 && k < V) {
    uint32_t prefix = 0;
    int k_rem = k;
    for (int d = 0; d < NDIG; ++d) {
      const int shift = KEYBITS - 8 * (d + 1);
      hist_clear(h);
      for_row(row, V, [&](int, T raw) {
        const uint32_t key = key_of(raw);
        if ((uint32_t)((uint64_t)key >> (shift + 8)) == prefix)
          atomicAdd(&h.cnt[(key >> shift) & 0xFFu], 1);
      });
      int above;
      const int b = select_by_count(h, k_rem, above);
      k_rem -= above;
      prefix = (prefix << 8) | (uint32_t)b;
    }
    tau = __fmul_rn(key_to_f32<T>(prefix), inv);
  }

  // ---- top-p over {z >= tau}: largest v with mass{z >= v} >= p * W ----
  if (p < 1.f) {
    uint32_t prefix = 0;
    u64 above = 0;
    double target = 0.0;
    for (int d = 0; d < NDIG; ++d) {
      const int shift = KEYBITS - 8 * (d + 1);
      hist_clear(h);
      for_row(row, V, [&](int, T raw) {
        const uint32_t key = key_of(raw);
        if ((uint32_t)((uint64_t)key >> (shift + 8)) != prefix) return;
        const float z = __fmul_rn(raw_to_f32(raw), inv);
        if (!(z >= tau)) return;
        const float w = expf(__fsub_rn(z, mz));
        const int bin = (key >> shift) & 0xFFu;
        atomicAdd(&h.cnt[bin], 1);
        atomicAdd(&h.mass[bin], (u64)__float2ull_rn(w * MASS_SCALE));
      });
      if (d == 0) {
        // W is the whole first histogram; sum it before selecting
        __syncthreads();
        const u64 mine = tid < 256 ? h.mass[tid] : 0;
        const u64 W = suffix_sum256<u64>(mine, h.wtot_m);
        if (tid == 0) h.sfx_mass[0] = W;
        __syncthreads();
        target = (double)p * (double)h.sfx_mass[0];
      }
      const int b = select_by_mass(h, target, above);
      prefix = (prefix << 8) | (uint32_t)b;
    }
    tau = fmaxf(tau, __fmul_rn(key_to_f32<T>(prefix), inv));
  }

  // ---- Gumbel-max over the kept set ----
  const uint64_t sd = (uint64_t)seed[r];
  const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
  const uint32_t n = (uint32_t)pos[r];
  float best = -INFINITY;
  int best_i = 0x7FFFFFFF;
  int kept = 0;
  int cached = -1;
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
  for_row(row, V, [&](int i, T raw) {
    const float z = __fmul_rn(raw_to_f32(raw), inv);
    if (!(z >= tau)) return;
    ++kept;
    const int blk = i >> 2;
    if (blk != cached) {
      philox4x32_10((uint32_t)blk, n, 0u, 0u, k0, k1, x0, x1, x2, x3);
      cached = blk;
    }
    const int wsel = i & 3;
    const uint32_t x = wsel == 0 ? x0 : wsel == 1 ? x1 : wsel == 2 ? x2 : x3;
    const float u =
        fminf(__fmul_rn(__fadd_rn((float)(x >> 8), 0.5f), U_SCALE), U_MAX);
    const float g = -logf(-logf(u));
    argmax_merge(best, best_i, __fadd_rn(z, g), i);
  });
  block_argmax(best, best_i, red_f, red_i);
  kept = block_sum_i32(kept, red_i);
  // the kept set holds the maximum, so only NaN logits can leave it empty
  if ((uint32_t)best_i >= (uint32_t)V) best_i = arg;
  if (tid == 0) {
    tokens[r] = best_i;
    logprobs[r] = raw_to_f32(row[best_i]) - lse;
    n_kept[r] = kept;
    threshold[r] = __fmul_rn(tau, T_);
  }
}

}  // namespace

extern "C" {

// One launch samples the whole batch: grid = B rows, no host sync.
// logits: [B, V] bf16 (is_f32 = 0) or fp32 (is_f32 = 1), rows contiguous.
hipError_t lds_sample(const void* logits, const float* temperature,
                      const int32_t* top_k, const float* top_p,
                      const int64_t* seed, const int32_t* pos, int B, int V,
                      int is_f32, int64_t* tokens, float* logprobs,
                      int32_t* n_kept, float* threshold, hipStream_t stream) {
  if (B == 0) return hipSuccess;
  if (V <= 0) return hipErrorInvalidValue;
  dim3 grid((uint32_t)B), block(SAMPLER_THREADS);
  if (is_f32) {
    hipLaunchKernelGGL(sample_kernel<float>, grid, block, 0, stream,
                       (const float*)logits, temperature, top_k, top_p, seed,
                       pos, V, tokens, logprobs, n_kept, threshold);
  } else {
    hipLaunchKernelGGL(sample_kernel<short>, grid, block, 0, stream,
                       (const short*)logits, temperature, top_k, top_p, seed,
                       pos, V, tokens, logprobs, n_kept, threshold);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
