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
//
// sample_ext is the same kernel with EXT = true: every pass sees the
// penalised fp32 logit x (repetition, frequency and presence penalties from
// the request's token-state row, computed on the fly), the selects run on
// the fp32 key of x (4 digit passes, also for bf16 input), min_p joins the
// thresholds, a top-N phase on the raw keys reports the alternatives, and
// the chosen token is counted into the state row. token_state_fill builds a
// state row from a request's prompt and output so far.
#include "hip_common.h"
#include "launchers.h"

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

// for_row with the request's token-state row alongside (sample_ext): calls
// f(index, raw element, state element). The logits keep for_row's thread
// mapping and order, so sums over a row round as they do there. A state row
// starts 16-byte aligned (Vs % 8 == 0), so when the logits row does too
// (head == 0) the state is read with one vector load per logits vector;
// otherwise element by element. st == nullptr (no state) passes 0.
template <typename T> struct StateVec;
template <> struct StateVec<short> { typedef short8 type; };
template <> struct StateVec<float> { typedef short4v type; };

template <typename T, typename F>
__device__ __forceinline__ void for_row_state(const T* __restrict__ row,
                                              const short* st, int V, F&& f) {
  typedef typename RowVec<T>::type vec_t;
  typedef typename StateVec<T>::type svec_t;
  constexpr int VEC = 16 / (int)sizeof(T);
  const int tid = threadIdx.x;
  int head = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) /
                   sizeof(T));
  if (head > V) head = V;
  if (tid < head) f(tid, row[tid], st ? st[tid] : (short)0);
  const int nvec = (V - head) / VEC;
  const vec_t* rv = (const vec_t*)(row + head);
  for (int c = tid; c < nvec; c += SAMPLER_THREADS) {
    const vec_t v = rv[c];
    const int base = head + c * VEC;
    svec_t sv = (svec_t)(short)0;
    if (st) {
      if (head == 0) {
        sv = ((const svec_t*)st)[c];
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) sv[j] = st[base + j];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) f(base + j, (T)v[j], (short)sv[j]);
  }
  const int t = head + nvec * VEC + tid;
  if (t < V) f(t, row[t], st ? st[t] : (short)0);
}

// Element access of sample_kernel<T, EXT>. Without EXT it is the identity:
// the value is the raw logit, the radix key is the key of its storage type
// and no state is read. With EXT the value is the penalised fp32 logit x of
// step 0 of the contract, computed on the fly from the raw logit and the
// state element, each operation rounded on its own (no FMA contraction),
// and the radix key is the fp32 key of x.
constexpr int STATE_COUNT_MASK = 0x3FFF;       // c, saturating at 16383

template <typename T, bool EXT> struct Elem;
template <typename T> struct Elem<T, false> {
  typedef T key_t;
  __device__ __forceinline__ float x(T raw, short) const {
    return raw_to_f32(raw);
  }
  __device__ __forceinline__ uint32_t key(T raw, short) const {
    return key_of(raw);
  }
  template <typename F>
  __device__ __forceinline__ void each(const T* __restrict__ row, int V,
                                       F&& f) const {
    for_row(row, V, [&](int i, T raw) { f(i, raw, (short)0); });
  }
};
template <typename T> struct Elem<T, true> {
  typedef float key_t;
  const short* st;
  float rep, pres, freq;
  __device__ __forceinline__ float x(T raw, short s) const {
    float v = raw_to_f32(raw);
    if (s != 0) v = v > 0.f ? __fdiv_rn(v, rep) : __fmul_rn(v, rep);
    const int c = (int)s & STATE_COUNT_MASK;
    v = __fsub_rn(v, __fmul_rn(freq, (float)c));
    return __fsub_rn(v, c > 0 ? pres : 0.f);
  }
  __device__ __forceinline__ uint32_t key(T raw, short s) const {
    return key_of(x(raw, s));
  }
  template <typename F>
  __device__ __forceinline__ void each(const T* __restrict__ row, int V,
                                       F&& f) const {
    for_row_state(row, st, V, f);
  }
};

// sample_ext adds ExtArgs (launchers.h) to the launch; the plain sampler
// carries nothing.
struct NoExtArgs {};
template <bool EXT> struct ExtArgsOf { typedef NoExtArgs type; };
template <> struct ExtArgsOf<true> { typedef ExtArgs type; };

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

// ---- top-N alternatives (sample_ext) ----
constexpr int TOPN_MAX = 20;

// Key of a raw logit for top-N: key_of with -0 folded onto +0, so that
// "equal value" and "equal key" are the same thing.
__device__ __forceinline__ uint32_t topn_key(short v) {
  return key_of(v == (short)0x8000 ? (short)0 : v);
}
__device__ __forceinline__ uint32_t topn_key(float v) {
  return key_of(v + 0.f);
}

// The N entries of one row with the largest raw logit, ordered by (value
// descending, index ascending), as (index, logit - lse); entries from N to
// n_top are (-1, -inf). Every thread of the block calls.
//   1. count select with k = N on the raw keys: the threshold key, and how
//      many of the elements that carry it are still needed (k_rem);
//   2. when not all of them are needed, a second count select, on V-1-index
//      among the elements with the threshold key: the k_rem-th lowest index;
//   3. one collect pass into LDS (exactly N entries), then each entry finds
//      its rank among the N by counting.
// bf16 rows tie heavily, so step 2 is a common path there.
template <typename T>
__device__ __forceinline__ void topn_phase(const T* __restrict__ row, int V,
                                           int N, int n_top, float lse,
                                           Hist& h,
                                           int64_t* __restrict__ out_tok,
                                           float* __restrict__ out_lp) {
  constexpr int KEYBITS = 8 * (int)sizeof(T);
  constexpr int NDIG = (int)sizeof(T);
  __shared__ uint32_t s_key[TOPN_MAX];
  __shared__ int s_idx[TOPN_MAX];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  if (N > n_top) N = n_top;
  if (N > V) N = V;
  if (N < 0) N = 0;
  if (tid >= N && tid < n_top) {
    out_tok[tid] = -1;
    out_lp[tid] = -INFINITY;
  }
  if (N == 0) return;

  uint32_t prefix = 0;
  int k_rem = N, ties = 0;
  for (int d = 0; d < NDIG; ++d) {
    const int shift = KEYBITS - 8 * (d + 1);
    hist_clear(h);
    for_row(row, V, [&](int, T raw) {
      const uint32_t key = topn_key(raw);
      if ((uint32_t)((uint64_t)key >> (shift + 8)) == prefix)
        atomicAdd(&h.cnt[(key >> shift) & 0xFFu], 1);
    });
    int above;
    const int b = select_by_count(h, k_rem, above);
    k_rem -= above;
    prefix = (prefix << 8) | (uint32_t)b;
    ties = h.cnt[b];
    __syncthreads();                     // read before the next clear
  }

  // elements with the threshold key are taken up to this index
  int idx_max = V - 1;
  if (k_rem < ties) {
    const int nbits = 32 - __clz(V - 1);           // ties >= 2, so V >= 2
    const int nd = (nbits + 7) / 8;
    uint32_t ip = 0;
    int kr = k_rem;
    for (int d = 0; d < nd; ++d) {
      const int shift = 8 * (nd - 1 - d);
      hist_clear(h);
      for_row(row, V, [&](int i, T raw) {
        if (topn_key(raw) != prefix) return;
        const uint32_t ik = (uint32_t)(V - 1 - i);
        if ((uint32_t)((uint64_t)ik >> (shift + 8)) == ip)
          atomicAdd(&h.cnt[(ik >> shift) & 0xFFu], 1);
      });
      int above;
      const int b = select_by_count(h, kr, above);
      kr -= above;
      ip = (ip << 8) | (uint32_t)b;
    }
    idx_max = V - 1 - (int)ip;
  }

  if (tid == 0) s_n = 0;
  __syncthreads();
  for_row(row, V, [&](int i, T raw) {
    const uint32_t key = topn_key(raw);
    if (key > prefix || (key == prefix && i <= idx_max)) {
      const int j = atomicAdd(&s_n, 1);
      if (j < TOPN_MAX) { s_key[j] = key; s_idx[j] = i; }
    }
  });
  __syncthreads();
  const int n = s_n < N ? s_n : N;
  if (tid < n) {
    const uint32_t key = s_key[tid];
    const int idx = s_idx[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j)
      rank += (s_key[j] > key || (s_key[j] == key && s_idx[j] < idx)) ? 1 : 0;
    out_tok[rank] = idx;
    out_lp[rank] = key_to_f32<T>(key) - lse;
  }
  __syncthreads();
}

// sample_kernel<T, false> is the plain sampler (lds_sample); <T, true> is
// sample_ext: penalties from the token state, min_p, top-N alternatives and
// the state update, sharing every pass with the plain one through Elem.
template <typename T, bool EXT>
__global__ __launch_bounds__(SAMPLER_THREADS) void sample_kernel(
    const T* __restrict__ logits, const float* __restrict__ temperature,
    const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
    const int64_t* __restrict__ seed, const int32_t* __restrict__ pos, int V,
    int64_t* __restrict__ tokens, float* __restrict__ logprobs,
    int32_t* __restrict__ n_kept, float* __restrict__ threshold,
    typename ExtArgsOf<EXT>::type ea) {
  typedef Elem<T, EXT> elem_t;
  typedef typename elem_t::key_t K;
  constexpr int KEYBITS = 8 * (int)sizeof(K);
  constexpr int NDIG = (int)sizeof(K);
  __shared__ Hist h;
  __shared__ float red_f[SAMPLER_WAVES];
  __shared__ int red_i[SAMPLER_WAVES];

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const T* row = logits + (int64_t)r * V;

  elem_t el;
  short* st_w = nullptr;                 // this row's state, if it has one
  if constexpr (EXT) {
    const int sr = ea.state_row[r];
    if (ea.state != nullptr && sr >= 0 && sr < ea.R)
      st_w = ea.state + (int64_t)sr * ea.Vs;
    el.st = st_w;
    el.rep = ea.rep[r];
    el.pres = ea.pres[r];
    el.freq = ea.freq[r];
  }

  // ---- pass 1: raw max (lowest index), online sum of exp(l - max); with
  // EXT also the maximum of x, which takes over argmax and m ----
  float m_t = -FLT_MAX, s_t = 0.f;
  int i_t = 0x7FFFFFFF;
  float mx_t = -FLT_MAX;
  int ix_t = 0x7FFFFFFF;
  el.each(row, V, [&](int i, T raw, short s) {
    const float l = raw_to_f32(raw);
    if (l > m_t) {
      s_t = s_t * expf(m_t - l) + 1.f;
      m_t = l;
      i_t = i;
    } else {
      s_t += expf(l - m_t);
      if (l == m_t && i < i_t) i_t = i;
    }
    if constexpr (EXT) argmax_merge(mx_t, ix_t, el.x(raw, s), i);
  });
  float M = m_t;
  int arg = i_t;
  block_argmax(M, arg, red_f, red_i);
  float Mx = M;                          // maximum of x: the raw one or
  if constexpr (EXT) {                   // the penalised one
    Mx = mx_t;
    arg = ix_t;
    block_argmax(Mx, arg, red_f, red_i);
  }
  if ((uint32_t)arg >= (uint32_t)V) arg = 0;     // an all-NaN row
  const float S = block_sum_f32(s_t * expf(m_t - M), red_f);
  const float lse = M + logf(S);

  if constexpr (EXT) {
    if (ea.n_top > 0)
      topn_phase<T>(row, V, ea.top_n[r], ea.n_top, lse, h,
                    ea.top_tokens + (int64_t)r * ea.n_top,
                    ea.top_logprobs + (int64_t)r * ea.n_top);
  }

  const float T_ = temperature[r];
  if (!(T_ > 0.f)) {
    if (tid == 0) {
      tokens[r] = arg;
      if constexpr (EXT) {
        logprobs[r] = raw_to_f32(row[arg]) - lse;
        // every read of the state row lies before block_argmax's barrier
        if (st_w != nullptr) {
          const short s = st_w[arg];
          if (((int)s & STATE_COUNT_MASK) < STATE_COUNT_MASK)
            st_w[arg] = (short)(s + 1);
        }
      } else {
        logprobs[r] = M - lse;
      }
      n_kept[r] = V;
      threshold[r] = -INFINITY;
    }
    return;
  }
  const float inv = 1.0f / T_;
  const float mz = __fmul_rn(Mx, inv);
  const int k = top_k[r];
  const float p = top_p[r];

  // ---- top-k: the k-th largest key, one digit per pass ----
  float tau = -INFINITY;
  if (k > 0 && k < V) {
    uint32_t prefix = 0;
    int k_rem = k;
    for (int d = 0; d < NDIG; ++d) {
      const int shift = KEYBITS - 8 * (d + 1);
      hist_clear(h);
      el.each(row, V, [&](int, T raw, short s) {
        const uint32_t key = el.key(raw, s);
        if ((uint32_t)((uint64_t)key >> (shift + 8)) == prefix)
          atomicAdd(&h.cnt[(key >> shift) & 0xFFu], 1);
      });
      int above;
      const int b = select_by_count(h, k_rem, above);
      k_rem -= above;
      prefix = (prefix << 8) | (uint32_t)b;
    }
    tau = __fmul_rn(key_to_f32<K>(prefix), inv);
  }

  // ---- top-p over {z >= tau}: largest v with mass{z >= v} >= p * W ----
  if (p < 1.f) {
    uint32_t prefix = 0;
    u64 above = 0;
    double target = 0.0;
    for (int d = 0; d < NDIG; ++d) {
      const int shift = KEYBITS - 8 * (d + 1);
      hist_clear(h);
      el.each(row, V, [&](int, T raw, short s) {
        const uint32_t key = el.key(raw, s);
        if ((uint32_t)((uint64_t)key >> (shift + 8)) != prefix) return;
        const float z = __fmul_rn(el.x(raw, s), inv);
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
    tau = fmaxf(tau, __fmul_rn(key_to_f32<K>(prefix), inv));
  }

  // ---- min_p: tau_m = max z + log(min_p), the log correctly rounded ----
  if constexpr (EXT) {
    const float mp = ea.min_p[r];
    if (mp > 0.f)
      tau = fmaxf(tau, __fadd_rn(mz, (float)log((double)mp)));
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
  el.each(row, V, [&](int i, T raw, short s) {
    const float z = __fmul_rn(el.x(raw, s), inv);
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
    if constexpr (EXT) {
      // the draw's barriers lie behind every read of the state row, and
      // this workgroup is the row's only writer
      if (st_w != nullptr) {
        const short s = st_w[best_i];
        if (((int)s & STATE_COUNT_MASK) < STATE_COUNT_MASK)
          st_w[best_i] = (short)(s + 1);
      }
    }
  }
}

// ---- token_state_fill ----
// One workgroup per listed state row: clear columns [0, V), set bit 14 for
// the prompt ids, count the output ids. Two ids 2j and 2j+1 share a 32-bit
// word (Vs is even, so a word never spans two rows), and the same id can
// come hundreds of times in one call, so all updates are 32-bit atomics on
// the word: an OR for bit 14, and for the count a compare-and-swap loop
// that adds to the 14-bit field alone and stops at 16383, so that nothing
// ever carries into bit 14 or into the neighbouring half-word. Equal ids
// within a wave are added in one go by the lowest lane that holds them,
// which keeps a 16400-fold id at a few hundred swaps.
constexpr int FILL_THREADS = 1024;

__global__ __launch_bounds__(FILL_THREADS) void token_state_fill_kernel(
    short* __restrict__ state, int R, int64_t Vs, int V,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ toks,
    int64_t n_toks, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ n_prompt) {
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  const int sr = rows[q];
  if (sr < 0 || sr >= R) return;
  short* st = state + (int64_t)sr * Vs;

  // clear [0, V): whole 16-byte vectors, then the last V % 8 elements one
  // by one (padding columns are never written)
  const int nvec = V / 8;
  short8* sv = (short8*)st;
  for (int c = tid; c < nvec; c += FILL_THREADS) sv[c] = (short8)(short)0;
  if (nvec * 8 + tid < V) st[nvec * 8 + tid] = 0;
  __threadfence_block();
  __syncthreads();

  int64_t beg = offsets[q], end = offsets[q + 1];
  beg = beg < 0 ? 0 : (beg > n_toks ? n_toks : beg);
  end = end < beg ? beg : (end > n_toks ? n_toks : end);
  int64_t np = n_prompt[q];
  np = np < 0 ? 0 : (np > end - beg ? end - beg : np);
  uint32_t* words = (uint32_t*)st;

  for (int64_t t = beg + tid; t < beg + np; t += FILL_THREADS) {
    const int id = toks[t];
    if (id < 0 || id >= V) continue;
    atomicOr(&words[id >> 1], 0x4000u << ((id & 1) * 16));
  }

  // every lane of a wave takes part in each round of the loop below
  const int64_t n_out = end - (beg + np);
  const int64_t rounds = (n_out + FILL_THREADS - 1) / FILL_THREADS;
  for (int64_t it = 0; it < rounds; ++it) {
    const int64_t t = beg + np + it * FILL_THREADS + tid;
    int id = t < end ? toks[t] : -1;
    if (id >= V) id = -1;
    bool todo = id >= 0;
    while (true) {
      const unsigned long long live = __ballot(todo);
      if (live == 0) break;
      const int leader = __ffsll((long long)live) - 1;
      const int lid = __shfl(id, leader, WAVE);
      const bool mine = todo && id == lid;
      const int add = __popcll(__ballot(mine));
      if (tid % WAVE == leader) {
        const int shift = (lid & 1) * 16;
        uint32_t* w = &words[lid >> 1];
        uint32_t old = *w;
        while (true) {
          const int c = (int)((old >> shift) & (uint32_t)STATE_COUNT_MASK);
          if (c == STATE_COUNT_MASK) break;
          int nc = c + add;
          if (nc > STATE_COUNT_MASK) nc = STATE_COUNT_MASK;
          const uint32_t want = old + ((uint32_t)(nc - c) << shift);
          const uint32_t prev = atomicCAS(w, old, want);
          if (prev == old) break;
          old = prev;
        }
      }
      if (mine) todo = false;
    }
  }
}

// One launch samples the whole batch: grid = B rows, no host sync.
template <bool EXT>
void launch_sample(const SampleArgs& a, typename ExtArgsOf<EXT>::type ea,
                   hipStream_t stream) {
  dim3 grid((uint32_t)a.B), block(SAMPLER_THREADS);
  if (a.is_f32) {
    hipLaunchKernelGGL((sample_kernel<float, EXT>), grid, block, 0, stream,
                       (const float*)a.logits, a.temperature, a.top_k,
                       a.top_p, a.seed, a.pos, a.V, a.tokens, a.logprobs,
                       a.n_kept, a.threshold, ea);
  } else {
    hipLaunchKernelGGL((sample_kernel<short, EXT>), grid, block, 0, stream,
                       (const short*)a.logits, a.temperature, a.top_k,
                       a.top_p, a.seed, a.pos, a.V, a.tokens, a.logprobs,
                       a.n_kept, a.threshold, ea);
  }
}

}  // namespace

hipError_t lds_sample(const SampleArgs& a, hipStream_t stream) {
  if (a.B == 0) return hipSuccess;
  if (a.V <= 0) return hipErrorInvalidValue;
  launch_sample<false>(a, NoExtArgs{}, stream);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// sample with penalties, min_p, top-N and the token-state update
// (DEVELOPMENT.md "Sampling").
hipError_t lds_sample_ext(const SampleArgs& a, const ExtArgs& ea,
                          hipStream_t stream) {
  if (a.B == 0) return hipSuccess;
  if (a.V <= 0 || ea.n_top < 0 || ea.n_top > TOPN_MAX)
    return hipErrorInvalidValue;
  if (ea.state != nullptr && (ea.Vs < a.V || ea.Vs % 8 != 0 || ea.R < 0))
    return hipErrorInvalidValue;
  launch_sample<true>(a, ea, stream);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_token_state_fill(int16_t* state, int R, int64_t Vs, int V,
                                const int32_t* rows, int n,
                                const int32_t* toks, int64_t n_toks,
                                const int64_t* offsets,
                                const int32_t* n_prompt, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (V <= 0 || Vs < V || Vs % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_state_fill_kernel, dim3((uint32_t)n),
                     dim3(FILL_THREADS), 0, stream, (short*)state, R, Vs, V,
                     rows, toks, n_toks, offsets, n_prompt);
  HIP_CHECK_LAST();
  return hipSuccess;
}
