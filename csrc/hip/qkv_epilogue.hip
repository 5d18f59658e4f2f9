// qkv_epilogue.hip — everything between the QKV GEMM and attention, in one
// kernel (gfx950).
//
// The GEMM returns qkv [T, (QH + 2*KVH) * D] bf16, one row per token:
// QH query heads, then KVH key heads, then KVH value heads. This kernel reads
// each row once and
//   * writes the rotated query heads to a contiguous q [T, QH, D],
//   * writes the rotated key heads and the plain value heads straight into
//     their paged-pool slot (bf16, or fp8 with optional per-head scales).
// It replaces three strided copies, rope_kernel and reshape_and_cache_kernel,
// and computes what they compute: the rotation is rope_rotate_pair and the
// store is store_kv8, the code those two kernels run (hip_common.h).
//
// All traffic is short8 (16 B per lane). One (token, head) task takes D/16
// lanes; a lane owns elements d..d+7 and d+D/2..d+D/2+7 of the head, so both
// halves of every rotate-half pair sit in the same lane. No LDS, no barriers.
#include "hip_common.h"
#include "launchers.h"

namespace {

// rotate 8 (lo[j], hi[j]) pairs by the angles cs[2*j], cs[2*j+1] = cos, sin
__device__ __forceinline__ void rope_rotate8(short8& lo, short8& hi,
                                             const float* __restrict__ cs) {
  const float4v* cs4 = (const float4v*)cs;  // 16 floats, 64-byte aligned
  float4v t[4] = {cs4[0], cs4[1], cs4[2], cs4[3]};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float c = t[j / 2][(j % 2) * 2];
    const float s = t[j / 2][(j % 2) * 2 + 1];
    short o1, o2;
    rope_rotate_pair(lo[j], hi[j], c, s, o1, o2);
    lo[j] = o1;
    hi[j] = o2;
  }
}

template <typename CT>
__device__ __forceinline__ void store_kv8_scaled(CT* p, short8 v,
                                                 const float* inv_scale,
                                                 int h) {
  if constexpr (std::is_same<CT, unsigned char>::value) {
    if (inv_scale != nullptr) {
      store_kv8(p, v, inv_scale[h]);
      return;
    }
  }
  store_kv8(p, v);
}

//  qkv: [T, (QH + 2*KVH) * D] bf16; cos_sin: [max_pos, D/2, 2] f32;
//  positions: [T] int32; slots: [T] int64 (block*BS + row, < 0 = padding:
//  no K/V store, q still written); q_out: [T, QH, D] bf16;
//  k_cache/v_cache: [NB, KVH, BS, D] bf16|fp8 (one layer's slice);
//  k_inv_scale/v_inv_scale: [KVH] f32, fp8 cache only; null = unscaled store
template <typename CT>
__global__ __launch_bounds__(256) void qkv_rope_cache_kernel(
    const short* __restrict__ qkv, const float* __restrict__ cos_sin,
    const int32_t* __restrict__ positions, const int64_t* __restrict__ slots,
    short* __restrict__ q_out, CT* __restrict__ k_cache,
    CT* __restrict__ v_cache, const float* __restrict__ k_inv_scale,
    const float* __restrict__ v_inv_scale, int64_t n_tokens, int qh, int kvh,
    int bs, int d) {
  const int half = d / 2;
  const int lanes = d / 16;           // lanes per (token, head) task
  const int heads = qh + 2 * kvh;
  const int64_t total = n_tokens * heads * lanes;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int d0 = (int)(i % lanes) * 8;
    const int64_t task = i / lanes;
    const int head = (int)(task % heads);
    const int64_t t = task / heads;
    const short* src = qkv + (t * heads + head) * d + d0;
    if (head < qh) {
      short8 lo = *(const short8*)src;
      short8 hi = *(const short8*)(src + half);
      rope_rotate8(lo, hi,
                   cos_sin + ((int64_t)positions[t] * half + d0) * 2);
      short* dst = q_out + (t * qh + head) * d + d0;
      *(short8*)dst = lo;
      *(short8*)(dst + half) = hi;
      continue;
    }
    const int64_t slot = slots[t];
    if (slot < 0) continue;  // padding token
    short8 lo = *(const short8*)src;
    short8 hi = *(const short8*)(src + half);
    const bool is_k = head < qh + kvh;
    const int h = is_k ? head - qh : head - qh - kvh;
    const int64_t block = slot / bs, row = slot % bs;
    const int64_t dst_off = (((block * kvh + h) * bs) + row) * d + d0;
    if (is_k) {
      rope_rotate8(lo, hi,
                   cos_sin + ((int64_t)positions[t] * half + d0) * 2);
      store_kv8_scaled(k_cache + dst_off, lo, k_inv_scale, h);
      store_kv8_scaled(k_cache + dst_off + half, hi, k_inv_scale, h);
    } else {
      store_kv8_scaled(v_cache + dst_off, lo, v_inv_scale, h);
      store_kv8_scaled(v_cache + dst_off + half, hi, v_inv_scale, h);
    }
  }
}

}  // namespace

hipError_t lds_qkv_rope_cache(const void* qkv, const float* cos_sin,
                              const int32_t* positions, const int64_t* slots,
                              void* q_out, void* k_cache, void* v_cache,
                              int64_t n_tokens, int n_q_heads, int kvh, int bs,
                              int d, int kv_fp8, const float* k_inv_scale,
                              const float* v_inv_scale, hipStream_t stream) {
  if (n_tokens == 0) return hipSuccess;
  const int threads = 256;
  const int64_t total = n_tokens * (n_q_heads + 2 * kvh) * (d / 16);
  // decode (T = 256, Llama-3-8B) is 384 blocks, over one per CU; a prefill
  // pass grid-strides over 2048 blocks (guide G11)
  int64_t blocks = (total + threads - 1) / threads;
  if (blocks > 2048) blocks = 2048;
  if (kv_fp8) {
    hipLaunchKernelGGL(qkv_rope_cache_kernel<unsigned char>,
                       dim3((uint32_t)blocks), dim3(threads), 0, stream,
                       (const short*)qkv, cos_sin, positions, slots,
                       (short*)q_out, (unsigned char*)k_cache,
                       (unsigned char*)v_cache, k_inv_scale, v_inv_scale,
                       n_tokens, n_q_heads, kvh, bs, d);
  } else {
    if (k_inv_scale || v_inv_scale) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qkv_rope_cache_kernel<short>, dim3((uint32_t)blocks),
                       dim3(threads), 0, stream, (const short*)qkv, cos_sin,
                       positions, slots, (short*)q_out, (short*)k_cache,
                       (short*)v_cache, nullptr, nullptr, n_tokens, n_q_heads,
                       kvh, bs, d);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}
