// kv_cache.hip — paged-KV pool maintenance kernels for gfx950.
//
// Pool layout (per GPU, sized for the 288 GB HBM3E budget):
//   kv_pool: [n_layers, 2(K/V), n_blocks, n_kv_heads, block_size, head_dim] bf16
// One (layer, K/V, block) = a contiguous [n_kv_heads, block_size, head_dim]
// chunk whose per-head [block_size x head_dim] rows are contiguous — the
// MFMA-tile-aligned layout consumed zero-repack by both the decode attention
// kernel and the xGMI transfer engine.
#include "hip_common.h"
#include "launchers.h"

namespace {

// Scatter the freshly projected K/V of each token into its pool slot.
//  k_new/v_new: [T, KVH, D] bf16; slot_mapping: [T] int64 (block*BS + row)
//  k_cache/v_cache: [NB, KVH, BS, D] bf16|fp8 (one layer's slice)
//  k_inv_scale/v_inv_scale: [KVH] fp32 (1 / per-head scale of this layer),
//  fp8 cache only; null = unscaled store
template <typename CT>
__global__ void reshape_and_cache_kernel(const short* __restrict__ k_new,
                                         const short* __restrict__ v_new,
                                         CT* __restrict__ k_cache,
                                         CT* __restrict__ v_cache,
                                         const int64_t* __restrict__ slots,
                                         const float* __restrict__ k_inv_scale,
                                         const float* __restrict__ v_inv_scale,
                                         int n_tokens, int kvh, int bs, int d) {
  const int t = blockIdx.x;
  if (t >= n_tokens) return;
  int64_t slot = slots[t];
  if (slot < 0) return;  // padding token
  int64_t block = slot / bs, row = slot % bs;
  // per (head, 16B chunk): blockDim.x = kvh * d/8 capped; grid-stride inside
  const int chunks_per_head = d / 8;
  const int total = kvh * chunks_per_head;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    int h = i / chunks_per_head, c = i % chunks_per_head;
    const short8* src_k = (const short8*)(k_new + ((int64_t)t * kvh + h) * d);
    const short8* src_v = (const short8*)(v_new + ((int64_t)t * kvh + h) * d);
    int64_t dst_off = (((block * kvh + h) * bs) + row) * d;
    if constexpr (std::is_same<CT, unsigned char>::value) {
      if (k_inv_scale != nullptr) {
        store_kv8(k_cache + dst_off + c * 8, src_k[c], k_inv_scale[h]);
      } else {
        store_kv8(k_cache + dst_off + c * 8, src_k[c]);
      }
      if (v_inv_scale != nullptr) {
        store_kv8(v_cache + dst_off + c * 8, src_v[c], v_inv_scale[h]);
      } else {
        store_kv8(v_cache + dst_off + c * 8, src_v[c]);
      }
    } else {
      store_kv8(k_cache + dst_off + c * 8, src_k[c]);
      store_kv8(v_cache + dst_off + c * 8, src_v[c]);
    }
  }
}

// Move whole KV blocks (all layers, K+V) between pools and staging buffers.
//   pool:    [L, 2, NB, KVH, BS, D], addressed through an id list [n_sel]
//   staging: [n_sel, L, 2, KVH, BS, D], contiguous in unit order
// One unit = one 16-byte short8 chunk of one (sel, layer, kv) block copy, so
// unit i of a staging buffer is element i. SRC_BY_ID / DST_BY_ID say which
// side is a pool:
//   <true, false>  gather  pool blocks src_ids -> staging (xGMI send)
//   <false, true>  scatter staging -> pool blocks dst_ids
//   <true, true>   peer pull: blocks src_ids of a PEER GPU's pool (mapped via
//                  hipIpcOpenMemHandle, so the loads travel over the direct
//                  xGMI link) into this GPU's pool blocks dst_ids. One-sided:
//                  no staging buffer, no send/recv rendezvous (SURVEY.md
//                  §5.8 names hipMemcpyPeerAsync; a gather kernel over the
//                  mapped peer pointer is the same xGMI path but handles
//                  the non-contiguous block list in one launch).
// The id list and block count of a staging side are not read.
template <bool SRC_BY_ID, bool DST_BY_ID>
__global__ void move_blocks_kernel(const short8* __restrict__ src,
                                   short8* __restrict__ dst,
                                   const int32_t* __restrict__ src_ids,
                                   const int32_t* __restrict__ dst_ids,
                                   int n_sel, int n_layers, int64_t src_nb,
                                   int64_t dst_nb,
                                   int64_t block_elems8 /* KVH*BS*D*size/16 */) {
  const int64_t per_sel = (int64_t)n_layers * 2 * block_elems8;
  const int64_t total = per_sel * n_sel;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t sel = i / per_sel;
    int64_t rem = i % per_sel;
    int64_t lkv = rem / block_elems8;       // layer*2 + kv
    int64_t off = rem % block_elems8;
    int64_t s = i, d = i;
    if constexpr (SRC_BY_ID)
      s = (lkv * src_nb + src_ids[sel]) * block_elems8 + off;
    if constexpr (DST_BY_ID)
      d = (lkv * dst_nb + dst_ids[sel]) * block_elems8 + off;
    dst[d] = src[s];
  }
}

template <bool SRC_BY_ID, bool DST_BY_ID>
hipError_t launch_move_blocks(const void* src, void* dst,
                              const int32_t* src_ids, const int32_t* dst_ids,
                              int n_sel, int n_layers, int64_t src_nb,
                              int64_t dst_nb, int64_t block_bytes,
                              hipStream_t stream) {
  if (n_sel == 0) return hipSuccess;
  // element-size agnostic: block_bytes is one (layer, K/V) block's bytes
  const int64_t block_elems8 = block_bytes / 16;
  const int64_t total = (int64_t)n_sel * n_layers * 2 * block_elems8;
  const int threads = 256;
  int blocks = (int)((total + threads - 1) / threads);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL((move_blocks_kernel<SRC_BY_ID, DST_BY_ID>), dim3(blocks),
                     dim3(threads), 0, stream, (const short8*)src,
                     (short8*)dst, src_ids, dst_ids, n_sel, n_layers, src_nb,
                     dst_nb, block_elems8);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // namespace

hipError_t lds_reshape_and_cache(const void* k_new, const void* v_new,
                                 void* k_cache, void* v_cache,
                                 const int64_t* slots, int n_tokens, int kvh,
                                 int bs, int d, int kv_fp8,
                                 const float* k_inv_scale,
                                 const float* v_inv_scale,
                                 hipStream_t stream) {
  if (n_tokens == 0) return hipSuccess;
  int threads = kvh * (d / 8);
  if (threads > 256) threads = 256;
  if (kv_fp8) {
    hipLaunchKernelGGL(reshape_and_cache_kernel<unsigned char>,
                       dim3(n_tokens), dim3(threads), 0, stream,
                       (const short*)k_new, (const short*)v_new,
                       (unsigned char*)k_cache, (unsigned char*)v_cache,
                       slots, k_inv_scale, v_inv_scale, n_tokens, kvh, bs, d);
  } else {
    if (k_inv_scale || v_inv_scale) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reshape_and_cache_kernel<short>, dim3(n_tokens),
                       dim3(threads), 0, stream, (const short*)k_new,
                       (const short*)v_new, (short*)k_cache, (short*)v_cache,
                       slots, nullptr, nullptr, n_tokens, kvh, bs, d);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t lds_gather_blocks(const void* pool, void* staging,
                             const int32_t* block_ids, int n_sel, int n_layers,
                             int64_t n_blocks, int64_t block_bytes,
                             int is_scatter, hipStream_t stream) {
  if (is_scatter)
    return launch_move_blocks<false, true>(staging, (void*)pool, nullptr,
                                           block_ids, n_sel, n_layers, 0,
                                           n_blocks, block_bytes, stream);
  return launch_move_blocks<true, false>(pool, staging, block_ids, nullptr,
                                         n_sel, n_layers, n_blocks, 0,
                                         block_bytes, stream);
}

hipError_t lds_copy_blocks_peer(const void* src_pool, void* dst_pool,
                                const int32_t* src_ids, const int32_t* dst_ids,
                                int n_sel, int n_layers, int64_t src_nb,
                                int64_t dst_nb, int64_t block_bytes,
                                hipStream_t stream) {
  return launch_move_blocks<true, true>(src_pool, dst_pool, src_ids, dst_ids,
                                        n_sel, n_layers, src_nb, dst_nb,
                                        block_bytes, stream);
}
