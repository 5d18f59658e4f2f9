// flash_prefill.h — host interface of the two flash-prefill kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// Block-table entries the glds kernel stages into LDS (16K-token context
// at block size 16). Wider tables take the plain kernel.
constexpr int FLASH_GLDS_BT_CAP = 1024;

extern "C" {

// convert-on-stage kernel: bf16 or fp8 KV, any table width; k_scale /
// v_scale are the [KVH] per-head dequant scales of an fp8 cache, or null
hipError_t lds_flash_prefill(const void* q, const void* k_cache,
                             const void* v_cache,
                             const int32_t* block_tables,
                             const int32_t* seq_meta, const int32_t* tiles,
                             void* out, int n_tiles, int n_q_heads, int kvh,
                             int bs, int head_dim, int max_blocks, int kv_fp8,
                             float scale, const float* k_scale,
                             const float* v_scale, hipStream_t stream);

// glds ring kernel: bf16 KV, max_blocks <= FLASH_GLDS_BT_CAP
hipError_t lds_flash_prefill_glds(
    const void* q, const void* k_cache, const void* v_cache,
    const int32_t* block_tables, const int32_t* seq_meta,
    const int32_t* tiles, void* out, int n_tiles, int n_q_heads, int kvh,
    int bs, int head_dim, int max_blocks, float scale, hipStream_t stream);

}  // extern "C"
