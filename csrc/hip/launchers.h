// launchers.h — host interface of every kernel launcher (`lds_*`).
//
// Each launcher is declared here once. The .hip file that defines it and
// the torch binding (ops.hip) both include this header, so the compiler
// checks every call against the definition, and a mismatch that slips past
// it fails at link time (C++ linkage). Launchers return a hipError_t and
// never throw; an empty launch (zero rows, tiles or blocks) is a no-op.
//
// The launchers trust their arguments: ops.hip checks every size, dtype and
// device before it fills a struct or calls one (DEVELOPMENT.md "Op argument
// contract").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// ---- prefix_kernels.hip --------------------------------------------------

hipError_t lds_hash_prompts(const int32_t* tokens, const int64_t* offsets,
                            int n_requests, int block_tokens, int max_blocks,
                            uint64_t seed0, uint64_t* out, int32_t* counts,
                            hipStream_t stream);
hipError_t lds_table_update(uint64_t* keys, unsigned long long* masks,
                            uint32_t cap_mask, const uint64_t* hashes,
                            int64_t n, int endpoint, int is_remove,
                            unsigned int* dropped, hipStream_t stream);
hipError_t lds_match_longest(const uint64_t* keys,
                             const unsigned long long* masks,
                             uint32_t cap_mask, const uint64_t* hashes,
                             const int32_t* counts, int n_requests,
                             int max_blocks, int n_endpoints, int32_t* out,
                             hipStream_t stream);

// ---- norm_rope_act.hip ---------------------------------------------------

// residual: null, or [n_rows, H] updated in place
hipError_t lds_rmsnorm(const void* x, void* residual, const void* w, void* y,
                       int64_t n_rows, int H, float eps, hipStream_t stream);
hipError_t lds_rope(void* q, void* k, const float* cos_sin,
                    const int32_t* positions, int n_tokens, int n_q_heads,
                    int n_kv_heads, int head_dim, hipStream_t stream);
hipError_t lds_silu_mul(const void* gate_up, void* y, int64_t T, int I,
                        hipStream_t stream);

// ---- qkv_epilogue.hip ----------------------------------------------------

// qkv: [n_tokens, (n_q_heads + 2*kvh) * d] bf16 -> q_out [n_tokens,
// n_q_heads, d] rotated; rotated K and plain V stored at slots[t] (< 0: not
// stored). d % 16 == 0; every pointer 16-byte aligned.
hipError_t lds_qkv_rope_cache(const void* qkv, const float* cos_sin,
                              const int32_t* positions, const int64_t* slots,
                              void* q_out, void* k_cache, void* v_cache,
                              int64_t n_tokens, int n_q_heads, int kvh, int bs,
                              int d, int kv_fp8, const float* k_inv_scale,
                              const float* v_inv_scale, hipStream_t stream);

// ---- kv_cache.hip --------------------------------------------------------

hipError_t lds_reshape_and_cache(const void* k_new, const void* v_new,
                                 void* k_cache, void* v_cache,
                                 const int64_t* slots, int n_tokens, int kvh,
                                 int bs, int d, int kv_fp8,
                                 const float* k_inv_scale,
                                 const float* v_inv_scale,
                                 hipStream_t stream);
// block_bytes: one (layer, K/V) block in bytes, a multiple of 16
hipError_t lds_gather_blocks(const void* pool, void* staging,
                             const int32_t* block_ids, int n_sel, int n_layers,
                             int64_t n_blocks, int64_t block_bytes,
                             int is_scatter, hipStream_t stream);
hipError_t lds_copy_blocks_peer(const void* src_pool, void* dst_pool,
                                const int32_t* src_ids, const int32_t* dst_ids,
                                int n_sel, int n_layers, int64_t src_nb,
                                int64_t dst_nb, int64_t block_bytes,
                                hipStream_t stream);

// ---- attention: paged_attention.hip, flash_prefill{,_glds}.hip -----------

// Block-table entries the glds prefill kernel stages into LDS (16K-token
// context at block size 16). Wider tables take the plain kernel.
constexpr int FLASH_GLDS_BT_CAP = 1024;

// One argument struct for the four attention launchers; each reads the
// common part and its own group and ignores the rest.
struct AttnArgs {
  const void* q;                // [N, QH, D] bf16
  const void* k_cache;          // [NB, KVH, BS, D] bf16 | fp8 (kv_fp8)
  const void* v_cache;
  const int32_t* block_tables;  // [B, max_blocks]
  void* out;                    // [N, QH, D] bf16
  const float* k_scale;         // [KVH] dequant scales of an fp8 cache,
  const float* v_scale;         // or null
  int n_q_heads, kvh, bs, head_dim, max_blocks;
  int kv_fp8;
  float scale;
  // decode (lds_paged_attention, lds_paged_attention_split)
  const int32_t* seq_lens;      // [B], B = N = n_seqs
  int n_seqs;
  int chunk;                    // online-softmax chunk: 256 or 512
  // split only
  float* part_o;                // [B, KVH, n_parts, QPG, D]
  float* part_ml;               // [B, KVH, n_parts, QPG, 2]
  int n_parts;                  // 1..64
  int part_tokens;
  // prefill (lds_flash_prefill, lds_flash_prefill_glds)
  const int32_t* seq_meta;      // [B, 3] start, chunk, prior
  const int32_t* tiles;         // [n_tiles, 2] seq, vrow0
  int n_tiles;
};

hipError_t lds_paged_attention(const AttnArgs& a, hipStream_t stream);
hipError_t lds_paged_attention_split(const AttnArgs& a, hipStream_t stream);
// convert-on-stage kernel: bf16 or fp8 KV, any table width
hipError_t lds_flash_prefill(const AttnArgs& a, hipStream_t stream);
// glds ring kernel: bf16 KV, max_blocks <= FLASH_GLDS_BT_CAP
hipError_t lds_flash_prefill_glds(const AttnArgs& a, hipStream_t stream);

// ---- lora.hip ------------------------------------------------------------

// Columns of `in` one shrink workgroup sums: the K split count is a function
// of `in` alone, so a row's bits do not depend on what else is launched.
constexpr int LORA_KCHUNK = 1024;
// Columns of `out` one expand workgroup owns.
constexpr int LORA_NBLOCK = 256;

inline int lora_k_splits(int in) { return (in + LORA_KCHUNK - 1) / LORA_KCHUNK; }

// y[perm rows] += (x[perm rows] · A[slot]ᵀ) · B[slot]ᵀ, one slot per tile.
// The caller guarantees, and nothing clamps: perm entries distinct and in
// [0, T); per tile 1 <= count <= 16, start + count <= len(perm), slot in
// [0, S).
struct LoraArgs {
  const void* x;          // [T, in] bf16, in % 32 == 0
  void* y;                // [T, out] bf16, out % 16 == 0, updated in place
  const void* A;          // [S, R, in] bf16
  const void* B;          // [S, out, R] bf16, alpha / rank folded in
  const int32_t* perm;    // adapter rows, grouped by slot
  const int32_t* tiles;   // [n_tiles, 3] start in perm, count, slot
  float* part;            // [lora_k_splits(in), n_tiles * 16, R] fp32 scratch
  int n_tiles;
  int in, out;
  int R;                  // 16, 32, 48 or 64
};

// part = x[perm rows] · A[slot]ᵀ, one fp32 partial per K split
hipError_t lds_lora_shrink(const LoraArgs& a, hipStream_t stream);
// y[perm rows] += bf16(sum of partials) · B[slot]ᵀ
hipError_t lds_lora_expand(const LoraArgs& a, hipStream_t stream);

// ---- sampler.hip ---------------------------------------------------------

// What every sampler launch carries: one workgroup per row, no host sync.
struct SampleArgs {
  const void* logits;           // [B, V] bf16, or fp32 with is_f32
  const float* temperature;     // per-row parameters, [B] each
  const int32_t* top_k;
  const float* top_p;
  const int64_t* seed;
  const int32_t* pos;
  int B, V, is_f32;
  int64_t* tokens;              // outputs, [B] each
  float* logprobs;
  int32_t* n_kept;
  float* threshold;
};

// What sample_ext adds to the launch (DEVELOPMENT.md "Sampling").
struct ExtArgs {
  const float* rep;
  const float* pres;
  const float* freq;
  const float* min_p;
  const int32_t* top_n;
  const int32_t* state_row;
  int16_t* state;            // [R, Vs] int16, or null: no row has state
  int64_t Vs;                // Vs % 8 == 0, Vs >= V, base 16-byte aligned
  int R;
  int n_top;                 // width of the top-N outputs, 0..20
  int64_t* top_tokens;       // [B, n_top]
  float* top_logprobs;       // [B, n_top]
};

hipError_t lds_sample(const SampleArgs& a, hipStream_t stream);
hipError_t lds_sample_ext(const SampleArgs& a, const ExtArgs& ea,
                          hipStream_t stream);
// state: [R, Vs] int16; rows, n_prompt: [n]; offsets: [n + 1] into toks
hipError_t lds_token_state_fill(int16_t* state, int R, int64_t Vs, int V,
                                const int32_t* rows, int n,
                                const int32_t* toks, int64_t n_toks,
                                const int64_t* offsets,
                                const int32_t* n_prompt, hipStream_t stream);
