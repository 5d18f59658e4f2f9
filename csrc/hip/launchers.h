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

// ---- linear_fp8.hip ------------------------------------------------------

// k a wave consumes per step: 16 weight bytes a lane, two MFMA K-steps.
constexpr int LINEAR_FP8_KBLOCK = 64;
// Output columns of one workgroup by rows (16, 32 and 64 are instantiated):
// x comes from L2 once per column block, 2 * T / BN times the weight bytes,
// so taller batches take the wider block. BN changes which workgroup sums
// an element, never the order of its sum.
constexpr int LINEAR_FP8_BN = 32;
inline int linear_fp8_bn(int T) { return T <= 16 ? LINEAR_FP8_BN : 64; }
// K is split across workgroups until a launch holds this many of them ...
constexpr int LINEAR_FP8_SPLIT_WGS = 512;
// ... while a split keeps at least this many k, 8 splits at the most.
constexpr int LINEAR_FP8_SPLIT_MIN_K = 1024;

// Workgroups along K of the fp8 linear kernel: a function of (in, out)
// alone, so a row's bits do not depend on what else is launched.
inline int linear_fp8_k_splits(int in, int out) {
  const int wgs = (out + LINEAR_FP8_BN - 1) / LINEAR_FP8_BN;
  int s = 1;
  while (s < 8 && wgs * s < LINEAR_FP8_SPLIT_WGS &&
         in / (2 * s) >= LINEAR_FP8_SPLIT_MIN_K)
    s *= 2;
  return s;
}

// y[m, n] = bf16(scale[n] * sum_k x[m, k] * float(wq[n, k])), fp32 sums.
struct LinearFp8Args {
  const void* x;        // [T, in] bf16, in % 64 == 0, 16-byte aligned
  const void* wq;       // [out, in] OCP e4m3, out % 16 == 0, 16-byte aligned
  const float* scale;   // [out]
  void* y;              // [T, out] bf16
  float* part;          // [n_split, T, out] fp32 scratch; unread if n_split 1
  int T, in, out;
  int n_split;          // linear_fp8_k_splits(in, out); 1 <= n_split
  int bn;               // linear_fp8_bn(T); 16, 32 or 64
};

hipError_t lds_linear_fp8(const LinearFp8Args& a, hipStream_t stream);
// W [in, out] bf16 = bf16(float(wq[n, k]) * scale[n]); in % 64 == 0,
// out % 16 == 0, wq and W 16-byte aligned
hipError_t lds_dequant_fp8_weight(const void* wq, const float* scale, void* W,
                                  int in, int out, hipStream_t stream);

// ---- linear_fp8_a8.hip ---------------------------------------------------

// bytes of K a workgroup stages per step: one 16x16x128 fp8 MFMA deep
constexpr int LINEAR_FP8_A8_BK = 128;
// The 128 x 128 tile reads half the LDS bytes per MFMA of the 64 x 64 one,
// but only pays once its grid gives every CU a workgroup (256 CUs); below
// that the small tile spreads the same work over four times the CUs.
constexpr int LINEAR_FP8_A8_FILL_WGS = 256;

// Output tile edge of the fp8-activation GEMM (64 and 128 are
// instantiated). The tile decides who computes an element, never the order
// of its sum.
inline int linear_fp8_a8_tile(int T, int out) {
  const int64_t wgs = (int64_t)((T + 127) / 128) * ((out + 127) / 128);
  return wgs >= LINEAR_FP8_A8_FILL_WGS ? 128 : 64;
}

// xq[m, k] = e4m3(clamp(x[m, k] / sx[m], +-448)), sx[m] = absmax(x[m, :]) /
// 448 (1 for a zero row): x [T, in] bf16, in % 64 == 0, x and xq 16-byte
// aligned.
hipError_t lds_quantize_rows_fp8(const void* x, void* xq, float* sx, int T,
                                 int in, hipStream_t stream);

// y[m, n] = bf16(sx[m] * scale[n] * sum_k float(xq[m, k]) * float(wq[n, k])),
// fp32 sums on the fp8 MFMA.
struct LinearFp8A8Args {
  const void* xq;       // [T, in] OCP e4m3, in % 64 == 0, 16-byte aligned
  const float* sx;      // [T]
  const void* wq;       // [out, in] OCP e4m3, out % 16 == 0, 16-byte aligned
  const float* scale;   // [out]
  void* y;              // [T, out] bf16, 16-byte aligned
  int T, in, out;
  int tile;             // linear_fp8_a8_tile(T, out); 64 or 128
};

hipError_t lds_linear_fp8_a8(const LinearFp8A8Args& a, hipStream_t stream);

// ---- linear_fp8_block.hip ------------------------------------------------

// k of one activation group and edge of one weight block: one 16x16x128 fp8
// MFMA deep, and one slab of the tiled kernel (LINEAR_FP8_A8_BK).
constexpr int LINEAR_FP8_BLOCK_GROUP = 128;
inline int linear_fp8_block_groups(int in) {
  return (in + LINEAR_FP8_BLOCK_GROUP - 1) / LINEAR_FP8_BLOCK_GROUP;
}
// The activation scales live on the device as [G, Tp], group-major with the
// row count rounded up to 4: a lane's four D rows of a group are one aligned
// 16-byte load, and a tile's rows of a slab are contiguous. Entries of the
// rows T .. Tp - 1 are never written and never reach a stored element.
__host__ __device__ inline int linear_fp8_block_tp(int T) {
  return (T + 3) & ~3;
}

// The skinny kernel splits K across workgroups by the rule of
// linear_fp8_k_splits, with the same constants (set by reasoning there, not
// re-measured here): until a launch at BN = 32 holds LINEAR_FP8_SPLIT_WGS
// workgroups, while a split keeps LINEAR_FP8_SPLIT_MIN_K k (8 groups, two a
// wave), 8 splits at the most. A function of (in, out) alone, so a row's
// bits do not depend on what else is launched.
inline int linear_fp8_block_k_splits(int in, int out) {
  return linear_fp8_k_splits(in, out);
}

constexpr int LINEAR_FP8_BLOCK_SKINNY = 1;
// Up to this many rows the skinny kernel always serves: the tiled kernel
// issues the four row blocks of a 64-row tile whatever T is and moves both
// operands through LDS. Measured at T = 1, 16 and 32 on the Llama-3-8B and
// Qwen3-32B projections (profiles/linear_fp8_block.md): the skinny kernel
// leads the 64 tile 1.17x to 5.5x on every one, 1.17x to 5.1x at 32.
constexpr int LINEAR_FP8_BLOCK_SKINNY_ALWAYS_T = 32;
// Above that, up to this many rows, the skinny kernel serves while the 64 x
// 64 grid of the tiled kernel would leave CUs idle (fewer than
// LINEAR_FP8_A8_FILL_WGS = 256 tiles): the tiled kernel has no K split, the
// skinny one re-reads the weights once per 64 rows but keeps every CU
// busy. Measured on the same projections: at T = 64 the 64 tile leads only
// where out >= 28672 (448 tiles and more: 45.2 against 50.2 us, 104.6
// against 109.2); at T = 128 the skinny kernel leads at out = 4096 .. 6144
// (128 to 192 tiles: 27.0 against 39.5 us, 33.8 against 39.8, 48.7 against
// 122.6) and trails from out = 10240 on (320 tiles: 52.0 against 49.1); at
// T = 256 and out = 4096 (256 tiles) it trails on wo (42.4 against 40.2).
// The rule cannot see `in`: on the deep wdown shapes the skinny kernel still
// leads at T = 256 (86.9 against 123.2 us), which this rule gives away. 256
// is the largest T at which the skinny kernel was timed; T from 33 to 63 was
// not timed and goes by the fill count as 64 does.
constexpr int LINEAR_FP8_BLOCK_SKINNY_MAX_T = 256;

// Kernel of the block-scaled linear by (T, out) alone: the skinny kernel
// (LINEAR_FP8_BLOCK_SKINNY) or the 64 tile. The 128 tile is kept as a
// measurement arm, reachable through the binding's `kernel` argument and
// tested there, but never picked: with the scaled adds in its slab loop it
// trails the 64 tile at every measured shape, the largest grids included
// (Qwen3-32B wgate_up at T = 4096, 12800 large tiles: 3763 against 3070
// us), so the fill reasoning of linear_fp8_a8_tile does not carry over. It
// is the arm a cheaper promotion is to be judged against. The skinny and
// the tiled kernel sum the groups of K in different orders: a row's bits
// may differ between launches that this rule sends to different kernels,
// never within either kernel.
inline int linear_fp8_block_kernel_for(int T, int out) {
  if (T <= LINEAR_FP8_BLOCK_SKINNY_ALWAYS_T) return LINEAR_FP8_BLOCK_SKINNY;
  const int64_t tiles = (int64_t)((T + 63) / 64) * ((out + 63) / 64);
  if (T <= LINEAR_FP8_BLOCK_SKINNY_MAX_T && tiles < LINEAR_FP8_A8_FILL_WGS)
    return LINEAR_FP8_BLOCK_SKINNY;
  return 64;
}

// xq[m, k] = e4m3(clamp(x[m, k] / sx[m, k / 128], +-448)), sx[m, g] =
// absmax(x[m, 128 g .. 128 g + 127]) / 448 (1 for a zero group), written to
// sx[g * Tp + m], Tp = linear_fp8_block_tp(T): x [T, in] bf16, in % 64 == 0
// (the last group may be 64 wide), x and xq 16-byte aligned.
hipError_t lds_quantize_groups_fp8(const void* x, void* xq, float* sx, int T,
                                   int in, hipStream_t stream);

// y[m, n] = bf16(sum_g sx[m, g] * scale[n / 128, g] * sum_{k in g}
// float(xq[m, k]) * float(wq[n, k])), fp32 sums on the fp8 MFMA.
struct LinearFp8BlockArgs {
  const void* xq;       // [T, in] OCP e4m3, in % 64 == 0, 16-byte aligned
  const float* sx;      // [G, Tp] as lds_quantize_groups_fp8 writes it,
                        // 16-byte aligned
  const void* wq;       // [out, in] OCP e4m3, out % 16 == 0, 16-byte aligned
  const float* scale;   // [ceil(out / 128), G]
  void* y;              // [T, out] bf16, 16-byte aligned
  float* part;          // [n_split, T, out] fp32 scratch of the skinny
                        // kernel; unread if n_split is 1
  int T, in, out;
  int n_split;          // linear_fp8_block_k_splits(in, out)
  int kernel;           // linear_fp8_block_kernel_for(T, out), or forced:
                        // 1, 64 or 128
};

hipError_t lds_linear_fp8_block(const LinearFp8BlockArgs& a,
                                hipStream_t stream);

// ---- linear_mxfp4.hip ----------------------------------------------------

// k a wave consumes per step: one 32-wide MX group a lane group, four MFMAs.
constexpr int LINEAR_MXFP4_KBLOCK = 128;
// Output columns of one workgroup by rows (16, 32 and 64 are instantiated),
// as for fp8: BN changes which workgroup sums an element, never the order.
constexpr int LINEAR_MXFP4_BN = 32;
inline int linear_mxfp4_bn(int T) { return T <= 16 ? LINEAR_MXFP4_BN : 64; }
// K is split across workgroups until a launch holds this many of them ...
constexpr int LINEAR_MXFP4_SPLIT_WGS = 512;
// ... while a split keeps at least this many k (16 K blocks, four a wave),
// 8 splits at the most.
constexpr int LINEAR_MXFP4_SPLIT_MIN_K = 2048;

// Workgroups along K of the mxfp4 linear kernel: a function of (in, out)
// alone, so a row's bits do not depend on what else is launched.
inline int linear_mxfp4_k_splits(int in, int out) {
  const int wgs = (out + LINEAR_MXFP4_BN - 1) / LINEAR_MXFP4_BN;
  int s = 1;
  while (s < 8 && wgs * s < LINEAR_MXFP4_SPLIT_WGS &&
         in / (2 * s) >= LINEAR_MXFP4_SPLIT_MIN_K)
    s *= 2;
  return s;
}

// y[m, n] = bf16(sum_k x[m, k] * e2m1(wq[n, k]) * 2^(scale[n, k/32] - 127)),
// fp32 sums.
struct LinearMxfp4Args {
  const void* x;        // [T, in] bf16, in % 128 == 0, 16-byte aligned
  const void* wq;       // [out, in / 2] uint8, out % 16 == 0, 16-byte aligned
  const void* scale;    // [out, in / 32] uint8 (e8m0)
  void* y;              // [T, out] bf16
  float* part;          // [n_split, T, out] fp32 scratch; unread if n_split 1
  int T, in, out;
  int n_split;          // linear_mxfp4_k_splits(in, out); 1 <= n_split
  int bn;               // linear_mxfp4_bn(T); 16, 32 or 64
};

hipError_t lds_linear_mxfp4(const LinearMxfp4Args& a, hipStream_t stream);
// W [in, out] bf16 = e2m1(wq[n, k]) * 2^(scale[n, k/32] - 127), exact;
// in % 128 == 0, out % 16 == 0, wq and W 16-byte aligned
hipError_t lds_dequant_mxfp4_weight(const void* wq, const void* scale,
                                    void* W, int in, int out,
                                    hipStream_t stream);

// ---- moe.hip -------------------------------------------------------------

constexpr int MOE_MAX_EXPERTS = 256;
constexpr int MOE_MAX_TOPK = 8;
// Tokens of one routing workgroup (one MFMA row block).
constexpr int MOE_ROUTE_TOKENS = 16;

// ids[t, :] = the k experts with the largest router logits (value descending,
// ties to the lower index); w[t, :] = their softmax over all E, divided by
// their sum with renorm.
struct MoeRouteArgs {
  const void* x;        // [T, H] bf16, H % 32 == 0, 16-byte aligned
  const void* router;   // [E, H] bf16, 16-byte aligned
  int32_t* ids;         // [T, k]
  float* w;             // [T, k]
  int T, H;
  int E;                // 1 .. MOE_MAX_EXPERTS
  int k;                // 1 .. min(MOE_MAX_TOPK, E)
  int renorm;
};

hipError_t lds_moe_route(const MoeRouteArgs& a, hipStream_t stream);

// Row blocks of a work-list tile, from the mean rows per expert alone:
// tiles are TM = 16 * MB rows tall. MB changes which workgroup computes a
// pair, never the order of its sums.
inline int moe_mb(int64_t P, int E) {
  const int64_t per = P / E;
  return per <= 16 ? 1 : per <= 32 ? 2 : 4;
}
// Tiles a work list can hold: an expert with c pairs takes ceil(c / TM).
inline int64_t moe_tile_bound(int64_t P, int E, int mb) {
  return P / (16 * mb) + (P < E ? P : E);
}

// y[t] = bf16(sum_j w[t, j] * (bf16(silu(x[t] Wg_e) * (x[t] Wu_e)) W2_e)),
// e = ids[t, j], fp32 sums, j in slot order. P = T * k (token, slot) pairs.
// An id outside [0, E) is read as the nearest expert: nothing is checked on
// the device, and nothing goes out of bounds.
struct MoeFfnArgs {
  const void* x;        // [T, H] bf16, H % 32 == 0, 16-byte aligned
  const void* w13;      // [E, 2 I, H] bf16: gate rows, then up rows
  const void* w2;       // [E, H, I] bf16, I % 16 == 0
  const int32_t* ids;   // [T, k]
  const float* w;       // [T, k]
  void* y;              // [T, H] bf16
  // scratch, every pointer 16-byte aligned
  void* act;            // [moe_tile_bound * TM, I] bf16, by sorted position
  float* y2;            // [P, H] fp32, by pair
  int32_t* tiles;       // [moe_tile_bound, 3] start, count <= TM, expert
  int32_t* n_tiles;     // [1]
  int32_t* perm;        // [moe_tile_bound * TM] sorted position -> pair
  int T, H, I, E, k;
  int mb;               // moe_mb(T * k, E)
};

hipError_t lds_moe_ffn(const MoeFfnArgs& a, hipStream_t stream);

// Row blocks of a work-list tile on MXFP4 experts: a ring stage of the 4-bit
// kernels holds 16 registers a row block, and MB = 4 leaves no room for a
// ring, so taller segments walk more tiles of 32 rows.
constexpr int MOE_MXFP4_MAX_MB = 2;
inline int moe_mxfp4_mb(int64_t P, int E) {
  const int mb = moe_mb(P, E);
  return mb < MOE_MXFP4_MAX_MB ? mb : MOE_MXFP4_MAX_MB;
}

// moe_ffn on MXFP4 experts: y is what MoeFfnArgs computes on the exactly
// dequantised experts e2m1(code) * 2^(scale - 127), every one of which is a
// bf16. Codes: two a byte, k = 2j in the low nibble; one e8m0 scale per 32 k.
struct MoeFfnMxfp4Args {
  const void* x;        // [T, H] bf16, H % 32 == 0, 16-byte aligned
  const void* w13q;     // [E, 2 I, H / 2] uint8, 16-byte aligned
  const void* w13s;     // [E, 2 I, H / 32] uint8
  const void* w2q;      // [E, H, I / 2] uint8, I % 32 == 0, 16-byte aligned
  const void* w2s;      // [E, H, I / 32] uint8
  const int32_t* ids;   // [T, k]
  const float* w;       // [T, k]
  void* y;              // [T, H] bf16
  // scratch as in MoeFfnArgs, with mb below
  void* act;
  float* y2;
  int32_t* tiles;
  int32_t* n_tiles;
  int32_t* perm;
  int T, H, I, E, k;
  int mb;               // moe_mxfp4_mb(T * k, E)
};

hipError_t lds_moe_ffn_mxfp4(const MoeFfnMxfp4Args& a, hipStream_t stream);

// moe_ffn on fp8 experts: e4m3 (OCP) weights with one fp32 scale per expert
// and output channel. The scales are applied to the fp32 sums, never to the
// weights: act = bf16(silu(w13s[e, n] * sum_g) * (w13s[e, I + n] * sum_u)),
// y2 = (w2s[e, n] * sum) * w[pair]. The tiles are those of MoeFfnArgs.
struct MoeFfnFp8Args {
  const void* x;        // [T, H] bf16, H % 32 == 0, 16-byte aligned
  const void* w13q;     // [E, 2 I, H] e4m3, 16-byte aligned, I % 16 == 0
  const float* w13s;    // [E, 2 I], 16-byte aligned
  const void* w2q;      // [E, H, I] e4m3, 16-byte aligned
  const float* w2s;     // [E, H], 16-byte aligned
  const int32_t* ids;   // [T, k]
  const float* w;       // [T, k]
  void* y;              // [T, H] bf16
  // scratch as in MoeFfnArgs
  void* act;
  float* y2;
  int32_t* tiles;
  int32_t* n_tiles;
  int32_t* perm;
  int T, H, I, E, k;
  int mb;               // moe_mb(T * k, E)
};

hipError_t lds_moe_ffn_fp8(const MoeFfnFp8Args& a, hipStream_t stream);

// The work list and the slot sum on their own, for moe_fp8_a8.hip: tiles
// [n, 3] = (start, count <= TM, expert), n_tiles and perm (sorted position ->
// pair) of the P pairs of ids, with every expert's segment padded to TM rows;
// y[t] = bf16(sum_j y2[t k + j]) in slot order. T >= 1.
hipError_t lds_moe_align(const int32_t* ids, int32_t* tiles, int32_t* n_tiles,
                         int32_t* perm, int64_t P, int E, int TM,
                         hipStream_t stream);
hipError_t lds_moe_combine(const float* y2, void* y, int T, int H, int k,
                           hipStream_t stream);

// ---- moe_fp8_a8.hip ------------------------------------------------------

// Tile height of the fp8-activation expert GEMMs (64 and 128 are
// instantiated), from the mean rows per expert alone. Every expert's segment
// is padded to whole tiles, half a tile of dead MFMA rows an expert on
// average: at a mean of 64 rows or fewer a 128-row tile would be half padding
// or worse, above it the taller tile reads each weight byte for twice the
// rows. The threshold is that reasoning about padding, not a sweep. The tile
// decides who computes an element, never its bits.
inline int moe_fp8_a8_tile(int64_t P, int E) { return P / E > 64 ? 128 : 64; }

// moe_ffn on fp8 experts with fp8 activations on the fp8 MFMA (W8A8):
//   (xq, sx) = quantize_rows_fp8(x)
//   act[p, n] = bf16(silu(g) * u), g = (sum_k xq[t, k] w13q[e, n, k]) * sx[t]
//               * w13s[e, n], u the same on row I + n; p = t k + j, e = ids[p]
//   (aq, sa) = quantize_rows_fp8(act), per pair row
//   y2[p, n] = (sum_k aq[p, k] w2q[e, n, k]) * sa[p] * w2s[e, n] * w[p]
//   y[t] = bf16(sum_j y2[t k + j])
struct MoeFfnFp8A8Args {
  const void* x;        // [T, H] bf16, H % 64 == 0, 16-byte aligned
  const void* w13q;     // [E, 2 I, H] e4m3, 16-byte aligned, I % 64 == 0
  const float* w13s;    // [E, 2 I]
  const void* w2q;      // [E, H, I] e4m3, 16-byte aligned
  const float* w2s;     // [E, H]
  const int32_t* ids;   // [T, k]
  const float* w;       // [T, k]
  void* y;              // [T, H] bf16
  // scratch, every pointer 16-byte aligned; P = T k
  void* xq;             // [T, H] e4m3
  float* sx;            // [T]
  void* act;            // [P, I] bf16, by pair: the scratch's, or act_out
  void* aq;             // [P, I] e4m3, by pair
  float* sa;            // [P]
  float* y2;            // [P, H] fp32, by pair
  int32_t* tiles;       // [moe_tile_bound, 3]
  int32_t* n_tiles;     // [1]
  int32_t* perm;        // [moe_tile_bound * tile]
  int T, H, I, E, k;
  int tile;             // moe_fp8_a8_tile(T * k, E); 64 or 128
};

hipError_t lds_moe_ffn_fp8_a8(const MoeFfnFp8A8Args& a, hipStream_t stream);

// ---- moe_fp8_block.hip ---------------------------------------------------

// From this many mean rows per expert (P / E) on, the 64-row LDS tiles serve
// block-scaled experts, below it the 16-row registers-only kernels. The rule
// started at 16, where an expert's segment still fits one short tile (the
// reasoning of moe_mb), and was then set to the smallest measured mean at
// which the 64-row tile is ahead, on a Qwen3-30B-A3B layer (E = 128, k = 8,
// profiles/moe_fp8_block.md): at T = 1, 0.0625 rows an expert, the 16-row
// kernels lead (69.2 against 84.3 us); at T = 16, 1 row an expert, the
// 64-row tiles already do (193.7 against 201.6 us), and at every larger T.
// Nothing between those two rows was timed.
constexpr int MOE_FP8_BLOCK_TILED_MIN_ROWS = 1;

// Tile height of the block-scaled expert GEMMs, 16 (the skinny kernels) or
// 64, from (P, E) alone: no sync. The two families sum the groups of K in
// different orders, so a pair's bits may differ between launches this rule
// sends to different families, never within either.
inline int moe_fp8_block_tile(int64_t P, int E) {
  return P < (int64_t)E * MOE_FP8_BLOCK_TILED_MIN_ROWS ? 16 : 64;
}

// moe_ffn on block-scaled fp8 experts with group-scaled fp8 activations
// (G_K = ceil(K / 128), NBI = ceil(I / 128), NBH = ceil(H / 128)):
//   (xq, sx) = quantize_groups_fp8(x)
//   act[p, n] = bf16(silu(g) * u), g = sum_g sx[t, g] * w13s[e, n / 128, g] *
//               sum_{k in g} xq[t, k] w13q[e, n, k], u the same on row I + n
//               with w13s[e, NBI + n / 128, g]; p = t k + j, e = ids[p]
//   (aq, sa) = quantize_groups_fp8(act), per pair row
//   y2[p, n] = (sum_g sa[p, g] * w2s[e, n / 128, g] * sum_{k in g} aq[p, k]
//              w2q[e, n, k]) * w[p]
//   y[t] = bf16(sum_j y2[t k + j])
struct MoeFfnFp8BlockArgs {
  const void* x;        // [T, H] bf16, H % 64 == 0, 16-byte aligned
  const void* w13q;     // [E, 2 I, H] e4m3, 16-byte aligned, I % 64 == 0
  const float* w13s;    // [E, 2 NBI, G_H]: gate blocks, then up blocks
  const void* w2q;      // [E, H, I] e4m3, 16-byte aligned
  const float* w2s;     // [E, NBH, G_I]
  const int32_t* ids;   // [T, k]
  const float* w;       // [T, k]
  void* y;              // [T, H] bf16
  // scratch, every pointer 16-byte aligned; P = T k
  void* xq;             // [T, H] e4m3
  float* sx;            // [G_H, linear_fp8_block_tp(T)]
  void* act;            // [P, I] bf16, by pair: the scratch's, or act_out
  void* aq;             // [P, I] e4m3, by pair
  float* sa;            // [G_I, linear_fp8_block_tp(P)]
  float* y2;            // [P, H] fp32, by pair
  int32_t* tiles;       // [moe_tile_bound, 3]
  int32_t* n_tiles;     // [1]
  int32_t* perm;        // [moe_tile_bound * tile]
  int T, H, I, E, k;
  int tile;             // moe_fp8_block_tile(T * k, E); 16 or 64
};

hipError_t lds_moe_ffn_fp8_block(const MoeFfnFp8BlockArgs& a,
                                 hipStream_t stream);

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
