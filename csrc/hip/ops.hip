// ops.hip — torch extension binding for the gfx950 kernels (`_hip_ops`).
// Pure HIP (no hipify, no CUDA shims): includes the ROCm-native ATen HIP
// headers directly and drives hipStream_t launchers from the .hip kernels.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <hip/hip_runtime.h>

#include <climits>

#include "flash_prefill.h"

#define CHECK_HIP(expr)                                                    \
  do {                                                                     \
    hipError_t err__ = (expr);                                             \
    TORCH_CHECK(err__ == hipSuccess, "HIP error: ", hipGetErrorString(err__)); \
  } while (0)

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous on GPU")

extern "C" {
hipError_t lds_hash_prompts(const int32_t*, const int64_t*, int, int, int,
                            uint64_t, uint64_t*, int32_t*, hipStream_t);
hipError_t lds_table_update(uint64_t*, unsigned long long*, uint32_t,
                            const uint64_t*, int64_t, int, int, unsigned int*,
                            hipStream_t);
hipError_t lds_match_longest(const uint64_t*, const unsigned long long*,
                             uint32_t, const uint64_t*, const int32_t*, int,
                             int, int, int32_t*, hipStream_t);
hipError_t lds_rmsnorm(const void*, void*, const void*, void*, int64_t, int,
                       float, hipStream_t);
hipError_t lds_rope(void*, void*, const float*, const int32_t*, int, int, int,
                    int, hipStream_t);
hipError_t lds_silu_mul(const void*, void*, int64_t, int, hipStream_t);
hipError_t lds_reshape_and_cache(const void*, const void*, void*, void*,
                                 const int64_t*, int, int, int, int, int,
                                 const float*, const float*, hipStream_t);
hipError_t lds_gather_blocks(const void*, void*, const int32_t*, int, int,
                             int64_t, int64_t, int, hipStream_t);
hipError_t lds_paged_attention(const void*, const void*, const void*,
                               const int32_t*, const int32_t*, void*, int, int,
                               int, int, int, int, int, int, float,
                               const float*, const float*, hipStream_t);
hipError_t lds_paged_attention_split(const void*, const void*, const void*,
                                     const int32_t*, const int32_t*, void*,
                                     float*, float*, int, int, int, int, int,
                                     int, int, int, int, int, float,
                                     const float*, const float*, hipStream_t);
hipError_t lds_sample(const void*, const float*, const int32_t*, const float*,
                      const int64_t*, const int32_t*, int, int, int, int64_t*,
                      float*, int32_t*, float*, hipStream_t);
hipError_t lds_sample_ext(const void*, const float*, const int32_t*,
                          const float*, const int64_t*, const int32_t*,
                          const float*, const float*, const float*,
                          const float*, const int32_t*, const int32_t*,
                          int16_t*, int, int64_t, int, int, int, int, int64_t*,
                          float*, int32_t*, float*, int64_t*, float*,
                          hipStream_t);
hipError_t lds_token_state_fill(int16_t*, int, int64_t, int, const int32_t*,
                                int, const int32_t*, int64_t, const int64_t*,
                                const int32_t*, hipStream_t);
}

namespace {

int kv_fp8_flag(const torch::Tensor& cache) {
  if (cache.scalar_type() == at::kFloat8_e4m3fn) return 1;
  TORCH_CHECK(cache.scalar_type() == at::kBFloat16,
              "KV cache must be bf16 or fp8_e4m3fn");
  return 0;
}

// Optional per-KV-head scale vector of an fp8 cache ([KVH] fp32, one
// layer's slice): its device pointer, or null when absent.
const float* kv_scale_ptr(const c10::optional<torch::Tensor>& s,
                          const torch::Tensor& cache, const char* name) {
  if (!s.has_value()) return nullptr;
  TORCH_CHECK(cache.scalar_type() == at::kFloat8_e4m3fn, name,
              " is only legal with an fp8_e4m3fn KV cache");
  TORCH_CHECK(s->is_cuda() && s->device() == cache.device(), name,
              " must be on the KV cache's device");
  TORCH_CHECK(s->scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(s->is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(s->numel() == cache.size(1), name, " must hold ",
              cache.size(1), " values (one per KV head), got ", s->numel());
  return s->data_ptr<float>();
}

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// ---- prefix-cache kernels ----

// Every argument is checked here, on the host, before anything is launched:
// the kernels trust their sizes.

// keys/masks of the device table: uint64, equally long, 2^k slots.
void check_table(const torch::Tensor& keys, const torch::Tensor& masks) {
  CHECK_GPU(keys); CHECK_GPU(masks);
  TORCH_CHECK(keys.scalar_type() == at::kUInt64 &&
              masks.scalar_type() == at::kUInt64,
              "table keys and masks must be uint64");
  TORCH_CHECK(masks.device() == keys.device(),
              "table keys and masks must be on one device");
  TORCH_CHECK(keys.numel() == masks.numel(), "table keys (", keys.numel(),
              ") and masks (", masks.numel(), ") must be equally long");
  int64_t cap = keys.numel();
  // 2^31 at most: the kernels count probes in a uint32 up to cap-1
  TORCH_CHECK(cap >= 1 && cap <= (int64_t(1) << 31) && (cap & (cap - 1)) == 0,
              "table cap must be 2^k, 1 <= cap <= 2^31");
}

void check_hashes(const torch::Tensor& hashes, const torch::Tensor& keys) {
  CHECK_GPU(hashes);
  TORCH_CHECK(hashes.scalar_type() == at::kUInt64, "hashes must be uint64");
  TORCH_CHECK(hashes.device() == keys.device(),
              "hashes must be on the table's device");
}

std::vector<torch::Tensor> hash_prompts(torch::Tensor tokens,
                                        torch::Tensor offsets,
                                        int64_t block_tokens,
                                        int64_t max_blocks, int64_t seed0) {
  CHECK_GPU(tokens);
  CHECK_GPU(offsets);
  TORCH_CHECK(tokens.dtype() == torch::kInt32 && offsets.dtype() == torch::kInt64);
  TORCH_CHECK(offsets.device() == tokens.device(),
              "tokens and offsets must be on one device");
  TORCH_CHECK(block_tokens >= 1 && block_tokens <= INT_MAX,
              "block_tokens must be >= 1, got ", block_tokens);
  TORCH_CHECK(max_blocks >= 1 && max_blocks <= INT_MAX,
              "max_blocks must be >= 1, got ", max_blocks);
  TORCH_CHECK(offsets.numel() >= 1,
              "offsets must hold R+1 >= 1 values (request starts and the end)");
  int n_req = (int)offsets.size(0) - 1;
  auto hashes = torch::zeros({n_req, max_blocks},
                             tokens.options().dtype(torch::kUInt64));
  auto counts = torch::zeros({n_req}, tokens.options().dtype(torch::kInt32));
  CHECK_HIP(lds_hash_prompts(
      tokens.data_ptr<int32_t>(), offsets.data_ptr<int64_t>(), n_req,
      (int)block_tokens, (int)max_blocks, (uint64_t)seed0,
      (uint64_t*)hashes.data_ptr(), counts.data_ptr<int32_t>(), cur_stream()));
  return {hashes, counts};
}

// dropped: optional one-element int32 counter on the table's device; an
// insert that finds no slot in cap probes adds 1 to it.
void table_update(torch::Tensor keys, torch::Tensor masks,
                  torch::Tensor hashes, int64_t endpoint, bool is_remove,
                  c10::optional<torch::Tensor> dropped) {
  check_table(keys, masks);
  check_hashes(hashes, keys);
  TORCH_CHECK(endpoint >= 0 && endpoint < 64,
              "endpoint must be in [0, 64), got ", endpoint);
  unsigned int* dropped_ptr = nullptr;
  if (dropped.has_value()) {
    CHECK_GPU(*dropped);
    TORCH_CHECK(dropped->scalar_type() == at::kInt && dropped->numel() == 1 &&
                dropped->device() == keys.device(),
                "dropped must be one int32 on the table's device");
    dropped_ptr = (unsigned int*)dropped->data_ptr<int32_t>();
  }
  CHECK_HIP(lds_table_update(
      (uint64_t*)keys.data_ptr(), (unsigned long long*)masks.data_ptr(),
      (uint32_t)(keys.size(0) - 1), (const uint64_t*)hashes.data_ptr(),
      hashes.numel(), (int)endpoint, is_remove ? 1 : 0, dropped_ptr,
      cur_stream()));
}

torch::Tensor match_longest(torch::Tensor keys, torch::Tensor masks,
                            torch::Tensor hashes, torch::Tensor counts,
                            int64_t n_endpoints) {
  check_table(keys, masks);
  check_hashes(hashes, keys);
  CHECK_GPU(counts);
  TORCH_CHECK(hashes.dim() == 2, "hashes must be [R, max_blocks]");
  TORCH_CHECK(hashes.size(1) <= INT_MAX, "hashes rows are too long");
  TORCH_CHECK(counts.scalar_type() == at::kInt &&
              counts.device() == keys.device(),
              "counts must be int32 on the table's device");
  TORCH_CHECK(counts.numel() == hashes.size(0), "counts (", counts.numel(),
              ") must hold one value per hashes row (", hashes.size(0), ")");
  TORCH_CHECK(n_endpoints >= 1 && n_endpoints <= 64,
              "n_endpoints must be in [1, 64], got ", n_endpoints);
  int n_req = (int)hashes.size(0);
  auto out = torch::zeros({n_req, n_endpoints},
                          hashes.options().dtype(torch::kInt32));
  CHECK_HIP(lds_match_longest(
      (const uint64_t*)keys.data_ptr(), (const unsigned long long*)masks.data_ptr(),
      (uint32_t)(keys.size(0) - 1), (const uint64_t*)hashes.data_ptr(),
      counts.data_ptr<int32_t>(), n_req, (int)hashes.size(1), (int)n_endpoints,
      out.data_ptr<int32_t>(), cur_stream()));
  return out;
}

// ---- engine kernels ----

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps,
                      c10::optional<torch::Tensor> residual) {
  CHECK_GPU(x); CHECK_GPU(w);
  TORCH_CHECK(x.dtype() == torch::kBFloat16, "rmsnorm expects bf16");
  auto y = torch::empty_like(x);
  int H = (int)x.size(-1);
  int64_t rows = x.numel() / H;
  void* res_ptr = nullptr;
  if (residual.has_value()) {
    CHECK_GPU(*residual);
    res_ptr = residual->data_ptr();
  }
  CHECK_HIP(lds_rmsnorm(x.data_ptr(), res_ptr, w.data_ptr(), y.data_ptr(),
                        rows, H, (float)eps, cur_stream()));
  return y;
}

void rope(torch::Tensor q, torch::Tensor k, torch::Tensor cos_sin,
          torch::Tensor positions) {
  CHECK_GPU(q); CHECK_GPU(k); CHECK_GPU(cos_sin); CHECK_GPU(positions);
  int T = (int)q.size(0);
  int qh = (int)q.size(1), kvh = (int)k.size(1), d = (int)q.size(2);
  CHECK_HIP(lds_rope(q.data_ptr(), k.data_ptr(), cos_sin.data_ptr<float>(),
                     positions.data_ptr<int32_t>(), T, qh, kvh, d,
                     cur_stream()));
}

torch::Tensor silu_mul(torch::Tensor gate_up) {
  CHECK_GPU(gate_up);
  int64_t I2 = gate_up.size(-1);
  int64_t T = gate_up.numel() / I2;
  auto sizes = gate_up.sizes().vec();
  sizes.back() = I2 / 2;
  auto y = torch::empty(sizes, gate_up.options());
  CHECK_HIP(lds_silu_mul(gate_up.data_ptr(), y.data_ptr(), T, (int)(I2 / 2),
                         cur_stream()));
  return y;
}

void reshape_and_cache(torch::Tensor k_new, torch::Tensor v_new,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor slots,
                       c10::optional<torch::Tensor> k_inv_scale,
                       c10::optional<torch::Tensor> v_inv_scale) {
  CHECK_GPU(k_new); CHECK_GPU(v_new); CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  CHECK_GPU(slots);
  const float* kis = kv_scale_ptr(k_inv_scale, k_cache, "k_inv_scale");
  const float* vis = kv_scale_ptr(v_inv_scale, v_cache, "v_inv_scale");
  int T = (int)k_new.size(0), kvh = (int)k_new.size(1), d = (int)k_new.size(2);
  int bs = (int)k_cache.size(2);
  CHECK_HIP(lds_reshape_and_cache(k_new.data_ptr(), v_new.data_ptr(),
                                  k_cache.data_ptr(), v_cache.data_ptr(),
                                  slots.data_ptr<int64_t>(), T, kvh, bs, d,
                                  kv_fp8_flag(k_cache), kis, vis,
                                  cur_stream()));
}

void move_blocks(torch::Tensor pool, torch::Tensor staging,
                 torch::Tensor block_ids, bool is_scatter) {
  CHECK_GPU(pool); CHECK_GPU(staging); CHECK_GPU(block_ids);
  // pool: [L, 2, NB, KVH, BS, D]; staging: [n, L, 2, KVH, BS, D]
  int L = (int)pool.size(0);
  int64_t nb = pool.size(2);
  int64_t block_bytes = pool.size(3) * pool.size(4) * pool.size(5) *
                        pool.element_size();
  CHECK_HIP(lds_gather_blocks(pool.data_ptr(), staging.data_ptr(),
                              block_ids.data_ptr<int32_t>(),
                              (int)block_ids.size(0), L, nb, block_bytes,
                              is_scatter ? 1 : 0, cur_stream()));
}

// ---- HIP IPC surface for the direct peer-pull transfer path -------------
// The KV pool is allocated with its own hipMalloc (NOT the caching
// allocator, whose suballocation offsets would corrupt IPC handles); the
// decode rank opens the prefill rank's handle once and pulls blocks with
// copy_blocks_peer over the mapped pointer (xGMI one-sided read).

torch::Tensor ipc_alloc_tensor(std::vector<int64_t> shape,
                               torch::Tensor like) {
  int64_t numel = 1;
  for (auto s : shape) numel *= s;
  int64_t nbytes = numel * like.element_size();
  void* ptr = nullptr;
  CHECK_HIP(hipMalloc(&ptr, nbytes));
  CHECK_HIP(hipMemset(ptr, 0, nbytes));
  auto deleter = [](void* p) { (void)hipFree(p); };
  return torch::from_blob(ptr, shape, deleter,
                          like.options());
}

py::bytes ipc_handle(torch::Tensor t) {
  hipIpcMemHandle_t h;
  CHECK_HIP(hipIpcGetMemHandle(&h, t.data_ptr()));
  return py::bytes(reinterpret_cast<const char*>(&h), sizeof(h));
}

uintptr_t ipc_open(py::bytes handle) {
  std::string s = handle;
  TORCH_CHECK(s.size() == sizeof(hipIpcMemHandle_t), "bad IPC handle size");
  hipIpcMemHandle_t h;
  memcpy(&h, s.data(), sizeof(h));
  void* ptr = nullptr;
  hipError_t err =
      hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
  TORCH_CHECK(err == hipSuccess, "hipIpcOpenMemHandle: ",
              hipGetErrorString(err));
  return reinterpret_cast<uintptr_t>(ptr);
}

void ipc_close(uintptr_t ptr) {
  CHECK_HIP(hipIpcCloseMemHandle(reinterpret_cast<void*>(ptr)));
}

extern "C" hipError_t lds_copy_blocks_peer(const void*, void*, const int32_t*,
                                           const int32_t*, int, int, int64_t,
                                           int64_t, int64_t, hipStream_t);

void copy_blocks_peer(uintptr_t src_pool_ptr, torch::Tensor dst_pool,
                      torch::Tensor src_ids, torch::Tensor dst_ids,
                      int64_t src_nb) {
  CHECK_GPU(dst_pool); CHECK_GPU(src_ids); CHECK_GPU(dst_ids);
  int L = (int)dst_pool.size(0);
  int64_t dst_nb = dst_pool.size(2);
  int64_t block_bytes = dst_pool.size(3) * dst_pool.size(4) *
                        dst_pool.size(5) * dst_pool.element_size();
  CHECK_HIP(lds_copy_blocks_peer(
      reinterpret_cast<const void*>(src_pool_ptr), dst_pool.data_ptr(),
      src_ids.data_ptr<int32_t>(), dst_ids.data_ptr<int32_t>(),
      (int)src_ids.size(0), L, src_nb, dst_nb, block_bytes, cur_stream()));
}

torch::Tensor paged_attention(torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache,
                              torch::Tensor block_tables,
                              torch::Tensor seq_lens, double scale,
                              int64_t chunk,
                              c10::optional<torch::Tensor> k_scale,
                              c10::optional<torch::Tensor> v_scale) {
  CHECK_GPU(q); CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  CHECK_GPU(block_tables); CHECK_GPU(seq_lens);
  const float* ks = kv_scale_ptr(k_scale, k_cache, "k_scale");
  const float* vs = kv_scale_ptr(v_scale, v_cache, "v_scale");
  int B = (int)q.size(0), qh = (int)q.size(1), d = (int)q.size(2);
  int kvh = (int)k_cache.size(1), bs = (int)k_cache.size(2);
  auto out = torch::empty_like(q);
  CHECK_HIP(lds_paged_attention(
      q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
      out.data_ptr(), B, qh, kvh, bs, d, (int)block_tables.size(1),
      kv_fp8_flag(k_cache), (int)chunk, (float)scale, ks, vs,
      cur_stream()));
  return out;
}

torch::Tensor paged_attention_split(torch::Tensor q, torch::Tensor k_cache,
                                    torch::Tensor v_cache,
                                    torch::Tensor block_tables,
                                    torch::Tensor seq_lens, int64_t n_parts,
                                    int64_t part_tokens, double scale,
                                    int64_t chunk,
                                    c10::optional<torch::Tensor> k_scale,
                                    c10::optional<torch::Tensor> v_scale) {
  CHECK_GPU(q); CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  CHECK_GPU(block_tables); CHECK_GPU(seq_lens);
  const float* ks = kv_scale_ptr(k_scale, k_cache, "k_scale");
  const float* vs = kv_scale_ptr(v_scale, v_cache, "v_scale");
  int B = (int)q.size(0), qh = (int)q.size(1), d = (int)q.size(2);
  int kvh = (int)k_cache.size(1), bs = (int)k_cache.size(2);
  int qpg = qh / kvh;
  auto out = torch::empty_like(q);
  auto f32 = q.options().dtype(torch::kFloat32);
  auto part_o = torch::empty({B, kvh, n_parts, qpg, d}, f32);
  auto part_ml = torch::empty({B, kvh, n_parts, qpg, 2}, f32);
  CHECK_HIP(lds_paged_attention_split(
      q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
      out.data_ptr(), part_o.data_ptr<float>(), part_ml.data_ptr<float>(), B,
      qh, kvh, bs, d, (int)block_tables.size(1), (int)n_parts,
      (int)part_tokens, kv_fp8_flag(k_cache), (int)chunk, (float)scale, ks,
      vs, cur_stream()));
  return out;
}

torch::Tensor flash_prefill(torch::Tensor q, torch::Tensor k_cache,
                            torch::Tensor v_cache, torch::Tensor block_tables,
                            torch::Tensor seq_meta, torch::Tensor tiles,
                            double scale,
                            c10::optional<torch::Tensor> k_scale,
                            c10::optional<torch::Tensor> v_scale) {
  CHECK_GPU(q); CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  CHECK_GPU(block_tables); CHECK_GPU(seq_meta); CHECK_GPU(tiles);
  const float* ks = kv_scale_ptr(k_scale, k_cache, "k_scale");
  const float* vs = kv_scale_ptr(v_scale, v_cache, "v_scale");
  TORCH_CHECK(q.dtype() == torch::kBFloat16, "flash_prefill expects bf16");
  int qh = (int)q.size(1), d = (int)q.size(2);
  int kvh = (int)k_cache.size(1), bs = (int)k_cache.size(2);
  auto out = torch::empty_like(q);
  // bf16 KV rides the glds staging pipeline; fp8 needs convert-on-stage.
  // LLMD_NO_GLDS=1 forces the plain-VGPR kernel (bisect knob for the
  // cross-stream wedge investigation, profiles/r02_notes.md).
  static const bool no_glds = []() {
    const char* e = getenv("LLMD_NO_GLDS");
    return e && e[0] == '1';
  }();
  if (!no_glds && !kv_fp8_flag(k_cache) &&
      block_tables.size(1) <= FLASH_GLDS_BT_CAP) {
    CHECK_HIP(lds_flash_prefill_glds(
        q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        block_tables.data_ptr<int32_t>(), seq_meta.data_ptr<int32_t>(),
        tiles.data_ptr<int32_t>(), out.data_ptr(), (int)tiles.size(0), qh,
        kvh, bs, d, (int)block_tables.size(1), (float)scale, cur_stream()));
    return out;
  }
  CHECK_HIP(lds_flash_prefill(
      q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr<int32_t>(), seq_meta.data_ptr<int32_t>(),
      tiles.data_ptr<int32_t>(), out.data_ptr(), (int)tiles.size(0), qh, kvh,
      bs, d, (int)block_tables.size(1), kv_fp8_flag(k_cache), (float)scale,
      ks, vs, cur_stream()));
  return out;
}

// ---- sampler ----

// One per-row parameter vector of sample(): [B], on the logits' device.
void check_sample_param(const torch::Tensor& t, const torch::Tensor& logits,
                        at::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == logits.device(), name,
              " must be on the logits' device");
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == logits.size(0), name,
              " must hold ", logits.size(0), " values (one per row), got ",
              t.numel());
}

std::vector<torch::Tensor> sample(torch::Tensor logits,
                                  torch::Tensor temperature,
                                  torch::Tensor top_k, torch::Tensor top_p,
                                  torch::Tensor seed, torch::Tensor pos) {
  TORCH_CHECK(logits.is_cuda(), "logits must be on GPU");
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  TORCH_CHECK(logits.is_contiguous(), "logits must be contiguous");
  const bool f32 = logits.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || logits.scalar_type() == at::kBFloat16,
              "logits must be bf16 or float32");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (1LL << 31),
              "vocabulary size out of range");
  check_sample_param(temperature, logits, at::kFloat, "temperature");
  check_sample_param(top_k, logits, at::kInt, "top_k");
  check_sample_param(top_p, logits, at::kFloat, "top_p");
  check_sample_param(seed, logits, at::kLong, "seed");
  check_sample_param(pos, logits, at::kInt, "pos");
  int B = (int)logits.size(0), V = (int)logits.size(1);
  auto opt = logits.options();
  auto tokens = torch::empty({B}, opt.dtype(torch::kInt64));
  auto logprobs = torch::empty({B}, opt.dtype(torch::kFloat32));
  auto n_kept = torch::empty({B}, opt.dtype(torch::kInt32));
  auto threshold = torch::empty({B}, opt.dtype(torch::kFloat32));
  CHECK_HIP(lds_sample(logits.data_ptr(), temperature.data_ptr<float>(),
                       top_k.data_ptr<int32_t>(), top_p.data_ptr<float>(),
                       seed.data_ptr<int64_t>(), pos.data_ptr<int32_t>(), B, V,
                       f32 ? 1 : 0, tokens.data_ptr<int64_t>(),
                       logprobs.data_ptr<float>(), n_kept.data_ptr<int32_t>(),
                       threshold.data_ptr<float>(), cur_stream()));
  return {tokens, logprobs, n_kept, threshold};
}

// The token state of sample_ext / token_state_fill: int16 [R, Vs] on
// `like`'s device, rows contiguous and 16-byte aligned, Vs = V rounded up
// to a multiple of 8.
void check_token_state(const torch::Tensor& state, const torch::Tensor& like,
                       int64_t V) {
  TORCH_CHECK(state.is_cuda() && state.device() == like.device(),
              "state must be on the same device as the other arguments");
  TORCH_CHECK(state.scalar_type() == at::kShort, "state must be int16");
  TORCH_CHECK(state.dim() == 2, "state must be [R, Vs]");
  TORCH_CHECK(state.is_contiguous(), "state must be contiguous");
  TORCH_CHECK(state.size(1) == (V + 7) / 8 * 8, "state must have Vs = ",
              (V + 7) / 8 * 8, " columns (V = ", V,
              " rounded up to a multiple of 8), got ", state.size(1));
  TORCH_CHECK(state.size(0) < (1LL << 31), "too many state rows");
  TORCH_CHECK(((uintptr_t)state.data_ptr() & 15u) == 0,
              "state must be 16-byte aligned");
}

// sample() plus repetition / presence / frequency penalties read from the
// token state, min_p, the top-N raw logprobs and the state update. n_top is
// the width of the top-N outputs; a row's top_n is clamped to it on device.
// Rows of one launch must not share a state_row >= 0 (not checkable without
// a sync; see DEVELOPMENT.md "Sampling").
std::vector<torch::Tensor> sample_ext(
    torch::Tensor logits, torch::Tensor temperature, torch::Tensor top_k,
    torch::Tensor top_p, torch::Tensor seed, torch::Tensor pos,
    torch::Tensor rep, torch::Tensor pres, torch::Tensor freq,
    torch::Tensor min_p, torch::Tensor top_n, torch::Tensor state_row,
    c10::optional<torch::Tensor> state, int64_t n_top) {
  TORCH_CHECK(logits.is_cuda(), "logits must be on GPU");
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  TORCH_CHECK(logits.is_contiguous(), "logits must be contiguous");
  const bool f32 = logits.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || logits.scalar_type() == at::kBFloat16,
              "logits must be bf16 or float32");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (1LL << 31),
              "vocabulary size out of range");
  check_sample_param(temperature, logits, at::kFloat, "temperature");
  check_sample_param(top_k, logits, at::kInt, "top_k");
  check_sample_param(top_p, logits, at::kFloat, "top_p");
  check_sample_param(seed, logits, at::kLong, "seed");
  check_sample_param(pos, logits, at::kInt, "pos");
  check_sample_param(rep, logits, at::kFloat, "rep");
  check_sample_param(pres, logits, at::kFloat, "pres");
  check_sample_param(freq, logits, at::kFloat, "freq");
  check_sample_param(min_p, logits, at::kFloat, "min_p");
  check_sample_param(top_n, logits, at::kInt, "top_n");
  check_sample_param(state_row, logits, at::kInt, "state_row");
  TORCH_CHECK(n_top >= 0 && n_top <= 20, "n_top must be in [0, 20], got ",
              n_top);
  int B = (int)logits.size(0), V = (int)logits.size(1);
  int16_t* st = nullptr;
  int R = 0;
  int64_t Vs = 0;
  if (state.has_value()) {
    check_token_state(*state, logits, V);
    st = state->data_ptr<int16_t>();
    R = (int)state->size(0);
    Vs = state->size(1);
  }
  auto opt = logits.options();
  auto tokens = torch::empty({B}, opt.dtype(torch::kInt64));
  auto logprobs = torch::empty({B}, opt.dtype(torch::kFloat32));
  auto n_kept = torch::empty({B}, opt.dtype(torch::kInt32));
  auto threshold = torch::empty({B}, opt.dtype(torch::kFloat32));
  auto top_tokens = torch::empty({B, n_top}, opt.dtype(torch::kInt64));
  auto top_logprobs = torch::empty({B, n_top}, opt.dtype(torch::kFloat32));
  CHECK_HIP(lds_sample_ext(
      logits.data_ptr(), temperature.data_ptr<float>(),
      top_k.data_ptr<int32_t>(), top_p.data_ptr<float>(),
      seed.data_ptr<int64_t>(), pos.data_ptr<int32_t>(),
      rep.data_ptr<float>(), pres.data_ptr<float>(), freq.data_ptr<float>(),
      min_p.data_ptr<float>(), top_n.data_ptr<int32_t>(),
      state_row.data_ptr<int32_t>(), st, R, Vs, B, V, f32 ? 1 : 0,
      (int)n_top, tokens.data_ptr<int64_t>(), logprobs.data_ptr<float>(),
      n_kept.data_ptr<int32_t>(), threshold.data_ptr<float>(),
      top_tokens.data_ptr<int64_t>(), top_logprobs.data_ptr<float>(),
      cur_stream()));
  return {tokens, logprobs, n_kept, threshold, top_tokens, top_logprobs};
}

// Rebuild the listed state rows from token histories: for entry q, row
// rows[q] is cleared, tokens[offsets[q] : offsets[q] + n_prompt[q]] set the
// prompt bit and tokens[offsets[q] + n_prompt[q] : offsets[q + 1]] are
// counted. V is the vocabulary size (state has Vs columns). The kernel
// clamps offsets into tokens and skips rows and ids out of range.
void token_state_fill(torch::Tensor state, torch::Tensor rows,
                      torch::Tensor tokens, torch::Tensor offsets,
                      torch::Tensor n_prompt, int64_t V) {
  TORCH_CHECK(V >= 1 && V < (1LL << 31), "vocabulary size out of range");
  TORCH_CHECK(rows.is_cuda(), "rows must be on GPU");
  check_token_state(state, rows, V);
  for (const torch::Tensor* t : {&tokens, &offsets, &n_prompt})
    TORCH_CHECK(t->is_cuda() && t->device() == rows.device(),
                "rows, tokens, offsets and n_prompt must be on one device");
  TORCH_CHECK(rows.scalar_type() == at::kInt &&
              tokens.scalar_type() == at::kInt &&
              n_prompt.scalar_type() == at::kInt,
              "rows, tokens and n_prompt must be int32");
  TORCH_CHECK(offsets.scalar_type() == at::kLong, "offsets must be int64");
  TORCH_CHECK(rows.dim() == 1 && tokens.dim() == 1 && offsets.dim() == 1 &&
              n_prompt.dim() == 1, "rows, tokens, offsets and n_prompt "
              "must be one-dimensional");
  TORCH_CHECK(rows.is_contiguous() && tokens.is_contiguous() &&
              offsets.is_contiguous() && n_prompt.is_contiguous(),
              "rows, tokens, offsets and n_prompt must be contiguous");
  TORCH_CHECK(n_prompt.numel() == rows.numel() &&
              offsets.numel() == rows.numel() + 1,
              "n_prompt must hold one value per row and offsets one more, "
              "got ", rows.numel(), " rows, ", n_prompt.numel(),
              " n_prompt, ", offsets.numel(), " offsets");
  TORCH_CHECK(rows.numel() < (1LL << 31), "too many rows");
  CHECK_HIP(lds_token_state_fill(
      state.data_ptr<int16_t>(), (int)state.size(0), state.size(1), (int)V,
      rows.data_ptr<int32_t>(), (int)rows.numel(),
      tokens.data_ptr<int32_t>(), tokens.numel(),
      offsets.data_ptr<int64_t>(), n_prompt.data_ptr<int32_t>(),
      cur_stream()));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X gfx950 kernels: prefix-cache hashing/match, paged KV, decode attention";
  m.def("hash_prompts", &hash_prompts, "batched chained block hashing");
  m.def("table_update", &table_update, "device prefix table insert/remove",
        py::arg("keys"), py::arg("masks"), py::arg("hashes"),
        py::arg("endpoint"), py::arg("is_remove"),
        py::arg("dropped") = py::none());
  m.def("match_longest", &match_longest, "device longest-prefix match");
  m.def("rmsnorm", &rmsnorm, py::arg("x"), py::arg("w"), py::arg("eps"),
        py::arg("residual") = py::none());
  m.def("rope", &rope, "in-place NeoX RoPE");
  m.def("silu_mul", &silu_mul, "fused SiLU*up on packed gate_up");
  m.def("reshape_and_cache", &reshape_and_cache,
        "scatter K/V into paged pool", py::arg("k_new"), py::arg("v_new"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("slots"),
        py::arg("k_inv_scale") = py::none(),
        py::arg("v_inv_scale") = py::none());
  m.def("move_blocks", &move_blocks, "gather/scatter KV blocks for xGMI transfer");
  m.def("ipc_alloc_tensor", &ipc_alloc_tensor,
        "hipMalloc-backed tensor (IPC-shareable, outside the caching allocator)");
  m.def("ipc_handle", &ipc_handle, "hipIpcGetMemHandle of a tensor");
  m.def("ipc_open", &ipc_open, "map a peer pool (hipIpcOpenMemHandle)");
  m.def("ipc_close", &ipc_close, "unmap a peer pool");
  m.def("copy_blocks_peer", &copy_blocks_peer,
        "one-sided xGMI pull of KV blocks from a mapped peer pool");
  m.def("paged_attention", &paged_attention,
        "GQA decode attention over paged KV", py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("block_tables"),
        py::arg("seq_lens"), py::arg("scale"), py::arg("chunk") = 256,
        py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none());
  m.def("paged_attention_split", &paged_attention_split,
        "flash-decoding GQA attention with sequence partitioning",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_lens"), py::arg("n_parts"),
        py::arg("part_tokens"), py::arg("scale"), py::arg("chunk") = 256,
        py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none());
  m.def("flash_prefill", &flash_prefill,
        "fused MFMA causal varlen prefill attention over paged KV",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_meta"), py::arg("tiles"),
        py::arg("scale"), py::arg("k_scale") = py::none(),
        py::arg("v_scale") = py::none());
  m.def("sample", &sample,
        "fused temperature/top-k/top-p/seeded sampler with logprobs -> "
        "(tokens, logprobs, n_kept, threshold)",
        py::arg("logits"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("seed"), py::arg("pos"));
  m.def("sample_ext", &sample_ext,
        "sample with penalties from the token state, min_p and top-N -> "
        "(tokens, logprobs, n_kept, threshold, top_tokens, top_logprobs)",
        py::arg("logits"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("seed"), py::arg("pos"), py::arg("rep"),
        py::arg("pres"), py::arg("freq"), py::arg("min_p"),
        py::arg("top_n"), py::arg("state_row"),
        py::arg("state") = py::none(), py::arg("n_top") = 0);
  m.def("token_state_fill", &token_state_fill,
        "rebuild token-state rows from prompt and output token lists",
        py::arg("state"), py::arg("rows"), py::arg("tokens"),
        py::arg("offsets"), py::arg("n_prompt"), py::arg("V"));
}
