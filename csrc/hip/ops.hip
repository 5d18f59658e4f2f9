// ops.hip — torch extension binding for the gfx950 kernels (`_hip_ops`).
// Pure HIP (no hipify, no CUDA shims): includes the ROCm-native ATen HIP
// headers directly and drives hipStream_t launchers from the .hip kernels.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <hip/hip_runtime.h>

#include <climits>

#include "launchers.h"

#define CHECK_HIP(expr)                                                    \
  do {                                                                     \
    hipError_t err__ = (expr);                                             \
    TORCH_CHECK(err__ == hipSuccess, "HIP error: ", hipGetErrorString(err__)); \
  } while (0)

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous on GPU")

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

// ---- the argument contract (DEVELOPMENT.md "Op argument contract") ----
// Every binding checks each argument with one of these before it allocates
// or launches anything: the launchers and kernels trust what they get.

// An integer argument or extent in [lo, hi] (hi <= INT_MAX), narrowed.
int check_int(int64_t v, int64_t lo, int64_t hi, const char* name) {
  TORCH_CHECK(v >= lo && v <= hi, name, " must be in [", lo, ", ", hi,
              "], got ", v);
  return (int)v;
}

// A tensor argument: on `anchor`'s device (a binding's first tensor is its
// own anchor), of `dtype`, contiguous.
void check_tensor(const torch::Tensor& t, const char* name,
                  const torch::Tensor& anchor, const char* anchor_name,
                  at::ScalarType dtype) {
  TORCH_CHECK(t.is_cuda(), name, " must be on a GPU");
  TORCH_CHECK(t.device() == anchor.device(), name, " must be on ",
              anchor_name, "'s device");
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// ... and of the rank of `shape`, with every extent that `shape` fixes.
constexpr int64_t ANY = -1;

std::string shape_str(at::IntArrayRef shape) {
  std::string s = "[";
  for (size_t i = 0; i < shape.size(); ++i)
    s += (i ? ", " : "") + (shape[i] == ANY ? "*" : std::to_string(shape[i]));
  return s + "]";
}

void check_tensor(const torch::Tensor& t, const char* name,
                  const torch::Tensor& anchor, const char* anchor_name,
                  at::ScalarType dtype, at::IntArrayRef shape) {
  check_tensor(t, name, anchor, anchor_name, dtype);
  bool ok = t.dim() == (int64_t)shape.size();
  for (size_t i = 0; ok && i < shape.size(); ++i)
    ok = shape[i] == ANY || t.size(i) == shape[i];
  TORCH_CHECK(ok, name, " must have shape ", shape_str(shape), ", got ",
              t.sizes());
}

// grid.y / grid.z limit: head counts and partitions ride there
constexpr int64_t GRID_YZ_MAX = 65535;

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
  int n_req = check_int(offsets.numel() - 1, 0, INT_MAX, "request count");
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
  int n_req = check_int(hashes.size(0), 0, INT_MAX, "hashes.size(0)");
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
  check_tensor(x, "x", x, "x", at::kBFloat16);
  TORCH_CHECK(x.dim() >= 1, "x must have at least one dimension");
  const int64_t H64 = x.size(-1);
  TORCH_CHECK(H64 % 8 == 0, "x.size(-1) must be a multiple of 8, got ", H64);
  const int H = check_int(H64, 8, INT_MAX, "x.size(-1)");
  const int64_t rows = check_int(x.numel() / H, 0, INT_MAX, "rows of x");
  check_tensor(w, "w", x, "x", at::kBFloat16, {H});
  void* res_ptr = nullptr;
  if (residual.has_value()) {
    check_tensor(*residual, "residual", x, "x", at::kBFloat16, x.sizes());
    res_ptr = residual->data_ptr();
  }
  auto y = torch::empty_like(x);
  CHECK_HIP(lds_rmsnorm(x.data_ptr(), res_ptr, w.data_ptr(), y.data_ptr(),
                        rows, H, (float)eps, cur_stream()));
  return y;
}

void rope(torch::Tensor q, torch::Tensor k, torch::Tensor cos_sin,
          torch::Tensor positions) {
  check_tensor(q, "q", q, "q", at::kBFloat16, {ANY, ANY, ANY});
  const int64_t T = q.size(0), D = q.size(2);
  TORCH_CHECK(D % 2 == 0, "head dim q.size(2) must be even, got ", D);
  const int d = check_int(D, 2, 2048, "head dim q.size(2)");
  check_tensor(k, "k", q, "q", at::kBFloat16, {T, ANY, D});
  check_tensor(cos_sin, "cos_sin", q, "q", at::kFloat, {ANY, D / 2, 2});
  check_tensor(positions, "positions", q, "q", at::kInt, {T});
  check_int(q.size(1) + k.size(1), 1, GRID_YZ_MAX, "q heads + k heads");
  CHECK_HIP(lds_rope(q.data_ptr(), k.data_ptr(), cos_sin.data_ptr<float>(),
                     positions.data_ptr<int32_t>(),
                     check_int(T, 0, INT_MAX, "q.size(0)"), (int)q.size(1),
                     (int)k.size(1), d, cur_stream()));
}

torch::Tensor silu_mul(torch::Tensor gate_up) {
  check_tensor(gate_up, "gate_up", gate_up, "gate_up", at::kBFloat16);
  TORCH_CHECK(gate_up.dim() >= 1, "gate_up must have at least one dimension");
  const int64_t I2 = gate_up.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "gate_up.size(-1) must be 2*I with I a multiple "
              "of 8, got ", I2);
  const int I = check_int(I2 / 2, 8, INT_MAX, "I = gate_up.size(-1) / 2");
  int64_t T = gate_up.numel() / I2;
  auto sizes = gate_up.sizes().vec();
  sizes.back() = I;
  auto y = torch::empty(sizes, gate_up.options());
  CHECK_HIP(lds_silu_mul(gate_up.data_ptr(), y.data_ptr(), T, I,
                         cur_stream()));
  return y;
}

void reshape_and_cache(torch::Tensor k_new, torch::Tensor v_new,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor slots,
                       c10::optional<torch::Tensor> k_inv_scale,
                       c10::optional<torch::Tensor> v_inv_scale) {
  check_tensor(k_new, "k_new", k_new, "k_new", at::kBFloat16,
               {ANY, ANY, ANY});
  const int64_t T = k_new.size(0), KVH = k_new.size(1), D = k_new.size(2);
  TORCH_CHECK(D % 8 == 0, "head dim k_new.size(2) must be a multiple of 8, "
              "got ", D);
  check_int(KVH * (D / 8), 1, INT_MAX, "KVH * D / 8");
  check_tensor(v_new, "v_new", k_new, "k_new", at::kBFloat16, {T, KVH, D});
  const int fp8 = kv_fp8_flag(k_cache);
  check_tensor(k_cache, "k_cache", k_new, "k_new", k_cache.scalar_type(),
               {ANY, KVH, ANY, D});
  check_tensor(v_cache, "v_cache", k_new, "k_new", k_cache.scalar_type(),
               k_cache.sizes());
  const int bs = check_int(k_cache.size(2), 1, INT_MAX,
                           "block size k_cache.size(2)");
  check_tensor(slots, "slots", k_new, "k_new", at::kLong, {T});
  const float* kis = kv_scale_ptr(k_inv_scale, k_cache, "k_inv_scale");
  const float* vis = kv_scale_ptr(v_inv_scale, v_cache, "v_inv_scale");
  CHECK_HIP(lds_reshape_and_cache(
      k_new.data_ptr(), v_new.data_ptr(), k_cache.data_ptr(),
      v_cache.data_ptr(), slots.data_ptr<int64_t>(),
      check_int(T, 0, INT_MAX, "k_new.size(0)"), (int)KVH, bs, (int)D, fp8,
      kis, vis, cur_stream()));
}

// The 16-byte accesses of qkv_rope_cache need their bases aligned.
void check_aligned16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(((uintptr_t)t.data_ptr() & 15u) == 0, name,
              " must be 16-byte aligned");
}

// The QKV GEMM's output row [q heads | k heads | v heads] -> rotated q
// [T, QH, D]; rotated K and plain V go to the caches at slots[t] (a negative
// slot stores nothing). Equals split + contiguous + rope + reshape_and_cache.
torch::Tensor qkv_rope_cache(torch::Tensor qkv, torch::Tensor cos_sin,
                             torch::Tensor positions, torch::Tensor slots,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             int64_t n_q_heads,
                             c10::optional<torch::Tensor> k_inv_scale,
                             c10::optional<torch::Tensor> v_inv_scale) {
  check_tensor(qkv, "qkv", qkv, "qkv", at::kBFloat16, {ANY, ANY});
  const int64_t T = check_int(qkv.size(0), 0, INT_MAX, "qkv.size(0)");
  const int fp8 = kv_fp8_flag(k_cache);
  check_tensor(k_cache, "k_cache", qkv, "qkv", k_cache.scalar_type(),
               {ANY, ANY, ANY, ANY});
  check_tensor(v_cache, "v_cache", qkv, "qkv", k_cache.scalar_type(),
               k_cache.sizes());
  const int kvh = check_int(k_cache.size(1), 1, 65536, "KV heads");
  const int bs = check_int(k_cache.size(2), 1, INT_MAX,
                           "block size k_cache.size(2)");
  const int64_t D = k_cache.size(3);
  TORCH_CHECK(D % 16 == 0, "head dim k_cache.size(3) must be a multiple of "
              "16, got ", D);
  const int d = check_int(D, 16, 2048, "head dim k_cache.size(3)");
  const int qh = check_int(n_q_heads, 1, 65536, "n_q_heads");
  TORCH_CHECK(qkv.size(1) == (qh + 2 * (int64_t)kvh) * D, "qkv.size(1) must "
              "be (n_q_heads + 2 * KV heads) * head dim = ",
              (qh + 2 * (int64_t)kvh) * D, ", got ", qkv.size(1));
  check_tensor(cos_sin, "cos_sin", qkv, "qkv", at::kFloat, {ANY, D / 2, 2});
  check_tensor(positions, "positions", qkv, "qkv", at::kInt, {T});
  check_tensor(slots, "slot_mapping", qkv, "qkv", at::kLong, {T});
  const float* kis = kv_scale_ptr(k_inv_scale, k_cache, "k_inv_scale");
  const float* vis = kv_scale_ptr(v_inv_scale, v_cache, "v_inv_scale");
  check_aligned16(qkv, "qkv");
  check_aligned16(cos_sin, "cos_sin");
  check_aligned16(k_cache, "k_cache");
  check_aligned16(v_cache, "v_cache");
  auto q = torch::empty({T, qh, D}, qkv.options());
  CHECK_HIP(lds_qkv_rope_cache(
      qkv.data_ptr(), cos_sin.data_ptr<float>(),
      positions.data_ptr<int32_t>(), slots.data_ptr<int64_t>(), q.data_ptr(),
      k_cache.data_ptr(), v_cache.data_ptr(), T, qh, kvh, bs, d, fp8, kis,
      vis, cur_stream()));
  return q;
}

// The KV pool of move_blocks / copy_blocks_peer: [L, 2, NB, KVH, BS, D] on
// a GPU, contiguous, one (layer, K/V) block a whole number of the 16-byte
// units the mover copies. Returns that block's bytes.
int64_t check_pool(const torch::Tensor& pool, const char* name) {
  check_tensor(pool, name, pool, name, pool.scalar_type(),
               {ANY, 2, ANY, ANY, ANY, ANY});
  TORCH_CHECK(pool.size(0) <= INT_MAX, name, " has too many layers (",
              pool.size(0), ")");
  const int64_t block_bytes = pool.size(3) * pool.size(4) * pool.size(5) *
                              (int64_t)pool.element_size();
  TORCH_CHECK(block_bytes % 16 == 0, name, ": one block (", block_bytes,
              " bytes) must be a multiple of 16 bytes");
  return block_bytes;
}

void move_blocks(torch::Tensor pool, torch::Tensor staging,
                 torch::Tensor block_ids, bool is_scatter) {
  const int64_t block_bytes = check_pool(pool, "pool");
  check_tensor(block_ids, "block_ids", pool, "pool", at::kInt, {ANY});
  const int64_t n = block_ids.size(0);
  check_tensor(staging, "staging", pool, "pool", pool.scalar_type(),
               {n, pool.size(0), 2, pool.size(3), pool.size(4), pool.size(5)});
  CHECK_HIP(lds_gather_blocks(pool.data_ptr(), staging.data_ptr(),
                              block_ids.data_ptr<int32_t>(),
                              check_int(n, 0, INT_MAX, "block_ids.size(0)"),
                              (int)pool.size(0), pool.size(2), block_bytes,
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

// src_pool_ptr: a peer pool [L, 2, src_nb, KVH, BS, D] mapped by ipc_open
// (or this process's own pool), of dst_pool's layout apart from src_nb.
void copy_blocks_peer(uintptr_t src_pool_ptr, torch::Tensor dst_pool,
                      torch::Tensor src_ids, torch::Tensor dst_ids,
                      int64_t src_nb) {
  TORCH_CHECK(src_pool_ptr != 0, "src_pool_ptr must not be null");
  const int64_t block_bytes = check_pool(dst_pool, "dst_pool");
  TORCH_CHECK(src_nb >= 1, "src_nb must be >= 1, got ", src_nb);
  check_tensor(src_ids, "src_ids", dst_pool, "dst_pool", at::kInt, {ANY});
  check_tensor(dst_ids, "dst_ids", dst_pool, "dst_pool", at::kInt, {ANY});
  TORCH_CHECK(src_ids.size(0) == dst_ids.size(0), "src_ids (",
              src_ids.size(0), ") and dst_ids (", dst_ids.size(0),
              ") must be equally long");
  CHECK_HIP(lds_copy_blocks_peer(
      reinterpret_cast<const void*>(src_pool_ptr), dst_pool.data_ptr(),
      src_ids.data_ptr<int32_t>(), dst_ids.data_ptr<int32_t>(),
      check_int(src_ids.size(0), 0, INT_MAX, "src_ids.size(0)"),
      (int)dst_pool.size(0), src_nb, dst_pool.size(2), block_bytes,
      cur_stream()));
}

// ---- attention ----

// What the three attention bindings share: q [N, QH, 128] bf16; the caches
// [NB, KVH, BS, 128], alike, bf16 or fp8; QH = 1, 2, 4 or 8 times KVH;
// block_tables [B, MB >= 1] int32; the optional fp8 scales. Returns the
// launch arguments with everything but `out` and the decode / prefill group
// filled in.
AttnArgs check_attention(const torch::Tensor& q, const torch::Tensor& k_cache,
                         const torch::Tensor& v_cache,
                         const torch::Tensor& block_tables, double scale,
                         const c10::optional<torch::Tensor>& k_scale,
                         const c10::optional<torch::Tensor>& v_scale) {
  AttnArgs a{};
  check_tensor(q, "q", q, "q", at::kBFloat16, {ANY, ANY, 128});
  check_int(q.size(0), 0, INT_MAX, "q.size(0)");
  a.kv_fp8 = kv_fp8_flag(k_cache);
  check_tensor(k_cache, "k_cache", q, "q", k_cache.scalar_type(),
               {ANY, ANY, ANY, 128});
  check_tensor(v_cache, "v_cache", q, "q", k_cache.scalar_type(),
               k_cache.sizes());
  a.kvh = check_int(k_cache.size(1), 1, GRID_YZ_MAX, "KV heads");
  a.bs = check_int(k_cache.size(2), 1, INT_MAX, "block size k_cache.size(2)");
  const int64_t QH = q.size(1), qpg = QH / a.kvh;
  TORCH_CHECK(QH % a.kvh == 0 &&
              (qpg == 1 || qpg == 2 || qpg == 4 || qpg == 8),
              "q heads (", QH, ") must be 1, 2, 4 or 8 times the KV heads (",
              a.kvh, ")");
  a.n_q_heads = (int)QH;
  a.head_dim = 128;
  check_tensor(block_tables, "block_tables", q, "q", at::kInt, {ANY, ANY});
  a.max_blocks = check_int(block_tables.size(1), 1, INT_MAX,
                           "max_blocks = block_tables.size(1)");
  a.k_scale = kv_scale_ptr(k_scale, k_cache, "k_scale");
  a.v_scale = kv_scale_ptr(v_scale, v_cache, "v_scale");
  a.q = q.data_ptr();
  a.k_cache = k_cache.data_ptr();
  a.v_cache = v_cache.data_ptr();
  a.block_tables = block_tables.data_ptr<int32_t>();
  a.scale = (float)scale;
  return a;
}

// Decode: one q row, one block_tables row and one seq_lens entry per
// sequence; chunk is the online-softmax chunk.
AttnArgs check_decode(const torch::Tensor& q, const torch::Tensor& k_cache,
                      const torch::Tensor& v_cache,
                      const torch::Tensor& block_tables,
                      const torch::Tensor& seq_lens, double scale,
                      int64_t chunk,
                      const c10::optional<torch::Tensor>& k_scale,
                      const c10::optional<torch::Tensor>& v_scale) {
  // The decode kernel keeps pool row indices (block*KVH + head)*BS + row in
  // an int32 table. This reads sizes alone, and comes first so that a pool
  // too large to allocate (a meta tensor) still reaches it.
  if (k_cache.dim() == 4) {
    const int64_t pool_rows =
        k_cache.size(0) * k_cache.size(1) * k_cache.size(2);
    TORCH_CHECK(pool_rows < (int64_t(1) << 31), "KV cache rows NB*KVH*BS (",
                pool_rows, ") must be below 2^31");
  }
  AttnArgs a = check_attention(q, k_cache, v_cache, block_tables, scale,
                               k_scale, v_scale);
  const int64_t B = block_tables.size(0);
  TORCH_CHECK(q.size(0) == B, "q (", q.size(0), " rows) and block_tables (",
              B, " rows) must hold one row per sequence");
  check_tensor(seq_lens, "seq_lens", q, "q", at::kInt, {B});
  TORCH_CHECK(chunk == 256 || chunk == 512, "chunk must be 256 or 512, got ",
              chunk);
  a.seq_lens = seq_lens.data_ptr<int32_t>();
  a.n_seqs = (int)B;
  a.chunk = (int)chunk;
  return a;
}

torch::Tensor paged_attention(torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache,
                              torch::Tensor block_tables,
                              torch::Tensor seq_lens, double scale,
                              int64_t chunk,
                              c10::optional<torch::Tensor> k_scale,
                              c10::optional<torch::Tensor> v_scale) {
  AttnArgs a = check_decode(q, k_cache, v_cache, block_tables, seq_lens,
                            scale, chunk, k_scale, v_scale);
  auto out = torch::empty_like(q);
  a.out = out.data_ptr();
  CHECK_HIP(lds_paged_attention(a, cur_stream()));
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
  AttnArgs a = check_decode(q, k_cache, v_cache, block_tables, seq_lens,
                            scale, chunk, k_scale, v_scale);
  // 64: the combine kernel's LDS table of per-partition scales
  a.n_parts = check_int(n_parts, 1, 64, "n_parts");
  a.part_tokens = check_int(part_tokens, 1, INT_MAX, "part_tokens");
  const int qpg = a.n_q_heads / a.kvh;
  auto out = torch::empty_like(q);
  auto f32 = q.options().dtype(torch::kFloat32);
  auto part_o = torch::empty({a.n_seqs, a.kvh, n_parts, qpg, 128}, f32);
  auto part_ml = torch::empty({a.n_seqs, a.kvh, n_parts, qpg, 2}, f32);
  a.out = out.data_ptr();
  a.part_o = part_o.data_ptr<float>();
  a.part_ml = part_ml.data_ptr<float>();
  CHECK_HIP(lds_paged_attention_split(a, cur_stream()));
  return out;
}

torch::Tensor flash_prefill(torch::Tensor q, torch::Tensor k_cache,
                            torch::Tensor v_cache, torch::Tensor block_tables,
                            torch::Tensor seq_meta, torch::Tensor tiles,
                            double scale,
                            c10::optional<torch::Tensor> k_scale,
                            c10::optional<torch::Tensor> v_scale) {
  AttnArgs a = check_attention(q, k_cache, v_cache, block_tables, scale,
                               k_scale, v_scale);
  // one (start, chunk, prior) row per block_tables row; tiles: (seq, vrow0)
  check_tensor(seq_meta, "seq_meta", q, "q", at::kInt,
               {block_tables.size(0), 3});
  check_tensor(tiles, "tiles", q, "q", at::kInt, {ANY, 2});
  a.seq_meta = seq_meta.data_ptr<int32_t>();
  a.tiles = tiles.data_ptr<int32_t>();
  a.n_tiles = check_int(tiles.size(0), 0, INT_MAX, "tiles.size(0)");
  auto out = torch::empty_like(q);
  a.out = out.data_ptr();
  // bf16 KV rides the glds staging pipeline; fp8 needs convert-on-stage.
  // LLMD_NO_GLDS=1 forces the plain-VGPR kernel (bisect knob for the
  // cross-stream wedge investigation, profiles/r02_notes.md).
  static const bool no_glds = []() {
    const char* e = getenv("LLMD_NO_GLDS");
    return e && e[0] == '1';
  }();
  if (!no_glds && !a.kv_fp8 && a.max_blocks <= FLASH_GLDS_BT_CAP)
    CHECK_HIP(lds_flash_prefill_glds(a, cur_stream()));
  else
    CHECK_HIP(lds_flash_prefill(a, cur_stream()));
  return out;
}

// ---- LoRA ----

// y[perm rows] += (x[perm rows] · A[slot]ᵀ) · B[slot]ᵀ in place, the slot
// taken from the row's tile (DEVELOPMENT.md "LoRA adapters"). perm: the
// adapter rows grouped by slot; tiles [n, 3]: (start in perm, count <= 16,
// slot). The entries of perm and tiles are the caller's to get right
// (ops.lora_worklist does): they are device data and checking them would
// cost a sync.
void lora_add(torch::Tensor y, torch::Tensor x, torch::Tensor A,
              torch::Tensor B, torch::Tensor perm, torch::Tensor tiles) {
  check_tensor(x, "x", x, "x", at::kBFloat16, {ANY, ANY});
  const int64_t T = x.size(0);
  check_int(T, 0, INT_MAX, "x.size(0)");
  TORCH_CHECK(x.size(1) % 32 == 0, "x.size(1) must be a multiple of 32, got ",
              x.size(1));
  check_tensor(y, "y", x, "x", at::kBFloat16, {T, ANY});
  TORCH_CHECK(y.size(1) % 16 == 0, "y.size(1) must be a multiple of 16, got ",
              y.size(1));
  check_tensor(A, "A", x, "x", at::kBFloat16, {ANY, ANY, x.size(1)});
  const int64_t S = A.size(0), R = A.size(1);
  TORCH_CHECK(S >= 1, "A must hold at least one slot");
  TORCH_CHECK(R % 16 == 0 && R >= 16 && R <= 64, "the pool rank A.size(1) "
              "must be a multiple of 16 in 16..64, got ", R);
  check_tensor(B, "B", x, "x", at::kBFloat16, {S, y.size(1), R});
  check_tensor(perm, "perm", x, "x", at::kInt, {ANY});
  TORCH_CHECK(perm.size(0) <= T, "perm (", perm.size(0), ") must not be "
              "longer than x has rows (", T, ")");
  check_tensor(tiles, "tiles", x, "x", at::kInt, {ANY, 3});
  check_aligned16(x, "x");
  check_aligned16(y, "y");
  check_aligned16(A, "A");
  check_aligned16(B, "B");
  LoraArgs a{};
  a.in = check_int(x.size(1), 0, INT_MAX, "x.size(1)");
  a.out = check_int(y.size(1), 0, GRID_YZ_MAX * (int64_t)LORA_NBLOCK,
                    "y.size(1)");
  a.R = (int)R;
  a.n_tiles = check_int(tiles.size(0), 0, INT_MAX / (16 * 64),
                        "tiles.size(0)");
  if (a.n_tiles == 0 || a.in == 0 || a.out == 0) return;
  const int n_split = check_int(lora_k_splits(a.in), 1, GRID_YZ_MAX,
                                "K splits of x.size(1)");
  auto part = torch::empty({n_split, (int64_t)a.n_tiles * 16, R},
                           x.options().dtype(torch::kFloat32));
  a.x = x.data_ptr();
  a.y = y.data_ptr();
  a.A = A.data_ptr();
  a.B = B.data_ptr();
  a.perm = perm.data_ptr<int32_t>();
  a.tiles = tiles.data_ptr<int32_t>();
  a.part = part.data_ptr<float>();
  CHECK_HIP(lds_lora_shrink(a, cur_stream()));
  CHECK_HIP(lds_lora_expand(a, cur_stream()));
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

// What sample() and sample_ext() share: the checks of the logits and of
// the five per-row vectors. Returns the launch arguments without outputs.
SampleArgs check_sample(const torch::Tensor& logits,
                        const torch::Tensor& temperature,
                        const torch::Tensor& top_k, const torch::Tensor& top_p,
                        const torch::Tensor& seed, const torch::Tensor& pos) {
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
  SampleArgs a{};
  a.logits = logits.data_ptr();
  a.temperature = temperature.data_ptr<float>();
  a.top_k = top_k.data_ptr<int32_t>();
  a.top_p = top_p.data_ptr<float>();
  a.seed = seed.data_ptr<int64_t>();
  a.pos = pos.data_ptr<int32_t>();
  a.B = check_int(logits.size(0), 0, INT_MAX, "logits.size(0)");
  a.V = (int)logits.size(1);
  a.is_f32 = f32 ? 1 : 0;
  return a;
}

// The four [B] outputs both samplers return, allocated and entered in `a`.
std::vector<torch::Tensor> alloc_sample_out(SampleArgs& a,
                                            const torch::Tensor& logits) {
  auto opt = logits.options();
  auto tokens = torch::empty({a.B}, opt.dtype(torch::kInt64));
  auto logprobs = torch::empty({a.B}, opt.dtype(torch::kFloat32));
  auto n_kept = torch::empty({a.B}, opt.dtype(torch::kInt32));
  auto threshold = torch::empty({a.B}, opt.dtype(torch::kFloat32));
  a.tokens = tokens.data_ptr<int64_t>();
  a.logprobs = logprobs.data_ptr<float>();
  a.n_kept = n_kept.data_ptr<int32_t>();
  a.threshold = threshold.data_ptr<float>();
  return {tokens, logprobs, n_kept, threshold};
}

std::vector<torch::Tensor> sample(torch::Tensor logits,
                                  torch::Tensor temperature,
                                  torch::Tensor top_k, torch::Tensor top_p,
                                  torch::Tensor seed, torch::Tensor pos) {
  SampleArgs a = check_sample(logits, temperature, top_k, top_p, seed, pos);
  auto out = alloc_sample_out(a, logits);
  CHECK_HIP(lds_sample(a, cur_stream()));
  return out;
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
  SampleArgs a = check_sample(logits, temperature, top_k, top_p, seed, pos);
  check_sample_param(rep, logits, at::kFloat, "rep");
  check_sample_param(pres, logits, at::kFloat, "pres");
  check_sample_param(freq, logits, at::kFloat, "freq");
  check_sample_param(min_p, logits, at::kFloat, "min_p");
  check_sample_param(top_n, logits, at::kInt, "top_n");
  check_sample_param(state_row, logits, at::kInt, "state_row");
  TORCH_CHECK(n_top >= 0 && n_top <= 20, "n_top must be in [0, 20], got ",
              n_top);
  ExtArgs ea{};
  ea.rep = rep.data_ptr<float>();
  ea.pres = pres.data_ptr<float>();
  ea.freq = freq.data_ptr<float>();
  ea.min_p = min_p.data_ptr<float>();
  ea.top_n = top_n.data_ptr<int32_t>();
  ea.state_row = state_row.data_ptr<int32_t>();
  ea.n_top = (int)n_top;
  if (state.has_value()) {
    check_token_state(*state, logits, a.V);
    ea.state = state->data_ptr<int16_t>();
    ea.R = (int)state->size(0);
    ea.Vs = state->size(1);
  }
  auto out = alloc_sample_out(a, logits);
  auto opt = logits.options();
  auto top_tokens = torch::empty({a.B, n_top}, opt.dtype(torch::kInt64));
  auto top_logprobs = torch::empty({a.B, n_top}, opt.dtype(torch::kFloat32));
  ea.top_tokens = top_tokens.data_ptr<int64_t>();
  ea.top_logprobs = top_logprobs.data_ptr<float>();
  CHECK_HIP(lds_sample_ext(a, ea, cur_stream()));
  out.push_back(top_tokens);
  out.push_back(top_logprobs);
  return out;
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
  m.def("qkv_rope_cache", &qkv_rope_cache,
        "QKV GEMM epilogue: rotated q out, rotated K and V into the pool",
        py::arg("qkv"), py::arg("cos_sin"), py::arg("positions"),
        py::arg("slot_mapping"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("n_q_heads"), py::arg("k_inv_scale") = py::none(),
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
  m.def("lora_add", &lora_add,
        "batched multi-adapter LoRA: y[perm rows] += (x A[slot]^T) B[slot]^T",
        py::arg("y"), py::arg("x"), py::arg("A"), py::arg("B"),
        py::arg("perm"), py::arg("tiles"));
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
