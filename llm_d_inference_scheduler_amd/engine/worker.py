"""Per-GPU worker engine: continuous batching over the paged KV pool.

This is the MI355X replacement for the reference's external vLLM model-server
pods (the router only steers them). One EngineWorker owns
one GPU: chunked prefill + batched decode (gfx950 paged-attention kernel),
role-aware behavior (decode | prefill | encode | combinations), and the
vLLM-compatible metrics snapshot the datalayer collectors scrape.

Decode hot loop design (MI355X-first): all per-step state — block tables,
sequence lengths, last sampled token ids — is device-resident; a step is
assembled and launched with no host→device traffic except on block-boundary
crossings and batch-membership changes, and sampled tokens are read back one
step late through a pinned buffer + event (the host never blocks the GPU on
a same-step sync). Finish decisions are made from host-side token *counts*,
so step N+1 launches before step N's token values have landed.
"""
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import ops
from ..datalayer.endpoint import Metrics, Role
from ..models.configs import ModelConfig
from ..models.llama import ForwardBatch, LlamaRunner, LoraBatch
from ..utils.logging import get_logger
from .kvcache import BLOCK_SIZE, BlockManager, KVPool, block_hashes
from .lora import LoraAdapter, LoraSlots, adapter_hash_seed

log = get_logger("engine.worker")


@dataclass
class EngineRequest:
    request_id: str
    prompt_tokens: List[int]
    max_tokens: int = 16
    temperature: float = 0.0
    is_embedding: bool = False
    prefill_only: bool = False      # disagg: stop after prefill + 1st token
    cached_tokens: int = 0          # prefix-cache reuse (engine-measured)
    priority: int = 0               # InferenceObjective priority (preemption)
    stop_token_ids: Optional[List[int]] = None  # finish_reason "stop"
    # multimodal: embeddings for the first len(prefix_embeds) prompt rows
    # (prompt_tokens must carry placeholder ids for those positions)
    prefix_embeds: "Optional[torch.Tensor]" = None
    # fused-sampler fields (DEVELOPMENT.md "Sampling"); any of them set
    # routes the steps this request takes part in through ops.sample
    top_k: int = 0                  # 0 = off
    top_p: float = 1.0              # 1.0 = off
    seed: Optional[int] = None      # None = derived from the worker's seed
    logprobs: bool = False          # return the sampled tokens' logprobs
    # ops.sample_ext fields; any of them set routes the request's steps
    # through it instead
    repetition_penalty: float = 1.0     # 1.0 = off
    presence_penalty: float = 0.0       # 0 = off
    frequency_penalty: float = 0.0      # 0 = off
    min_p: float = 0.0                  # 0 = off
    top_logprobs: int = 0               # alternatives per token, 0..20
    # name of a registered LoRA adapter, "" = the base model
    adapter: str = ""
    # runtime state
    computed: int = 0               # prompt tokens already prefilled
    generated: List[int] = field(default_factory=list)
    inflight: int = 0               # sampled on device, not yet collected
    slo_ok: bool = True             # TTFT met the SLO (goodput accounting)
    arrival_t: float = 0.0
    first_token_t: float = 0.0
    block_hashes: Optional[object] = None   # np.uint64 per full prompt block
    registered_blocks: int = 0              # hashes published so far
    _prompt_np: Optional[object] = field(default=None, repr=False)
    logprob_vals: List[float] = field(default_factory=list)
    _seed64: Optional[int] = field(default=None, repr=False)  # resolved u64
    # per generated token: [(token id, logprob)] * top_logprobs
    top_logprob_vals: List[list] = field(default_factory=list)
    # prompt length at admission: _preempt folds the generation into
    # prompt_tokens, the token state must still count it as output
    orig_prompt_len: Optional[int] = None

    def __post_init__(self):
        if not self.arrival_t:
            self.arrival_t = time.time()

    @property
    def prompt_len(self) -> int:
        return len(self.prompt_tokens)

    @property
    def token_count(self) -> int:
        """Generated + in-flight tokens (host-known without a sync)."""
        return len(self.generated) + self.inflight

    @property
    def uses_sampler(self) -> bool:
        """True when the request sets a field only the fused sampler
        implements."""
        return (self.top_k > 0 or self.top_p < 1.0 or self.seed is not None
                or self.logprobs or self.uses_ext)

    @property
    def needs_token_state(self) -> bool:
        """True when a penalty is on: the request needs a token-state row."""
        return (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0
                or self.frequency_penalty != 0.0)

    @property
    def uses_ext(self) -> bool:
        """True when the request sets a field only ops.sample_ext
        implements."""
        return (self.needs_token_state or self.min_p > 0.0
                or self.top_logprobs > 0)


@dataclass
class RequestOutput:
    request_id: str
    new_tokens: List[int]
    finished: bool = False
    finish_reason: str = "length"   # length | stop
    kind: str = "decode"            # decode | prefill_done | embedding
    # prefill_done payload (disagg hand-off):
    kv_blocks: Optional[List[int]] = None
    seq_len: int = 0
    first_token: int = 0
    # embedding payload:
    embedding: Optional[torch.Tensor] = None
    all_tokens: Optional[List[int]] = None  # full generation, on finish
    # logprobs=True requests: one value per entry of new_tokens, and the
    # whole generation's on finish
    new_logprobs: Optional[List[float]] = None
    all_logprobs: Optional[List[float]] = None
    # top_logprobs > 0 requests: per token, the [(token id, logprob)] of the
    # best raw logits, best first
    new_top_logprobs: Optional[List[list]] = None
    all_top_logprobs: Optional[List[list]] = None
    # usage on finish:
    prompt_tokens: int = 0
    completion_tokens: int = 0
    cached_tokens: int = 0
    ttft_ms: Optional[float] = None
    tpot_ms: Optional[float] = None
    e2e_ms: Optional[float] = None
    error: str = ""                 # terminal engine-side failure


_U64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(x: int) -> int:
    """One splitmix64 output for state x (u64 in, u64 out)."""
    z = (x + 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def _as_i64(u: int) -> int:
    """The int64 holding the bits of u64 u (sampler seeds travel as i64)."""
    u &= _U64
    return u - (1 << 64) if u >> 63 else u


class DecodeState:
    """Device-resident decode batch state (grows on demand)."""

    def __init__(self, capacity: int, max_blocks: int, device: torch.device):
        self.device = device
        self.max_blocks = max_blocks
        self.capacity = 0
        self.bt = None
        self.seq_lens = None
        self.last_tok = None
        self.temps = None
        # fused-sampler parameters per row, written in join. pos_off is the
        # row's completion index minus its sequence length: seq_lens already
        # advances on device every step, so the index of the token being
        # sampled is seq_lens + pos_off with no further per-step state.
        self.top_k = None
        self.top_p = None
        self.seed = None
        self.pos_off = None
        # ops.sample_ext parameters per row. They hold their off values
        # except on the rows in ext_rows, which join() resets when such a
        # row goes to a request that does not use them.
        self.rep = None
        self.pres = None
        self.freq = None
        self.min_p = None
        self.top_n = None
        self.state_row = None
        self.ext_rows: set = set()
        # LoRA slot per row (host side), -1 = none; the work list of the
        # active rows is cached like rows_for's tensor
        self.lora_slot: List[int] = []
        self._lora_ids: Optional[List[str]] = None
        self._lora_batch: Optional[LoraBatch] = None
        self.free_rows: List[int] = []
        self.row_of: Dict[str, int] = {}
        self._active_ids: List[str] = []
        self._rows_t: Optional[torch.Tensor] = None
        self._grow(capacity)

    def _grow(self, new_cap: int) -> None:
        old = self.capacity
        bt = torch.zeros((new_cap, self.max_blocks), dtype=torch.int32,
                         device=self.device)
        sl = torch.zeros(new_cap, dtype=torch.int32, device=self.device)
        lt = torch.zeros(new_cap, dtype=torch.int64, device=self.device)
        tp = torch.zeros(new_cap, dtype=torch.float32, device=self.device)
        tk = torch.zeros(new_cap, dtype=torch.int32, device=self.device)
        pp = torch.ones(new_cap, dtype=torch.float32, device=self.device)
        sd = torch.zeros(new_cap, dtype=torch.int64, device=self.device)
        po = torch.zeros(new_cap, dtype=torch.int32, device=self.device)
        f32, i32 = torch.float32, torch.int32
        ext = {"rep": torch.ones(new_cap, dtype=f32, device=self.device),
               "pres": torch.zeros(new_cap, dtype=f32, device=self.device),
               "freq": torch.zeros(new_cap, dtype=f32, device=self.device),
               "min_p": torch.zeros(new_cap, dtype=f32, device=self.device),
               "top_n": torch.zeros(new_cap, dtype=i32, device=self.device),
               "state_row": torch.full((new_cap,), -1, dtype=i32,
                                       device=self.device)}
        for name, t in ext.items():
            if old:
                t[:old] = getattr(self, name)
            setattr(self, name, t)
        if old:
            bt[:old] = self.bt
            sl[:old] = self.seq_lens
            lt[:old] = self.last_tok
            tp[:old] = self.temps
            tk[:old] = self.top_k
            pp[:old] = self.top_p
            sd[:old] = self.seed
            po[:old] = self.pos_off
        self.bt, self.seq_lens, self.last_tok, self.temps = bt, sl, lt, tp
        self.top_k, self.top_p, self.seed, self.pos_off = tk, pp, sd, po
        self.free_rows.extend(range(new_cap - 1, old - 1, -1))
        self.lora_slot.extend([-1] * (new_cap - old))
        self.capacity = new_cap

    def take_row(self) -> int:
        if not self.free_rows:
            self._grow(max(8, self.capacity * 2))
        return self.free_rows.pop()

    def join(self, req: EngineRequest, table: List[int], seq_len: int,
             last_token: int, state_row: int = -1,
             lora_slot: int = -1) -> None:
        """state_row: the request's row of the token-state pool, -1 = none.
        lora_slot: the slot its adapter is resident in, -1 = base model."""
        row = self.take_row()
        self.lora_slot[row] = lora_slot
        self._lora_ids = None
        if req.uses_ext:
            self.rep[row] = req.repetition_penalty
            self.pres[row] = req.presence_penalty
            self.freq[row] = req.frequency_penalty
            self.min_p[row] = req.min_p
            self.top_n[row] = req.top_logprobs
            self.state_row[row] = state_row
            self.ext_rows.add(row)
        elif row in self.ext_rows:
            self.rep[row] = 1.0
            self.pres[row] = 0.0
            self.freq[row] = 0.0
            self.min_p[row] = 0.0
            self.top_n[row] = 0
            self.state_row[row] = -1
            self.ext_rows.discard(row)
        self.row_of[req.request_id] = row
        # any membership mutation invalidates the cached row-index tensor:
        # an identical id list can recur with different row assignments
        # after a leave/rejoin (chunked-decode continuations)
        self._active_ids = []
        self._rows_t = None
        if len(table) > self.max_blocks:
            raise RuntimeError("sequence exceeds decode-state max_blocks")
        self.bt[row, :len(table)] = torch.tensor(
            table, dtype=torch.int32).to(self.device, non_blocking=True)
        self.seq_lens[row] = seq_len
        self.last_tok[row] = last_token
        self.temps[row] = req.temperature
        if req.temperature > 0 or req.uses_sampler:
            # (a plain greedy row never reads these: the sampler's T <= 0
            # branch ignores filters, seed and position)
            self.top_k[row] = req.top_k
            self.top_p[row] = req.top_p
            self.seed[row] = _as_i64(req._seed64 or 0)
            # the next token sampled for this row has completion index
            # req.token_count, at sequence length seq_len
            self.pos_off[row] = req.token_count - seq_len

    def leave(self, request_id: str) -> None:
        row = self.row_of.pop(request_id, None)
        if row is not None:
            self.free_rows.append(row)
            self._active_ids = []
            self._rows_t = None
            self._lora_ids = None

    def rows_for(self, ids: List[str]) -> torch.Tensor:
        if ids != self._active_ids:
            self._rows_t = torch.tensor(
                [self.row_of[i] for i in ids], dtype=torch.int64,
                device=self.device)
            self._active_ids = list(ids)
        return self._rows_t

    def lora_for(self, ids: List[str]) -> Optional[LoraBatch]:
        """The LoRA work list of a decode batch over `ids`, in batch order;
        None when no row has an adapter. Rebuilt (one small H2D copy) only
        when membership changed since the last call."""
        if ids != self._lora_ids:
            row_slot = [self.lora_slot[self.row_of[i]] for i in ids]
            self._lora_batch = None
            if any(s >= 0 for s in row_slot):
                perm, tiles = ops.lora_worklist(row_slot)
                self._lora_batch = LoraBatch(
                    perm.to(self.device, non_blocking=True),
                    tiles.to(self.device, non_blocking=True))
            self._lora_ids = list(ids)
        return self._lora_batch


class TokenStatePool:
    """Token-occurrence state of the penalised requests (DEVELOPMENT.md
    "Sampling"): one int16 row of Vs columns per request, keyed by request
    id, on the device. Allocated at the first request that needs it and
    doubled on demand; the sampler itself counts each chosen token, so a
    decode step moves nothing from the host."""

    def __init__(self, vocab_size: int, device: torch.device):
        self.V = vocab_size
        self.device = device
        self.tensor: Optional[torch.Tensor] = None
        self.free_rows: List[int] = []
        self.row_of: Dict[str, int] = {}

    def take(self, request_id: str) -> int:
        row = self.row_of.get(request_id)
        if row is not None:
            return row
        if not self.free_rows:
            old = 0 if self.tensor is None else self.tensor.shape[0]
            new = max(4, old * 2)
            if old and self.device.type == "cuda":
                # rows may be in use by work queued on another stream
                torch.cuda.synchronize(self.device)
            t = ops.token_state_alloc(new, self.V, self.device)
            if old:
                t[:old] = self.tensor
            self.tensor = t
            self.free_rows.extend(range(new - 1, old - 1, -1))
        row = self.free_rows.pop()
        self.row_of[request_id] = row
        return row

    def free(self, request_id: str) -> None:
        row = self.row_of.pop(request_id, None)
        if row is not None:
            self.free_rows.append(row)

    def fill(self, reqs: List[EngineRequest]) -> None:
        """Take a row for each request that needs one and rebuild it from
        the original prompt and the output so far."""
        reqs = [r for r in reqs if r.needs_token_state]
        if not reqs:
            return
        rows = [self.take(r.request_id) for r in reqs]
        toks: List[int] = []
        offs, n_p = [0], []
        for r in reqs:
            n = r.prompt_len if r.orig_prompt_len is None \
                else r.orig_prompt_len
            toks.extend(r.prompt_tokens[:n])
            toks.extend(r.generated)
            offs.append(len(toks))
            n_p.append(n)
        dev = self.device
        ops.token_state_fill(
            self.tensor,
            torch.tensor(rows, dtype=torch.int32).to(dev, non_blocking=True),
            torch.tensor(toks, dtype=torch.int32).to(dev, non_blocking=True),
            torch.tensor(offs, dtype=torch.int64).to(dev, non_blocking=True),
            torch.tensor(n_p, dtype=torch.int32).to(dev, non_blocking=True),
            self.V)


class EngineWorker:
    def __init__(self, config: ModelConfig, device,
                 role: Role = Role.DECODE,
                 kv_blocks: Optional[int] = None,
                 kv_budget_bytes: int = 8 << 30,
                 dtype: torch.dtype = torch.bfloat16,
                 prefill_chunk_tokens: int = 8192,
                 max_decode_batch: int = 256,
                 max_model_len: int = 8192,
                 ttft_slo_ms: float = None,
                 prefix_caching: bool = True,
                 kv_cache_dtype: str = "auto",
                 prefill_min_tokens: int = 4096,
                 prefill_max_delay_ms: float = 60.0,
                 ipc_pool: bool = False,
                 overlap_streams: Optional[bool] = None,
                 seed: int = 0,
                 kv_scales: str = "none",
                 kv_scale_headroom: float = 2.0,
                 kv_calib_tokens: int = 2048,
                 max_loras: int = 0,
                 max_lora_rank: int = 16):
        """kv_scales selects the per-head scales of an fp8 KV cache
        (KVPool): "none" (unscaled direct cast), "calibrate" (run
        calibrate_kv_scales() at start-up) or the path of a scales JSON
        (KVPool.save_scales format). Calibration runs synthetic uniform
        random tokens, which are not representative of real traffic; how
        far off they are has not been measured, so a deployment with a
        calibrated checkpoint should pass its scales file. Where fp8 falls
        back to the compute dtype (non-GPU devices) kv_scales is accepted
        and ignored, and pool.scales stays None.

        max_loras adapters can be resident at once, in slot pools of rank
        max_lora_rank rounded up to a multiple of 16 (DEVELOPMENT.md "LoRA
        adapters"); with max_loras=0 nothing is allocated and no request may
        name an adapter."""
        self.cfg = config
        self.device = torch.device(device)
        self._is_cuda_dev = lambda: self.device.type == "cuda"
        self.role = role
        self.dtype = dtype
        self.prefill_chunk_tokens = prefill_chunk_tokens
        self.prefill_min_tokens = prefill_min_tokens
        self.prefill_max_delay_ms = prefill_max_delay_ms
        self.max_decode_batch = max_decode_batch
        self.max_model_len = max_model_len
        self.ttft_slo_ms = ttft_slo_ms
        cache_dtype = {"auto": dtype, "bf16": torch.bfloat16,
                       "fp8": torch.float8_e4m3fn}[kv_cache_dtype]
        if cache_dtype == torch.float8_e4m3fn and \
                self.device.type != "cuda":
            cache_dtype = dtype     # fp8 path needs the gfx950 kernels
        if kv_blocks is None:
            kv_blocks = KVPool.blocks_for_budget(
                config, kv_budget_bytes,
                dtype_bytes=cache_dtype.itemsize)
        self.pool = KVPool(config, kv_blocks, self.device, dtype,
                           cache_dtype=cache_dtype,
                           ipc_alloc=ipc_pool and self._is_cuda_dev())
        self.mgr = BlockManager(kv_blocks, self.pool.block_size,
                                prefix_caching=prefix_caching)
        self.model = LlamaRunner(config, self.device, dtype, seed=seed)
        self.seed = seed
        self.max_loras = max_loras
        self.adapters: Dict[str, LoraAdapter] = {}   # registered, on the host
        self._adapter_tensors: Dict[str, list] = {}  # as a slot holds them
        # request id -> adapter of a KV hand-off on its way here: its slot is
        # held from reserve_lora_slot until admit_transferred or abort
        self._lora_pins: Dict[str, str] = {}
        self.lora: Optional[LoraSlots] = None
        if max_loras > 0:
            self.lora = LoraSlots(config, max_loras,
                                  -(-max_lora_rank // 16) * 16, self.device,
                                  dtype)
        self._admitted = 0      # admission counter (derived sampler seeds)
        self.kv_scale_headroom = kv_scale_headroom
        self.kv_calib_tokens = kv_calib_tokens
        self.waiting: List[EngineRequest] = []
        self.running: List[EngineRequest] = []
        self._by_id: Dict[str, EngineRequest] = {}
        # rows must hold prompt + generation; add_request clamps
        # prompt + max_tokens <= max_model_len, so this bound is exact
        max_blocks = max_model_len // self.pool.block_size + 2
        self.dstate = DecodeState(min(64, max_decode_batch), max_blocks,
                                  self.device)
        import os as _os
        self._cuda = self.device.type == "cuda"
        # Prefill/decode stream overlap measured +11.8% at mixed
        # prefill/decode shapes (profiles/r02_notes.md) but wedged two
        # long open-loop runs non-deterministically (sweep r30 mono, r20
        # fc — suspect a shared-resource race between concurrent GEMMs on
        # the two streams). Tri-state: explicit True/False from the
        # constructor wins (tests force it on); the None default is
        # OFF unless LLMD_ENABLE_OVERLAP=1, until the wedge is
        # root-caused.
        if overlap_streams is None:
            self._overlap = _os.environ.get("LLMD_ENABLE_OVERLAP",
                                            "0") == "1"
        else:
            self._overlap = bool(overlap_streams)
        self._prefill_stream = None   # lazy; see step() overlap
        self._pin = None
        self._pending = None   # (reqs, event|None, n) — one-step readback lag
        self._pin_lp = None
        self._pending_lp = None   # logprobs of the pending step, if sampled
        self.tstate = TokenStatePool(config.vocab_size, self.device)
        self._pin_top = None      # (tokens i64, logprobs f32), [cap, 20]
        self._pending_top = None  # top-N of the pending step, if asked for
        self.steps = 0
        self._rejects: List[RequestOutput] = []
        self._carry: List[RequestOutput] = []   # outputs surfaced early
        self.total_generated = 0
        self.total_generated_slo = 0
        self.total_prefilled = 0
        if kv_scales not in (None, "", "none") and \
                self.pool.cache_dtype == torch.float8_e4m3fn:
            if kv_scales == "calibrate":
                self.calibrate_kv_scales()
            else:
                self.pool.load_scales(kv_scales)
            log.info("fp8 KV scales", source=kv_scales,
                     scales_id=self.pool.scales_id)

    # ---- fp8 KV scales -------------------------------------------------
    def _require_empty_pool(self, what: str) -> None:
        if self.has_work or self.mgr.tables or self.mgr.allocated_blocks:
            raise RuntimeError(
                f"{what} needs an idle engine with no KV block allocated: "
                "stored bytes mean something else under new scales")

    def _invalidate_cached_kv(self) -> None:
        # freed blocks keep their content for prefix reuse; under new
        # scales that content is stale, so forget every hash (evicted
        # events go out with the next drain_events)
        self.mgr.drop_cached()

    def set_kv_scales(self, k, v) -> None:
        """Install per-layer, per-KV-head fp8 scales: k, v are [L, KVH]
        (tensor or nested lists) or scalars applied to every head. Both
        None returns to the unscaled cache. Raises while the engine has
        work or any block is allocated."""
        self._require_empty_pool("set_kv_scales")
        if k is not None or v is not None:
            shape = (self.cfg.num_layers, self.cfg.num_kv_heads)
            k, v = (torch.as_tensor(s, dtype=torch.float32)
                    for s in (k, v))
            k = k.expand(shape) if k.dim() == 0 else k
            v = v.expand(shape) if v.dim() == 0 else v
        self.pool.set_scales(k, v)
        self._invalidate_cached_kv()

    def calibrate_kv_scales(self, seq_len: int = 512):
        """Derive power-of-two scales (scales_from_amax) from the per-head
        absolute maxima of post-RoPE K and of V over a synthetic prefill,
        and install them. Returns (k_amax, v_amax), each [L, KVH].

        ceil(kv_calib_tokens / seq_len) sequences of seq_len tokens are
        drawn uniformly over the vocabulary from torch.Generator(seed) and
        prefilled against a temporary bf16 scratch pool, never the real
        one: a saturated fp8 layer would corrupt the statistics of every
        layer after it. Runs once at start-up, in plain torch apart from
        the model's own kernels."""
        from .kvcache import scales_from_amax
        self._require_empty_pool("calibrate_kv_scales")
        if self.pool.cache_dtype != torch.float8_e4m3fn:
            raise ValueError("KV scales are only legal with an fp8 cache")
        c = self.cfg
        bs = self.pool.block_size
        seq_len = max(1, min(seq_len, self.max_model_len - 1,
                             c.max_position))
        n_seqs = max(1, -(-self.kv_calib_tokens // seq_len))
        blocks_per_seq = -(-seq_len // bs)
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        amax = torch.zeros(c.num_layers, 2, c.num_kv_heads,
                           dtype=torch.float32, device=self.device)

        def observe(li, k, v):
            amax[li, 0] = torch.maximum(
                amax[li, 0], k.float().abs().amax(dim=(0, 2)))
            amax[li, 1] = torch.maximum(
                amax[li, 1], v.float().abs().amax(dim=(0, 2)))

        # one sequence per pass against a scratch pool of exactly its size
        scratch = torch.zeros(
            (c.num_layers, 2, blocks_per_seq, c.num_kv_heads, bs,
             c.head_dim), dtype=self.dtype, device=self.device)
        table = list(range(blocks_per_seq))
        for _ in range(n_seqs):
            ids = torch.randint(0, c.vocab_size, (seq_len,), generator=gen,
                                dtype=torch.int64)
            batch = self._prefill_batch(
                ids.numpy(), np.arange(seq_len, dtype=np.int64),
                np.arange(seq_len, dtype=np.int64), [0, seq_len],
                [seq_len], [table], [(0, seq_len, 0)], [])
            self.model.forward(batch, scratch, kv_observer=observe)
        amax = amax.cpu()
        k = scales_from_amax(amax[:, 0], self.kv_scale_headroom)
        v = scales_from_amax(amax[:, 1], self.kv_scale_headroom)
        self.pool.set_scales(k, v)
        self._invalidate_cached_kv()
        return amax[:, 0], amax[:, 1]

    # ---- LoRA adapters -------------------------------------------------
    def _adapter_users(self) -> List[str]:
        """Adapters a slot reload would pull from under: those of running
        requests (a pending decode step's requests are among them) and of
        waiting requests whose prefill has begun."""
        return [r.adapter for r in self.running if r.adapter] + \
               [r.adapter for r in self.waiting
                if r.adapter and r.request_id in self.mgr.tables] + \
               list(self._lora_pins.values())

    def reserve_lora_slot(self, request_id: str, adapter: str) -> bool:
        """Make `adapter` resident for a request that will arrive through
        admit_transferred, and hold its slot until then (or until abort /
        release_lora_slot). False when the adapter is not registered or every
        slot is in use by others; nothing is held then. True for ""."""
        if not adapter:
            return True
        if adapter not in self.adapters or \
                self._lora_slot_for(adapter) is None:
            return False
        self._lora_pins[request_id] = adapter
        return True

    def release_lora_slot(self, request_id: str) -> None:
        self._lora_pins.pop(request_id, None)

    def register_adapter(self, adapter: LoraAdapter) -> None:
        """Make `adapter` servable under its name. It stays on the host,
        padded and folded as a slot holds it, until a request needs it.
        Other content under a registered name raises: the prefix-cache seed
        is the name, so a silent swap would hand the new adapter KV computed
        under the old one. Unregister first."""
        if self.lora is None:
            raise RuntimeError("this worker was built with max_loras=0")
        old = self.adapters.get(adapter.name)
        if old is not None:
            if old.content_id != adapter.content_id:
                raise ValueError(f"adapter {adapter.name} is registered with "
                                 "other content; unregister it first")
            return
        self._adapter_tensors[adapter.name] = self.lora.host_tensors(adapter)
        self.adapters[adapter.name] = adapter

    def unregister_adapter(self, name: str) -> None:
        """Forget `name`. Cached KV is forgotten with it (all of it: blocks
        do not record their adapter), so a later adapter of that name never
        matches blocks computed under this one."""
        if any(r.adapter == name for r in self._by_id.values()):
            raise RuntimeError(f"adapter {name} is in use")
        if self.adapters.pop(name, None) is not None:
            self._adapter_tensors.pop(name, None)
            self.lora.drop(name)
            self._invalidate_cached_kv()

    def _lora_slot(self, req: EngineRequest) -> int:
        """The slot `req`'s adapter is resident in, loading it if need be;
        -1 for a base request, None when every slot is in use by others."""
        return self._lora_slot_for(req.adapter)

    def _lora_slot_for(self, adapter: str) -> int:
        if not adapter:
            return -1
        ls = self.lora
        if adapter in ls.slot_of:
            return ls.touch(adapter)
        slot = ls.victim(self._adapter_users())
        if slot is None:
            return None
        # The copy runs on the current stream. With the overlap on, kernels
        # of the other stream may still read the slot's old content and will
        # read the new: order the copy against both.
        other = None
        if self._cuda and self._prefill_stream is not None:
            cur = torch.cuda.current_stream(self.device)
            other = self._prefill_stream
            if cur == other:
                other = torch.cuda.default_stream(self.device)
            cur.wait_stream(other)
        ls.load(slot, adapter, self._adapter_tensors[adapter])
        if other is not None:
            other.wait_stream(torch.cuda.current_stream(self.device))
        return slot

    def _hash_prompt(self, req: EngineRequest) -> None:
        if req.block_hashes is None:
            req.block_hashes = block_hashes(
                req.prompt_tokens, self.pool.block_size,
                adapter_hash_seed(req.adapter))

    # ------------------------------------------------------------------
    def _reject(self, req: EngineRequest, error: str) -> None:
        self._rejects.append(RequestOutput(
            request_id=req.request_id, new_tokens=[], finished=True,
            finish_reason="error", prompt_tokens=len(req.prompt_tokens),
            error=error))

    def add_request(self, req: EngineRequest) -> None:
        if not req.prompt_tokens:
            # an empty prompt would be silently dropped in _prefill_pass
            # (remaining <= 0) and the client would hang until timeout
            self._reject(req, "empty_prompt: prompt tokenized to 0 tokens")
            return
        if req.adapter and req.adapter not in self.adapters:
            self._reject(req, f"adapter_not_found: {req.adapter}")
            return
        if len(req.prompt_tokens) >= self.max_model_len:
            # reject, never truncate: a silently-truncated prompt produces
            # a generation the caller cannot interpret (vLLM analog:
            # context_length_exceeded)
            self._reject(
                req, f"context_length_exceeded: prompt "
                     f"{len(req.prompt_tokens)} >= max_model_len "
                     f"{self.max_model_len}")
            return
        if any(t >= self.cfg.vocab_size or t < 0
               for t in req.prompt_tokens):
            # defensive clamp: a mismatched tokenizer must not crash the
            # engine loop (ids fold into the vocab deterministically)
            req.prompt_tokens = [t % self.cfg.vocab_size
                                 for t in req.prompt_tokens]
        capacity = self.pool.num_blocks * self.pool.block_size
        if len(req.prompt_tokens) >= capacity:
            # the prompt alone can never fit: reject instead of the
            # infinite preempt/recompute loop the engine-lifecycle fuzz
            # found (vLLM analog: scheduler watermark rejection)
            self._reject(
                req, f"kv_capacity_exceeded: prompt "
                     f"{len(req.prompt_tokens)} >= pool {capacity} tokens")
            return
        # generation ceiling: both the KV pool AND the model context window
        # (positions past max_model_len walk off the RoPE table and past
        # DecodeState's block-table width)
        ceiling = min(capacity, self.max_model_len)
        if len(req.prompt_tokens) + req.max_tokens > ceiling:
            clamped = ceiling - len(req.prompt_tokens)
            log.warning("max_tokens clamped to capacity",
                        req=req.request_id, requested=req.max_tokens,
                        clamped=clamped)
            req.max_tokens = clamped
        self._resolve_seed(req)
        if req.orig_prompt_len is None:
            req.orig_prompt_len = len(req.prompt_tokens)
        self.waiting.append(req)
        self._by_id[req.request_id] = req

    def _resolve_seed(self, req: EngineRequest) -> None:
        """The u64 Philox key of a request: its own seed, else one derived
        from the worker's seed and the admission counter, so a worker fed
        the same requests in the same order repeats its draws."""
        if req._seed64 is None:
            if req.seed is not None:
                req._seed64 = int(req.seed) & _U64
            else:
                req._seed64 = _splitmix64(
                    _splitmix64(self.seed & _U64) ^ self._admitted)
        self._admitted += 1

    def admit_transferred(self, req: EngineRequest, local_blocks: List[int],
                          seq_len: int, first_token: int,
                          first_logprob: Optional[float] = None,
                          first_top_logprobs: Optional[list] = None) -> None:
        """Adopt a prefilled sequence whose KV arrived over xGMI. The
        adopted full blocks are registered in the prefix cache: a
        transferred prefix is as reusable as a locally-computed one.
        first_logprob is the first token's logprob from the prefill side,
        for a logprobs=True request, first_top_logprobs its top-N list. A
        penalised request's token state is rebuilt here from the prompt and
        the first token, which counts as output."""
        if req.adapter and req.adapter not in self.adapters:
            raise RuntimeError(f"adapter_not_found: {req.adapter}")
        # a caller that moves KV here reserves the slot first
        # (reserve_lora_slot), so this finds the adapter resident
        lora_slot = self._lora_slot(req)
        if lora_slot is None:
            raise RuntimeError("no LoRA slot free for a transferred request: "
                               "reserve_lora_slot() before the transfer")
        self.mgr.adopt(req.request_id, local_blocks, seq_len)
        self._hash_prompt(req)
        full = min(len(local_blocks), req.prompt_len // self.pool.block_size)
        for b in range(full):
            self.mgr.register_block(req.request_id, b,
                                    int(req.block_hashes[b]))
        self._resolve_seed(req)
        req.computed = req.prompt_len
        req.generated = [first_token]
        req.logprob_vals = [] if first_logprob is None else [first_logprob]
        req.top_logprob_vals = [] if first_top_logprobs is None \
            else [[tuple(e) for e in first_top_logprobs]]
        if req.orig_prompt_len is None:
            req.orig_prompt_len = req.prompt_len
        if not req.first_token_t:
            req.first_token_t = time.time()
        if self.ttft_slo_ms is not None and req.arrival_t and \
                (req.first_token_t - req.arrival_t) * 1e3 > self.ttft_slo_ms:
            req.slo_ok = False
        self._by_id[req.request_id] = req
        self.running.append(req)
        self._lora_pins.pop(req.request_id, None)   # running holds it now
        self.tstate.fill([req])
        self.dstate.join(req, local_blocks, seq_len, first_token,
                         self.tstate.row_of.get(req.request_id, -1),
                         lora_slot)

    def abort(self, request_id: str) -> None:
        self._lora_pins.pop(request_id, None)
        req = self._by_id.pop(request_id, None)
        if req is None:
            return
        if req in self.waiting:
            self.waiting.remove(req)
        if req in self.running:
            self.running.remove(req)
        self.dstate.leave(request_id)
        self.tstate.free(request_id)
        self.mgr.free(request_id)

    # ------------------------------------------------------------------
    def metrics_snapshot(self) -> Metrics:
        def by_adapter(reqs):
            counts: Dict[str, int] = {}
            for r in reqs:
                if r.adapter:
                    counts[r.adapter] = counts.get(r.adapter, 0) + 1
            return counts
        return Metrics(
            waiting_queue_size=len(self.waiting),
            running_requests_size=len(self.running),
            kv_cache_usage=self.mgr.usage,
            cache_block_size=self.pool.block_size,
            cache_num_blocks=self.pool.num_blocks,
            active_models=by_adapter(self.running),
            waiting_models=by_adapter(self.waiting),
            max_active_models=self.max_loras,
        )

    @property
    def has_work(self) -> bool:
        return bool(self.waiting or self.running or self._pending
                    or self._rejects)

    # ------------------------------------------------------------------
    def step(self) -> List[RequestOutput]:
        """One engine iteration: a chunked-prefill pass (if any waiting) and
        one decode pass over the running batch. Decode token values surface
        one step late (pipelined readback)."""
        outputs: List[RequestOutput] = []
        if self._rejects:
            outputs.extend(self._rejects)
            self._rejects = []
        if self._carry:
            outputs.extend(self._carry)
            self._carry = []
        do_prefill = bool(self.waiting) and self._should_prefill()
        if self._cuda and self._overlap and do_prefill and self.running:
            # Overlap the two passes: decode (HBM-bound paged attention +
            # skinny GEMMs) launches first on the default stream; prefill
            # (MFMA-bound flash attention + fat GEMMs) runs concurrently
            # on its own stream. Safe because the passes touch DISJOINT
            # sequences and KV blocks (freed blocks re-enter the pool only
            # after their final reader's event synchronized, and cached
            # prefix blocks are immutable), and weights are read-only.
            # No ps.wait_stream(default) on entry — that would serialize
            # the two passes and defeat the overlap.
            outputs.extend(self._decode_pass())
            if self._prefill_stream is None:
                self._prefill_stream = torch.cuda.Stream(self.device)
            ps = self._prefill_stream
            with torch.cuda.stream(ps):
                outputs.extend(self._prefill_pass())
            # _prefill_pass host-syncs ps for first-token sampling, but
            # dstate.join() enqueues block-table copies on ps AFTER that
            # sync point: the next step's decode (default stream) must
            # observe them
            torch.cuda.current_stream(self.device).wait_stream(ps)
        else:
            if do_prefill:
                outputs.extend(self._prefill_pass())
            if self.running:
                outputs.extend(self._decode_pass())
            elif self._pending is not None:
                outputs.extend(self._collect_pending())
        self.steps += 1
        return outputs

    def _should_prefill(self) -> bool:
        """Batch prefill work: a small per-step chunk (one trickling
        arrival) launches a half-empty grid every layer; accumulating
        arrivals to `prefill_min_tokens` fills the chip and amortizes the
        pass, bounded by `prefill_max_delay_ms` of added TTFT."""
        if not self.running:
            return True                    # decode idle (or prefill role)
        if self.waiting[0].computed > 0:
            return True                    # finish a split chunk promptly
        pending = sum(r.prompt_len - r.computed for r in self.waiting)
        if pending >= self.prefill_min_tokens:
            return True
        oldest = self.waiting[0].arrival_t
        return oldest > 0 and \
            (time.time() - oldest) * 1e3 >= self.prefill_max_delay_ms

    # ---- prefill ----
    def _admit_prompt(self, req: EngineRequest) -> None:
        """First touch: match + reuse cached prefix blocks (engine APC)."""
        self._hash_prompt(req)
        matched = self.mgr.allocate_prompt(req.request_id, req.block_hashes,
                                           req.prompt_len)
        req.computed = matched
        req.cached_tokens = matched
        req.registered_blocks = matched // self.pool.block_size
        self.mgr.set_seq_len(req.request_id, matched)

    def _prefill_batch(self, input_ids, positions, slots, seq_starts,
                       ctx_lens, tables, metas, logit_rows,
                       embed_rows=(), embed_vals=(),
                       row_slot=None) -> ForwardBatch:
        """The ForwardBatch of one prefill pass from host-side arrays:
        flash-prefill metadata on the GPU path, per-sequence block tables
        for the composed path otherwise."""
        qpg = self.cfg.num_heads // self.cfg.num_kv_heads
        flash_ok = (self._cuda and self.cfg.head_dim == 128
                    and qpg in (1, 2, 4, 8)
                    and self.dtype == torch.bfloat16)
        prefill_bt = prefill_meta = prefill_tiles = None
        bt_list = None
        if flash_ok:
            maxb = max(len(t) for t in tables)
            bt_np = np.zeros((len(tables), maxb), dtype=np.int32)
            for i, t in enumerate(tables):
                bt_np[i, :len(t)] = t
            prefill_bt = torch.from_numpy(bt_np).to(self.device,
                                                    non_blocking=True)
            prefill_meta = torch.tensor(metas, dtype=torch.int32).to(
                self.device, non_blocking=True)
            tl = [(i, v0) for i, (_, chunk, _) in enumerate(metas)
                  for v0 in range(0, chunk * qpg, 128)]
            prefill_tiles = torch.tensor(tl, dtype=torch.int32).to(
                self.device, non_blocking=True)
        else:
            bt_list = [torch.tensor(t, dtype=torch.int32,
                                    device=self.device) for t in tables]
        lora = None
        if row_slot is not None:
            perm, tiles = ops.lora_worklist(row_slot)
            lora = LoraBatch(perm.to(self.device, non_blocking=True),
                             tiles.to(self.device, non_blocking=True))
        batch = ForwardBatch(
            lora=lora,
            input_ids=torch.from_numpy(input_ids).to(self.device,
                                                     non_blocking=True),
            positions=torch.from_numpy(
                positions.astype(np.int32)).to(self.device,
                                               non_blocking=True),
            slot_mapping=torch.from_numpy(slots).to(self.device,
                                                    non_blocking=True),
            is_decode=False, seq_starts=seq_starts, ctx_lens=ctx_lens,
            prefill_block_tables=bt_list,
            prefill_bt=prefill_bt, prefill_meta=prefill_meta,
            prefill_tiles=prefill_tiles,
            logit_rows=torch.tensor(logit_rows, dtype=torch.int64,
                                    device=self.device)
            if logit_rows else torch.zeros(0, dtype=torch.int64,
                                           device=self.device),
            embed_rows=torch.tensor(list(embed_rows), dtype=torch.int64,
                                    device=self.device)
            if embed_rows else None,
            embed_values=torch.cat(list(embed_vals)).to(self.device)
            if embed_vals else None)
        return batch

    def _prefill_pass(self) -> List[RequestOutput]:
        budget = self.prefill_chunk_tokens
        selected: List[tuple] = []
        # priority-ordered admission (stable within a priority class):
        # a preempted victim must not re-grab blocks freed FOR a
        # higher-priority waiter
        for req in sorted(self.waiting, key=lambda r: -r.priority):
            if budget <= 0:
                break
            if req.request_id not in self.mgr.tables:
                if self._lora_slot(req) is None:
                    # every slot is held by requests in flight: the request
                    # waits, later ones may pass it
                    continue
                self._admit_prompt(req)
            remaining = req.prompt_len - req.computed
            if remaining <= 0:
                self.waiting.remove(req)
                continue
            chunk = min(remaining, budget)
            if not self.mgr.can_allocate(req.computed + chunk,
                                         req.request_id) and not selected:
                # cannot even fit one: a higher-priority arrival preempts
                # the lowest-priority running request NOW instead of
                # stalling until full KV exhaustion (InferenceObjective
                # priority semantics; round-1 notes refinement)
                self._maybe_preempt_for(req)
                break
            if not self.mgr.allocate(req.request_id, req.computed + chunk):
                break
            selected.append((req, chunk))
            budget -= chunk
        if not selected:
            return []

        ids_np, pos_np, slots_np = [], [], []
        seq_starts, ctx_lens, tables, logit_rows = [0], [], [], []
        embed_rows, embed_vals = [], []
        finishing: List[EngineRequest] = []
        bs = self.pool.block_size
        metas = []                      # (seq_start, chunk, prior) per seq
        row_slot = None
        if any(req.adapter for req, _ in selected):
            row_slot = np.concatenate([
                np.full(chunk, self._lora_slot(req), dtype=np.int32)
                for req, chunk in selected])
        for req, chunk in selected:
            start, end = req.computed, req.computed + chunk
            metas.append((seq_starts[-1], chunk, start))
            if req.prefix_embeds is not None and start < req.prefix_embeds.shape[0]:
                e_end = min(end, req.prefix_embeds.shape[0])
                base_row = seq_starts[-1] + 0
                embed_rows.extend(range(base_row, base_row + (e_end - start)))
                embed_vals.append(req.prefix_embeds[start:e_end])
            # vectorized assembly (a per-token python loop here was ~ms per
            # 4k-token pass and left the GPU idle at steady state)
            if req._prompt_np is None or len(req._prompt_np) != req.prompt_len:
                req._prompt_np = np.asarray(req.prompt_tokens, dtype=np.int64)
            ids_np.append(req._prompt_np[start:end])
            p = np.arange(start, end, dtype=np.int64)
            pos_np.append(p)
            table_np = np.asarray(self.mgr.tables[req.request_id],
                                  dtype=np.int64)
            slots_np.append(table_np[p // bs] * bs + p % bs)
            self.mgr.set_seq_len(req.request_id, end)
            ctx_lens.append(end)
            tables.append(self.mgr.tables[req.request_id])
            seq_starts.append(seq_starts[-1] + chunk)
            if end == req.prompt_len:
                logit_rows.append(seq_starts[-1] - 1)
                finishing.append(req)
            req.computed = end
            self.total_prefilled += chunk
            # publish content hashes of now-complete blocks (prefill only;
            # shared cached blocks are immutable by construction)
            full = end // bs
            for b in range(req.registered_blocks, full):
                self.mgr.register_block(req.request_id, b,
                                        int(req.block_hashes[b]))
            req.registered_blocks = max(req.registered_blocks, full)
        input_ids = np.concatenate(ids_np)
        positions = np.concatenate(pos_np)
        slots = np.concatenate(slots_np)

        batch = self._prefill_batch(input_ids, positions, slots, seq_starts,
                                    ctx_lens, tables, metas, logit_rows,
                                    embed_rows, embed_vals, row_slot)
        embedding_reqs = [r for r in finishing if r.is_embedding]
        hidden_or_logits = self.model.forward(
            batch, self.pool.tensor, embeddings_out=bool(embedding_reqs),
            kv_scales=self.pool.all_layer_scales(),
            **self._lora_kw(batch))

        outputs: List[RequestOutput] = []
        now = time.time()
        if embedding_reqs:
            # embeddings: mean-pool each finished sequence's chunk rows
            for i, (req, chunk) in enumerate(selected):
                if req not in embedding_reqs:
                    continue
                rows = hidden_or_logits[seq_starts[i]:seq_starts[i + 1]]
                emb = rows.float().mean(dim=0)
                outputs.append(RequestOutput(
                    request_id=req.request_id, new_tokens=[], finished=True,
                    kind="embedding", embedding=emb.cpu(),
                    prompt_tokens=req.prompt_len,
                    e2e_ms=(now - req.arrival_t) * 1e3))
                self.waiting.remove(req)
                self.mgr.free(req.request_id)
                self._by_id.pop(req.request_id, None)
            non_emb = [r for r in finishing if not r.is_embedding]
            if non_emb:
                # mixed batch: recompute logits for the non-embedding rows
                rows = torch.tensor(
                    [seq_starts[i + 1] - 1 for i, (r, _) in enumerate(selected)
                     if r in non_emb], dtype=torch.int64, device=self.device)
                logits = hidden_or_logits[rows] @ self.model.lm_head.t()
                self._finish_prefills(non_emb, logits, outputs)
        else:
            if finishing:
                self._finish_prefills(finishing, hidden_or_logits, outputs)
        return outputs

    def _finish_prefills(self, finishing, logits, outputs) -> None:
        lps = tops = None
        if any(r.uses_sampler for r in finishing):
            # the first token is penalised against the prompt (and, after a
            # preemption, against the output so far)
            self.tstate.fill(finishing)
            tokens, lps, tops = self._sample_first(logits, finishing)
        else:
            tokens = self._sample_host(logits,
                                       [r.temperature for r in finishing])
        now = time.time()
        for i, (req, tok) in enumerate(zip(finishing, tokens)):
            new_lp = None
            if req.logprobs and lps is not None:
                new_lp = [lps[i]]
                req.logprob_vals.append(lps[i])
            new_top = None
            if req.top_logprobs > 0 and tops is not None:
                new_top = [tops[i][:req.top_logprobs]]
                req.top_logprob_vals.append(new_top[0])
            if not req.first_token_t:     # preempted reqs keep their TTFT
                req.first_token_t = now
                if self.ttft_slo_ms is not None and req.arrival_t and \
                        (now - req.arrival_t) * 1e3 > self.ttft_slo_ms:
                    req.slo_ok = False
            self.waiting.remove(req)
            if req.prefill_only:
                outputs.append(RequestOutput(
                    request_id=req.request_id, new_tokens=[int(tok)],
                    kind="prefill_done",
                    kv_blocks=list(self.mgr.tables[req.request_id]),
                    seq_len=self.mgr.seq_lens[req.request_id],
                    first_token=int(tok), prompt_tokens=req.prompt_len,
                    cached_tokens=req.cached_tokens,
                    ttft_ms=(now - req.arrival_t) * 1e3,
                    new_logprobs=new_lp, new_top_logprobs=new_top))
                self.tstate.free(req.request_id)
                # blocks stay allocated until the transfer engine releases
                self._by_id.pop(req.request_id, None)
            else:
                req.generated.append(int(tok))
                if req.slo_ok:
                    self.total_generated_slo += 1
                self.running.append(req)
                self.dstate.join(req, self.mgr.tables[req.request_id],
                                 self.mgr.seq_lens[req.request_id], int(tok),
                                 self.tstate.row_of.get(req.request_id, -1),
                                 self._lora_slot(req))
                outputs.append(RequestOutput(
                    request_id=req.request_id, new_tokens=[int(tok)],
                    ttft_ms=(now - req.arrival_t) * 1e3,
                    cached_tokens=req.cached_tokens, new_logprobs=new_lp,
                    new_top_logprobs=new_top))
                self.total_generated += 1

    def _lora_kw(self, batch: ForwardBatch) -> dict:
        """forward()'s LoRA argument: absent on a batch without adapter rows,
        so that call is today's."""
        return {} if batch.lora is None else {"lora_weights": self.lora.pools}

    def release_prefilled(self, request_id: str) -> None:
        """Free a prefill-only sequence after its KV was shipped over xGMI."""
        self.mgr.free(request_id)

    # ---- decode ----
    def _decode_pass(self) -> List[RequestOutput]:
        """Assemble and launch step N, then collect step N-1's tokens.
        Membership and finishes are decided from host-side counts, so the
        launch never waits on token values."""
        st = self.dstate
        bs = self.pool.block_size
        active: List[EngineRequest] = []
        upd_rows: List[int] = []
        upd_idx: List[int] = []
        upd_val: List[int] = []
        done_now: List[EngineRequest] = []
        for req in self.running:
            if len(active) >= self.max_decode_batch:
                break
            if req.token_count >= req.max_tokens:
                if req.inflight == 0:
                    done_now.append(req)  # all tokens came from prefill
                continue          # else final token in flight; collect soon
            rid = req.request_id
            cur = self.mgr.seq_lens[rid]
            if cur % bs == 0 and len(self.mgr.tables[rid]) <= cur // bs:
                if not self.mgr.allocate(rid, cur + 1):
                    continue      # out of KV blocks: stall this sequence
                upd_rows.append(st.row_of[rid])
                upd_idx.append(cur // bs)
                upd_val.append(self.mgr.tables[rid][-1])
            self.mgr.set_seq_len(rid, cur + 1)
            req.inflight += 1
            active.append(req)

        finals = [self._finalize(r) for r in done_now]
        if not active:
            outs = self._collect_pending() + finals
            # KV exhaustion with every decodable sequence stalled: nothing
            # will ever free blocks — preempt the youngest running request
            # (vLLM-style recompute; the prefix cache usually resurrects
            # its just-freed blocks, so the recompute is mostly free)
            if self.running and self.mgr.free_blocks == 0:
                # victim: lowest InferenceObjective priority, youngest last
                victim = min(reversed(self.running),
                             key=lambda r: r.priority)
                po = self._preempt(victim)
                if po is not None:
                    outs.append(po)
            return outs

        if upd_rows:
            st.bt[torch.tensor(upd_rows, dtype=torch.int64, device=self.device),
                  torch.tensor(upd_idx, dtype=torch.int64, device=self.device)
                  ] = torch.tensor(upd_val, dtype=torch.int32,
                                   device=self.device)

        active_ids = [r.request_id for r in active]
        rows_t = st.rows_for(active_ids)
        lens = st.seq_lens.index_select(0, rows_t)
        new_len = lens + 1
        pos = new_len - 1                           # int32 positions
        bt_rows = st.bt.index_select(0, rows_t)
        blk = bt_rows.gather(
            1, (pos // bs).to(torch.int64).unsqueeze(1)).squeeze(1)
        slot = blk.to(torch.int64) * bs + (pos % bs).to(torch.int64)
        st.seq_lens.index_copy_(0, rows_t, new_len)
        batch = ForwardBatch(
            input_ids=st.last_tok.index_select(0, rows_t),
            positions=pos, slot_mapping=slot, is_decode=True,
            block_tables=bt_rows, seq_lens=new_len,
            max_seq_len=max(self.mgr.seq_lens[r.request_id]
                            for r in active))
        if self.lora is not None:
            batch.lora = st.lora_for(active_ids)
        logits = self.model.forward(batch, self.pool.tensor,
                                    kv_scales=self.pool.all_layer_scales(),
                                    **self._lora_kw(batch))
        lp = top = None
        if any(r.uses_ext for r in active):
            # as below, through sample_ext: it reads each row's penalties
            # from the token state and counts the chosen token into it
            sel = lambda t: t.index_select(0, rows_t)
            n_top = max(r.top_logprobs for r in active)
            tok, lp, _, _, top_t, top_l = ops.sample_ext(
                logits, sel(st.temps), sel(st.top_k), sel(st.top_p),
                sel(st.seed), lens + sel(st.pos_off), sel(st.rep),
                sel(st.pres), sel(st.freq), sel(st.min_p), sel(st.top_n),
                sel(st.state_row), self.tstate.tensor, n_top)
            if n_top:
                top = (top_t, top_l)
        elif any(r.uses_sampler for r in active):
            # the fused sampler takes the whole step: T <= 0 rows go
            # through its greedy branch; `lens` is the pre-step length
            tok, lp, _, _ = ops.sample(
                logits, st.temps.index_select(0, rows_t),
                st.top_k.index_select(0, rows_t),
                st.top_p.index_select(0, rows_t),
                st.seed.index_select(0, rows_t),
                lens + st.pos_off.index_select(0, rows_t))
        else:
            any_temp = any(r.temperature > 0 for r in active)
            tok = self._sample_device(logits, rows_t, any_temp)
        st.last_tok.index_copy_(0, rows_t, tok)

        n = tok.shape[0]
        prev = self._collect_pending()     # read N-1 BEFORE reusing buffer
        if self._cuda:
            if self._pin is None or self._pin.shape[0] < st.capacity:
                self._pin = torch.empty(st.capacity, dtype=torch.int64,
                                        pin_memory=True)
            self._pin[:n].copy_(tok, non_blocking=True)
            if lp is not None:
                # logprobs ride the same pinned read-back and event
                if self._pin_lp is None or \
                        self._pin_lp.shape[0] < st.capacity:
                    self._pin_lp = torch.empty(
                        st.capacity, dtype=torch.float32, pin_memory=True)
                self._pin_lp[:n].copy_(lp, non_blocking=True)
            if top is not None:
                # so do the top-N alternatives
                if self._pin_top is None or \
                        self._pin_top[0].shape[0] < st.capacity:
                    self._pin_top = (
                        torch.empty((st.capacity, 20), dtype=torch.int64,
                                    pin_memory=True),
                        torch.empty((st.capacity, 20), dtype=torch.float32,
                                    pin_memory=True))
                w = top[0].shape[1]
                self._pin_top[0][:n, :w].copy_(top[0], non_blocking=True)
                self._pin_top[1][:n, :w].copy_(top[1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (active, ev, n)
        else:
            self._pending = (active, None, tok)
        self._pending_lp = lp
        self._pending_top = top
        return prev + finals

    def _collect_pending(self) -> List[RequestOutput]:
        if self._pending is None:
            return []
        reqs, ev, payload = self._pending
        lp_t, self._pending_lp = self._pending_lp, None
        top_t, self._pending_top = self._pending_top, None
        self._pending = None
        lps = tops = None
        if ev is not None:
            ev.synchronize()
            vals = self._pin[:payload].tolist()
            if lp_t is not None:
                lps = self._pin_lp[:payload].tolist()
            if top_t is not None:
                w = top_t[0].shape[1]
                tops = self._top_lists(self._pin_top[0][:payload, :w],
                                       self._pin_top[1][:payload, :w])
        else:
            vals = payload.tolist()
            if lp_t is not None:
                lps = lp_t.tolist()
            if top_t is not None:
                tops = self._top_lists(*top_t)
        outputs: List[RequestOutput] = []
        now = time.time()
        for i, (req, tok) in enumerate(zip(reqs, vals)):
            if self._by_id.get(req.request_id) is not req:
                continue                      # aborted while in flight
            req.inflight -= 1
            req.generated.append(int(tok))
            if req.logprobs and lps is not None:
                req.logprob_vals.append(lps[i])
            self.total_generated += 1
            if req.slo_ok:
                self.total_generated_slo += 1
            stopped = bool(req.stop_token_ids) and \
                int(tok) in req.stop_token_ids
            finished = stopped or len(req.generated) >= req.max_tokens
            out = RequestOutput(request_id=req.request_id,
                                new_tokens=[int(tok)], finished=finished,
                                finish_reason="stop" if stopped
                                else "length")
            if req.logprobs and lps is not None:
                out.new_logprobs = [lps[i]]
            if req.top_logprobs > 0 and tops is not None:
                out.new_top_logprobs = [tops[i][:req.top_logprobs]]
                req.top_logprob_vals.append(out.new_top_logprobs[0])
            if finished:
                n_gen = len(req.generated)
                out.all_tokens = list(req.generated)
                if req.logprobs:
                    out.all_logprobs = list(req.logprob_vals)
                if req.top_logprobs > 0:
                    out.all_top_logprobs = list(req.top_logprob_vals)
                out.prompt_tokens = req.prompt_len
                out.completion_tokens = n_gen
                out.cached_tokens = req.cached_tokens
                out.ttft_ms = (req.first_token_t - req.arrival_t) * 1e3
                if n_gen > 1:
                    out.tpot_ms = (now - req.first_token_t) * 1e3 / (n_gen - 1)
                out.e2e_ms = (now - req.arrival_t) * 1e3
                self.running.remove(req)
                self.dstate.leave(req.request_id)
                self.tstate.free(req.request_id)
                self.mgr.free(req.request_id)
                self._by_id.pop(req.request_id, None)
            outputs.append(out)
        return outputs

    def _maybe_preempt_for(self, waiter: EngineRequest) -> bool:
        """Free KV for a strictly-higher-priority waiter by preempting the
        lowest-priority running request (youngest last) whose pending
        tokens are already collected. Returns True if a victim was
        preempted (its blocks free on the next step's allocation)."""
        # the pipelined decode keeps one token in flight on every running
        # request at prefill time: collect step N-1's tokens first so
        # victims become preemptible (their outputs surface via _carry)
        if any(r.inflight for r in self.running):
            self._carry.extend(self._collect_pending())
        candidates = [r for r in self.running
                      if r.inflight == 0 and r.priority < waiter.priority]
        if not candidates:
            return False
        victim = min(reversed(candidates), key=lambda r: r.priority)
        out = self._preempt(victim)
        if out is not None:
            self._rejects.append(out)   # surfaced next step()
        return True

    def _preempt(self, req: EngineRequest) -> Optional[RequestOutput]:
        """Evict a running request and requeue it for recompute: its
        generation so far folds into the prompt (prefill of prompt+generated
        produces the next token's logits, so accounting continues exactly).
        Pending tokens must be collected first (req.inflight == 0).

        If prompt+generated no longer fits the context window (can only
        happen for requests admitted before a config change — add_request
        clamps prompt+max_tokens to max_model_len), finish the request
        (finish_reason=length) instead of truncating: truncation would
        recompute KV that no longer corresponds to the retained generation
        and re-emit dropped tokens through all_tokens."""
        assert req.inflight == 0, "collect pending before preempting"
        merged = req.prompt_tokens + req.generated
        if len(merged) > self.max_model_len - 1:
            log.info("preempt would exceed context window; finishing",
                     req=req.request_id, generated=len(req.generated))
            return self._finalize(req)
        log.info("preempting for KV space", req=req.request_id,
                 generated=len(req.generated))
        self.running.remove(req)
        self.dstate.leave(req.request_id)
        self.tstate.free(req.request_id)
        self.mgr.free(req.request_id)
        req.prompt_tokens = merged
        req.computed = 0
        req.block_hashes = None
        req.registered_blocks = 0
        self.waiting.insert(0, req)
        return None

    def _finalize(self, req: EngineRequest) -> RequestOutput:
        """Emit the finished output for a request with no in-flight token
        (its full generation came from prefill, e.g. max_tokens=1)."""
        now = time.time()
        n_gen = len(req.generated)
        out = RequestOutput(
            request_id=req.request_id, new_tokens=[], finished=True,
            all_tokens=list(req.generated), prompt_tokens=req.prompt_len,
            completion_tokens=n_gen, cached_tokens=req.cached_tokens,
            ttft_ms=(req.first_token_t - req.arrival_t) * 1e3,
            e2e_ms=(now - req.arrival_t) * 1e3)
        if req.logprobs:
            out.all_logprobs = list(req.logprob_vals)
        if req.top_logprobs > 0:
            out.all_top_logprobs = list(req.top_logprob_vals)
        if n_gen > 1:
            out.tpot_ms = (now - req.first_token_t) * 1e3 / (n_gen - 1)
        self.running.remove(req)
        self.dstate.leave(req.request_id)
        self.tstate.free(req.request_id)
        self.mgr.free(req.request_id)
        self._by_id.pop(req.request_id, None)
        return out

    # ---- sampling ----
    def _sample_device(self, logits: torch.Tensor, rows_t: torch.Tensor,
                       any_temp: bool) -> torch.Tensor:
        """Greedy argmax, or gumbel-max for temperature>0 rows — entirely on
        device (no host sync)."""
        if not any_temp:
            return logits.argmax(dim=-1)
        temps = self.dstate.temps.index_select(0, rows_t)
        hot = temps > 0
        inv = torch.where(hot, 1.0 / temps.clamp(min=1e-6),
                          torch.ones_like(temps))
        y = logits.float() * inv.unsqueeze(1)
        u = torch.rand_like(y).clamp_min(1e-20)
        gumbel = -torch.log(-torch.log(u).clamp_min(1e-20))
        y = y + gumbel * hot.unsqueeze(1)
        return y.argmax(dim=-1)

    def _sample_first(self, logits: torch.Tensor,
                      reqs: List[EngineRequest]):
        """First-token sampling through the fused sampler, on the logits
        where they live: (tokens, logprobs, top-N lists or None) as host
        lists. The token's completion index is len(req.generated): 0, or
        where a preempted request left off. With a request that sets a
        sample_ext field the call goes through ops.sample_ext, the token
        state rows having been filled by the caller."""
        dev = logits.device
        f32, i32 = torch.float32, torch.int32
        col = lambda f, dt: torch.tensor([f(r) for r in reqs], dtype=dt,
                                         device=dev)
        base = (logits,
                col(lambda r: r.temperature, f32),
                col(lambda r: r.top_k, i32),
                col(lambda r: r.top_p, f32),
                col(lambda r: _as_i64(r._seed64), torch.int64),
                col(lambda r: len(r.generated), i32))
        if not any(r.uses_ext for r in reqs):
            tok, lp, _, _ = ops.sample(*base)
            return tok.tolist(), lp.tolist(), None
        n_top = max(r.top_logprobs for r in reqs)
        tok, lp, _, _, top_t, top_l = ops.sample_ext(
            *base,
            col(lambda r: r.repetition_penalty, f32),
            col(lambda r: r.presence_penalty, f32),
            col(lambda r: r.frequency_penalty, f32),
            col(lambda r: r.min_p, f32),
            col(lambda r: r.top_logprobs, i32),
            col(lambda r: self.tstate.row_of.get(r.request_id, -1), i32),
            self.tstate.tensor, n_top)
        tops = self._top_lists(top_t, top_l) if n_top else None
        return tok.tolist(), lp.tolist(), tops

    @staticmethod
    def _top_lists(top_tokens: torch.Tensor, top_logprobs: torch.Tensor):
        """[B, n] top-N outputs -> per row [(token id, logprob)], without
        the -1 entries past a row's own N."""
        return [[(t, l) for t, l in zip(tr, lr) if t >= 0]
                for tr, lr in zip(top_tokens.tolist(),
                                  top_logprobs.tolist())]

    def _sample_host(self, logits: torch.Tensor,
                     temps: List[float]) -> List[int]:
        """Prefill first-token sampling (host-visible; prefill already
        syncs for TTFT bookkeeping)."""
        if logits.numel() == 0:
            return []
        greedy = logits.argmax(dim=-1)
        if all(t <= 0 for t in temps):
            return greedy.tolist()
        out = []
        for i, t in enumerate(temps):
            if t <= 0:
                out.append(int(greedy[i]))
            else:
                p = torch.softmax(logits[i].float() / t, dim=-1)
                out.append(int(torch.multinomial(p, 1)))
        return out
