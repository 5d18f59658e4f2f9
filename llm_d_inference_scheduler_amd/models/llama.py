"""Llama-family model runner (random-init weights, paged KV, bf16).

MI355X-native execution path: plain-GEMM projections go through
hipBLASLt/rocBLAS via torch.matmul; the fused hot ops (residual+RMSNorm,
RoPE, SiLU*up, GQA paged decode attention, KV scatter) are the gfx950 HIP
kernels in csrc/hip dispatched through ops/. Prefill attention is composed
chunked torch-matmul attention over KV gathered from the paged pool (an
LDS-tiled MFMA flash kernel is the planned replacement; no Triton, no SDPA
multi-backend dispatch is used anywhere).

The reference router never runs a model — its pods do (vLLM). This runner
is the per-GPU worker engine's model, SURVEY.md §2.12 "worker shim".
"""
import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .. import ops
from ..ops import ref as ops_ref
from ..utils.logging import get_logger
from .configs import ModelConfig

log = get_logger("models.llama")

_TUNED_GEMM_LOADED = False


def _load_tuned_gemms() -> None:
    """Load offline hipBLASLt autotune results (tools/tune_gemms.py) so the
    skinny decode GEMMs use tuned solutions instead of the default pick
    (~2.6x off the weights-bound floor, profiles/r01_bench_kernel_stats_v3)."""
    global _TUNED_GEMM_LOADED
    if _TUNED_GEMM_LOADED:
        return
    _TUNED_GEMM_LOADED = True
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "..", "..", "profiles", "tuned_gemm_gfx950.csv")
    if os.environ.get("LLMD_NO_TUNED_GEMM", "0") == "1":
        # bisect knob: TunableOp is the prime suspect for the
        # multi-stream wedge (profiles/r02_notes.md)
        return
    if os.path.exists(path):
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.read_file(path)
        log.info("loaded tuned GEMM solutions", path=path)


@dataclass
class ForwardBatch:
    """One model invocation over a token-flattened batch.

    For decode: T == number of sequences, each contributing its newest token.
    For prefill: T == sum of chunk lengths; `seq_starts` delimits sequences.
    """
    input_ids: torch.Tensor          # [T] int64
    positions: torch.Tensor         # [T] int32
    slot_mapping: torch.Tensor      # [T] int64 into the paged pool
    is_decode: bool
    # decode-only:
    block_tables: Optional[torch.Tensor] = None   # [B, max_blocks] int32
    seq_lens: Optional[torch.Tensor] = None       # [B] int32 (incl. new token)
    max_seq_len: Optional[int] = None             # host-known max (no sync)
    # prefill-only:
    seq_starts: Optional[List[int]] = None        # len B+1 offsets into T
    ctx_lens: Optional[List[int]] = None          # [B] total ctx after chunk
    prefill_block_tables: Optional[List[torch.Tensor]] = None
    # fused flash-prefill metadata (GPU path; see flash_prefill.hip)
    prefill_bt: Optional[torch.Tensor] = None     # [S, max_blocks] int32
    prefill_meta: Optional[torch.Tensor] = None   # [S, 3] start,chunk,prior
    prefill_tiles: Optional[torch.Tensor] = None  # [n_tiles, 2] seq,vrow0
    logit_rows: Optional[torch.Tensor] = None     # rows needing logits
    # multimodal: rows whose input embedding is provided (encode hand-off)
    embed_rows: Optional[torch.Tensor] = None     # [n] int64 into T
    embed_values: Optional[torch.Tensor] = None   # [n, hidden]
    # LoRA work list (ops.lora_worklist) as device tensors, or None: no row
    # of this batch has an adapter
    lora: Optional["LoraBatch"] = None


@dataclass
class LoraBatch:
    perm: torch.Tensor               # int32, adapter rows grouped by slot
    tiles: torch.Tensor              # [n, 3] int32 start, count, slot


LORA_TARGETS = ("wqkv", "wo", "wgate_up", "wdown")


class LlamaRunner:
    def __init__(self, config: ModelConfig, device: torch.device,
                 dtype: torch.dtype = torch.bfloat16, seed: int = 0):
        self.cfg = config
        self.device = device
        self.dtype = dtype
        self.scale = 1.0 / math.sqrt(config.head_dim)
        # False forces the split / rope / reshape_and_cache chain (tests
        # compare the two paths)
        self._fused_qkv = True
        c = config
        if c.num_experts and self.device.type == "cuda" and \
                dtype != torch.bfloat16:
            raise ValueError("an MoE model on the GPU needs a bf16 runner")
        if self.device.type == "cuda":
            _load_tuned_gemms()
            # init directly on the GPU (16 GB of weights for Llama-3-8B —
            # CPU-side init would dominate startup). Same seed => identical
            # weights on every rank (required by the P/D KV hand-off).
            torch.cuda.manual_seed_all(seed)

            def w(*shape, std=0.02):
                t = torch.empty(*shape, dtype=torch.float32,
                                device=self.device)
                t.normal_(0.0, std)
                return t.to(dtype)
        else:
            gen = torch.Generator(device="cpu").manual_seed(seed)

            def w(*shape, std=0.02):
                t = torch.empty(*shape, dtype=torch.float32)
                t.normal_(0.0, std, generator=gen)
                return t.to(dtype).to(device)

        out_std = 0.02 / math.sqrt(2 * c.num_layers)
        self.embed = w(c.vocab_size, c.hidden_size)
        self.layers: List[Dict[str, torch.Tensor]] = []
        for _ in range(c.num_layers):
            self.layers.append({
                "input_norm": torch.ones(c.hidden_size, dtype=dtype,
                                         device=device),
                "wqkv": w(c.hidden_size, c.q_size + 2 * c.kv_size),
                "wo": w(c.q_size, c.hidden_size, std=out_std),
                "post_norm": torch.ones(c.hidden_size, dtype=dtype,
                                        device=device),
                **({"q_norm": torch.ones(c.head_dim, dtype=dtype,
                                         device=device),
                    "k_norm": torch.ones(c.head_dim, dtype=dtype,
                                         device=device)}
                   if c.qk_norm else {}),
                **({"router": w(c.num_experts, c.hidden_size),
                    "w13": w(c.num_experts, 2 * c.moe_intermediate_size,
                             c.hidden_size),
                    "w2": w(c.num_experts, c.hidden_size,
                            c.moe_intermediate_size, std=out_std)}
                   if c.num_experts else
                   {"wgate_up": w(c.hidden_size, 2 * c.intermediate_size),
                    "wdown": w(c.intermediate_size, c.hidden_size,
                               std=out_std)}),
            })
        self.final_norm = torch.ones(c.hidden_size, dtype=dtype, device=device)
        self.lm_head = self.embed if c.tie_embeddings else \
            w(c.vocab_size, c.hidden_size)
        self.cos_sin = ops_ref.rope_table(c.max_position, c.head_dim,
                                          c.rope_theta, device=device)

        # quantised weights (quantize_weights): batches of up to this many
        # rows go through ops.linear_fp8 / ops.linear_mxfp4, larger ones
        # through a dequantised bf16 copy and torch.matmul (crossovers:
        # profiles/linear_fp8.md, profiles/linear_mxfp4.md)
        # "fp8_block" pairs (a 2-D fp32 scale) go through
        # ops.linear_fp8_block at every batch size
        self.weight_dtype = "bf16"
        self.expert_dtype = "bf16"     # w13 and w2 (quantize_experts)
        self._fp8_kernel_max_t = 128
        self._mxfp4_kernel_max_t = 128
        # "fp8" (set_activation_dtype): fp8 pairs at batches above
        # _fp8_kernel_max_t go through ops.linear_fp8_a8 instead, and the
        # bf16 scratch below is never allocated
        self.activation_dtype = "bf16"
        self._fp8_scratch: Dict[int, torch.Tensor] = {}
        # ops.moe_ffn / moe_ffn_mxfp4 / moe_ffn_fp8 / moe_ffn_fp8_a8 /
        # moe_ffn_fp8_block scratch, one per stream, sized by the largest T
        # seen
        self._moe_scratch: Dict[int, torch.Tensor] = {}
        # "fp8" (set_expert_activation_dtype): fp8 experts at batches of
        # more than _moe_a8_min_rows mean rows per expert (T k / E) go
        # through ops.moe_ffn_fp8_a8, the others through ops.moe_ffn_fp8. 8
        # is the measured crossover on a Qwen3-30B-A3B layer: at 8 rows an
        # expert the two ops tie (0.99x), at 16 moe_ffn_fp8_a8 leads 1.15x
        # (profiles/moe_fp8_a8.md)
        self.expert_activation_dtype = "bf16"
        self._moe_a8_min_rows = 8
        # "fp8_block128" experts (a 3-D fp32 scale) go through
        # ops.moe_ffn_fp8_block at every batch size

    def weight_bytes(self) -> int:
        tensors = [self.embed, self.lm_head, self.final_norm]
        for layer in self.layers:
            for w in layer.values():
                tensors.extend(w if isinstance(w, tuple) else (w,))
        return sum(t.numel() * t.element_size() for t in tensors)

    # ---- quantised weights (DEVELOPMENT.md "fp8 weights", "MXFP4 weights")
    def quantize_weights(self, weight_dtype: str,
                         experts: bool = True) -> None:
        """Convert the four projections of every layer in place to a
        weight-only format. "fp8": layer[name] becomes the pair (wq
        [out, in] float8_e4m3fn, scale [out] fp32) of
        ops.ref.quantize_weight_fp8. "fp8_block": the pair (wq [out, in]
        float8_e4m3fn, scale [ceil(out / 128), ceil(in / 128)] fp32) of
        ops.ref.quantize_weight_fp8_block, told apart from "fp8" by its 2-D
        scale; it is multiplied with fp8 activations at every batch size
        (DEVELOPMENT.md "fp8 block scales"). "mxfp4": the pair (wq
        [out, in / 2] uint8, scale [out, in / 32] uint8) of
        ops.ref.quantize_weight_mxfp4, told apart by wq's dtype. Layer by
        layer, each bf16
        tensor dropped as it is converted. The embedding, lm_head and the
        norms keep the runner's dtype. A quantised runner cannot be
        converted to another format: the bf16 weights are gone.
        On an MoE model the experts go with the projections, and "mxfp4" is
        the only format this takes: wqkv and wo as above, w13 and w2 as
        quantize_experts("mxfp4") leaves them, and the router keeps the
        runner's dtype. experts=False converts wqkv and wo alone, in either
        format, and leaves the experts to quantize_experts."""
        if weight_dtype in ("auto", "bf16"):
            return
        if weight_dtype not in ("fp8", "fp8_block", "mxfp4"):
            raise ValueError(f"unknown weight_dtype {weight_dtype!r}")
        experts = experts and bool(self.cfg.num_experts)
        if experts and weight_dtype == "fp8_block":
            raise ValueError(
                'weight_dtype "fp8_block" alone is not supported for an MoE '
                'model: pass expert_dtype "fp8_block128" for block-scaled '
                'experts (or "bf16", "fp8" or "mxfp4") and fp8_block covers '
                "wqkv and wo")
        if experts and weight_dtype != "mxfp4":
            raise ValueError(
                f"weight_dtype {weight_dtype!r} alone is not supported for an "
                f"MoE model: pass expert_dtype={weight_dtype!r} to quantise "
                "its experts as well")
        if experts:
            self._check_expert_dtype(weight_dtype, self.weight_dtype)
        if self.weight_dtype == weight_dtype:
            return
        if self.weight_dtype != "bf16":
            raise ValueError(f"weights are already {self.weight_dtype}, "
                             f"cannot convert them to {weight_dtype}")
        if self.device.type == "cuda" and self.dtype != torch.bfloat16:
            raise ValueError(f"{weight_dtype} weights on the GPU need a bf16 "
                             "runner")
        quantize = {"fp8": ops_ref.quantize_weight_fp8,
                    "fp8_block": ops_ref.quantize_weight_fp8_block,
                    "mxfp4": ops_ref.quantize_weight_mxfp4}[weight_dtype]
        for layer in self.layers:
            for name in LORA_TARGETS:
                if name in layer:
                    layer[name] = quantize(layer[name])
        self.weight_dtype = weight_dtype
        if experts:
            self.quantize_experts(weight_dtype)

    def set_activation_dtype(self, activation_dtype: str) -> None:
        """With "fp8" (DEVELOPMENT.md "fp8 activations") batches of more than
        _fp8_kernel_max_t rows are quantised per row to e4m3 with a dynamic
        scale and multiplied by the fp8 weights on the fp8 MFMA
        (ops.linear_fp8_a8) instead of going through a dequantised bf16 copy
        and torch.matmul. Needs quantize_weights("fp8") first. Smaller
        batches keep the weight-only kernel, so the quantisation a row sees
        depends on the size of the batch it ran in. The experts of an MoE
        model are untouched: set_expert_activation_dtype is their option.
        "auto" and "bf16" change nothing. "fp8_block" weights are a W8A8
        format by definition: "auto" and "fp8" change nothing there, and
        "bf16" is a ValueError."""
        if activation_dtype not in ("auto", "bf16", "fp8"):
            raise ValueError(f"unknown activation_dtype {activation_dtype!r}")
        if self.weight_dtype == "fp8_block":
            if activation_dtype == "bf16":
                raise ValueError(
                    'activation_dtype "bf16" is not available with '
                    'weight_dtype "fp8_block": the format is defined with '
                    "fp8 activations, one scale per token and 128-wide "
                    "group, and no kernel multiplies its weights by bf16 "
                    "rows")
            return
        if activation_dtype != "fp8":
            return
        if self.weight_dtype != "fp8":
            raise ValueError(
                'activation_dtype "fp8" needs weight_dtype "fp8", the '
                f"weights are {self.weight_dtype}")
        self.activation_dtype = "fp8"

    def set_expert_activation_dtype(self, expert_activation_dtype: str) -> None:
        """With "fp8" (DEVELOPMENT.md "Mixture of experts") batches of more
        than _moe_a8_min_rows mean rows per expert run the fp8 experts with
        fp8 activations: x and silu(g) * u are quantised per row to e4m3 with
        a dynamic scale and both expert GEMMs run on the fp8 MFMA
        (ops.moe_ffn_fp8_a8). Needs quantize_experts("fp8") first, and
        hidden_size and moe_intermediate_size multiples of 64. Smaller
        batches keep ops.moe_ffn_fp8, so the quantisation a row sees depends
        on the size of the batch it ran in. "auto" and "bf16" change
        nothing. "fp8_block128" experts are a W8A8 format by definition:
        "auto" and "fp8" change nothing there, and "bf16" is a ValueError."""
        if expert_activation_dtype not in ("auto", "bf16", "fp8"):
            raise ValueError("unknown expert_activation_dtype "
                             f"{expert_activation_dtype!r}")
        if self.expert_dtype == "fp8_block128":
            if expert_activation_dtype == "bf16":
                raise ValueError(
                    'expert_activation_dtype "bf16" is not available with '
                    'expert_dtype "fp8_block128": the format is defined '
                    "with fp8 activations, one scale per row and 128-wide "
                    "group, and no kernel multiplies its experts by bf16 "
                    "rows")
            return
        if expert_activation_dtype != "fp8":
            return
        if self.expert_dtype != "fp8":
            raise ValueError(
                'expert_activation_dtype "fp8" needs expert_dtype "fp8", the '
                f"experts are {self.expert_dtype}")
        c = self.cfg
        if c.hidden_size % 64 or c.moe_intermediate_size % 64:
            raise ValueError(
                'expert_activation_dtype "fp8" needs hidden_size and '
                "moe_intermediate_size to be multiples of 64, got "
                f"{c.hidden_size} and {c.moe_intermediate_size}")
        self.expert_activation_dtype = "fp8"

    def _check_expert_dtype(self, expert_dtype: str, allowed: str) -> None:
        """ValueError unless the experts can become expert_dtype: an MoE model
        whose experts are still bf16 (or, from quantize_weights on a runner
        it has converted before, already `allowed`)."""
        c = self.cfg
        if expert_dtype not in ("fp8", "fp8_block128", "mxfp4"):
            raise ValueError(f"unknown expert_dtype {expert_dtype!r}")
        if not c.num_experts:
            raise ValueError("expert_dtype needs an MoE model: a dense model "
                             "has no experts")
        if self.expert_dtype not in ("bf16", allowed):
            raise ValueError(f"experts are already {self.expert_dtype}, "
                             f"cannot convert them to {expert_dtype}")
        if self.device.type == "cuda" and self.dtype != torch.bfloat16:
            raise ValueError(f"{expert_dtype} experts on the GPU need a bf16 "
                             "runner")
        if expert_dtype == "mxfp4" and (c.hidden_size % 32 or
                                        c.moe_intermediate_size % 32):
            raise ValueError(
                "mxfp4 experts need hidden_size and moe_intermediate_size to "
                f"be multiples of 32, got {c.hidden_size} and "
                f"{c.moe_intermediate_size}")
        if expert_dtype == "fp8_block128" and (c.hidden_size % 64 or
                                               c.moe_intermediate_size % 64):
            raise ValueError(
                "fp8_block128 experts need hidden_size and "
                "moe_intermediate_size to be multiples of 64, got "
                f"{c.hidden_size} and {c.moe_intermediate_size}")

    def quantize_experts(self, expert_dtype: str) -> None:
        """Convert w13 and w2 of every layer in place, expert by expert, each
        bf16 tensor dropped as it is converted. "fp8": the pairs (w13q
        [E, 2 I, H] float8_e4m3fn, w13s [E, 2 I] fp32) and (w2q [E, H, I],
        w2s [E, H]) of ops.ref.quantize_experts_fp8, legal for every MoE
        config. "mxfp4": (w13q [E, 2 I, H / 2], w13s [E, 2 I, H / 32]) and
        (w2q [E, H, I / 2], w2s [E, H, I / 32]), all uint8;
        hidden_size and moe_intermediate_size must be multiples of 32, the
        MX group. "fp8_block128" (DEVELOPMENT.md "Mixture of experts"): the
        block-scaled pairs of ops.ref.quantize_experts_fp8_block, (w13q
        [E, 2 I, H], w13s [E, 2 ceil(I / 128), ceil(H / 128)] fp32) with the
        gate and the up rows blocked apart, and (w2q [E, H, I], w2s
        [E, ceil(H / 128), ceil(I / 128)]), told apart from "fp8" by their
        3-D scale and multiplied with fp8 activations at every batch size;
        hidden_size and moe_intermediate_size must be multiples of 64. wqkv,
        wo, the router, the embedding, lm_head and the norms
        are left alone. Experts that are already quantised cannot be
        converted again: the bf16 weights are gone."""
        self._check_expert_dtype(expert_dtype, "bf16")
        quantize = {
            "fp8": lambda W, halves: ops_ref.quantize_experts_fp8(W),
            "fp8_block128": ops_ref.quantize_experts_fp8_block,
            "mxfp4": lambda W, halves: ops_ref.quantize_experts_mxfp4(W),
        }[expert_dtype]
        for layer in self.layers:
            for name, halves in (("w13", 2), ("w2", 1)):
                layer[name] = quantize(layer[name], halves)
        self.expert_dtype = expert_dtype

    def dense_layers(self) -> List[Dict[str, torch.Tensor]]:
        """self.layers with the four projections as fp32 [in, out] tensors,
        an fp8, fp8_block or mxfp4 pair dequantised exactly: the weights the
        forward pass applies. MXFP4, fp8 and block-scaled fp8 experts come
        back as fp32 [E, out, in]."""
        def dense(w):
            if not isinstance(w, tuple):
                return w.float()
            if w[0].dtype == torch.uint8:
                return ops_ref.dequant_mxfp4_weight(*w, dtype=torch.float32)
            if w[1].dim() == 2:
                return (w[0].float() * ops_ref.expand_fp8_block_scale(
                    w[1], *w[0].shape)).t()
            return (w[0].float() * w[1][:, None]).t()
        def experts(w, halves):
            if not isinstance(w, tuple):
                return w
            if w[1].dim() == 3 and w[1].dtype == torch.float32:
                return ops_ref.dequant_experts_fp8_block(*w, halves=halves)
            return ops_ref.dequant_experts_mxfp4(*w) \
                if w[0].dtype == torch.uint8 else \
                ops_ref.dequant_experts_fp8(*w)
        return [{k: dense(w) if k in LORA_TARGETS else
                 experts(w, 2 if k == "w13" else 1) if k in ("w13", "w2")
                 else w
                 for k, w in layer.items()} for layer in self.layers]

    # ---- mixture of experts (DEVELOPMENT.md "Mixture of experts") ----
    def upcycle_to_moe(self, num_experts: int, experts_per_token: int,
                       seed: int = 0) -> None:
        """Sparse upcycling of a dense runner, in place: every layer's w13
        and w2 become num_experts copies of its transposed wgate_up and
        wdown, the router is drawn at random, and self.cfg becomes the MoE
        config with norm_topk_prob=True. With identical experts and
        renormalised weights the layer computes the dense FFN in exact
        arithmetic, whichever experts a token is routed to. Dense weights in
        the runner's dtype only."""
        if self.cfg.num_experts:
            raise ValueError("the runner is already an MoE model")
        if self.weight_dtype != "bf16":
            raise ValueError(f"cannot upcycle {self.weight_dtype} weights")
        cfg = dataclasses.replace(
            self.cfg, num_experts=num_experts,
            experts_per_token=experts_per_token,
            moe_intermediate_size=self.cfg.intermediate_size,
            norm_topk_prob=True)
        if self.device.type == "cuda" and self.dtype != torch.bfloat16:
            raise ValueError("an MoE model on the GPU needs a bf16 runner")
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for layer in self.layers:
            router = torch.empty(num_experts, cfg.hidden_size)
            router.normal_(0.0, 0.02, generator=gen)
            layer["router"] = router.to(self.dtype).to(self.device)
            w13 = layer.pop("wgate_up").t().contiguous()
            w2 = layer.pop("wdown").t().contiguous()
            layer["w13"] = w13.unsqueeze(0).repeat(num_experts, 1, 1)
            layer["w2"] = w2.unsqueeze(0).repeat(num_experts, 1, 1)
        self.cfg = cfg

    def _moe(self, x: torch.Tensor, layer) -> torch.Tensor:
        """The routed FFN of one layer. Nothing on this path waits for the
        device: routing and the work list stay there."""
        c = self.cfg
        ids, w = ops.moe_route(x, layer["router"], c.experts_per_token,
                               c.norm_topk_prob)
        # a bf16 tensor, an MXFP4 pair (uint8), an fp8 pair or a block-scaled
        # fp8 pair (a 3-D fp32 scale)
        mx = a8 = blk = False
        if not isinstance(layer["w13"], tuple):
            ffn, experts = ops.moe_ffn, (layer["w13"], layer["w2"])
        else:
            mx = layer["w13"][0].dtype == torch.uint8
            # host arithmetic on the batch size alone: no sync
            blk = not mx and layer["w13"][1].dim() == 3
            a8 = not mx and not blk and \
                self.expert_activation_dtype == "fp8" and \
                x.shape[0] * c.experts_per_token > \
                self._moe_a8_min_rows * c.num_experts
            ffn = ops.moe_ffn_mxfp4 if mx else \
                ops.moe_ffn_fp8_block if blk else \
                ops.moe_ffn_fp8_a8 if a8 else ops.moe_ffn_fp8
            experts = (*layer["w13"], *layer["w2"])
        if not x.is_cuda:
            return ffn(x, *experts, ids, w)
        key = torch.cuda.current_stream(x.device).cuda_stream
        shape = (x.shape[0], c.experts_per_token, c.num_experts,
                 c.hidden_size, c.moe_intermediate_size)
        need = ops.moe_fp8_block_scratch_bytes(*shape) if blk else \
            ops.moe_scratch_bytes(*shape, mxfp4=mx)
        if not blk and self.expert_activation_dtype == "fp8":
            # one buffer serves both ops: the larger of the two needs
            need = max(need, ops.moe_fp8_a8_scratch_bytes(*shape))
        buf = self._moe_scratch.get(key)
        if buf is None or buf.numel() < need:
            buf = self._moe_scratch[key] = torch.empty(
                need, dtype=torch.uint8, device=x.device)
        return ffn(x, *experts, ids, w, buf)

    def _linear(self, x: torch.Tensor, w) -> torch.Tensor:
        """x @ w for a projection of self.layers: dense, an fp8 pair, an
        fp8_block pair (the scale is 2-D) or an mxfp4 pair (wq is uint8)."""
        if not isinstance(w, tuple):
            return x @ w
        wq, scale = w
        mx = wq.dtype == torch.uint8
        if not mx and scale.dim() == 2:
            return ops.linear_fp8_block(x, wq, scale)
        max_t = self._mxfp4_kernel_max_t if mx else self._fp8_kernel_max_t
        if not mx and self.activation_dtype == "fp8" and x.shape[0] > max_t:
            return ops.linear_fp8_a8(x, wq, scale)
        if not x.is_cuda or x.shape[0] <= max_t:
            return ops.linear_mxfp4(x, wq, scale) if mx else \
                ops.linear_fp8(x, wq, scale)
        # one bf16 scratch per stream (prefill and decode may overlap),
        # sized for the largest projection: in * out elements, which is
        # twice wq.numel() for mxfp4
        key = torch.cuda.current_stream(x.device).cuda_stream
        buf = self._fp8_scratch.get(key)
        if buf is None:
            n = max(layer[name][0].numel() for layer in self.layers
                    for name in LORA_TARGETS if name in layer)
            buf = self._fp8_scratch[key] = torch.empty(
                2 * n if mx else n, dtype=torch.bfloat16, device=x.device)
        n_out, n_in = wq.shape[0], x.shape[1]
        dense = buf[:n_in * n_out].view(n_in, n_out)
        if mx:
            return x @ ops.dequant_mxfp4_weight(wq, scale, dense)
        return x @ ops.dequant_fp8_weight(wq, scale, dense)

    # ------------------------------------------------------------------
    def forward(self, batch: ForwardBatch, kv_pool: torch.Tensor,
                embeddings_out: bool = False,
                kv_scales=None, kv_observer=None,
                lora_weights=None) -> torch.Tensor:
        """Returns logits [n_logit_rows, vocab] (or final hidden states for
        embeddings_out). kv_pool: [L, 2, NB, KVH, BS, D].

        kv_scales: the pool's scales for a scaled fp8 cache
        (KVPool.all_layer_scales(): per layer the [KVH] fp32 views k_scale,
        v_scale, k_inv_scale, v_inv_scale), None otherwise.
        kv_observer(li, k, v), if given, sees each layer's post-RoPE K and
        its V [T, KVH, D] just before the store (calibration).
        lora_weights: per layer, target -> (A [S, R, in], B [S, out, R]) slot
        pools; read only when batch.lora names rows (DEVELOPMENT.md "LoRA
        adapters"). The update of the fused wqkv goes into qkv, ahead of
        RoPE and the KV store."""
        c = self.cfg
        lora = batch.lora
        if lora is not None and lora_weights is None:
            raise ValueError("batch.lora needs lora_weights")
        if lora is not None and c.num_experts:
            raise ValueError("LoRA adapters are not supported for an MoE "
                             "model")

        def lora_add(y, x, li, target):
            A, B = lora_weights[li][target]
            ops.lora_add(y, x, A, B, lora.perm, lora.tiles)
        hidden = self.embed[batch.input_ids]
        if batch.embed_rows is not None and batch.embed_rows.numel():
            hidden[batch.embed_rows] = batch.embed_values.to(hidden.dtype)
        residual = None
        pos32 = batch.positions.to(torch.int32)
        # one kernel from the QKV GEMM's output to q and the stored K/V
        # (ops.qkv_rope_cache). Calibration needs k and v as tensors and
        # QK-norm sits between the split and RoPE: both keep the op chain.
        # So does an fp8 pool for now: tests/test_gpu_kv_scales.py watches
        # the scales (or their absence) arrive at ops.reshape_and_cache.
        fused_qkv = (self._fused_qkv and kv_observer is None
                     and kv_pool.dtype == torch.bfloat16
                     and not c.qk_norm and c.head_dim % 16 == 0)
        for li, layer in enumerate(self.layers):
            if residual is None:
                residual = hidden.clone()
                normed = ops.rmsnorm(hidden, layer["input_norm"], c.rms_eps)
            else:
                normed = ops.rmsnorm(hidden, layer["input_norm"], c.rms_eps,
                                     residual=residual)
            qkv = self._linear(normed, layer["wqkv"])
            if lora is not None:
                lora_add(qkv, normed, li, "wqkv")
            T = qkv.shape[0]
            k_cache = kv_pool[li, 0]
            v_cache = kv_pool[li, 1]
            k_scale = v_scale = k_inv = v_inv = None
            if kv_scales is not None:
                k_scale, v_scale, k_inv, v_inv = kv_scales[li]
            if fused_qkv:
                q = ops.qkv_rope_cache(qkv, self.cos_sin, pos32,
                                       batch.slot_mapping, k_cache, v_cache,
                                       c.num_heads, k_inv_scale=k_inv,
                                       v_inv_scale=v_inv)
            else:
                q, k, v = qkv.split([c.q_size, c.kv_size, c.kv_size], dim=-1)
                q = q.view(T, c.num_heads, c.head_dim).contiguous()
                k = k.view(T, c.num_kv_heads, c.head_dim).contiguous()
                v = v.view(T, c.num_kv_heads, c.head_dim).contiguous()
                if c.qk_norm:
                    # Qwen3 per-head QK-RMSNorm before RoPE: each head's
                    # D-vector normalized with a learned gain (the rmsnorm
                    # kernel treats [T*H, D] rows like any hidden dim)
                    q = ops.rmsnorm(q.view(T * c.num_heads, c.head_dim),
                                    layer["q_norm"],
                                    c.rms_eps).view(T, c.num_heads,
                                                    c.head_dim)
                    k = ops.rmsnorm(k.view(T * c.num_kv_heads, c.head_dim),
                                    layer["k_norm"],
                                    c.rms_eps).view(T, c.num_kv_heads,
                                                    c.head_dim)
                ops.rope(q, k, self.cos_sin, pos32)
                if kv_observer is not None:
                    kv_observer(li, k, v)
                ops.reshape_and_cache(k, v, k_cache, v_cache,
                                      batch.slot_mapping,
                                      k_inv_scale=k_inv, v_inv_scale=v_inv)
            if batch.is_decode:
                attn = ops.paged_attention(q, k_cache, v_cache,
                                           batch.block_tables, batch.seq_lens,
                                           self.scale,
                                           max_seq_len=batch.max_seq_len,
                                           k_scale=k_scale, v_scale=v_scale)
            else:
                attn = self._prefill_attention(batch, q, k_cache, v_cache,
                                               k_scale, v_scale)
            attn = attn.view(T, c.q_size)
            o = self._linear(attn, layer["wo"])
            if lora is not None:
                lora_add(o, attn, li, "wo")
            normed2 = ops.rmsnorm(o, layer["post_norm"], c.rms_eps,
                                  residual=residual)
            if c.num_experts:
                hidden = self._moe(normed2, layer)
                continue
            gate_up = self._linear(normed2, layer["wgate_up"])
            if lora is not None:
                lora_add(gate_up, normed2, li, "wgate_up")
            act = ops.silu_mul(gate_up)
            hidden = self._linear(act, layer["wdown"])
            if lora is not None:
                lora_add(hidden, act, li, "wdown")
        final = ops.rmsnorm(hidden, self.final_norm, c.rms_eps,
                            residual=residual)
        # `residual` now holds the pre-norm sum; `final` the normed states
        if embeddings_out:
            return final
        rows = batch.logit_rows
        sel = final if rows is None else final[rows]
        return sel @ self.lm_head.t()

    def _prefill_attention(self, batch: ForwardBatch, q: torch.Tensor,
                           k_cache: torch.Tensor,
                           v_cache: torch.Tensor,
                           k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
        """Causal varlen attention per sequence. GPU: fused MFMA flash
        kernel (flash_prefill.hip) — S never materialized. CPU fallback:
        composed chunked torch attention over pool-gathered KV."""
        c = self.cfg
        if (q.is_cuda and batch.prefill_tiles is not None
                and c.head_dim == 128
                and c.num_heads // c.num_kv_heads in (1, 2, 4, 8)):
            return ops.flash_prefill(
                q, k_cache, v_cache, batch.prefill_bt, batch.prefill_meta,
                batch.prefill_tiles, self.scale,
                k_scale=k_scale, v_scale=v_scale)
        qpg = c.num_heads // c.num_kv_heads
        out = torch.empty_like(q)
        starts = batch.seq_starts
        for i in range(len(starts) - 1):
            s, e = starts[i], starts[i + 1]
            chunk = e - s
            ctx = batch.ctx_lens[i]
            prior = ctx - chunk
            kk, vv = ops_ref.gather_prefix(k_cache, v_cache,
                                           batch.prefill_block_tables[i], ctx)
            # [KVH, ctx, D]
            kk = ops_ref.dequant(kk.permute(1, 0, 2), k_scale)
            vv = ops_ref.dequant(vv.permute(1, 0, 2), v_scale)
            qi = q[s:e].view(chunk, c.num_kv_heads, qpg,
                             c.head_dim).permute(1, 2, 0, 3)  # [KVH,qpg,chunk,D]
            scores = torch.einsum("hgtd,hsd->hgts", qi.float(), kk.float())
            scores *= self.scale
            # causal mask: query t (global pos prior+t) sees keys <= prior+t
            t_idx = torch.arange(chunk, device=q.device).view(1, 1, chunk, 1)
            s_idx = torch.arange(ctx, device=q.device).view(1, 1, 1, ctx)
            scores.masked_fill_(s_idx > t_idx + prior, float("-inf"))
            p = torch.softmax(scores, dim=-1)
            o = torch.einsum("hgts,hsd->hgtd", p, vv.float())
            out[s:e] = o.permute(2, 0, 1, 3).reshape(
                chunk, c.num_heads, c.head_dim).to(q.dtype)
        return out
