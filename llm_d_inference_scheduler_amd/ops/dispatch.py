"""Op dispatch: gfx950 HIP kernels on GPU tensors, torch reference on CPU.

Policy (driver contract): on a GPU box the HIP extension is REQUIRED — a
CUDA-device tensor with `_hip_ops` missing raises immediately rather than
silently falling back to eager torch. CPU tensors (tests, tiny gloo runs)
use ops.ref.
"""
from typing import Optional

import torch

from . import ref

try:
    from .. import _hip_ops as _ext
except ImportError:  # extension not built
    _ext = None


def hip_ops():
    """The raw extension module (router prefix kernels etc.). Fail-loud."""
    if _ext is None:
        raise RuntimeError(
            "_hip_ops extension is not built; run "
            "`python setup.py build_ext --inplace` (gfx950 HIP kernels are "
            "mandatory on GPU hosts — no eager fallback)")
    return _ext


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    hip_ops()  # raises if missing on a GPU path
    return True


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float,
            residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _use_hip(x):
        return _ext.rmsnorm(x, w, eps, residual)
    return ref.rmsnorm(x, w, eps, residual)


def rope(q: torch.Tensor, k: torch.Tensor, cos_sin: torch.Tensor,
         positions: torch.Tensor) -> None:
    if _use_hip(q):
        _ext.rope(q, k, cos_sin, positions.to(torch.int32))
        return
    ref.rope(q, k, cos_sin, positions)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    if _use_hip(gate_up):
        return _ext.silu_mul(gate_up)
    return ref.silu_mul(gate_up)


def reshape_and_cache(k_new: torch.Tensor, v_new: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor,
                      slots: torch.Tensor, *,
                      k_inv_scale: Optional[torch.Tensor] = None,
                      v_inv_scale: Optional[torch.Tensor] = None) -> None:
    """k_inv_scale / v_inv_scale: [KVH] fp32 reciprocal per-head scales of
    a scaled fp8 cache (engine/kvcache.py KVPool); None = unscaled."""
    if _use_hip(k_new):
        _ext.reshape_and_cache(k_new, v_new, k_cache, v_cache,
                               slots.to(torch.int64), k_inv_scale,
                               v_inv_scale)
        return
    ref.reshape_and_cache(k_new, v_new, k_cache, v_cache, slots,
                          k_inv_scale=k_inv_scale, v_inv_scale=v_inv_scale)


def qkv_rope_cache(qkv: torch.Tensor, cos_sin: torch.Tensor,
                   positions: torch.Tensor, slot_mapping: torch.Tensor,
                   k_cache: torch.Tensor, v_cache: torch.Tensor,
                   n_q_heads: int, *,
                   k_inv_scale: Optional[torch.Tensor] = None,
                   v_inv_scale: Optional[torch.Tensor] = None
                   ) -> torch.Tensor:
    """The QKV GEMM's epilogue in one kernel: qkv [T, (QH + 2*KVH) * D] as
    the GEMM returns it -> rotated q [T, QH, D] (new, contiguous); rotated K
    and plain V are stored in the caches [NB, KVH, BS, D] at slot_mapping[t]
    (negative: nothing stored, q still returned). Bit-equal to split, three
    .contiguous(), rope and reshape_and_cache, which the CPU path runs."""
    if _use_hip(qkv):
        return _ext.qkv_rope_cache(qkv, cos_sin, positions.to(torch.int32),
                                   slot_mapping.to(torch.int64), k_cache,
                                   v_cache, n_q_heads, k_inv_scale,
                                   v_inv_scale)
    T = qkv.shape[0]
    kvh, d = k_cache.shape[1], k_cache.shape[3]
    q, k, v = qkv.split([n_q_heads * d, kvh * d, kvh * d], dim=-1)
    # clone, not contiguous(): at T == 1 the views are contiguous already
    # and the in-place rope would rotate the caller's qkv
    q = q.reshape(T, n_q_heads, d).clone()
    k = k.reshape(T, kvh, d).clone()
    v = v.reshape(T, kvh, d)
    ref.rope(q, k, cos_sin, positions)
    ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping,
                          k_inv_scale=k_inv_scale, v_inv_scale=v_inv_scale)
    return q


import os as _os

# online-softmax chunk of the decode kernel: 512 halves barrier count
# (bisect knob; 256 is the measured default)
_ATTN_CHUNK = int(_os.environ.get("LLMD_ATTN_CHUNK", "256"))


def split_geometry(n_wgs: int, max_seq_len: Optional[int],
                   chunk: int = _ATTN_CHUNK):
    """Flash-decoding partition geometry: (n_parts, part_tokens) when the
    split kernel should run for a launch of n_wgs = B*KVH workgroups over
    sequences of up to max_seq_len tokens, else None (single-pass kernel).

    The plain kernel launches only B*KVH workgroups — far short of the
    256-CU chip's >=2 WG/CU need. Long sequences are partitioned so the grid
    fills the chip; a combine kernel merges the unnormalized partials."""
    if max_seq_len is None or n_wgs >= 1024 or max_seq_len <= 512:
        return None
    target_np = min(64, max(1, 1024 // max(1, n_wgs)))
    # partition size: ceil-divide then round up to the kernel's
    # online-softmax chunk
    part = max(chunk, ((max_seq_len + target_np - 1) // target_np
                       + chunk - 1) // chunk * chunk)
    np_ = (max_seq_len + part - 1) // part
    return (np_, part) if np_ > 1 else None


def paged_attention(q: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, block_tables: torch.Tensor,
                    seq_lens: torch.Tensor, scale: float,
                    max_seq_len: Optional[int] = None, *,
                    k_scale: Optional[torch.Tensor] = None,
                    v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """k_scale / v_scale: [KVH] fp32 per-head dequant scales of a scaled
    fp8 cache; None = the cache holds the values themselves."""
    if _use_hip(q):
        bt = block_tables.to(torch.int32)
        sl = seq_lens.to(torch.int32)
        geom = split_geometry(q.shape[0] * k_cache.shape[1], max_seq_len)
        if geom is not None:
            return _ext.paged_attention_split(q, k_cache, v_cache, bt, sl,
                                              geom[0], geom[1], scale,
                                              _ATTN_CHUNK, k_scale, v_scale)
        return _ext.paged_attention(q, k_cache, v_cache, bt, sl, scale,
                                    _ATTN_CHUNK, k_scale, v_scale)
    return ref.paged_attention(q, k_cache, v_cache, block_tables, seq_lens,
                               scale, k_scale=k_scale, v_scale=v_scale)


def flash_prefill(q: torch.Tensor, k_cache: torch.Tensor,
                  v_cache: torch.Tensor, block_tables: torch.Tensor,
                  seq_meta: torch.Tensor, tiles: torch.Tensor,
                  scale: float, *,
                  k_scale: Optional[torch.Tensor] = None,
                  v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused MFMA causal varlen prefill attention (GPU-only; callers fall
    back to the composed reference path when unsupported). k_scale /
    v_scale as in paged_attention."""
    return hip_ops().flash_prefill(q, k_cache, v_cache, block_tables,
                                   seq_meta, tiles, scale, k_scale, v_scale)


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
           pos: torch.Tensor):
    """Fused sampler (DEVELOPMENT.md "Sampling"): logits [B, V] bf16|fp32 and
    per-row temperature f32, top_k i32 (0 = off), top_p f32 (1 = off), seed
    i64 (the bits of a u64) and pos i32 -> (tokens i64, logprobs f32,
    n_kept i32, threshold f32), all [B] on the logits' device."""
    if _use_hip(logits):
        return _ext.sample(logits.contiguous(), temperature, top_k, top_p,
                           seed, pos)
    return ref.sample(logits, temperature, top_k, top_p, seed, pos)


def sample_ext(logits: torch.Tensor, temperature: torch.Tensor,
               top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
               pos: torch.Tensor, rep: torch.Tensor, pres: torch.Tensor,
               freq: torch.Tensor, min_p: torch.Tensor, top_n: torch.Tensor,
               state_row: torch.Tensor,
               state: Optional[torch.Tensor] = None, n_top: int = 0):
    """sample() with repetition / presence / frequency penalties (rep, pres,
    freq f32 [B]) read from the token state (int16 [R, Vs], row state_row[r]
    or -1 for none; updated in place with the chosen token), min_p f32 [B]
    and the top_n[r] <= n_top best raw logprobs -> (tokens, logprobs,
    n_kept, threshold, top_tokens i64 [B, n_top], top_logprobs f32
    [B, n_top]). Rows of one call must not share a state_row >= 0."""
    if _use_hip(logits):
        return _ext.sample_ext(logits.contiguous(), temperature, top_k,
                               top_p, seed, pos, rep, pres, freq, min_p,
                               top_n, state_row, state, n_top)
    return ref.sample_ext(logits, temperature, top_k, top_p, seed, pos, rep,
                          pres, freq, min_p, top_n, state_row, state, n_top)


def token_state_alloc(rows: int, V: int, device) -> torch.Tensor:
    """Zeroed token state for `rows` requests over a vocabulary of V."""
    return ref.token_state_alloc(rows, V, device)


def token_state_fill(state: torch.Tensor, rows: torch.Tensor,
                     tokens: torch.Tensor, offsets: torch.Tensor,
                     n_prompt: torch.Tensor, V: int) -> None:
    """Rebuild state rows `rows` (i32 [n]) from token lists: entry q covers
    tokens[offsets[q] : offsets[q + 1]] (tokens i32, offsets i64 [n + 1]),
    its first n_prompt[q] (i32 [n]) ids being the prompt, the rest output."""
    if _use_hip(state):
        _ext.token_state_fill(state, rows, tokens, offsets, n_prompt, V)
        return
    ref.token_state_fill(state, rows, tokens, offsets, n_prompt, V)


def lora_worklist(row_slot):
    """(perm, tiles) of a batch from its per-row adapter slots, -1 for none
    (CPU int32 tensors; ops.ref.lora_worklist)."""
    return ref.lora_worklist(row_slot)


def lora_add(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
             B: torch.Tensor, perm: torch.Tensor, tiles: torch.Tensor) -> None:
    """Batched multi-adapter LoRA, in place (DEVELOPMENT.md "LoRA adapters"):
    y[row] += (x[row] · A[slot]ᵀ) · B[slot]ᵀ for the rows listed in perm
    (int32, grouped by slot), the slot from tiles [n, 3] int32 = (start in
    perm, count <= 16, slot). x [T, in], y [T, out] bf16; slot pools
    A [S, R, in], B [S, out, R] with alpha / rank folded into B."""
    if _use_hip(x):
        _ext.lora_add(y, x, A, B, perm, tiles)
        return
    ref.lora_add(y, x, A, B, perm, tiles)


def move_blocks(pool: torch.Tensor, staging: torch.Tensor,
                block_ids: torch.Tensor, is_scatter: bool) -> None:
    if _use_hip(pool):
        _ext.move_blocks(pool, staging, block_ids.to(torch.int32), is_scatter)
        return
    # CPU reference: pool [L, 2, NB, KVH, BS, D]; staging [n, L, 2, KVH, BS, D]
    ids = block_ids.long()
    if is_scatter:
        pool[:, :, ids] = staging.permute(1, 2, 0, 3, 4, 5)
    else:
        staging.copy_(pool[:, :, ids].permute(2, 0, 1, 3, 4, 5))
