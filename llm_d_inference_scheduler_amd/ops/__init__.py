from .dispatch import (  # noqa: F401
    flash_prefill, hip_ops, lora_add, lora_worklist, move_blocks,
    paged_attention, qkv_rope_cache, reshape_and_cache, rmsnorm, rope, sample,
    sample_ext, silu_mul, token_state_alloc, token_state_fill,
)
