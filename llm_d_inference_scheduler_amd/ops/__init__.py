from .dispatch import (  # noqa: F401
    dequant_fp8_weight, dequant_mxfp4_weight, flash_prefill, hip_ops,
    linear_fp8, linear_fp8_a8, linear_fp8_block, linear_mxfp4, lora_add,
    lora_worklist, moe_ffn,
    moe_ffn_fp8, moe_ffn_fp8_a8, moe_ffn_fp8_block, moe_ffn_mxfp4,
    moe_fp8_a8_scratch_bytes, moe_fp8_block_scratch_bytes, moe_route, moe_scratch_bytes, move_blocks,
    paged_attention, qkv_rope_cache, quantize_groups_fp8, quantize_rows_fp8,
    reshape_and_cache, rmsnorm, rope, sample, sample_ext, silu_mul,
    token_state_alloc, token_state_fill,
)
