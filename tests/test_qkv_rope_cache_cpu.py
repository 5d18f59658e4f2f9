"""ops.qkv_rope_cache on CPU tensors against the chain of ref ops it stands
for: split, three .contiguous(), rope, reshape_and_cache."""
import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref


def chain(qkv, cos_sin, pos, slots, kc, vc, qh, k_inv=None, v_inv=None):
    T = qkv.shape[0]
    kvh, d = kc.shape[1], kc.shape[3]
    q, k, v = qkv.split([qh * d, kvh * d, kvh * d], dim=-1)
    q = q.view(T, qh, d).contiguous()
    k = k.view(T, kvh, d).contiguous()
    v = v.view(T, kvh, d).contiguous()
    ref.rope(q, k, cos_sin, pos)
    ref.reshape_and_cache(k, v, kc, vc, slots, k_inv_scale=k_inv,
                          v_inv_scale=v_inv)
    return q


@pytest.mark.parametrize("cache", ["bf16", "fp8", "fp8_scaled"])
@pytest.mark.parametrize("T,qh,kvh", [(1, 4, 4), (5, 8, 2)])
def test_matches_ref_chain(T, qh, kvh, cache):
    torch.manual_seed(T * 100 + qh)
    d, bs, nb, max_pos = 32, 4, 6, 64
    x = torch.randn(T, 48).bfloat16()
    w = torch.randn(48, (qh + 2 * kvh) * d).bfloat16()
    qkv = x @ w
    cos_sin = ref.rope_table(max_pos, d, 10000.0)
    pos = torch.randint(0, max_pos, (T,), dtype=torch.int32)
    pos[0] = max_pos - 1
    slots = torch.randperm(nb * bs)[:T].to(torch.int64)
    if T > 1:
        slots[1] = -1
    dtype = torch.bfloat16 if cache == "bf16" else torch.float8_e4m3fn
    kc0 = torch.randn(nb, kvh, bs, d).to(dtype)
    vc0 = torch.randn(nb, kvh, bs, d).to(dtype)
    k_inv = v_inv = None
    if cache == "fp8_scaled":
        k_inv = torch.linspace(0.5, 2.0, kvh)
        v_inv = torch.linspace(3.0, 0.25, kvh)

    kc_a, vc_a = kc0.clone(), vc0.clone()
    q_a = chain(qkv.clone(), cos_sin, pos, slots, kc_a, vc_a, qh, k_inv,
                v_inv)
    kc_b, vc_b = kc0.clone(), vc0.clone()
    qkv_in = qkv.clone()
    q_b = ops.qkv_rope_cache(qkv_in, cos_sin, pos, slots, kc_b, vc_b, qh,
                             k_inv_scale=k_inv, v_inv_scale=v_inv)

    assert q_b.shape == (T, qh, d) and q_b.is_contiguous()
    assert torch.equal(q_a, q_b)
    # whole caches, viewed as bytes: untouched slots stay untouched
    assert torch.equal(kc_a.view(torch.uint8), kc_b.view(torch.uint8))
    assert torch.equal(vc_a.view(torch.uint8), vc_b.view(torch.uint8))
    assert torch.equal(qkv_in, qkv)          # the input is not rotated
    assert not torch.equal(kc_b.view(torch.uint8), kc0.view(torch.uint8))


def test_runner_fused_equals_chain():
    """LlamaRunner.forward gives the same logits and the same pool with the
    fused op and with it forced off."""
    import dataclasses

    from llm_d_inference_scheduler_amd.models.configs import LLAMA_3_8B
    from llm_d_inference_scheduler_amd.models.llama import (ForwardBatch,
                                                            LlamaRunner)
    cfg = dataclasses.replace(
        LLAMA_3_8B, num_layers=2, hidden_size=64, intermediate_size=128,
        num_heads=4, num_kv_heads=2, head_dim=16, vocab_size=97,
        max_position=64)
    runner = LlamaRunner(cfg, torch.device("cpu"), seed=3)
    bs, nb = 4, 8
    T = 3
    batch = ForwardBatch(
        input_ids=torch.tensor([5, 17, 42]),
        positions=torch.tensor([6, 0, 9], dtype=torch.int32),
        slot_mapping=torch.tensor([6, 8, 17], dtype=torch.int64),
        is_decode=True,
        block_tables=torch.tensor([[0, 1], [2, 0], [3, 4]],
                                  dtype=torch.int32),
        seq_lens=torch.tensor([7, 1, 6], dtype=torch.int32), max_seq_len=7)
    outs = []
    for fused in (True, False):
        runner._fused_qkv = fused
        torch.manual_seed(0)
        pool = torch.randn(cfg.num_layers, 2, nb, cfg.num_kv_heads, bs,
                           cfg.head_dim).bfloat16()
        outs.append((runner.forward(batch, pool), pool))
    assert outs[0][0].shape == (T, cfg.vocab_size)
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
