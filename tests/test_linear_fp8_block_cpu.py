"""Block-scaled fp8 linears on the CPU path (DEVELOPMENT.md "fp8 block
scales"): the reference quantisers, ops.ref.linear_fp8_block, the runner's
conversion and validation, and a CPU EngineWorker with fp8_block weights."""
import dataclasses

import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.models.llama import LlamaRunner
from llm_d_inference_scheduler_amd.ops import ref

# two groups and a 64-wide tail; one full block row and a 16-row ragged one
T, IN, OUT = 5, 320, 144


def _case():
    gen = torch.Generator().manual_seed(0)
    a = torch.tensor([-5.0, 0.0, 5.0]).repeat_interleave(128)[:IN]
    W = torch.randn(IN, OUT, generator=gen) * torch.exp2(-a)[:, None]
    W[128:256, :128] = 0                     # block (0, 1) is all zero
    x = torch.randn(T, IN, generator=gen) * torch.exp2(a)
    x[2] = 0
    x[3, 128:256] = 0
    return x.to(torch.bfloat16), W.to(torch.bfloat16)


def _half_step(q, s):
    """e4m3's half ulp at code q under scale s: 2^-4 relative, 2^-10 absolute
    below the normals."""
    return s * torch.maximum(q.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10))


def test_quantize_weight_block():
    W = _case()[1]
    wq, scale = ref.quantize_weight_fp8_block(W)
    assert wq.dtype == torch.float8_e4m3fn and tuple(wq.shape) == (OUT, IN)
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (2, 3)
    wt = W.float().t()
    assert float(scale[0, 1]) == 1.0 and not wq[:128, 128:256].float().any()
    assert torch.equal(scale[0, 0], wt[:128, :128].abs().max() / 448)
    assert torch.equal(scale[1, 2], wt[128:, 256:].abs().max() / 448)  # ragged
    full = ref.expand_fp8_block_scale(scale, OUT, IN)
    q = wq.float()
    assert bool(((wt - q * full).abs() <= _half_step(q, full)).all())


def test_quantize_groups():
    x = _case()[0]
    xq, sx = ref.quantize_groups_fp8(x)
    assert xq.dtype == torch.float8_e4m3fn and tuple(xq.shape) == (T, IN)
    assert sx.dtype == torch.float32 and tuple(sx.shape) == (T, 3)
    assert bool((sx[2] == 1).all()) and float(sx[3, 1]) == 1.0
    assert torch.equal(sx[0, 2], x[0, 256:].float().abs().max() / 448)  # tail
    full = sx.repeat_interleave(128, 1)[:, :IN]
    q = xq.float()
    assert bool(((x.float() - q * full).abs() <= _half_step(q, full)).all())
    assert float(sx[0].max() / sx[0].min()) >= 2.0 ** 8


def test_ref_linear_against_float64():
    x, W = _case()
    wq, scale = ref.quantize_weight_fp8_block(W)
    y = ops.linear_fp8_block(x, wq, scale)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, OUT)
    xq, sx = ops.quantize_groups_fp8(x)
    x64 = xq.double() * sx.double().repeat_interleave(128, 1)[:, :IN]
    w64 = wq.double() * ref.expand_fp8_block_scale(scale.double(), OUT, IN)
    y64 = x64 @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + IN * 2.0 ** -23 * (x64.abs()
                                                       @ w64.abs().t())
    assert bool(((y.double() - y64).abs() <= bound).all())


def test_runner_conversion_and_dense_layers():
    m = LlamaRunner(TINY_LLAMA, torch.device("cpu"), torch.bfloat16)
    m.quantize_weights("fp8_block")
    assert m.weight_dtype == "fp8_block"
    for layer, dense in zip(m.layers, m.dense_layers()):
        for name in ("wqkv", "wo", "wgate_up", "wdown"):
            wq, scale = layer[name]
            assert wq.dtype == torch.float8_e4m3fn and scale.dim() == 2
            exact = wq.double() * ref.expand_fp8_block_scale(
                scale.double(), *wq.shape)
            assert torch.equal(dense[name], exact.float().t())
    m.set_activation_dtype("auto")
    m.set_activation_dtype("fp8")
    with pytest.raises(ValueError, match="defined with fp8 activations"):
        m.set_activation_dtype("bf16")
    with pytest.raises(ValueError, match="already fp8_block"):
        m.quantize_weights("fp8")


def test_moe_rules():
    moe = dataclasses.replace(TINY_LLAMA, num_experts=4, experts_per_token=2,
                              moe_intermediate_size=64)
    with pytest.raises(ValueError, match="alone is not supported"):
        EngineWorker(moe, "cpu", kv_blocks=16, weight_dtype="fp8_block")
    with pytest.raises(ValueError, match="unknown expert_dtype"):
        EngineWorker(moe, "cpu", kv_blocks=16, expert_dtype="fp8_block")
    worker = EngineWorker(moe, "cpu", kv_blocks=16, weight_dtype="fp8_block",
                          expert_dtype="fp8")
    layer = worker.model.layers[0]
    assert layer["wqkv"][1].dim() == 2 and layer["w13"][1].dim() == 2
    assert layer["w13"][0].dim() == 3      # per-channel fp8 experts


def test_cpu_worker_with_fp8_block_weights(monkeypatch):
    worker = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=16,
                          weight_dtype="fp8_block")
    seen, block = [], ops.linear_fp8_block
    monkeypatch.setattr(ops, "linear_fp8_block", lambda x, wq, scale:
                        seen.append(x.shape[0]) or block(x, wq, scale))
    worker.add_request(EngineRequest("r", prompt_tokens=list(range(3, 23)),
                                     max_tokens=3))
    outs = []
    for _ in range(16):
        outs.extend(worker.step())
        if not worker.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert fin and fin[0].completion_tokens == 3 and not fin[0].error
    per_pass = 4 * TINY_LLAMA.num_layers
    assert seen[:per_pass] == [20] * per_pass and set(seen[per_pass:]) == {1}
    assert not worker.model._fp8_scratch
