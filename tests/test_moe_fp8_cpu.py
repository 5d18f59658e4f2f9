"""fp8 experts without a GPU (DEVELOPMENT.md "Mixture of experts"): the
plain-torch op against the float64 bound, the quantiser, and the CPU engine
with expert_dtype."""
import dataclasses

import pytest
import torch

import moe_cases as mc
import moe_fp8_cases as f8c
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA, TINY_MOE
from llm_d_inference_scheduler_amd.models.llama import LlamaRunner


@pytest.mark.parametrize("name", list(f8c.CASES))
def test_ref_against_float64(name):
    args, (w13, w2) = f8c.build(name, "cpu")
    y = ops.moe_ffn_fp8(*args)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    assert mc.ffn_excess(y, args[0], w13, w2, *args[5:]) <= 0


def test_quantize_experts_is_per_expert():
    W = torch.randn(3, 32, 48, generator=torch.Generator().manual_seed(0))
    W[1] *= 100.0
    wq, scale = ops.ref.quantize_experts_fp8(W.bfloat16())
    assert wq.dtype == torch.float8_e4m3fn and wq.shape == W.shape
    assert scale.dtype == torch.float32 and scale.shape == (3, 32)
    for e in range(3):
        q, s = ops.ref.quantize_weight_fp8(W[e].bfloat16().t())
        assert torch.equal(wq[e].view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(scale[e], s)
    assert torch.equal(ops.ref.dequant_experts_fp8(wq, scale),
                       wq.float() * scale[..., None])


@pytest.mark.parametrize("weight_dtype, expert_dtype",
                         [("auto", "fp8"), ("fp8", "fp8"), ("auto", "mxfp4")])
def test_cpu_engine_with_expert_dtype(weight_dtype, expert_dtype):
    worker = EngineWorker(TINY_MOE, "cpu", kv_blocks=64,
                          weight_dtype=weight_dtype, expert_dtype=expert_dtype)
    m = worker.model
    assert m.expert_dtype == expert_dtype
    want = torch.float8_e4m3fn if expert_dtype == "fp8" else torch.uint8
    for layer, exact in zip(m.layers, m.dense_layers()):
        assert layer["router"].dtype == torch.bfloat16
        assert isinstance(layer["wqkv"], tuple) == (weight_dtype == "fp8")
        E, n_out, n_in = exact["w13"].shape
        assert exact["w13"].dtype == torch.float32
        assert (n_out, n_in) == (2 * TINY_MOE.moe_intermediate_size,
                                 TINY_MOE.hidden_size)
        for name in ("w13", "w2"):
            assert layer[name][0].dtype == want
        if expert_dtype == "fp8":
            assert layer["w13"][1].shape == (E, n_out)
    assert m.weight_bytes() < LlamaRunner(
        TINY_MOE, torch.device("cpu")).weight_bytes()
    worker.add_request(EngineRequest("r", prompt_tokens=list(range(40, 73)),
                                     max_tokens=5))
    toks = [t for _ in range(20) for o in worker.step() for t in o.new_tokens]
    assert len(toks) == 5 and not worker.has_work


def test_out_of_scope_raises():
    with pytest.raises(ValueError):
        EngineWorker(TINY_LLAMA, "cpu", kv_blocks=64, expert_dtype="fp8")
    with pytest.raises(ValueError, match="expert_dtype"):
        EngineWorker(TINY_MOE, "cpu", kv_blocks=64, weight_dtype="fp8")
    runner = LlamaRunner(TINY_MOE, torch.device("cpu"))
    runner.quantize_experts("fp8")
    with pytest.raises(ValueError):
        runner.quantize_experts("fp8")
    runner = LlamaRunner(dataclasses.replace(
        TINY_MOE, moe_intermediate_size=48), torch.device("cpu"))
    with pytest.raises(ValueError):
        runner.quantize_experts("mxfp4")
    runner.quantize_experts("fp8")      # I = 48 is legal for fp8 experts
