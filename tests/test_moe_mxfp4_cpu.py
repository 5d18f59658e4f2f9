"""MXFP4 experts without a GPU (DEVELOPMENT.md "Mixture of experts"): the
plain-torch op and the CPU engine."""
import dataclasses

import pytest
import torch

import moe_mxfp4_cases as mxc
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_MOE
from llm_d_inference_scheduler_amd.models.llama import LlamaRunner


def test_ref_is_moe_ffn_on_the_dequantised_experts():
    args, (w13, w2) = mxc.build("tail", "cpu")
    y = ops.moe_ffn_mxfp4(*args)
    assert torch.equal(y, ops.ref.moe_ffn(args[0], w13, w2, *args[5:]))


def _generate(worker):
    worker.add_request(EngineRequest("r", prompt_tokens=list(range(40, 73)),
                                     max_tokens=5))
    toks = []
    for _ in range(50):
        for o in worker.step():
            toks.extend(o.new_tokens)
        if not worker.has_work:
            break
    return toks


def test_cpu_engine_with_mxfp4_experts():
    make = lambda **kw: EngineWorker(TINY_MOE, "cpu", kv_blocks=64, **kw)
    dense, workers = make().model, [make(weight_dtype="mxfp4")
                                    for _ in range(2)]
    m = workers[0].model
    for layer, was, exact in zip(m.layers, dense.layers, m.dense_layers()):
        assert layer["router"].dtype == torch.bfloat16
        for name in ("w13", "w2"):
            wq, scale = layer[name]
            assert wq.dtype == scale.dtype == torch.uint8
            assert wq.shape == (*was[name].shape[:2], was[name].shape[2] // 2)
            assert scale.shape[2] == was[name].shape[2] // 32
            want = torch.stack([ops.ref.dequant_mxfp4_weight(
                *ops.ref.quantize_weight_mxfp4(w.t()), dtype=torch.float32).t()
                for w in was[name]])
            assert exact[name].dtype == torch.float32
            assert torch.equal(exact[name], want)
    assert m.weight_bytes() < dense.weight_bytes()
    runs = [_generate(w) for w in workers]
    assert len(runs[0]) == 5 and runs[0] == runs[1]


def test_intermediate_size_48_raises():
    runner = LlamaRunner(dataclasses.replace(
        TINY_MOE, moe_intermediate_size=48), torch.device("cpu"))
    with pytest.raises(ValueError):
        runner.quantize_weights("mxfp4")
