"""Scenario A of engine_cases on the device through the MoE path with fp8
experts and fp8 expert activations (DEVELOPMENT.md "Mixture of experts"). As
in test_gpu_engine_moe_fp8 the worker is upcycled to 8 identical experts, 2 a
token, and the float64 dense model reads the dequantised expert 0 with
full-precision activations: what remains is activation rounding, here with
the two e4m3 roundings of the prefill rows' experts in it."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_MOE
from test_gpu_engine_moe_fp8 import upcycle_and_quantize

# The worst row error of the bf16 CPU worker (ops.ref) on the same upcycled
# scenario with fp8 experts, fp8 expert activations and _moe_a8_min_rows = 4,
# as measured (7.653e-3) and rounded up to two digits
CPU_WORST_MOE_FP8_A8 = 0.0077
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_MOE_FP8_A8


def setup_a8(ref):
    quantize = upcycle_and_quantize(ref)

    def setup(worker):
        quantize(worker)
        worker.model.set_expert_activation_dtype("fp8")
        # A's prefill chunks are 48 rows, 12 a expert in the mean; its decode
        # batches 3 at the most, under one a expert
        worker.model._moe_a8_min_rows = 4
    return setup


@pytest.mark.gpu
def test_scenario_a_moe_fp8_a8(monkeypatch):
    calls = {"fp8": [], "a8": []}
    ffn, a8 = ops.moe_ffn_fp8, ops.moe_ffn_fp8_a8

    def spy_ffn(x, *a):
        calls["fp8"].append(x.shape[0])
        return ffn(x, *a)

    def spy_a8(x, *a):
        calls["a8"].append(x.shape[0])
        return a8(x, *a)

    monkeypatch.setattr(ops, "moe_ffn_fp8", spy_ffn)
    monkeypatch.setattr(ops, "moe_ffn_fp8_a8", spy_a8)
    ref = types.SimpleNamespace()
    res = ec.run("A", "cuda:0", setup=setup_a8(ref), ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A moe fp8 a8|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    # every layer of every pass went to one of the two ops, by its batch size
    n_dec = sum(r.is_decode for r in res.rec.records)
    n_pre = len(res.rec.records) - n_dec
    assert n_dec and n_pre
    assert len(calls["fp8"]) + len(calls["a8"]) == \
        len(res.rec.records) * ec.CONFIG.num_layers
    assert len(calls["fp8"]) >= n_dec * ec.CONFIG.num_layers
    assert calls["a8"] and min(calls["a8"]) * 2 > 4 * 8
    assert max(calls["fp8"]) * 2 <= 4 * 8
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst


def test_expert_activation_dtype_needs_fp8_experts():
    for expert_dtype in ("auto", "bf16", "mxfp4"):
        with pytest.raises(ValueError, match="expert_activation_dtype"):
            EngineWorker(TINY_MOE, "cpu", kv_blocks=16,
                         expert_dtype=expert_dtype,
                         expert_activation_dtype="fp8")
    worker = EngineWorker(TINY_MOE, "cpu", kv_blocks=16, expert_dtype="fp8",
                          expert_activation_dtype="fp8")
    assert worker.model.expert_activation_dtype == "fp8"
    # "auto" leaves the experts alone, whatever activation_dtype says
    worker = EngineWorker(TINY_MOE, "cpu", kv_blocks=16, weight_dtype="fp8",
                          expert_dtype="fp8", activation_dtype="fp8")
    assert worker.model.expert_activation_dtype == "bf16"
