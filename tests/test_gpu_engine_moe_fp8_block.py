"""Scenario A of engine_cases on the device through the MoE path with
block-scaled fp8 experts (DEVELOPMENT.md "Mixture of experts"). As in
test_gpu_engine_moe_fp8 the worker is upcycled to 8 identical experts, 2 a
token, and the float64 dense model reads the dequantised expert 0 with
full-precision activations: what remains is activation rounding, here with
the two group-scaled e4m3 roundings of every row's experts in it."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

# The worst row error of the bf16 CPU worker (ops.ref) on the same upcycled
# scenario with fp8_block128 experts, as measured (7.313e-3) and rounded up to
# two digits
CPU_WORST_MOE_FP8_BLOCK = 0.0074
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_MOE_FP8_BLOCK


def upcycle_and_quantize(ref):
    def setup(worker):
        m = worker.model
        ref.cfg, ref.cos_sin, ref.embed = m.cfg, m.cos_sin, m.embed
        ref.final_norm, ref.lm_head = m.final_norm, m.lm_head
        m.upcycle_to_moe(8, 2)
        m.quantize_experts("fp8_block128")
        ref.layers = [
            {**{k: w for k, w in layer.items() if k not in ("w13", "w2")},
             "wgate_up": layer["w13"][0].t(), "wdown": layer["w2"][0].t()}
            for layer in m.dense_layers()]
    return setup


def test_scenario_a_moe_fp8_block(monkeypatch):
    calls = []
    ffn = ops.moe_ffn_fp8_block

    def spy_ffn(x, *a):
        calls.append(x.is_cuda and all(t.is_cuda for t in a[:6]))
        return ffn(x, *a)

    monkeypatch.setattr(ops, "moe_ffn_fp8_block", spy_ffn)
    ref = types.SimpleNamespace()
    res = ec.run("A", "cuda:0", setup=upcycle_and_quantize(ref), ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A moe fp8 block|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    # every layer of every decode pass and every prefill pass
    n_calls = len(res.rec.records) * ec.CONFIG.num_layers
    assert any(r.is_decode for r in res.rec.records)
    assert any(not r.is_decode for r in res.rec.records)
    assert len(calls) == n_calls and all(calls)
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst
