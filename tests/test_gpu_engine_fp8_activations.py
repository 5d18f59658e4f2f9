"""Scenario A of engine_cases on the device with fp8 weights and fp8
activations (DEVELOPMENT.md "fp8 activations"): the float64 dense model
reads the dequantised weights and full-precision activations, so what
remains is activation rounding, here with the e4m3 rounding of the prefill
rows in it."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

# The worst row error of the bf16 CPU worker (ops.ref) on scenario A with
# quantised weights, fp8 activations and _fp8_kernel_max_t = 16, as measured
# (4.4849e-2) and rounded up to two digits
CPU_WORST_FP8A = 0.045
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_FP8A


def test_scenario_a_fp8_activations(monkeypatch):
    calls = {"linear": [], "a8": [], "dequant": 0}
    linear, a8, dequant = ops.linear_fp8, ops.linear_fp8_a8, \
        ops.dequant_fp8_weight

    def spy_linear(x, wq, scale):
        calls["linear"].append(x.shape[0])
        return linear(x, wq, scale)

    def spy_a8(x, wq, scale):
        calls["a8"].append(x.shape[0])
        return a8(x, wq, scale)

    def spy_dequant(wq, scale, out):
        calls["dequant"] += 1
        return dequant(wq, scale, out)

    monkeypatch.setattr(ops, "linear_fp8", spy_linear)
    monkeypatch.setattr(ops, "linear_fp8_a8", spy_a8)
    monkeypatch.setattr(ops, "dequant_fp8_weight", spy_dequant)
    ref = types.SimpleNamespace()

    def setup(worker):
        m = worker.model
        m.quantize_weights("fp8")
        m.set_activation_dtype("fp8")
        # A's prefill chunks are 48 rows, its decode batches 3 at the most
        m._fp8_kernel_max_t = 16
        ref.cfg, ref.cos_sin, ref.embed = m.cfg, m.cos_sin, m.embed
        ref.final_norm, ref.lm_head = m.final_norm, m.lm_head
        ref.layers = m.dense_layers()

    res = ec.run("A", "cuda:0", setup=setup, ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A fp8a|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    n_dec = sum(r.is_decode for r in res.rec.records)
    per_pass = 4 * ec.CONFIG.num_layers
    assert len([t for t in calls["linear"] if t <= 3]) >= n_dec * per_pass
    assert max(calls["linear"]) <= 16 and calls["dequant"] == 0
    assert len(calls["a8"]) >= per_pass and min(calls["a8"]) > 16
    assert not res.worker.model._fp8_scratch
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst
