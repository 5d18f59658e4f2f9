"""Scenario A of engine_cases on the device with MXFP4 weights
(DEVELOPMENT.md "MXFP4 weights"): the float64 dense model reads the exact
dequantisation, so what remains is activation rounding, as in the bf16 tier."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

# The worst row error of the bf16 CPU worker (ops.ref) on scenario A with
# mxfp4 weights, as measured (8.261e-3) and rounded up to two digits
CPU_WORST_MXFP4W = 0.0083
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_MXFP4W


def test_scenario_a_mxfp4_weights(monkeypatch):
    calls = {"linear": [], "dequant": 0}
    linear, dequant = ops.linear_mxfp4, ops.dequant_mxfp4_weight

    def spy_linear(x, wq, scale):
        calls["linear"].append(x.shape[0])
        return linear(x, wq, scale)

    def spy_dequant(wq, scale, out):
        calls["dequant"] += 1
        return dequant(wq, scale, out)

    monkeypatch.setattr(ops, "linear_mxfp4", spy_linear)
    monkeypatch.setattr(ops, "dequant_mxfp4_weight", spy_dequant)
    ref = types.SimpleNamespace()

    def setup(worker):
        m = worker.model
        m.quantize_weights("mxfp4")
        # A's prefill chunks are 48 rows, its decode batches 3 at the most
        m._mxfp4_kernel_max_t = 16
        ref.cfg, ref.cos_sin, ref.embed = m.cfg, m.cos_sin, m.embed
        ref.final_norm, ref.lm_head = m.final_norm, m.lm_head
        ref.layers = m.dense_layers()

    res = ec.run("A", "cuda:0", setup=setup, ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A mxfp4w|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    n_dec = sum(r.is_decode for r in res.rec.records)
    per_pass = 4 * ec.CONFIG.num_layers
    assert len([t for t in calls["linear"] if t <= 3]) >= n_dec * per_pass
    assert calls["dequant"] >= per_pass and max(calls["linear"]) <= 16
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst
