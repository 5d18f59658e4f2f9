"""Scenario A of engine_cases on the device with block-scaled fp8 weights
(DEVELOPMENT.md "fp8 block scales"): the float64 dense model reads the
dequantised weights and full-precision activations, so what remains is
activation rounding, here with the e4m3 rounding of every row's 128-wide
groups in it."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

# The worst row error of the bf16 CPU worker (ops.ref) on scenario A with
# fp8_block weights, as measured (5.1441e-2) and rounded up to two digits
CPU_WORST_FP8_BLOCK = 0.052
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_FP8_BLOCK


def test_scenario_a_fp8_block(monkeypatch):
    calls = {"block": [], "other": 0}
    block = ops.linear_fp8_block

    def spy_block(x, wq, scale):
        calls["block"].append(x.shape[0])
        return block(x, wq, scale)

    def spy_other(*args, **kwargs):
        calls["other"] += 1
        raise AssertionError("an fp8_block runner left ops.linear_fp8_block")

    monkeypatch.setattr(ops, "linear_fp8_block", spy_block)
    for name in ("linear_fp8", "linear_fp8_a8", "dequant_fp8_weight"):
        monkeypatch.setattr(ops, name, spy_other)
    ref = types.SimpleNamespace()

    def setup(worker):
        m = worker.model
        m.quantize_weights("fp8_block")
        ref.cfg, ref.cos_sin, ref.embed = m.cfg, m.cos_sin, m.embed
        ref.final_norm, ref.lm_head = m.final_norm, m.lm_head
        ref.layers = m.dense_layers()

    res = ec.run("A", "cuda:0", setup=setup, ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A fp8_block|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    # every projection of every forward pass, prefill chunks (48 rows) and
    # decode batches (3 rows at the most) alike
    n_dec = sum(r.is_decode for r in res.rec.records)
    per_pass = 4 * ec.CONFIG.num_layers
    assert len(calls["block"]) % per_pass == 0
    assert len([t for t in calls["block"] if t <= 3]) >= n_dec * per_pass
    assert max(calls["block"]) > 16
    assert calls["other"] == 0 and not res.worker.model._fp8_scratch
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst
