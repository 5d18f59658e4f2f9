"""Scenario A of engine_cases on the device through the MoE path (DEVELOPMENT.md
"Mixture of experts"). The worker is upcycled to 8 identical experts, 2 a
token, with renormalised weights: in exact arithmetic the MoE layer is the
dense FFN whichever experts the router picks, so the float64 dense model,
reading the weights snapshotted before the upcycling, judges it."""
import types

import pytest

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

# The worst row error of the bf16 CPU worker (ops.ref) on the same upcycled
# scenario, as measured (7.138e-3) and rounded up to two digits
CPU_WORST_MOE = 0.0072
LIMIT = ec.LIMIT_FACTOR * CPU_WORST_MOE


def upcycle(ref):
    def setup(worker):
        m = worker.model
        ref.cfg, ref.cos_sin, ref.embed = m.cfg, m.cos_sin, m.embed
        ref.final_norm, ref.lm_head = m.final_norm, m.lm_head
        ref.layers = m.dense_layers()
        m.upcycle_to_moe(8, 2)
    return setup


def test_scenario_a_moe(monkeypatch):
    calls = {"route": [], "ffn": []}
    route, ffn = ops.moe_route, ops.moe_ffn

    def spy_route(x, *a):
        calls["route"].append(x.is_cuda)
        return route(x, *a)

    def spy_ffn(x, *a):
        calls["ffn"].append(x.is_cuda and a[2].is_cuda)
        return ffn(x, *a)

    monkeypatch.setattr(ops, "moe_route", spy_route)
    monkeypatch.setattr(ops, "moe_ffn", spy_ffn)
    ref = types.SimpleNamespace()
    res = ec.run("A", "cuda:0", setup=upcycle(ref), ref_model=ref)
    for rid, worst in res.worst.items():
        print(f"ENGINE|A moe|{rid}|{LIMIT:.4f}|{worst:.3e}")
    ec.check_scenario_a(res)
    res.check_token_path()
    # every layer of every decode pass and every prefill pass
    n_calls = len(res.rec.records) * ec.CONFIG.num_layers
    assert any(r.is_decode for r in res.rec.records)
    assert any(not r.is_decode for r in res.rec.records)
    assert len(calls["route"]) == n_calls and all(calls["route"])
    assert len(calls["ffn"]) == n_calls and all(calls["ffn"])
    assert all(worst <= LIMIT for worst in res.worst.values()), res.worst
