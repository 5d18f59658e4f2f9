"""CPU proof of tests/lora_engine_cases.py: the bf16 CPU worker stays inside
each scenario's limit and reaches what the scenario is for, every fault the
GPU tier must catch moves the worst row by more than 10x the limit, and a
worker with adapters registered but unused computes what one without LoRA
computes, bit for bit."""
import pytest
import torch

import engine_cases as ec
import lora_engine_cases as lec
from llm_d_inference_scheduler_amd.engine import (EngineRequest, LoraAdapter,
                                                  adapter_hash_seed)

CHECKS = {"L1": lec.check_l1, "L2": lec.check_l2}


@pytest.fixture(scope="module")
def clean():
    return {name: lec.run(name, "cpu") for name in lec.SCENARIOS}


@pytest.mark.parametrize("name", list(lec.SCENARIOS))
def test_cpu_worker_inside_limit(name, clean):
    res = clean[name]
    worst = max(res.worst.values())
    print(f"LORA_ENGINE_CPU|{name}|{lec.limit(name):.3e}|{worst:.3e}")
    # The limit is 4x this very figure, so the CPU tier does not judge the
    # CPU worker by it; it bounds the limit, which must stay far enough
    # below 1 / 10 for the faults below to mean something.
    assert lec.limit(name) < 0.06
    CHECKS[name](res)
    ec.check_token_path(res.rec.records, res.hist, res.plens)


FAULTS = [("L1", "drop", dict(mutate=lec.drop_adapter)),
          ("L1", "other", dict(mutate=lec.other_adapter)),
          ("L1", "decode", dict(mutate=lec.decode_without_adapter)),
          ("L1", "base_prefix", dict(patch_seed=True)),
          ("L2", "drop", dict(mutate=lec.drop_adapter)),
          ("L2", "decode", dict(mutate=lec.decode_without_adapter))]


@pytest.mark.parametrize("name,fault,kw", FAULTS,
                         ids=[f"{n}-{f}" for n, f, _ in FAULTS])
def test_fault_exceeds_ten_times_limit(name, fault, kw):
    res = lec.run(name, "cpu", **kw)
    assert max(res.worst.values()) > 10 * lec.limit(name), res.worst
    # requests on the base model never notice
    base = [rid for rid, r in res.reqs.items() if not r.adapter]
    if fault != "base_prefix":
        assert all(res.worst[rid] <= lec.limit(name) for rid in base)


def _scenario_a_logits(max_loras):
    sc = ec.SCENARIOS["A"]()
    if max_loras:
        worker = lec.make_worker("cpu", max_loras, **sc["worker"])
    else:
        worker = ec.make_worker("cpu", **sc["worker"])
    rec, _ = ec.run_scenario(worker, sc["arrivals"])
    return [r.logits for r in rec.records]


def test_unused_adapters_change_nothing():
    with_lora, without = _scenario_a_logits(2), _scenario_a_logits(0)
    assert len(with_lora) == len(without)
    assert all(torch.equal(a, b) for a, b in zip(with_lora, without))


def test_unknown_adapter_is_rejected_and_metrics_name_adapters():
    worker = lec.make_worker("cpu", 2, kv_blocks=64)
    worker.add_request(EngineRequest("x", [1, 2, 3], adapter="nope"))
    out = worker.step()
    assert out and out[0].error.startswith("adapter_not_found")
    worker.add_request(EngineRequest("y", lec.Y, max_tokens=4, adapter="p"))
    m = worker.metrics_snapshot()
    assert m.waiting_models == {"p": 1} and m.max_active_models == 2
    worker.step()
    assert worker.metrics_snapshot().active_models == {"p": 1}
    with pytest.raises(RuntimeError):
        worker.unregister_adapter("p")
    plain = ec.make_worker("cpu", kv_blocks=64)
    assert plain.lora is None and plain.metrics_snapshot().max_active_models == 0
    plain.add_request(EngineRequest("z", [1, 2, 3], adapter="p"))
    assert plain.step()[0].error.startswith("adapter_not_found")


def test_adapter_save_load_and_hash_seed(tmp_path):
    ad = lec.adapters()["p"]
    path = str(tmp_path / "p.pt")
    ad.save(path)
    back = LoraAdapter.load(path)
    assert back.name == "p" and back.content_id == ad.content_id
    assert lec.adapters()["q"].content_id != ad.content_id
    from llm_d_inference_scheduler_amd.engine.kvcache import block_hashes
    import inspect
    default = inspect.signature(block_hashes).parameters["seed"].default
    assert adapter_hash_seed("") == default
    assert len({adapter_hash_seed(n) for n in ("", "p", "q")}) == 3
