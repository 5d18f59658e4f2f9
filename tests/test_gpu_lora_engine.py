"""The LoRA engine scenarios of tests/lora_engine_cases.py on the device:
every logits row inside the scenario's limit against the float64 dense model
with the request's adapter merged in, the scenario's events reached, and a
worker whose adapters nobody uses bit-equal to one built without LoRA."""
import pytest
import torch

import engine_cases as ec
import lora_engine_cases as lec

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHECKS = {"L1": lec.check_l1, "L2": lec.check_l2}


@pytest.mark.parametrize("name", list(lec.SCENARIOS))
def test_scenario_inside_limit(name):
    res = lec.run(name, DEV)
    worst = max(res.worst.values())
    print(f"LORA_ENGINE|{name}|{lec.limit(name):.3e}|{worst:.3e}")
    assert worst <= lec.limit(name), res.worst
    CHECKS[name](res)
    ec.check_token_path(res.rec.records, res.hist, res.plens)


def _scenario_a_logits(max_loras):
    sc = ec.SCENARIOS["A"]()
    if max_loras:
        worker = lec.make_worker(DEV, max_loras, **sc["worker"])
    else:
        worker = ec.make_worker(DEV, **sc["worker"])
    rec, _ = ec.run_scenario(worker, sc["arrivals"])
    return [r.logits for r in rec.records]


def test_unused_adapters_change_nothing():
    with_lora, without = _scenario_a_logits(2), _scenario_a_logits(0)
    assert len(with_lora) == len(without)
    assert all(torch.equal(a, b) for a, b in zip(with_lora, without))
