"""The engine serving LoRA adapters, judged against a float64 dense model
with the adapter merged into the weights (DEVELOPMENT.md "LoRA adapters").

Built on tests/engine_cases.py: its config, sharpened weights, recorder and
dense_logits64. The oracle of a request under an adapter is dense_logits64
over a model whose four fused matrices are W + (B·A)ᵀ, A and B being the
bf16 tensors a slot holds (alpha / rank already folded into B), so the fold
and the rounding of the adapter are not sources of error.

The adapters are strong: A, B ~ N(0, STD^2) at ranks 8 and 16 change a
logits row by O(1) of its norm, so that dropping an adapter, applying another
request's, applying it in prefill only, or reusing KV computed under the base
model each move the worst row by more than 10x the limit
(tests/test_lora_engine_cases.py proves it on the CPU).
"""
import functools
from types import SimpleNamespace
from typing import Dict, List

import torch

import engine_cases as ec
from llm_d_inference_scheduler_amd.engine import EngineRequest
from llm_d_inference_scheduler_amd.engine import lora as lora_mod
from llm_d_inference_scheduler_amd.engine import worker as worker_mod
from llm_d_inference_scheduler_amd.engine.lora import LoraAdapter
from llm_d_inference_scheduler_amd.models.llama import LORA_TARGETS

STD = 0.12
POOL_RANK = 16


def adapters() -> Dict[str, LoraAdapter]:
    """p: rank 8 (zero-padded in the rank-16 pool), q: rank 16."""
    return {"p": LoraAdapter.random(ec.CONFIG, 8, seed=101, std=STD, name="p"),
            "q": LoraAdapter.random(ec.CONFIG, 16, seed=202, std=STD,
                                    name="q")}


def make_worker(device, max_loras, dtype=torch.bfloat16, **kw):
    worker = ec.make_worker(device, dtype, max_loras=max_loras,
                            max_lora_rank=POOL_RANK, **kw)
    for ad in adapters().values():
        worker.register_adapter(ad)
    return worker


def merged_model(model, adapter: LoraAdapter):
    """What dense_logits64 reads of a runner, with `adapter` merged in."""
    slots = adapter.pool_tensors(model.cfg, POOL_RANK, torch.bfloat16)
    layers = []
    for layer, slot in zip(model.layers, slots):
        merged = {k: v.detach().to("cpu", torch.float64)
                  for k, v in layer.items()}
        for t in LORA_TARGETS:
            A, B = slot[t]
            merged[t] = merged[t] + (B.double() @ A.double()).T
        layers.append(merged)
    return SimpleNamespace(cfg=model.cfg, layers=layers, embed=model.embed,
                           lm_head=model.lm_head,
                           final_norm=model.final_norm,
                           cos_sin=model.cos_sin)


def _req(rid, prompt, max_tokens, adapter=""):
    return EngineRequest(rid, prompt_tokens=list(prompt),
                         max_tokens=max_tokens, adapter=adapter)


X = ec.long_prompt(80, salt=3)
Y = ec.long_prompt(70, salt=5)


def scenario_l1():
    """max_loras=2. base and p1 prefill together in 48-token chunks, q1
    arrives one step later with p1's prompt (and base's: what a prefix cache
    that ignored the adapter would hand it). p2, again that prompt under p,
    arrives once p1's blocks are registered. All decode in one batch; 19
    blocks run out while they do, so one request is preempted and
    recomputed."""
    return dict(
        worker=dict(max_loras=2, kv_blocks=19, prefill_chunk_tokens=48),
        arrivals=[(0, _req("base", X, 24)),
                  (0, _req("p1", X, 24, "p")),
                  (1, _req("q1", X, 24, "q")),
                  (7, _req("p2", X, 6, "p"))])


def scenario_l2():
    """max_loras=1. pA runs; qB arrives with it and has no slot, so base2,
    arriving a step later, passes it. When pA ends q takes the slot (an
    eviction), and pC afterwards forces p's reload."""
    return dict(
        worker=dict(max_loras=1, kv_blocks=64, prefill_chunk_tokens=256),
        arrivals=[(0, _req("pA", Y, 6, "p")),
                  (0, _req("qB", X, 5, "q")),
                  (1, _req("base2", ec.long_prompt(40, salt=7), 12)),
                  (9, _req("pC", ec.long_prompt(50, salt=9), 5, "p"))])


SCENARIOS = {"L1": scenario_l1, "L2": scenario_l2}


@functools.lru_cache(maxsize=None)
def cpu_worst(name: str) -> float:
    """The worst row error of the bf16 CPU worker (ops.ref) on the scenario,
    run here and now (a fraction of a second): 9.8e-3 on L1 and 7.1e-3 on L2
    where this was written. A constant would tie the limit to one host's
    bf16 matmul, which moves such figures by a few percent."""
    return max(run(name, "cpu").worst.values())


def limit(name: str) -> float:
    """LIMIT_FACTOR times the bf16 CPU worker's worst row, as
    engine_cases.limit does it."""
    return ec.LIMIT_FACTOR * cpu_worst(name)


def run(name: str, device, dtype=torch.bfloat16, mutate=None,
        patch_seed=False) -> ec.Result:
    """Run a scenario on a fresh worker and judge every logits row against
    its request's merged float64 model. patch_seed: the fault of hashing
    every prompt with the base seed."""
    sc = SCENARIOS[name]()
    worker = make_worker(device, dtype=dtype, **sc["worker"])
    reqs = {r.request_id: r for _, r in sc["arrivals"]}
    plens = {rid: len(r.prompt_tokens) for rid, r in reqs.items()}
    real_seed = worker_mod.adapter_hash_seed
    if patch_seed:
        worker_mod.adapter_hash_seed = lambda name: lora_mod.BASE_HASH_SEED
    try:
        rec, hist = ec.run_scenario(worker, sc["arrivals"], mutate=mutate)
    finally:
        worker_mod.adapter_hash_seed = real_seed
    ads = adapters()
    models = {"": worker.model}
    models.update({n: merged_model(worker.model, a) for n, a in ads.items()})
    refs = {rid: ec.dense_logits64(models[reqs[rid].adapter], h)
            for rid, h in hist.items()}
    worst = ec.judge(rec.records, hist, worker.model, refs)
    return ec.Result(worker, rec, hist, worst, plens, reqs)


# ---- the faults (mutate hooks on the recorder) ------------------------------

def drop_adapter(batch):
    batch.lora = None


def decode_without_adapter(batch):
    if batch.is_decode:
        batch.lora = None


def other_adapter(batch):
    """Every tile reads the other slot (both are resident in L1)."""
    if batch.lora is not None:
        batch.lora.tiles = batch.lora.tiles.clone()
        batch.lora.tiles[:, 2] = 1 - batch.lora.tiles[:, 2]


# ---- what each scenario must have reached -----------------------------------

def first_outputs(res) -> Dict[str, int]:
    """Index into rec.outputs of each request's first token."""
    first = {}
    for i, o in enumerate(res.rec.outputs):
        if o.new_tokens:
            first.setdefault(o.request_id, i)
    return first


def check_l1(res) -> None:
    recs = res.rec.records
    pre = [r for r in recs if not r.is_decode]
    dec = [r for r in recs if r.is_decode]
    assert any({"base", "p1"} <= {s[0] for s in r.spans} for r in pre), \
        "base and p1 never shared a prefill pass"
    assert any({rid for rid, _ in r.rows} >= {"base", "p1", "q1"}
               for r in dec), "no decode batch mixing base, p and q"
    fin = {o.request_id: o for o in res.rec.outputs if o.finished}
    first_q1 = [o for o in res.rec.outputs
                if o.request_id == "q1" and o.new_tokens][0]
    assert first_q1.cached_tokens == 0, "q1 reused KV of another adapter"
    first_p2 = [o for o in res.rec.outputs
                if o.request_id == "p2" and o.new_tokens][0]
    assert first_p2.cached_tokens >= 64, "p2 missed p1's prefix"
    victims = [rid for rid, r in res.reqs.items()
               if r.prompt_len > r.orig_prompt_len]
    assert victims, "no request was preempted"
    # ... and one of them runs under an adapter, which it must keep through
    # the recompute (its rows after it are judged against the merged model)
    assert any(res.reqs[rid].adapter for rid in victims), victims
    assert all(len(res.hist[rid]) - res.plens[rid] == res.reqs[rid].max_tokens
               for rid in fin)
    assert res.worker.lora.loads == 2


def check_l2(res) -> None:
    first = first_outputs(res)
    assert first["base2"] < first["qB"], "base2 did not pass the waiting qB"
    assert first["pA"] < first["qB"] < first["pC"]
    # p, then q over it, then p again
    assert res.worker.lora.loads == 3
    fin = {o.request_id: o for o in res.rec.outputs if o.finished}
    assert set(fin) == {"pA", "qB", "base2", "pC"}
