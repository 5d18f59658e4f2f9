"""LoRA adapters through the node, the router and the API (CPU, hermetic):
the adapter is chosen by the request's model name, /v1/models lists it, the
endpoint's metrics and lora-affinity-scorer see it, every place that hashes
prompt blocks seeds with it, and a P/D hand-off refuses KV computed under
other adapter content."""
import json

import pytest
import torch
import torch.multiprocessing as mp
from fastapi.testclient import TestClient

from llm_d_inference_scheduler_amd.engine import (EngineRequest, EngineWorker,
                                                  LoraAdapter,
                                                  adapter_hash_seed)
from llm_d_inference_scheduler_amd.engine.kvcache import block_hashes
from llm_d_inference_scheduler_amd.engine.lora import adapter_from_spec
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.models.tokenizer import HashTokenizer
from llm_d_inference_scheduler_amd.node import NodeConfig, NodeRunner
from llm_d_inference_scheduler_amd.plugins.scorers import (
    LoraAffinityScorer, PrecisePrefixCacheScorer)
from llm_d_inference_scheduler_amd.scheduling.types import (LLMRequest,
                                                            SchedulingContext)
from llm_d_inference_scheduler_amd.server import NodeService, build_app

# strong enough to move the argmax of the randomly initialised tiny model
SPEC_P = "random:rank=8,seed=11,std=0.5"
SPEC_Q = "random:rank=16,seed=12,std=0.5"
ADAPTERS = {"tiny-p": SPEC_P, "tiny-q": SPEC_Q}
# the tokenizer the node's in-process token producer uses
TOK = HashTokenizer(TINY_LLAMA.vocab_size)
PROMPT = "the quick brown fox jumps over the lazy dog again and again"


def node_config(**kw):
    return NodeConfig(model=TINY_LLAMA, world_size=1, topology="mono",
                      device="cpu", dtype=torch.float32, kv_blocks=256,
                      max_loras=2, max_lora_rank=16,
                      lora_adapters=dict(ADAPTERS), **kw)


def direct_tokens(prompt_tokens, adapter, max_tokens, seed=0):
    """What an EngineWorker alone generates, greedy."""
    w = EngineWorker(TINY_LLAMA, "cpu", dtype=torch.float32, kv_blocks=256,
                     seed=seed, max_loras=2, max_lora_rank=16)
    for name, spec in ADAPTERS.items():
        w.register_adapter(adapter_from_spec(name, spec, TINY_LLAMA))
    w.add_request(EngineRequest("d", prompt_tokens=list(prompt_tokens),
                                max_tokens=max_tokens, adapter=adapter))
    toks = []
    for _ in range(100):
        for o in w.step():
            assert not o.error, o
            toks.extend(o.new_tokens)
        if not w.has_work:
            break
    return toks


@pytest.fixture(scope="class")
def client():
    """Class-scoped: the service's stepping thread must not run beside the
    other tests."""
    # the direct engines run first, not beside the stepping thread
    for adapter in ("", "tiny-p", "tiny-q"):
        DIRECT[adapter] = direct_tokens(TOK(PROMPT), adapter, 6)
    service = NodeService(NodeRunner(node_config()))
    service.start()
    with TestClient(build_app(service, tokenizer=TOK)) as c:
        yield c
    service.stop()


DIRECT = {}     # adapter -> what a direct EngineWorker generates for PROMPT


def complete(client, model, max_tokens=6):
    r = client.post("/v1/completions", json={
        "model": model, "prompt": PROMPT, "max_tokens": max_tokens,
        "temperature": 0})
    assert r.status_code == 200, r.text
    return r.json()


class TestApi:
    def test_models_lists_adapters_with_parent(self, client):
        data = client.get("/v1/models").json()["data"]
        assert data[0]["id"] == "tiny-llama" and "parent" not in data[0]
        assert [(d["id"], d["parent"]) for d in data[1:]] == [
            ("tiny-p", "tiny-llama"), ("tiny-q", "tiny-llama")]

    def test_adapter_completion_matches_direct_engine(self, client):
        text = TOK.decode
        want_p, want_base = DIRECT["tiny-p"], DIRECT[""]
        assert want_p != want_base
        body = complete(client, "tiny-p")
        assert body["model"] == "tiny-p"          # responses echo req.model
        assert body["choices"][0]["text"] == text(want_p)
        assert complete(client, "tiny-q")["choices"][0]["text"] == \
            text(DIRECT["tiny-q"])
        assert complete(client, "tiny-llama")["choices"][0]["text"] == \
            text(want_base)

    def test_unregistered_name_is_answered_by_the_base_model(self, client):
        base = complete(client, "tiny-llama")["choices"][0]["text"]
        body = complete(client, "somebodys-fine-tune")
        assert body["choices"][0]["text"] == base


def test_metrics_and_lora_affinity_see_the_local_engine():
    node = NodeRunner(node_config())
    ep = node.datastore.get_endpoint("gpu0")
    req = LLMRequest(request_id="m1", model="tiny-p",
                     prompt_tokens=list(range(100, 140)), prompt="x",
                     max_tokens=12)
    ctx = SchedulingContext(request=LLMRequest(
        request_id="next", model="tiny-p", prompt="x"))
    scorer = LoraAffinityScorer()
    # idle: a free slot, nothing active
    node.step()
    assert ep.metrics.max_active_models == 2
    assert scorer.score(ctx, [ep]) == {"gpu0": 0.8}
    node.submit(req)
    seen_active = False
    done = []
    for _ in range(100):
        node.step()
        done.extend(node.drain_completions())
        if ep.metrics.active_models == {"tiny-p": 1}:
            seen_active = True
            assert ep.metrics.max_active_models == 2
            assert scorer.score(ctx, [ep]) == {"gpu0": 1.0}
        if done:
            break
    assert seen_active and done and not done[0].error
    assert done[0].tokens == direct_tokens(range(100, 140), "tiny-p", 12)
    node.shutdown()


def test_every_hash_site_seeds_with_the_adapter():
    toks = list(range(100, 164))
    base = [int(h) for h in block_hashes(toks, 16)]
    under_p = [int(h) for h in block_hashes(toks, 16,
                                            adapter_hash_seed("tiny-p"))]
    assert adapter_hash_seed("") != adapter_hash_seed("tiny-p") \
        != adapter_hash_seed("tiny-q")
    assert base != under_p
    # the precise scorer, as the node configures it
    scorer = PrecisePrefixCacheScorer()
    scorer.adapter_names = {"tiny-p", "tiny-q"}
    hashes = lambda model: scorer._hashes(SchedulingContext(
        request=LLMRequest(request_id="s", model=model, prompt="x",
                           prompt_tokens=toks)))
    assert hashes("tiny-p") == under_p
    assert hashes("tiny-llama") == base
    assert hashes("somebodys-fine-tune") == base
    # the node's shared-storage probe and the engine's admission
    node = NodeRunner(node_config())
    probe = lambda adapter: [int(h) for h in node._probe_hashes(
        EngineRequest("x", prompt_tokens=toks, adapter=adapter))]
    assert probe("tiny-p") == under_p and probe("") == base
    req = EngineRequest("e", prompt_tokens=toks, max_tokens=1,
                        adapter="tiny-p")
    node.engine.add_request(req)
    node.engine.step()
    assert [int(h) for h in req.block_hashes] == under_p
    # the node handed the scorer its adapter names
    yaml = """
plugins:
  - type: precise-prefix-cache-scorer
  - type: max-score-picker
schedulingProfiles:
  - name: default
    plugins:
      - {pluginRef: precise-prefix-cache-scorer}
      - {pluginRef: max-score-picker}
"""
    node2 = NodeRunner(node_config(epp_yaml=yaml))
    assert node2._precise.adapter_names == {"tiny-p", "tiny-q"}
    node.shutdown()
    node2.shutdown()


def test_adapter_needs_slots_and_swap_is_refused():
    with pytest.raises(ValueError):
        NodeRunner(NodeConfig(model=TINY_LLAMA, world_size=1,
                              topology="mono", device="cpu",
                              dtype=torch.float32, kv_blocks=64,
                              lora_adapters={"tiny-p": SPEC_P}))
    w = EngineWorker(TINY_LLAMA, "cpu", dtype=torch.float32, kv_blocks=64,
                     max_loras=1)
    w.register_adapter(adapter_from_spec("a", SPEC_P, TINY_LLAMA))
    w.register_adapter(adapter_from_spec("a", SPEC_P, TINY_LLAMA))  # same
    with pytest.raises(ValueError):
        w.register_adapter(adapter_from_spec(
            "a", "random:rank=8,seed=99", TINY_LLAMA))
    # unregistering forgets cached KV, so a new "a" cannot match old blocks
    toks = list(range(100, 164))
    run = lambda rid: [w.add_request(EngineRequest(
        rid, prompt_tokens=toks, max_tokens=1, adapter="a"))] and \
        [o for _ in range(5) for o in w.step() if o.finished][0]
    assert run("one").cached_tokens == 0
    assert run("two").cached_tokens > 0
    w.unregister_adapter("a")
    w.register_adapter(adapter_from_spec("a", "random:rank=8,seed=99",
                                         TINY_LLAMA))
    assert run("three").cached_tokens == 0


def test_save_load_round_trips_content_id(tmp_path):
    ad = adapter_from_spec("tiny-p", SPEC_P, TINY_LLAMA)
    path = str(tmp_path / "p.pt")
    ad.save(path)
    assert LoraAdapter.load(path).content_id == ad.content_id
    assert adapter_from_spec("other-name", path, TINY_LLAMA).content_id == \
        ad.content_id
    from llm_d_inference_scheduler_amd.server.__main__ import (parse_args,
                                                               parse_lora_args)
    args = parse_args(["--max-loras", "2", "--max-lora-rank", "32",
                       "--lora", "tiny-p=" + SPEC_P, "--lora", "f=" + path])
    assert args.max_loras == 2 and args.max_lora_rank == 32
    assert parse_lora_args(args.lora) == {"tiny-p": SPEC_P, "f": path}


# ---- world-2 P/D ------------------------------------------------------------

EPP_YAML_TIGHT_DISAGG = """
plugins:
  - type: decode-filter
  - type: prefill-filter
  - type: queue-scorer
  - type: max-score-picker
  - type: prefix-based-pd-decider
    parameters: {nonCachedTokens: 16}
  - type: disagg-profile-handler
    parameters:
      pdDecider: prefix-based-pd-decider
schedulingProfiles:
  - name: decode
    plugins:
      - {pluginRef: decode-filter}
      - {pluginRef: queue-scorer, weight: 1}
      - {pluginRef: max-score-picker}
  - name: prefill
    plugins:
      - {pluginRef: prefill-filter}
      - {pluginRef: queue-scorer, weight: 1}
      - {pluginRef: max-score-picker}
"""


def _pd_worker(rank, world_size, init_file, out_file):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{init_file}",
                            rank=rank, world_size=world_size)
    try:
        # tiny-p is the same adapter on both ranks; the decode rank holds
        # other content under the name tiny-q
        adapters = {"tiny-p": SPEC_P,
                    "tiny-q": SPEC_Q if rank == 0
                    else "random:rank=16,seed=77,std=0.5"}
        cfg = NodeConfig(model=TINY_LLAMA, rank=rank, world_size=world_size,
                         topology="pd:1p1d", device="cpu",
                         dtype=torch.float32, kv_blocks=256,
                         epp_yaml=EPP_YAML_TIGHT_DISAGG, seed=3,
                         max_loras=2, lora_adapters=adapters)
        node = NodeRunner(cfg)
        results = []
        if rank == 0:
            for rid, model in (("rp", "tiny-p"), ("rq", "tiny-q"),
                               ("rb", "tiny-llama")):
                node.submit(LLMRequest(
                    request_id=rid, model=model, prompt="x " * 48,
                    prompt_tokens=list(range(100, 148)), max_tokens=4))
        for _ in range(300):
            node.step()
            if rank == 0:
                results.extend(node.drain_completions())
            flag = torch.tensor([1 if len(results) >= 3 else 0])
            dist.broadcast(flag, src=0)
            if flag.item():
                break
        if rank == 0:
            with open(out_file, "w") as f:
                json.dump({c.request_id: {"tokens": c.tokens,
                                          "error": c.error}
                           for c in results}, f)
        node.shutdown()
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_pd_handoff_checks_the_adapter_content(tmp_path):
    init_file, out_file = str(tmp_path / "pg"), str(tmp_path / "out.json")
    mp.start_processes(_pd_worker, args=(2, init_file, out_file), nprocs=2,
                       join=True, start_method="spawn")
    with open(out_file) as f:
        res = json.load(f)
    assert set(res) == {"rp", "rq", "rb"}
    toks = list(range(100, 148))
    assert not res["rp"]["error"]
    assert res["rp"]["tokens"] == direct_tokens(toks, "tiny-p", 4, seed=3)
    assert not res["rb"]["error"]
    assert res["rb"]["tokens"] == direct_tokens(toks, "", 4, seed=3)
    assert res["rp"]["tokens"] != res["rb"]["tokens"]
    assert res["rq"]["error"] == "adapter_mismatch"


def _pd_one_slot_worker(rank, world_size, init_file, out_file):
    """max_loras=1 with two adapters in flight: rp decodes for a while on the
    decode rank, rq's hand-off arrives meanwhile and finds no slot; once both
    are answered, rq2 finds the slot free."""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{init_file}",
                            rank=rank, world_size=world_size)
    try:
        cfg = NodeConfig(model=TINY_LLAMA, rank=rank, world_size=world_size,
                         topology="pd:1p1d", device="cpu",
                         dtype=torch.float32, kv_blocks=256,
                         epp_yaml=EPP_YAML_TIGHT_DISAGG, seed=3,
                         max_loras=1, lora_adapters=dict(ADAPTERS))
        node = NodeRunner(cfg)
        results, sent_late = [], False
        toks = list(range(100, 148))
        mk = lambda rid, model, n: LLMRequest(
            request_id=rid, model=model, prompt="x " * 48,
            prompt_tokens=toks, max_tokens=n)
        if rank == 0:
            node.submit(mk("rp", "tiny-p", 40))
            node.submit(mk("rq", "tiny-q", 4))
        for _ in range(600):
            node.step()          # must never raise, on either rank
            if rank == 0:
                results.extend(node.drain_completions())
                if len(results) == 2 and not sent_late:
                    node.submit(mk("rq2", "tiny-q", 4))
                    sent_late = True
            flag = torch.tensor([1 if len(results) >= 3 else 0])
            dist.broadcast(flag, src=0)
            if flag.item():
                break
        leaked = torch.tensor([node.engine.mgr.allocated_blocks
                               + len(node.engine._lora_pins)])
        dist.all_reduce(leaked)
        if rank == 0:
            with open(out_file, "w") as f:
                json.dump({"leaked": int(leaked),
                           "res": {c.request_id: {"tokens": c.tokens,
                                                  "error": c.error}
                                   for c in results}}, f)
        node.shutdown()
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_pd_handoff_without_a_free_slot_fails_cleanly(tmp_path):
    init_file, out_file = str(tmp_path / "pg"), str(tmp_path / "out.json")
    mp.start_processes(_pd_one_slot_worker, args=(2, init_file, out_file),
                       nprocs=2, join=True, start_method="spawn")
    with open(out_file) as f:
        out = json.load(f)
    res = out["res"]
    assert set(res) == {"rp", "rq", "rq2"}
    toks = list(range(100, 148))
    assert not res["rp"]["error"]
    assert res["rp"]["tokens"] == direct_tokens(toks, "tiny-p", 40, seed=3)
    assert res["rq"]["error"] == "lora_slots_busy"
    assert not res["rq2"]["error"]
    assert res["rq2"]["tokens"] == direct_tokens(toks, "tiny-q", 4, seed=3)
    # nothing stays taken on either rank: blocks, reservations, slot holds
    assert out["leaked"] == 0
