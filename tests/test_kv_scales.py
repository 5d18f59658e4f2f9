"""CPU tier of the fp8 KV-scale feature: the calibration helper, the pool's
scale bookkeeping (validation, digest, JSON round trip), the torch
reference's dequantisation, the engine entry points, and the P/D hand-off
check. The kernels themselves are judged in tests/test_gpu_kv_scales.py."""
import json
import math

import pytest
import torch

from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.engine.kvcache import (KVPool,
                                                          scales_from_amax)
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.ops import ref

FP8 = torch.float8_e4m3fn


def fp8_pool(num_blocks=4):
    return KVPool(TINY_LLAMA, num_blocks, torch.device("cpu"),
                  dtype=torch.float32, cache_dtype=FP8)


def some_scales(gen_seed=0):
    g = torch.Generator().manual_seed(gen_seed)
    shape = (TINY_LLAMA.num_layers, TINY_LLAMA.num_kv_heads)
    # arbitrary positive fp32 values, not powers of two: the round trip has
    # to keep every mantissa bit
    k = torch.rand(shape, generator=g) * 3 + 1e-3
    v = torch.exp(torch.randn(shape, generator=g) * 4)
    return k, v


# ---- scales_from_amax -----------------------------------------------------

AMAX = [1e-30, 1e-6, 0.1, 0.874, 1.0, 3.5, 7.0, 112.0, 224.0, 224.0001,
        447.9, 448.0, 448.1, 1e4, 3e38]


@pytest.mark.parametrize("headroom", [1.0, 2.0, 3.7])
def test_scales_from_amax_bounds(headroom):
    amax = torch.tensor(AMAX, dtype=torch.float64)
    s = scales_from_amax(amax, headroom)
    assert s.dtype == torch.float32 and s.shape == amax.shape
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())                   # powers of two
    x = amax * headroom / s.double()
    assert bool((x <= 448.0).all()), x
    assert bool((2 * x > 448.0).all()), x


def test_scales_from_amax_default_headroom_is_two():
    amax = torch.tensor([[1.0, 224.0], [448.0, 100.0]])
    assert torch.equal(scales_from_amax(amax), scales_from_amax(amax, 2.0))
    # 224 * 2 / 448 == 1 exactly: a power of two maps to itself
    assert scales_from_amax(torch.tensor([224.0])).item() == 1.0
    assert scales_from_amax(torch.tensor([448.0])).item() == 2.0
    assert scales_from_amax(torch.tensor([225.0])).item() == 2.0


def test_scales_from_amax_zero_gives_one():
    s = scales_from_amax(torch.tensor([0.0, 5.0, 0.0]))
    assert s[0].item() == 1.0 and s[2].item() == 1.0
    assert s[1].item() == 2.0 ** math.ceil(math.log2(5.0 * 2 / 448))


def test_scales_from_amax_rejects_bad_input():
    with pytest.raises(ValueError):
        scales_from_amax(torch.tensor([-1.0]))
    with pytest.raises(ValueError):
        scales_from_amax(torch.tensor([float("nan")]))
    with pytest.raises(ValueError):
        scales_from_amax(torch.tensor([1.0]), headroom=0.0)


# ---- KVPool bookkeeping ---------------------------------------------------

def test_pool_scales_views_and_inverse():
    pool = fp8_pool()
    assert pool.scales is None and pool.inv_scales is None
    assert pool.layer_scales(0) == (None, None, None, None)
    assert pool.all_layer_scales() is None
    k, v = some_scales()
    pool.set_scales(k, v)
    L, KVH = TINY_LLAMA.num_layers, TINY_LLAMA.num_kv_heads
    assert pool.scales.shape == (L, 2, KVH)
    assert pool.scales.dtype == torch.float32
    assert torch.equal(pool.scales[:, 0], k)
    assert torch.equal(pool.scales[:, 1], v)
    assert torch.equal(pool.inv_scales, 1.0 / pool.scales)
    for li in range(L):
        ks, vs, ki, vi = pool.layer_scales(li)
        assert torch.equal(ks, k[li]) and torch.equal(vs, v[li])
        assert torch.equal(ki, 1.0 / k[li]) and torch.equal(vi, 1.0 / v[li])
        assert ks.is_contiguous() and vi.is_contiguous()
    pool.set_scales(None, None)
    assert pool.scales is None and pool.scales_id == ""


def test_pool_set_scales_validates():
    pool = fp8_pool()
    k, v = some_scales()
    with pytest.raises(ValueError, match="shape"):
        pool.set_scales(k[:, :1], v)
    bad = k.clone()
    bad[0, 0] = 0.0
    with pytest.raises(ValueError, match="> 0"):
        pool.set_scales(bad, v)
    bad[0, 0] = -1.0
    with pytest.raises(ValueError, match="> 0"):
        pool.set_scales(k, bad)
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError):
        pool.set_scales(bad, v)
    assert pool.scales is None                      # nothing half-installed
    bf16 = KVPool(TINY_LLAMA, 4, torch.device("cpu"), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fp8"):
        bf16.set_scales(k, v)


def test_scales_id():
    pool, other = fp8_pool(), fp8_pool()
    assert pool.scales_id == ""
    k, v = some_scales()
    pool.set_scales(k, v)
    other.set_scales(k.clone(), v.clone())
    sid = pool.scales_id
    assert sid and sid == pool.scales_id == other.scales_id
    assert len(sid) == 16 and int(sid, 16) >= 0
    k2 = k.clone()
    k2[-1, -1] = torch.nextafter(k2[-1, -1], torch.tensor(10.0))
    other.set_scales(k2, v)
    assert other.scales_id != sid
    # K and V are not interchangeable
    other.set_scales(v, k)
    assert other.scales_id != sid


def test_scales_json_round_trip(tmp_path):
    pool = fp8_pool()
    k, v = some_scales(3)
    pool.set_scales(k, v)
    path = str(tmp_path / "scales.json")
    pool.save_scales(path)
    with open(path) as f:
        doc = json.load(f)
    assert sorted(doc) == ["k", "v"]
    assert len(doc["k"]) == TINY_LLAMA.num_layers
    assert len(doc["k"][0]) == TINY_LLAMA.num_kv_heads
    fresh = fp8_pool()
    fresh.load_scales(path)
    assert torch.equal(fresh.scales.view(torch.int32),
                       pool.scales.view(torch.int32))       # bit for bit
    assert torch.equal(fresh.inv_scales.view(torch.int32),
                       pool.inv_scales.view(torch.int32))
    assert fresh.scales_id == pool.scales_id


def test_scales_json_wrong_shape_names_both(tmp_path):
    pool = fp8_pool()
    L, KVH = TINY_LLAMA.num_layers, TINY_LLAMA.num_kv_heads
    path = str(tmp_path / "wrong.json")
    with open(path, "w") as f:
        json.dump({"k": [[1.0] * (KVH + 1)] * L,
                   "v": [[1.0] * (KVH + 1)] * L}, f)
    with pytest.raises(ValueError) as e:
        pool.load_scales(path)
    assert str((L, KVH + 1)) in str(e.value)
    assert str((L, KVH)) in str(e.value)
    assert pool.scales is None
    with pytest.raises(ValueError):
        fp8_pool().save_scales(str(tmp_path / "none.json"))


# ---- the torch reference --------------------------------------------------

def test_ref_paged_attention_scales_equal_premultiplied_cache():
    g = torch.Generator().manual_seed(5)
    B, KVH, qpg, D, BS, NB = 3, 2, 4, 64, 16, 12
    seq_lens = torch.tensor([1, 37, 64], dtype=torch.int32)
    q = torch.randn(B, KVH * qpg, D, generator=g)
    k_cache = (torch.randn(NB, KVH, BS, D, generator=g) * 50).clamp(
        -448, 448).to(FP8)
    v_cache = (torch.randn(NB, KVH, BS, D, generator=g) * 50).clamp(
        -448, 448).to(FP8)
    bt = (torch.randperm(NB, generator=g)[:B * 4].view(B, 4)).to(torch.int32)
    k_scale = torch.tensor([0.7, 2.0 ** -3])
    v_scale = torch.tensor([5.0, 0.37])
    got = ref.paged_attention(q, k_cache, v_cache, bt, seq_lens, D ** -0.5,
                              k_scale=k_scale, v_scale=v_scale)
    k_pre = k_cache.float() * k_scale.view(1, -1, 1, 1)
    v_pre = v_cache.float() * v_scale.view(1, -1, 1, 1)
    want = ref.paged_attention(q, k_pre, v_pre, bt, seq_lens, D ** -0.5)
    assert torch.allclose(got, want, rtol=1e-6, atol=0.0)
    # and the scales do something: swapping the heads' scales differs
    swapped = ref.paged_attention(q, k_cache, v_cache, bt, seq_lens,
                                  D ** -0.5, k_scale=k_scale.flip(0),
                                  v_scale=v_scale.flip(0))
    assert not torch.allclose(swapped, want, rtol=1e-3, atol=0.0)


def test_ref_reshape_and_cache_scaled():
    g = torch.Generator().manual_seed(6)
    T, KVH, D, BS, NB = 5, 2, 16, 4, 3
    k = (torch.randn(T, KVH, D, generator=g) * 300).bfloat16()
    v = (torch.randn(T, KVH, D, generator=g) * 300).bfloat16()
    kc = torch.zeros(NB, KVH, BS, D).to(FP8)
    vc = torch.zeros(NB, KVH, BS, D).to(FP8)
    slots = torch.tensor([3, -1, 0, 11, 6])
    k_inv = 1.0 / torch.tensor([4.0, 0.25])
    v_inv = 1.0 / torch.tensor([1.7, 100.0])
    ref.reshape_and_cache(k, v, kc, vc, slots, k_inv_scale=k_inv,
                          v_inv_scale=v_inv)
    for t, s in enumerate(slots.tolist()):
        if s < 0:
            continue
        want_k = (k[t].float() * k_inv.view(-1, 1)).clamp(-448, 448).to(FP8)
        want_v = (v[t].float() * v_inv.view(-1, 1)).clamp(-448, 448).to(FP8)
        assert torch.equal(kc[s // BS, :, s % BS].view(torch.uint8),
                           want_k.view(torch.uint8))
        assert torch.equal(vc[s // BS, :, s % BS].view(torch.uint8),
                           want_v.view(torch.uint8))
    assert bool((kc[0, :, 1].float() == 0).all())   # slot 1 never written
    assert bool(torch.isfinite(kc.float()).all())   # clamped, not NaN


# ---- engine ---------------------------------------------------------------

def run(worker, n_steps=60):
    toks = []
    for _ in range(n_steps):
        for o in worker.step():
            toks.extend(o.new_tokens)
        if not worker.has_work:
            break
    return toks


def test_cpu_worker_accepts_and_ignores_kv_scales():
    w = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=32, dtype=torch.float32,
                     kv_cache_dtype="fp8", kv_scales="calibrate")
    assert w.pool.cache_dtype == torch.float32      # fp8 needs the GPU
    assert w.pool.scales is None and w.pool.scales_id == ""
    w.add_request(EngineRequest("a", list(range(5, 45)), max_tokens=5))
    toks = run(w)
    assert len(toks) == 5
    plain = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=32,
                         dtype=torch.float32)
    plain.add_request(EngineRequest("a", list(range(5, 45)), max_tokens=5))
    assert run(plain) == toks


def test_set_kv_scales_raises_with_request_in_flight():
    w = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=32, dtype=torch.float32)
    w.add_request(EngineRequest("a", list(range(5, 45)), max_tokens=4))
    with pytest.raises(RuntimeError, match="idle"):
        w.set_kv_scales(1.0, 1.0)
    w.step()                                        # prefilled, decoding
    assert w.mgr.allocated_blocks > 0
    with pytest.raises(RuntimeError, match="idle"):
        w.set_kv_scales(1.0, 1.0)
    with pytest.raises(RuntimeError, match="idle"):
        w.calibrate_kv_scales()
    run(w)
    assert not w.has_work and w.mgr.allocated_blocks == 0
    # idle again: the call gets as far as the pool, which refuses scales
    # on a cache that is not fp8
    with pytest.raises(ValueError, match="fp8"):
        w.set_kv_scales(1.0, 1.0)


def test_new_scales_drop_cached_blocks_and_emit_evictions():
    w = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=32, dtype=torch.float32)
    prompt = list(range(5, 45))                     # two full blocks
    w.add_request(EngineRequest("a", prompt, max_tokens=2))
    run(w)
    stored, evicted = w.mgr.drain_events()
    assert len(stored) == 2 and not evicted
    w.set_kv_scales(None, None)                     # legal on any cache
    stored2, evicted2 = w.mgr.drain_events()
    assert not stored2 and sorted(evicted2) == sorted(stored)
    w.add_request(EngineRequest("b", prompt, max_tokens=2))
    run(w)
    assert w.mgr.cached_tokens_total == 0           # nothing was reused


# ---- P/D hand-off ---------------------------------------------------------

def handoff_node():
    from llm_d_inference_scheduler_amd.node import NodeConfig, NodeRunner
    node = NodeRunner(NodeConfig(model=TINY_LLAMA, world_size=1,
                                 topology="mono", device="cpu",
                                 dtype=torch.float32, kv_blocks=64))
    node.rank = 0
    calls = {"recv": [], "discard": []}
    node.transfer.recv_blocks = \
        lambda src, local, on_complete=None: calls["recv"].append(
            (src, list(local), on_complete))
    node.transfer.recv_discard = \
        lambda src, n, **kw: calls["discard"].append((src, n))
    return node, calls


def kv_job(**kw):
    job = {"type": "kv_ready", "req_id": "rx", "src": 1, "dst": 0,
           "blocks": [4, 5, 6], "seq_len": 40, "first_token": 7}
    job.update(kw)
    return job


@pytest.mark.parametrize("reserved", [False, True])
def test_handoff_with_foreign_scales_is_dropped(reserved):
    node, calls = handoff_node()
    mgr = node.engine.mgr
    free0 = mgr.free_blocks
    req = EngineRequest("rx", list(range(40)), max_tokens=4)
    node._pending_adoption["rx"] = {
        "req": req, "src": 1,
        "reserved": mgr.take_blocks(3) if reserved else None}
    node._start_kv_job(kv_job(kv_scales_id="00c0ffee00c0ffee"))
    done = [m for m in node._outbox if m.get("type") == "done"]
    assert len(done) == 1 and done[0]["req_id"] == "rx"
    assert done[0]["error"] == "kv_scale_mismatch"
    assert mgr.free_blocks == free0                 # nothing held or leaked
    assert "rx" not in node._pending_adoption
    assert "rx" not in mgr.tables
    # the staged transport still receives, into scratch, so the sender's
    # send has its partner
    assert calls["discard"] == [(1, 3)] and not calls["recv"]
    node.shutdown()


@pytest.mark.parametrize("job_kw", [{}, {"kv_scales_id": ""}])
def test_handoff_with_matching_scales_proceeds(job_kw):
    """An unscaled pool has id "", which is also what a kv_ready without
    the field means."""
    node, calls = handoff_node()
    mgr = node.engine.mgr
    free0 = mgr.free_blocks
    req = EngineRequest("rx", list(range(40)), max_tokens=4)
    node._pending_adoption["rx"] = {"req": req, "src": 1, "reserved": None}
    node._start_kv_job(kv_job(**job_kw))
    assert not [m for m in node._outbox if m.get("type") == "done"]
    assert len(calls["recv"]) == 1 and not calls["discard"]
    src, local, on_complete = calls["recv"][0]
    assert src == 1 and len(local) == 3
    assert mgr.free_blocks == free0 - 3
    on_complete()
    assert mgr.tables["rx"] == local
    node.shutdown()


def test_kv_ready_carries_scales_id():
    from llm_d_inference_scheduler_amd.engine.worker import RequestOutput
    node, _ = handoff_node()
    node._handle_outputs([RequestOutput(
        request_id="p", new_tokens=[1], kind="prefill_done",
        kv_blocks=[1, 2], seq_len=20, first_token=1)])
    ready = [m for m in node._outbox if m.get("type") == "kv_ready"]
    assert len(ready) == 1
    assert ready[0]["kv_scales_id"] == node.engine.pool.scales_id == ""
    node.shutdown()
