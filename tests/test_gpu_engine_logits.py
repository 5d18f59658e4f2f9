"""GPU tier of the engine logits tests: the worker's device path (flash
prefill, the decode kernels through dispatch, the fused QKV epilogue, the
device-resident decode state) against a float64 dense model of the same
weights (tests/engine_cases.py; DEVELOPMENT.md "Engine logits tests").
tests/test_engine_cases.py proves on the CPU that a position off by one, a
decode that misses its newest token, an ignored prior, a wrong slot or a
foreign block-table entry moves a row beyond 10x the limit asserted here, and
likewise for the faults of the prefill -> decode hand-off (H), of the
sampler's per-row state (S, by replaying every sampled token from its recorded
row) and of the QK-norm chain (Q).

Each test prints one `ENGINE|scenario|request|limit|worst` line per request
before it asserts (pytest -s shows them). The limit is 4x the worst row error
of the bf16 CPU worker on the same scenario."""
import functools

import pytest
import torch

import engine_cases as ec

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(name, fused=True, copy=None):
    if copy is not None:
        return ec.run(name, "cuda:0", torch.bfloat16, copy=copy)

    def setup(worker):
        worker.model._fused_qkv = fused
    return ec.run(name, "cuda:0", torch.bfloat16, setup=setup)


def judge(name, res, label=None):
    limit = ec.limit(name)
    for rid, worst in res.worst.items():
        print(f"ENGINE|{label or name}|{rid}|{limit:.3e}|{worst:.3e}")
    res.check_token_path()
    for rid, worst in res.worst.items():
        assert worst <= limit, (label or name, rid, worst, limit)


def test_mixed_traffic():
    """A: multi-sequence flash launches, continuation chunks with a prior,
    a prior out of the prefix cache, a one-token tail, the split decode
    kernel through dispatch, a decode batch of one long and two short
    rows, a block-table patch at a block edge."""
    res = run("A")
    assert res.worker.model._fused_qkv
    assert all(r.prefill_meta is not None
               for r in res.rec.records if not r.is_decode)
    ec.check_scenario_a(res)
    judge("A", res)


def test_row_reuse_and_growth():
    """B: decode-state rows taken over from longer requests, and a decode
    state that grows while its rows are live."""
    res = run("B")
    ec.check_scenario_b(res)
    judge("B", res)


def test_preemption_and_recompute():
    """C: a preempted request is recomputed from prompt plus output, and
    its logits afterwards match the dense model over the full history."""
    res = run("C")
    ec.check_scenario_c(res)
    judge("C", res)


def test_unfused_qkv_path_is_bit_equal():
    """D: scenario A through split / rope / reshape_and_cache. Same limit,
    and the logits of every call equal the fused run's bit for bit, as
    ops.dispatch.qkv_rope_cache documents."""
    chain = run("A", fused=False)
    assert not chain.worker.model._fused_qkv
    ec.check_scenario_a(chain)
    judge("A", chain, label="A unfused")
    fused = run("A")
    assert chain.hist == fused.hist
    assert len(chain.rec.records) == len(fused.rec.records)
    for rc, rf in zip(chain.rec.records, fused.rec.records):
        assert rc.rows == rf.rows and rc.spans == rf.spans
        assert torch.equal(rc.logits, rf.logits), (rc.step, rc.rows)


@pytest.mark.parametrize("copy", ["peer", "staged"])
def test_handoff(copy):
    """H: requests prefilled on one worker, their blocks copied by
    copy_blocks_peer or by a move_blocks gather and scatter into scattered
    blocks of a busy decode worker, adopted there and decoded on: a partial
    last block under the split kernel, a first decode token in a block the
    decode worker allocates, a transferred prefix reused from the prefix
    cache, and a seeded request drawn on both workers."""
    res = run("H", copy=copy)
    ec.check_scenario_h(res)
    judge("H", res, label=f"H {copy}")


def test_handoff_transports_are_bit_equal():
    """The two copies move the same bytes: equal histories, and logits
    equal bit for bit call by call, on both workers."""
    peer, staged = run("H", copy="peer"), run("H", copy="staged")
    assert peer.hist == staged.hist and peer.moves == staged.moves
    assert len(peer.records) == len(staged.records)
    for rp, rs in zip(peer.records, staged.records):
        assert rp.rows == rs.rows and rp.spans == rs.spans
        assert torch.equal(rp.logits, rs.logits), (rp.step, rp.rows)


def test_sampled_rows():
    """S: every token of a sampled request is what ops.ref.sample (or
    sample_ext over a rebuilt token state) draws from the recorded row
    with the request's own parameters, seed and completion index, through
    rows taken over from other requests, a growing decode state,
    preemption and recompute; greedy requests among them stay greedy."""
    res = run("S")
    ec.check_scenario_s(res)
    judge("S", res)


def test_qk_norm(monkeypatch):
    """Q: scenario A under QK-norm with gains that differ from each other
    and from 1. The config forces the unfused chain: the fused epilogue
    never runs, and rmsnorm sees the [T * H, 128] views of q and k of
    every call."""
    from llm_d_inference_scheduler_amd import ops
    norms, fused = [], []
    rmsnorm, qkv_rope_cache = ops.rmsnorm, ops.qkv_rope_cache

    def spy_norm(x, w, eps, **kw):
        norms.append(tuple(x.shape))
        return rmsnorm(x, w, eps, **kw)

    def spy_fused(*args, **kw):
        fused.append(1)
        return qkv_rope_cache(*args, **kw)
    monkeypatch.setattr(ops, "rmsnorm", spy_norm)
    monkeypatch.setattr(ops, "qkv_rope_cache", spy_fused)
    res = ec.run("Q", "cuda:0", torch.bfloat16)
    monkeypatch.undo()
    cfg = res.worker.cfg
    assert cfg.qk_norm and res.worker.model._fused_qkv and not fused
    for r in res.rec.records:
        T = r.input_ids.shape[0]
        for heads in (cfg.num_heads, cfg.num_kv_heads):
            assert norms.count((T * heads, 128)) >= cfg.num_layers, \
                (r.step, T, heads)
    ec.check_scenario_a(res)
    judge("Q", res)
