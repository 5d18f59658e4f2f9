"""GPU tier of the engine logits tests: the worker's device path (flash
prefill, the decode kernels through dispatch, the fused QKV epilogue, the
device-resident decode state) against a float64 dense model of the same
weights (tests/engine_cases.py; DEVELOPMENT.md "Engine logits tests").
tests/test_engine_cases.py proves on the CPU that a position off by one, a
decode that misses its newest token, an ignored prior, a wrong slot or a
foreign block-table entry moves a row beyond 10x the limit asserted here.

Each test prints one `ENGINE|scenario|request|limit|worst` line per request
before it asserts (pytest -s shows them). The limit is 4x the worst row error
of the bf16 CPU worker on the same scenario."""
import functools

import pytest
import torch

import engine_cases as ec

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(name, fused=True):
    def setup(worker):
        worker.model._fused_qkv = fused
    return ec.run(name, "cuda:0", torch.bfloat16, setup=setup)


def judge(name, res, label=None):
    limit = ec.limit(name)
    for rid, worst in res.worst.items():
        print(f"ENGINE|{label or name}|{rid}|{limit:.3e}|{worst:.3e}")
    ec.check_token_path(res.rec.records, res.hist, res.plens)
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
