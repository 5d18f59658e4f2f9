"""CPU proof of the engine logits oracle (tests/engine_cases.py;
DEVELOPMENT.md "Engine logits tests").

Every scenario of the GPU tier runs here on a CPU worker. In float32 the
engine's composed path must agree with the float64 dense model to float32
precision, which checks the reference itself. In bf16 (the ops.ref path) the
worst row error must stay within the committed CPU_WORST, from which the GPU
tier takes its limit. Then eight faults of the layer under test, each applied
to the batch on its way into the model, must each move the worst row of the
560-token request of scenario A beyond 10x that limit."""
import functools

import pytest
import torch

import engine_cases as ec


@functools.lru_cache(maxsize=None)
def clean(name, dtype):
    return ec.run(name, "cpu", dtype)


# ---- clean runs ----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ec.SCENARIOS))
def test_fp32_engine_matches_dense_reference(name):
    _, rec, hist, worst, plens = clean(name, torch.float32)
    print(f"ENGINE-CPU|{name}|fp32|{max(worst.values()):.3e}")
    assert max(worst.values()) < 1e-4, worst
    ec.check_token_path(rec.records, hist, plens)


@pytest.mark.parametrize("name", sorted(ec.SCENARIOS))
def test_bf16_engine_within_cpu_worst(name):
    _, rec, hist, worst, plens = clean(name, torch.bfloat16)
    print(f"ENGINE-CPU|{name}|bf16|{max(worst.values()):.3e}")
    assert max(worst.values()) <= ec.CPU_WORST[name], worst
    ec.check_token_path(rec.records, hist, plens)


def test_scenarios_reach_what_they_are_for():
    """The coverage each scenario claims, read from the records."""
    ec.check_scenario_a(clean("A", torch.bfloat16))
    ec.check_scenario_b(clean("B", torch.bfloat16))
    ec.check_scenario_c(clean("C", torch.bfloat16))


def test_reference_is_causal_and_unpaged():
    """dense_logits64 of a prefix equals the prefix of dense_logits64."""
    w = ec.make_worker("cpu", torch.float32, kv_blocks=8)
    toks = ec.long_prompt(70)
    full = ec.dense_logits64(w.model, toks)
    part = ec.dense_logits64(w.model, toks[:33])
    assert full.shape == (70, ec.CONFIG.vocab_size)
    assert full.dtype == torch.float64
    assert float((full[:33] - part).abs().max()) < 1e-12


def test_sharpen_gives_cpu_and_any_device_the_same_model():
    a = ec.make_worker("cpu", torch.bfloat16, kv_blocks=8).model
    b = ec.make_worker("cpu", torch.bfloat16, kv_blocks=8, seed=99).model
    assert torch.equal(a.embed, b.embed)
    assert torch.equal(a.lm_head, b.lm_head)
    for la, lb in zip(a.layers, b.layers):
        for key in la:
            assert torch.equal(la[key], lb[key]), key


# ---- mutants -------------------------------------------------------------

class Mutant:
    """A fault applied to the batch before the model sees it. `recorder` is
    set by the Recorder; recorder.current holds the call's spans."""
    recorder = None

    def __call__(self, batch):
        if batch.is_decode:
            self.decode(batch)
        else:
            self.prefill(batch)

    def decode(self, batch):
        pass

    def prefill(self, batch):
        pass


class DecodePositionsPlusOne(Mutant):
    def decode(self, batch):
        batch.positions = batch.positions + 1


class DecodeSeqLensMinusOne(Mutant):
    def decode(self, batch):
        batch.seq_lens = batch.seq_lens - 1


class DecodeSlotsMovedOneRow(Mutant):
    def decode(self, batch):
        batch.slot_mapping = torch.roll(batch.slot_mapping, 1)


class DecodeFirstBlocksSwapped(Mutant):
    def decode(self, batch):
        if batch.block_tables.shape[0] >= 2:
            bt = batch.block_tables.clone()
            bt[[0, 1], 0] = bt[[1, 0], 0]
            batch.block_tables = bt


class DecodeStaleInputIds(Mutant):
    def __init__(self):
        self.last = {}

    def decode(self, batch):
        ids = batch.input_ids.clone()
        for rid, _, _, row in self.recorder.current:
            now = int(ids[row])
            if rid in self.last:
                ids[row] = self.last[rid]
            self.last[rid] = now
        batch.input_ids = ids


class PrefillPriorIgnored(Mutant):
    def prefill(self, batch):
        s = batch.seq_starts
        batch.ctx_lens = [s[i + 1] - s[i] for i in range(len(s) - 1)]


class PrefillPositionsRestart(Mutant):
    def prefill(self, batch):
        pos = batch.positions.clone()
        for _, start, end, row in self.recorder.current:
            if start > 0:
                pos[row:row + end - start] = torch.arange(
                    end - start, dtype=pos.dtype)
        batch.positions = pos


class PrefillLastRowSlot(Mutant):
    def prefill(self, batch):
        slots = batch.slot_mapping.clone()
        for _, start, end, row in self.recorder.current:
            if end - start >= 2:
                last = row + end - start - 1
                slots[last] = slots[last - 1]
        batch.slot_mapping = slots


MUTANTS = [DecodePositionsPlusOne, DecodeSeqLensMinusOne,
           DecodeSlotsMovedOneRow, DecodeFirstBlocksSwapped,
           DecodeStaleInputIds, PrefillPriorIgnored, PrefillPositionsRestart,
           PrefillLastRowSlot]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_mutant_is_noticed_on_the_long_request(mutant):
    """Each fault moves the worst row of b, the 560-token request of
    scenario A, beyond 10x the limit the GPU tier asserts."""
    _, _, _, worst, _ = ec.run("A", "cpu", torch.bfloat16, mutate=mutant())
    bound = 10 * ec.limit("A")
    print(f"MUTANT|{mutant.__name__}|b|{bound:.3e}|{worst['b']:.3e}|"
          f"{worst['b'] / ec.limit('A'):.1f}x")
    assert worst["b"] > bound, (mutant.__name__, worst)


def test_limit_is_four_times_the_reference_path():
    for name in ec.SCENARIOS:
        assert ec.limit(name) == 4 * ec.CPU_WORST[name] > 0
