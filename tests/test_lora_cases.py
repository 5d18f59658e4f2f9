"""CPU proof of tests/lora_cases.py: the project's fp32 reference and the
rounding emulation stay inside every case's limit, and each fault a LoRA
kernel can plausibly have exceeds 10x that limit on every case that can show
it, so the GPU tier (tests/test_gpu_lora.py) fails on such a kernel."""
import pytest
import torch

import lora_cases as lc
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref


@pytest.mark.parametrize("name", lc.NAMES)
def test_reference_and_emulation_inside_limit(name):
    c = lc.build(name)
    assert c.limit < 0.05, "a limit this wide could not tell the mutants"
    assert c.emu_worst <= c.limit
    y = c.y0.clone()
    ops.lora_add(y, c.x, c.A, c.B, c.perm, c.tiles)   # CPU: ops.ref
    worst = float(lc.row_errors(y, c).max())
    print(f"LORA_REF|{name}|{c.limit:.3e}|{worst:.3e}")
    assert worst <= c.limit
    assert not torch.isnan(y.float()).any()
    rest = torch.ones(c.spec.T, dtype=torch.bool)
    rest[c.perm.long()] = False
    assert torch.equal(y[rest], c.y0[rest])


# the cases on which each mutant must be visible (elsewhere it may be a no-op)
MUST_SHOW = {
    "neighbour_slot": lc.NAMES,
    "perm_ignored": [n for n in lc.NAMES if n != "a_T1"],
    "tail_row_dropped": lc.NAMES,
    "last_split_dropped": lc.NAMES,
    "upper_R_dropped": [n for n in lc.NAMES if n != "f_rank8_R16"],
    "column_block_shifted": lc.NAMES,
}


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_mutant_exceeds_ten_times_limit(mutant):
    for name in lc.NAMES:
        c = lc.build(name)
        y = lc.emulate(c, mutant)
        if y is None:
            assert name not in MUST_SHOW[mutant], (mutant, name)
            continue
        assert name in MUST_SHOW[mutant], (mutant, name)
        worst = float(lc.row_errors(y, c).max())
        assert worst > lc.MUTANT_FACTOR * c.limit, (mutant, name, worst,
                                                    c.limit)


def test_long_k_case_has_several_splits():
    c = lc.build("d_longK")
    assert c.spec.n_in // lc.KCHUNK >= 2
    # dropping only the last split must still be caught, not just "all of K"
    y = lc.emulate(c, "last_split_dropped")
    worst = float(lc.row_errors(y, c).max())
    assert lc.MUTANT_FACTOR * c.limit < worst < 0.9


def test_worklist():
    perm, tiles = ops.lora_worklist([2, -1, 0, 0, 2, 1] + [0] * 16)
    assert perm.dtype == tiles.dtype == torch.int32
    assert perm.tolist() == [2, 3] + list(range(6, 22)) + [5, 0, 4]
    assert tiles.tolist() == [[0, 16, 0], [16, 2, 0], [18, 1, 1], [19, 2, 2]]
    perm, tiles = ops.lora_worklist([-1, -1])
    assert perm.shape == (0,) and tiles.shape == (0, 3)
    assert ref.lora_worklist([])[1].shape == (0, 3)


def test_single_row_matches_full_launch_on_reference():
    """What the GPU tier asserts bit for bit, on the CPU reference."""
    c = lc.build("c_T40_mixed")
    y = c.y0.clone()
    ops.lora_add(y, c.x, c.A, c.B, c.perm, c.tiles)
    for row in c.perm.tolist()[:4]:
        x1, y1, p1, t1 = lc.single_row(c, row)
        ops.lora_add(y1, x1, c.A, c.B, p1, t1)
        assert torch.equal(y1[0], y[row])
