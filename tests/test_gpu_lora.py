"""The batched LoRA kernels on the device against tests/lora_cases.py: every
case inside its limit, untouched rows bit-equal, no NaN read from a row or a
slot the work list does not name, and a row's bits independent of where it
sits in the launch."""
import pytest
import torch

import lora_cases as lc
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run(c, x, y0, perm, tiles):
    y = y0.to(DEV)
    ops.lora_add(y, x.to(DEV), c.A.to(DEV), c.B.to(DEV), perm.to(DEV),
                 tiles.to(DEV))
    return y.cpu()


@pytest.fixture(scope="module")
def results():
    cache = {}

    def get(name):
        if name not in cache:
            c = lc.build(name)
            cache[name] = run(c, c.x, c.y0, c.perm, c.tiles)
        return cache[name]
    return get


@pytest.mark.parametrize("name", lc.NAMES)
def test_case_inside_limit(name, results):
    c = lc.build(name)
    y = results(name)
    worst = float(lc.row_errors(y, c).max())
    print(f"LORA|{name}|{c.limit:.3e}|{worst:.3e}")
    assert worst <= c.limit
    assert not torch.isnan(y.float()).any()
    rest = torch.ones(c.spec.T, dtype=torch.bool)
    rest[c.perm.long()] = False
    assert torch.equal(y[rest].view(torch.int16),
                       c.y0[rest].view(torch.int16))


@pytest.mark.parametrize("name", ["b_T17", "c_T40_mixed"])
def test_row_bits_do_not_depend_on_the_launch(name, results):
    c = lc.build(name)
    y = results(name)
    for row in c.perm.tolist():
        x1, y1, p1, t1 = lc.single_row(c, row)
        alone = run(c, x1, y1, p1, t1)
        assert torch.equal(alone[0].view(torch.int16),
                           y[row].view(torch.int16)), row


def test_empty_worklist_is_a_noop():
    c = lc.build("c_T40_mixed")
    y = run(c, c.x, c.y0, torch.zeros(0, dtype=torch.int32),
            torch.zeros(0, 3, dtype=torch.int32))
    assert torch.equal(y.view(torch.int16), c.y0.view(torch.int16))
