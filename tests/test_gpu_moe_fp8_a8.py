"""ops.moe_ffn_fp8_a8 on the device (DEVELOPMENT.md "Mixture of experts")
under the two-stage float64 bound of moe_fp8_a8_cases."""
import pytest
import torch

import moe_fp8_a8_cases as a8c
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _act_out(args):
    T, k, I = args[0].shape[0], args[5].shape[1], args[1].shape[1] // 2
    return torch.full((T * k, I), float("nan"), dtype=torch.bfloat16,
                      device=DEV)


@pytest.fixture(scope="module")
def tall():
    """The 130-row case and its batch result, shared and left unchanged."""
    args = [a.to(DEV) for a in a8c.build("tall", "cpu")[0]]
    return args, ops.moe_ffn_fp8_a8(*args)


@pytest.mark.parametrize("name", list(a8c.CASES))
def test_ffn_against_float64(name):
    cpu_args, dense = a8c.build(name, "cpu")
    args = [a.to(DEV) for a in cpu_args]
    if name == "scales":    # neighbouring output rows differ in their scale
        assert float((args[2][:, 1:] != args[2][:, :-1]).float().mean()) > 0.5
    act_out = _act_out(args)
    y = ops.moe_ffn_fp8_a8(*args, act_out=act_out)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    # judged on the CPU: the kernels' quantiser has the bytes of the CPU's
    # ref.quantize_rows_fp8, which torch's own division on the device misses
    e1, e2 = a8c.excess(y.cpu(), act_out.cpu(), cpu_args, dense)
    print(f"MOE_FFN_FP8_A8|{name}|act={e1:.3e}|y={e2:.3e}")
    assert e1 <= 0 and e2 <= 0
    # the tile decides who computes an element, never its bits
    for tile in (64, 128):
        forced_act = _act_out(args)
        forced = ops.hip_ops().moe_ffn_fp8_a8(*args, None, tile, forced_act)
        assert torch.equal(forced, y) and torch.equal(forced_act, act_out)


@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(tall, r):
    (x, *wts, ids, w), full = tall
    one = ops.moe_ffn_fp8_a8(x[r:r + 1].clone(), *wts, ids[r:r + 1].clone(),
                             w[r:r + 1].clone())
    assert torch.equal(full[r:r + 1], one)


def test_repeatable(tall):
    args, full = tall
    scratch = torch.empty(ops.moe_fp8_a8_scratch_bytes(130, 2, 4, 128, 128),
                          dtype=torch.uint8, device=DEV)
    assert torch.equal(ops.moe_ffn_fp8_a8(*args), full)
    assert torch.equal(ops.moe_ffn_fp8_a8(*args, scratch), full)
    assert torch.equal(
        ops.moe_ffn_fp8_a8(*args, scratch, act_out=_act_out(args)), full)


@pytest.mark.parametrize("bad", ["H=32", "I=48", "bf16 w13s", "cpu w2s",
                                 "act_out shape"])
def test_contract_rejects(bad):
    E, H, I = 4, 32 if bad == "H=32" else 64, 48 if bad == "I=48" else 64
    zeros = lambda *s, **kw: torch.zeros(*s, **{"device": DEV, **kw})
    f8 = torch.float8_e4m3fn
    x = zeros(4, H, dtype=torch.bfloat16)
    w13q = zeros(E, 2 * I, H, dtype=torch.uint8).view(f8)
    w13s = zeros(E, 2 * I, dtype=torch.bfloat16 if bad == "bf16 w13s"
                 else torch.float32)
    w2q = zeros(E, H, I, dtype=torch.uint8).view(f8)
    w2s = zeros(E, H, device="cpu" if bad == "cpu w2s" else DEV)
    ids = zeros(4, 2, dtype=torch.int32)
    w = zeros(4, 2) + 1
    act_out = zeros(8 if bad != "act_out shape" else 4, I,
                    dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.moe_ffn_fp8_a8(x, w13q, w13s, w2q, w2s, ids, w, act_out=act_out)


def test_no_rows():
    x, *wts, ids, w = (a.to(DEV) for a in a8c.build("one", "cpu")[0])
    y = ops.moe_ffn_fp8_a8(x[:0], *wts, ids[:0], w[:0])
    assert tuple(y.shape) == (0, 64)
