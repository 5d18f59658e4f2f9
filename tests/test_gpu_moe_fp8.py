"""ops.moe_ffn_fp8 on the device (DEVELOPMENT.md "Mixture of experts")
against float64 on the experts wq * scale: the bound of moe_cases applies
unchanged (moe_fp8_cases)."""
import pytest
import torch

import moe_cases as mc
import moe_fp8_cases as f8c
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tall():
    """The 130-row case and its batch result, shared and left unchanged."""
    args, _ = f8c.build("tall", DEV)
    return args, ops.moe_ffn_fp8(*args)


@pytest.mark.parametrize("name", list(f8c.CASES))
def test_ffn_against_float64(name):
    args, (w13, w2) = f8c.build(name, DEV)
    if name == "scales":    # neighbouring output rows differ in their scale
        assert float((args[2][:, 1:] != args[2][:, :-1]).float().mean()) > 0.5
    y = ops.moe_ffn_fp8(*args)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    excess = mc.ffn_excess(y, args[0], w13, w2, *args[5:])
    print(f"MOE_FFN_FP8|{name}|excess={excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(tall, r):
    (x, *wts, ids, w), full = tall
    one = ops.moe_ffn_fp8(x[r:r + 1].clone(), *wts, ids[r:r + 1].clone(),
                          w[r:r + 1].clone())
    assert torch.equal(full[r:r + 1], one)


def test_repeatable(tall):
    args, full = tall
    scratch = torch.empty(ops.moe_scratch_bytes(130, 2, 4, 128, 80),
                          dtype=torch.uint8, device=DEV)
    assert torch.equal(ops.moe_ffn_fp8(*args), full)
    assert torch.equal(ops.moe_ffn_fp8(*args, scratch), full)


@pytest.mark.parametrize("bad", ["uint8 w13q", "bf16 w13s", "I=24",
                                 "cpu w13s", "w2q rows", "w2s half"])
def test_contract_rejects(bad):
    E, H, I = 4, 64, 24 if bad == "I=24" else 32
    zeros = lambda *s, **kw: torch.zeros(*s, **{"device": DEV, **kw})
    f8 = torch.float8_e4m3fn
    x = zeros(4, H, dtype=torch.bfloat16)
    w13q = zeros(E, 2 * I, H, dtype=torch.uint8).view(
        torch.uint8 if bad == "uint8 w13q" else f8)
    w13s = zeros(E, 2 * I, device="cpu" if bad == "cpu w13s" else DEV,
                 dtype=torch.bfloat16 if bad == "bf16 w13s" else torch.float32)
    w2q = zeros(E, H + 32 if bad == "w2q rows" else H, I,
                dtype=torch.uint8).view(f8)
    w2s = zeros(E, H // 2 if bad == "w2s half" else H)
    ids = zeros(4, 2, dtype=torch.int32)
    w = zeros(4, 2) + 1
    with pytest.raises(RuntimeError):
        ops.hip_ops().moe_ffn_fp8(x, w13q, w13s, w2q, w2s, ids, w)


def test_no_rows():
    (x, *wts, ids, w), _ = f8c.build("one_group", DEV)
    y = ops.moe_ffn_fp8(x[:0], *wts, ids[:0], w[:0])
    assert tuple(y.shape) == (0, 32)
