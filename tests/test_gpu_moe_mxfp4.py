"""ops.moe_ffn_mxfp4 on the device (DEVELOPMENT.md "Mixture of experts")
against float64 on the exactly dequantised experts: the bound of moe_cases
applies unchanged, because every dequantised value is a bf16."""
import pytest
import torch

import moe_cases as mc
import moe_mxfp4_cases as mxc
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(name):
    return mxc.build(name, DEV)


@pytest.fixture(scope="module")
def tall():
    """The 130-row case and its batch result, shared and left unchanged."""
    args, _ = build("tall")
    return args, ops.moe_ffn_mxfp4(*args)


@pytest.mark.parametrize("name", list(mxc.CASES))
def test_ffn_against_float64(name):
    args, (w13, w2) = build(name)
    if name == "scales":    # neighbouring groups differ in their scale byte
        assert float((args[2][..., 1:] != args[2][..., :-1]).float().mean()) \
            > 0.5
    y = ops.moe_ffn_mxfp4(*args)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    excess = mc.ffn_excess(y, args[0], w13, w2, *args[5:])
    print(f"MOE_FFN_MXFP4|{name}|excess={excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(tall, r):
    (x, *wts, ids, w), full = tall
    one = ops.moe_ffn_mxfp4(x[r:r + 1].clone(), *wts, ids[r:r + 1].clone(),
                            w[r:r + 1].clone())
    assert torch.equal(full[r:r + 1], one)


def test_repeatable(tall):
    args, full = tall
    scratch = torch.empty(ops.moe_scratch_bytes(130, 2, 4, 128, 64,
                                                mxfp4=True),
                          dtype=torch.uint8, device=DEV)
    assert torch.equal(ops.moe_ffn_mxfp4(*args), full)
    assert torch.equal(ops.moe_ffn_mxfp4(*args, scratch), full)


@pytest.mark.parametrize("bad", ["int8 w13q", "groups of 16", "I=48",
                                 "cpu w13s", "w2q rows"])
def test_contract_rejects(bad):
    E, H, I = 4, 64, 48 if bad == "I=48" else 64
    u8 = lambda *s, **kw: torch.zeros(*s, **{"dtype": torch.uint8,
                                             "device": DEV, **kw})
    x = torch.zeros(4, H, dtype=torch.bfloat16, device=DEV)
    w13q = u8(E, 2 * I, H // 2,
              dtype=torch.int8 if bad == "int8 w13q" else torch.uint8)
    w13s = u8(E, 2 * I, H // (16 if bad == "groups of 16" else 32),
              device="cpu" if bad == "cpu w13s" else DEV)
    w2q = u8(E, H + 32 if bad == "w2q rows" else H, I // 2)
    w2s = u8(E, H, I // 32)
    ids = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    w = torch.ones(4, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ops.hip_ops().moe_ffn_mxfp4(x, w13q, w13s, w2q, w2s, ids, w)


def test_no_rows():
    (x, *wts, ids, w), _ = build("one_group")
    y = ops.moe_ffn_mxfp4(x[:0], *wts, ids[:0], w[:0])
    assert tuple(y.shape) == (0, 32)
