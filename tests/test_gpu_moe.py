"""ops.moe_route and ops.moe_ffn on the device (DEVELOPMENT.md "Mixture of
experts") against float64 (moe_cases)."""
import pytest
import torch

import moe_cases as mc
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("T,H,E,k", mc.ROUTE_CASES)
@pytest.mark.parametrize("renorm", [True, False])
def test_route_against_float64(T, H, E, k, renorm):
    x, router = mc.route_case(T, H, E, DEV)
    ids, w = ops.moe_route(x, router, k, renorm)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert tuple(ids.shape) == (T, k) and tuple(w.shape) == (T, k)
    mc.check_route(ids, w, x, router, k, renorm)


@pytest.fixture(scope="module")
def mb4():
    """The 130-row case and its batch result, shared and left unchanged."""
    case = mc.ffn_case("mb4", DEV)
    return case, ops.moe_ffn(*case)


@pytest.mark.parametrize("name", list(mc.FFN_CASES))
def test_ffn_against_float64(name):
    case = mc.ffn_case(name, DEV)
    y = ops.moe_ffn(*case)
    assert y.dtype == torch.bfloat16 and y.shape == case[0].shape
    excess = mc.ffn_excess(y, *case)
    print(f"MOE_FFN|{name}|excess={excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(mb4, r):
    (x, w13, w2, ids, w), full = mb4
    one = ops.moe_ffn(x[r:r + 1].clone(), w13, w2, ids[r:r + 1].clone(),
                      w[r:r + 1].clone())
    assert torch.equal(full[r:r + 1], one)


def test_repeatable(mb4):
    case, full = mb4
    scratch = torch.empty(ops.moe_scratch_bytes(130, 2, 4, 64, 48),
                          dtype=torch.uint8, device=DEV)
    assert torch.equal(ops.moe_ffn(*case), full)
    assert torch.equal(ops.moe_ffn(*case, scratch), full)


@pytest.mark.parametrize("bad", ["k=9", "E=300", "H=48", "int64 ids", "cpu w"])
def test_contract_rejects(bad):
    E, k = (300 if bad == "E=300" else 16), (9 if bad == "k=9" else 2)
    H = 48 if bad == "H=48" else 64
    x = torch.zeros(4, H, dtype=torch.bfloat16, device=DEV)
    w13 = torch.zeros(E, 32, H, dtype=torch.bfloat16, device=DEV)
    w2 = torch.zeros(E, H, 16, dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(4, k, device=DEV, dtype=torch.int64
                      if bad == "int64 ids" else torch.int32)
    w = torch.ones(4, k, device="cpu" if bad == "cpu w" else DEV)
    with pytest.raises(RuntimeError):
        ops.hip_ops().moe_ffn(x, w13, w2, ids, w)
    if bad in ("k=9", "E=300", "H=48"):
        with pytest.raises(RuntimeError):
            ops.hip_ops().moe_route(x, w13[:, 0].contiguous(), k, True)


def test_no_rows():
    x, w13, w2, ids, w = mc.ffn_case("one", DEV)
    assert tuple(ops.moe_ffn(x[:0], w13, w2, ids[:0], w[:0]).shape) == (0, 64)
    ids0, w0 = ops.moe_route(x[:0], w13[:, 0].contiguous(), 1, True)
    assert tuple(ids0.shape) == (0, 1) and tuple(w0.shape) == (0, 1)
