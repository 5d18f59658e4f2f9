"""ops.moe_ffn_fp8_block on the device (DEVELOPMENT.md "Mixture of experts")
under the two-stage float64 bound of moe_fp8_block_cases, as served and with
each kernel family forced (tile 16: the skinny kernels, 64: the LDS tiles)."""
import pytest
import torch

import moe_fp8_block_cases as bc
from llm_d_inference_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = (16, 64)


def _act_out(args):
    T, k, I = args[0].shape[0], args[5].shape[1], args[1].shape[1] // 2
    return torch.full((T * k, I), float("nan"), dtype=torch.bfloat16,
                      device=DEV)


def _forced(args, tile, scratch=None, act_out=None):
    return ops.hip_ops().moe_ffn_fp8_block(*args, scratch, tile, act_out)


@pytest.fixture(scope="module")
def tall():
    """The 130-row case and its result at each forced tile, shared and left
    unchanged."""
    args = [a.to(DEV) for a in bc.build("tall", "cpu")[0]]
    return args, {tile: _forced(args, tile) for tile in TILES}


@pytest.mark.parametrize("tile", (0,) + TILES)
@pytest.mark.parametrize("name", list(bc.CASES))
def test_ffn_against_float64(name, tile):
    cpu_args, dense = bc.build(name, "cpu")
    args = [a.to(DEV) for a in cpu_args]
    act_out = _act_out(args)
    y = _forced(args, tile, act_out=act_out) if tile else \
        ops.moe_ffn_fp8_block(*args, act_out=act_out)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    # judged on the CPU: the kernels' quantiser has the bytes of the CPU's
    # ref.quantize_groups_fp8, which torch's own division on the device misses
    e1, e2 = bc.excess(y.cpu(), act_out.cpu(), cpu_args, dense)
    print(f"MOE_FFN_FP8_BLOCK|{name}|{tile}|act={e1:.3e}|y={e2:.3e}")
    assert e1 <= 0 and e2 <= 0


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(tall, r, tile):
    (x, *wts, ids, w), full = tall
    one = _forced((x[r:r + 1].clone(), *wts, ids[r:r + 1].clone(),
                   w[r:r + 1].clone()), tile)
    assert torch.equal(full[tile][r:r + 1], one)


def test_repeatable(tall):
    args, full = tall
    scratch = torch.empty(ops.moe_fp8_block_scratch_bytes(130, 2, 4, 128, 128),
                          dtype=torch.uint8, device=DEV)
    # 130 * 2 / 4 rows an expert: served by the 64-row tiles
    assert torch.equal(ops.moe_ffn_fp8_block(*args), full[64])
    assert torch.equal(ops.moe_ffn_fp8_block(*args, scratch), full[64])
    for tile in TILES:
        assert torch.equal(_forced(args, tile, scratch, _act_out(args)),
                           full[tile])


@pytest.mark.parametrize("bad", ["H=32", "I=48", "2-D w13s", "merged w13s",
                                 "bf16 w13s", "cpu w2s", "act_out shape"])
def test_contract_rejects(bad):
    E, H = 4, 32 if bad == "H=32" else 64
    I = 48 if bad == "I=48" else 320 if bad == "merged w13s" else 64
    zeros = lambda *s, **kw: torch.zeros(*s, **{"device": DEV, **kw})
    f8 = torch.float8_e4m3fn
    nbi = -(-I // 128)
    x = zeros(4, H, dtype=torch.bfloat16)
    w13q = zeros(E, 2 * I, H, dtype=torch.uint8).view(f8)
    # blocked as the merged [2 I, H] matrix, I = 320 has 5 block rows, not 6
    s13 = (E, 2 * I) if bad == "2-D w13s" else \
        (E, 5, 1) if bad == "merged w13s" else (E, 2 * nbi, 1)
    w13s = zeros(*s13, dtype=torch.bfloat16 if bad == "bf16 w13s"
                 else torch.float32)
    w2q = zeros(E, H, I, dtype=torch.uint8).view(f8)
    w2s = zeros(E, 1, nbi, device="cpu" if bad == "cpu w2s" else DEV)
    ids = zeros(4, 2, dtype=torch.int32)
    w = zeros(4, 2) + 1
    act_out = zeros(8 if bad != "act_out shape" else 4, I,
                    dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.moe_ffn_fp8_block(x, w13q, w13s, w2q, w2s, ids, w,
                              act_out=act_out)


def test_no_rows():
    x, *wts, ids, w = (a.to(DEV) for a in bc.build("one", "cpu")[0])
    y = ops.moe_ffn_fp8_block(x[:0], *wts, ids[:0], w[:0])
    assert tuple(y.shape) == (0, 64)
