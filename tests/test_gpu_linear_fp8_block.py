"""ops.quantize_groups_fp8 and ops.linear_fp8_block on the device
(DEVELOPMENT.md "fp8 block scales") against ops.ref and float64."""
import functools

import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# As in test_gpu_linear_fp8_a8: the coefficient of (|x| @ |w|^T) in units of
# 2^-23 is twice the worst measured error of one fp8 MFMA, and K where K is
# larger. It carries over: the instruction's error is relative to its own
# sum of magnitudes, which after scaling is the dequantised sum of
# magnitudes of its group; the multiply and fused add per group and the wave
# and split sums are fp32 operations counted under K.
MFMA_COEFF = 2 * 1718
SKINNY = 1


@functools.lru_cache(maxsize=None)
def _case(T, n_in, n_out, seed=0):
    """x [T, in] bf16 and a block-scaled weight (CPU tensors) whose scales
    matter: K group g of W is scaled by 2^-a_g and of x by 2^+a_g, a_g from
    -6 to 6, so every group contributes alike to y while neighbouring scales
    differ by orders of magnitude; output channels run from 2^-3.5 to about
    2^12, two octaves within a 128-row block and the rest between blocks.
    With five rows, row 2 is zero, row 1 has a zero group and row 3 its
    absmax in its last element (the 64-wide tail's, where there is one)."""
    gen = torch.Generator().manual_seed(seed)
    G = -(-n_in // 128)
    a = torch.linspace(-6, 6, G).repeat_interleave(128)[:n_in]
    n = torch.arange(n_out)
    chan = torch.linspace(-3.5, 10, -(-n_out // 128))[n // 128] + \
        (n % 128) / 64.0
    W = torch.randn(n_in, n_out, generator=gen) * torch.exp2(-a)[:, None] * \
        torch.exp2(chan)
    wq, scale = ref.quantize_weight_fp8_block(W.to(torch.bfloat16))
    x = torch.randn(T, n_in, generator=gen) * torch.exp2(a) * \
        (1 + torch.arange(T, dtype=torch.float32) % 7)[:, None]
    if T == 5:
        x[2] = 0
        x[1, :128] = 0
        x[3, -1] = 64 * 2.0 ** float(a[-1])
    return x.to(torch.bfloat16), wq, scale


def _spans(t, dim):
    """max / min of a tensor of scales along dim, at its widest."""
    return float((t.amax(dim) / t.amin(dim)).max())


# in: the 64-wide tail group alone; one group + tail; many + tail; no tail
# and enough groups (128) that a row spans four workgroups.
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n_in", [64, 192, 2112, 16384])
def test_quantiser_matches_ref_bytes(T, n_in):
    x = _case(T, n_in, 16, seed=3)[0]
    xq_ref, sx_ref = ref.quantize_groups_fp8(x)
    if T == 5:
        assert int(x[3, -64:].float().abs().argmax()) == 63
        assert bool((sx_ref[2] == 1).all()) and float(sx_ref[1, 0]) == 1
    if n_in > 64:
        assert _spans(sx_ref[:1], 1) >= 2.0 ** 10
    xq, sx = ops.quantize_groups_fp8(x.to(DEV))
    assert xq.dtype == torch.float8_e4m3fn and sx.dtype == torch.float32
    assert torch.equal(sx.cpu(), sx_ref)
    assert torch.equal(xq.cpu().view(torch.uint8), xq_ref.view(torch.uint8))


# kernel: 1 the skinny kernel, 64 / 128 a tile, forced through the raw
# binding where the serving rule (linear_fp8_block_kernel_for) picks
# another; every case also runs as served. in: 64 the zero-filled tail
# alone; 192 one group + tail; 2112 many + tail; 3072 no tail. out: 16 below
# a block; 144 crosses the 128-row scale boundary with masked columns; 1040
# many.
# Skinny: T 1, 5 (the zero row and zero group of _case), 16 (MB 1), 17
# (MB 2), 33, 64 (MB 4), 65 (a second row tile).
# By linear_fp8_block_k_splits, in = 2112 and 3072 are split in two at
# every out here, in = 64 and 192 are not split. At those sizes a wave has
# at most three groups, fewer than two ring depths, so every stage is
# checked against the wave's count. The steady-state ring (pre-loaded, with
# unchecked refills) needs 2 DEPTH groups a wave: at out = 16 K splits in
# eight, so (1, 32768) is 8 groups a wave at depth 4, (33, 16384) 4 at depth
# 2, and (17, 28736) 8, 7, 7, 7 (the last split 6, 6, 5, 5 with the tail
# group) at depth 3: steady rounds followed by a partial one.
# Tiles: T 1, 63 below a tile; 65 across the small one; 129 across the large
# one; 257 two large tiles past. (257, 64, 11008) is 3 x 86 = 258 large
# tiles, where the fill rule of linear_fp8_a8_tile picks 128; the block rule
# keeps the 64 tile there by measurement (profiles/linear_fp8_block.md), so
# the last two cases run that shape as served and with 128 forced.
@pytest.mark.parametrize("T,n_in,n_out,kernel", [
    (1, 64, 16, SKINNY), (1, 3072, 1040, SKINNY), (5, 2112, 144, SKINNY),
    (16, 192, 144, SKINNY), (16, 2112, 144, SKINNY),
    (17, 2112, 16, SKINNY), (17, 192, 1040, SKINNY),
    (33, 3072, 144, SKINNY), (33, 64, 1040, SKINNY), (64, 2112, 1040, SKINNY),
    (64, 64, 144, SKINNY), (65, 192, 1040, SKINNY), (65, 3072, 16, SKINNY),
    (1, 32768, 16, SKINNY), (33, 16384, 16, SKINNY), (17, 28736, 16, SKINNY),
    (1, 192, 16, 64), (63, 2112, 144, 64), (65, 2112, 16, 64),
    (129, 3072, 144, 64), (257, 64, 1040, 64), (257, 2112, 144, 64),
    (1, 3072, 1040, 64), (65, 192, 1040, 64), (129, 64, 16, 64),
    (63, 3072, 1040, 64),
    (1, 192, 16, 128), (63, 2112, 144, 128), (129, 64, 1040, 128),
    (257, 3072, 144, 128), (65, 2112, 1040, 128), (129, 192, 16, 128),
    (1, 3072, 144, 128), (257, 64, 11008, 0), (257, 64, 11008, 128)])
def test_linear_against_float64(T, n_in, n_out, kernel):
    x, wq, scale = _case(T, n_in, n_out)
    if scale.shape[0] > 1:
        assert _spans(scale, 0) >= 2.0 ** 10
    xq, sx = ref.quantize_groups_fp8(x)
    if scale.shape[1] > 1:
        assert _spans(scale, 1) >= 2.0 ** 10 and _spans(sx, 1) >= 2.0 ** 10
    x64 = xq.double() * sx.double().repeat_interleave(128, 1)[:, :n_in]
    w64 = wq.double() * ref.expand_fp8_block_scale(scale.double(), n_out, n_in)
    y64 = x64 @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + max(n_in, MFMA_COEFF) * 2.0 ** -23 * (
        x64.abs() @ w64.abs().t())
    xd, wd, sd = x.to(DEV), wq.to(DEV), scale.to(DEV)
    for k in sorted({0, kernel}):
        y = ops.hip_ops().linear_fp8_block(xd, wd, sd, k)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, n_out)
        excess = ((y.cpu().double() - y64).abs() - bound).max()
        print(f"LINEAR_FP8_BLOCK|T={T} in={n_in} out={n_out} kernel={k}"
              f"|excess={float(excess):.3e}")
        assert float(excess) <= 0


@functools.lru_cache(maxsize=None)
def _full(kernel, T, n_in, n_out):
    x, wq, scale = (t.to(DEV) for t in _case(T, n_in, n_out, seed=1))
    return x, wq, scale, ops.hip_ops().linear_fp8_block(x, wq, scale, kernel)


# The deep shape runs the skinny kernel's steady-state ring at depth 2 in
# the full launch (MB 4) and at depth 4 in the one-row launch (MB 1).
@pytest.mark.parametrize("kernel,T,n_in,n_out,r", [
    (k, 257, 2112, 144, r) for k in (SKINNY, 64, 128)
    for r in (0, 63, 64, 256)] + [
    (SKINNY, 33, 32768, 16, 0), (SKINNY, 33, 32768, 16, 32)])
def test_row_invariance(kernel, T, n_in, n_out, r):
    x, wq, scale, full = _full(kernel, T, n_in, n_out)
    one = ops.hip_ops().linear_fp8_block(x[r:r + 1].clone(), wq, scale,
                                         kernel)
    assert torch.equal(full[r:r + 1], one)


@pytest.mark.parametrize("bad", ["in=32", "out=8", "1-D scale",
                                 "scale a block row short", "bf16 wq",
                                 "cpu scale"])
def test_contract_rejects(bad):
    n_in, n_out = (32 if bad == "in=32" else 64), (8 if bad == "out=8" else 16)
    x = torch.zeros(2, n_in, dtype=torch.bfloat16, device=DEV)
    wq = torch.zeros(n_out, n_in, device=DEV).to(
        torch.bfloat16 if bad == "bf16 wq" else torch.float8_e4m3fn)
    shape = {"1-D scale": (1,), "scale a block row short": (0, 1)}.get(
        bad, (1, 1))
    scale = torch.ones(shape, device="cpu" if bad == "cpu scale" else DEV)
    with pytest.raises(RuntimeError):
        ops.linear_fp8_block(x, wq, scale)


def test_no_rows():
    x, wq, scale = (t.to(DEV) for t in _case(1, 64, 16))
    assert tuple(ops.linear_fp8_block(x[:0], wq, scale).shape) == (0, 16)
    xq, sx = ops.quantize_groups_fp8(x[:0])
    assert tuple(xq.shape) == (0, 64) and tuple(sx.shape) == (0, 1)
