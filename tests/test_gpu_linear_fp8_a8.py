"""ops.quantize_rows_fp8 and ops.linear_fp8_a8 on the device (DEVELOPMENT.md
"fp8 activations") against ops.ref and float64."""
import functools

import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The coefficient of (|x| @ |w|^T) in the bound, in units of 2^-23. The
# bound of test_gpu_linear_fp8 has K there, for K fp32 additions. The fp8
# MFMA does not sum its 128 products that well: one
# v_mfma_scale_f32_16x16x128_f8f6f4 on its own, against float64, is off by
# up to 1718 * 2^-23 of sum_k |a_k b_k| (uniform random e4m3 codes; 158 to
# 198 for gaussian rows scaled to absmax 448; profiles/linear_fp8_a8.md).
# That error is relative to the instruction's own sum of magnitudes, so over
# the slabs of a row it adds up to the same fraction of the whole sum and
# does not grow with K; the fp32 additions between instructions (K / 128 of
# them) are far below it. The coefficient is twice the instruction's worst
# measured figure, and K where K is larger. The three in = 64 cases with
# out >= 1040 fail under K alone (by up to 2.0 at |y| of about 2^17),
# and only by this term: every other case passes under it.
MFMA_COEFF = 2 * 1718


def _case(T, n_in, n_out, seed=0):
    """As _case of test_gpu_linear_fp8: x [T, in] bf16 whose rows differ in
    magnitude, and an fp8 weight whose channel scales run from about 2^-10
    to 2^4 (CPU tensors)."""
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(n_in, n_out, generator=gen) * \
        torch.exp2(torch.linspace(-3.5, 12, n_out))
    wq, scale = ref.quantize_weight_fp8(W.to(torch.bfloat16))
    x = torch.randn(T, n_in, generator=gen) * \
        (1 + torch.arange(T, dtype=torch.float32) % 7)[:, None]
    return x.to(torch.bfloat16), wq, scale


# in: one chunk a thread for eight threads, held chunks with idle threads,
# every held chunk (16384 = 256 threads * 8 chunks * 8), and the re-read
# loop past them (25600). With five rows, row 2 is zero and row 3 has its
# absmax in its last element.
@pytest.mark.parametrize("T,n_in", [
    (1, 64), (5, 64), (1, 2112), (5, 2112), (1, 16384), (5, 16384),
    (5, 25600)])
def test_quantiser_matches_ref_bytes(T, n_in):
    x = _case(T, n_in, 16, seed=3)[0]
    if T == 5:
        x[2] = 0
        x[3, -1] = 64.0
        assert int(x[3].float().abs().argmax()) == n_in - 1
    xq, sx = ops.quantize_rows_fp8(x.to(DEV))
    xq_ref, sx_ref = ref.quantize_rows_fp8(x)
    assert xq.dtype == torch.float8_e4m3fn and sx.dtype == torch.float32
    assert torch.equal(sx.cpu(), sx_ref)
    assert torch.equal(xq.cpu().view(torch.uint8), xq_ref.view(torch.uint8))


# The tiles are 64 x 64 and 128 x 128 over 128-byte K slabs. tile 0 is what
# serves (64 at all of these sizes but the last), tile 128 forces the large
# one through the raw binding. T: 1, 63 below a tile; 65 across the small
# one; 129 two small tiles past and across the large one; 257 two large
# tiles past. in: 64 the zero-filled tail alone; 192 one slab + tail; 2112
# many + tail; 3072 no tail, 24 slabs of steady-state double buffering. out:
# 16 below a tile; 144 no multiple of either (masked columns); 1040 many.
# (257, 64, 11008) is 3 x 86 = 258 large tiles: the one size here at which
# the serving rule itself picks 128.
@pytest.mark.parametrize("T,n_in,n_out,tile", [
    (1, 64, 16, 0), (63, 192, 144, 0), (65, 2112, 16, 0),
    (129, 3072, 144, 0), (257, 64, 1040, 0), (257, 2112, 144, 0),
    (1, 3072, 1040, 0), (65, 192, 1040, 0),
    (1, 192, 16, 128), (63, 2112, 144, 128), (129, 64, 1040, 128),
    (257, 3072, 144, 128), (65, 2112, 1040, 128), (257, 64, 11008, 0)])
def test_linear_against_float64(T, n_in, n_out, tile):
    x, wq, scale = _case(T, n_in, n_out)
    assert float(scale.min()) <= 2.0 ** -10 and float(scale.max()) >= 2.0 ** 4
    xd, wd, sd = x.to(DEV), wq.to(DEV), scale.to(DEV)
    y = ops.linear_fp8_a8(xd, wd, sd)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, n_out)
    if tile:  # the tile decides who computes an element, never its bits
        forced = ops.hip_ops().linear_fp8_a8(xd, wd, sd, tile)
        assert torch.equal(forced, y)
        y = forced
    xq, sx = ref.quantize_rows_fp8(x)
    x64 = xq.double() * sx.double()[:, None]
    w64 = wq.double() * scale.double()[:, None]
    y64 = x64 @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + max(n_in, MFMA_COEFF) * 2.0 ** -23 * (
        x64.abs() @ w64.abs().t())
    excess = ((y.cpu().double() - y64).abs() - bound).max()
    print(f"LINEAR_FP8_A8|T={T} in={n_in} out={n_out} tile={tile}"
          f"|excess={float(excess):.3e}")
    assert float(excess) <= 0


@functools.lru_cache(maxsize=None)
def _full():
    x, wq, scale = (t.to(DEV) for t in _case(257, 2112, 144, seed=1))
    return x, wq, scale, ops.linear_fp8_a8(x, wq, scale)


@pytest.mark.parametrize("r", [0, 63, 64, 256])
def test_row_invariance(r):
    x, wq, scale, full = _full()
    one = ops.linear_fp8_a8(x[r:r + 1].clone(), wq, scale)
    assert torch.equal(full[r:r + 1], one)


@pytest.mark.parametrize("bad", ["in=32", "out=8", "bf16 wq", "cpu scale"])
def test_contract_rejects(bad):
    n_in, n_out = (32 if bad == "in=32" else 64), (8 if bad == "out=8" else 16)
    x = torch.zeros(2, n_in, dtype=torch.bfloat16, device=DEV)
    wq = torch.zeros(n_out, n_in, device=DEV).to(
        torch.bfloat16 if bad == "bf16 wq" else torch.float8_e4m3fn)
    scale = torch.ones(n_out, device="cpu" if bad == "cpu scale" else DEV)
    with pytest.raises(RuntimeError):
        ops.linear_fp8_a8(x, wq, scale)


def test_no_rows():
    x, wq, scale = (t.to(DEV) for t in _case(1, 64, 16))
    assert tuple(ops.linear_fp8_a8(x[:0], wq, scale).shape) == (0, 16)
    xq, sx = ops.quantize_rows_fp8(x[:0])
    assert tuple(xq.shape) == (0, 64) and tuple(sx.shape) == (0,)
