"""ops.linear_mxfp4 and ops.dequant_mxfp4_weight on the device
(DEVELOPMENT.md "MXFP4 weights") against float64 and ops.ref."""
import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref
from test_linear_mxfp4_cpu import mx_weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(T, n_in, n_out, seed=0):
    """x [T, in] bf16 whose rows differ in magnitude, and an mxfp4 weight
    whose group scales run over 2^-10 .. 2^4 and more along n and along k
    (CPU tensors)."""
    wq, scale = ref.quantize_weight_mxfp4(mx_weight(n_in, n_out, seed))
    x = torch.randn(T, n_in, generator=torch.Generator().manual_seed(seed)) \
        * (1 + torch.arange(T, dtype=torch.float32) % 7)[:, None]
    return x.to(torch.bfloat16), wq, scale


# A K block is 128 k, four waves take a split's blocks round-robin, K is
# split across workgroups from in = 4096, T <= 16 runs MB 1 / BN 32 / DEPTH 4
# and T > 16 MB 2 / BN 64 / DEPTH 3 over 32-row tiles; the ring's steady-state
# turns need 2 * DEPTH blocks a wave.
#   in = 128: one block, three waves idle; 384: one wave idle; 2176: 17
#   blocks, 5/4/4/4 a wave, all in the tail turns; 3072: 6 a wave, steady
#   state at DEPTH 3 only; 3840: 30 blocks, 8/8/7/7 a wave, steady state at
#   both depths for two waves and tail only (DEPTH 4) for the others; 4224:
#   two splits of 17 and 16 blocks; 7680: two splits of 30, steady state
#   behind a split.
#   out = 16: below BN; 48: no multiple of BN, a clamped column block at
#   BN 32 and at BN 64; 1040: 33 and 17 column blocks.
#   T = 1, 15: MB 1; 17: MB 2 with one row in the second block; 64: two full
#   tiles; 65, 130: a tile of one and of two rows at the end.
@pytest.mark.parametrize("T,n_in,n_out", [
    (1, 128, 16), (1, 2176, 1040), (15, 384, 48), (17, 2176, 48),
    (17, 384, 1040), (64, 2176, 16), (64, 384, 1040), (65, 128, 48),
    (65, 4224, 1040), (130, 384, 16), (130, 2176, 48), (130, 128, 1040),
    (65, 3072, 48), (17, 3840, 48), (1, 3840, 48), (15, 7680, 48)])
def test_linear_against_float64(T, n_in, n_out):
    x, wq, scale = _case(T, n_in, n_out)
    for s in (scale[:, 0], scale[0]):       # along n, along k
        assert int(s.min()) <= 127 - 10 and int(s.max()) >= 127 + 4
    assert len(torch.cat((wq & 15, wq >> 4)).unique()) == 16
    y = ops.linear_mxfp4(x.to(DEV), wq.to(DEV), scale.to(DEV))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, n_out)
    w64 = ref.dequant_mxfp4_weight(wq, scale, dtype=torch.float64)
    y64 = x.double() @ w64
    bound = 2.0 ** -8 * y64.abs() + n_in * 2.0 ** -23 * (
        x.double().abs() @ w64.abs())
    excess = ((y.cpu().double() - y64).abs() - bound).max()
    print(f"LINEAR_MXFP4|T={T} in={n_in} out={n_out}|"
          f"excess={float(excess):.3e}")
    assert float(excess) <= 0


# in = 2176: both calls stay in the tail turns; 3072: the T = 130 call takes
# the steady-state turns (DEPTH 3), the T = 1 call only the tail (DEPTH 4);
# 3840: both take them; 4224: behind the workgroup split
@pytest.mark.parametrize("n_in", [2176, 3072, 3840, 4224])
@pytest.mark.parametrize("r", [0, 31, 32, 129])
def test_row_invariance(r, n_in):
    x, wq, scale = (t.to(DEV) for t in _case(130, n_in, 48, seed=1))
    full = ops.linear_mxfp4(x, wq, scale)
    one = ops.linear_mxfp4(x[r:r + 1].clone(), wq, scale)
    assert torch.equal(full[r:r + 1], one)


# pins the nibble order of the convert instruction against the format's
@pytest.mark.parametrize("n_in,n_out", [(128, 16), (384, 1040)])
def test_dequant_matches_ref(n_in, n_out):
    _, wq, scale = _case(1, n_in, n_out, seed=2)
    out = torch.empty(n_in, n_out, dtype=torch.bfloat16, device=DEV)
    ops.dequant_mxfp4_weight(wq.to(DEV), scale.to(DEV), out)
    assert torch.equal(out.cpu(), ref.dequant_mxfp4_weight(wq, scale))


@pytest.mark.parametrize("bad", ["in=64", "out=8", "float8 wq",
                                 "scale shape", "cpu scale"])
def test_contract_rejects(bad):
    n_in, n_out = (64 if bad == "in=64" else 128), (8 if bad == "out=8"
                                                    else 16)
    x = torch.zeros(2, n_in, dtype=torch.bfloat16, device=DEV)
    wq = torch.zeros(n_out, n_in // 2, dtype=torch.uint8, device=DEV)
    if bad == "float8 wq":
        wq = wq.view(torch.float8_e4m3fn)
    scale = torch.full((n_out, n_in // (16 if bad == "scale shape" else 32)),
                       127, dtype=torch.uint8,
                       device="cpu" if bad == "cpu scale" else DEV)
    with pytest.raises(RuntimeError):
        ops.hip_ops().linear_mxfp4(x, wq, scale)


def test_no_rows():
    x, wq, scale = (t.to(DEV) for t in _case(1, 128, 16))
    assert tuple(ops.linear_mxfp4(x[:0], wq, scale).shape) == (0, 16)
