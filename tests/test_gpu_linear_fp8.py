"""ops.linear_fp8 and ops.dequant_fp8_weight on the device (DEVELOPMENT.md
"fp8 weights") against float64 and ops.ref."""
import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(T, n_in, n_out, seed=0):
    """x [T, in] bf16 whose rows differ in magnitude, and an fp8 weight
    whose channel scales run from about 2^-10 to 2^4 (CPU tensors)."""
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(n_in, n_out, generator=gen) * \
        torch.exp2(torch.linspace(-3.5, 12, n_out))
    wq, scale = ref.quantize_weight_fp8(W.to(torch.bfloat16))
    x = torch.randn(T, n_in, generator=gen) * \
        (1 + torch.arange(T, dtype=torch.float32) % 7)[:, None]
    return x.to(torch.bfloat16), wq, scale


# T: row-block and 64-row-tile edges; in: one K step, an uneven split across
# the four waves, past the workgroup split; out: below BN, no multiple of
# BN, many blocks. The last three reach the steady-state turns of the
# register ring, which need 2 * DEPTH K blocks a wave: in = 3072 is 24
# blocks a split (6 a wave, DEPTH 3 at T > 32), in = 16384 is 32 a split
# (8 a wave, DEPTH 4 at T <= 32).
@pytest.mark.parametrize("T,n_in,n_out", [
    (1, 64, 16), (1, 2112, 1040), (15, 192, 48), (17, 2112, 48),
    (17, 192, 1040), (64, 2112, 16), (64, 192, 1040), (65, 64, 48),
    (65, 2112, 1040), (130, 192, 16), (130, 2112, 48), (130, 64, 1040),
    (65, 3072, 48), (17, 16384, 48), (1, 16384, 48)])
def test_linear_against_float64(T, n_in, n_out):
    x, wq, scale = _case(T, n_in, n_out)
    assert float(scale.min()) <= 2.0 ** -10 and float(scale.max()) >= 2.0 ** 4
    y = ops.linear_fp8(x.to(DEV), wq.to(DEV), scale.to(DEV))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, n_out)
    w64 = wq.double() * scale.double()[:, None]
    y64 = x.double() @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + n_in * 2.0 ** -23 * (
        x.double().abs() @ w64.abs().t())
    excess = ((y.cpu().double() - y64).abs() - bound).max()
    print(f"LINEAR_FP8|T={T} in={n_in} out={n_out}|excess={float(excess):.3e}")
    assert float(excess) <= 0


# in = 3072: the T = 130 call takes the steady-state turns (DEPTH 3), the
# T = 1 call only the tail (DEPTH 4); in = 16384: both take them
@pytest.mark.parametrize("n_in", [2112, 3072, 16384])
@pytest.mark.parametrize("r", [0, 63, 64, 129])
def test_row_invariance(r, n_in):
    x, wq, scale = (t.to(DEV) for t in _case(130, n_in, 48, seed=1))
    full = ops.linear_fp8(x, wq, scale)
    one = ops.linear_fp8(x[r:r + 1].clone(), wq, scale)
    assert torch.equal(full[r:r + 1], one)


@pytest.mark.parametrize("n_in,n_out", [(64, 16), (192, 1040)])
def test_dequant_matches_ref(n_in, n_out):
    _, wq, scale = _case(1, n_in, n_out, seed=2)
    out = torch.empty(n_in, n_out, dtype=torch.bfloat16, device=DEV)
    ops.dequant_fp8_weight(wq.to(DEV), scale.to(DEV), out)
    assert torch.equal(out.cpu(), ref.dequant_fp8_weight(wq, scale))


@pytest.mark.parametrize("bad", ["in=32", "out=8", "bf16 wq", "cpu scale"])
def test_contract_rejects(bad):
    n_in, n_out = (32 if bad == "in=32" else 64), (8 if bad == "out=8" else 16)
    x = torch.zeros(2, n_in, dtype=torch.bfloat16, device=DEV)
    wq = torch.zeros(n_out, n_in, device=DEV).to(
        torch.bfloat16 if bad == "bf16 wq" else torch.float8_e4m3fn)
    scale = torch.ones(n_out, device="cpu" if bad == "cpu scale" else DEV)
    with pytest.raises(RuntimeError):
        ops.hip_ops().linear_fp8(x, wq, scale)


def test_no_rows():
    x, wq, scale = (t.to(DEV) for t in _case(1, 64, 16))
    assert tuple(ops.linear_fp8(x[:0], wq, scale).shape) == (0, 16)
