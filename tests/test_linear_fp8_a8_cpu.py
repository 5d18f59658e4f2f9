"""fp8 activations on the CPU path (DEVELOPMENT.md "fp8 activations"): the
per-row quantiser, ops.ref.linear_fp8_a8, the option's validation and a CPU
EngineWorker with fp8 weights and fp8 activations."""
import pytest
import torch

from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.ops import ref

T, IN, OUT = 9, 192, 48


def _rows():
    """[T, IN] bf16, row magnitudes from 2^-8 to 2^6, row 3 zero."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(T, IN, generator=gen) * \
        torch.exp2(torch.linspace(-8, 6, T))[:, None]
    x[3] = 0
    return x.to(torch.bfloat16)


def test_quantize_rows_round_trip():
    x = _rows()
    xq, sx = ref.quantize_rows_fp8(x)
    assert xq.dtype == torch.float8_e4m3fn and tuple(xq.shape) == (T, IN)
    assert sx.dtype == torch.float32 and tuple(sx.shape) == (T,)
    assert float(sx[3]) == 1.0 and not xq[3].float().any()
    assert torch.equal(sx[4], x[4].float().abs().max() / 448)
    q = xq.float()
    # e4m3's half ulp: 2^-4 relative, 2^-10 absolute below the normals
    bound = sx[:, None] * torch.maximum(q.abs() * 2.0 ** -4,
                                        torch.tensor(2.0 ** -10))
    assert bool(((x.float() - q * sx[:, None]).abs() <= bound).all())
    # the absmax element of every non-zero row maps to +-448
    live = [m for m in range(T) if m != 3]
    at = x.float().abs().argmax(dim=1)
    assert bool((q[live, at[live]].abs() == 448).all())


def test_ref_linear_against_float64():
    gen = torch.Generator().manual_seed(1)
    W = torch.randn(IN, OUT, generator=gen) * \
        torch.exp2(torch.linspace(-10, 4, OUT))
    wq, scale = ref.quantize_weight_fp8(W.to(torch.bfloat16))
    x = _rows()
    y = ops.linear_fp8_a8(x, wq, scale)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (T, OUT)
    xq, sx = ops.quantize_rows_fp8(x)
    x64 = xq.double() * sx.double()[:, None]
    w64 = wq.double() * scale.double()[:, None]
    y64 = x64 @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + IN * 2.0 ** -23 * (x64.abs()
                                                       @ w64.abs().t())
    assert bool(((y.double() - y64).abs() <= bound).all())


@pytest.mark.parametrize("weight_dtype", ["auto", "bf16", "mxfp4"])
def test_fp8_activations_need_fp8_weights(weight_dtype):
    with pytest.raises(ValueError, match='needs weight_dtype "fp8"'):
        EngineWorker(TINY_LLAMA, "cpu", kv_blocks=16,
                     weight_dtype=weight_dtype, activation_dtype="fp8")
    with pytest.raises(ValueError, match="unknown activation_dtype"):
        EngineWorker(TINY_LLAMA, "cpu", kv_blocks=16, activation_dtype="int8")


def test_cpu_worker_with_fp8_activations(monkeypatch):
    worker = EngineWorker(TINY_LLAMA, "cpu", kv_blocks=16, weight_dtype="fp8",
                          activation_dtype="fp8")
    assert worker.model.activation_dtype == "fp8"
    worker.model._fp8_kernel_max_t = 16   # the 20-row prefill is above it
    seen, a8 = [], ops.linear_fp8_a8
    monkeypatch.setattr(ops, "linear_fp8_a8", lambda x, wq, scale:
                        seen.append(x.shape[0]) or a8(x, wq, scale))
    worker.add_request(EngineRequest("r", prompt_tokens=list(range(3, 23)),
                                     max_tokens=3))
    outs = []
    for _ in range(16):
        outs.extend(worker.step())
        if not worker.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert fin and fin[0].completion_tokens == 3 and not fin[0].error
    assert seen == [20] * 4 * TINY_LLAMA.num_layers
