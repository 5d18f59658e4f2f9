"""Weight-only fp8 on the CPU path (DEVELOPMENT.md "fp8 weights"): the
quantiser, ops.ref.linear_fp8 and an fp8-weights EngineWorker."""
import torch

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.ops import ref

IN, OUT = 192, 48


def _weight():
    """[IN, OUT] bf16, column magnitudes from 2^-10 to 2^4, column 5 zero."""
    gen = torch.Generator().manual_seed(0)
    W = torch.randn(IN, OUT, generator=gen) * \
        torch.exp2(torch.linspace(-10, 4, OUT))
    W[:, 5] = 0
    return W.to(torch.bfloat16)


def test_quantize_round_trip():
    W = _weight()
    wq, scale = ref.quantize_weight_fp8(W)
    assert wq.dtype == torch.float8_e4m3fn and tuple(wq.shape) == (OUT, IN)
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (OUT,)
    assert float(scale[5]) == 1.0 and not wq[5].float().any()
    assert torch.equal(scale[6], W[:, 6].float().abs().max() / 448)
    q = wq.float()
    # e4m3's half ulp: 2^-4 relative, 2^-10 absolute below the normals
    bound = scale[:, None] * torch.maximum(q.abs() * 2.0 ** -4,
                                           torch.tensor(2.0 ** -10))
    assert bool(((W.float().t() - q * scale[:, None]).abs() <= bound).all())
    deq = ref.dequant_fp8_weight(wq, scale)
    assert deq.dtype == torch.bfloat16 and tuple(deq.shape) == (IN, OUT)
    assert torch.equal(deq, (q * scale[:, None]).to(torch.bfloat16).t())


def test_ref_linear_against_float64():
    wq, scale = ref.quantize_weight_fp8(_weight())
    x = torch.randn(17, IN, generator=torch.Generator().manual_seed(1)) \
        .to(torch.bfloat16)
    y = ops.linear_fp8(x, wq, scale)
    assert y.dtype == torch.bfloat16
    w64 = wq.double() * scale.double()[:, None]
    y64 = x.double() @ w64.t()
    bound = 2.0 ** -8 * y64.abs() + IN * 2.0 ** -23 * (x.double().abs()
                                                       @ w64.abs().t())
    assert bool(((y.double() - y64).abs() <= bound).all())


def test_cpu_worker_with_fp8_weights():
    bf16 = EngineWorker(ec.CONFIG, "cpu", kv_blocks=16)
    fp8 = EngineWorker(ec.CONFIG, "cpu", kv_blocks=16, weight_dtype="fp8")
    assert fp8.model.weight_bytes() < bf16.model.weight_bytes()
    for layer in fp8.model.layers:
        for name in ("wqkv", "wo", "wgate_up", "wdown"):
            wq, scale = layer[name]
            assert wq.dtype == torch.float8_e4m3fn
            assert scale.dtype == torch.float32
    dense = fp8.model.dense_layers()[0]["wqkv"]
    assert dense.dtype == torch.float32 and \
        dense.shape == bf16.model.layers[0]["wqkv"].shape
    logits, forward = [], fp8.model.forward
    fp8.model.forward = lambda *a, **kw: logits.append(forward(*a, **kw)) \
        or logits[-1]
    fp8.add_request(EngineRequest("r", prompt_tokens=list(range(3, 23)),
                                  max_tokens=3))
    outs = []
    for _ in range(16):
        outs.extend(fp8.step())
        if not fp8.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert fin and fin[0].completion_tokens == 3 and not fin[0].error
    assert logits and all(
        row.shape[-1] == ec.CONFIG.vocab_size and bool(row.isfinite().all())
        for row in logits)
