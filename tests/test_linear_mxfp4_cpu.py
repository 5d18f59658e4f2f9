"""MXFP4 weights on the CPU path (DEVELOPMENT.md "MXFP4 weights"): the
quantiser, ops.ref.linear_mxfp4 and an mxfp4-weights EngineWorker."""
import pytest
import torch

import engine_cases as ec
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.ops import ref

IN, OUT = 384, 48


def mx_weight(n_in, n_out, seed=0):
    """[n_in, n_out] bf16 whose 32-wide groups along k have magnitudes from
    2^-12 to 2^6, a function of (5 * group + n) % 16: the full range along n
    within 16 columns and along k within four groups. Shared with
    test_gpu_linear_mxfp4.py."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.arange(n_in)[:, None] // 32
    e = -12 + 18 * ((5 * g + torch.arange(n_out)[None, :]) % 16) / 15
    return (torch.randn(n_in, n_out, generator=gen) * torch.exp2(e)) \
        .to(torch.bfloat16)


def test_quantize_round_trip():
    W = mx_weight(IN, OUT)
    W[32:64, 5] = 0
    wq, scale = ref.quantize_weight_mxfp4(W)
    assert wq.dtype == torch.uint8 and tuple(wq.shape) == (OUT, IN // 2)
    assert scale.dtype == torch.uint8 and tuple(scale.shape) == (OUT, IN // 32)
    assert int(scale[5, 1]) == 127 and not wq[5, 16:32].any()
    grp = W.float().t().reshape(OUT, IN // 32, 32)
    amax = grp.abs().amax(dim=2).double()
    rule = torch.floor(torch.log2(amax)) - 2 + 127
    rule[5, 1] = 127
    assert int(scale.min()) <= 117 and int(scale.max()) >= 131
    assert torch.equal(scale.double(), rule)
    # dequantised by hand: code -> e2m1 value, times 2^(scale - 127)
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6,
                        -0., -.5, -1, -1.5, -2, -3, -4, -6])
    codes = torch.stack((wq & 15, wq >> 4), dim=2).reshape(OUT, IN).long()
    assert len(codes.unique()) == 16
    sc = torch.ldexp(torch.ones(OUT, IN // 32), scale.int() - 127) \
        .repeat_interleave(32, dim=1)
    q = lut[codes] * sc
    # half the e2m1 spacing at the value, or the gap to 6 beyond it
    v, a = W.float().t() / sc, (q / sc).abs()
    half = torch.where(a >= 4, 1.0, torch.where(a >= 2, 0.5, 0.25))
    bound = torch.where(v.abs() > 6, v.abs() - 6, half) * sc
    assert bool(((W.float().t() - q).abs() <= bound).all())
    deq = ref.dequant_mxfp4_weight(wq, scale)
    assert deq.dtype == torch.bfloat16 and tuple(deq.shape) == (IN, OUT)
    assert torch.equal(deq.float(), q.t())
    assert torch.equal(ref.dequant_mxfp4_weight(wq, scale,
                                                dtype=torch.float32), q.t())


def test_ref_linear_against_float64():
    wq, scale = ref.quantize_weight_mxfp4(mx_weight(IN, OUT))
    x = torch.randn(17, IN, generator=torch.Generator().manual_seed(1)) \
        .to(torch.bfloat16)
    y = ops.linear_mxfp4(x, wq, scale)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (17, OUT)
    w64 = ref.dequant_mxfp4_weight(wq, scale, dtype=torch.float64)
    y64 = x.double() @ w64
    bound = 2.0 ** -8 * y64.abs() + IN * 2.0 ** -23 * (x.double().abs()
                                                       @ w64.abs())
    assert bool(((y.double() - y64).abs() <= bound).all())


def test_cpu_worker_with_mxfp4_weights():
    fp8 = EngineWorker(ec.CONFIG, "cpu", kv_blocks=16, weight_dtype="fp8")
    mx = EngineWorker(ec.CONFIG, "cpu", kv_blocks=16, weight_dtype="mxfp4")
    assert mx.model.weight_dtype == "mxfp4"
    assert mx.model.weight_bytes() < fp8.model.weight_bytes()
    with pytest.raises(ValueError):
        mx.model.quantize_weights("fp8")
    for layer, dense in zip(mx.model.layers, mx.model.dense_layers()):
        for name in ("wqkv", "wo", "wgate_up", "wdown"):
            wq, scale = layer[name]
            assert wq.dtype == torch.uint8 and scale.dtype == torch.uint8
            assert dense[name].dtype == torch.float32 and \
                tuple(dense[name].shape) == (2 * wq.shape[1], wq.shape[0])
    logits, forward = [], mx.model.forward
    mx.model.forward = lambda *a, **kw: logits.append(forward(*a, **kw)) \
        or logits[-1]
    mx.add_request(EngineRequest("r", prompt_tokens=list(range(3, 23)),
                                 max_tokens=3))
    outs = []
    for _ in range(16):
        outs.extend(mx.step())
        if not mx.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert fin and fin[0].completion_tokens == 3 and not fin[0].error
    assert logits and all(
        row.shape[-1] == ec.CONFIG.vocab_size and bool(row.isfinite().all())
        for row in logits)
