"""Block-scaled fp8 experts without a GPU (DEVELOPMENT.md "Mixture of
experts"): ops.ref.moe_ffn_fp8_block under the two-stage float64 bound the
device op is asked to meet, the format, and the runner and engine rules."""
import dataclasses

import pytest
import torch

import moe_fp8_block_cases as bc
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.ops import ref

MOE = dataclasses.replace(TINY_LLAMA, num_experts=4, experts_per_token=2,
                          moe_intermediate_size=64)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_ref_inside_bound(name):
    args, dense = bc.build(name, "cpu")
    T, k, I = args[0].shape[0], args[5].shape[1], args[1].shape[1] // 2
    if name == "scales":
        # neighbouring scales span 2^10 along expert, half, block row, group
        E = args[2].shape[0]
        for s in (args[2].view(E, 2, -1, args[2].shape[2]), args[4]):
            for dim in range(s.dim()):
                assert float((s.amax(dim) / s.amin(dim)).max()) >= 2.0 ** 10
    act_out = torch.full((T * k, I), float("nan"), dtype=torch.bfloat16)
    y = ops.moe_ffn_fp8_block(*args, act_out=act_out)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    assert torch.equal(y, ops.moe_ffn_fp8_block(*args))
    e1, e2 = bc.excess(y, act_out, args, dense)
    print(f"MOE_FFN_FP8_BLOCK|{name}|ref|act={e1:.3e}|y={e2:.3e}")
    assert e1 <= 0 and e2 <= 0


def test_halves_are_blocked_apart():
    I, H = 320, 192
    w13 = torch.randn(2, 2 * I, H, generator=torch.Generator().manual_seed(0))
    w13[:, I:] *= 64         # the up half: another scale from row 320 on
    wq, scale = ref.quantize_experts_fp8_block(w13, halves=2)
    assert tuple(scale.shape) == (2, 6, 2)
    for e in range(2):
        for h in range(2):
            q, s = ref.quantize_weight_fp8_block(w13[e, h * I:(h + 1) * I].t())
            assert torch.equal(wq[e, h * I:(h + 1) * I].view(torch.uint8),
                               q.view(torch.uint8))
            assert torch.equal(scale[e, 3 * h:3 * h + 3], s)
    # the merged [2 I, H] matrix has five block rows, and other bytes
    merged = ref.quantize_weight_fp8_block(w13[0].t())
    assert tuple(merged[1].shape) == (5, 2)
    assert not torch.equal(merged[0].view(torch.uint8), wq[0].view(torch.uint8))
    back = ref.dequant_experts_fp8_block(wq, scale, halves=2)
    assert float((back - w13).abs().max() / w13.abs().max()) < 2.0 ** -4


@pytest.mark.parametrize("rule", ["scale", "mod64", "bf16 activations",
                                  "dense_layers"])
def test_runner_rules(rule):
    cfg = dataclasses.replace(MOE, moe_intermediate_size=96) \
        if rule == "mod64" else MOE
    worker = EngineWorker(cfg, "cpu", kv_blocks=16)
    m = worker.model
    if rule == "mod64":
        with pytest.raises(ValueError, match="multiples of 64"):
            m.quantize_experts("fp8_block128")
        return
    w13 = m.layers[0]["w13"]
    m.quantize_experts("fp8_block128")
    q13, q2 = m.layers[0]["w13"], m.layers[0]["w2"]
    assert m.expert_dtype == "fp8_block128"
    if rule == "scale":
        H = cfg.hidden_size
        assert tuple(q13[1].shape) == (4, 2, -(-H // 128))
        assert tuple(q2[1].shape) == (4, -(-H // 128), 1)
        assert q13[0].dtype == torch.float8_e4m3fn
    elif rule == "bf16 activations":
        m.set_expert_activation_dtype("auto")
        m.set_expert_activation_dtype("fp8")
        with pytest.raises(ValueError, match="fp8_block128"):
            m.set_expert_activation_dtype("bf16")
    else:
        dense = m.dense_layers()[0]["w13"]
        assert torch.equal(
            dense, ref.dequant_experts_fp8_block(*q13, halves=2))
        assert float((dense - w13.float()).abs().max() /
                     w13.float().abs().max()) < 2.0 ** -4


def test_cpu_worker_whole_checkpoint_recipe(monkeypatch):
    worker = EngineWorker(MOE, "cpu", kv_blocks=16, weight_dtype="fp8_block",
                          expert_dtype="fp8_block128",
                          expert_activation_dtype="fp8")
    layer = worker.model.layers[0]
    assert layer["wqkv"][1].dim() == 2 and layer["w13"][1].dim() == 3
    seen, block = [], ops.moe_ffn_fp8_block
    monkeypatch.setattr(ops, "moe_ffn_fp8_block", lambda x, *a:
                        seen.append(x.shape[0]) or block(x, *a))
    worker.add_request(EngineRequest("r", prompt_tokens=list(range(3, 23)),
                                     max_tokens=3))
    outs = []
    for _ in range(16):
        outs.extend(worker.step())
        if not worker.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert fin and fin[0].completion_tokens == 3 and not fin[0].error
    n = MOE.num_layers
    assert seen[:n] == [20] * n and set(seen[n:]) == {1}
