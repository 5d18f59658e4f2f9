"""ops.ref.moe_ffn_fp8_a8, the CPU path of ops.moe_ffn_fp8_a8, under the
two-stage float64 bound of moe_fp8_a8_cases: the reference alone stays inside
what the device op is asked to meet."""
import pytest
import torch

import moe_fp8_a8_cases as a8c
from llm_d_inference_scheduler_amd import ops


@pytest.mark.parametrize("name", list(a8c.CASES))
def test_ref_inside_bound(name):
    args, dense = a8c.build(name, "cpu")
    T, k, I = args[0].shape[0], args[5].shape[1], args[1].shape[1] // 2
    act_out = torch.full((T * k, I), float("nan"), dtype=torch.bfloat16)
    y = ops.moe_ffn_fp8_a8(*args, act_out=act_out)
    assert y.dtype == torch.bfloat16 and y.shape == args[0].shape
    assert torch.equal(y, ops.moe_ffn_fp8_a8(*args))
    e1, e2 = a8c.excess(y, act_out, args, dense)
    print(f"MOE_FFN_FP8_A8|{name}|ref|act={e1:.3e}|y={e2:.3e}")
    assert e1 <= 0 and e2 <= 0

