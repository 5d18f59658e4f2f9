"""Microbench of the fp8-weights linear against the bf16 GEMM it replaces
(results: profiles/linear_fp8.md).

    python tools/linear_fp8_bench.py [--format fp8|mxfp4|fp8a8] [--rounds 9]
                                     [--geometry]

Shapes: the four projections of Llama-3-8B and of Qwen3-32B, for T in
{1, 8, 16, 32, 64, 128, 256}. Arms, timed in one process in interleaved
rounds (arm order rotates each round) with device events around a window of
back-to-back calls (enough for 10 ms of device time), on random data:
  kernel   ops.linear_fp8 as the runner calls it (scratch allocation and,
           where K is split across workgroups, the reduce launch inside)
  dequant  ops.dequant_fp8_weight into a resident scratch, then torch.matmul
  bf16     x @ W in bf16 with the runner's tuned hipBLASLt solutions: what
           the runner does without fp8 weights
A decode step streams every layer's weights, so a projection's weight is cold
when its GEMM starts. Each arm therefore walks round-robin over enough copies
of its weight to hold COLD_BYTES (twice the 256 MB Infinity Cache): a call
never finds its weight where the call before left it. --warm times one copy
instead.
--geometry times the kernel alone under other launch geometries instead
(column block BN x K splits) at T in {1, 16, 32, 64}.
Before a shape is timed, the kernel and the dequant arm are compared with
the float64 product under the bound of tests/test_gpu_linear_fp8.py, at
every geometry that is timed.
Reported per arm: the median per-call time over the rounds, in us; `floor` is
the weight bytes (fp8) over 8 TB/s.
--format mxfp4 (results: profiles/linear_mxfp4.md) times ops.linear_mxfp4 and
ops.dequant_mxfp4_weight + matmul as `kernel` and `dequant` instead, for T in
{1, 4, 16, 32, 64, 128, 256}, keeps the fp8 kernel as the arm `fp8` in the
same rounds, and adds `<arm>_spread`, the largest minus the smallest round of
an arm; `floor` then counts the codes and the scale bytes.
--format fp8a8 (results: profiles/linear_fp8_a8.md) is the prefill side, T in
{128, 256, 512, 1024, 2048, 4096}: `a8` is ops.linear_fp8_a8 as the runner
calls it (per-row quantiser + fp8 MFMA GEMM), `quant` the quantiser alone
(its share of `a8`), `dequant` and `bf16` as above, with `<arm>_spread`. `a8`
is first compared with the float64 product of the dequantised codes under
the bound of tests/test_gpu_linear_fp8_a8.py.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_d_inference_scheduler_amd import ops  # noqa: E402
from llm_d_inference_scheduler_amd.models.configs import (  # noqa: E402
    LLAMA_3_8B, QWEN3_32B)
from llm_d_inference_scheduler_amd.models.llama import (  # noqa: E402
    _load_tuned_gemms)

DEV = "cuda"
TS = (1, 8, 16, 32, 64, 128, 256)
TS_MXFP4 = (1, 4, 16, 32, 64, 128, 256)
TS_A8 = (128, 256, 512, 1024, 2048, 4096)
A8_MFMA_COEFF = 2 * 1718    # tests/test_gpu_linear_fp8_a8.py MFMA_COEFF
WINDOW_US = 10000.0
COLD_BYTES = 512 << 20
HBM_BYTES_PER_US = 8e6


def projections(c):
    return {"wqkv": (c.hidden_size, c.q_size + 2 * c.kv_size),
            "wo": (c.q_size, c.hidden_size),
            "wgate_up": (c.hidden_size, 2 * c.intermediate_size),
            "wdown": (c.intermediate_size, c.hidden_size)}


def time_arm(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # us per call


def bench(fns, rounds, spread=False):
    names = list(fns)
    for fn in fns.values():                                # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = {n: max(5, int(WINDOW_US / time_arm(fns[n], 5)) + 1)
             for n in names}
    times = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(time_arm(fns[n], iters[n]))
    res = {n: round(statistics.median(ts), 2) for n, ts in times.items()}
    if spread:
        res.update({n + "_spread": round(max(ts) - min(ts), 2)
                    for n, ts in times.items()})
    return res


def rotating(fn, n):
    """fn(i) over i = 0 .. n - 1, round-robin, one step a call."""
    state = [0]

    def call():
        state[0] = (state[0] + 1) % n
        return fn(state[0])
    return call


def check(y, x, wq, scale, what, mx=False):
    """y against the float64 product, first 8 rows, under the tests' bound
    (bf16 rounding of y plus fp32 accumulation in any order, doubled; the
    dequant arm also rounds the weight and sums in bf16 GEMM order, which
    the 2^-7 |x||w| term covers)."""
    n = min(8, x.shape[0])
    w64 = ops.ref.dequant_mxfp4_weight(wq, scale, dtype=torch.float64) \
        if mx else (wq.double() * scale.double()[:, None]).t()
    x64 = x[:n].double()
    y64 = x64 @ w64
    mag = x64.abs() @ w64.abs()
    slack = 2.0 ** -7 if what == "dequant" else x.shape[1] * 2.0 ** -23
    bad = (y[:n].double() - y64).abs() > 2.0 ** -8 * y64.abs() + slack * mag
    if bool(bad.any()):
        raise SystemExit(f"{what}: {int(bad.sum())} elements out of bound")


def check_a8(y, x, wq, scale):
    """ops.linear_fp8_a8's y against float64 on the dequantised codes, first
    8 rows, under the bound of tests/test_gpu_linear_fp8_a8.py."""
    n = min(8, x.shape[0])
    xq, sx = ops.quantize_rows_fp8(x[:n].contiguous())
    x64 = xq.double() * sx.double()[:, None]
    w64 = (wq.double() * scale.double()[:, None]).t()
    y64 = x64 @ w64
    coeff = max(x.shape[1], A8_MFMA_COEFF) * 2.0 ** -23
    bad = (y[:n].double() - y64).abs() > \
        2.0 ** -8 * y64.abs() + coeff * (x64.abs() @ w64.abs())
    if bool(bad.any()):
        raise SystemExit(f"a8: {int(bad.sum())} elements out of bound")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["fp8", "mxfp4", "fp8a8"],
                    default="fp8")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--geometry", action="store_true")
    ap.add_argument("--warm", action="store_true")
    args = ap.parse_args()
    ext = ops.hip_ops()
    mx = args.format == "mxfp4"
    a8 = args.format == "fp8a8"
    if a8 and args.geometry:
        raise SystemExit("--geometry is not defined for --format fp8a8")
    linear, dequant = (ops.linear_mxfp4, ops.dequant_mxfp4_weight) if mx \
        else (ops.linear_fp8, ops.dequant_fp8_weight)
    ext_linear = ext.linear_mxfp4 if mx else ext.linear_fp8
    _load_tuned_gemms()     # the bf16 arm runs the GEMMs the runner runs
    gen = torch.Generator().manual_seed(0)
    geometries = [(bn, s) for bn in (16, 32, 64) for s in (1, 2, 4, 8)]
    for c in (LLAMA_3_8B, QWEN3_32B):
        for proj, (n_in, n_out) in projections(c).items():
            W = (torch.randn(n_in, n_out, generator=gen) * 0.02) \
                .to(torch.bfloat16).to(DEV)
            wq, scale = ops.ref.quantize_weight_mxfp4(W) if mx else \
                ops.ref.quantize_weight_fp8(W)
            dense = torch.empty_like(W)
            n8 = 1 if args.warm else -(-COLD_BYTES // wq.numel())
            if mx and not args.geometry:       # the fp8 arm of the same run
                wq8, scale8 = ops.ref.quantize_weight_fp8(W)
                m8 = 1 if args.warm else -(-COLD_BYTES // wq8.numel())
                wq8s = [wq8] + [wq8.clone() for _ in range(m8 - 1)]
            n16 = 1 if args.warm or args.geometry else \
                -(-COLD_BYTES // (2 * W.numel()))
            wqs = [wq] + [wq.clone() for _ in range(n8 - 1)]
            Ws = [W] + [W.clone() for _ in range(n16 - 1)]
            for T in TS_A8 if a8 else TS_MXFP4 if mx else TS:
                if args.geometry and T not in (1, 16, 32, 64):
                    continue
                x = torch.randn(T, n_in, generator=gen).to(torch.bfloat16) \
                    .to(DEV)
                if args.geometry:
                    for bn, s in geometries:
                        check(ext_linear(x, wq, scale, bn, s), x, wq,
                              scale, f"bn{bn}_s{s}", mx)
                    fns = {f"bn{bn}_s{s}": rotating(
                        lambda i, bn=bn, s=s: ext_linear(
                            x, wqs[i], scale, bn, s), n8)
                        for bn, s in geometries}
                elif a8:
                    check_a8(ops.linear_fp8_a8(x, wq, scale), x, wq, scale)
                    check(x @ dequant(wq, scale, dense), x, wq, scale,
                          "dequant")
                    fns = {
                        "a8": rotating(lambda i: ops.linear_fp8_a8(
                            x, wqs[i], scale), n8),
                        "quant": lambda: ops.quantize_rows_fp8(x),
                        "dequant": rotating(
                            lambda i: x @ dequant(wqs[i], scale, dense), n8),
                        "bf16": rotating(lambda i: x @ Ws[i], n16)}
                else:
                    check(linear(x, wq, scale), x, wq, scale, "kernel", mx)
                    check(x @ dequant(wq, scale, dense), x, wq, scale,
                          "dequant", mx)
                    fns = {
                        "kernel": rotating(lambda i: linear(
                            x, wqs[i], scale), n8),
                        "dequant": rotating(
                            lambda i: x @ dequant(wqs[i], scale, dense), n8),
                        "bf16": rotating(lambda i: x @ Ws[i], n16)}
                    if mx:
                        fns["fp8"] = rotating(lambda i: ops.linear_fp8(
                            x, wq8s[i], scale8), m8)
                print(json.dumps(dict(
                    model=c.name, proj=proj, n_in=n_in, n_out=n_out, T=T,
                    copies=n8, floor=round(
                        (wq.numel() + (scale.numel() if mx else 0))
                        / HBM_BYTES_PER_US, 2),
                    **bench(fns, args.rounds, spread=mx or a8))), flush=True)
            del W, wq, scale, dense, wqs, Ws
            if mx and not args.geometry:
                del wq8, scale8, wq8s
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
