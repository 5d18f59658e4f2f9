"""Block-scaled fp8 linears against the per-channel fp8 path and bf16
(results: profiles/linear_fp8_block.md).

    python tools/linear_fp8_block_bench.py [--rounds 7] [--warm]

Per projection of Llama-3-8B and Qwen3-32B and T in {1, 16, 32, 64, 128,
256, 1024, 4096}, one JSON line of median microseconds per call (and the spread
max - min over the rounds as <arm>_spread):
  block    ops.linear_fp8_block as the runner calls it: the group quantiser,
           the kernel linear_fp8_block_kernel_for picks, the split reduce
  skinny, t64, t128   the same with the kernel forced through the raw
           binding (skinny up to 256 rows only: beyond, it re-reads the
           weights once per 64 rows and is not a candidate)
  quant    ops.quantize_groups_fp8 alone; it also transposes the scales to
           the documented [T, G], which the linear op does not do
  fp8      the per-channel fp8 path at that T: ops.linear_fp8 up to 128 rows,
           ops.linear_fp8_a8 above
  bf16     x @ W with the tuned GEMMs the runner runs
Timing is that of tools/linear_fp8_bench.py: device events around windows of
about 10 ms, arms alternated over the rounds, and (without --warm) weights
rotated through 512 MiB of copies so that every call reads them from HBM.
`floor` is the weight and scale bytes over 8 TB/s. `skinny_bytes` is what the
skinny kernel moves at that T by its own work split, from shapes: the weights
once per 64-row tile, the codes and row scales once per column block (from
L2), the split partials written and read, y written.
Before timing, the served output's first 8 rows are judged against float64
under the bound of tests/test_gpu_linear_fp8_block.py, and every forced
variant's against the same."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from linear_fp8_bench import (  # noqa: E402
    A8_MFMA_COEFF, COLD_BYTES, DEV, HBM_BYTES_PER_US, bench, projections,
    rotating)
from llm_d_inference_scheduler_amd import ops  # noqa: E402
from llm_d_inference_scheduler_amd.models.configs import (  # noqa: E402
    LLAMA_3_8B, QWEN3_32B)
from llm_d_inference_scheduler_amd.models.llama import (  # noqa: E402
    _load_tuned_gemms)

TS = (1, 16, 32, 64, 128, 256, 1024, 4096)
SKINNY_MAX_T = 256       # rows up to which the forced skinny arm is timed
FP8_KERNEL_MAX_T = 128   # LlamaRunner._fp8_kernel_max_t


def check_block(y, x, w64, what):
    """y's first 8 rows against float64 on the dequantised codes; w64 [out,
    in] is the dequantised weight."""
    n, n_in = min(8, x.shape[0]), x.shape[1]
    xq, sx = ops.quantize_groups_fp8(x[:n].contiguous())
    x64 = xq.double() * sx.double().repeat_interleave(128, 1)[:, :n_in]
    y64 = x64 @ w64.t()
    coeff = max(n_in, A8_MFMA_COEFF) * 2.0 ** -23
    bad = (y[:n].double() - y64).abs() > \
        2.0 ** -8 * y64.abs() + coeff * (x64.abs() @ w64.abs().t())
    if bool(bad.any()):
        raise SystemExit(f"{what}: {int(bad.sum())} elements out of bound")


def skinny_bytes(T, n_in, n_out, n_split):
    G, bn = -(-n_in // 128), 32 if T <= 16 else 64
    col_blocks, row_tiles = -(-n_out // bn), -(-T // 64)
    return (row_tiles * (n_out * n_in + 4 * G * -(-n_out // 128))
            + col_blocks * T * (n_in + 4 * G)
            + (2 * 4 * n_split * T * n_out if n_split > 1 else 0)
            + 2 * T * n_out)


def k_splits(n_in, n_out):
    """linear_fp8_block_k_splits of csrc/hip/launchers.h."""
    wgs, s = -(-n_out // 32), 1
    while s < 8 and wgs * s < 512 and n_in // (2 * s) >= 1024:
        s *= 2
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", action="store_true")
    args = ap.parse_args()
    ext = ops.hip_ops()
    _load_tuned_gemms()
    gen = torch.Generator().manual_seed(0)
    for c in (LLAMA_3_8B, QWEN3_32B):
        for proj, (n_in, n_out) in projections(c).items():
            W = (torch.randn(n_in, n_out, generator=gen) * 0.02) \
                .to(torch.bfloat16).to(DEV)
            wq, scale = ops.ref.quantize_weight_fp8_block(W)
            wq8, scale8 = ops.ref.quantize_weight_fp8(W)
            w64 = wq.double() * ops.ref.expand_fp8_block_scale(
                scale.double(), n_out, n_in)
            n8 = 1 if args.warm else -(-COLD_BYTES // wq.numel())
            n16 = 1 if args.warm else -(-COLD_BYTES // (2 * W.numel()))
            wqs = [wq] + [wq.clone() for _ in range(n8 - 1)]
            wq8s = [wq8] + [wq8.clone() for _ in range(n8 - 1)]
            Ws = [W] + [W.clone() for _ in range(n16 - 1)]
            for T in TS:
                x = torch.randn(T, n_in, generator=gen).to(torch.bfloat16) \
                    .to(DEV)
                forced = {"t64": 64, "t128": 128}
                if T <= SKINNY_MAX_T:
                    forced["skinny"] = 1
                check_block(ops.linear_fp8_block(x, wq, scale), x, w64,
                            "block")
                for name, k in forced.items():
                    check_block(ext.linear_fp8_block(x, wq, scale, k), x,
                                w64, name)
                fp8 = ops.linear_fp8 if T <= FP8_KERNEL_MAX_T else \
                    ops.linear_fp8_a8
                fns = {
                    "block": rotating(lambda i: ops.linear_fp8_block(
                        x, wqs[i], scale), n8),
                    **{name: rotating(lambda i, k=k: ext.linear_fp8_block(
                        x, wqs[i], scale, k), n8)
                       for name, k in forced.items()},
                    "quant": lambda: ops.quantize_groups_fp8(x),
                    "fp8": rotating(lambda i: fp8(x, wq8s[i], scale8), n8),
                    "bf16": rotating(lambda i: x @ Ws[i], n16)}
                print(json.dumps(dict(
                    model=c.name, proj=proj, n_in=n_in, n_out=n_out, T=T,
                    copies=n8, floor=round(
                        (wq.numel() + 4 * scale.numel()) / HBM_BYTES_PER_US,
                        2),
                    skinny_bytes=skinny_bytes(T, n_in, n_out,
                                              k_splits(n_in, n_out)),
                    **bench(fns, args.rounds, spread=True))), flush=True)
            del W, wq, scale, wq8, scale8, w64, wqs, wq8s, Ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
