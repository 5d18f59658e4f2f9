"""Microbench of ops.lora_add against the composed torch path and the base
GEMM, at a decode and a prefill shape (results: profiles/lora.md).

    python tools/lora_bench.py [--rounds 15] [--iters 20]

Shapes: the four Llama-3-8B projections (wqkv 4096->6144, wo 4096->4096,
wgate_up 4096->28672, wdown 14336->4096), R = 16, 8 adapters.
  decode   T = 256 rows, adapters interleaved row by row
  prefill  T = 4096 rows in 4 segments of 1024, one adapter each

Three arms per shape, timed in one process in interleaved rounds (arm order
rotates each round) with device events around a window of back-to-back calls
(at least `iters`, and enough for 5 ms of device time per window), on random
data. A hip call is the binding as the engine calls it: its scratch
allocation and both launches are inside.
  hip       ops.lora_add (shrink + expand kernels)
  composed  index_select of A / B per row, two bmm, add (not the code under
            test: what one would write without the kernels)
  gemm      the base projection x @ W of the same shape, for scale
Reported per arm: median, min and the p10..p90 spread of the per-call time
over the rounds.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_d_inference_scheduler_amd import ops  # noqa: E402

PROJ = {"wqkv": (4096, 6144), "wo": (4096, 4096), "wgate_up": (4096, 28672),
        "wdown": (14336, 4096)}
S, R = 8, 16
DEV = "cuda"


def make(T, row_slot, n_in, n_out, gen):
    bf = torch.bfloat16
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale) \
        .to(bf).to(DEV)
    x, y = rnd(T, n_in), rnd(T, n_out)
    A = rnd(S, R, n_in, scale=n_in ** -0.5)
    B = rnd(S, n_out, R, scale=R ** -0.5)
    W = rnd(n_in, n_out, scale=0.02)
    perm, tiles = ops.lora_worklist(row_slot)
    slots = torch.tensor(row_slot, dtype=torch.int64, device=DEV)
    return dict(x=x, y=y, A=A, B=B, W=W, perm=perm.to(DEV),
                tiles=tiles.to(DEV), slots=slots)


def arms(d):
    def hip():
        ops.lora_add(d["y"], d["x"], d["A"], d["B"], d["perm"], d["tiles"])

    def composed():
        a = d["A"].index_select(0, d["slots"])            # [T, R, in]
        b = d["B"].index_select(0, d["slots"])            # [T, out, R]
        tmp = torch.bmm(a, d["x"].unsqueeze(2))           # [T, R, 1]
        d["y"].add_(torch.bmm(b, tmp).squeeze(2))

    def gemm():
        return d["x"] @ d["W"]

    return {"hip": hip, "composed": composed, "gemm": gemm}


def time_arm(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # us per call


WINDOW_US = 5000.0      # a timed window is at least this long


def bench(d, rounds, min_iters):
    fns = arms(d)
    names = list(fns)
    for fn in fns.values():                                # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # calls per window, per arm: enough for WINDOW_US of device time
    iters = {n: max(min_iters, int(WINDOW_US / time_arm(fns[n], 10)) + 1)
             for n in names}
    times = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            times[n].append(time_arm(fns[n], iters[n]))
    out = {}
    for n, ts in times.items():
        q = statistics.quantiles(ts, n=10)
        out[n] = dict(median_us=round(statistics.median(ts), 2),
                      min_us=round(min(ts), 2), p10_us=round(q[0], 2),
                      p90_us=round(q[-1], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    shapes = {"decode": (256, [i % S for i in range(256)]),
              "prefill": (4096, [i // 1024 for i in range(4096)])}
    for shape, (T, row_slot) in shapes.items():
        for proj, (n_in, n_out) in PROJ.items():
            d = make(T, row_slot, n_in, n_out, gen)
            res = bench(d, args.rounds, args.iters)
            print(json.dumps(dict(shape=shape, T=T, proj=proj, n_in=n_in,
                                  n_out=n_out, **{f"{a}_{k}": v
                                                  for a, r in res.items()
                                                  for k, v in r.items()})),
                  flush=True)
            del d
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
