"""Time the fused sampler (csrc/hip/sampler.hip) against two torch
formulations, on one GPU.

  python tools/sampler_bench.py            # markdown table on stdout

Shapes: B in {1, 32, 256} x V in {128256, 151936}, bf16 logits, T=0.8,
top_k=50, top_p=0.9.
  * fused        ops.sample with the filters on
  * sort         torch sort + cumsum + mask + Gumbel over [B, V], the same
                 contract (torch.rand noise instead of Philox)
  * fused k0p1   ops.sample with top_k=0, top_p=1 (temperature only)
  * eager        EngineWorker._sample_device's five-op Gumbel path, which
                 the temperature-only fused call would replace

Each figure is the median over 7 repeats of the mean of 20 launches timed
with torch.cuda.Event after 5 warm-up launches, in microseconds.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from llm_d_inference_scheduler_amd import ops


def time_us(run, iters=20, repeats=7, warmup=5):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(iters):
            run()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / iters * 1e3)
    samples.sort()
    return samples[len(samples) // 2]


def sort_sample(logits, temps, top_k, top_p):
    """Sort formulation of the contract: top-k ties kept, top-p over the
    top-k survivors against p * W, Gumbel-max draw."""
    z = logits.float() / temps.unsqueeze(1)
    zs, idx = z.sort(dim=-1, descending=True)
    kth = zs.gather(1, (top_k.long() - 1).clamp(min=0).unsqueeze(1))
    keep = zs >= kth
    w = torch.exp(zs - zs[:, :1]) * keep
    cum = w.cumsum(dim=-1)
    target = top_p.unsqueeze(1) * cum[:, -1:]
    keep &= (cum - w) < target
    u = torch.rand_like(zs).clamp_min(1e-20)
    score = torch.where(keep, zs - torch.log(-torch.log(u)),
                        torch.full_like(zs, float("-inf")))
    return idx.gather(1, score.argmax(dim=-1, keepdim=True)).squeeze(1)


def eager_gumbel(logits, temps):
    hot = temps > 0
    inv = torch.where(hot, 1.0 / temps.clamp(min=1e-6),
                      torch.ones_like(temps))
    y = logits.float() * inv.unsqueeze(1)
    u = torch.rand_like(y).clamp_min(1e-20)
    gumbel = -torch.log(-torch.log(u).clamp_min(1e-20))
    y = y + gumbel * hot.unsqueeze(1)
    return y.argmax(dim=-1)


def main():
    dev = "cuda"
    print("| B | V | fused us | sort us | sort/fused | fused k0p1 us | "
          "eager us | eager/fused k0p1 |")
    print("|---|---|---|---|---|---|---|---|")
    for V in (128256, 151936):
        for B in (1, 32, 256):
            g = torch.Generator(device=dev).manual_seed(B + V)
            logits = (torch.randn(B, V, generator=g, device=dev) * 4
                      ).bfloat16()
            T = torch.full((B,), 0.8, device=dev)
            k = torch.full((B,), 50, dtype=torch.int32, device=dev)
            p = torch.full((B,), 0.9, device=dev)
            k0 = torch.zeros_like(k)
            p1 = torch.ones_like(p)
            seed = torch.arange(B, dtype=torch.int64, device=dev)
            pos = torch.zeros(B, dtype=torch.int32, device=dev)
            fused = time_us(lambda: ops.sample(logits, T, k, p, seed, pos))
            srt = time_us(lambda: sort_sample(logits, T, k, p))
            plain = time_us(lambda: ops.sample(logits, T, k0, p1, seed, pos))
            eager = time_us(lambda: eager_gumbel(logits, T))
            print(f"| {B} | {V} | {fused:.1f} | {srt:.1f} | "
                  f"{srt / fused:.1f}x | {plain:.1f} | {eager:.1f} | "
                  f"{eager / plain:.2f}x |", flush=True)


if __name__ == "__main__":
    sys.exit(main())
