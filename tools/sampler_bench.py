"""Time the fused sampler (csrc/hip/sampler.hip) against two torch
formulations, on one GPU.

  python tools/sampler_bench.py            # markdown table on stdout
  python tools/sampler_bench.py --ext      # sample_ext / token_state_fill
  python tools/sampler_bench.py --sample-only   # the `fused` column alone

Shapes: B in {1, 32, 256} x V in {128256, 151936}, bf16 logits, T=0.8,
top_k=50, top_p=0.9.
  * fused        ops.sample with the filters on
  * sort         torch sort + cumsum + mask + Gumbel over [B, V], the same
                 contract (torch.rand noise instead of Philox)
  * fused k0p1   ops.sample with top_k=0, top_p=1 (temperature only)
  * eager        EngineWorker._sample_device's five-op Gumbel path, which
                 the temperature-only fused call would replace

--ext times, at the same shapes and filters:
  * sample       ops.sample (the `fused` column above)
  * ext off      ops.sample_ext, every new input off, no token state: what
                 fp32 keys (4 digit passes per select instead of 2) cost
  * ext off+st   the same with a state row per request (all zero), rep = 1,
                 freq = pres = 0: adds the state reads
  * ext pen      rep 1.3, freq 0.7, pres 1.1 over state rows built from a
                 4096-token history (1024 prompt, 3072 output ids)
  * ext top20    every penalty off, no state, top_n = 20
  * fill         ops.token_state_fill of B rows from 4096-token histories
                 (the state is rebuilt before every timed ext pen launch
                 group, outside the timed region)

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


def ext_table():
    dev = "cuda"
    print("| B | V | sample us | ext off us | ext off+st us | ext pen us | "
          "ext top20 us | fill us |")
    print("|---|---|---|---|---|---|---|---|")
    f32, i32 = torch.float32, torch.int32
    for V in (128256, 151936):
        for B in (1, 32, 256):
            g = torch.Generator(device=dev).manual_seed(B + V)
            logits = (torch.randn(B, V, generator=g, device=dev) * 4
                      ).bfloat16()
            T = torch.full((B,), 0.8, device=dev)
            k = torch.full((B,), 50, dtype=i32, device=dev)
            p = torch.full((B,), 0.9, device=dev)
            seed = torch.arange(B, dtype=torch.int64, device=dev)
            pos = torch.zeros(B, dtype=i32, device=dev)
            base = (logits, T, k, p, seed, pos)
            one = torch.ones(B, dtype=f32, device=dev)
            zero = torch.zeros(B, dtype=f32, device=dev)
            n0 = torch.zeros(B, dtype=i32, device=dev)
            n20 = torch.full((B,), 20, dtype=i32, device=dev)
            none = torch.full((B,), -1, dtype=i32, device=dev)
            rows = torch.arange(B, dtype=i32, device=dev)
            state = ops.token_state_alloc(B, V, dev)
            hist = torch.randint(0, V, (B * 4096,), generator=g, device=dev,
                                 dtype=torch.int64).to(i32)
            offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * 4096
            n_p = torch.full((B,), 1024, dtype=i32, device=dev)
            fill = lambda: ops.token_state_fill(state, rows, hist, offs,
                                                n_p, V)
            t_sample = time_us(lambda: ops.sample(*base))
            t_off = time_us(lambda: ops.sample_ext(
                *base, one, zero, zero, zero, n0, none, None, 0))
            t_off_st = time_us(lambda: ops.sample_ext(
                *base, one, zero, zero, zero, n0, rows, state, 0))
            t_fill = time_us(fill)
            t_pen = time_us(lambda: ops.sample_ext(
                *base, one * 1.3, one * 1.1, one * 0.7, zero, n0, rows,
                state, 0))
            t_top = time_us(lambda: ops.sample_ext(
                *base, one, zero, zero, zero, n20, none, None, 20))
            print(f"| {B} | {V} | {t_sample:.1f} | {t_off:.1f} | "
                  f"{t_off_st:.1f} | {t_pen:.1f} | {t_top:.1f} | "
                  f"{t_fill:.1f} |", flush=True)


def sample_only():
    dev = "cuda"
    print("| B | V | fused us |")
    print("|---|---|---|")
    for V in (128256, 151936):
        for B in (1, 32, 256):
            g = torch.Generator(device=dev).manual_seed(B + V)
            logits = (torch.randn(B, V, generator=g, device=dev) * 4
                      ).bfloat16()
            T = torch.full((B,), 0.8, device=dev)
            k = torch.full((B,), 50, dtype=torch.int32, device=dev)
            p = torch.full((B,), 0.9, device=dev)
            seed = torch.arange(B, dtype=torch.int64, device=dev)
            pos = torch.zeros(B, dtype=torch.int32, device=dev)
            fused = time_us(lambda: ops.sample(logits, T, k, p, seed, pos))
            print(f"| {B} | {V} | {fused:.1f} |", flush=True)


def main():
    if "--ext" in sys.argv[1:]:
        return ext_table()
    if "--sample-only" in sys.argv[1:]:
        return sample_only()
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
