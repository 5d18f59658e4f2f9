"""Decode attention alone, at the flagship's geometry (run on a GPU box).

ops.paged_attention as LlamaRunner calls it for Llama-3-8B at 256 sequences:
B=256, QH=32, KVH=8, D=128, block size 16; contexts all 1152, or a seeded mix
of 1024..2048; bf16 and fp8 KV. Each call sits between two HIP events; 10
warm-up calls, then the median [min, max] of 40 timed calls, in microseconds.

To compare two builds, run this once per process, several processes per build,
alternating the builds (profiles/decode_glue.md).
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(
    os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from llm_d_inference_scheduler_amd import ops  # noqa: E402

B, QH, KVH, D, BS = 256, 32, 8, 128, 16
WARMUP, TIMED = 10, 40


def make(seq_lens, fp8, seed=0):
    g = torch.Generator().manual_seed(seed)
    max_blocks = (max(seq_lens) + BS - 1) // BS
    need = sum((s + BS - 1) // BS for s in seq_lens)
    NB = need + 1
    dev = "cuda"
    q = torch.randn(B, QH, D, device=dev).bfloat16()
    kc = torch.randn(NB, KVH, BS, D, device=dev).bfloat16()
    vc = torch.randn(NB, KVH, BS, D, device=dev).bfloat16()
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    # blocks handed out from a shuffled free list, as a pool in use does
    perm = torch.randperm(NB - 1, generator=g) + 1
    bt = torch.zeros(B, max_blocks, dtype=torch.int32)
    k = 0
    for b, s in enumerate(seq_lens):
        nb = (s + BS - 1) // BS
        bt[b, :nb] = perm[k:k + nb]
        k += nb
    sl = torch.tensor(seq_lens, dtype=torch.int32)
    return q, kc, vc, bt.to(dev), sl.to(dev)


def time_us(run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    samples = []
    for _ in range(TIMED):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        run()
        t1.record()
        t1.synchronize()
        samples.append(t0.elapsed_time(t1) * 1e3)
    samples.sort()
    return samples[len(samples) // 2], samples[0], samples[-1]


def main():
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    mixed = torch.randint(1024, 2049, (B,), generator=g).tolist()
    cases = (("ctx=1152", [1152] * B), ("ctx=1024..2048", mixed))
    for fp8 in (False, True):
        for name, lens in cases:
            q, kc, vc, bt, sl = make(lens, fp8)
            med, lo, hi = time_us(lambda: ops.paged_attention(
                q, kc, vc, bt, sl, D ** -0.5, max_seq_len=max(lens)))
            kv_bytes = sum(lens) * KVH * D * 2 * kc.element_size()
            print(f"{'fp8 ' if fp8 else 'bf16'} {name:15s} median {med:8.1f} "
                  f"us [{lo:.1f}, {hi:.1f}]  "
                  f"{kv_bytes / med / 1e6:5.2f} TB/s of KV", flush=True)


if __name__ == "__main__":
    main()
