"""Decode paged-attention kernel microbenchmark (run on a GPU box).
Times the production kernel at serving shapes with/without sequence split,
against the pipelined v4 (producer/consumer waves, double-buffered logits).
Also checks v4 numerics against v1 before timing.

    --chunks      online-softmax chunk 256 vs 512
    --kv-scales   fp8 KV with per-head scales: numerics against the torch
                  reference, then scaled vs unscaled fp8 in one process
    --medians     the standard shapes on bf16 and on unscaled fp8 KV, median
                  [min, max] of 7 repeats of 50 launches: the figures to
                  compare two builds by (run each build several times,
                  alternating)
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(
    os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from llm_d_inference_scheduler_amd.ops import hip_ops  # noqa: E402

ext = hip_ops()
KVH, D, BS = 8, 128, 16


def make(B, ctx, qpg, fp8=False, seed=0):
    torch.manual_seed(seed)
    max_blocks = (ctx + BS - 1) // BS
    NB = max_blocks * B + 1
    q = torch.randn(B, KVH * qpg, D, device="cuda").bfloat16()
    kc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
    vc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
    if fp8:
        kc = kc.to(torch.float8_e4m3fn)
        vc = vc.to(torch.float8_e4m3fn)
    bt = torch.arange(1, NB, dtype=torch.int32,
                      device="cuda").view(B, max_blocks)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    return q, kc, vc, bt, sl


def check(kernel, qpg=4, fp8=False):
    fn = getattr(ext, f"paged_attention_{kernel}")
    for B, ctx, np_, part in ((4, 300, 1, 0), (8, 1152, 1, 0),
                              (8, 1152, 4, 320), (3, 70, 1, 0)):
        q, kc, vc, bt, sl = make(B, ctx, qpg, fp8)
        scale = D ** -0.5
        ref = ext.paged_attention(q, kc, vc, bt, sl, scale)
        got = fn(q, kc, vc, bt, sl, np_,
                 part if np_ > 1 else ctx + 256, scale)
        diff = (ref.float() - got.float()).abs().max().item()
        status = "OK" if diff < 3e-2 else "FAIL"
        print(f"{kernel} numerics qpg={qpg} fp8={int(fp8)} B={B} ctx={ctx} "
              f"np={np_}: max|d|={diff:.4f} {status}")


def bench(B, ctx, np_=None, part=512, iters=50, kernel="v1", qpg=4):
    q, kc, vc, bt, sl = make(B, ctx, qpg)
    scale = D ** -0.5

    def run():
        if np_:
            return ext.paged_attention_split(q, kc, vc, bt, sl, np_, part,
                                             scale)
        return ext.paged_attention(q, kc, vc, bt, sl, scale)

    for _ in range(10):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        run()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / iters * 1e6
    kv_gb = B * ctx * KVH * D * 2 * 2 / 1e9
    print(f"B={B:4d} ctx={ctx:5d} np={np_ or 1:2d} {kernel}: {us:8.1f} us  "
          f"({kv_gb / (us / 1e6) / 1e3:6.2f} TB/s effective)")


if __name__ == "__main__" and not {"--chunks", "--kv-scales",
                                   "--medians"} & set(sys.argv):
    for B in (64, 128, 256):
        bench(B, 1152)
        for np_ in (2, 4):
            part = ((1152 + np_ - 1) // np_ + 255) // 256 * 256
            bench(B, 1152, np_=np_, part=part)
    bench(8, 8192, np_=16, part=512)
    bench(128, 1536)



def bench_chunk(B, ctx, chunk, iters=50, qpg=4):
    q, kc, vc, bt, sl = make(B, ctx, qpg)
    scale = D ** -0.5
    ref = ext.paged_attention(q, kc, vc, bt, sl, scale, 256)
    got = ext.paged_attention(q, kc, vc, bt, sl, scale, chunk)
    diff = (ref.float() - got.float()).abs().max().item()
    for _ in range(10):
        ext.paged_attention(q, kc, vc, bt, sl, scale, chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ext.paged_attention(q, kc, vc, bt, sl, scale, chunk)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / iters * 1e6
    kv_gb = B * ctx * KVH * D * 2 * 2 / 1e9
    print(f"B={B:4d} ctx={ctx:5d} chunk={chunk}: {us:8.1f} us "
          f"({kv_gb / (us / 1e6) / 1e3:6.2f} TB/s) max|d|={diff:.4f}")


if __name__ == "__main__" and "--chunks" in sys.argv:
    for B in (64, 128, 256):
        for chunk in (256, 512):
            bench_chunk(B, 1152, chunk)
    bench_chunk(128, 2048, 256)
    bench_chunk(128, 2048, 512)


# ---- fp8 KV with per-head scales ------------------------------------------

def kv_scales(seed=0):
    """Per-head (k_scale, v_scale): powers of two next to values that are
    not, all far from 1 so a dropped or misplaced scale shows."""
    g = torch.Generator().manual_seed(seed)
    ks = torch.tensor([2.0 ** -3, 0.7, 2.0 ** 2, 1.9] * (KVH // 4))
    vs = torch.exp(torch.randn(KVH, generator=g) * 2).float()
    return ks.float().cuda(), vs.cuda()


def check_scaled(qpg=4):
    """Scaled kernels against ops.ref on the same bytes and scales."""
    from llm_d_inference_scheduler_amd.ops import ref
    ks, vs = kv_scales()
    for B, ctx, np_, part in ((4, 300, 1, 0), (8, 1152, 1, 0),
                              (8, 1152, 4, 512), (3, 70, 1, 0)):
        q, kc, vc, bt, sl = make(B, ctx, qpg, fp8=True)
        scale = D ** -0.5
        if np_ > 1:
            got = ext.paged_attention_split(q, kc, vc, bt, sl, np_, part,
                                            scale, 256, ks, vs)
        else:
            got = ext.paged_attention(q, kc, vc, bt, sl, scale, 256, ks, vs)
        want = ref.paged_attention(q.float().cpu(), kc.cpu(), vc.cpu(),
                                   bt.cpu(), sl.cpu(), scale,
                                   k_scale=ks.cpu(), v_scale=vs.cpu())
        rel = ((got.float().cpu() - want).norm(dim=-1) /
               want.norm(dim=-1)).max().item()
        status = "OK" if rel < 2.0 ** -6 else "FAIL"
        print(f"scaled numerics qpg={qpg} B={B} ctx={ctx} np={np_}: "
              f"max row rel err={rel:.2e} {status}")


def time_us(run, iters=50, repeats=7):
    """Median over `repeats` of the mean time of `iters` launches."""
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) / iters * 1e6)
    samples.sort()
    return samples[len(samples) // 2], samples[0], samples[-1]


STANDARD_SHAPES = (
    [(B, 1152, np_, ((1152 + np_ - 1) // np_ + 255) // 256 * 256 if np_
      else 0) for B in (64, 128, 256) for np_ in (None, 2, 4)]
    + [(8, 8192, 16, 512), (128, 1536, None, 0)])


def bench_medians(qpg=4):
    scale = D ** -0.5
    for fp8 in (False, True):
        for B, ctx, np_, part in STANDARD_SHAPES:
            q, kc, vc, bt, sl = make(B, ctx, qpg, fp8)
            if np_:
                med, lo, hi = time_us(lambda: ext.paged_attention_split(
                    q, kc, vc, bt, sl, np_, part, scale))
            else:
                med, lo, hi = time_us(lambda: ext.paged_attention(
                    q, kc, vc, bt, sl, scale))
            print(f"{'fp8 ' if fp8 else 'bf16'} B={B:4d} ctx={ctx:5d} "
                  f"np={np_ or 1:2d}: {med:8.1f} us [{lo:.1f}, {hi:.1f}]")


def bench_scaled(B, ctx, np_=None, part=512, qpg=4):
    """Unscaled and scaled fp8 on the same tensors, timed alternately."""
    q, kc, vc, bt, sl = make(B, ctx, qpg, fp8=True)
    ks, vs = kv_scales()
    scale = D ** -0.5

    def run(k_scale, v_scale):
        if np_:
            return lambda: ext.paged_attention_split(
                q, kc, vc, bt, sl, np_, part, scale, 256, k_scale, v_scale)
        return lambda: ext.paged_attention(q, kc, vc, bt, sl, scale, 256,
                                           k_scale, v_scale)

    plain, scaled = [], []
    for _ in range(3):
        plain.append(time_us(run(None, None), repeats=3)[0])
        scaled.append(time_us(run(ks, vs), repeats=3)[0])
    plain.sort()
    scaled.sort()
    kv_gb = B * ctx * KVH * D * 2 / 1e9          # one byte per element
    print(f"B={B:4d} ctx={ctx:5d} np={np_ or 1:2d} fp8: unscaled "
          f"{plain[1]:8.1f} us [{plain[0]:.1f}, {plain[2]:.1f}]  scaled "
          f"{scaled[1]:8.1f} us [{scaled[0]:.1f}, {scaled[2]:.1f}]  "
          f"ratio {scaled[1] / plain[1]:.3f}  "
          f"({kv_gb / (scaled[1] / 1e6) / 1e3:5.2f} TB/s scaled)")


if __name__ == "__main__" and "--medians" in sys.argv:
    bench_medians()

if __name__ == "__main__" and "--kv-scales" in sys.argv:
    check_scaled()
    for B, ctx, np_, part in STANDARD_SHAPES:
        bench_scaled(B, ctx, np_=np_, part=part)
