"""Routing cost of the batched prefix path on the GPU: hash_prompts_batch +
match_batch for a 64-request admission burst (256 blocks of 16 tokens each)
against a device table holding 100k keys (profiles/prefix_tests.md).

    python tools/prefix_bench.py [package-root]

`package-root` (default: this checkout) lets two builds be timed alternately
from one shell loop. Prints one JSON line: the per-burst time including the
host work of GpuPrefixIndex (list -> tensor, H2D copy), and the two kernels
alone on inputs already on the device; each is the median of 7 windows, every
window ends in a device synchronise."""
import hashlib
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                       os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from llm_d_inference_scheduler_amd import _router_core as rc  # noqa: E402
from llm_d_inference_scheduler_amd.ops.prefix import (GpuPrefixIndex,  # noqa: E402
                                                      _i64)

assert torch.cuda.is_available(), "prefix_bench needs a GPU"
rng = np.random.default_rng(0)
seed0 = rc.model_seed("llama-3-8b", "")
idx = GpuPrefixIndex("cuda:0", capacity_pow2=1 << 21)
prompts = [rng.integers(256, 100000, size=4096).astype(np.int32)
           for _ in range(64)]
# half the burst is known to some endpoint, to varying depth
n_keys = 0
for i in range(0, 64, 2):
    h = rc.hash_tokens(prompts[i], 16, 256, seed0)[: 16 * (1 + i % 16)]
    idx.add(i % 8, h)
    n_keys += len(h)
filler = rng.integers(2, 2**63, size=100_000 - n_keys, dtype=np.uint64)
for e, part in enumerate(np.array_split(filler, 8)):
    idx.add(e, part)
lists = [p.tolist() for p in prompts]


def burst():
    hashes, counts = idx.hash_prompts_batch(lists, 16, 256, seed0)
    return hashes, counts, idx.match_batch(hashes, counts, 8)


flat = torch.from_numpy(np.concatenate(prompts)).cuda()
offs = torch.from_numpy(np.arange(65, dtype=np.int64) * 4096).cuda()


def kernels():
    h, c = idx.ext.hash_prompts(flat, offs, 16, 256, _i64(seed0))
    return idx.ext.match_longest(idx.keys, idx.masks, h, c, 8)


def windows(fn, iters):
    for _ in range(20):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        t = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) / iters * 1e3)
    return ms, out


burst_ms, out = windows(burst, 100)
kernels_ms, _ = windows(kernels, 500)
digest = hashlib.sha256(
    b"".join(x.cpu().numpy().tobytes() for x in out)).hexdigest()[:16]
print(json.dumps({
    "root": root,
    "burst_ms": [round(s, 4) for s in burst_ms],
    "burst_ms_median": round(float(np.median(burst_ms)), 4),
    "kernels_ms": [round(s, 4) for s in kernels_ms],
    "kernels_ms_median": round(float(np.median(kernels_ms)), 4),
    "match_sum": int(out[2].sum()), "outputs_sha256": digest}))
