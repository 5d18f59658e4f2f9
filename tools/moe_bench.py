"""Microbench of the MoE layer (ops.moe_route + ops.moe_ffn) at
Qwen3-30B-A3B shapes (results: profiles/moe.md).

    python tools/moe_bench.py [--rounds 7] [--copies 8]
                              [--weights mxfp4|fp8|fp8_a8|fp8_block128]

One layer: H 2048, 128 experts of I 768, 8 a token, for T in {1, 16, 64, 256,
1024, 4096}. Arms, timed in one process in interleaved rounds (arm order
rotates each round) with device events around a window of back-to-back calls
(enough for 10 ms of device time), on random data:
  kernel   ops.moe_route, then ops.moe_ffn with a resident scratch, as the
           runner calls them: five launches and no host synchronisation
  torch    the same math composed from torch ops: matmul, softmax, topk, and
           per expert nonzero + index_select + two matmuls + index_add. The
           nonzero makes the host wait once per expert; that wait is part of
           what the composition costs.
A decode step streams every layer's weights, so a layer's experts are cold
when its FFN starts. Each arm therefore walks round-robin over --copies
copies of the layer (router, w13, w2) and as many different x: a call never
finds its experts where the call before left them, as long as copies times
the touched bytes exceed the 256 MB Infinity Cache (at T = 1 that needs 4).
Before a T is timed, both arms are compared with float64 under the bound of
tests/moe_cases.py.
Reported per arm: the median per-call time over the rounds and the largest
minus the smallest round, in us; `floor` is the bytes of the router and of
the experts the calls actually touch (mean over the copies) over 8 TB/s;
`experts` is that mean count.

--weights mxfp4 (results: profiles/moe_mxfp4.md) quantises every copy's
experts with ops.ref.quantize_weight_mxfp4 and times two arms instead:
  mxfp4    ops.moe_route, then ops.moe_ffn_mxfp4 on the MXFP4 pairs
  bf16     ops.moe_route, then ops.moe_ffn on the dequantised bf16 copy of
           the same experts: the same function, bit for bit in exact terms
`floor` is then that of the mxfp4 arm, 4.25 bits a weight (codes and scale
bytes), and `floor_bf16` the bf16 arm's. The mxfp4 output is checked against
the float64 bound on the dequantised experts before each T is timed.

--weights fp8 (results: profiles/moe_fp8.md) does the same with
ops.ref.quantize_experts_fp8:
  fp8      ops.moe_route, then ops.moe_ffn_fp8 on the fp8 pairs
  bf16     ops.moe_route, then ops.moe_ffn on the dequantised experts rounded
           to bf16 (an fp8 weight times its scale is not a bf16, so this arm
           computes a neighbouring function, at the same cost)
`floor` is 1 byte a weight plus the fp32 scales of the touched experts. The
fp8 output is checked against the float64 bound on the float64 experts
wq * scale before each T is timed, the bf16 arm on its own bf16 experts.

--weights fp8_a8 (results: profiles/moe_fp8_a8.md) times the two ops the
runner chooses between on fp8 experts, for T in {64, 128, ..., 4096}:
  fp8_a8   ops.moe_route, then ops.moe_ffn_fp8_a8: fp8 activations, LDS-staged
           tiles on the fp8 MFMA
  fp8      ops.moe_route, then ops.moe_ffn_fp8: bf16 activations, the skinny
           kernels
`rows` is the mean rows per expert T k / E, the unit of the runner's
_moe_a8_min_rows, and `ratio` fp8 over fp8_a8. At T = 64 the fp8_a8 output is
judged by the two-stage float64 bound of tests/moe_fp8_a8_cases.py; at every
larger T its first 64 rows must be those bits again (a row's bits do not
depend on the batch).

--weights fp8_block128 (results: profiles/moe_fp8_block.md) times
ops.moe_ffn_fp8_block on block-scaled experts for T in {1, 16, ..., 4096}:
  block     as served (moe_fp8_block_tile)
  block16   the 16-row registers-only kernels forced
  block64   the 64-row LDS tiles forced
  fp8_a8, fp8   ops.moe_ffn_fp8_a8 and ops.moe_ffn_fp8 on per-channel pairs of
            the same experts, for context
  quant_x, quant_act   ops.quantize_groups_fp8 on [T, H] and on [T k, I]: the
            two quantiser passes on their own
Every arm but the last two includes ops.moe_route. `floor` is 1 byte a weight
plus the block scales of the touched experts, the router, and x in and y out.
Up to T = 64 both forced arms are judged by the two-stage float64 bound of
tests/moe_fp8_block_cases.py before they are timed.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import moe_cases  # noqa: E402
import moe_fp8_a8_cases  # noqa: E402
import moe_fp8_block_cases  # noqa: E402
from llm_d_inference_scheduler_amd import ops  # noqa: E402
from llm_d_inference_scheduler_amd.models.configs import (  # noqa: E402
    QWEN3_30B_A3B)

DEV = "cuda"
TS = (1, 16, 64, 256, 1024, 4096)
TS_A8 = (64, 128, 256, 512, 1024, 2048, 4096)
WINDOW_US = 10000.0
HBM_BYTES_PER_US = 8e6


def time_arm(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # us per call


def bench(fns, rounds):
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


def torch_route(x, router, k):
    p = torch.softmax(x.float() @ router.float().t(), dim=-1)
    w, ids = torch.topk(p, k, dim=-1)
    return ids, w / w.sum(dim=-1, keepdim=True)


def torch_moe(x, router, w13, w2, k):
    """The layer from torch ops, bf16 GEMMs, per expert over its rows."""
    ids, w = torch_route(x, router, k)
    I = w2.shape[2]
    y = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(w13.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        g, u = (x.index_select(0, t) @ w13[e].t()).split(I, dim=-1)
        act = torch.nn.functional.silu(g) * u
        y.index_add_(0, t, (act @ w2[e].t()).float() * w[t, j][:, None])
    return y.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--weights", choices=["bf16", "mxfp4", "fp8", "fp8_a8",
                                          "fp8_block128"], default="bf16")
    args = ap.parse_args()
    ops.hip_ops()
    c = QWEN3_30B_A3B
    H, I, E, k = (c.hidden_size, c.moe_intermediate_size, c.num_experts,
                  c.experts_per_token)
    gen = torch.Generator(device=DEV).manual_seed(0)
    randn = lambda *s: torch.randn(*s, generator=gen, device=DEV)
    n = args.copies
    routers = [randn(E, H).mul_(0.02).bfloat16() for _ in range(n)]
    w13s = [randn(E, 2 * I, H).mul_(0.02).bfloat16() for _ in range(n)]
    w2s = [randn(E, H, I).mul_(0.02).bfloat16() for _ in range(n)]
    expert_bytes = 3 * I * H * 2
    if args.weights == "fp8_a8":
        return main_fp8_a8(args, routers, w13s, w2s, randn)
    if args.weights == "fp8_block128":
        return main_fp8_block(args, routers, w13s, w2s, randn)
    if args.weights != "bf16":
        return main_quantised(args, routers, w13s, w2s, randn)
    for T in TS:
        xs = [randn(T, H).bfloat16() for _ in range(n)]
        scratch = torch.empty(ops.moe_scratch_bytes(T, k, E, H, I),
                              dtype=torch.uint8, device=DEV)

        def kernel(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn(xs[i], w13s[i], w2s[i], ids, w, scratch)

        def composed(i):
            return torch_moe(xs[i], routers[i], w13s[i], w2s[i], k)

        ids, w = ops.moe_route(xs[0], routers[0], k, True)
        moe_cases.check_route(ids, w, xs[0], routers[0], k, True)
        for what, y in (("kernel", kernel(0)), ("torch", composed(0))):
            excess = moe_cases.ffn_excess(y, xs[0], w13s[0], w2s[0], ids, w)
            # the composition rounds g, u and the expert output to bf16 as
            # well: three more half-ulps of |y| than the bound allows for
            if excess > 0 and what == "kernel":
                raise SystemExit(f"T={T} {what}: excess {excess:.3e}")
            print(f"# T={T} {what} excess {excess:.3e}", flush=True)
        touched = statistics.mean(
            int(torch_route(xs[i], routers[i], k)[0].unique().numel())
            for i in range(n))
        fns = {"kernel": rotating(kernel, n), "torch": rotating(composed, n)}
        print(json.dumps(dict(
            T=T, H=H, I=I, E=E, k=k, copies=n, experts=round(touched, 1),
            floor=round((touched * expert_bytes + E * H * 2)
                        / HBM_BYTES_PER_US, 2),
            **bench(fns, args.rounds))), flush=True)
        del xs, scratch


def main_quantised(args, routers, w13s, w2s, randn):
    """--weights mxfp4 / fp8: the quantised arm against the bf16 kernels on a
    bf16 copy of the same experts."""
    fmt = args.weights
    n, (E, _, H), I = args.copies, w13s[0].shape, w2s[0].shape[2]
    k = QWEN3_30B_A3B.experts_per_token
    ref = ops.ref
    quantize, dequant, ffn_q, bits = {
        "mxfp4": (ref.quantize_experts_mxfp4, ref.dequant_experts_mxfp4,
                  ops.moe_ffn_mxfp4, 4.25),
        "fp8": (ref.quantize_experts_fp8, ref.dequant_experts_fp8,
                ops.moe_ffn_fp8, 8.0)}[fmt]
    q13s, q2s = [], []
    for i in range(n):      # each bf16 copy becomes its own dequantisation
        q13s.append(quantize(w13s[i]))
        q2s.append(quantize(w2s[i]))
        w13s[i] = dequant(*q13s[i], dtype=torch.bfloat16)
        w2s[i] = dequant(*q2s[i], dtype=torch.bfloat16)
    # what the quantised arm is judged on: for mxfp4 the bf16 copy is exact;
    # an fp8 weight times its scale is not a bf16, so float64 holds it
    exact = (w13s[0], w2s[0]) if fmt == "mxfp4" else tuple(
        wq.double() * sc.double()[..., None] for wq, sc in (q13s[0], q2s[0]))
    weights = 3 * I * H
    scale_bytes = 0 if fmt == "mxfp4" else (2 * I + H) * 4   # per expert
    mx = fmt == "mxfp4"
    for T in TS:
        xs = [randn(T, H).bfloat16() for _ in range(n)]
        scratch = {q: torch.empty(
            ops.moe_scratch_bytes(T, k, E, H, I, mxfp4=q and mx),
            dtype=torch.uint8, device=DEV) for q in (True, False)}

        def quantised(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ffn_q(xs[i], *q13s[i], *q2s[i], ids, w, scratch[True])

        def bf16(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn(xs[i], w13s[i], w2s[i], ids, w, scratch[False])

        ids, w = ops.moe_route(xs[0], routers[0], k, True)
        for what, y, (e13, e2) in ((fmt, quantised(0), exact),
                                   ("bf16", bf16(0), (w13s[0], w2s[0]))):
            excess = moe_cases.ffn_excess(y, xs[0], e13, e2, ids, w)
            if excess > 0:
                raise SystemExit(f"T={T} {what}: excess {excess:.3e}")
            print(f"# T={T} {what} excess {excess:.3e}", flush=True)
        touched = statistics.mean(
            int(torch_route(xs[i], routers[i], k)[0].unique().numel())
            for i in range(n))
        fns = {fmt: rotating(quantised, n), "bf16": rotating(bf16, n)}
        floor = lambda bits, extra: round(
            (touched * (weights * bits / 8 + extra) + E * H * 2)
            / HBM_BYTES_PER_US, 2)
        print(json.dumps(dict(
            T=T, H=H, I=I, E=E, k=k, copies=n, experts=round(touched, 1),
            floor=floor(bits, scale_bytes), floor_bf16=floor(16, 0),
            **bench(fns, args.rounds))), flush=True)
        del xs, scratch


def main_fp8_a8(args, routers, w13s, w2s, randn):
    """--weights fp8_a8: ops.moe_ffn_fp8_a8 against ops.moe_ffn_fp8 on the
    same fp8 experts."""
    n, (E, _, H), I = args.copies, w13s[0].shape, w2s[0].shape[2]
    k = QWEN3_30B_A3B.experts_per_token
    quantize = ops.ref.quantize_experts_fp8
    q13s, q2s = [], []
    for i in range(n):
        q13s.append(quantize(w13s[i]))
        q2s.append(quantize(w2s[i]))
        w13s[i] = w2s[i] = None
    x0 = randn(max(TS_A8), H).bfloat16()    # copy 0's x at every T: a prefix
    y_first = None
    for T in TS_A8:
        xs = [x0[:T]] + [randn(T, H).bfloat16() for _ in range(n - 1)]
        scratch = {
            "fp8_a8": ops.moe_fp8_a8_scratch_bytes(T, k, E, H, I),
            "fp8": ops.moe_scratch_bytes(T, k, E, H, I)}
        scratch = {a: torch.empty(b, dtype=torch.uint8, device=DEV)
                   for a, b in scratch.items()}

        def a8(i, **kw):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn_fp8_a8(xs[i], *q13s[i], *q2s[i], ids, w,
                                      scratch["fp8_a8"], **kw)

        def fp8(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn_fp8(xs[i], *q13s[i], *q2s[i], ids, w,
                                   scratch["fp8"])

        if y_first is None:
            ids, w = ops.moe_route(xs[0], routers[0], k, True)
            act = torch.empty(T * k, I, dtype=torch.bfloat16, device=DEV)
            y_first = a8(0, act_out=act)
            cpu = [t.cpu() for t in (xs[0], *q13s[0], *q2s[0], ids, w)]
            dense = tuple(wq.double() * sc.double()[..., None]
                          for wq, sc in ((cpu[1], cpu[2]), (cpu[3], cpu[4])))
            e1, e2 = moe_fp8_a8_cases.excess(y_first.cpu(), act.cpu(), cpu,
                                             dense)
            if e1 > 0 or e2 > 0:
                raise SystemExit(f"T={T} fp8_a8: excess {e1:.3e} {e2:.3e}")
            print(f"# T={T} fp8_a8 excess {e1:.3e} {e2:.3e}", flush=True)
        elif not torch.equal(a8(0)[:y_first.shape[0]], y_first):
            raise SystemExit(f"T={T} fp8_a8: the first rows changed")
        fns = {"fp8_a8": rotating(a8, n), "fp8": rotating(fp8, n)}
        res = bench(fns, args.rounds)
        print(json.dumps(dict(
            T=T, H=H, I=I, E=E, k=k, copies=n, rows=T * k / E, **res,
            ratio=round(res["fp8"] / res["fp8_a8"], 2))), flush=True)
        del xs, scratch


def main_fp8_block(args, routers, w13s, w2s, randn):
    """--weights fp8_block128: ops.moe_ffn_fp8_block as served and with each
    kernel family forced, with ops.moe_ffn_fp8 and ops.moe_ffn_fp8_a8 on
    per-channel pairs of the same experts for context."""
    n, (E, _, H), I = args.copies, w13s[0].shape, w2s[0].shape[2]
    k = QWEN3_30B_A3B.experts_per_token
    ref, ext = ops.ref, ops.hip_ops()
    b13s, b2s, q13s, q2s = [], [], [], []
    for i in range(n):
        b13s.append(ref.quantize_experts_fp8_block(w13s[i], halves=2))
        b2s.append(ref.quantize_experts_fp8_block(w2s[i]))
        q13s.append(ref.quantize_experts_fp8(w13s[i]))
        q2s.append(ref.quantize_experts_fp8(w2s[i]))
        w13s[i] = w2s[i] = None
    scale_bytes = (b13s[0][1][0].numel() + b2s[0][1][0].numel()) * 4
    for T in TS:
        xs = [randn(T, H).bfloat16() for _ in range(n)]
        acts = [randn(T * k, I).bfloat16() for _ in range(n)]
        scratch = {
            "block": ops.moe_fp8_block_scratch_bytes(T, k, E, H, I),
            "fp8_a8": ops.moe_fp8_a8_scratch_bytes(T, k, E, H, I),
            "fp8": ops.moe_scratch_bytes(T, k, E, H, I)}
        scratch = {a: torch.empty(b, dtype=torch.uint8, device=DEV)
                   for a, b in scratch.items()}

        def block(tile):
            def call(i, act_out=None):
                ids, w = ops.moe_route(xs[i], routers[i], k, True)
                return ext.moe_ffn_fp8_block(xs[i], *b13s[i], *b2s[i], ids, w,
                                             scratch["block"], tile, act_out)
            return call

        def a8(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn_fp8_a8(xs[i], *q13s[i], *q2s[i], ids, w,
                                      scratch["fp8_a8"])

        def fp8(i):
            ids, w = ops.moe_route(xs[i], routers[i], k, True)
            return ops.moe_ffn_fp8(xs[i], *q13s[i], *q2s[i], ids, w,
                                   scratch["fp8"])

        if T <= 64:     # judged on the CPU: small batches only
            ids, w = ops.moe_route(xs[0], routers[0], k, True)
            cpu = [t.cpu() for t in (xs[0], *b13s[0], *b2s[0], ids, w)]
            dense = (ref.dequant_experts_fp8_block(cpu[1], cpu[2], halves=2,
                                                   dtype=torch.float64),
                     ref.dequant_experts_fp8_block(cpu[3], cpu[4],
                                                   dtype=torch.float64))
            for tile in (16, 64):
                act = torch.empty(T * k, I, dtype=torch.bfloat16, device=DEV)
                y = block(tile)(0, act)
                e1, e2 = moe_fp8_block_cases.excess(y.cpu(), act.cpu(), cpu,
                                                    dense)
                if e1 > 0 or e2 > 0:
                    raise SystemExit(
                        f"T={T} tile {tile}: excess {e1:.3e} {e2:.3e}")
                print(f"# T={T} tile {tile} excess {e1:.3e} {e2:.3e}",
                      flush=True)
        touched = statistics.mean(
            int(torch_route(xs[i], routers[i], k)[0].unique().numel())
            for i in range(n))
        fns = {"block": rotating(block(0), n),
               "block16": rotating(block(16), n),
               "block64": rotating(block(64), n),
               "fp8_a8": rotating(a8, n), "fp8": rotating(fp8, n),
               # the two quantiser passes on their own (they allocate their
               # outputs, which the op does not)
               "quant_x": rotating(
                   lambda i: ops.quantize_groups_fp8(xs[i]), n),
               "quant_act": rotating(
                   lambda i: ops.quantize_groups_fp8(acts[i]), n)}
        res = bench(fns, args.rounds)
        print(json.dumps(dict(
            T=T, H=H, I=I, E=E, k=k, copies=n, rows=T * k / E,
            experts=round(touched, 1),
            floor=round((touched * (3 * I * H + scale_bytes) + E * H * 2 +
                         T * H * 4) / HBM_BYTES_PER_US, 2),
            **res)), flush=True)
        del xs, acts, scratch


if __name__ == "__main__":
    main()
