"""Cases and the two-stage float64 judge of ops.moe_ffn_fp8_block
(DEVELOPMENT.md "Mixture of experts"), shared by test_moe_fp8_block_cpu.py and
test_gpu_moe_fp8_block.py: moe_fp8_a8_cases with both quantisers per 128-wide
group and the experts block-scaled."""
import torch

from llm_d_inference_scheduler_amd.ops import ref
from moe_fp8_a8_cases import C

# (T, H, I, E, k, routing); K = H for gate-up, I for down, in 128-wide groups
CASES = {
    "one": (1, 64, 64, 2, 1, "random"),      # both K: the zero-filled tail alone
    # segments of 17: a full short tile plus one row; K = 128 + 64 and 2 * 128
    # + 64; I = 320: the up half's blocks start at row 320 and each half's
    # last block is 64 rows; H = 192: a ragged second block row of w2s and a
    # masked column tile in down; x[2] = 0: scale 1 in both quantisers
    "tails": (17, 192, 320, 8, 2, "two"),
    "ragged": (65, 192, 64, 8, 2, "random"),
    # segments of 64 + 64 + 2 rows at tile 64, nine short tiles at 16
    "tall": (130, 128, 128, 4, 2, "two"),
    # The skinny kernels' waves take the groups round-robin, wave v gets
    # ceil((G - v) / 4) of them, and run unchecked rounds of the ring (3
    # stages) while 2 * 3 groups are left. H = 3072: G = 24, six a wave, so
    # every wave runs one unchecked round and a checked one. I = 3136: G = 25
    # with a 64-wide tail group, which wave 0 takes as its seventh (one
    # unchecked round, then checked rounds of 3 and 1). The tiled kernels run
    # 24 and 25 slabs.
    "deep_h": (16, 3072, 64, 8, 2, "random"),
    "deep_i": (16, 64, 3136, 4, 2, "random"),
    # "tails" with K group g of every expert times 2^-a_g and of x times
    # 2^+a_g, a_g from -6 to 6, and every (expert, half, 128-row block) times
    # 2^n, n uniform in [-12, 12]: a scale read from the wrong expert, half,
    # block row or group is off by orders of magnitude
    "scales": (17, 192, 320, 8, 2, "two"),
}


def _blocks(E, halves, rows, gen):
    """[E, halves * rows, 1]: 2^n per (expert, half, 128-row block)."""
    nb = -(-rows // 128)
    n = torch.randint(-12, 13, (E, halves, nb), generator=gen)
    return torch.exp2(n.float()).repeat_interleave(128, 2)[:, :, :rows] \
        .reshape(E, halves * rows, 1)


def build(name, device):
    """((x, w13q, w13s, w2q, w2s, ids, w), (w13, w2)): the arguments of
    moe_ffn_fp8_block and the dequantised experts in float64. x rows differ
    in magnitude; a token's routing weights are positive and sum to 1."""
    T, H, I, E, k, routing = CASES[name]
    gen = torch.Generator().manual_seed(len(name) + T)
    randn = lambda *s: torch.randn(*s, generator=gen)
    x = randn(T, H) * (1 + torch.arange(T) % 7)[:, None]
    if name in ("tails", "scales"):
        x[2] = 0
    w13, w2 = randn(E, 2 * I, H) / H ** 0.5, randn(E, H, I) / I ** 0.5
    if name == "scales":
        group = lambda K: torch.exp2(torch.linspace(-6, 6, -(-K // 128))
                                     .repeat_interleave(128)[:K])
        x = x * group(H)
        w13 = w13 / group(H) * _blocks(E, 2, I, gen)
        w2 = w2 / group(I) * _blocks(E, 1, H, gen)
    if routing == "two":
        ids = torch.arange(2).repeat(T, 1)[:, :k]
    else:
        ids = torch.rand(T, E, generator=gen).argsort(1)[:, :k]
    w = torch.rand(T, k, generator=gen) + 0.1
    w = w / w.sum(1, keepdim=True)
    q13 = ref.quantize_experts_fp8_block(w13.bfloat16(), halves=2)
    q2 = ref.quantize_experts_fp8_block(w2.bfloat16())
    dense = (ref.dequant_experts_fp8_block(*q13, halves=2, dtype=torch.float64),
             ref.dequant_experts_fp8_block(*q2, dtype=torch.float64))
    args = (x.bfloat16(), *q13, *q2, ids.to(torch.int32), w)
    return tuple(a.to(device) for a in args), \
        tuple(d.to(device) for d in dense)


def _dequant_groups(x):
    xq, sx = ref.quantize_groups_fp8(x)
    return xq.double() * sx.double().repeat_interleave(128, 1)[:, :x.shape[1]]


def excess(y, act_out, args, dense):
    """(stage 1, stage 2) of moe_fp8_a8_cases.excess with quantize_groups_fp8
    in place of quantize_rows_fp8: xd = xq * sx[group] and A = aq * sa[group]
    of act_out. The bounds and C(K) are unchanged: the per-group multiply and
    fused add and the wave sums are fp32 operations counted under K
    (test_gpu_linear_fp8_block.py), and the + 2 of stage 1 and the + 4 of
    stage 2 stand for the scale products."""
    x, ids, w = args[0], args[5].long(), args[6].double()
    W13, W2 = dense
    T, H = x.shape
    I, k = W13.shape[1] // 2, ids.shape[1]
    xd, A = _dequant_groups(x), _dequant_groups(act_out)
    e1 = torch.tensor(-float("inf"), dtype=torch.float64, device=x.device)
    y64 = torch.zeros(T, H, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y64)
    for e in range(W13.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        p = t * k + j
        g, u = (xd[t] @ W13[e].t()).split(I, dim=-1)
        bg, bu = ((C(H) + 2) * 2.0 ** -23 *
                  (xd[t].abs() @ W13[e].abs().t())).split(I, dim=-1)
        silu = g * torch.sigmoid(g)
        a = silu * u
        # |silu'| <= 1.1
        da = 1.1 * bg * u.abs() + silu.abs() * bu + 1.1 * bg * bu + \
            2.0 ** -21 * a.abs()
        bound = 2.0 ** -9 * a.abs() + 1.01 * da
        e1 = torch.maximum(
            e1, ((act_out[p].double() - a).abs() - bound).max())
        wt = w[t, j][:, None]
        y64.index_put_((t,), wt * (A[p] @ W2[e].t()), accumulate=True)
        mag.index_put_((t,), wt * (A[p].abs() @ W2[e].abs().t()),
                       accumulate=True)
    bound = 2.0 ** -8 * y64.abs() + (C(I) + k + 4) * 2.0 ** -23 * mag
    return float(e1), float(((y.double() - y64).abs() - bound).max())
