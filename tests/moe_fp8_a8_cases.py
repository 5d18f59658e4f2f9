"""Cases and the two-stage float64 judge of ops.moe_ffn_fp8_a8 (DEVELOPMENT.md
"Mixture of experts"), shared by test_moe_fp8_a8_cpu.py and
test_gpu_moe_fp8_a8.py. The op quantises twice, and the second quantiser's
decisions depend on the last bit of act, so it is judged in two stages: act
against float64 on the quantised x, then y against float64 on the quantised
act the op itself produced (act_out)."""
import torch

from llm_d_inference_scheduler_amd.ops import ref

# (T, H, I, E, k, routing) as in moe_cases.FFN_CASES; K = H for gate-up, I
# for down, in 128-byte slabs
CASES = {
    "one": (1, 64, 64, 2, 1, "random"),      # both K: the zero-filled tail alone
    # segments of 17, six empty experts; K = 128 + 64 and 2 * 128 + 64; x[2]
    # = 0: scale 1 in both quantisers; H = 192: a masked column tile in down
    "tails": (17, 192, 320, 8, 2, "two"),
    "ragged": (65, 192, 64, 8, 2, "random"),
    "tall": (130, 128, 128, 4, 2, "two"),    # segments of 64 + 64 + 2, 128 + 2
    "slabs_h": (16, 3072, 64, 8, 2, "random"),   # 24 slabs in gate-up
    "slabs_i": (16, 64, 2112, 4, 2, "random"),   # 16 slabs + tail in down
    # "tails" with every (expert, output row) times 2^n, n uniform in
    # [-12, 12], before quantising: a scale read from the wrong row or expert
    # is off by orders of magnitude
    "scales": (17, 192, 320, 8, 2, "two"),
}

# The coefficient, in units of 2^-23, of the sum of magnitudes in the error of
# a K-term sum on v_mfma_scale_f32_16x16x128_f8f6f4: MFMA_COEFF of
# test_gpu_linear_fp8_a8.py, the instruction's measured summation error
# doubled, and K where K is larger.
def C(K):
    return max(K, 2 * 1718)


def build(name, device):
    """((x, w13q, w13s, w2q, w2s, ids, w), (w13, w2)): the arguments of
    moe_ffn_fp8_a8 and the experts wq * scale in float64. x rows differ in
    magnitude; a token's routing weights are positive and sum to 1."""
    T, H, I, E, k, routing = CASES[name]
    gen = torch.Generator(device=device).manual_seed(len(name) + T)
    randn = lambda *s: torch.randn(*s, generator=gen, device=device)
    x = randn(T, H) * (1 + torch.arange(T, device=device) % 7)[:, None]
    if name in ("tails", "scales"):
        x[2] = 0
    w13 = (randn(E, 2 * I, H) / H ** 0.5).bfloat16()
    w2 = (randn(E, H, I) / I ** 0.5).bfloat16()
    if name == "scales":
        for t in (w13, w2):
            n = torch.randint(-12, 13, (E, t.shape[1], 1), generator=gen,
                              device=device)
            t.copy_(t.float() * 2.0 ** n)
    if routing == "two":
        ids = torch.arange(2, device=device).repeat(T, 1)[:, :k]
    else:
        ids = torch.rand(T, E, generator=gen, device=device).argsort(1)[:, :k]
    w = torch.rand(T, k, generator=gen, device=device) + 0.1
    w = w / w.sum(1, keepdim=True)
    q13, q2 = ref.quantize_experts_fp8(w13), ref.quantize_experts_fp8(w2)
    dense = tuple(wq.double() * scale.double()[..., None]
                  for wq, scale in (q13, q2))
    return (x.bfloat16(), *q13, *q2, ids.to(torch.int32), w), dense


def excess(y, act_out, args, dense):
    """(stage 1, stage 2): the largest |error| - bound, <= 0 for a conforming
    op. Stage 1: act_out against a64 = silu(g) * u on xd = xq * sx and W13,
    under the bound of moe_cases.ffn_float64 with (C(H) + 2) * 2^-23 for the
    sums (the two scale multiplies are the + 2). Stage 2: y against y64[t] =
    sum_j w (A @ W2^T) on A = aq * sa of ref.quantize_rows_fp8(act_out), under
    2^-8 |y64| + (C(I) + k + 4) * 2^-23 * sum_j w (|A| @ |W2|^T): the sum, two
    scale multiplies, the weighting, the slot sum and the last rounding."""
    x, ids, w = args[0], args[5].long(), args[6].double()
    W13, W2 = dense
    T, H = x.shape
    I, k = W13.shape[1] // 2, ids.shape[1]
    xq, sx = ref.quantize_rows_fp8(x)
    xd = xq.double() * sx.double()[:, None]
    aq, sa = ref.quantize_rows_fp8(act_out)
    A = aq.double() * sa.double()[:, None]
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
