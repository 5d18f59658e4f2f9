"""Cases of ops.moe_ffn_fp8 (DEVELOPMENT.md "Mixture of experts"), shared by
test_moe_fp8_cpu.py and test_gpu_moe_fp8.py. They are judged by the float64
bound of moe_cases on the float64 experts wq * scale: the op differs from what
the bound describes by one fp32 multiply per sum (2^-24), which the bound's
K * 2^-23 term covers."""
import torch

from llm_d_inference_scheduler_amd.ops import ref

# (T, H, I, E, k, routing) as in moe_cases.FFN_CASES; K = H for gate-up, I
# for down, in 64-wide blocks of four 16-wide lane groups
CASES = {
    "one_group": (1, 32, 16, 2, 1, "random"),     # two live groups, and one
    "tail": (17, 160, 112, 8, 2, "two"),          # 2 * 64 + 32 and 64 + 48
    "mb2": (65, 192, 48, 8, 2, "random"),
    "tall": (130, 128, 80, 4, 2, "two"),          # MB 4; one-group tail in down
    "ring": (16, 4160, 64, 8, 2, "random"),       # 65 blocks: 17 / 16 / 16 / 16
    # the tail shape with every (expert, output row) times 2^n, n uniform in
    # [-12, 12], before quantising: a scale read from the wrong row or expert
    # is off by orders of magnitude
    "scales": (17, 160, 112, 8, 2, "two"),
}


def build(name, device):
    """((x, w13q, w13s, w2q, w2s, ids, w), (w13, w2)): the arguments of
    moe_ffn_fp8 and the experts wq * scale in float64. x rows differ in
    magnitude; a token's routing weights are positive and sum to 1."""
    T, H, I, E, k, routing = CASES[name]
    gen = torch.Generator(device=device).manual_seed(len(name) + T)
    randn = lambda *s: torch.randn(*s, generator=gen, device=device)
    x = randn(T, H) * (1 + torch.arange(T, device=device) % 7)[:, None]
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
