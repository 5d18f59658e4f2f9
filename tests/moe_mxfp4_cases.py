"""Cases of ops.moe_ffn_mxfp4 (DEVELOPMENT.md "Mixture of experts"), shared by
test_moe_mxfp4_cpu.py and test_gpu_moe_mxfp4.py. They are judged by the
float64 bound of moe_cases on the dequantised experts, which applies
unchanged: the dequantisation is exact and every value of it is a bf16."""
import torch

from llm_d_inference_scheduler_amd.ops import ref

# (T, H, I, E, k, routing) as in moe_cases.FFN_CASES
CASES = {
    "one_group": (1, 32, 32, 2, 1, "random"),     # one live lane group
    "tail": (17, 160, 96, 8, 2, "two"),           # K = 128 + 32 and 3 groups
    "mb2": (65, 256, 64, 8, 2, "random"),
    "tall": (130, 128, 64, 4, 2, "two"),          # moe_mb says 4: 32-row tiles
    "ring": (16, 4160, 64, 8, 2, "random"),       # steady state, 2-group tail
    # the tail shape with every (expert, row, group) times 2^n, n uniform in
    # [-12, 12]: neighbouring groups get different scale bytes, which plain
    # Gaussian weights never do
    "scales": (17, 160, 96, 8, 2, "two"),
}


def build(name, device):
    """((x, w13q, w13s, w2q, w2s, ids, w), (w13, w2)): the arguments of
    moe_ffn_mxfp4 and the dequantised experts in bf16. x rows differ in
    magnitude; a token's routing weights are positive and sum to 1."""
    T, H, I, E, k, routing = CASES[name]
    gen = torch.Generator(device=device).manual_seed(len(name) + T)
    randn = lambda *s: torch.randn(*s, generator=gen, device=device)
    x = randn(T, H) * (1 + torch.arange(T, device=device) % 7)[:, None]
    w13 = (randn(E, 2 * I, H) / H ** 0.5).bfloat16()
    w2 = (randn(E, H, I) / I ** 0.5).bfloat16()
    if name == "scales":
        for t in (w13, w2):
            n = torch.randint(-12, 13, (E, t.shape[1], t.shape[2] // 32, 1),
                              generator=gen, device=device)
            t.copy_((t.float().unflatten(2, (-1, 32)) * 2.0 ** n).flatten(2))
    if routing == "two":
        ids = torch.arange(2, device=device).repeat(T, 1)[:, :k]
    else:
        ids = torch.rand(T, E, generator=gen, device=device).argsort(1)[:, :k]
    w = torch.rand(T, k, generator=gen, device=device) + 0.1
    w = w / w.sum(1, keepdim=True)
    q13, q2 = ref.quantize_experts_mxfp4(w13), ref.quantize_experts_mxfp4(w2)
    dense = tuple(ref.dequant_experts_mxfp4(*q, dtype=torch.bfloat16)
                  for q in (q13, q2))
    return (x.bfloat16(), *q13, *q2, ids.to(torch.int32), w), dense
