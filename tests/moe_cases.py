"""Cases, the float64 reference and the error bound of the MoE ops
(DEVELOPMENT.md "Mixture of experts"), shared by test_moe_cpu.py and
test_gpu_moe.py. Everything is built on the device it is asked for, so the
large case costs the CPU nothing."""
import torch

# (T, H, I, E, k, routing): "random" draws k distinct experts per token,
# "two" sends every token to experts 0 and 1.
FFN_CASES = {
    "one": (1, 64, 16, 2, 1, "random"),
    "straddle16": (17, 192, 48, 8, 2, "two"),     # segments of 17, 6 empty
    "uneven_k": (65, 2112, 1040, 128, 8, "random"),   # MB 1, K uneven
    "mb2": (65, 192, 48, 8, 2, "random"),
    "mb4": (130, 64, 48, 4, 2, "two"),            # segments of 130
    "ring": (16, 4096, 48, 8, 2, "random"),       # the ring's steady state
}


def ffn_case(name, device, dtype=torch.bfloat16):
    """(x, w13, w2, ids, w) of FFN_CASES[name]: x rows differ in magnitude,
    the routing weights of a token are positive and sum to 1."""
    T, H, I, E, k, routing = FFN_CASES[name]
    gen = torch.Generator(device=device).manual_seed(len(name) + T)
    randn = lambda *s: torch.randn(*s, generator=gen, device=device)
    x = randn(T, H) * (1 + torch.arange(T, device=device) % 7)[:, None]
    w13 = randn(E, 2 * I, H) / H ** 0.5
    w2 = randn(E, H, I) / I ** 0.5
    if routing == "two":
        ids = torch.arange(2, device=device).repeat(T, 1)[:, :k]
    else:
        ids = torch.rand(T, E, generator=gen, device=device).argsort(1)[:, :k]
    w = torch.rand(T, k, generator=gen, device=device) + 0.1
    w = w / w.sum(1, keepdim=True)
    return (x.to(dtype), w13.to(dtype), w2.to(dtype), ids.to(torch.int32), w)


def ffn_float64(x, w13, w2, ids, w):
    """(y64, bound), both [T, H] float64: a loop over experts in float64, and
    the error a conforming moe_ffn may have per element, composed from its
    rounding points: fp32 sums of K terms (K * 2^-23 of the absolute sum, for
    both GEMMs), silu and the product in fp32, one bf16 rounding of the
    activation (2^-9) carried through |W2| and w, the fp32 weighting and slot
    sum, and the final rounding (2^-8 |y64|)."""
    T, H = x.shape
    I, k = w13.shape[1] // 2, ids.shape[1]
    x64, w64 = x.double(), w.double()
    y64 = torch.zeros(T, H, dtype=torch.float64, device=x.device)
    err = torch.zeros_like(y64)
    for e in range(w13.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        W13, W2 = w13[e].double(), w2[e].double().t()
        g, u = (x64[t] @ W13.t()).split(I, dim=-1)
        bg, bu = (H * 2.0 ** -23 * (x64[t].abs() @ W13.abs().t())).split(
            I, dim=-1)
        silu = g * torch.sigmoid(g)
        a = silu * u
        # |silu'| <= 1.1
        da = 1.1 * bg * u.abs() + silu.abs() * bu + 1.1 * bg * bu + \
            2.0 ** -21 * a.abs()
        a_err = 2.0 ** -9 * a.abs() + 1.01 * da
        wt = w64[t, j][:, None]
        y64.index_put_((t,), wt * (a @ W2), accumulate=True)
        z_abs = a.abs() @ W2.abs()
        err.index_put_((t,), wt * (
            1.01 * (a_err @ W2.abs()) +
            I * 2.0 ** -23 * ((a.abs() + a_err) @ W2.abs()) +
            (k + 2) * 2.0 ** -23 * z_abs), accumulate=True)
    return y64, err + 2.0 ** -8 * y64.abs()


def ffn_excess(y, x, w13, w2, ids, w):
    """max over elements of |y - y64| - bound: <= 0 for a conforming y."""
    y64, bound = ffn_float64(x, w13, w2, ids, w)
    return float(((y.double() - y64).abs() - bound).max())


# (T, H, E, k)
ROUTE_CASES = [(1, 64, 2, 1), (17, 192, 8, 2), (16, 2112, 128, 8),
               (33, 256, 40, 8), (5, 64, 256, 8)]


def route_case(T, H, E, device, dtype=torch.bfloat16):
    gen = torch.Generator(device=device).manual_seed(T * 1000 + E)
    x = torch.randn(T, H, generator=gen, device=device) * \
        (0.25 * (1 + torch.arange(T, device=device) % 5))[:, None]
    router = torch.randn(E, H, generator=gen, device=device) / H ** 0.5
    return x.to(dtype), router.to(dtype)


def check_route(ids, w, x, router, k, renorm):
    """ids / w of a moe_route against float64. With b_t = H * 2^-23 * max_e
    sum |x||r| bounding the error of an fp32 logit: the ids of a token are
    distinct; every chosen logit is within 2 b_t of the k-th largest; and w
    is the float64 softmax (over the chosen ids with renorm) to the relative
    error a shift of every logit by up to b_t allows, exp(2 b_t) - 1, plus
    the fp32 steps: exp of a difference d (|d| 2^-24 and a few ulps), a sum
    of E terms, a division, and with renorm a sum of k terms and another."""
    T, H = x.shape
    E = router.shape[0]
    x64, r64 = x.double(), router.double()
    L = x64 @ r64.t()
    b = H * 2.0 ** -23 * (x64.abs() @ r64.abs().t()).amax(1)
    ids = ids.long()
    assert ids.min() >= 0 and ids.max() < E
    assert all(len(set(row)) == k for row in ids.tolist())
    chosen = L.gather(1, ids)
    kth = L.sort(1, descending=True).values[:, k - 1]
    assert bool((chosen >= (kth - 2 * b)[:, None]).all())
    p = torch.softmax(L, 1).gather(1, ids)
    if renorm:
        p = p / p.sum(1, keepdim=True)
    spread = L.amax(1) - chosen.amin(1)
    tol = torch.expm1(2 * b) + (E + k + 8 + spread) * 2.0 ** -23
    rel = ((w.double() - p).abs() / p).amax(1)
    print(f"MOE_ROUTE|T={T} H={H} E={E} k={k} renorm={renorm}|"
          f"rel/tol={float((rel / tol).max()):.3f}")
    assert bool((rel <= tol).all())
