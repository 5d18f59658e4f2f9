"""The host-side argument contract of the engine bindings (DEVELOPMENT.md
"Op argument contract"): each rule that small tensors can break is broken
once, alone, on the smallest legal call, and must raise before anything is
allocated or launched; next to them the same smallest legal calls go through
and equal ops.ref, and the merged block mover is compared in its three
directions. The grid and narrowing guards (more than 65535 heads, more than
2^31-1 rows or layers) would need huge tensors and are not broken here.

Only what the host can see is tested here. Values that live in device memory
(sequence lengths, block ids, slots, positions) are the caller's obligation
and get no test: a call that breaks them cannot be rejected, only run."""
import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
F16, FP8 = torch.float16, kc.FP8


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def rnd(*shape, dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed + len(shape))
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def zeros(*shape, dtype=I32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


# ---- the smallest legal call of every binding, as keyword arguments ------

def attn_common():
    """B=1, QH=KVH=1, D=128, BS=1, NB=1, MB=1."""
    return dict(q=rnd(1, 1, 128), k_cache=rnd(1, 1, 1, 128, seed=1),
                v_cache=rnd(1, 1, 1, 128, seed=2), block_tables=zeros(1, 1))


def legal_paged_attention():
    return dict(attn_common(), seq_lens=torch.ones(1, dtype=I32, device=DEV),
                scale=128 ** -0.5, chunk=256)


def legal_paged_attention_split():
    a = legal_paged_attention()
    del a["scale"], a["chunk"]
    return dict(a, n_parts=1, part_tokens=256, scale=128 ** -0.5, chunk=256)


def legal_flash_prefill():
    return dict(attn_common(),
                seq_meta=torch.tensor([[0, 1, 0]], dtype=I32, device=DEV),
                tiles=zeros(1, 2), scale=128 ** -0.5)


def legal_rmsnorm():
    return dict(x=rnd(1, 8), w=rnd(8, seed=1), eps=1e-5,
                residual=rnd(1, 8, seed=2))


def legal_rope():
    from llm_d_inference_scheduler_amd.ops import ref
    return dict(q=rnd(1, 1, 2), k=rnd(1, 1, 2, seed=1),
                cos_sin=ref.rope_table(4, 2, 10000.0, device=DEV),
                positions=torch.full((1,), 3, dtype=I32, device=DEV))


def legal_silu_mul():
    return dict(gate_up=rnd(1, 16))


def legal_reshape_and_cache():
    return dict(k_new=rnd(1, 1, 8), v_new=rnd(1, 1, 8, seed=1),
                k_cache=rnd(1, 1, 1, 8, seed=2),
                v_cache=rnd(1, 1, 1, 8, seed=3), slots=zeros(1, dtype=I64))


def legal_move_blocks():
    return dict(pool=rnd(1, 2, 1, 1, 1, 8), staging=rnd(1, 1, 2, 1, 1, 8),
                block_ids=zeros(1), is_scatter=False)


def legal_copy_blocks_peer():
    src = rnd(1, 2, 1, 1, 1, 8, seed=5)
    return dict(src_pool_ptr=src.data_ptr(), dst_pool=rnd(1, 2, 1, 1, 1, 8),
                src_ids=zeros(1), dst_ids=zeros(1), src_nb=1, _keep=src)


LEGAL = {
    "paged_attention": legal_paged_attention,
    "paged_attention_split": legal_paged_attention_split,
    "flash_prefill": legal_flash_prefill,
    "rmsnorm": legal_rmsnorm,
    "rope": legal_rope,
    "silu_mul": legal_silu_mul,
    "reshape_and_cache": legal_reshape_and_cache,
    "move_blocks": legal_move_blocks,
    "copy_blocks_peer": legal_copy_blocks_peer,
}


def call(ext, op, args):
    args = {k: v for k, v in args.items() if not k.startswith("_")}
    return getattr(ext, op)(*args.values())


# ---- one broken rule each: (op, argument(s) replaced, message) -----------
# A callable value is given the legal arguments and returns the replacement.

def strided(t):
    """t's values, shape and dtype, not contiguous."""
    return torch.stack([t, t], dim=-1)[..., 0]


ATTN_RULES = [
    (dict(q=lambda a: a["q"].to(F16)), "q must be BFloat16"),
    (dict(q=lambda a: a["q"].cpu()), "q must be on a GPU"),
    (dict(q=lambda a: strided(a["q"])), "q must be contiguous"),
    (dict(q=lambda a: a["q"][0]), "q must have shape"),
    (dict(q=lambda a: rnd(1, 1, 64)), "q must have shape"),          # D
    (dict(k_cache=lambda a: a["k_cache"].to(F16)), "bf16 or fp8"),
    (dict(k_cache=lambda a: a["k_cache"].cpu()), "k_cache must be on a GPU"),
    (dict(k_cache=lambda a: a["k_cache"][0]), "k_cache must have shape"),
    (dict(k_cache=lambda a: strided(a["k_cache"])),
     "k_cache must be contiguous"),
    (dict(v_cache=lambda a: rnd(2, 1, 1, 128)), "v_cache must have shape"),
    (dict(v_cache=lambda a: a["v_cache"].to(FP8)),
     "v_cache must be BFloat16"),
    (dict(v_cache=lambda a: a["v_cache"].cpu()), "v_cache must be on a GPU"),
    (dict(k_cache=lambda a: rnd(1, 1, 0, 128),
          v_cache=lambda a: rnd(1, 1, 0, 128)), "block size"),       # BS
    # 12 query heads over 8 KV heads; then 3 over 1
    (dict(q=lambda a: rnd(1, 12, 128), k_cache=lambda a: rnd(1, 8, 1, 128),
          v_cache=lambda a: rnd(1, 8, 1, 128)), "q heads"),
    (dict(q=lambda a: rnd(1, 3, 128)), "q heads"),
    (dict(block_tables=lambda a: zeros(1, 1, dtype=I64)),
     "block_tables must be Int"),
    (dict(block_tables=lambda a: zeros(1)), "block_tables must have shape"),
    (dict(block_tables=lambda a: zeros(1, 0)), "max_blocks"),
    (dict(block_tables=lambda a: zeros(1, 1).cpu()),
     "block_tables must be on a GPU"),
    (dict(k_scale=lambda a: torch.ones(1, device=DEV)), "fp8"),
]

DECODE_RULES = [
    (dict(seq_lens=lambda a: zeros(1, dtype=I64)), "seq_lens must be Int"),
    (dict(seq_lens=lambda a: zeros(2)), "seq_lens must have shape"),
    (dict(seq_lens=lambda a: zeros(1).cpu()), "seq_lens must be on a GPU"),
    (dict(q=lambda a: rnd(2, 1, 128)), "one row per sequence"),       # B != N
    (dict(block_tables=lambda a: zeros(2, 1)), "one row per sequence"),
    (dict(chunk=128), "chunk must be 256 or 512"),
    (dict(chunk=0), "chunk must be 256 or 512"),
]

RULES = (
    [(op, r, m) for op in ("paged_attention", "paged_attention_split",
                           "flash_prefill") for r, m in ATTN_RULES] +
    [(op, r, m) for op in ("paged_attention", "paged_attention_split")
     for r, m in DECODE_RULES] + [
        ("paged_attention_split", dict(n_parts=0), "n_parts"),
        ("paged_attention_split", dict(n_parts=65), "n_parts"),
        ("paged_attention_split", dict(part_tokens=0), "part_tokens"),
        ("paged_attention_split", dict(part_tokens=1 << 31), "part_tokens"),

        ("flash_prefill", dict(seq_meta=lambda a: zeros(1, 3, dtype=I64)),
         "seq_meta must be Int"),
        ("flash_prefill", dict(seq_meta=lambda a: zeros(1, 2)),
         "seq_meta must have shape"),
        ("flash_prefill", dict(seq_meta=lambda a: zeros(2, 3)),
         "seq_meta must have shape"),
        ("flash_prefill", dict(seq_meta=lambda a: zeros(3)),
         "seq_meta must have shape"),
        ("flash_prefill", dict(tiles=lambda a: zeros(1, 2, dtype=I64)),
         "tiles must be Int"),
        ("flash_prefill", dict(tiles=lambda a: zeros(1, 3)),
         "tiles must have shape"),
        ("flash_prefill", dict(tiles=lambda a: zeros(2)),
         "tiles must have shape"),

        ("rmsnorm", dict(x=lambda a: a["x"].float(), residual=None),
         "x must be BFloat16"),
        ("rmsnorm", dict(x=lambda a: strided(a["x"]), residual=None),
         "x must be contiguous"),
        ("rmsnorm", dict(x=lambda a: rnd(1, 12), w=lambda a: rnd(12),
                         residual=None), "multiple of 8"),
        ("rmsnorm", dict(x=lambda a: rnd(1, 0), w=lambda a: rnd(0),
                         residual=None), r"x.size\(-1\) must be in"),
        ("rmsnorm", dict(w=lambda a: rnd(16)), "w must have shape"),
        ("rmsnorm", dict(w=lambda a: rnd(1, 8)), "w must have shape"),
        ("rmsnorm", dict(w=lambda a: a["w"].float()), "w must be BFloat16"),
        ("rmsnorm", dict(w=lambda a: a["w"].cpu()), "w must be on a GPU"),
        ("rmsnorm", dict(residual=lambda a: rnd(2, 8)),
         "residual must have shape"),
        ("rmsnorm", dict(residual=lambda a: rnd(8)),
         "residual must have shape"),
        ("rmsnorm", dict(residual=lambda a: a["residual"].float()),
         "residual must be BFloat16"),
        ("rmsnorm", dict(residual=lambda a: a["residual"].cpu()),
         "residual must be on a GPU"),

        ("rope", dict(q=lambda a: a["q"].float()), "q must be BFloat16"),
        ("rope", dict(q=lambda a: a["q"][0]), "q must have shape"),
        ("rope", dict(k=lambda a: a["k"].float()), "k must be BFloat16"),
        ("rope", dict(q=lambda a: rnd(1, 1, 3), k=lambda a: rnd(1, 1, 3),
                      cos_sin=lambda a: rnd(4, 1, 2, dtype=F32)), "even"),
        ("rope", dict(q=lambda a: rnd(1, 1, 0), k=lambda a: rnd(1, 1, 0),
                      cos_sin=lambda a: rnd(4, 0, 2, dtype=F32)), "head dim"),
        ("rope", dict(q=lambda a: rnd(1, 1, 2050), k=lambda a: rnd(1, 1, 2050),
                      cos_sin=lambda a: rnd(4, 1025, 2, dtype=F32)),
         "head dim"),
        ("rope", dict(k=lambda a: rnd(1, 1, 4)), "k must have shape"),   # D
        ("rope", dict(k=lambda a: rnd(2, 1, 2)), "k must have shape"),   # T
        ("rope", dict(cos_sin=lambda a: a["cos_sin"].to(BF16)),
         "cos_sin must be Float,"),
        ("rope", dict(cos_sin=lambda a: rnd(4, 2, 2, dtype=F32)),
         "cos_sin must have shape"),
        ("rope", dict(cos_sin=lambda a: rnd(4, 2, dtype=F32)),
         "cos_sin must have shape"),
        ("rope", dict(positions=lambda a: zeros(1, dtype=I64)),
         "positions must be Int"),
        ("rope", dict(positions=lambda a: zeros(2)),
         "positions must have shape"),
        ("rope", dict(positions=lambda a: zeros(1).cpu()),
         "positions must be on a GPU"),

        ("silu_mul", dict(gate_up=lambda a: a["gate_up"].float()),
         "gate_up must be BFloat16"),
        ("silu_mul", dict(gate_up=lambda a: rnd(1, 24)), "multiple"),   # I=12
        ("silu_mul", dict(gate_up=lambda a: rnd(1, 8)), "multiple"),    # I=4
        ("silu_mul", dict(gate_up=lambda a: rnd(1, 0)), "gate_up.size"),
        ("silu_mul", dict(gate_up=lambda a: strided(a["gate_up"])),
         "contiguous"),

        ("reshape_and_cache", dict(k_new=lambda a: a["k_new"].float()),
         "k_new must be BFloat16"),
        ("reshape_and_cache", dict(k_new=lambda a: a["k_new"][0]),
         "k_new must have shape"),
        ("reshape_and_cache", dict(v_new=lambda a: a["v_new"].float()),
         "v_new must be BFloat16"),
        ("reshape_and_cache", dict(v_new=lambda a: rnd(2, 1, 8)),
         "v_new must have shape"),
        ("reshape_and_cache",
         dict(k_new=lambda a: rnd(1, 1, 4), v_new=lambda a: rnd(1, 1, 4),
              k_cache=lambda a: rnd(1, 1, 1, 4),
              v_cache=lambda a: rnd(1, 1, 1, 4)), "multiple of 8"),
        ("reshape_and_cache", dict(k_cache=lambda a: rnd(1, 2, 1, 8),
                                   v_cache=lambda a: rnd(1, 2, 1, 8)),
         "k_cache must have shape"),                                  # KVH
        ("reshape_and_cache", dict(k_cache=lambda a: rnd(1, 1, 1, 16),
                                   v_cache=lambda a: rnd(1, 1, 1, 16)),
         "k_cache must have shape"),                                  # D
        ("reshape_and_cache", dict(k_cache=lambda a: a["k_cache"].to(F16)),
         "bf16 or fp8"),
        ("reshape_and_cache", dict(v_cache=lambda a: rnd(2, 1, 1, 8)),
         "v_cache must have shape"),
        ("reshape_and_cache", dict(v_cache=lambda a: a["v_cache"].to(FP8)),
         "v_cache must be BFloat16"),
        ("reshape_and_cache", dict(k_cache=lambda a: rnd(1, 1, 0, 8),
                                   v_cache=lambda a: rnd(1, 1, 0, 8)),
         "block size"),
        ("reshape_and_cache", dict(slots=lambda a: zeros(1)),
         "slots must be Long"),
        ("reshape_and_cache", dict(slots=lambda a: zeros(2, dtype=I64)),
         "slots must have shape"),

        ("move_blocks", dict(pool=lambda a: a["pool"][0]),
         "pool must have shape"),
        ("move_blocks", dict(pool=lambda a: rnd(1, 3, 1, 1, 1, 8)),
         "pool must have shape"),
        ("move_blocks", dict(pool=lambda a: a["pool"].cpu()),
         "pool must be on a GPU"),
        ("move_blocks", dict(pool=lambda a: rnd(1, 2, 1, 1, 1, 4),
                             staging=lambda a: rnd(1, 1, 2, 1, 1, 4)),
         "multiple of 16"),
        ("move_blocks", dict(staging=lambda a: rnd(2, 1, 2, 1, 1, 8)),
         "staging must have shape"),                                  # n
        ("move_blocks", dict(staging=lambda a: rnd(1, 2, 1, 1, 1, 8)),
         "staging must have shape"),
        ("move_blocks", dict(staging=lambda a: rnd(1, 1, 2, 1, 1, 16)),
         "staging must have shape"),
        ("move_blocks", dict(staging=lambda a: rnd(1, 1, 2, 1, 1, 8,
                                                   dtype=F16)),
         "staging must be BFloat16"),
        ("move_blocks", dict(block_ids=lambda a: zeros(1, dtype=I64)),
         "block_ids must be Int"),
        ("move_blocks", dict(block_ids=lambda a: zeros(1, 1)),
         "block_ids must have shape"),
        ("move_blocks", dict(block_ids=lambda a: zeros(1).cpu()),
         "block_ids must be on a GPU"),

        ("copy_blocks_peer", dict(src_pool_ptr=0), "null"),
        ("copy_blocks_peer", dict(src_nb=0), "src_nb"),
        ("copy_blocks_peer", dict(dst_pool=lambda a: a["dst_pool"][0]),
         "dst_pool must have shape"),
        ("copy_blocks_peer", dict(dst_pool=lambda a: rnd(1, 3, 1, 1, 1, 8)),
         "dst_pool must have shape"),
        ("copy_blocks_peer", dict(dst_pool=lambda a: rnd(1, 2, 1, 1, 1, 4)),
         "multiple of 16"),
        ("copy_blocks_peer", dict(src_ids=lambda a: zeros(1, dtype=I64)),
         "src_ids must be Int"),
        ("copy_blocks_peer", dict(dst_ids=lambda a: zeros(1, dtype=I64)),
         "dst_ids must be Int"),
        ("copy_blocks_peer", dict(dst_ids=lambda a: zeros(2)),
         "equally long"),
        ("copy_blocks_peer", dict(src_ids=lambda a: zeros(1, 1)),
         "src_ids must have shape"),
    ])


@pytest.mark.parametrize(
    "rule", RULES, ids=[f"{i}-{op}-{'+'.join(repl)}"
                        for i, (op, repl, _) in enumerate(RULES)])
def test_rejects(ext, rule):
    """The call raises with the rule's message. The allocator's count of
    allocations did not move, so no output was allocated first, and no
    tensor argument changed, so nothing was launched."""
    op, repl, match = rule
    legal = LEGAL[op]()
    args = dict(legal)
    for name, new in repl.items():        # k_scale: positional, after the rest
        args[name] = new(legal) if callable(new) else new

    def n_allocations():
        return torch.cuda.memory_stats()["allocation.all.allocated"]

    def raw(t):
        return t.contiguous().view(torch.uint8)

    before = {k: raw(v).clone() for k, v in args.items()
              if isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    allocations = n_allocations()
    with pytest.raises(RuntimeError, match=match):
        call(ext, op, args)
    assert n_allocations() == allocations
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(raw(args[k]), v), k


# ---- the same smallest calls are accepted and equal ops.ref --------------

def cpu(args):
    return {k: v.cpu() if isinstance(v, torch.Tensor) else v
            for k, v in args.items()}


def one_bf16_step(got, want):
    """got and want are both bf16 roundings of fp32 results that agree to a
    few fp32 ulps (reduction order, fma contraction, rsqrt and exp
    approximations: all below 2^-20 relative, against a bf16 step of 2^-8),
    so they are equal or, where the two fp32 values straddle a rounding
    boundary, one bf16 step apart."""
    w = want.double()
    return bool(((got.double() - w).abs() <= kc.bf16_ulp(w)).all())


@pytest.mark.parametrize("op", ["paged_attention", "paged_attention_split",
                                "flash_prefill"])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_accepts_attention(ext, op, kv_dtype):
    """One token attends to itself: the softmax weight is exactly 1 and the
    output is the V row, in every kernel and in the reference."""
    from llm_d_inference_scheduler_amd.ops import ref
    a = LEGAL[op]()
    if kv_dtype == "fp8":
        a["k_cache"], a["v_cache"] = a["k_cache"].to(FP8), a["v_cache"].to(FP8)
    out = call(ext, op, a)
    c = cpu(a)
    want = ref.paged_attention(c["q"], c["k_cache"], c["v_cache"],
                               c["block_tables"],
                               torch.ones(1, dtype=I32), c["scale"])
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out.cpu()[0], c["v_cache"][0, :, 0].float().to(BF16))


@pytest.mark.parametrize("with_residual", [False, True])
def test_accepts_rmsnorm(ext, with_residual):
    from llm_d_inference_scheduler_amd.ops import ref
    a = legal_rmsnorm()
    if not with_residual:
        a["residual"] = None
    c = cpu(a)
    if with_residual:
        c["residual"] = c["residual"].clone()
    y = ext.rmsnorm(*a.values())
    want = ref.rmsnorm(*c.values())
    assert one_bf16_step(y.cpu(), want)
    if with_residual:
        # bf16(x + r): one rounded fp32 add on both sides
        assert torch.equal(a["residual"].cpu(), c["residual"])


def test_accepts_rope(ext):
    from llm_d_inference_scheduler_amd.ops import ref
    a = legal_rope()
    c = {k: v.clone() for k, v in cpu(a).items()}
    ext.rope(*a.values())
    ref.rope(*c.values())
    assert one_bf16_step(a["q"].cpu(), c["q"])
    assert one_bf16_step(a["k"].cpu(), c["k"])
    assert not torch.equal(a["q"].cpu(), cpu(legal_rope())["q"])  # it ran


def test_accepts_silu_mul(ext):
    from llm_d_inference_scheduler_amd.ops import ref
    a = legal_silu_mul()
    y = ext.silu_mul(*a.values())
    assert y.shape == (1, 8)
    assert one_bf16_step(y.cpu(), ref.silu_mul(a["gate_up"].cpu()))


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_accepts_reshape_and_cache(ext, kv_dtype):
    from llm_d_inference_scheduler_amd.ops import ref
    a = legal_reshape_and_cache()
    if kv_dtype == "fp8":
        a["k_cache"], a["v_cache"] = a["k_cache"].to(FP8), a["v_cache"].to(FP8)
    c = {k: v.clone() for k, v in cpu(a).items()}
    ext.reshape_and_cache(*a.values())
    ref.reshape_and_cache(*c.values())
    for name in ("k_cache", "v_cache"):
        assert torch.equal(a[name].cpu().view(torch.uint8),
                           c[name].view(torch.uint8))
    want = c["k_new"] if kv_dtype == "bf16" else c["k_new"].to(FP8)
    assert torch.equal(a["k_cache"].cpu()[0, :, 0].view(torch.uint8),
                       want[0].view(torch.uint8))


def test_accepts_smallest_movers(ext):
    a = legal_move_blocks()
    ext.move_blocks(*a.values())
    assert torch.equal(a["staging"][0], a["pool"][:, :, 0])
    p = legal_copy_blocks_peer()
    call(ext, "copy_blocks_peer", p)
    torch.cuda.synchronize()
    assert torch.equal(p["dst_pool"], p["_keep"])


# ---- the merged mover: gather, scatter, peer -----------------------------

@pytest.mark.parametrize("kv_dtype,d", [("bf16", 8), ("fp8", 16)])
def test_mover_three_directions(ext, kv_dtype, d):
    """Pool [L=2, 2, NB=3, KVH=1, BS=1, D]: one block is exactly one 16-byte
    unit, so an off-by-one in the unit index moves a whole wrong block. The
    id lists are permutations without a fixed point and differ between
    source and destination. The peer copy runs against this process's own
    pool pointer."""
    g = torch.Generator().manual_seed(31)
    L, NB = 2, 3
    size = 2 if kv_dtype == "bf16" else 1
    typed = BF16 if kv_dtype == "bf16" else FP8

    def pool_bytes(*shape):
        return torch.randint(0, 256, (*shape, d * size), generator=g,
                             dtype=torch.uint8)

    src_b, dst_b = pool_bytes(L, 2, NB, 1, 1), pool_bytes(L, 2, NB, 1, 1)
    assert src_b[0, 0, 0].numel() == 16
    src_ids = torch.tensor([2, 0, 1], dtype=I32)
    dst_ids = torch.tensor([1, 2, 0], dtype=I32)
    src = src_b.view(typed).to(DEV)
    # gather <by id, identity>
    staging = pool_bytes(NB, L, 2, 1, 1).view(typed).to(DEV)
    ext.move_blocks(src, staging, src_ids.to(DEV), False)
    want_staging = src_b[:, :, src_ids.long()].permute(2, 0, 1, 3, 4, 5)
    assert torch.equal(staging.cpu().view(torch.uint8), want_staging)
    assert torch.equal(src.cpu().view(torch.uint8), src_b)
    # scatter <identity, by id>
    want = dst_b.clone()
    want[:, :, dst_ids.long()] = src_b[:, :, src_ids.long()]
    dst = dst_b.view(typed).to(DEV)
    ext.move_blocks(dst, staging, dst_ids.to(DEV), True)
    assert torch.equal(dst.cpu().view(torch.uint8), want)
    # peer <by id, by id>
    dst2 = dst_b.view(typed).to(DEV)
    ext.copy_blocks_peer(src.data_ptr(), dst2, src_ids.to(DEV),
                         dst_ids.to(DEV), NB)
    torch.cuda.synchronize()
    assert torch.equal(dst2.cpu().view(torch.uint8), want)
    assert torch.equal(src.cpu().view(torch.uint8), src_b)
