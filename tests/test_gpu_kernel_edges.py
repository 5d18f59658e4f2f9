"""GPU tier of the kernel edge tests: every HIP kernel against a float64
reference at the shapes where its code takes another path, with needle
queries over a poisoned KV pool and a per-row relative error limit derived
from a rounding emulation (tests/kernel_cases.py; DEVELOPMENT.md "Kernel
edge tests"). tests/test_kernel_cases.py proves on the CPU that these inputs
and this metric notice a skipped tile, a lost token or partition, a mask off
by one or a wrong block-table entry.

Each attention test prints one `EDGE|kernel|case|limit|worst` line before it
asserts (pytest -s shows them)."""
import functools

import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def judge(kernel, name, out, case):
    """Every row of the case against float64, under the case's limit."""
    limit, _ = case.limit()
    worst = float(kc.row_rel_err(out.cpu(), case.reference()).max())
    print(f"EDGE|{kernel}|{name}|{limit:.3e}|{worst:.3e}")
    assert worst <= limit, (kernel, name, worst, limit)


# ---- flash prefill -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def prefill_case(qpg, kv_dtype="bf16"):
    return kc.make_prefill_case(qpg, kv_dtype=kv_dtype)


def run_flash(ext, case, width=None):
    bt = case.block_tables if width is None else case.widened(width)
    i32 = dict(dtype=torch.int32, device="cuda")
    return ext.flash_prefill(
        case.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(), bt.cuda(),
        torch.tensor(case.metas, **i32), torch.tensor(case.tiles, **i32),
        case.scale).cpu()


@pytest.mark.parametrize("qpg", [1, 2, 4, 8])
def test_flash_prefill_glds(ext, qpg):
    """bf16 KV, block table <= 1024 columns: the glds ring kernel. One
    launch holds a one-token chunk after a 300-token prior, chunk*QPG < 32
    (waves 1-3 idle), ctx of exactly 1, 2 and 3 KV tiles, a block-aligned
    ctx and two long chunked continuations; table widths differ."""
    case = prefill_case(qpg)
    judge("flash_prefill_glds", f"qpg{qpg}", run_flash(ext, case), case)


@pytest.mark.parametrize("qpg", [1, 2, 4, 8])
def test_flash_prefill_plain_bf16(ext, qpg):
    """A block table wider than 1024 columns (a context beyond 16K tokens
    in production) routes bf16 KV to the plain kernel. The padding columns
    point at the poisoned block 0. Plain and glds run one tile body
    (flash_tile.h) over the same sequence of 32-token sub-tiles, so on
    bf16 KV their outputs are equal bit for bit."""
    case = prefill_case(qpg)
    plain = run_flash(ext, case, width=1025)
    judge("flash_prefill_plain_bf16", f"qpg{qpg}", plain, case)
    glds = run_flash(ext, case)
    limit, _ = case.limit()
    agree = float(kc.row_rel_err(plain, glds.double()).max())
    print(f"EDGE|flash_prefill plain vs glds|qpg{qpg}|{limit:.3e}|{agree:.3e}")
    assert agree <= limit
    assert torch.equal(plain, glds)


@pytest.mark.parametrize("qpg", [2, 4])
def test_flash_prefill_fp8(ext, qpg):
    """fp8 KV (convert-on-stage plain kernel) against float64 on the
    dequantised values; poison is 448."""
    case = prefill_case(qpg, "fp8")
    judge("flash_prefill_fp8", f"qpg{qpg}", run_flash(ext, case), case)


# ---- paged decode --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def decode_case(qpg, kv_dtype):
    return kc.make_decode_case(qpg, kc.DECODE_SEQS, kv_dtype=kv_dtype)


@functools.lru_cache(maxsize=None)
def split_case(qpg, kv_dtype, np_, part):
    return kc.make_decode_case(qpg, kc.split_seqs(np_, part),
                               part_tokens=part, kv_dtype=kv_dtype)


def decode_args(case):
    return (case.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(),
            case.block_tables.cuda(),
            torch.tensor(case.seq_lens, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("qpg", [1, 2, 4, 8])
@pytest.mark.parametrize("chunk", [256, 512])
def test_paged_attention(ext, chunk, qpg, kv_dtype):
    """Single-pass decode at both online-softmax chunk sizes; lengths sit
    on both sides of the block, wave, chunk and 2-chunk boundaries."""
    case = decode_case(qpg, kv_dtype)
    out = ext.paged_attention(*decode_args(case), case.scale, chunk).cpu()
    assert case.seq_lens[0] == 0
    assert bool((out[0].float() == 0).all())       # l == 0 -> exact zeros
    judge("paged_attention", f"chunk{chunk} qpg{qpg} {kv_dtype}", out, case)


@pytest.mark.parametrize("np_,part,chunk,qpg,kv_dtype", [
    (4, 512, 256, 4, "bf16"), (9, 256, 256, 4, "bf16"),
    (3, 768, 256, 4, "bf16"), (3, 1024, 512, 4, "bf16"),
    (4, 512, 256, 1, "bf16"), (9, 256, 256, 2, "bf16"),
    (3, 768, 256, 8, "bf16"), (3, 1024, 512, 2, "fp8"),
    (9, 256, 256, 4, "fp8")])
def test_paged_attention_split(ext, np_, part, chunk, qpg, kv_dtype):
    """Partitioned decode + combine against float64: a one-token last
    partition (k*part + 1), rows of one token next to rows filling every
    partition, empty partitions in between."""
    case = split_case(qpg, kv_dtype, np_, part)
    out = ext.paged_attention_split(*decode_args(case), np_, part,
                                    case.scale, chunk).cpu()
    judge("paged_attention_split",
          f"np{np_} part{part} chunk{chunk} qpg{qpg} {kv_dtype}", out, case)


@pytest.mark.parametrize("seq_lens,max_seq_len", [([2049], 2049),
                                                  ([4096, 1, 513], 4096)])
def test_paged_attention_dispatch_geometry(ext, seq_lens, max_seq_len):
    """The partition geometry ops.dispatch.paged_attention derives from
    max_seq_len, and the split kernel run through it."""
    from llm_d_inference_scheduler_amd.ops import dispatch
    kvh, qpg = 2, 4
    geom = dispatch.split_geometry(len(seq_lens) * kvh, max_seq_len)
    assert geom is not None
    np_, part = geom
    assert np_ * part >= max_seq_len
    assert np_ <= 64
    assert part % dispatch._ATTN_CHUNK == 0
    case = kc.make_decode_case(qpg, seq_lens, part_tokens=part, kvh=kvh,
                               diffuse_extra=False)
    out = dispatch.paged_attention(*decode_args(case), case.scale,
                                   max_seq_len=max_seq_len).cpu()
    judge("dispatch.paged_attention", f"B{len(seq_lens)} max{max_seq_len} "
          f"-> np{np_} part{part}", out, case)


# ---- rmsnorm -------------------------------------------------------------

@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("rows,H", [(1000, 128), (37, 2056), (6, 16384 + 8)])
def test_rmsnorm(ext, rows, H, with_residual):
    """H=128: 16 chunks for 256 threads (the QK-norm shape); H=2056: 257
    chunks, one thread takes a second; H=16392: one chunk past the register
    cache, re-read from x or from the updated residual. The float64
    reference uses the unrounded x + r below element 16384 and the bf16
    value written back to the residual from there on (kc.rmsnorm_ref64), so
    the limit is the bf16 output rounding step alone."""
    g = torch.Generator().manual_seed(H + with_residual)
    x = torch.randn(rows, H, generator=g).bfloat16()
    w = torch.randn(H, generator=g).bfloat16()
    r = torch.randn(rows, H, generator=g).bfloat16() if with_residual else None
    r_hip = r.cuda() if with_residual else None
    y = ext.rmsnorm(x.cuda(), w.cuda(), 1e-5, r_hip).cpu()
    y64, r_new = kc.rmsnorm_ref64(x, w, 1e-5, r)
    if with_residual:
        assert torch.equal(r_hip.cpu(), r_new)     # bf16(x + r), bit-exact
    worst = float(kc.row_rel_err(y, y64).max())
    print(f"EDGE|rmsnorm|{rows}x{H} res={with_residual}|{kc.FLOOR:.3e}|"
          f"{worst:.3e}")
    assert worst <= kc.FLOOR


# ---- rope ----------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 128])
def test_rope(ext, d):
    """D=64: half the 64-thread block exits early. Positions include 0 and
    the last table row. No reduction is involved, so every element must
    equal the fp32 rotation rounded to bf16. The compiler contracts
    x1*c - x2*s into fma(x1, c, -(x2*s)) (v_fma_f32 in the gfx950 code), so
    an element may equal either the contracted or the uncontracted fp32
    evaluation, and is within one bf16 step of float64 in both."""
    from llm_d_inference_scheduler_amd.ops import ref
    g = torch.Generator().manual_seed(d)
    T, QH, KVH, max_pos = 37, 6, 2, 4096
    q = torch.randn(T, QH, d, generator=g).bfloat16()
    k = torch.randn(T, KVH, d, generator=g).bfloat16()
    table = ref.rope_table(max_pos, d, 500000.0)
    pos = torch.randint(0, max_pos, (T,), generator=g, dtype=torch.int32)
    pos[0], pos[1], pos[-1] = 0, max_pos - 1, max_pos - 1
    q_hip, k_hip = q.cuda(), k.cuda()
    ext.rope(q_hip, k_hip, table.cuda(), pos.cuda())
    for got, src in ((q_hip.cpu(), q), (k_hip.cpu(), k)):
        plain = got == kc.rope_ref32(src, table, pos)
        fused = got == kc.rope_ref32(src, table, pos, fused=True)
        want64 = kc.rope_ref64(src, table, pos)
        print(f"EDGE|rope|D{d} {tuple(src.shape)}|equal|"
              f"{int((~plain).sum())} differ from plain fp32, "
              f"{int((~fused).sum())} from contracted, "
              f"{int((~(plain | fused)).sum())} from both")
        assert bool((plain | fused).all())
        assert bool(((got.double() - want64).abs()
                     <= kc.bf16_ulp(want64)).all())
    # position 0 is the identity
    assert torch.equal(q_hip.cpu()[0], q[0])


# ---- silu_mul ------------------------------------------------------------

def test_silu_mul_grid_stride_and_saturation(ext):
    """T*(I/8) = 257*2048 chunks > 2048 blocks * 256 threads + 3, so the
    grid-stride loop takes a second pass (all of the last row). Gates of
    +-{0, 1e-3, 20, 88, 100, 3e4} sit in the first and in the last row:
    __expf(-g) overflows to inf for g <= -89 and must give 0, not NaN."""
    T, inter = 257, 16384
    assert T * (inter // 8) > 2048 * 256 + 3
    g = torch.Generator().manual_seed(8)
    gu = torch.randn(T, 2 * inter, generator=g)
    gates = torch.tensor([0.0, 1e-3, 20.0, 88.0, 100.0, 3e4])
    gates = torch.cat([gates, -gates])
    for row in (0, T - 1):
        gu[row, :inter] = gates.repeat(inter // len(gates) + 1)[:inter]
    gu = gu.bfloat16()
    y = ext.silu_mul(gu.cuda()).cpu()
    assert bool(torch.isfinite(y.float()).all())
    want = kc.silu_mul_ref64(gu)
    ulps = (y.double() - want).abs() / kc.bf16_ulp(want)
    print(f"EDGE|silu_mul|{T}x{inter}|2 ulp|{float(ulps.max()):.3f} ulp")
    assert float(ulps.max()) <= 2.0


# ---- KV pool maintenance -------------------------------------------------

def raw(t):
    """Bit pattern of a bf16 / fp8 tensor."""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.uint8)


@pytest.mark.parametrize("kvh", [32, 2])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_reshape_and_cache_whole_cache(ext, kv_dtype, kvh):
    """KVH=32: 512 chunks for 256 threads, the in-block loop iterates.
    Slots hold -1 (padding, no write), 0 and the last slot; the whole cache
    must equal the expected one, so every other row is proven untouched."""
    g = torch.Generator().manual_seed(kvh)
    T, NB = 40, 6
    spread = 40.0 if kv_dtype == "fp8" else 1.0
    k = (torch.randn(T, kvh, kc.D, generator=g) * spread).clamp(
        -kc.FP8_MAX, kc.FP8_MAX).bfloat16()
    v = (torch.randn(T, kvh, kc.D, generator=g) * spread).clamp(
        -kc.FP8_MAX, kc.FP8_MAX).bfloat16()
    k_cache = kc.to_cache(torch.randn(NB, kvh, kc.BS, kc.D, generator=g) * 3,
                          kv_dtype)
    v_cache = kc.to_cache(torch.randn(NB, kvh, kc.BS, kc.D, generator=g) * 3,
                          kv_dtype)
    slots = torch.randperm(NB * kc.BS - 2, generator=g)[:T] + 1
    slots[3], slots[17] = 0, NB * kc.BS - 1
    slots[[0, 9, 10, T - 1]] = -1
    want_k, want_v = raw(k_cache).clone(), raw(v_cache).clone()
    new_k = raw(kc.to_cache(k.float(), kv_dtype))
    new_v = raw(kc.to_cache(v.float(), kv_dtype))
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            want_k[s // kc.BS, :, s % kc.BS] = new_k[t]
            want_v[s // kc.BS, :, s % kc.BS] = new_v[t]
    k_hip, v_hip = k_cache.cuda(), v_cache.cuda()
    ext.reshape_and_cache(k.cuda(), v.cuda(), k_hip, v_hip, slots.cuda())
    assert torch.equal(raw(k_hip.cpu()), want_k)
    assert torch.equal(raw(v_hip.cpu()), want_v)


def random_pool(g, shape, kv_dtype):
    """A pool of random bits, as bytes [..., D * itemsize] and typed."""
    size = 2 if kv_dtype == "bf16" else 1
    b = torch.randint(0, 256, (*shape[:-1], shape[-1] * size), generator=g,
                      dtype=torch.uint8)
    return b, b.view(torch.bfloat16 if kv_dtype == "bf16" else kc.FP8)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_move_blocks_whole_pool(ext, kv_dtype):
    """Gather then scatter with ids that include block 0 and the last
    block: the staging buffer equals the gathered reference and the whole
    destination pool equals the expected pool, unselected blocks included."""
    g = torch.Generator().manual_seed(21)
    L, NB, KVH = 2, 12, 2
    ids = torch.tensor([0, NB - 1, 5, 3], dtype=torch.int32)
    src_b, src = random_pool(g, (L, 2, NB, KVH, kc.BS, kc.D), kv_dtype)
    dst_b, dst = random_pool(g, (L, 2, NB, KVH, kc.BS, kc.D), kv_dtype)
    _, staging = random_pool(g, (len(ids), L, 2, KVH, kc.BS, kc.D), kv_dtype)
    src_hip, dst_hip, staging_hip = src.cuda(), dst.cuda(), staging.cuda()
    ext.move_blocks(src_hip, staging_hip, ids.cuda(), False)
    want_staging = src_b[:, :, ids.long()].permute(2, 0, 1, 3, 4, 5)
    assert torch.equal(staging_hip.cpu().view(torch.uint8), want_staging)
    assert torch.equal(src_hip.cpu().view(torch.uint8), src_b)
    ext.move_blocks(dst_hip, staging_hip, ids.cuda(), True)
    want = dst_b.clone()
    want[:, :, ids.long()] = src_b[:, :, ids.long()]
    assert torch.equal(dst_hip.cpu().view(torch.uint8), want)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_copy_blocks_peer_whole_pool(ext, kv_dtype):
    g = torch.Generator().manual_seed(22)
    L, KVH, src_nb, dst_nb = 2, 2, 12, 9
    src_ids = torch.tensor([0, src_nb - 1, 4], dtype=torch.int32)
    dst_ids = torch.tensor([dst_nb - 1, 0, 3], dtype=torch.int32)
    src_b, src = random_pool(g, (L, 2, src_nb, KVH, kc.BS, kc.D), kv_dtype)
    dst_b, dst = random_pool(g, (L, 2, dst_nb, KVH, kc.BS, kc.D), kv_dtype)
    src_hip, dst_hip = src.cuda(), dst.cuda()
    ext.copy_blocks_peer(src_hip.data_ptr(), dst_hip, src_ids.cuda(),
                         dst_ids.cuda(), src_nb)
    torch.cuda.synchronize()
    want = dst_b.clone()
    want[:, :, dst_ids.long()] = src_b[:, :, src_ids.long()]
    assert torch.equal(dst_hip.cpu().view(torch.uint8), want)
    assert torch.equal(src_hip.cpu().view(torch.uint8), src_b)
