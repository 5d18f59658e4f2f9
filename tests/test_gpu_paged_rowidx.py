"""GPU: decode attention with the per-chunk pool-row table (Phase A writes
each token's pool row to LDS, Phase C forms the V address from it) against
ops.ref.paged_attention, at the tolerance of tests/test_gpu_kernels.py.
Lengths sit on both sides of every boundary the table has: one row, a block
(bs), a chunk (256 or 512 tokens), the 8-row V batch and the 64 tokens a
wave owns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KVH, D = 2, 128
ATOL = RTOL = 3e-2          # test_gpu_kernels.py::test_paged_attention


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def to_f32(t):
    return t.float().cpu()


def make_case(seqs, qpg, bs, fp8, seed):
    """Random q and pool; every sequence's blocks drawn from one shuffled
    permutation of the pool, so tables are non-monotonic and interleaved.
    Block 0 is never used and table entries past a sequence's end point at
    it."""
    g = torch.Generator().manual_seed(seed)
    B = len(seqs)
    max_blocks = (max(seqs) + bs - 1) // bs
    need = sum((s + bs - 1) // bs for s in seqs)
    NB = need + 3
    q = torch.randn(B, KVH * qpg, D, generator=g).bfloat16().cuda()
    kc = torch.randn(NB, KVH, bs, D, generator=g)
    vc = torch.randn(NB, KVH, bs, D, generator=g)
    dtype = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc, vc = kc.to(dtype).cuda(), vc.to(dtype).cuda()
    perm = torch.randperm(NB - 1, generator=g) + 1
    bt = torch.zeros(B, max_blocks, dtype=torch.int32)
    k = 0
    for b, s in enumerate(seqs):
        nb = (s + bs - 1) // bs
        bt[b, :nb] = perm[k:k + nb]
        k += nb
    longest = bt[seqs.index(max(seqs)), :(max(seqs) + bs - 1) // bs]
    assert len(longest) < 3 or (longest[:-1] > longest[1:]).any()
    sl =torch.tensor(seqs, dtype=torch.int32)
    return q, kc, vc, bt, sl


def reference(q, kc, vc, bt, sl, k_scale=None, v_scale=None):
    from llm_d_inference_scheduler_amd.ops import ref
    return ref.paged_attention(
        to_f32(q), to_f32(kc), to_f32(vc), bt, sl, D ** -0.5,
        k_scale=None if k_scale is None else k_scale.cpu(),
        v_scale=None if v_scale is None else v_scale.cpu())


def close(out, want):
    diff = (to_f32(out) - want).abs().max()
    assert torch.allclose(to_f32(out), want, atol=ATOL, rtol=RTOL), diff


def lengths(bs, chunk):
    return [1, bs - 1, bs, bs + 1, chunk - 1, chunk, chunk + 1,
            2 * chunk + 17]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("qpg", [1, 4, 8])
def test_boundary_lengths(ext, qpg, fp8):
    """The eight lengths in two launches of B = 4."""
    bs, chunk = 16, 256
    seqs = lengths(bs, chunk)
    for part, seed in ((seqs[0::2], 1), (seqs[1::2], 2)):
        q, kc, vc, bt, sl = make_case(part, qpg, bs, fp8, seed + 10 * qpg)
        out = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(), D ** -0.5)
        close(out, reference(q, kc, vc, bt, sl))


def test_chunk_512(ext):
    """The table is CHUNK entries long: the 512-token chunk has its own
    boundaries, and a wave then owns 128 tokens of it."""
    bs, chunk = 16, 512
    seqs = lengths(bs, chunk)
    for part, seed in ((seqs[0::2], 3), (seqs[1::2], 4)):
        q, kc, vc, bt, sl = make_case(part, 4, bs, False, seed)
        out = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(), D ** -0.5,
                                  chunk)
        close(out, reference(q, kc, vc, bt, sl))


def test_block_size_32(ext):
    bs = 32
    seqs = [bs - 1, bs + 1, 256 + 1, 2 * 256 + 17]
    q, kc, vc, bt, sl = make_case(seqs, 4, bs, False, 5)
    out = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(), D ** -0.5)
    close(out, reference(q, kc, vc, bt, sl))


def test_fp8_scaled(ext):
    seqs = [15, 257, 529]
    q, kc, vc, bt, sl = make_case(seqs, 4, 16, True, 6)
    ks = torch.tensor([0.5, 1.25], device="cuda")
    vs = torch.tensor([2.0, 0.75], device="cuda")
    out = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(), D ** -0.5,
                              256, ks, vs)
    close(out, reference(q, kc, vc, bt, sl, ks, vs))


def test_split_three_partitions_last_partial(ext):
    """Partitions of 256 tokens over 529: 256 + 256 + 17; the shorter
    sequences leave partitions partial or empty."""
    seqs = [529, 300, 16]
    q, kc, vc, bt, sl = make_case(seqs, 4, 16, False, 7)
    out = ext.paged_attention_split(q, kc, vc, bt.cuda(), sl.cuda(), 3, 256,
                                    D ** -0.5)
    close(out, reference(q, kc, vc, bt, sl))


def test_pool_rows_must_fit_int32(ext):
    """The row table is int32: a pool of 2^31 rows is refused by both decode
    bindings on its sizes alone (a meta tensor stands in for the 256 GiB),
    one row less passes that check."""
    q = torch.zeros(1, KVH * 4, D, dtype=torch.bfloat16, device="cuda")
    bt = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    sl = torch.ones(1, dtype=torch.int32, device="cuda")
    big = torch.empty((1 << 26, KVH, 16, D), dtype=torch.float8_e4m3fn,
                      device="meta")
    assert big.shape[0] * big.shape[1] * big.shape[2] == 1 << 31
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        ext.paged_attention(q, big, big, bt, sl, D ** -0.5)
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        ext.paged_attention_split(q, big, big, bt, sl, 2, 256, D ** -0.5)
    fits = torch.empty(((1 << 26) - 1, KVH, 16, D),
                       dtype=torch.float8_e4m3fn, device="meta")
    with pytest.raises(RuntimeError) as err:       # refused for the device
        ext.paged_attention(q, fits, fits, bt, sl, D ** -0.5)
    assert "2^31" not in str(err.value) and "GPU" in str(err.value)
