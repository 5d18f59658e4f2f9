"""CPU tier of the kernel edge tests: proves, without a GPU, that the needle
inputs and the row-relative metric of tests/kernel_cases.py notice the bugs
the GPU tier (tests/test_gpu_kernel_edges.py) is there to catch. Mutants of
the float64 reference run through the same metric and limit as the kernels;
the rounding emulation and the project's fp32 ops.ref must stay inside it."""
import functools
import math

import pytest
import torch

import kernel_cases as kc
from llm_d_inference_scheduler_amd.ops import ref
from llm_d_inference_scheduler_amd.ops.dispatch import split_geometry

QPG = 4


@functools.lru_cache(maxsize=None)
def prefill_case(kv_dtype="bf16"):
    return kc.make_prefill_case(QPG, kv_dtype=kv_dtype)


@functools.lru_cache(maxsize=None)
def decode_case():
    return kc.make_decode_case(QPG, kc.DECODE_SEQS)


@functools.lru_cache(maxsize=None)
def split_case(np_=4, part=512):
    return kc.make_decode_case(QPG, kc.split_seqs(np_, part),
                               part_tokens=part)


def worst(out, case):
    return float(kc.row_rel_err(out, case.reference()).max())


# ---- the inputs ----------------------------------------------------------

@pytest.mark.parametrize("qpg", [1, 2, 4, 8])
def test_prefill_case_coverage(qpg):
    case = prefill_case() if qpg == QPG else kc.make_prefill_case(qpg)
    # only the one-token chunk lacks the rows to reach each of its 10 tiles
    assert set(case.uncovered) <= {(1, 300)}
    all_t = set()
    for (start, chunk, prior), tgt in zip(case.metas, case.targets):
        own = prior + torch.arange(chunk).view(-1, 1)
        needles = tgt >= 0
        if chunk >= 4:
            assert bool((tgt == own)[needles].any())
            assert bool((tgt == own - 1)[needles].any())
        # a quarter of the rows stays diffuse
        if chunk * qpg >= 32:
            assert abs(float((~needles).float().mean()) - 0.25) < 0.02
        all_t |= set(tgt[needles].tolist())
    assert 0 in all_t
    # block-table widths differ within the launch; unused columns -> block 0
    nbs = [(c + p + kc.BS - 1) // kc.BS for c, p in case.seqs]
    assert len(set(nbs)) > 1
    for i, nb in enumerate(nbs):
        assert bool((case.block_tables[i, nb:] == 0).all())
        assert bool((case.block_tables[i, :nb] > 0).all())


def test_needles_dominate():
    """A needle row's softmax puts nearly all weight on its target."""
    case = prefill_case()
    kcf = kc.cache_to_f64(case.k_cache)
    start, chunk, prior = case.metas[7]            # (600, 171)
    kk = kc.gather_tokens(kcf, case.block_tables[7], chunk + prior)
    q = case.q[start:start + chunk].double()
    p_idx, h_idx = torch.nonzero(case.targets[7] >= 0, as_tuple=True)
    logits = torch.einsum("nd,nsd->ns", q[p_idx, h_idx],
                          kk[h_idx // QPG]) * case.scale
    vis = torch.arange(chunk + prior).view(1, -1) <= (prior + p_idx).view(-1, 1)
    w = torch.softmax(logits.masked_fill(~vis, -math.inf), dim=-1)
    on_target = w[torch.arange(len(p_idx)), case.targets[7][p_idx, h_idx]]
    assert float(on_target.median()) > 0.999
    assert float(on_target.min()) > 0.5


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_pool_is_poisoned(kv_dtype):
    case = kc.make_decode_case(2, [1, 17, 40], kv_dtype=kv_dtype)
    k = case.k_cache.float()
    bad = torch.isnan(k) if kv_dtype == "bf16" else (k == kc.FP8_MAX)
    row_bad = bad.all(dim=-1).all(dim=1)           # [NB, BS]
    assert bool(row_bad[0].all())                  # block 0
    for b, S in enumerate(case.seq_lens):
        blocks = case.block_tables[b, :(S + kc.BS - 1) // kc.BS].long()
        flat = row_bad[blocks].reshape(-1)
        assert not bool(flat[:S].any()) and bool(flat[S:].all())
    used = set(case.block_tables.flatten().tolist())
    for blk in range(case.k_cache.shape[0]):
        if blk not in used:
            assert bool(row_bad[blk].all())
    # the reference never touches a poisoned row
    assert bool(torch.isfinite(case.reference()).all())


def test_metric_judges_every_row():
    ref64 = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    out = torch.tensor([[3.0, 4.5], [0.0, 0.0], [math.nan, 0.0]])
    err = kc.row_rel_err(out, ref64)
    assert err.tolist() == [0.1, 0.0, math.inf]
    assert kc.row_rel_err(torch.ones(1, 2), torch.zeros(1, 2)).tolist() == \
        [math.inf]
    # an all-zero output is 100 % wrong on every row, whatever the signal size
    case = decode_case()
    z = kc.row_rel_err(torch.zeros_like(case.reference()), case.reference())
    nonzero = case.reference().norm(dim=-1) > 0
    assert bool((z[nonzero] == 1.0).all())


# ---- limits, emulation, ops.ref ------------------------------------------

def test_limits_are_tight():
    for case in (prefill_case(), prefill_case("fp8"), decode_case(),
                 split_case()):
        limit, emul_worst = case.limit()
        assert kc.FLOOR <= limit < 0.03, limit
        assert emul_worst <= limit / kc.MARGIN + 1e-12


def test_prefill_ops_ref_within_limit():
    """The composed fp32 path of the model (ops.ref.gather_prefix + softmax)
    stays inside the limit on every row."""
    case = prefill_case()
    limit, _ = case.limit()
    kf, vf = case.k_cache.float(), case.v_cache.float()
    out = torch.empty(case.q.shape)
    for i, (start, chunk, prior) in enumerate(case.metas):
        ctx = chunk + prior
        kk, vv = ref.gather_prefix(kf, vf, case.block_tables[i], ctx)
        qi = case.q[start:start + chunk].float().view(
            chunk, case.kvh, QPG, kc.D).permute(1, 2, 0, 3)
        s = torch.einsum("hgtd,hsd->hgts", qi, kk.permute(1, 0, 2))
        s *= case.scale
        hid = torch.arange(ctx).view(1, -1) > \
            torch.arange(chunk).view(-1, 1) + prior
        p = torch.softmax(s.masked_fill(hid, -math.inf), dim=-1)
        o = torch.einsum("hgts,hsd->hgtd", p, vv.permute(1, 0, 2))
        out[start:start + chunk] = o.permute(2, 0, 1, 3).reshape(chunk, -1,
                                                                 kc.D)
    assert worst(out, case) <= limit


@pytest.mark.parametrize("which", ["single", "split"])
def test_decode_ops_ref_within_limit(which):
    case = decode_case() if which == "single" else split_case()
    limit, _ = case.limit()
    out = ref.paged_attention(
        case.q.float(), case.k_cache.float(), case.v_cache.float(),
        case.block_tables, torch.tensor(case.seq_lens), case.scale)
    live = torch.tensor(case.seq_lens) > 0
    err = kc.row_rel_err(out[live], case.reference()[live])
    assert float(err.max()) <= limit


def test_ops_ref_matches_float64():
    """ops/ref.py against the independent float64 versions, small shapes."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 256, generator=g).bfloat16()
    r = torch.randn(5, 256, generator=g).bfloat16()
    w = torch.randn(256, generator=g).bfloat16()
    y64, _ = kc.rmsnorm_ref64(x, w, 1e-5)
    assert float(kc.row_rel_err(ref.rmsnorm(x, w, 1e-5), y64).max()) < kc.FLOOR
    r_ref = r.clone()
    y = ref.rmsnorm(x, w, 1e-5, residual=r_ref)
    y64, r64 = kc.rmsnorm_ref64(x, w, 1e-5, residual=r)
    assert torch.equal(r_ref, r64)
    assert float(kc.row_rel_err(y, y64).max()) < kc.FLOOR

    for d in (64, 128):
        table = ref.rope_table(64, d, 10000.0)
        pos = torch.tensor([0, 63, 7, 1], dtype=torch.int32)
        q = torch.randn(4, 3, d, generator=g).bfloat16()
        k = torch.randn(4, 1, d, generator=g).bfloat16()
        q_ref, k_ref = q.clone(), k.clone()
        ref.rope(q_ref, k_ref, table, pos)
        for got, src in ((q_ref, q), (k_ref, k)):
            want = kc.rope_ref64(src, table, pos)
            assert bool(((got.double() - want).abs()
                         <= kc.bf16_ulp(want)).all())
            assert torch.equal(got, kc.rope_ref32(src, table, pos))

    gu = torch.randn(7, 64, generator=g).bfloat16()
    gu[0, :6] = torch.tensor([-100.0, 100.0, -88.0, 88.0, -3e4, 3e4])
    want = kc.silu_mul_ref64(gu)
    got = ref.silu_mul(gu)
    assert bool(torch.isfinite(got).all())
    assert bool(((got.double() - want).abs() <= kc.bf16_ulp(want)).all())


# ---- mutants -------------------------------------------------------------

@pytest.mark.parametrize("mutant", kc.PREFILL_MUTANTS)
def test_prefill_mutant_is_caught(mutant):
    case = prefill_case()
    limit, _ = case.limit()
    w = worst(kc.prefill_reference(case, mutant=mutant), case)
    assert w > 10 * limit, (mutant, w, limit)


def test_prefill_emulation_within_limit():
    for kv_dtype in ("bf16", "fp8"):
        case = prefill_case(kv_dtype)
        limit, emul_worst = case.limit()
        assert emul_worst <= limit


@pytest.mark.parametrize("mutant", ["drop_last_token", "drop_chunk_tail",
                                    "row_off_by_one"])
def test_decode_mutant_is_caught(mutant):
    case = decode_case()
    limit, emul_worst = case.limit()
    assert emul_worst <= limit
    w = worst(kc.decode_reference(case, mutant=mutant), case)
    assert w > 10 * limit, (mutant, w, limit)


@pytest.mark.parametrize("mutant", kc.DECODE_MUTANTS)
def test_split_decode_mutant_is_caught(mutant):
    case = split_case()
    limit, emul_worst = case.limit()
    assert emul_worst <= limit
    w = worst(kc.decode_reference(case, mutant=mutant), case)
    assert w > 10 * limit, (mutant, w, limit)


# ---- partition geometry of ops.dispatch.paged_attention -------------------

@pytest.mark.parametrize("batch,max_seq_len", [(1, 2049), (3, 4096)])
@pytest.mark.parametrize("chunk", [256, 512])
def test_split_geometry(batch, max_seq_len, chunk):
    np_, part = split_geometry(batch * 2, max_seq_len, chunk)
    assert np_ * part >= max_seq_len
    assert 1 < np_ <= 64
    assert part % chunk == 0


def test_split_geometry_single_pass():
    assert split_geometry(2, None) is None
    assert split_geometry(2, 512) is None
    assert split_geometry(1024, 8192) is None
    # never more than 64 partitions, whatever the length
    for n_wgs in (1, 2, 7, 16, 600, 1023):
        for msl in (513, 2049, 16384, 131072, 1 << 20):
            geom = split_geometry(n_wgs, msl)
            if geom is not None:
                assert geom[0] <= 64 and geom[0] * geom[1] >= msl
                assert geom[1] % 256 == 0
