"""GPU: the fused QKV epilogue (ops.qkv_rope_cache) against the op chain it
replaces, bit for bit: three .contiguous() copies, ops.rope,
ops.reshape_and_cache. Both start from clones of the same randomly filled
caches and the whole caches are compared, so untouched slots are proven
untouched."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

D, BS, NB, MAX_POS = 128, 16, 24, 512


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


@pytest.fixture(scope="module")
def cos_sin():
    from llm_d_inference_scheduler_amd.ops import ref
    return ref.rope_table(MAX_POS, D, 500000.0, device="cuda")


def make_inputs(T, qh, kvh, cache, seed):
    """qkv as a GEMM returns it, positions with 0 and MAX_POS - 1, slots a
    shuffled permutation holding a block's first and last row and (T >= 3)
    two -1 padding slots, randomly filled caches, per-head inverse scales."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, 256, generator=g).bfloat16().cuda()
    w = (torch.randn(256, (qh + 2 * kvh) * D, generator=g) / 16
         ).bfloat16().cuda()
    qkv = x @ w
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[0] = MAX_POS - 1
    pos[-1] = 0 if T > 1 else MAX_POS - 1
    slots = torch.randperm(NB * BS, generator=g)[:T].to(torch.int64)
    # block 5's last row (and, from T = 3, its first), unless the draw
    # holds them already; T = 1 and T = 3 have no room for all of it
    fixed = {T - 1: 5 * BS + BS - 1}
    if T >= 3:
        fixed[0] = 5 * BS
    for i in (1, T // 2 + 1):
        if i < T and i not in fixed:
            slots[i] = -1
    for i, want in fixed.items():
        if want not in slots.tolist():
            slots[i] = want
    dtype = torch.bfloat16 if cache == "bf16" else torch.float8_e4m3fn
    kc = torch.randn(NB, kvh, BS, D, generator=g).to(dtype).cuda()
    vc = torch.randn(NB, kvh, BS, D, generator=g).to(dtype).cuda()
    k_inv = v_inv = None
    if cache == "fp8_scaled":
        k_inv = torch.linspace(0.5, 2.0, kvh).cuda()
        v_inv = torch.linspace(3.0, 0.25, kvh).cuda()
    return qkv, pos.cuda(), slots.cuda(), kc, vc, k_inv, v_inv


def chain(qkv, cos_sin, pos, slots, kc, vc, qh, k_inv, v_inv):
    from llm_d_inference_scheduler_amd import ops
    T = qkv.shape[0]
    kvh = kc.shape[1]
    q, k, v = qkv.split([qh * D, kvh * D, kvh * D], dim=-1)
    q = q.view(T, qh, D).contiguous()
    k = k.view(T, kvh, D).contiguous()
    v = v.view(T, kvh, D).contiguous()
    ops.rope(q, k, cos_sin, pos)
    ops.reshape_and_cache(k, v, kc, vc, slots, k_inv_scale=k_inv,
                          v_inv_scale=v_inv)
    return q


def same_bytes(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("cache", ["bf16", "fp8", "fp8_scaled"])
@pytest.mark.parametrize("qh,kvh", [(8, 2), (4, 4), (32, 8)])
@pytest.mark.parametrize("T", [1, 3, 257])
def test_fused_equals_chain(ext, cos_sin, T, qh, kvh, cache):
    from llm_d_inference_scheduler_amd import ops
    qkv, pos, slots, kc0, vc0, k_inv, v_inv = make_inputs(
        T, qh, kvh, cache, seed=T * 1000 + qh * 10 + kvh)
    assert qkv.is_contiguous()
    kc_a, vc_a = kc0.clone(), vc0.clone()
    # the chain rotates its q and k copies in place; at T == 1 those "copies"
    # are views of qkv, so it gets a clone
    q_a = chain(qkv.clone(), cos_sin, pos, slots, kc_a, vc_a, qh, k_inv,
                v_inv)
    kc_b, vc_b = kc0.clone(), vc0.clone()
    qkv_in = qkv.clone()
    q_b = ops.qkv_rope_cache(qkv_in, cos_sin, pos, slots, kc_b, vc_b, qh,
                             k_inv_scale=k_inv, v_inv_scale=v_inv)
    torch.cuda.synchronize()
    assert q_b.shape == (T, qh, D) and q_b.is_contiguous()
    assert torch.equal(q_a, q_b)
    assert same_bytes(kc_a, kc_b)
    assert same_bytes(vc_a, vc_b)
    assert torch.equal(qkv_in, qkv)                 # input left alone
    assert not same_bytes(kc_b, kc0)                # and something stored
    # exactly the slots that are not padding changed
    changed = (kc_b.view(torch.uint8) != kc0.view(torch.uint8)).any(
        dim=3).any(dim=1).sum().item()
    assert changed == int((slots >= 0).sum())
    assert int((slots < 0).sum()) == {1: 0, 3: 1, 257: 2}[T]


def test_all_padding_stores_nothing(ext, cos_sin):
    from llm_d_inference_scheduler_amd import ops
    qkv, pos, slots, kc0, vc0, _, _ = make_inputs(3, 8, 2, "bf16", seed=7)
    slots[:] = -1
    kc, vc = kc0.clone(), vc0.clone()
    q = ops.qkv_rope_cache(qkv, cos_sin, pos, slots, kc, vc, 8)
    q_ref = chain(qkv.clone(), cos_sin, pos, slots, kc0.clone(),
                  vc0.clone(), 8, None, None)
    assert torch.equal(q, q_ref)
    assert same_bytes(kc, kc0) and same_bytes(vc, vc0)


def test_empty_batch(ext, cos_sin):
    qkv = torch.empty(0, 12 * D, dtype=torch.bfloat16, device="cuda")
    pos = torch.empty(0, dtype=torch.int32, device="cuda")
    slots = torch.empty(0, dtype=torch.int64, device="cuda")
    kc = torch.zeros(NB, 2, BS, D, dtype=torch.bfloat16, device="cuda")
    q = ext.qkv_rope_cache(qkv, cos_sin, pos, slots, kc, kc.clone(), 8)
    assert q.shape == (0, 8, D)


class TestArgumentContract:
    """The binding refuses what the launcher must never see."""

    def args(self, cos_sin):
        qkv, pos, slots, kc, vc, _, _ = make_inputs(3, 8, 2, "bf16", seed=1)
        return dict(qkv=qkv, cos_sin=cos_sin, positions=pos,
                    slot_mapping=slots, k_cache=kc, v_cache=vc, n_q_heads=8)

    def test_accepts_the_good_call(self, ext, cos_sin):
        ext.qkv_rope_cache(**self.args(cos_sin))

    def test_non_contiguous_qkv(self, ext, cos_sin):
        a = self.args(cos_sin)
        wide = torch.zeros(3, 2 * a["qkv"].shape[1], dtype=torch.bfloat16,
                           device="cuda")
        a["qkv"] = wide[:, :a["qkv"].shape[1]]
        with pytest.raises(RuntimeError, match="contiguous"):
            ext.qkv_rope_cache(**a)

    def test_wrong_last_dimension(self, ext, cos_sin):
        a = self.args(cos_sin)
        a["qkv"] = torch.zeros(3, 13 * D, dtype=torch.bfloat16,
                               device="cuda")
        with pytest.raises(RuntimeError, match=r"qkv\.size\(1\)"):
            ext.qkv_rope_cache(**a)

    def test_int32_slot_mapping(self, ext, cos_sin):
        a = self.args(cos_sin)
        a["slot_mapping"] = a["slot_mapping"].to(torch.int32)
        with pytest.raises(RuntimeError, match="slot_mapping"):
            ext.qkv_rope_cache(**a)

    def test_cache_on_another_device(self, ext, cos_sin):
        a = self.args(cos_sin)
        a["k_cache"] = a["k_cache"].cpu()
        with pytest.raises(RuntimeError, match="k_cache"):
            ext.qkv_rope_cache(**a)

    def test_float_positions_and_short_slots(self, ext, cos_sin):
        a = self.args(cos_sin)
        a["positions"] = a["positions"].float()
        with pytest.raises(RuntimeError, match="positions"):
            ext.qkv_rope_cache(**a)
        a = self.args(cos_sin)
        a["slot_mapping"] = a["slot_mapping"][:2].contiguous()
        with pytest.raises(RuntimeError, match="slot_mapping"):
            ext.qkv_rope_cache(**a)

    def test_scales_need_an_fp8_cache(self, ext, cos_sin):
        a = self.args(cos_sin)
        a["k_inv_scale"] = torch.ones(2, device="cuda")
        with pytest.raises(RuntimeError, match="fp8"):
            ext.qkv_rope_cache(**a)


def test_runner_fused_equals_chain():
    """A tiny LlamaRunner on the GPU, one prefill chunk and then one decode
    step, with the fused path and with it forced off: equal logits, equal
    pools."""
    from llm_d_inference_scheduler_amd.models.configs import LLAMA_3_8B
    from llm_d_inference_scheduler_amd.models.llama import (ForwardBatch,
                                                            LlamaRunner)
    cfg = dataclasses.replace(
        LLAMA_3_8B, num_layers=2, hidden_size=256, intermediate_size=512,
        num_heads=8, num_kv_heads=2, vocab_size=1024, max_position=MAX_POS)
    dev = torch.device("cuda")
    runner = LlamaRunner(cfg, dev, seed=11)
    qpg = cfg.num_heads // cfg.num_kv_heads
    # two sequences: 37 and 21 prompt tokens in blocks (3, 1, 6) and (4, 2)
    lens = [37, 21]
    tables = [[3, 1, 6], [4, 2, 0]]
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, cfg.vocab_size, (sum(lens),), generator=g)
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    slots = torch.cat([
        torch.tensor([tables[s][p // BS] * BS + p % BS
                      for p in range(n)]) for s, n in enumerate(lens)])
    bt = torch.tensor(tables, dtype=torch.int32, device=dev)
    tiles = [(s, v) for s, n in enumerate(lens)
             for v in range(0, n * qpg, 128)]
    prefill = ForwardBatch(
        input_ids=ids.to(dev), positions=pos.to(dev),
        slot_mapping=slots.to(torch.int64).to(dev), is_decode=False,
        seq_starts=[0, lens[0], sum(lens)], ctx_lens=lens,
        prefill_bt=bt,
        prefill_meta=torch.tensor([[0, lens[0], 0], [lens[0], lens[1], 0]],
                                  dtype=torch.int32, device=dev),
        prefill_tiles=torch.tensor(tiles, dtype=torch.int32, device=dev),
        logit_rows=torch.tensor([lens[0] - 1, sum(lens) - 1], device=dev))
    decode = ForwardBatch(
        input_ids=torch.tensor([7, 9], device=dev),
        positions=torch.tensor(lens, dtype=torch.int32, device=dev),
        slot_mapping=torch.tensor(
            [tables[s][n // BS] * BS + n % BS for s, n in enumerate(lens)],
            dtype=torch.int64, device=dev),
        is_decode=True, block_tables=bt,
        seq_lens=torch.tensor([n + 1 for n in lens], dtype=torch.int32,
                              device=dev),
        max_seq_len=max(lens) + 1)
    runs = []
    for fused in (True, False):
        runner._fused_qkv = fused
        pool = torch.zeros(cfg.num_layers, 2, 8, cfg.num_kv_heads, BS, D,
                           dtype=torch.bfloat16, device=dev)
        runs.append((runner.forward(prefill, pool),
                     runner.forward(decode, pool), pool))
    torch.cuda.synchronize()
    assert runs[0][0].shape == (2, cfg.vocab_size)
    assert torch.isfinite(runs[0][1].float()).all()
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])
    assert runs[0][2].any()
