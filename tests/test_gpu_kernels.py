"""GPU numerics: every gfx950 HIP kernel vs the plain-torch fp32 reference
(ops.ref), plus the prefix kernels vs the C++ CPU core (bitwise)."""
import numpy as np
import pytest
import torch

from llm_d_inference_scheduler_amd.ops.prefix import _i64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def to_f32(t):
    return t.float().cpu()


class TestPrefixKernelsGPU:
    def test_hash_prompts_matches_cpu(self, ext):
        from llm_d_inference_scheduler_amd import _router_core as rc
        rng = np.random.default_rng(0)
        lens = [16, 33, 100, 256, 4096, 7]
        toks = [rng.integers(0, 2**31 - 1, size=n).astype(np.int32)
                for n in lens]
        flat = np.concatenate(toks)
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        seed0 = rc.model_seed("llama-3-8b", "")
        hashes, counts = ext.hash_prompts(
            torch.from_numpy(flat).cuda(),
            torch.from_numpy(offsets).cuda(), 16, 256, _i64(seed0))
        hashes = hashes.cpu().numpy()
        counts = counts.cpu().numpy()
        for i, t in enumerate(toks):
            cpu = rc.hash_tokens(t, 16, 256, seed0)
            assert counts[i] == len(cpu)
            assert list(hashes[i, :len(cpu)].astype(np.uint64)) == list(cpu)

    def test_table_and_match_matches_cpu(self, ext):
        from llm_d_inference_scheduler_amd import _router_core as rc
        rng = np.random.default_rng(1)
        seed0 = rc.model_seed("m", "")
        cap = 1 << 16
        keys = torch.zeros(cap, dtype=torch.uint64, device="cuda")
        masks = torch.zeros(cap, dtype=torch.uint64, device="cuda")
        cpu_idx = rc.PrefixIndex(100000)
        # 8 endpoints with random prefix sets of a shared token stream
        base = rng.integers(0, 2**31 - 1, size=64 * 16).astype(np.int32)
        h = rc.hash_tokens(base, 16, 256, seed0)
        for e in range(8):
            n = int(rng.integers(1, len(h) + 1))
            cpu_idx.add(e, h[:n])
            ext.table_update(keys, masks,
                             torch.from_numpy(h[:n].astype(np.uint64)).cuda(),
                             e, False)
        # query: the full chain for this prompt
        hq = torch.from_numpy(h.astype(np.uint64)).cuda().view(1, -1)
        counts = torch.tensor([len(h)], dtype=torch.int32, device="cuda")
        gpu = ext.match_longest(keys, masks, hq, counts, 8).cpu().numpy()[0]
        cpu = cpu_idx.match_longest(h, 8)
        assert list(gpu) == list(cpu)
        # removal parity
        ext.table_update(keys, masks,
                         torch.from_numpy(h[:4].astype(np.uint64)).cuda(),
                         0, True)
        gpu2 = ext.match_longest(keys, masks, hq, counts, 8).cpu().numpy()[0]
        assert gpu2[0] == 0  # leading blocks removed -> no prefix match
        # the same history through the table model (ops.ref): equal
        # (key, mask) entries, dead keys included, and equal matches for
        # every endpoint, not endpoint 0 alone
        from llm_d_inference_scheduler_amd.ops import ref
        mk = torch.zeros(cap, dtype=torch.uint64)
        mm = torch.zeros(cap, dtype=torch.uint64)
        rng = np.random.default_rng(1)
        rng.integers(0, 2**31 - 1, size=64 * 16)    # replay the draws above
        for e in range(8):
            n = int(rng.integers(1, len(h) + 1))
            ref.table_update(mk, mm, torch.from_numpy(h[:n].astype(np.uint64)),
                             e, False)
        ref.table_update(mk, mm, torch.from_numpy(h[:4].astype(np.uint64)),
                         0, True)

        def entries(k, m):
            k, m = k.cpu().numpy(), m.cpu().numpy()
            return sorted(zip(k[k != 0].tolist(), m[k != 0].tolist()))
        assert entries(keys, masks) == entries(mk, mm)
        model2 = ref.match_longest(mk, mm, hq.cpu(), counts.cpu(), 8).numpy()[0]
        assert list(gpu2) == list(model2)
        assert list(gpu2[1:]) == list(gpu[1:])      # other endpoints unmoved
        # and the host index agrees once endpoint 0 is rebuilt without its
        # first four blocks
        n0 = int(cpu[0])
        cpu_idx.remove_endpoint(0)
        cpu_idx.add(0, h[4:n0])
        assert list(gpu2) == list(cpu_idx.match_longest(h, 8))


class TestEngineKernelsGPU:
    def test_rmsnorm(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(0)
        x = torch.randn(129, 4096, device="cuda").bfloat16()
        w = torch.randn(4096, device="cuda").bfloat16()
        y = ext.rmsnorm(x, w, 1e-5, None)
        y_ref = ref.rmsnorm(x.clone(), w, 1e-5)
        assert torch.allclose(to_f32(y), to_f32(y_ref), atol=2e-2, rtol=2e-2)

    def test_rmsnorm_residual(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(1)
        x = torch.randn(64, 4096, device="cuda").bfloat16()
        r_hip = torch.randn(64, 4096, device="cuda").bfloat16()
        r_ref = r_hip.clone()
        w = torch.randn(4096, device="cuda").bfloat16()
        y = ext.rmsnorm(x, w, 1e-5, r_hip)
        y_ref = ref.rmsnorm(x.clone(), w, 1e-5, residual=r_ref)
        assert torch.allclose(to_f32(r_hip), to_f32(r_ref), atol=2e-2,
                              rtol=2e-2)
        assert torch.allclose(to_f32(y), to_f32(y_ref), atol=2e-2, rtol=2e-2)

    def test_rmsnorm_large_h(self, ext):
        """H > 256*8 cache chunks exercises the re-read overflow path."""
        from llm_d_inference_scheduler_amd.ops import ref
        x = torch.randn(8, 16384 + 4096, device="cuda").bfloat16()
        w = torch.ones(16384 + 4096, device="cuda").bfloat16()
        y = ext.rmsnorm(x, w, 1e-5, None)
        y_ref = ref.rmsnorm(x.clone(), w, 1e-5)
        assert torch.allclose(to_f32(y), to_f32(y_ref), atol=2e-2, rtol=2e-2)

    def test_rope(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(2)
        T, QH, KVH, D = 33, 32, 8, 128
        q_hip = torch.randn(T, QH, D, device="cuda").bfloat16()
        k_hip = torch.randn(T, KVH, D, device="cuda").bfloat16()
        q_ref, k_ref = q_hip.clone(), k_hip.clone()
        table = ref.rope_table(4096, D, 500000.0, device="cuda")
        pos = torch.randint(0, 4096, (T,), dtype=torch.int32, device="cuda")
        ext.rope(q_hip, k_hip, table, pos)
        ref.rope(q_ref, k_ref, table, pos)
        assert torch.allclose(to_f32(q_hip), to_f32(q_ref), atol=2e-2,
                              rtol=2e-2)
        assert torch.allclose(to_f32(k_hip), to_f32(k_ref), atol=2e-2,
                              rtol=2e-2)

    def test_silu_mul(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(3)
        gu = torch.randn(77, 2 * 14336, device="cuda").bfloat16()
        y = ext.silu_mul(gu)
        y_ref = ref.silu_mul(gu)
        assert torch.allclose(to_f32(y), to_f32(y_ref), atol=2e-2, rtol=2e-2)

    def test_reshape_and_cache(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(4)
        T, KVH, D, NB, BS = 50, 8, 128, 32, 16
        k = torch.randn(T, KVH, D, device="cuda").bfloat16()
        v = torch.randn(T, KVH, D, device="cuda").bfloat16()
        kc = torch.zeros(NB, KVH, BS, D, device="cuda").bfloat16()
        vc = torch.zeros_like(kc)
        kc_ref, vc_ref = kc.clone().cpu(), vc.clone().cpu()
        slots = torch.randperm(NB * BS)[:T].to(torch.int64)
        ext.reshape_and_cache(k, v, kc, vc, slots.cuda())
        ref.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots)
        assert torch.equal(kc.cpu(), kc_ref)
        assert torch.equal(vc.cpu(), vc_ref)

    @pytest.mark.parametrize("qpg,seqs", [(4, [1, 16, 333, 1024, 2049]),
                                          (8, [500]), (1, [77])])
    def test_paged_attention(self, ext, qpg, seqs):
        from llm_d_inference_scheduler_amd.ops import ref
        torch.manual_seed(5)
        KVH, D, BS = 8, 128, 16
        QH = KVH * qpg
        B = len(seqs)
        max_blocks = (max(seqs) + BS - 1) // BS
        NB = max_blocks * B + 1
        q = torch.randn(B, QH, D, device="cuda").bfloat16()
        kc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        vc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        bt = torch.zeros(B, max_blocks, dtype=torch.int32)
        perm = torch.randperm(NB - 1) + 1
        k = 0
        for b, s in enumerate(seqs):
            nb = (s + BS - 1) // BS
            bt[b, :nb] = perm[k:k + nb]
            k += nb
        sl = torch.tensor(seqs, dtype=torch.int32)
        out = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(),
                                  D ** -0.5)
        out_ref = ref.paged_attention(to_f32(q), to_f32(kc), to_f32(vc),
                                      bt, sl, D ** -0.5)
        assert torch.allclose(to_f32(out), out_ref, atol=3e-2, rtol=3e-2), \
            (to_f32(out) - out_ref).abs().max()

    @pytest.mark.parametrize("seqs,np_,part", [([1024, 2049, 333], 4, 768),
                                               ([8192], 16, 512),
                                               ([100, 700], 2, 512)])
    def test_paged_attention_split(self, ext, seqs, np_, part):
        """Flash-decoding partitioned kernel == the single-pass kernel."""
        torch.manual_seed(6)
        KVH, D, BS, qpg = 8, 128, 16, 4
        QH = KVH * qpg
        B = len(seqs)
        max_blocks = (max(seqs) + BS - 1) // BS
        NB = max_blocks * B + 1
        q = torch.randn(B, QH, D, device="cuda").bfloat16()
        kc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        vc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        bt = torch.zeros(B, max_blocks, dtype=torch.int32)
        perm = torch.randperm(NB - 1) + 1
        k = 0
        for b, s in enumerate(seqs):
            nb = (s + BS - 1) // BS
            bt[b, :nb] = perm[k:k + nb]
            k += nb
        sl = torch.tensor(seqs, dtype=torch.int32)
        base = ext.paged_attention(q, kc, vc, bt.cuda(), sl.cuda(), D ** -0.5)
        split = ext.paged_attention_split(q, kc, vc, bt.cuda(), sl.cuda(),
                                          np_, part, D ** -0.5)
        assert torch.allclose(to_f32(base), to_f32(split), atol=2e-2,
                              rtol=2e-2), (to_f32(base) - to_f32(split)).abs().max()

    @pytest.mark.parametrize(
        "qpg,chunks,priors",
        [(4, [128, 333, 1024], [0, 171, 0]),     # mixed varlen + chunked
         (8, [257], [512]),                      # chunked continuation
         (1, [64], [0]),                         # MHA (LLaVA text shape)
         (4, [2048], [0])])                      # long single prefill
    def test_flash_prefill(self, ext, qpg, chunks, priors):
        """Fused MFMA flash prefill vs fp32 composed causal attention."""
        torch.manual_seed(7)
        KVH, D, BS = 8, 128, 16
        QH = KVH * qpg
        ctxs = [c + p for c, p in zip(chunks, priors)]
        max_blocks = (max(ctxs) + BS - 1) // BS
        NB = max_blocks * len(chunks) + 1
        T = sum(chunks)
        q = torch.randn(T, QH, D, device="cuda").bfloat16()
        kc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        vc = torch.randn(NB, KVH, BS, D, device="cuda").bfloat16()
        bt = torch.zeros(len(chunks), max_blocks, dtype=torch.int32)
        perm = torch.randperm(NB - 1) + 1
        k = 0
        starts = [0]
        for i, ctx in enumerate(ctxs):
            nb = (ctx + BS - 1) // BS
            bt[i, :nb] = perm[k:k + nb]
            k += nb
            starts.append(starts[-1] + chunks[i])
        metas = [(starts[i], chunks[i], priors[i])
                 for i in range(len(chunks))]
        tiles = [(i, v0) for i in range(len(chunks))
                 for v0 in range(0, chunks[i] * qpg, 128)]
        scale = D ** -0.5
        out = ext.flash_prefill(
            q, kc, vc, bt.cuda(),
            torch.tensor(metas, dtype=torch.int32, device="cuda"),
            torch.tensor(tiles, dtype=torch.int32, device="cuda"), scale)
        # fp32 reference: gather each sequence's KV, causal softmax
        out_ref = torch.empty(T, QH, D)
        qf = to_f32(q)
        kcf, vcf = to_f32(kc), to_f32(vc)
        for i, ctx in enumerate(ctxs):
            rows = bt[i, :(ctx + BS - 1) // BS].long()
            kk = kcf[rows].permute(1, 0, 2, 3).reshape(KVH, -1, D)[:, :ctx]
            vv = vcf[rows].permute(1, 0, 2, 3).reshape(KVH, -1, D)[:, :ctx]
            qi = qf[starts[i]:starts[i + 1]].view(
                chunks[i], KVH, qpg, D).permute(1, 2, 0, 3)
            s = torch.einsum("hgtd,hsd->hgts", qi, kk) * scale
            t_idx = torch.arange(chunks[i]).view(1, 1, -1, 1)
            s_idx = torch.arange(ctx).view(1, 1, 1, -1)
            s.masked_fill_(s_idx > t_idx + priors[i], float("-inf"))
            p = torch.softmax(s, dim=-1)
            o = torch.einsum("hgts,hsd->hgtd", p, vv)
            out_ref[starts[i]:starts[i + 1]] = o.permute(2, 0, 1, 3).reshape(
                chunks[i], QH, D)
        diff = (to_f32(out) - out_ref).abs().max()
        assert torch.allclose(to_f32(out), out_ref, atol=3e-2,
                              rtol=3e-2), diff

    def test_move_blocks_roundtrip(self, ext):
        L, NB, KVH, BS, D = 4, 64, 8, 16, 128
        pool = torch.randn(L, 2, NB, KVH, BS, D, device="cuda").bfloat16()
        pool2 = torch.zeros_like(pool)
        ids = torch.tensor([3, 17, 42, 5], dtype=torch.int32, device="cuda")
        staging = torch.empty(4, L, 2, KVH, BS, D, device="cuda",
                              dtype=torch.bfloat16)
        ext.move_blocks(pool, staging, ids, False)   # gather
        ext.move_blocks(pool2, staging, ids, True)   # scatter
        assert torch.equal(pool[:, :, ids.long()], pool2[:, :, ids.long()])

    def test_copy_blocks_peer_same_process(self, ext):
        """Peer-pull gather kernel over a raw device pointer (the IPC
        mapping itself is exercised by the 2-process P/D rig): pulled
        blocks land bit-exact in the destination pool slots."""
        L, NB, KVH, BS, D = 4, 48, 8, 16, 128
        src = torch.randn(L, 2, NB, KVH, BS, D, device="cuda").bfloat16()
        dst = torch.zeros(L, 2, 32, KVH, BS, D, device="cuda",
                          dtype=torch.bfloat16)
        src_ids = torch.tensor([7, 0, 41], dtype=torch.int32, device="cuda")
        dst_ids = torch.tensor([2, 30, 11], dtype=torch.int32, device="cuda")
        ext.copy_blocks_peer(src.data_ptr(), dst, src_ids, dst_ids, NB)
        torch.cuda.synchronize()
        assert torch.equal(dst[:, :, dst_ids.long()],
                           src[:, :, src_ids.long()])

    def test_ipc_alloc_tensor(self, ext):
        """hipMalloc-backed pool: normal tensor semantics + handle export."""
        like = torch.empty(0, dtype=torch.bfloat16, device="cuda")
        t = ext.ipc_alloc_tensor([2, 2, 8, 4, 16, 64], like)
        assert t.is_cuda and t.dtype == torch.bfloat16
        assert float(t.abs().sum()) == 0.0          # zero-initialized
        t.fill_(1.5)
        assert float(t.mean()) == 1.5
        h = ext.ipc_handle(t)
        assert isinstance(h, bytes) and len(h) == 64


class TestEngineGPU:
    def test_tiny_engine_decode_gpu_vs_cpu_shape(self):
        """Engine runs end-to-end on GPU with the HIP path and produces the
        contracted output shapes; greedy decode is deterministic."""
        from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                          EngineWorker)
        from llm_d_inference_scheduler_amd.models.configs import ModelConfig
        cfg = ModelConfig(name="gpu-test", vocab_size=2048, hidden_size=1024,
                          intermediate_size=2048, num_layers=2, num_heads=8,
                          num_kv_heads=2, head_dim=128, rope_theta=10000.0)
        gens = []
        for _ in range(2):
            w = EngineWorker(cfg, "cuda:0", kv_blocks=256,
                             dtype=torch.bfloat16, seed=9)
            w.add_request(EngineRequest("a", prompt_tokens=list(range(300,
                                                                     430)),
                                        max_tokens=6))
            toks = []
            for _ in range(30):
                for o in w.step():
                    toks.extend(o.new_tokens)
                if not w.has_work:
                    break
            gens.append(toks)
        assert len(gens[0]) == 6
        assert gens[0] == gens[1]


class TestGpuPrefixIndex:
    def test_batched_router_path_matches_host(self):
        """GpuPrefixIndex batch hash+match == host C++ index for the same
        insert history (the production router path on GPU boxes)."""
        from llm_d_inference_scheduler_amd import _router_core as rc
        from llm_d_inference_scheduler_amd.ops.prefix import GpuPrefixIndex
        rng = np.random.default_rng(7)
        gpu = GpuPrefixIndex("cuda:0", capacity_pow2=1 << 16)
        host = rc.PrefixIndex(10000)
        seed0 = rc.model_seed("llama-3-8b", "")
        prompts = [rng.integers(256, 100000, size=int(n)).astype(np.int32)
                   for n in rng.integers(16, 800, size=12)]
        # seed both indexes with a few routed prompts
        for e, p in enumerate(prompts[:6]):
            h = rc.hash_tokens(p, 16, 256, seed0)
            host.add(e % 4, h)
            gpu.add(e % 4, h)
        # query batch: mix of seen/unseen with shared prefixes
        queries = [prompts[0], prompts[3][:64],
                   np.concatenate([prompts[1][:32], prompts[9][:32]]),
                   prompts[11]]
        hashes, counts = gpu.hash_prompts_batch(
            [q.tolist() for q in queries], 16, 256, seed0)
        match = gpu.match_batch(hashes, counts, 4).cpu().numpy()
        for i, q in enumerate(queries):
            hq = rc.hash_tokens(q, 16, 256, seed0)
            expect = host.match_longest(hq, 4)
            assert list(match[i]) == list(expect), i


class TestFp8KVCacheGPU:
    """fp8 (OCP e4m3) KV-cache kernels vs fp32 reference computed on the
    SAME quantized values — isolates kernel correctness from quantization."""

    def _setup(self, B, seqs_max, qpg=4):
        KVH, D, BS = 8, 128, 16
        QH = KVH * qpg
        max_blocks = (seqs_max + BS - 1) // BS
        NB = max_blocks * B + 1
        torch.manual_seed(11)
        q = torch.randn(B, QH, D, device="cuda").bfloat16()
        kc8 = torch.randn(NB, KVH, BS, D, device="cuda").to(
            torch.float8_e4m3fn)
        vc8 = torch.randn(NB, KVH, BS, D, device="cuda").to(
            torch.float8_e4m3fn)
        bt = torch.arange(1, NB, dtype=torch.int32,
                          device="cuda").view(B, max_blocks)
        return q, kc8, vc8, bt, KVH, D, BS

    def test_reshape_and_cache_fp8(self, ext):
        T, KVH, D, NB, BS = 40, 8, 128, 16, 16
        k = torch.randn(T, KVH, D, device="cuda").bfloat16()
        v = torch.randn(T, KVH, D, device="cuda").bfloat16()
        kc = torch.zeros(NB, KVH, BS, D, device="cuda").to(
            torch.float8_e4m3fn)
        vc = torch.zeros_like(kc)
        slots = torch.randperm(NB * BS)[:T].to(torch.int64).cuda()
        ext.reshape_and_cache(k, v, kc, vc, slots)
        # the hardware v_cvt_pk_fp8_f32 pack should round like torch's cast
        # (both round-to-nearest-even); compare exactly on scattered slots
        want_k = k.float().to(torch.float8_e4m3fn).float().cpu()
        want_v = v.float().to(torch.float8_e4m3fn).float().cpu()
        for t in range(T):
            s = int(slots[t])
            blk, row = s // BS, s % BS
            assert torch.equal(kc[blk, :, row].float().cpu(), want_k[t]), t
            assert torch.equal(vc[blk, :, row].float().cpu(), want_v[t]), t

    def test_paged_attention_fp8(self, ext):
        from llm_d_inference_scheduler_amd.ops import ref
        seqs = [77, 1024, 333]
        q, kc8, vc8, bt, KVH, D, BS = self._setup(len(seqs), max(seqs))
        sl = torch.tensor(seqs, dtype=torch.int32)
        out = ext.paged_attention(q, kc8, vc8, bt, sl.cuda(), D ** -0.5)
        out_ref = ref.paged_attention(to_f32(q), kc8.float().cpu(),
                                      vc8.float().cpu(), bt.cpu(), sl,
                                      D ** -0.5)
        assert torch.allclose(to_f32(out), out_ref, atol=3e-2, rtol=3e-2), \
            (to_f32(out) - out_ref).abs().max()
        # split path agrees
        out2 = ext.paged_attention_split(q, kc8, vc8, bt, sl.cuda(), 4, 512,
                                         D ** -0.5)
        assert torch.allclose(to_f32(out), to_f32(out2), atol=2e-2,
                              rtol=2e-2)

    def test_flash_prefill_fp8(self, ext):
        KVH, D, BS, qpg = 8, 128, 16, 4
        QH = KVH * qpg
        chunk, prior = 333, 171
        ctx = chunk + prior
        nb = (ctx + BS - 1) // BS
        torch.manual_seed(12)
        q = torch.randn(chunk, QH, D, device="cuda").bfloat16()
        kc8 = torch.randn(nb + 1, KVH, BS, D, device="cuda").to(
            torch.float8_e4m3fn)
        vc8 = torch.randn(nb + 1, KVH, BS, D, device="cuda").to(
            torch.float8_e4m3fn)
        bt = torch.arange(1, nb + 1, dtype=torch.int32,
                          device="cuda").view(1, -1)
        meta = torch.tensor([[0, chunk, prior]], dtype=torch.int32,
                            device="cuda")
        tiles = torch.tensor([(0, v) for v in range(0, chunk * qpg, 128)],
                             dtype=torch.int32, device="cuda")
        scale = D ** -0.5
        out = ext.flash_prefill(q, kc8, vc8, bt, meta, tiles, scale)
        kk = kc8.float().cpu()[1:].permute(1, 0, 2, 3).reshape(
            KVH, -1, D)[:, :ctx]
        vv = vc8.float().cpu()[1:].permute(1, 0, 2, 3).reshape(
            KVH, -1, D)[:, :ctx]
        qi = to_f32(q).view(chunk, KVH, qpg, D).permute(1, 2, 0, 3)
        s = torch.einsum("hgtd,hsd->hgts", qi, kk) * scale
        t_idx = torch.arange(chunk).view(1, 1, -1, 1)
        s_idx = torch.arange(ctx).view(1, 1, 1, -1)
        s.masked_fill_(s_idx > t_idx + prior, float("-inf"))
        o = torch.einsum("hgts,hsd->hgtd", torch.softmax(s, -1), vv)
        out_ref = o.permute(2, 0, 1, 3).reshape(chunk, QH, D)
        assert torch.allclose(to_f32(out), out_ref, atol=3e-2, rtol=3e-2), \
            (to_f32(out) - out_ref).abs().max()

    def test_engine_fp8_end_to_end(self):
        from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                          EngineWorker)
        from llm_d_inference_scheduler_amd.models.configs import ModelConfig
        cfg = ModelConfig(name="gpu-test", vocab_size=2048, hidden_size=1024,
                          intermediate_size=2048, num_layers=2, num_heads=8,
                          num_kv_heads=2, head_dim=128, rope_theta=10000.0)
        w = EngineWorker(cfg, "cuda:0", kv_blocks=256, dtype=torch.bfloat16,
                         kv_cache_dtype="fp8", seed=9)
        assert w.pool.tensor.dtype == torch.float8_e4m3fn
        w.add_request(EngineRequest("a", prompt_tokens=list(range(300, 430)),
                                    max_tokens=6))
        toks = []
        for _ in range(30):
            for o in w.step():
                toks.extend(o.new_tokens)
            if not w.has_work:
                break
        assert len(toks) == 6


class TestEngineFeaturesGPU:
    def _cfg(self):
        from llm_d_inference_scheduler_amd.models.configs import ModelConfig
        return ModelConfig(name="gpu-test", vocab_size=2048,
                           hidden_size=1024, intermediate_size=2048,
                           num_layers=2, num_heads=8, num_kv_heads=2,
                           head_dim=128, rope_theta=10000.0)

    def test_chunked_decode_node_gpu(self):
        from llm_d_inference_scheduler_amd.node import NodeConfig, NodeRunner
        from llm_d_inference_scheduler_amd.scheduling.types import LLMRequest
        results = {}
        for chunk in (None, 4):
            node = NodeRunner(NodeConfig(
                model=self._cfg(), world_size=1, topology="mono",
                device="cuda:0", dtype=torch.bfloat16, kv_blocks=512,
                decode_chunk_tokens=chunk, seed=7))
            node.submit(LLMRequest(request_id="r", model="gpu-test",
                                   prompt="", prompt_tokens=list(range(300,
                                                                       400)),
                                   max_tokens=10))
            got = []
            for _ in range(200):
                node.step()
                got.extend(node.drain_completions())
                if got:
                    break
            node.shutdown()
            assert got and not got[0].error
            assert got[0].usage.completion_tokens == 10
            results[chunk] = got[0].tokens
        assert results[None] == results[4]

    def test_preemption_gpu(self):
        from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                          EngineWorker)
        w = EngineWorker(self._cfg(), "cuda:0", kv_blocks=24,
                         dtype=torch.bfloat16, seed=5)
        for i in range(3):
            w.add_request(EngineRequest(f"r{i}",
                                        list(range(100 + i, 180 + i)),
                                        max_tokens=40))
        outs = []
        for _ in range(600):
            outs.extend(w.step())
            if not w.has_work:
                break
        fins = {o.request_id: o for o in outs if o.finished}
        assert len(fins) == 3
        assert all(o.completion_tokens == 40 for o in fins.values())


class TestStreamOverlapGPU:
    def test_overlap_matches_sequential(self):
        """Prefill/decode stream overlap (engine/worker.py step()) is
        bit-identical to the sequential path: same kernels, same order
        within each pass, disjoint sequences."""
        import dataclasses
        from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                          EngineWorker)
        from llm_d_inference_scheduler_amd.models.configs import ModelConfig
        cfg = ModelConfig(name="gpu-ov", vocab_size=2048, hidden_size=1024,
                          intermediate_size=2048, num_layers=2, num_heads=8,
                          num_kv_heads=2, head_dim=128, rope_theta=10000.0)
        results = {}
        for overlap in (False, True):
            w = EngineWorker(cfg, "cuda:0", kv_blocks=512,
                             dtype=torch.bfloat16, seed=11,
                             overlap_streams=overlap,
                             prefill_min_tokens=64)
            toks = {}
            # staggered arrivals force waiting+running coexistence
            w.add_request(EngineRequest("a", list(range(300, 500)),
                                        max_tokens=24))
            for step in range(80):
                if step == 4:
                    w.add_request(EngineRequest("b", list(range(700, 1020)),
                                                max_tokens=16))
                if step == 8:
                    w.add_request(EngineRequest("c", list(range(64, 192)),
                                                max_tokens=12))
                for o in w.step():
                    if o.finished:
                        toks[o.request_id] = o.all_tokens
                if not w.has_work:
                    break
            assert set(toks) == {"a", "b", "c"}
            results[overlap] = toks
        assert results[False] == results[True]


class TestQKNormGPU:
    def test_qwen_qk_norm_hip_path(self):
        """Per-head QK-RMSNorm rides the HIP rmsnorm kernel on [T*H, D]
        rows: GPU generation matches the structure of the CPU run (same
        count; norm toggling changes outputs)."""
        import dataclasses
        from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                          EngineWorker)
        from llm_d_inference_scheduler_amd.models.configs import ModelConfig
        cfg = ModelConfig(name="gpu-qk", vocab_size=2048, hidden_size=1024,
                          intermediate_size=2048, num_layers=2, num_heads=8,
                          num_kv_heads=2, head_dim=128, rope_theta=1e4,
                          qk_norm=True)
        outs = {}
        for qk in (True, False):
            c = dataclasses.replace(cfg, qk_norm=qk)
            w = EngineWorker(c, "cuda:0", kv_blocks=256,
                             dtype=torch.bfloat16, seed=13)
            w.add_request(EngineRequest("q", list(range(300, 430)),
                                        max_tokens=6))
            toks = []
            for _ in range(30):
                for o in w.step():
                    toks.extend(o.new_tokens)
                if not w.has_work:
                    break
            assert len(toks) == 6
            outs[qk] = toks
        assert outs[True] != outs[False]
