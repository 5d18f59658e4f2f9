"""GPU tier of the fp8 KV-scale feature: the scaled store bit for bit, the
scaled decode / split / prefill kernels against float64 on the dequantised
values (the inputs, poison and per-row limit of tests/kernel_cases.py), and
the engine end to end on a model rescaled by powers of two.

A stored byte is fp8_rne(clamp(float(x) * inv_scale[h], -448, 448)) and
means float(byte) * scale[h]; see KVPool (engine/kvcache.py).

Each kernel test prints one `EDGE|kernel|case|limit|worst` line before it
asserts (pytest -s shows them)."""
import dataclasses

import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu

K_SCALE = [2.0 ** -3, 2.0 ** 2]     # KVH is 2 in the kernel cases: a head
V_SCALE = [0.37, 5.0]               # index mistake shows


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def f32(values):
    return torch.tensor(values, dtype=torch.float32)


def judge(kernel, name, out, case):
    limit, _ = case.limit()
    worst = float(kc.row_rel_err(out.cpu(), case.reference()).max())
    print(f"EDGE|{kernel}|{name}|{limit:.3e}|{worst:.3e}")
    assert worst <= limit, (kernel, name, worst, limit)


def dequantised(case, k_scale, v_scale, rescale_q):
    """The case the kernel output is judged against: caches replaced by
    the fp32 values the scaled bytes mean, so reference() and limit()
    describe the true dequantised attention; with rescale_q, q divided per
    KV-head group by k_scale (a power of two: exact in bf16), which keeps
    the needle logits where the case designed them."""
    ks, vs = f32(k_scale), f32(v_scale)
    assert case.kvh == len(k_scale) == len(v_scale)
    q = case.q
    if rescale_q:
        per_head = (1.0 / ks).repeat_interleave(case.qpg)       # [QH]
        q = (case.q.float() * per_head.view(1, -1, 1)).bfloat16()
        assert torch.equal(q.float() * (1.0 / per_head).view(1, -1, 1),
                           case.q.float())                      # exact
    return dataclasses.replace(
        case, q=q,
        k_cache=case.k_cache.float() * ks.view(1, -1, 1, 1),
        v_cache=case.v_cache.float() * vs.view(1, -1, 1, 1),
        _cache={})


def decode_args(judged, case):
    """Rescaled q, the ORIGINAL fp8 caches."""
    assert case.k_cache.dtype == kc.FP8
    return (judged.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(),
            case.block_tables.cuda(),
            torch.tensor(case.seq_lens, dtype=torch.int32, device="cuda"))


def raw(t):
    return t.view(torch.uint8)


# ---- 1. store ------------------------------------------------------------

def store_inputs():
    g = torch.Generator().manual_seed(40)
    T, KVH, D, BS, NB = 40, 4, 128, 16, 16
    k_scale = f32([0.25, 1.0, 3.0, 0.013])
    v_scale = f32([8.0, 0.5, 1.7, 100.0])
    spread = f32([1.0, 30.0, 600.0, 1e-2]).view(1, KVH, 1)
    new = []
    for scale in (k_scale, v_scale):
        x = torch.randn(T, KVH, D, generator=g) * spread
        amax = x.abs().amax(dim=(0, 2))
        for h in range(KVH):
            x[1, h, 0] = 0.0
            x[3, h, 7] = amax[h]
            x[4, h, 9] = -amax[h]
            # beyond the e4m3 range after scaling, whatever the head's spread
            x[6 + h, h, 11] = 448.0 * 1.5 * float(scale[h])
            x[20 + h, h, 13] = -448.0 * 40.0 * float(scale[h])
        new.append(x.bfloat16())
    k, v = new
    assert float(k[:, 1].abs().max()) > 448 and float(k[:, 2].abs().max()) > 448
    inv_k, inv_v = 1.0 / k_scale, 1.0 / v_scale
    for x, inv in ((k, inv_k), (v, inv_v)):
        over = (x.float() * inv.view(1, -1, 1)).abs() > 448
        assert bool(over.any(dim=2).any(dim=0).all())   # in every head
    # slots over blocks 0..NB-3, shuffled; two padding tokens; the last two
    # blocks are never written
    slots = torch.randperm((NB - 2) * BS, generator=g)[:T].to(torch.int64)
    slots[12], slots[31] = -1, -1
    k_cache = torch.randint(0, 256, (NB, KVH, BS, D), generator=g,
                            dtype=torch.uint8).view(kc.FP8)
    v_cache = torch.randint(0, 256, (NB, KVH, BS, D), generator=g,
                            dtype=torch.uint8).view(kc.FP8)
    return k, v, k_cache, v_cache, slots, inv_k, inv_v


def expected_store(k, v, k_cache, v_cache, slots, inv_k, inv_v):
    BS = k_cache.shape[2]
    want_k, want_v = raw(k_cache).clone(), raw(v_cache).clone()
    new_k = raw((k.float() * inv_k.view(1, -1, 1)).clamp(-448, 448).to(kc.FP8))
    new_v = raw((v.float() * inv_v.view(1, -1, 1)).clamp(-448, 448).to(kc.FP8))
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            want_k[s // BS, :, s % BS] = new_k[t]
            want_v[s // BS, :, s % BS] = new_v[t]
    return want_k, want_v


def test_store_scaled_bitwise(ext):
    """One IEEE fp32 multiply, a clamp and round-to-nearest-even on both
    sides, so written rows are equal bit for bit; every other row of the
    cache (padding tokens, unwritten rows and blocks) keeps its bytes."""
    k, v, k_cache, v_cache, slots, inv_k, inv_v = store_inputs()
    want_k, want_v = expected_store(k, v, k_cache, v_cache, slots,
                                    inv_k, inv_v)
    k_hip, v_hip = k_cache.cuda(), v_cache.cuda()
    ext.reshape_and_cache(k.cuda(), v.cuda(), k_hip, v_hip, slots.cuda(),
                          inv_k.cuda(), inv_v.cuda())
    got_k, got_v = raw(k_hip.cpu()), raw(v_hip.cpu())
    BS = k_cache.shape[2]
    written = torch.zeros(k_cache.shape[0], BS, dtype=torch.bool)
    for s in slots.tolist():
        if s >= 0:
            written[s // BS, s % BS] = True
    assert int(written.sum()) == 38 and not written[-2:].any()
    for got, want, old in ((got_k, want_k, raw(k_cache)),
                           (got_v, want_v, raw(v_cache))):
        g_rows, w_rows = got.permute(0, 2, 1, 3), want.permute(0, 2, 1, 3)
        n_bad = int((g_rows[written] != w_rows[written]).sum())
        print(f"EDGE|reshape_and_cache scaled|written rows|0|{n_bad} bytes")
        assert torch.equal(g_rows[written], w_rows[written])
        # saturated elements are +-448 (0x7e / 0xfe), never NaN (0x7f)
        assert bool(((g_rows[written] & 0x7F) != 0x7F).all())
        assert int(((g_rows[written] & 0x7F) == 0x7E).sum()) >= 8
        # padding tokens, unwritten rows and blocks: bytes unchanged
        assert torch.equal(g_rows[~written],
                           old.permute(0, 2, 1, 3)[~written])
        assert torch.equal(got, want)


def test_store_unit_scales_equal_unscaled(ext):
    """Without scales the kernel takes the code path it always took; with
    all-ones scales it multiplies by 1.0 and clamps. The inputs here are
    the store test's, clamped to the e4m3 range first: beyond 448 the
    unscaled path leaves the result to the conversion instruction, which
    is exactly what the scaled path must not depend on."""
    k, v, k_cache, v_cache, slots, _, _ = store_inputs()
    k = k.float().clamp(-448, 448).bfloat16()
    v = v.float().clamp(-448, 448).bfloat16()
    ones = torch.ones(4, dtype=torch.float32, device="cuda")
    plain_k, plain_v = k_cache.cuda(), v_cache.cuda()
    ext.reshape_and_cache(k.cuda(), v.cuda(), plain_k, plain_v, slots.cuda())
    unit_k, unit_v = k_cache.cuda(), v_cache.cuda()
    ext.reshape_and_cache(k.cuda(), v.cuda(), unit_k, unit_v, slots.cuda(),
                          ones, ones)
    assert torch.equal(raw(plain_k.cpu()), raw(unit_k.cpu()))
    assert torch.equal(raw(plain_v.cpu()), raw(unit_v.cpu()))
    # and only one of the two scales may be given
    half_k, half_v = k_cache.cuda(), v_cache.cuda()
    ext.reshape_and_cache(k.cuda(), v.cuda(), half_k, half_v, slots.cuda(),
                          None, ones)
    assert torch.equal(raw(plain_k.cpu()), raw(half_k.cpu()))
    assert torch.equal(raw(plain_v.cpu()), raw(half_v.cpu()))


# ---- 2. decode, plain ----------------------------------------------------

@pytest.mark.parametrize("qpg", [1, 4])
def test_paged_attention_scaled(ext, qpg):
    case = kc.make_decode_case(qpg, kc.DECODE_SEQS, kv_dtype="fp8")
    judged = dequantised(case, K_SCALE, V_SCALE, rescale_q=True)
    out = ext.paged_attention(*decode_args(judged, case), case.scale, 256,
                              f32(K_SCALE).cuda(), f32(V_SCALE).cuda()).cpu()
    assert case.seq_lens[0] == 0
    assert bool((out[0].float() == 0).all())        # l == 0 -> exact zeros
    # the 448 poison stays finite under these scales and must not leak
    assert bool(torch.isfinite(judged.v_cache).all())
    judge("paged_attention scaled", f"chunk256 qpg{qpg} fp8", out, judged)
    # the same bytes without the scales are a different attention: the
    # judged reference is not satisfied by ignoring them
    plain = ext.paged_attention(*decode_args(judged, case), case.scale,
                                256).cpu()
    limit, _ = judged.limit()
    assert float(kc.row_rel_err(plain, judged.reference()).max()) > limit


# ---- 3. decode, split ----------------------------------------------------

@pytest.mark.parametrize("np_,part,chunk,qpg", [(3, 1024, 512, 2),
                                                (9, 256, 256, 4)])
def test_paged_attention_split_scaled(ext, np_, part, chunk, qpg):
    """The partials already carry v_scale; the combine kernel is the
    unscaled one."""
    case = kc.make_decode_case(qpg, kc.split_seqs(np_, part),
                               part_tokens=part, kv_dtype="fp8")
    judged = dequantised(case, K_SCALE, V_SCALE, rescale_q=True)
    out = ext.paged_attention_split(
        *decode_args(judged, case), np_, part, case.scale, chunk,
        f32(K_SCALE).cuda(), f32(V_SCALE).cuda()).cpu()
    judge("paged_attention_split scaled",
          f"np{np_} part{part} chunk{chunk} qpg{qpg} fp8", out, judged)


# ---- 4. decode, k_scale that is no power of two --------------------------

def test_paged_attention_scaled_non_power_of_two(ext):
    """q stays as it is, so the logits really are 0.7x and 1.9x the
    unscaled ones; diffuse rows only (needle=False)."""
    qpg = 4
    k_scale = [0.7, 1.9]
    case = kc.make_decode_case(qpg, kc.DECODE_SEQS, kv_dtype="fp8",
                               needle=False)
    judged = dequantised(case, k_scale, V_SCALE, rescale_q=False)
    out = ext.paged_attention(*decode_args(judged, case), case.scale, 256,
                              f32(k_scale).cuda(), f32(V_SCALE).cuda()).cpu()
    judge("paged_attention scaled", f"k_scale {k_scale} qpg{qpg} fp8", out,
          judged)


# ---- 5. prefill ----------------------------------------------------------

@pytest.mark.parametrize("qpg", [2, 4])
def test_flash_prefill_scaled(ext, qpg):
    """fp8 KV runs the convert-on-stage kernel."""
    case = kc.make_prefill_case(qpg, kv_dtype="fp8")
    judged = dequantised(case, K_SCALE, V_SCALE, rescale_q=True)
    i32 = dict(dtype=torch.int32, device="cuda")
    out = ext.flash_prefill(
        judged.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(),
        case.block_tables.cuda(), torch.tensor(case.metas, **i32),
        torch.tensor(case.tiles, **i32), case.scale,
        f32(K_SCALE).cuda(), f32(V_SCALE).cuda()).cpu()
    judge("flash_prefill scaled", f"qpg{qpg} fp8", out, judged)


# ---- 6. scales are legal only with an fp8 cache --------------------------

def test_scales_with_bf16_cache_raise(ext):
    case = kc.make_decode_case(2, [17, 40], kv_dtype="bf16", needle=False)
    ks, vs = f32(K_SCALE).cuda(), f32(V_SCALE).cuda()
    args = (case.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(),
            case.block_tables.cuda(),
            torch.tensor(case.seq_lens, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="fp8"):
        ext.paged_attention(*args, case.scale, 256, ks, vs)
    with pytest.raises(RuntimeError, match="fp8"):
        ext.paged_attention(*args, case.scale, 256, None, vs)
    with pytest.raises(RuntimeError, match="fp8"):
        ext.paged_attention_split(*args, 2, 256, case.scale, 256, ks, vs)
    pre = kc.make_prefill_case(2, seqs=[(5, 0)], kv_dtype="bf16",
                               needle=False)
    i32 = dict(dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="fp8"):
        ext.flash_prefill(pre.q.cuda(), pre.k_cache.cuda(),
                          pre.v_cache.cuda(), pre.block_tables.cuda(),
                          torch.tensor(pre.metas, **i32),
                          torch.tensor(pre.tiles, **i32), pre.scale, ks, vs)
    k_new = torch.zeros(1, 2, kc.D, dtype=torch.bfloat16, device="cuda")
    slots = torch.zeros(1, dtype=torch.int64, device="cuda")
    before = case.k_cache.clone()
    k_hip, v_hip = case.k_cache.cuda(), case.v_cache.cuda()
    with pytest.raises(RuntimeError, match="fp8"):
        ext.reshape_and_cache(k_new, k_new, k_hip, v_hip, slots, ks, vs)
    assert torch.equal(k_hip.cpu().view(torch.int16),
                       before.view(torch.int16))    # nothing was launched


def test_malformed_scales_raise(ext):
    case = kc.make_decode_case(2, [17, 40], kv_dtype="fp8", needle=False)
    args = (case.q.cuda(), case.k_cache.cuda(), case.v_cache.cuda(),
            case.block_tables.cuda(),
            torch.tensor(case.seq_lens, dtype=torch.int32, device="cuda"))
    good = f32(V_SCALE).cuda()
    for bad in (f32([1.0, 2.0, 3.0]).cuda(),              # numel != KVH
                f32(K_SCALE).double().cuda(),             # not float32
                f32(K_SCALE),                             # not on the GPU
                f32([1.0, 9.0, 2.0, 9.0]).cuda()[::2]):   # not contiguous
        with pytest.raises(RuntimeError):
            ext.paged_attention(*args, case.scale, 256, bad, good)


# ---- 7. / 8. engine ------------------------------------------------------

PROMPT_A = list(range(300, 430))      # 130 tokens: 8 blocks + 2, flash prefill
PROMPT_B = list(range(700, 730))      # 30 + 6 tokens: decode crosses slot 32


def engine_cfg():
    from llm_d_inference_scheduler_amd.models.configs import ModelConfig
    return ModelConfig(name="gpu-test", vocab_size=2048, hidden_size=1024,
                       intermediate_size=2048, num_layers=2, num_heads=8,
                       num_kv_heads=2, head_dim=128, rope_theta=10000.0)


def make_worker(rescaled):
    """Worker A, or worker B: the same weights with V projected 2048 times
    larger and divided out again in wo, Q 64 times larger and K 64 times
    smaller. All powers of two, so B is exactly the same function, and
    with k_scale = 1/64, v_scale = 2048 its stored bytes, logits and GEMM
    inputs are exact power-of-two images of A's."""
    from llm_d_inference_scheduler_amd.engine import EngineWorker
    cfg = engine_cfg()
    w = EngineWorker(cfg, "cuda:0", kv_blocks=256, dtype=torch.bfloat16,
                     kv_cache_dtype="fp8", seed=9)
    assert w.pool.tensor.dtype == kc.FP8 and w.pool.scales is None
    if rescaled:
        q, kv = cfg.q_size, cfg.kv_size
        for layer in w.model.layers:
            layer["wqkv"][:, :q] *= 64.0
            layer["wqkv"][:, q:q + kv] /= 64.0
            layer["wqkv"][:, q + kv:] *= 2048.0
            layer["wo"] /= 2048.0
    return w


def generate(w):
    from llm_d_inference_scheduler_amd.engine import EngineRequest
    w.add_request(EngineRequest("a", prompt_tokens=list(PROMPT_A),
                                max_tokens=6))
    w.add_request(EngineRequest("b", prompt_tokens=list(PROMPT_B),
                                max_tokens=6))
    toks = {"a": [], "b": []}
    for _ in range(40):
        for o in w.step():
            toks[o.request_id].extend(o.new_tokens)
        if not w.has_work:
            break
    assert not w.has_work
    assert len(toks["a"]) == 6 and len(toks["b"]) == 6
    return toks


def spy_on_scales(monkeypatch):
    """Records, per attention op, whether each call carried scales."""
    from llm_d_inference_scheduler_amd import ops
    seen = {"reshape_and_cache": [], "paged_attention": [],
            "flash_prefill": []}

    def wrap(name, keys):
        inner = getattr(ops, name)

        def spy(*a, **kw):
            seen[name].append(all(kw.get(k) is not None for k in keys))
            return inner(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    wrap("reshape_and_cache", ("k_inv_scale", "v_inv_scale"))
    wrap("paged_attention", ("k_scale", "v_scale"))
    wrap("flash_prefill", ("k_scale", "v_scale"))
    return seen


def test_engine_rescaled_model_exact(monkeypatch):
    toks_a = generate(make_worker(False))
    b = make_worker(True)
    b.set_kv_scales(k=1.0 / 64, v=2048.0)
    L, KVH = 2, 2
    assert b.pool.scales.shape == (L, 2, KVH)
    assert bool((b.pool.scales[:, 0] == 1.0 / 64).all())
    assert bool((b.pool.scales[:, 1] == 2048.0).all())
    assert bool((b.pool.inv_scales[:, 0] == 64.0).all())
    seen = spy_on_scales(monkeypatch)
    toks_b = generate(b)
    print(f"EDGE|engine rescaled|tokens|equal|A={toks_a} B={toks_b}")
    # the pool's scales reached the store, the prefill and the decode path
    for name, calls in seen.items():
        assert calls and all(calls), (name, calls)
    assert toks_b == toks_a
    # scales can only change on an idle, empty engine
    from llm_d_inference_scheduler_amd.engine import EngineRequest
    b.add_request(EngineRequest("c", prompt_tokens=list(PROMPT_B),
                                max_tokens=3))
    with pytest.raises(RuntimeError):
        b.set_kv_scales(k=1.0, v=1.0)


def test_engine_unscaled_worker_passes_no_scales(monkeypatch):
    seen = spy_on_scales(monkeypatch)
    generate(make_worker(False))
    for name, calls in seen.items():
        assert calls and not any(calls), (name, calls)


def test_engine_calibrate(tmp_path):
    a, b = make_worker(False), make_worker(True)
    a.calibrate_kv_scales()
    b.calibrate_kv_scales()
    sa, sb = a.pool.scales.cpu(), b.pool.scales.cpu()
    for s in (sa, sb):
        m, _ = torch.frexp(s)
        assert bool((m == 0.5).all()), s            # powers of two
    print(f"EDGE|calibrate|scales A|-|{sa.tolist()}")
    assert torch.equal(sb[:, 1], sa[:, 1] * 2048.0)
    assert torch.equal(sb[:, 0], sa[:, 0] / 64.0)
    assert a.pool.scales_id and b.pool.scales_id
    assert a.pool.scales_id != b.pool.scales_id
    assert generate(a) == generate(b)
    # calibration is deterministic, and a scales file reproduces it
    path = str(tmp_path / "scales.json")
    a2 = make_worker(False)
    a2.calibrate_kv_scales()
    assert a2.pool.scales_id == a.pool.scales_id
    a2.pool.save_scales(path)
    from llm_d_inference_scheduler_amd.engine import EngineWorker
    a3 = EngineWorker(engine_cfg(), "cuda:0", kv_blocks=256,
                      dtype=torch.bfloat16, kv_cache_dtype="fp8", seed=9,
                      kv_scales=path)
    assert a3.pool.scales_id == a.pool.scales_id
    assert torch.equal(a3.pool.scales.cpu(), sa)
