"""GPU tier of the sampler tests: the fused HIP sampler against ops.ref.sample
(exact tokens and kept-set sizes, bit-equal thresholds), its logprob against
float64, and the engine paths that route through it (DEVELOPMENT.md
"Sampling"; inputs in tests/sampler_cases.py).

Prints one `EDGE|sample|<case>|limit|worst` line per shape for the logprob
and one `UNDECIDED|sample|<case>|share` line before asserting (pytest -s)."""
import pytest
import torch

import sampler_cases as sc

pytestmark = pytest.mark.gpu

LOGPROB_LIMIT = 1e-4


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def case_name(V, B, dtype):
    return f"V{V}_B{B}_{'bf16' if dtype == torch.bfloat16 else 'f32'}"


@pytest.mark.parametrize("V,B,dtype,gen_seed", sc.SHAPES)
def test_matches_reference(ext, V, B, dtype, gen_seed):
    launches = sc.make_case(V, B, dtype, gen_seed)
    name = case_name(V, B, dtype)
    share = sc.undecided_share(launches)
    print(f"UNDECIDED|sample|{name}|{share:.4f}")
    assert share <= sc.MAX_UNDECIDED_SHARE
    worst_lp = 0.0
    for li, L in enumerate(launches):
        tok, lp, nk, th = (t.cpu() for t in ext.sample(*L.args("cuda")))
        # logprob of the token the kernel chose, against float64
        want = torch.log_softmax(L.logits.double(), dim=-1).gather(
            1, tok.unsqueeze(1)).squeeze(1)
        assert torch.isfinite(lp).all()
        worst_lp = max(worst_lp, float((lp.double() - want).abs().max()))
        for r in range(B):
            where = (name, li, r, float(L.temperature[r]), int(L.top_k[r]),
                     float(L.top_p[r]))
            if L.kept_undecided[r]:
                continue
            assert int(nk[r]) == int(L.n_kept[r]), where
            # bit-equal, -inf included
            assert th[r].view(torch.int32) == \
                L.threshold[r].view(torch.int32), where
            if not L.token_undecided[r]:
                assert int(tok[r]) == int(L.tokens[r]), where
    print(f"EDGE|sample|{name}|{LOGPROB_LIMIT:.3e}|{worst_lp:.3e}")
    assert worst_lp <= LOGPROB_LIMIT


def test_position_independence(ext):
    """The same row alone and at index 6 of a batch of 7."""
    g = torch.Generator().manual_seed(21)
    V = 1001
    logits = (torch.randn(7, V, generator=g) * 4).bfloat16()
    T = torch.full((7,), 0.8)
    k = torch.full((7,), 40, dtype=torch.int32)
    p = torch.full((7,), 0.9)
    seed = torch.arange(7, dtype=torch.int64) + 100
    pos = torch.arange(7, dtype=torch.int32)
    full = ext.sample(*(t.cuda() for t in (logits, T, k, p, seed, pos)))
    one = ext.sample(*(t[6:7].contiguous().cuda()
                       for t in (logits, T, k, p, seed, pos)))
    for a, b in zip(full, one):
        assert torch.equal(a[6:7].cpu(), b.cpu())


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_poisoned_padding(ext, poison):
    """Rows around the sampled ones hold +inf or NaN: no row may read past
    its own V elements. V is odd, so the middle rows start misaligned."""
    L = sc.make_case(1001, 3, torch.bfloat16, 11)[1]
    B, V = L.logits.shape
    buf = torch.full((B + 2, V), poison, dtype=L.logits.dtype, device="cuda")
    buf[1:B + 1] = L.logits.cuda()
    args = L.args("cuda")
    clean = ext.sample(*args)
    got = ext.sample(buf[1:B + 1], *args[1:])
    for a, b in zip(clean, got):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32
                           else a, b.view(torch.int32)
                           if b.dtype == torch.float32 else b)


def test_binding_checks(ext):
    lg = torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")
    T = torch.ones(2, device="cuda")
    k = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = torch.ones(2, device="cuda")
    s = torch.zeros(2, dtype=torch.int64, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    ext.sample(lg, T, k, p, s, n)
    with pytest.raises(RuntimeError):
        ext.sample(lg.half(), T, k, p, s, n)            # dtype
    with pytest.raises(RuntimeError):
        ext.sample(lg.t().contiguous().t(), T, k, p, s, n)   # contiguity
    with pytest.raises(RuntimeError):
        ext.sample(lg, T[:1], k, p, s, n)               # length
    with pytest.raises(RuntimeError):
        ext.sample(lg, T, k.long(), p, s, n)            # parameter dtype
    with pytest.raises(RuntimeError):
        ext.sample(lg, T.cpu(), k, p, s, n)             # device


# ---- engine on the GPU ----------------------------------------------------
# tiny-llama's head_dim of 32 is outside what the attention kernels take
# (128), so the engine runs the small GPU config of tests/test_gpu_kernels.py.

def _cfg():
    from llm_d_inference_scheduler_amd.models.configs import ModelConfig
    return ModelConfig(name="gpu-test", vocab_size=2048, hidden_size=1024,
                       intermediate_size=2048, num_layers=2, num_heads=8,
                       num_kv_heads=2, head_dim=128, rope_theta=10000.0)


def _generate(**req_kw):
    from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                      EngineWorker)
    w = EngineWorker(_cfg(), "cuda:0", kv_blocks=256, dtype=torch.bfloat16,
                     seed=9)
    w.add_request(EngineRequest("a", prompt_tokens=list(range(300, 430)),
                                max_tokens=6, **req_kw))
    outs = []
    for _ in range(64):
        outs.extend(w.step())
        if not w.has_work:
            break
    fin = [o for o in outs if o.finished]
    assert len(fin) == 1
    return fin[0]


@pytest.fixture(scope="module")
def greedy_tokens():
    return _generate().all_tokens


def test_engine_seeded_repeats(greedy_tokens):
    a = _generate(temperature=1.0, top_p=0.9, seed=1234, logprobs=True)
    b = _generate(temperature=1.0, top_p=0.9, seed=1234, logprobs=True)
    assert a.all_tokens == b.all_tokens and len(a.all_tokens) == 6
    assert a.all_logprobs == b.all_logprobs
    assert len(a.all_logprobs) == 6
    assert all(lp <= 0 and lp == lp for lp in a.all_logprobs)


def test_engine_top_k_1_is_greedy(greedy_tokens, monkeypatch):
    """temperature=2, top_k=1 reproduces the greedy generation. The random
    bf16 model's logits tie at the maximum now and then (measured: step 3 of
    this prompt); the contract keeps every tied token, so from such a step
    on only `the token attains the row maximum` can be asked. Every step
    before it must equal the greedy token."""
    from llm_d_inference_scheduler_amd import ops
    seen = []
    real = ops.sample

    def spy(logits, *a):
        out = real(logits, *a)
        seen.append((logits.float().cpu(), out[0].cpu()))
        return out

    monkeypatch.setattr(ops, "sample", spy)
    toks = _generate(temperature=2.0, top_k=1).all_tokens
    assert len(seen) == len(toks) == len(greedy_tokens)
    compared = 0
    for (lg, tk), tok, want in zip(seen, toks, greedy_tokens):
        assert int(tk[0]) == tok
        assert float(lg[0, tok]) == float(lg[0].max())
        if int((lg[0] == lg[0].max()).sum()) > 1:
            break
        assert tok == want
        compared += 1
    assert compared >= 1


def test_engine_greedy_skips_fused_op(greedy_tokens, monkeypatch):
    from llm_d_inference_scheduler_amd import ops
    calls = []
    real = ops.sample
    monkeypatch.setattr(ops, "sample",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    assert _generate().all_tokens == greedy_tokens
    assert not calls
    _generate(temperature=1.0, seed=5)
    assert calls
