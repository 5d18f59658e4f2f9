"""Sampler on the CPU: the contract of DEVELOPMENT.md "Sampling" as ops.ref
implements it (Philox known answers, filters on hand-made rows, the drawn
distribution), the engine paths through it, the parsers and the HTTP API."""
import math

import pytest
import torch

import sampler_cases as sc
from llm_d_inference_scheduler_amd.datalayer.endpoint import Role
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.handlers.parsers import (OpenAIParser,
                                                            VertexAIParser)
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.ops import ref
from llm_d_inference_scheduler_amd import ops


# ---- Philox ----------------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF),
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344],
     (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    out = ref.philox4x32_10(torch.tensor([ctr], dtype=torch.int64), key)[0]
    assert " ".join("%08x" % int(v) for v in out) == want


def test_gumbel_noise_is_finite_and_bounded():
    """u never reaches 1 (x >> 8 = 2^24 - 1 would round there in fp32), so
    g stays finite and under about 17."""
    g = ref.gumbel_noise(torch.arange(1 << 16), seed=3, pos=0)
    assert torch.isfinite(g).all() and float(g.max()) < 17.0
    u = torch.tensor([(1 << 24) - 1], dtype=torch.float32) + 0.5
    assert float(u * 2.0 ** -24) == 1.0        # why the contract clamps


# ---- contract on hand-made rows ---------------------------------------------

def run1(row, T=1.0, k=0, p=1.0, seed=1, pos=0, dtype=torch.float32):
    out = ref.sample(torch.tensor([row], dtype=dtype),
                     torch.tensor([T]), torch.tensor([k], dtype=torch.int32),
                     torch.tensor([p]), torch.tensor([seed]),
                     torch.tensor([pos], dtype=torch.int32))
    return int(out[0][0]), float(out[1][0]), int(out[2][0]), float(out[3][0])


def test_top_k_ties_at_boundary_all_kept():
    tok, _, nk, th = run1([5.0, 3.0, 3.0, 3.0, 1.0, 0.0], k=2)
    assert nk == 4 and th == 3.0 and tok in (0, 1, 2, 3)


def test_top_k_at_least_v_is_off():
    for k in (6, 7, 1000):
        _, _, nk, th = run1([5.0, 3.0, 3.0, 3.0, 1.0, 0.0], k=k)
        assert nk == 6 and th == float("-inf")


def test_top_p_one_is_off():
    _, _, nk, th = run1([5.0, 3.0, 1.0], p=1.0)
    assert nk == 3 and th == float("-inf")


def test_tiny_top_p_keeps_only_the_maximum():
    tok, _, nk, th = run1([1.0, 5.0, 3.0, 4.5], p=1e-6)
    assert (tok, nk, th) == (1, 1, 5.0)


def test_top_p_after_top_k_targets_p_times_w():
    """Weights 8 : 4 : 2 : 1 : 1 (logits ln 8 ... 0). top_k=2 keeps 8 and 4,
    W = 12/16 of the row. p = 0.7: p*W = 8.4/16 > 8/16, so both stay. Were
    the target p of the whole row (11.2/16) the answer would be the same,
    so also p = 0.6: p*W = 7.2/16 <= 8/16 keeps one, while 0.6 of the whole
    row (9.6/16) would keep two."""
    row = [math.log(8), math.log(4), math.log(2), 0.0, 0.0]
    assert run1(row, k=2, p=0.7)[2] == 2
    assert run1(row, k=2, p=0.6)[2] == 1
    assert run1(row, k=0, p=0.6)[2] == 2
    # temperature scales z before the filters: T=0.5 squares the weights
    assert run1(row, T=0.5, k=0, p=0.6)[2] == 1


def test_threshold_is_scaled_back_to_a_raw_logit():
    _, _, nk, th = run1([4.0, 2.0, 1.0, -3.0], T=0.5, k=2)
    assert nk == 2 and th == 2.0


def test_greedy_tied_maximum_returns_lowest_index():
    for T in (0.0, -1.0):
        tok, lp, nk, th = run1([1.0, 7.0, 7.0, 2.0, 7.0], T=T, k=1, p=0.1)
        assert (tok, nk, th) == (1, 5, float("-inf"))
        want = torch.log_softmax(torch.tensor([1.0, 7, 7, 2, 7]).double(), 0)
        assert abs(lp - float(want[1])) < 1e-6


def test_top_k_1_equals_argmax_on_random_rows():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(200, 333, generator=g) * 4
    B = logits.shape[0]
    tok, lp, nk, _ = ref.sample(
        logits, torch.full((B,), 5.0), torch.ones(B, dtype=torch.int32),
        torch.ones(B), torch.arange(B), torch.zeros(B, dtype=torch.int32))
    assert torch.equal(tok, logits.argmax(dim=-1))
    assert (nk == 1).all()
    want = torch.log_softmax(logits.double(), -1).gather(
        1, tok.unsqueeze(1)).squeeze(1)
    assert float((lp.double() - want).abs().max()) < 1e-5


def test_draw_does_not_depend_on_batch_position():
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(7, 500, generator=g) * 4).bfloat16()
    args = (torch.full((7,), 0.8), torch.full((7,), 40, dtype=torch.int32),
            torch.full((7,), 0.9), torch.arange(7) + 100,
            torch.arange(7, dtype=torch.int32))
    full = ref.sample(logits, *args)
    one = ref.sample(logits[6:7], *(a[6:7] for a in args))
    for a, b in zip(full, one):
        assert torch.equal(a[6:7], b)


# ---- distribution -------------------------------------------------------------

def chi2_quantile(q_upper_tail: float, df: int) -> float:
    """Upper-tail quantile of chi-square(df)."""
    try:
        from scipy import stats
        return float(stats.chi2.isf(q_upper_tail, df))
    except ImportError:
        # Wilson-Hilferty, with the normal quantile from erfc by bisection
        lo, hi = 0.0, 10.0
        for _ in range(80):
            mid = (lo + hi) / 2
            if 0.5 * math.erfc(mid / math.sqrt(2)) > q_upper_tail:
                lo = mid
            else:
                hi = mid
        z = (lo + hi) / 2
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def test_distribution_matches_renormalised_kept_set():
    V, N, T = 64, 20000, 0.7
    g = torch.Generator().manual_seed(7)
    row = torch.randn(V, generator=g) * 2
    logits = row.unsqueeze(0).expand(N, V).contiguous()
    tok, _, nk, th = ref.sample(
        logits, torch.full((N,), T), torch.full((N,), 8, dtype=torch.int32),
        torch.full((N,), 0.9), torch.full((N,), 99),
        torch.arange(N, dtype=torch.int32))
    n_kept = int(nk[0])
    assert (nk == n_kept).all() and 1 < n_kept <= 8
    # threshold is tau * T in fp32: the boundary logit up to two roundings
    boundary = row.topk(n_kept).values[-1]
    assert abs(float(th[0]) - float(boundary)) <= 4e-7 * abs(float(boundary))
    kept = row >= boundary
    assert int(kept.sum()) == n_kept
    assert kept[tok].all()                      # nothing outside the kept set
    probs = torch.softmax(row.double() / T, 0) * kept
    probs = probs / probs.sum()
    counts = torch.bincount(tok, minlength=V).double()
    idx = kept.nonzero().squeeze(1)
    chi2 = float((((counts - N * probs) ** 2)[idx] / (N * probs[idx])).sum())
    limit = chi2_quantile(1e-6, n_kept - 1)
    print(f"chi2={chi2:.2f} limit={limit:.2f} df={n_kept - 1}")
    assert chi2 < limit


@pytest.mark.parametrize("V,B,dtype,gen_seed", sc.SHAPES)
def test_case_seeds_leave_rows_decided(V, B, dtype, gen_seed):
    """The GPU tier skips rows that fp32 rounding decides; with these
    generator seeds the reference names none (limit: 2%)."""
    share = sc.undecided_share(sc.make_case(V, B, dtype, gen_seed))
    print(f"UNDECIDED|sample|V{V}_B{B}|{share:.4f}")
    assert share <= sc.MAX_UNDECIDED_SHARE


def test_reference_is_fast_at_the_real_vocabulary():
    L = sc.make_case(151936, 2, torch.bfloat16, 14)[0]
    assert L.tokens.shape == (2,)


# ---- engine ---------------------------------------------------------------------

PROMPT = list(range(50, 90))


def make_worker(**kw):
    kw.setdefault("kv_blocks", 128)
    kw.setdefault("dtype", torch.float32)
    kw.setdefault("seed", 3)
    return EngineWorker(TINY_LLAMA, "cpu", **kw)


def run_to_completion(worker, max_steps=200):
    outs = []
    for _ in range(max_steps):
        outs.extend(worker.step())
        if not worker.has_work:
            break
    return outs


def generate(worker=None, others=(), **kw):
    w = worker or make_worker()
    kw.setdefault("max_tokens", 8)
    w.add_request(EngineRequest("r", prompt_tokens=PROMPT, **kw))
    for o in others:
        w.add_request(o)
    outs = run_to_completion(w)
    return [o for o in outs if o.finished and o.request_id == "r"][0]


SEEDED = dict(temperature=1.0, top_p=0.9, seed=7)


@pytest.fixture(scope="module")
def seeded_tokens():
    return generate(**SEEDED).all_tokens


@pytest.fixture(scope="module")
def greedy_tokens():
    return generate().all_tokens


def test_engine_same_seed_same_tokens(seeded_tokens, greedy_tokens):
    assert generate(**SEEDED).all_tokens == seeded_tokens
    assert len(seeded_tokens) == 8 and seeded_tokens != greedy_tokens
    # nothing here touches the global torch RNG
    torch.manual_seed(12345)
    assert generate(**SEEDED).all_tokens == seeded_tokens


def test_engine_other_seed_other_tokens(seeded_tokens):
    assert generate(**dict(SEEDED, seed=8)).all_tokens != seeded_tokens


def test_engine_top_k_1_reproduces_greedy(greedy_tokens):
    assert generate(temperature=2.0, top_k=1).all_tokens == greedy_tokens


def test_engine_seeded_request_ignores_its_neighbours(seeded_tokens):
    others = [EngineRequest(f"g{i}", prompt_tokens=list(range(10 + i, 45)),
                            max_tokens=8) for i in range(3)]
    assert generate(others=others, **SEEDED).all_tokens == seeded_tokens


def test_engine_unseeded_requests_follow_the_worker_seed():
    a = generate(make_worker(seed=3), temperature=1.0, top_k=50).all_tokens
    b = generate(make_worker(seed=3), temperature=1.0, top_k=50).all_tokens
    c = generate(make_worker(seed=3, kv_blocks=127), temperature=1.0,
                 top_k=50).all_tokens
    assert a == b == c


def test_engine_logprobs(monkeypatch):
    """One finite value <= 0 per token, equal to log_softmax of the logits
    that token was sampled from. Bound: the fp32 logsumexp of 1024 terms,
    about 1024 * 2^-24 relative on a sum, far inside 1e-4."""
    seen = []
    real = ops.sample

    def spy(logits, *a):
        out = real(logits, *a)
        seen.append((logits.double(), out[0]))
        return out

    monkeypatch.setattr(ops, "sample", spy)
    w = make_worker()
    w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=6,
                                temperature=0.8, top_k=20, logprobs=True))
    outs = run_to_completion(w)
    fin = [o for o in outs if o.finished][0]
    assert len(fin.all_logprobs) == len(fin.all_tokens) == 6
    assert all(math.isfinite(v) and v <= 0 for v in fin.all_logprobs)
    per_step = [lp for o in outs for lp in (o.new_logprobs or [])]
    assert per_step == fin.all_logprobs
    assert len(seen) == 6
    for (lg, tk), tok, lp in zip(seen, fin.all_tokens, fin.all_logprobs):
        assert int(tk[0]) == tok
        assert abs(float(torch.log_softmax(lg[0], -1)[tok]) - lp) < 1e-4


def test_engine_without_logprobs_returns_none():
    fin = generate(**SEEDED)
    assert fin.all_logprobs is None


def test_engine_greedy_step_skips_the_fused_op(monkeypatch, greedy_tokens):
    calls = []
    real = ops.sample
    monkeypatch.setattr(ops, "sample",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    assert generate().all_tokens == greedy_tokens
    generate(temperature=0.7)
    assert not calls
    generate(temperature=0.7, top_p=0.95)
    assert calls


def test_engine_preempted_seeded_request_resumes(seeded_tokens):
    w = make_worker()
    req = EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8, **SEEDED)
    w.add_request(req)
    outs = []
    for _ in range(4):
        outs.extend(w.step())
    outs.extend(w._collect_pending())
    assert 0 < len(req.generated) < 8 and req.inflight == 0
    assert w._preempt(req) is None and req in w.waiting
    outs.extend(run_to_completion(w))
    fin = [o for o in outs if o.finished][0]
    assert fin.all_tokens == seeded_tokens


def test_engine_seeded_handoff_matches_monolithic(seeded_tokens):
    pre = make_worker(role=Role.PREFILL)
    dec = make_worker(role=Role.DECODE)
    pre.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                  prefill_only=True, **SEEDED))
    pd = [o for o in run_to_completion(pre, max_steps=5)
          if o.kind == "prefill_done"][0]
    dst_blocks = dec.mgr.take_blocks(len(pd.kv_blocks))
    dec.pool.tensor[:, :, torch.tensor(dst_blocks)] = \
        pre.pool.tensor[:, :, torch.tensor(pd.kv_blocks)]
    dec.admit_transferred(
        EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8, **SEEDED),
        dst_blocks, pd.seq_len, pd.first_token)
    toks = [pd.first_token] + \
        [t for o in run_to_completion(dec) for t in o.new_tokens]
    assert toks == seeded_tokens


# ---- parsers and API --------------------------------------------------------------

def parse(body, parser=None):
    import json
    return (parser or OpenAIParser()).parse_request(
        json.dumps(body).encode(), {}, "/v1/completions")


def test_openai_parser_reads_sampler_fields():
    r = parse({"model": "m", "prompt": "x", "temperature": 0.7,
               "top_p": 0.9, "top_k": 40, "seed": 2 ** 63 + 5,
               "logprobs": True}).request
    assert (r.top_p, r.top_k, r.seed, r.logprobs) == (0.9, 40, 2 ** 63 + 5,
                                                      True)
    r = parse({"model": "m", "prompt": "x"}).request
    assert (r.top_p, r.top_k, r.seed, r.logprobs) == (1.0, 0, None, False)
    for off in (-1, 0):
        assert parse({"model": "m", "prompt": "x",
                      "top_k": off}).request.top_k == 0
    assert parse({"model": "m", "prompt": "x",
                  "logprobs": 1}).request.logprobs is True
    assert parse({"model": "m", "prompt": "x",
                  "logprobs": False}).request.logprobs is False


@pytest.mark.parametrize("field,value", [
    ("top_p", 0), ("top_p", -0.1), ("top_p", 1.5), ("top_p", "0.5"),
    ("top_k", -2), ("top_k", 1.5), ("seed", -1), ("seed", 1.5),
    ("seed", "7"), ("logprobs", -1),
])
def test_openai_parser_rejects_out_of_range(field, value):
    res = parse({"model": "m", "prompt": "x", field: value})
    assert res.request is None and res.error and field in res.error


def test_generation_config_parser_reads_sampler_fields():
    body = {"model": "m", "contents": [{"parts": [{"text": "hi"}]}],
            "generationConfig": {"topP": 0.8, "topK": 5, "seed": 11}}
    r = parse(body, VertexAIParser()).request
    assert (r.top_p, r.top_k, r.seed) == (0.8, 5, 11)
    body["generationConfig"]["topP"] = 2
    assert "topP" in parse(body, VertexAIParser()).error


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient
    from llm_d_inference_scheduler_amd.node import NodeConfig, NodeRunner
    from llm_d_inference_scheduler_amd.server import NodeService, build_app
    cfg = NodeConfig(model=TINY_LLAMA, world_size=1, topology="mono",
                     device="cpu", dtype=torch.float32, kv_blocks=256)
    service = NodeService(NodeRunner(cfg))
    service.start()
    with TestClient(build_app(service)) as c:
        yield c
    service.stop()


def test_api_completions_logprobs(client):
    body = {"model": "tiny-llama", "prompt": "hello world test prompt",
            "max_tokens": 5, "temperature": 0.8, "top_p": 0.9, "seed": 3,
            "logprobs": 1}
    r = client.post("/v1/completions", json=body)
    assert r.status_code == 200, r.text
    out = r.json()
    lp = out["choices"][0]["logprobs"]
    n = out["usage"]["completion_tokens"]
    assert n == 5 and len(lp["token_logprobs"]) == len(lp["tokens"]) == n
    assert all(v <= 0 for v in lp["token_logprobs"])
    again = client.post("/v1/completions", json=body).json()
    assert again["choices"][0]["text"] == out["choices"][0]["text"]
    assert again["choices"][0]["logprobs"] == lp
    plain = client.post("/v1/completions", json={
        "model": "tiny-llama", "prompt": "hello", "max_tokens": 2}).json()
    assert "logprobs" not in plain["choices"][0]


def test_api_chat_logprobs_and_validation(client):
    r = client.post("/v1/chat/completions", json={
        "model": "tiny-llama", "max_tokens": 3, "logprobs": True,
        "messages": [{"role": "user", "content": "hi there"}]})
    assert r.status_code == 200, r.text
    content = r.json()["choices"][0]["logprobs"]["content"]
    assert len(content) == 3
    assert all(set(c) == {"token", "logprob"} for c in content)
    bad = client.post("/v1/completions", json={
        "model": "tiny-llama", "prompt": "x", "top_p": 1.5})
    assert bad.status_code == 400
