"""sample_ext on the CPU: step 0 of the contract (DEVELOPMENT.md "Sampling")
against an independent dense formulation, equality with sample() when every
new input is off, mutants of the reference that named cases must reject, the
engine's token state, the parsers and the HTTP API."""
import json
import math
from collections import Counter

import pytest
import torch

import sampler_cases as sc
import sampler_ext_cases as xc
from llm_d_inference_scheduler_amd import ops
from llm_d_inference_scheduler_amd.datalayer.endpoint import Role
from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.handlers.parsers import OpenAIParser
from llm_d_inference_scheduler_amd.models.configs import TINY_LLAMA
from llm_d_inference_scheduler_amd.ops import ref

MASK, PBIT = ref.STATE_COUNT_MASK, ref.STATE_PROMPT_BIT


# ---- the cases -------------------------------------------------------------

@pytest.mark.parametrize("V,B,dtype,gen_seed", xc.SHAPES)
def test_case_seeds_leave_rows_decided(V, B, dtype, gen_seed):
    share = xc.undecided_share(xc.make_case(V, B, dtype, gen_seed))
    print(f"UNDECIDED|sample_ext|V{V}_B{B}|{share:.4f}")
    assert share == 0.0 <= xc.MAX_UNDECIDED_SHARE


def test_small_cases_cross_every_pair_of_values():
    for V in (100, 1001, 1024):
        plan = xc.row_plan(V, 0)
        assert {p[3:8] for p in plan} == set(xc.NEW_COMBOS)
        for j in range(3, 8):
            assert {(p[j], p[:3]) for p in plan} >= {
                (v, c) for v in {q[j] for q in plan} for c in sc.COMBOS}
            assert {(p[j], p[8]) for p in plan} >= {
                (v, h) for v in {q[j] for q in plan} for h in xc.HISTORIES}


def test_cases_exercise_what_they_claim():
    """Greedy flips on argmax-history rows with a penalty on, min_p decides
    thresholds, top-N rows tie at the cut."""
    flips = minp = ties = 0
    for L in xc.make_case(*xc.SHAPES[1]):
        for r, p in enumerate(L.plan):
            T, rep, freq, pres, hist = p[0], p[3], p[4], p[5], p[8]
            raw_arg = int(L.logits[r].float().argmax())
            if T == 0 and hist == "argmax" and int(L.tokens[r]) != raw_arg:
                flips += 1
            if math.isfinite(L.details[r]["minp_margin"]) and T > 0:
                minp += 1
            n = int(L.top_n[r])
            if n and n < 1001:
                v = L.logits[r].float()
                cut = v[L.top_tokens[r, n - 1]]
                if int((v == cut).sum()) > int(
                        (v[L.top_tokens[r, :n]] == cut).sum()):
                    ties += 1
    assert flips >= 3 and minp >= 20 and ties >= 5


# ---- step 0 against a dense formulation ---------------------------------------

def dense_step0(l, prompt, out, rep, pres, freq):
    """vLLM's formulation: masks and counts as dense tensors."""
    V = l.shape[0]
    cnt = torch.zeros(V)
    for t in out:
        cnt[t] += 1
    seen = cnt > 0
    for t in prompt:
        seen[t] = True
    x = l.clone()
    pen = torch.where(seen, torch.tensor(rep), torch.tensor(1.0))
    x = torch.where(x > 0, x / pen, x * pen)
    x = x - torch.tensor(freq) * cnt
    x = x - torch.tensor(pres) * (cnt > 0).float()
    return x


def test_step0_matches_the_dense_formulation():
    model = ref.SamplerExtModel()
    for L in xc.make_case(*xc.SHAPES[2])[:20]:
        for r, p in enumerate(L.plan):
            sr = int(L.state_row[r])
            if sr < 0:
                continue
            V = L.logits.shape[1]
            s = L.state_before[sr, :V].to(torch.int32)
            got = model.penalise(L.logits[r].float(), s, p[3], p[5], p[4])
            want = dense_step0(L.logits[r].float(), *L.histories[r],
                               p[3], p[5], p[4])
            # pres * 1.0 and pres are the same fp32 number; so are x / 1, x
            assert torch.equal(got, want), (r, p)


def test_all_off_equals_sample_exactly():
    for shape in sc.SHAPES[:4]:
        V, B = shape[0], shape[1]
        state = torch.randint(0, 0x7FFF, (B, (V + 7) // 8 * 8),
                              dtype=torch.int16)
        for L in sc.make_case(*shape)[:6]:
            a = (L.logits, L.temperature, L.top_k, L.top_p, L.seed, L.pos)
            off = (torch.ones(B), torch.zeros(B), torch.zeros(B),
                   torch.zeros(B), torch.zeros(B, dtype=torch.int32))
            for srow in (torch.full((B,), -1, dtype=torch.int32),
                         torch.arange(B, dtype=torch.int32)):
                got = ref.sample_ext(*a, *off, srow, state.clone(), 0)
                for g, w in zip(got[:4], (L.tokens, L.logprobs, L.n_kept,
                                          L.threshold)):
                    assert torch.equal(g, w)


# ---- mutants -------------------------------------------------------------------

def one(model, row, state=None, T=0.0, rep=1.0, pres=0.0, freq=0.0,
        min_p=0.0, top_n=0):
    """One fp32 row through model.sample_ext -> (token, n_kept, threshold,
    top tokens, state row after). state: {token: state element}."""
    V = len(row)
    st = ref.token_state_alloc(1, V, "cpu")
    for t, s in (state or {}).items():
        st[0, t] = s
    out = model.sample_ext(
        torch.tensor([row]), torch.tensor([T]),
        torch.zeros(1, dtype=torch.int32), torch.ones(1),
        torch.tensor([5]), torch.zeros(1, dtype=torch.int32),
        torch.tensor([rep]), torch.tensor([pres]), torch.tensor([freq]),
        torch.tensor([min_p]), torch.tensor([top_n], dtype=torch.int32),
        torch.zeros(1, dtype=torch.int32), st, top_n)
    return (int(out[0][0]), int(out[2][0]), float(out[3][0]),
            out[4][0].tolist(), st[0, :V].tolist())


class RepPromptOnly(ref.SamplerExtModel):
    def rep_mask(self, s):
        return (s & PBIT) != 0


class NegativesDivided(ref.SamplerExtModel):
    def rep_apply(self, x, rep):
        return x / rep


class PresenceOnPrompt(ref.SamplerExtModel):
    def pres_mask(self, s):
        return s != 0


class FrequencyAsFlag(ref.SamplerExtModel):
    def freq_count(self, s):
        return ((s & MASK) > 0).to(torch.float32)


class MinPFromRawMax(ref.SamplerExtModel):
    def minp_base(self, z, z_raw):
        return z_raw.max()


class TopNFromPenalised(ref.SamplerExtModel):
    def topn_values(self, l, x):
        return x


class TopNTiesHighest(ref.SamplerExtModel):
    def topn_pick(self, v, n):
        V = v.shape[0]
        return V - 1 - torch.argsort(v.flip(0), descending=True,
                                     stable=True)[:n]


class StateNotUpdated(ref.SamplerExtModel):
    def update_state(self, row, tok):
        pass


class SaturationCarries(ref.SamplerExtModel):
    def bump(self, s):
        return s + 1


# name -> (mutant, kwargs of one(), what the contract gives)
MUTANT_CASES = {
    "repetition_hits_output_only_tokens": (
        RepPromptOnly, dict(row=[2.0, 1.9], state={0: 1}, rep=2.0),
        lambda o: o[0] == 1),
    "repetition_multiplies_negatives": (
        NegativesDivided, dict(row=[-1.0, -1.5], state={0: PBIT}, rep=2.0),
        lambda o: o[0] == 1),
    "presence_ignores_prompt_only_tokens": (
        PresenceOnPrompt, dict(row=[2.0, 1.9], state={0: PBIT}, pres=1.0),
        lambda o: o[0] == 0),
    "frequency_scales_with_the_count": (
        FrequencyAsFlag, dict(row=[3.0, 1.9], state={0: 3}, freq=0.5),
        lambda o: o[0] == 1),
    "min_p_measured_from_the_penalised_maximum": (
        MinPFromRawMax, dict(row=[2.5, 2.0, 1.0], state={0: 1}, freq=1.0,
                             T=1.0, min_p=0.5),
        lambda o: o[1] == 2),
    "top_n_from_raw_logits": (
        TopNFromPenalised, dict(row=[3.0, 2.0, 1.0], state={0: 9}, freq=1.0,
                                top_n=2),
        lambda o: o[3] == [0, 1]),
    "top_n_ties_by_lowest_index": (
        TopNTiesHighest, dict(row=[1.0, 1.0, 1.0, 0.0], top_n=2),
        lambda o: o[3] == [0, 1]),
    "state_counts_the_drawn_token": (
        StateNotUpdated, dict(row=[1.0, 2.0], state={1: PBIT + 4}),
        lambda o: o[4] == [0, PBIT + 5]),
    "saturation_stops_below_bit_14": (
        SaturationCarries, dict(row=[1.0, 2.0], state={1: MASK}),
        lambda o: o[4] == [0, MASK]),
}


@pytest.mark.parametrize("name", sorted(MUTANT_CASES))
def test_named_case_rejects_its_mutant(name):
    mutant, kw, holds = MUTANT_CASES[name]
    good = one(ref.SamplerExtModel(), **kw)
    bad = one(mutant(), **kw)
    assert holds(good), good
    assert not holds(bad) and bad != good, bad


def test_fill_saturation_mutant_is_rejected():
    V = 16
    args = (torch.tensor([0], dtype=torch.int32),
            torch.tensor([3] + [4] * 16400, dtype=torch.int32),
            torch.tensor([0, 16401]), torch.tensor([1], dtype=torch.int32), V)
    good = ref.token_state_alloc(1, V, "cpu")
    ref.token_state_fill(good, *args)
    assert good[0].tolist() == [0, 0, 0, PBIT, MASK] + [0] * 11
    bad = ref.token_state_alloc(1, V, "cpu")
    SaturationCarries().token_state_fill(bad, *args)
    assert not torch.equal(good, bad)


def test_token_state_layout():
    st = ops.token_state_alloc(3, 1001, "cpu")
    assert st.shape == (3, 1008) and st.dtype == torch.int16
    assert st.stride(0) * 2 % 16 == 0 and int(st.abs().sum()) == 0


def test_top_n_is_independent_of_everything_else():
    L = xc.make_case(*xc.SHAPES[0])[5]
    for r in range(3):
        n = int(L.top_n[r])
        v = L.logits[r].float()
        order = sorted(range(100), key=lambda i: (-float(v[i]), i))[:n]
        assert L.top_tokens[r, :n].tolist() == order
        assert (L.top_tokens[r, n:] == -1).all()
        want = torch.log_softmax(v.double(), 0)[order]
        assert float((L.top_logprobs[r, :n].double() - want).abs().max()
                     if n else 0.0) < 1e-5


# ---- engine ---------------------------------------------------------------------

PROMPT = list(range(50, 90)) + [60, 61]
PENALISED = dict(temperature=0.8, seed=7, repetition_penalty=1.3,
                 frequency_penalty=0.5, presence_penalty=0.2,
                 top_logprobs=3, logprobs=True)


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


def decode_row(row):
    """state row -> (set of prompt tokens, Counter of output tokens)."""
    r = row.to(torch.int32)
    prompt = set(torch.nonzero(r & PBIT).squeeze(1).tolist())
    cnt = Counter({int(i): int(r[i] & MASK)
                   for i in torch.nonzero(r & MASK).squeeze(1)})
    return prompt, cnt


@pytest.fixture
def recorded(monkeypatch):
    """ops.sample_ext wrapped: the first row's decoded state row, as it is
    before each call."""
    seen = []
    real = ops.sample_ext

    def spy(*a):
        state_row, state = a[11], a[12]
        assert len(set(state_row.tolist())) == len(state_row)
        seen.append(decode_row(state[int(state_row[0]), :a[0].shape[1]]))
        return real(*a)

    monkeypatch.setattr(ops, "sample_ext", spy)
    return seen


def check_recorded(seen, tokens):
    assert len(seen) == len(tokens)
    for j, (prompt, cnt) in enumerate(seen):
        assert prompt == set(PROMPT), j
        assert cnt == Counter(tokens[:j]), j


@pytest.fixture(scope="module")
def penalised_tokens():
    w = make_worker()
    w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                **PENALISED))
    return [o for o in run_to_completion(w) if o.finished][0].all_tokens


def test_engine_state_follows_the_generation(recorded, penalised_tokens):
    w = make_worker()
    w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                **PENALISED))
    outs = run_to_completion(w)
    fin = [o for o in outs if o.finished][0]
    assert fin.all_tokens == penalised_tokens and len(penalised_tokens) == 8
    check_recorded(recorded, fin.all_tokens)
    assert not w.tstate.row_of and len(w.tstate.free_rows) == 4
    # top-N: three alternatives per token, best first, raw logprobs
    assert len(fin.all_top_logprobs) == 8
    per_step = [t for o in outs for t in (o.new_top_logprobs or [])]
    assert per_step == fin.all_top_logprobs
    for alts, tok, lp in zip(fin.all_top_logprobs, fin.all_tokens,
                             fin.all_logprobs):
        assert len(alts) == 3
        assert [l for _, l in alts] == sorted((l for _, l in alts),
                                              reverse=True)
        assert all(l <= 0 for _, l in alts)
        if tok in dict(alts):
            assert dict(alts)[tok] == lp


def test_engine_penalties_change_the_generation():
    """repetition_penalty < 1 favours seen tokens: greedy then stays inside
    the prompt, which the plain greedy generation does not."""
    def gen(**kw):
        w = make_worker()
        w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                    **kw))
        return [o for o in run_to_completion(w) if o.finished][0].all_tokens

    plain, boosted = gen(), gen(repetition_penalty=0.02)
    assert not set(plain) <= set(PROMPT)
    assert set(boosted) <= set(PROMPT)


def test_engine_state_survives_preempt_and_recompute(recorded,
                                                     penalised_tokens):
    w = make_worker()
    req = EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8, **PENALISED)
    w.add_request(req)
    outs = []
    for _ in range(4):
        outs.extend(w.step())
    outs.extend(w._collect_pending())
    assert 0 < len(req.generated) < 8 and req.inflight == 0
    assert w._preempt(req) is None and req in w.waiting
    assert not w.tstate.row_of                      # freed on preempt
    assert req.orig_prompt_len == len(PROMPT) < req.prompt_len
    outs.extend(run_to_completion(w))
    fin = [o for o in outs if o.finished][0]
    assert fin.all_tokens == penalised_tokens
    check_recorded(recorded, fin.all_tokens)


def test_engine_state_survives_the_handoff(recorded, penalised_tokens):
    pre = make_worker(role=Role.PREFILL)
    dec = make_worker(role=Role.DECODE)
    pre.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                  prefill_only=True, **PENALISED))
    pd = [o for o in run_to_completion(pre, max_steps=5)
          if o.kind == "prefill_done"][0]
    assert not pre.tstate.row_of                    # freed on completion
    dst = dec.mgr.take_blocks(len(pd.kv_blocks))
    dec.pool.tensor[:, :, torch.tensor(dst)] = \
        pre.pool.tensor[:, :, torch.tensor(pd.kv_blocks)]
    dec.admit_transferred(
        EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8, **PENALISED),
        dst, pd.seq_len, pd.first_token, pd.new_logprobs[0],
        pd.new_top_logprobs[0])
    fin = [o for o in run_to_completion(dec) if o.finished][0]
    assert fin.all_tokens == penalised_tokens
    assert len(fin.all_top_logprobs) == 8
    check_recorded(recorded, fin.all_tokens)


def test_engine_abort_frees_the_state_row():
    w = make_worker()
    w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=8,
                                **PENALISED))
    w.step()
    assert list(w.tstate.row_of) == ["r"]
    w.abort("r")
    assert not w.tstate.row_of


def test_engine_pool_grows_and_rows_stay_apart(recorded):
    w = make_worker()
    for i in range(6):
        w.add_request(EngineRequest(
            f"r{i}", prompt_tokens=[100 + i] * 5, max_tokens=3,
            temperature=0.0, frequency_penalty=1.0))
    fins = [o for o in run_to_completion(w) if o.finished]
    assert len(fins) == 6 and w.tstate.tensor.shape[0] == 8
    assert not w.tstate.row_of


def test_engine_dispatch_rule(monkeypatch):
    calls = []
    real = ops.sample_ext
    monkeypatch.setattr(ops, "sample_ext",
                        lambda *a: calls.append(a[12]) or real(*a))

    def gen(**kw):
        w = make_worker()
        w.add_request(EngineRequest("r", prompt_tokens=PROMPT, max_tokens=4,
                                    **kw))
        return [o for o in run_to_completion(w) if o.finished][0]

    gen()
    gen(temperature=0.7, top_p=0.9, seed=1, logprobs=True)
    assert not calls                       # the existing paths are untouched
    assert not EngineRequest("x", [1]).uses_ext
    fin = gen(temperature=0.7, min_p=0.2)
    assert len(calls) == 4 and all(s is None for s in calls)   # no state
    assert fin.all_top_logprobs is None
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=0.1),
               dict(frequency_penalty=-0.1), dict(min_p=0.1),
               dict(top_logprobs=1)):
        r = EngineRequest("x", [1], **kw)
        assert r.uses_ext and r.uses_sampler


# ---- parsers and API --------------------------------------------------------------

def parse(body):
    return OpenAIParser().parse_request(json.dumps(body).encode(), {},
                                        "/v1/completions")


def test_parser_reads_the_new_fields():
    r = parse({"model": "m", "prompt": "x", "presence_penalty": -2,
               "frequency_penalty": 1.5, "repetition_penalty": 1.2,
               "min_p": 0.05, "logprobs": True, "top_logprobs": 20}).request
    assert (r.presence_penalty, r.frequency_penalty, r.repetition_penalty,
            r.min_p, r.top_logprobs, r.logprobs) == (-2.0, 1.5, 1.2, 0.05,
                                                     20, True)
    r = parse({"model": "m", "prompt": "x"}).request
    assert (r.presence_penalty, r.frequency_penalty, r.repetition_penalty,
            r.min_p, r.top_logprobs) == (0.0, 0.0, 1.0, 0.0, 0)
    # top_logprobs: 0 needs no logprobs; the legacy count still means "on"
    assert parse({"model": "m", "prompt": "x",
                  "top_logprobs": 0}).request.top_logprobs == 0
    r = parse({"model": "m", "prompt": "x", "logprobs": 3}).request
    assert r.logprobs is True and r.top_logprobs == 0
    r = parse({"model": "m", "prompt": "x", "logprobs": 1,
               "top_logprobs": 2}).request
    assert r.top_logprobs == 2


@pytest.mark.parametrize("field,value", [
    ("presence_penalty", 2.1), ("presence_penalty", -2.5),
    ("presence_penalty", "1"), ("presence_penalty", True),
    ("frequency_penalty", 3), ("frequency_penalty", -2.01),
    ("frequency_penalty", [1]),
    ("repetition_penalty", 0), ("repetition_penalty", -1.0),
    ("repetition_penalty", "1.1"), ("repetition_penalty", float("inf")),
    ("min_p", -0.1), ("min_p", 1.01), ("min_p", "0.1"),
    ("top_logprobs", 21), ("top_logprobs", -1), ("top_logprobs", 1.5),
    ("top_logprobs", True),
])
def test_parser_rejects_out_of_range(field, value):
    body = {"model": "m", "prompt": "x", "logprobs": True, field: value}
    res = OpenAIParser().parse_request(
        json.dumps(body).encode(), {}, "/v1/completions")
    assert res.request is None and res.error and field in res.error


def test_parser_top_logprobs_requires_logprobs():
    for body in ({"top_logprobs": 2}, {"top_logprobs": 2, "logprobs": False},
                 {"top_logprobs": 2, "logprobs": 0}):
        res = parse(dict(body, model="m", prompt="x"))
        assert res.request is None and "top_logprobs requires" in res.error


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


def test_api_chat_top_logprobs(client):
    body = {"model": "tiny-llama", "max_tokens": 4, "logprobs": True,
            "top_logprobs": 3, "temperature": 0.8, "seed": 4,
            "presence_penalty": 0.5, "frequency_penalty": 0.5,
            "repetition_penalty": 1.2, "min_p": 0.01,
            "messages": [{"role": "user", "content": "hi there you"}]}
    r = client.post("/v1/chat/completions", json=body)
    assert r.status_code == 200, r.text
    content = r.json()["choices"][0]["logprobs"]["content"]
    assert len(content) == 4
    for c in content:
        assert set(c) == {"token", "logprob", "top_logprobs"}
        assert len(c["top_logprobs"]) == 3
        assert all(set(a) == {"token", "logprob"} for a in c["top_logprobs"])
        lps = [a["logprob"] for a in c["top_logprobs"]]
        assert lps == sorted(lps, reverse=True) and lps[0] <= 0
    again = client.post("/v1/chat/completions", json=body).json()
    assert again["choices"][0] == r.json()["choices"][0]
    # the penalties reach the sampler: without them the text differs
    for k in ("presence_penalty", "frequency_penalty", "repetition_penalty"):
        body.pop(k)
    body.update(max_tokens=12, temperature=0)
    plain = client.post("/v1/chat/completions", json=body).json()
    body.update(repetition_penalty=0.02)
    pen = client.post("/v1/chat/completions", json=body).json()
    assert plain["choices"][0]["message"] != pen["choices"][0]["message"]


def test_api_completions_top_logprobs_and_validation(client):
    body = {"model": "tiny-llama", "prompt": "hello world test prompt",
            "max_tokens": 3, "logprobs": 1, "top_logprobs": 2}
    r = client.post("/v1/completions", json=body)
    assert r.status_code == 200, r.text
    lp = r.json()["choices"][0]["logprobs"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == 3
    assert len(lp["top_logprobs"]) == 3
    for alts, best in zip(lp["top_logprobs"], lp["token_logprobs"]):
        assert isinstance(alts, dict) and 1 <= len(alts) <= 2
        # greedy: the sampled token is the best alternative
        assert max(alts.values()) == best
    plain = client.post("/v1/completions", json={
        "model": "tiny-llama", "prompt": "hello", "max_tokens": 2,
        "logprobs": 1}).json()
    assert "top_logprobs" not in plain["choices"][0]["logprobs"]
    for bad in ({"min_p": 2}, {"presence_penalty": 5},
                {"frequency_penalty": -5}, {"repetition_penalty": 0},
                {"top_logprobs": 30, "logprobs": 1}, {"top_logprobs": 2}):
        r = client.post("/v1/completions", json=dict(
            {"model": "tiny-llama", "prompt": "x"}, **bad))
        assert r.status_code == 400, bad
