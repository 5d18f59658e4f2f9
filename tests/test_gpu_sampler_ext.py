"""GPU tier of the sample_ext tests: the HIP kernel against ops.ref.sample_ext
(exact tokens, kept-set sizes, thresholds, top-N indices and state-after),
bit equality with the plain sampler when every new input is off,
token_state_fill on its hazard cases, the bindings' argument checks and one
engine run (DEVELOPMENT.md "Sampling"; inputs in tests/sampler_ext_cases.py).

Prints `EDGE|sample_ext|<case>|limit|worst` lines for the logprobs and one
`UNDECIDED|sample_ext|<case>|share` line before asserting (pytest -s)."""
from collections import Counter

import pytest
import torch

import sampler_cases as sc
import sampler_ext_cases as xc
from llm_d_inference_scheduler_amd.ops import ref

pytestmark = pytest.mark.gpu

LOGPROB_LIMIT = 1e-4            # the limit test_gpu_sampler.py uses


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def case_name(V, B, dtype):
    return f"V{V}_B{B}_{'bf16' if dtype == torch.bfloat16 else 'f32'}"


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("V,B,dtype,gen_seed", xc.SHAPES)
def test_matches_reference(ext, V, B, dtype, gen_seed):
    launches = xc.make_case(V, B, dtype, gen_seed)
    name = case_name(V, B, dtype)
    share = xc.undecided_share(launches)
    print(f"UNDECIDED|sample_ext|{name}|{share:.4f}")
    assert share <= xc.MAX_UNDECIDED_SHARE
    worst_lp = worst_top = 0.0
    for li, L in enumerate(launches):
        args = L.args("cuda")
        state = args[-1]
        tok, lp, nk, th, ttok, tlp = (
            t.cpu() for t in ext.sample_ext(*args, n_top=xc.N_TOP))
        lsm = torch.log_softmax(L.logits.double(), dim=-1)
        want = lsm.gather(1, tok.unsqueeze(1)).squeeze(1)
        assert torch.isfinite(lp).all()
        worst_lp = max(worst_lp, float((lp.double() - want).abs().max()))
        # top-N does not depend on penalties, filters or rounding: all rows
        assert torch.equal(ttok, L.top_tokens), (name, li)
        on = ttok >= 0
        assert torch.equal(tlp[~on], L.top_logprobs[~on])       # -inf
        want_top = lsm.gather(1, ttok.clamp(min=0))
        if on.any():
            worst_top = max(worst_top, float(
                (tlp.double() - want_top)[on].abs().max()))
        state = state.cpu()
        for r in range(B):
            where = (name, li, r) + L.plan[r]
            if L.kept_undecided[r]:
                continue
            assert int(nk[r]) == int(L.n_kept[r]), where
            assert th[r].view(torch.int32) == \
                L.threshold[r].view(torch.int32), where
            if not L.token_undecided[r]:
                assert int(tok[r]) == int(L.tokens[r]), where
                sr = int(L.state_row[r])
                if sr >= 0:
                    assert torch.equal(state[sr], L.state_after[sr]), where
        # junk row, padding columns and the rows of skipped requests
        decided = [not (a or b) for a, b in
                   zip(L.kept_undecided, L.token_undecided)]
        if all(decided):
            assert torch.equal(state, L.state_after), (name, li)
        assert torch.equal(state[0], L.state_before[0])
        assert torch.equal(state[:, V:], L.state_before[:, V:])
    print(f"EDGE|sample_ext|{name}|{LOGPROB_LIMIT:.3e}|{worst_lp:.3e}")
    print(f"EDGE|sample_ext_top|{name}|{LOGPROB_LIMIT:.3e}|{worst_top:.3e}")
    assert worst_lp <= LOGPROB_LIMIT
    assert worst_top <= LOGPROB_LIMIT


@pytest.mark.parametrize("V,B,dtype,gen_seed", xc.SHAPES)
def test_fill_builds_the_case_states(ext, V, B, dtype, gen_seed):
    """token_state_fill on the device rebuilds every launch's state from the
    histories, starting from a used (junk) tensor."""
    for L in xc.make_case(V, B, dtype, gen_seed)[:12]:
        state = torch.full_like(L.state_before, xc.JUNK).cuda()
        rows, toks, offs, n_p, v = L.fill_args
        ext.token_state_fill(state, rows.cuda(), toks.cuda(), offs.cuda(),
                             n_p.cuda(), v)
        want = torch.full_like(L.state_before, xc.JUNK)
        ref.token_state_fill(want, *L.fill_args)
        assert torch.equal(state.cpu(), want)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("V,B,dtype,gen_seed", sc.SHAPES)
def test_neutral_equals_plain_sampler(ext, V, B, dtype, gen_seed, with_rows):
    """Every new input off: bit-equal to ext.sample on all rows, undecided
    ones included, whether the rows have no state (state_row = -1) or point
    into a state tensor full of junk (rep = 1, freq = pres = 0 make every
    state value a no-op)."""
    dev = "cuda"
    f32, i32 = torch.float32, torch.int32
    off = (torch.ones(B, dtype=f32, device=dev),
           torch.zeros(B, dtype=f32, device=dev),
           torch.zeros(B, dtype=f32, device=dev),
           torch.zeros(B, dtype=f32, device=dev),
           torch.zeros(B, dtype=i32, device=dev))
    srow = torch.arange(B, dtype=i32, device=dev) if with_rows else \
        torch.full((B,), -1, dtype=i32, device=dev)
    for L in sc.make_case(V, B, dtype, gen_seed):
        state = torch.randint(0, 0x7FFF, (B, (V + 7) // 8 * 8),
                              dtype=torch.int16, device=dev)
        args = L.args(dev)
        plain = ext.sample(*args)
        got = ext.sample_ext(*args, *off, srow, state, 0)
        for a, b in zip(plain, got[:4]):
            assert torch.equal(bits(a), bits(b))
        assert got[4].shape == (B, 0) and got[5].shape == (B, 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_all_equal_logits_top20_is_the_first_20(ext, dtype):
    B, V = 2, 100
    dev = "cuda"
    lg = torch.zeros(B, V, dtype=dtype, device=dev)
    z = lambda dt: torch.zeros(B, dtype=dt, device=dev)
    o = lambda dt: torch.ones(B, dtype=dt, device=dev)
    out = ext.sample_ext(
        lg, torch.tensor([0.0, 1.0], device=dev), z(torch.int32),
        o(torch.float32), z(torch.int64), z(torch.int32), o(torch.float32),
        z(torch.float32), z(torch.float32), z(torch.float32),
        torch.tensor([20, 20], dtype=torch.int32, device=dev),
        torch.full((B,), -1, dtype=torch.int32, device=dev), None, 20)
    want = torch.arange(20).expand(B, 20)
    assert torch.equal(out[4].cpu(), want)
    import math
    assert float((out[5].cpu() + math.log(V)).abs().max()) <= LOGPROB_LIMIT


# ---- token_state_fill -------------------------------------------------------

def fill_both(ext, R, V, rows, prompt_out, junk=0):
    """Device and reference fill of the same lists -> (device, reference)."""
    i32 = torch.int32
    toks, offs, n_p = [], [0], []
    for pr, out in prompt_out:
        toks += list(pr) + list(out)
        offs.append(len(toks))
        n_p.append(len(pr))
    a = (torch.tensor(rows, dtype=i32), torch.tensor(toks, dtype=i32),
         torch.tensor(offs, dtype=torch.int64), torch.tensor(n_p, dtype=i32))
    want = ref.token_state_alloc(R, V, "cpu")
    want[:] = junk
    dev = want.clone().cuda()
    ref.token_state_fill(want, *a, V)
    ext.token_state_fill(dev, *(t.cuda() for t in a), V)
    return dev.cpu(), want


def test_fill_same_id_600_times_and_adjacent_pairs(ext):
    V = 1001
    pairs = [t for j in range(0, 120, 2) for t in (j, j + 1, j + 1)]
    out = [777] * 600 + pairs
    got, want = fill_both(ext, 2, V, [1], [([776, 777, 0], out)])
    assert torch.equal(got, want)
    assert int(got[1, 777]) == 0x4000 + 600 and int(got[1, 776]) == 0x4000
    assert int(got[1, 778]) == 0
    assert int(got[1, 0]) == 0x4000 + 1 and int(got[1, 1]) == 2
    assert int(got[0].abs().sum()) == 0


def test_fill_saturates_without_carry(ext):
    """16400 occurrences: c stops at 16383; bit 14 (clear for the output-only
    id, set for its prompt neighbour) and both neighbours stay as they are."""
    V = 100
    got, want = fill_both(ext, 1, V, [0],
                          [([40, 42], [41] * 16400 + [40, 42, 42])])
    assert torch.equal(got, want)
    assert int(got[0, 41]) == 16383
    assert int(got[0, 40]) == 0x4000 + 1 and int(got[0, 42]) == 0x4000 + 2
    # and with the prompt bit on the saturated id itself
    got, want = fill_both(ext, 1, V, [0], [([41], [41] * 16400)])
    assert torch.equal(got, want) and int(got[0, 41]) == 0x4000 + 16383
    assert int(got[0, 40]) == 0 and int(got[0, 42]) == 0


def test_fill_skips_ids_out_of_range(ext):
    """-1 and V aimed at the middle row: the outer rows and the padding
    columns (V = 1001: column V shares a word with column V - 1) stay."""
    V = 1001
    got, want = fill_both(ext, 3, V, [1],
                          [([-1, V, V - 1], [-1, V, V + 6, 2 ** 30, 0])],
                          junk=xc.JUNK)
    assert torch.equal(got, want)
    assert (got[0] == xc.JUNK).all() and (got[2] == xc.JUNK).all()
    assert (got[1, V:] == xc.JUNK).all()
    assert int(got[1, V - 1]) == 0x4000 and int(got[1, 0]) == 1
    assert int(got[1, 1:V - 1].abs().sum()) == 0


def test_refill_clears_a_used_row(ext):
    V = 32064
    g = torch.Generator().manual_seed(3)
    first = torch.randint(0, V, (4096,), generator=g).tolist()
    i32 = torch.int32
    state = ref.token_state_alloc(2, V, "cuda")
    rows = torch.tensor([1], dtype=i32).cuda()
    ext.token_state_fill(state, rows, torch.tensor(first, dtype=i32).cuda(),
                         torch.tensor([0, 4096]).cuda(),
                         torch.tensor([100], dtype=i32).cuda(), V)
    assert int((state[1] != 0).sum()) > 3000
    ext.token_state_fill(state, rows, torch.tensor([5], dtype=i32).cuda(),
                         torch.tensor([0, 1]).cuda(),
                         torch.tensor([0], dtype=i32).cuda(), V)
    want = ref.token_state_alloc(2, V, "cpu")
    want[1, 5] = 1
    assert torch.equal(state.cpu(), want)


# ---- argument checks: rejected on the host, nothing launched ---------------

def _good(B=2, V=16):
    dev = "cuda"
    f32, i32 = torch.float32, torch.int32
    return dict(
        logits=torch.zeros(B, V, dtype=torch.bfloat16, device=dev),
        temperature=torch.ones(B, device=dev),
        top_k=torch.zeros(B, dtype=i32, device=dev),
        top_p=torch.ones(B, device=dev),
        seed=torch.zeros(B, dtype=torch.int64, device=dev),
        pos=torch.zeros(B, dtype=i32, device=dev),
        rep=torch.ones(B, device=dev), pres=torch.zeros(B, device=dev),
        freq=torch.zeros(B, device=dev), min_p=torch.zeros(B, device=dev),
        top_n=torch.zeros(B, dtype=i32, device=dev),
        state_row=torch.arange(B, dtype=i32, device=dev),
        state=torch.zeros(B, V, dtype=torch.int16, device=dev), n_top=4)


SAMPLE_EXT_BAD = {
    "logits_dtype": lambda a: a.update(logits=a["logits"].half()),
    "logits_dim": lambda a: a.update(logits=a["logits"][0]),
    "logits_contiguous": lambda a: a.update(
        logits=a["logits"].t().contiguous().t()),
    "logits_device": lambda a: a.update(logits=a["logits"].cpu()),
    "n_top_high": lambda a: a.update(n_top=21),
    "n_top_negative": lambda a: a.update(n_top=-1),
    "state_dtype": lambda a: a.update(state=a["state"].int()),
    "state_dim": lambda a: a.update(state=a["state"][0]),
    "state_device": lambda a: a.update(state=a["state"].cpu()),
    "state_contiguous": lambda a: a.update(
        state=torch.zeros(2, 32, dtype=torch.int16,
                          device="cuda")[:, :16]),
    "state_vs": lambda a: a.update(
        state=torch.zeros(2, 24, dtype=torch.int16, device="cuda")),
    "state_alignment": lambda a: a.update(
        state=torch.zeros(2 * 16 + 1, dtype=torch.int16,
                          device="cuda")[1:].view(2, 16)),
}
for _name, _dt in [("temperature", torch.float32), ("top_k", torch.int32),
                   ("top_p", torch.float32), ("seed", torch.int64),
                   ("pos", torch.int32), ("rep", torch.float32),
                   ("pres", torch.float32), ("freq", torch.float32),
                   ("min_p", torch.float32), ("top_n", torch.int32),
                   ("state_row", torch.int32)]:
    SAMPLE_EXT_BAD[_name + "_dtype"] = \
        lambda a, n=_name: a.update({n: a[n].double()})
    SAMPLE_EXT_BAD[_name + "_length"] = \
        lambda a, n=_name: a.update({n: a[n][:1]})
    SAMPLE_EXT_BAD[_name + "_device"] = \
        lambda a, n=_name: a.update({n: a[n].cpu()})


def test_sample_ext_accepts_the_good_arguments(ext):
    out = ext.sample_ext(**_good())
    assert out[4].shape == (2, 4)
    a = _good()
    a["state"] = None
    assert ext.sample_ext(**a)[0].shape == (2,)


@pytest.mark.parametrize("bad", sorted(SAMPLE_EXT_BAD))
def test_sample_ext_binding_checks(ext, bad):
    a = _good()
    SAMPLE_EXT_BAD[bad](a)
    with pytest.raises(RuntimeError):
        ext.sample_ext(**a)


def _good_fill(V=16):
    dev = "cuda"
    i32 = torch.int32
    return dict(state=torch.zeros(2, V, dtype=torch.int16, device=dev),
                rows=torch.tensor([0, 1], dtype=i32, device=dev),
                tokens=torch.tensor([1, 2, 3], dtype=i32, device=dev),
                offsets=torch.tensor([0, 2, 3], device=dev),
                n_prompt=torch.tensor([1, 0], dtype=i32, device=dev), V=V)


FILL_BAD = {
    "v_zero": lambda a: a.update(V=0),
    "vs_mismatch": lambda a: a.update(V=17),
    "state_dtype": lambda a: a.update(state=a["state"].int()),
    "state_device": lambda a: a.update(state=a["state"].cpu()),
    "rows_dtype": lambda a: a.update(rows=a["rows"].long()),
    "rows_device": lambda a: a.update(rows=a["rows"].cpu()),
    "tokens_dtype": lambda a: a.update(tokens=a["tokens"].long()),
    "tokens_device": lambda a: a.update(tokens=a["tokens"].cpu()),
    "tokens_dim": lambda a: a.update(tokens=a["tokens"].view(1, 3)),
    "offsets_dtype": lambda a: a.update(offsets=a["offsets"].int()),
    "offsets_length": lambda a: a.update(offsets=a["offsets"][:2]),
    "n_prompt_dtype": lambda a: a.update(n_prompt=a["n_prompt"].long()),
    "n_prompt_length": lambda a: a.update(n_prompt=a["n_prompt"][:1]),
    "rows_contiguous": lambda a: a.update(
        rows=torch.zeros(4, dtype=torch.int32, device="cuda")[::2]),
}


@pytest.mark.parametrize("bad", sorted(FILL_BAD))
def test_token_state_fill_binding_checks(ext, bad):
    a = _good_fill()
    ext.token_state_fill(**a)
    FILL_BAD[bad](a)
    before = a["state"].clone() if a["state"].is_cuda else None
    with pytest.raises(RuntimeError):
        ext.token_state_fill(**a)
    if before is not None and before.dtype == torch.int16:
        assert torch.equal(a["state"], before)


# ---- engine on the GPU ----------------------------------------------------

def test_engine_state_follows_the_generation(monkeypatch):
    """One penalised request through the engine on the device: before every
    sample_ext call its state row decodes to (prompt tokens, Counter of the
    output so far), and top-N alternatives come back with every token."""
    from llm_d_inference_scheduler_amd import ops
    from llm_d_inference_scheduler_amd.engine import (EngineRequest,
                                                      EngineWorker)
    from llm_d_inference_scheduler_amd.models.configs import ModelConfig
    cfg = ModelConfig(name="gpu-test", vocab_size=2048, hidden_size=1024,
                      intermediate_size=2048, num_layers=2, num_heads=8,
                      num_kv_heads=2, head_dim=128, rope_theta=10000.0)
    prompt = list(range(300, 430)) + [301, 302]
    seen = []
    real = ops.sample_ext

    def spy(*a):
        row = a[12][int(a[11][0]), :a[0].shape[1]].to(torch.int32).cpu()
        seen.append((set(torch.nonzero(row & 0x4000).squeeze(1).tolist()),
                     Counter({int(i): int(row[i] & 0x3FFF) for i in
                              torch.nonzero(row & 0x3FFF).squeeze(1)})))
        return real(*a)

    monkeypatch.setattr(ops, "sample_ext", spy)
    w = EngineWorker(cfg, "cuda:0", kv_blocks=256, dtype=torch.bfloat16,
                     seed=9)
    w.add_request(EngineRequest(
        "a", prompt_tokens=prompt, max_tokens=6, temperature=0.9, seed=11,
        repetition_penalty=0.5, frequency_penalty=0.3, presence_penalty=0.1,
        min_p=0.01, top_logprobs=4, logprobs=True))
    outs = []
    for _ in range(64):
        outs.extend(w.step())
        if not w.has_work:
            break
    fin = [o for o in outs if o.finished][0]
    toks = fin.all_tokens
    assert len(toks) == len(seen) == 6
    for j, (pr, cnt) in enumerate(seen):
        assert pr == set(prompt) and cnt == Counter(toks[:j]), j
    assert not w.tstate.row_of
    assert len(fin.all_top_logprobs) == 6
    for alts, lp, tok in zip(fin.all_top_logprobs, fin.all_logprobs, toks):
        assert len(alts) == 4
        assert [l for _, l in alts] == sorted((l for _, l in alts),
                                              reverse=True)
        if tok in dict(alts):
            assert dict(alts)[tok] == lp
