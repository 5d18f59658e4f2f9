"""The engine's logits against a float64 dense model (DEVELOPMENT.md "Engine
logits tests").

The kernel tiers judge each HIP kernel on its own. This module judges the
layer above them, the code that turns requests into kernel arguments:
positions, slots, block tables, (start, chunk, prior) metas, decode rows,
sequence lengths. It records every `model.forward` of a worker, maps each
logits row to a (request, position) from the engine's host-side bookkeeping,
and compares the row with one causal, unpaged, unchunked float64 pass over
the request's final token history.

With the weights the runner initialises attention is nearly uniform and a
wrong position, slot or length moves a logits row by less than bf16 rounding
does. `sharpen` therefore overwrites the weights so that every query puts
O(1) of its attention on a few specific tokens: itself and repeats of
itself, the token before it, and the first tokens of its sequence.
tests/test_engine_cases.py proves on the CPU that the faults listed there
move the worst row by more than 10x the limit the GPU tier asserts.
"""
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from llm_d_inference_scheduler_amd.engine import EngineRequest, EngineWorker
from llm_d_inference_scheduler_amd.models.configs import ModelConfig

# The smallest sizes the device path accepts: flash prefill and the decode
# kernels need D = 128.
CONFIG = ModelConfig(
    name="engine-cases", vocab_size=512, hidden_size=256,
    intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2,
    head_dim=128, rope_theta=10000.0, max_position=1024)

SHARPEN_SEED = 1234


def make_worker(device, dtype=torch.bfloat16, **kw) -> EngineWorker:
    """A sharpened worker whose pass boundaries do not depend on the
    wall clock (prefill_min_tokens=1, prefill_max_delay_ms=0)."""
    kw.setdefault("kv_blocks", 256)
    kw.setdefault("max_model_len", 1024)
    worker = EngineWorker(CONFIG, device, dtype=dtype, prefill_min_tokens=1,
                          prefill_max_delay_ms=0.0, overlap_streams=False,
                          **kw)
    sharpen(worker.model, SHARPEN_SEED)
    return worker


# ---- the reference --------------------------------------------------------

def _rms64(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * w


def _rope64(x, cos, sin):
    """NeoX rotate-half on [T, H, D] with cos, sin [T, 1, D/2]."""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def dense_logits64(model, tokens: List[int]) -> torch.Tensor:
    """Logits [len(tokens), V] of one causal pass of the Llama block in
    float64 over the whole token list: no pages, chunks, block tables or
    slots. The weights are the runner's, as float64 on the CPU; of ops.ref
    only the RoPE table the runner already holds is read."""
    c = model.cfg
    f64 = lambda t: t.detach().to("cpu", torch.float64)
    T = len(tokens)
    ids = torch.tensor(tokens, dtype=torch.int64)
    cs = f64(model.cos_sin)[:T]                       # [T, D/2, 2]
    cos, sin = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    qpg = c.num_heads // c.num_kv_heads
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    x = f64(model.embed)[ids]
    for layer in model.layers:
        h = _rms64(x, f64(layer["input_norm"]), c.rms_eps)
        q, k, v = (h @ f64(layer["wqkv"])).split(
            [c.q_size, c.kv_size, c.kv_size], dim=-1)
        q = _rope64(q.view(T, c.num_heads, c.head_dim), cos, sin)
        k = _rope64(k.view(T, c.num_kv_heads, c.head_dim), cos, sin)
        v = v.view(T, c.num_kv_heads, c.head_dim)
        k = k.repeat_interleave(qpg, dim=1)           # [T, QH, D]
        v = v.repeat_interleave(qpg, dim=1)
        s = torch.einsum("thd,shd->hts", q, k) / math.sqrt(c.head_dim)
        s = s.masked_fill(~causal, float("-inf"))
        o = torch.einsum("hts,shd->thd", torch.softmax(s, dim=-1), v)
        x = x + o.reshape(T, c.q_size) @ f64(layer["wo"])
        h = _rms64(x, f64(layer["post_norm"]), c.rms_eps)
        g, u = (h @ f64(layer["wgate_up"])).split(c.intermediate_size, dim=-1)
        x = x + (g * torch.sigmoid(g) * u) @ f64(layer["wdown"])
    h = _rms64(x, f64(model.final_norm), c.rms_eps)
    return h @ f64(model.lm_head).t()


# ---- the weights ----------------------------------------------------------

# sharpen() knobs (see its docstring)
QKV_STD = 0.05
COMMON = 0.5          # share of an embedding's energy in the common direction
POS_PEAK = 10.0       # a position head's logit at its offset, in nats
POS_OFFSETS = (1, 0.5)  # positions back, of query heads 1 and 2
POS_FAST = 16         # position heads read RoPE pairs [0, POS_FAST)
SINK_PEAK = 10.0      # the sink head's logit for a sink token, in nats
SINK_SLOW = 48        # the sink head reads RoPE pairs [SINK_SLOW, D / 2)
SINK_TOKENS = tuple(range(496, 512))
N_SINKS = 4           # sink tokens at the head of every prompt
WO_GAIN = 8.0
HEAD_GAIN = (1.0, 1.0, 1.0, 1.0)   # per query head, on top of WO_GAIN


def sharpen(model, seed: int) -> None:
    """Overwrite the runner's weights in place so that attention is sharp.

    Everything is drawn from a CPU generator in fp32, rounded to the
    runner's dtype and copied to its device: a CPU run and a GPU run hold
    the same model.

    - Every embedding is a random vector plus one common direction c, which
      V, the MLP and the LM head do not read: it only steers attention.
    - wqkv ~ N(0, QKV_STD^2). Per layer, KV head 0's K columns equal the Q
      columns of query head 0: after RoPE q_t.k_t = |q_t|^2, so that head
      attends to its own token and to nearby repeats of it.
    - Query heads 1 and 2 are position heads. Their q is the same for every
      token (it reads c): K's image of c on the fastest RoPE pairs, rotated
      back by 1 (head 1) or half a position (head 2). R(t)q . R(s)k then
      peaks at s = t - 1, or evenly at t and t - 1, by POS_PEAK nats,
      whatever the tokens are, and falls off within about two positions.
    - Query head 3 is a sink head: its q is a fixed vector r on the slowest
      RoPE pairs, and the embeddings of SINK_TOKENS carry the direction K
      maps onto r. It attends to the sink tokens of its sequence from any
      distance. Every prompt begins with its own choice of them.
    - wo is multiplied by WO_GAIN so that attention carries the residual.

    So the newest token, the tokens just before it and the first block each
    hold O(1) of some head's weight at any sequence length, and what a row
    attends to changes from one position to the next."""
    c = model.cfg
    assert c.num_heads == 4 and c.num_kv_heads == 2 and not c.qk_norm
    H, D = c.hidden_size, c.head_dim
    half = D // 2
    gen = torch.Generator(device="cpu").manual_seed(seed)

    def randn(*shape, std=1.0):
        return torch.empty(*shape, dtype=torch.float32).normal_(
            0.0, std, generator=gen)

    def put(dst, src):
        dst.copy_(src.to(dst.dtype).to(dst.device))

    def blind(w):
        """w [H, n] with the common direction removed from its input."""
        return w - torch.outer(common, common @ w)

    def rotated(vec, by):
        """vec [D] rotated by `by` positions (NeoX halves)."""
        ang = inv_freq * by
        cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
        v1, v2 = vec[:half], vec[half:]
        return torch.cat([v1 * cos - v2 * sin, v2 * cos + v1 * sin])

    common = randn(H)
    common /= common.norm()
    embed = blind(randn(c.vocab_size, H).t()).t() * math.sqrt(1.0 - COMMON) \
        + common * math.sqrt(COMMON * H)
    # on a normed row x: c . x = sqrt(COMMON * H)
    cx = math.sqrt(COMMON * H)
    inv_freq = 1.0 / (c.rope_theta ** (torch.arange(half).double() / half))
    fast = torch.zeros(D)
    fast[:POS_FAST] = 1.0
    fast[half:half + POS_FAST] = 1.0
    slow = torch.zeros(D)
    slow[SINK_SLOW:half] = 1.0
    slow[half + SINK_SLOW:] = 1.0
    sink_dir = None
    for li, layer in enumerate(model.layers):
        wqkv = randn(H, c.q_size + 2 * c.kv_size, std=QKV_STD)
        q = wqkv[:, :c.q_size].view(H, c.num_heads, D)
        k = wqkv[:, c.q_size:c.q_size + c.kv_size].view(H, c.num_kv_heads, D)
        wqkv[:, c.q_size + c.kv_size:] = blind(
            wqkv[:, c.q_size + c.kv_size:])
        k[:, 0] = q[:, 0]
        for head, kvh, off in ((1, 0, POS_OFFSETS[0]), (2, 1, POS_OFFSETS[1])):
            # every k_s holds cx * kc; q = g * cx * R(-off) kc peaks at
            # s = t - off with g * cx^2 * |kc|^2 / sqrt(D)
            kc = (common @ k[:, kvh]) * fast
            g = POS_PEAK * math.sqrt(D) / (cx * cx * float(kc.dot(kc)))
            q[:, head] = g * torch.outer(common, rotated(kc, -off))
        # a sink token carries sqrt(H) / 2 of u, which K maps onto r
        u = k[:, 1] @ slow
        g = SINK_PEAK * math.sqrt(D) / (
            cx * float(u.norm()) * math.sqrt(H) / 2)
        q[:, 3] = g * torch.outer(common, slow)
        if li == 0:
            sink_dir = blind(u.unsqueeze(1)).squeeze(1)
            sink_dir /= sink_dir.norm()
        put(layer["wqkv"], wqkv)
        wo = randn(c.q_size, H, std=0.02 / math.sqrt(2 * c.num_layers))
        wo = wo.view(c.num_heads, D, H) * WO_GAIN * torch.tensor(
            HEAD_GAIN).view(-1, 1, 1)
        put(layer["wo"], wo.view(c.q_size, H))
        put(layer["wgate_up"], blind(
            randn(H, 2 * c.intermediate_size, std=0.02)))
        put(layer["wdown"], randn(c.intermediate_size, H, std=0.02))
        put(layer["input_norm"], 1.0 + 0.05 * randn(H))
        put(layer["post_norm"], 1.0 + 0.05 * randn(H))
    # the sink tokens: a quarter of their energy along layer 0's sink
    # direction (layer 1 reads states, not embeddings: its sink head is
    # whatever it is)
    for tok in SINK_TOKENS:
        embed[tok] = (embed[tok] - common * cx) * math.sqrt(
            (0.75 - COMMON) / (1.0 - COMMON)) + common * cx + \
            sink_dir * math.sqrt(H) / 2
    put(model.embed, embed)
    if model.lm_head is not model.embed:
        put(model.lm_head, blind(randn(c.vocab_size, H, std=0.02).t()).t())
    put(model.final_norm, 1.0 + 0.05 * randn(H))


# ---- recording ------------------------------------------------------------

@dataclass
class Record:
    """One model.forward call. spans: (request id, first position, one past
    the last position, first batch row) per sequence, in batch order. rows:
    the (request id, position) of each logits row."""
    step: int
    is_decode: bool
    input_ids: torch.Tensor
    positions: torch.Tensor
    slot_mapping: torch.Tensor
    seq_lens: Optional[torch.Tensor]
    max_seq_len: Optional[int]
    seq_starts: Optional[List[int]]
    ctx_lens: Optional[List[int]]
    prefill_meta: Optional[torch.Tensor]
    spans: List[Tuple[str, int, int, int]]
    rows: List[Tuple[str, int]]
    dstate_rows: Optional[List[int]]
    logits: torch.Tensor                  # fp32 on the CPU


class Recorder:
    """Wraps worker.model.forward (and _prefill_pass, to see the state a
    pass starts from) on the instance. The (request, position) of every row
    comes from the engine's bookkeeping, never from the batch tensors:

    - prefill: the waiting requests in admission order whose `computed`
      advanced in this pass; a chunk runs from the value before the pass
      (for a request admitted in this pass, its prefix-cache hit) to the
      value now, and has a logits row when it ends the prompt;
    - decode: the ids the decode state gathered its rows for, each at the
      block manager's sequence length minus one.

    mutate(batch), if given, runs before the real forward and may change
    the batch in place or return another; `current` then holds the spans of
    the call. The record keeps the batch as the model saw it."""

    def __init__(self, worker: EngineWorker,
                 mutate: Optional[Callable] = None):
        self.worker = worker
        self.mutate = mutate
        if mutate is not None and hasattr(mutate, "recorder"):
            mutate.recorder = self
        self.records: List[Record] = []
        self.current: List[Tuple[str, int, int, int]] = []
        self.outputs = []
        self._before: Dict[str, int] = {}
        self._forward = worker.model.forward
        self._prefill_pass = worker._prefill_pass
        worker.model.forward = self._wrapped_forward
        worker._prefill_pass = self._wrapped_prefill_pass

    def _wrapped_prefill_pass(self):
        w = self.worker
        self._before = {r.request_id: r.computed for r in w.waiting
                        if r.request_id in w.mgr.tables}
        return self._prefill_pass()

    def _spans(self, is_decode: bool):
        w = self.worker
        spans, rows, drows = [], [], None
        if is_decode:
            ids = list(w.dstate._active_ids)
            drows = [w.dstate.row_of[i] for i in ids]
            for i, rid in enumerate(ids):
                pos = w.mgr.seq_lens[rid] - 1
                spans.append((rid, pos, pos + 1, i))
                rows.append((rid, pos))
            return spans, rows, drows
        row = 0
        for req in sorted(w.waiting, key=lambda r: -r.priority):
            rid = req.request_id
            if rid not in w.mgr.tables:
                continue
            start = self._before.get(rid, req.cached_tokens)
            end = req.computed
            if end <= start:
                continue
            spans.append((rid, start, end, row))
            row += end - start
            if end == req.prompt_len:
                rows.append((rid, end - 1))
        return spans, rows, drows

    def _wrapped_forward(self, batch, kv_pool, *args, **kw):
        spans, rows, drows = self._spans(batch.is_decode)
        self.current = spans
        if self.mutate is not None:
            batch = self.mutate(batch) or batch
        logits = self._forward(batch, kv_pool, *args, **kw)
        cpu = lambda t: None if t is None else t.detach().cpu().clone()
        self.records.append(Record(
            step=self.worker.steps, is_decode=batch.is_decode,
            input_ids=cpu(batch.input_ids), positions=cpu(batch.positions),
            slot_mapping=cpu(batch.slot_mapping),
            seq_lens=cpu(batch.seq_lens), max_seq_len=batch.max_seq_len,
            seq_starts=None if batch.seq_starts is None
            else list(batch.seq_starts),
            ctx_lens=None if batch.ctx_lens is None
            else list(batch.ctx_lens),
            prefill_meta=cpu(batch.prefill_meta), spans=spans, rows=rows,
            dstate_rows=drows, logits=logits.detach().float().cpu()))
        return logits

    def close(self) -> None:
        self.worker.model.forward = self._forward
        self.worker._prefill_pass = self._prefill_pass


def run_scenario(worker: EngineWorker, arrivals, max_steps: int = 400,
                 mutate: Optional[Callable] = None):
    """Drive the worker: arrivals is a list of (step, EngineRequest), each
    request added before that step runs. Returns the recorder (its
    `outputs` hold every RequestOutput) and {request id: prompt +
    generated} for every request."""
    rec = Recorder(worker, mutate)
    prompts = {r.request_id: list(r.prompt_tokens) for _, r in arrivals}
    generated = {rid: [] for rid in prompts}
    pending = sorted(arrivals, key=lambda a: a[0])
    try:
        for step in range(max_steps):
            while pending and pending[0][0] <= step:
                worker.add_request(pending.pop(0)[1])
            for out in worker.step():
                rec.outputs.append(out)
                assert not out.error, out
                generated[out.request_id].extend(out.new_tokens)
            if not pending and not worker.has_work:
                break
        else:
            raise AssertionError("scenario did not finish")
    finally:
        rec.close()
    return rec, {rid: prompts[rid] + generated[rid] for rid in prompts}


# ---- judging --------------------------------------------------------------

def judge(records: List[Record], histories: Dict[str, List[int]], model,
          refs: Optional[Dict[str, torch.Tensor]] = None
          ) -> Dict[str, float]:
    """The worst |row - ref[pos]| / |ref[pos]| per request id over every
    recorded logits row. One dense_logits64 per request serves every step:
    the engine's decoding is teacher-forced by its own tokens."""
    if refs is None:
        refs = {rid: dense_logits64(model, h) for rid, h in histories.items()}
    worst = {rid: 0.0 for rid in histories}
    for rec in records:
        assert rec.logits.shape[0] == len(rec.rows), (rec.step, rec.rows)
        for i, (rid, pos) in enumerate(rec.rows):
            ref = refs[rid][pos]
            err = float((rec.logits[i].double() - ref).norm() / ref.norm())
            if not err <= worst[rid]:          # NaN counts as the worst
                worst[rid] = err if err == err else float("inf")
    return worst


def check_token_path(records: List[Record], histories: Dict[str, List[int]],
                     prompt_lens: Dict[str, int]) -> None:
    """Exact checks on the path of the tokens (greedy requests only):

    - every input row the engine fed the model holds the history's token
      of its position: prompt chunks, and for a decode row the token the
      engine emitted one step before;
    - every emitted token has a recorded logits row, that of the position
      before it, and its logit equals the row's maximum;
    - no position is fed twice without a preemption in between, and every
      position below the last is fed."""
    row_of = {}
    for rec in records:
        for rid, start, end, row0 in rec.spans:
            got = rec.input_ids[row0:row0 + end - start].tolist()
            assert got == histories[rid][start:end], \
                ("input_ids", rec.step, rid, start, end)
        for i, key in enumerate(rec.rows):
            row_of.setdefault(key, []).append(rec.logits[i])
    for rid, hist in histories.items():
        for pos in range(prompt_lens[rid], len(hist)):
            rows = row_of.get((rid, pos - 1))
            assert rows, ("no logits row", rid, pos - 1)
            for row in rows:
                assert float(row[hist[pos]]) == float(row.max()), \
                    ("emitted token is not the argmax", rid, pos)


def long_prompt(n: int, salt: int = 0, alphabet: int = 23) -> List[int]:
    """n tokens of a small alphabet, so that tokens repeat throughout the
    context, behind the sink tokens every prompt begins with."""
    ns = len(SINK_TOKENS)
    sinks = [SINK_TOKENS[(5 * salt + 3 * j) % ns] for j in range(N_SINKS)]
    body = [(7 * i * i + 3 * (salt + 1) + salt * i) % alphabet + 29 * salt
            for i in range(n - N_SINKS)]
    return sinks + body


# ---- scenarios ------------------------------------------------------------

def _req(rid, prompt, max_tokens):
    return EngineRequest(rid, prompt_tokens=list(prompt),
                         max_tokens=max_tokens)


SHARED_PREFIX = long_prompt(64, salt=1)


def scenario_a():
    """Mixed traffic: b (560 tokens, decode beyond 512: the split kernel)
    prefills first in 48-token chunks; a (a 64-token prefix plus a tail,
    109 tokens, decodes across the block edge at 112) follows it; c arrives
    at step 6 with the same prefix, finds it in the prefix cache, and ends
    its prompt on a one-token chunk."""
    a = SHARED_PREFIX + [(5 * i + 11) % 23 + 40 for i in range(45)]
    c = SHARED_PREFIX + [(3 * i * i + 2) % 23 + 70 for i in range(52)]
    return dict(
        worker=dict(kv_blocks=256, prefill_chunk_tokens=48),
        arrivals=[(0, _req("b", long_prompt(560), 14)),
                  (0, _req("a", a, 6)),
                  (6, _req("c", c, 4))])


def scenario_b():
    """Row reuse and growth: a decode state of 4 rows, requests of 20 to
    200 tokens with 2 to 10 output tokens, staggered so that short ones
    finish and later ones take their rows while more than 4 run."""
    lens = [200, 150, 37, 96, 23, 180, 20, 31, 64, 120]
    outs = [10, 2, 3, 9, 6, 8, 4, 5, 6, 7]
    at = [0, 0, 0, 0, 3, 4, 5, 6, 7, 8]
    arrivals = [(at[i], _req(f"r{i}", long_prompt(lens[i], salt=i + 2),
                             outs[i])) for i in range(len(lens))]
    return dict(worker=dict(kv_blocks=256, max_decode_batch=4,
                            prefill_chunk_tokens=256),
                arrivals=arrivals)


def scenario_c():
    """Preemption and recompute: three 80-token prompts with 40 output
    tokens each need 3 * 8 blocks. A pool of 24 holds them all, so nothing
    is ever preempted; 20 blocks run out while they decode."""
    arrivals = [(0, _req(f"p{i}", long_prompt(80, salt=i + 13), 40))
                for i in range(3)]
    return dict(worker=dict(kv_blocks=20), arrivals=arrivals)


SCENARIOS = {"A": scenario_a, "B": scenario_b, "C": scenario_c}

# The worst row error of the bf16 CPU worker (ops.ref) per scenario, as
# measured (7.43e-3, 7.96e-3, 7.86e-3) and rounded up to two digits; the
# device limit is LIMIT_FACTOR times it.
CPU_WORST = {"A": 0.0075, "B": 0.0080, "C": 0.0079}
LIMIT_FACTOR = 4.0


def limit(scenario: str) -> float:
    return LIMIT_FACTOR * CPU_WORST[scenario]


@dataclass
class Result:
    worker: EngineWorker
    rec: Recorder
    hist: Dict[str, List[int]]
    worst: Dict[str, float]
    plens: Dict[str, int]
    reqs: Dict[str, EngineRequest]

    def __iter__(self):
        return iter((self.worker, self.rec, self.hist, self.worst,
                     self.plens))


def run(name: str, device, dtype=torch.bfloat16, mutate=None,
        setup=None) -> Result:
    """Run a scenario on a fresh worker and judge it."""
    sc = SCENARIOS[name]()
    worker = make_worker(device, dtype, **sc["worker"])
    if setup is not None:
        setup(worker)
    reqs = {r.request_id: r for _, r in sc["arrivals"]}
    plens = {rid: len(r.prompt_tokens) for rid, r in reqs.items()}
    rec, hist = run_scenario(worker, sc["arrivals"], mutate=mutate)
    worst = judge(rec.records, hist, worker.model)
    return Result(worker, rec, hist, worst, plens, reqs)


# ---- what each scenario must have reached -----------------------------------

def check_scenario_a(res: Result) -> None:
    from llm_d_inference_scheduler_amd.ops.dispatch import split_geometry
    recs = res.rec.records
    pre = [r for r in recs if not r.is_decode]
    dec = [r for r in recs if r.is_decode]
    spans = [s for r in pre for s in r.spans]
    assert any(len(r.spans) >= 2 for r in pre), "no multi-sequence launch"
    assert any(rid == "b" and start > 0 for rid, start, _, _ in spans), \
        "no continuation chunk"
    # c's first chunk starts behind the prefix the cache supplied
    assert [s for s in spans if s[0] == "c"][0][1] == 64
    fin = {o.request_id: o for o in res.rec.outputs if o.finished}
    assert fin["c"].cached_tokens == 64
    assert fin["a"].cached_tokens == 0
    assert any(end - start == 1 and start > 0 for _, start, end, _ in spans), \
        "no one-token tail"
    # a's decode writes the first slot of a block it had to allocate
    a_pos = [pos for r in dec for rid, pos in r.rows if rid == "a"]
    assert min(a_pos) < 112 <= max(a_pos), a_pos
    assert any({rid for rid, _ in r.rows} == {"a", "b", "c"} for r in dec), \
        "no decode batch mixing the long and the two short rows"
    # every decode step holds b beyond 512 tokens: the split kernel and its
    # combine are what runs on the device
    assert dec
    for r in dec:
        assert "b" in {rid for rid, _ in r.rows}
        assert r.max_seq_len > 512
        assert split_geometry(len(r.rows) * CONFIG.num_kv_heads,
                              r.max_seq_len) is not None


def check_scenario_b(res: Result) -> None:
    st = res.worker.dstate
    assert st.capacity > 4, "the decode state never grew"
    # a row was reused by a request shorter than the one that left it: the
    # row's block table still holds the longer table's tail
    occupants: Dict[int, List[str]] = {}
    for r in res.rec.records:
        if r.is_decode:
            assert len(r.rows) <= 4
            for (rid, _), row in zip(r.rows, r.dstate_rows):
                occ = occupants.setdefault(row, [])
                if not occ or occ[-1] != rid:
                    occ.append(rid)
    assert any(len(res.hist[x]) > len(res.hist[y]) + 16
               for occ in occupants.values()
               for x, y in zip(occ, occ[1:])), occupants
    # rows that were live when the state grew went on decoding afterwards
    assert any(row >= 4 for row in occupants), occupants


def check_scenario_c(res: Result) -> None:
    # _preempt folds the generation into the prompt
    victims = [rid for rid, r in res.reqs.items()
               if r.prompt_len > r.orig_prompt_len]
    assert victims, "no request was preempted"
    for rid in victims:
        # the recompute: a prefill that starts over after decode rows, and
        # decode rows after it
        kinds = [(r.is_decode, start) for r in res.rec.records
                 for srid, start, _, _ in r.spans if srid == rid]
        first_dec = kinds.index(next(k for k in kinds if k[0]))
        redo = [i for i, k in enumerate(kinds)
                if i > first_dec and not k[0]]
        assert redo, kinds
        assert any(k[0] for k in kinds[redo[-1]:]), kinds
    fin = {o.request_id: o for o in res.rec.outputs if o.finished}
    assert all(len(res.hist[rid]) - res.plens[rid] ==
               res.reqs[rid].max_tokens for rid in fin)
