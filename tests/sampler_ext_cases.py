"""Inputs of the sample_ext / token_state_fill tests, shared by the CPU and
the GPU tier (DEVELOPMENT.md "Sampling"), in the style of sampler_cases.py.

A case is one logits shape [B, V] of sampler_cases.SHAPES. Its rows cross
the new parameters
    rep in {1, 1.3, 0.8}, freq in {0, 0.7, -0.5}, pres in {0, 1.1},
    min_p in {0, 0.05, 0.5}, top_n in {0, 1, 5, 20}          (216 combinations)
with the T/k/p grid of sampler_cases (36 combinations) and six token
histories. The full product is 46656 rows per shape and the reference takes
about 10 ms per row at the real vocabulary, so: shapes with V <= 1024 run
all 216 combinations of the new parameters, row i taking T/k/p combination
(i + i // 6) % 36 and history (i + i // 6) % 6, so that every value of a
new parameter meets every T/k/p combination and every history
(test_sampler_ext.py::test_small_cases_cross_every_pair_of_values); the two
large vocabularies run 36 rows, T/k/p combination i with new-parameter
combination (7 * i + shape offset) % 216 (7 is coprime to 216, so the 36 are
spread over the product).

Histories (built with the reference's token_state_fill from a prompt and an
output list):
  none    state_row = -1
  empty   a state row of zeros
  one     one output token
  big     about 700 output tokens: one id 600 times, 50 pairs 2j, 2j+1
  both    one token in the prompt and twice in the output, with other
          prompt-only and output-only tokens
  argmax  the row's own argmax three times in the output and its runner-up
          in the prompt, so that greedy flips when a penalty is on

State rows are assigned in reverse (row r of a launch uses state row B - r);
state row 0 belongs to nobody, holds junk and must come back unchanged.

A row is undecided when sampler_cases' criteria say so, or when the nearest
z_i lies within 16 * ulp32(max(32, max|z|)) of tau_m: z_i and tau_m are each
a few fp32 operations from their inputs and implementations agree on them
bit for bit only by contract, so the margin is the one already used for the
perturbed scores."""
import functools
import itertools

import torch

import sampler_cases as sc
from llm_d_inference_scheduler_amd.ops import ref

REPS = (1.0, 1.3, 0.8)
FREQS = (0.0, 0.7, -0.5)
PRESS = (0.0, 1.1)
MIN_PS = (0.0, 0.05, 0.5)
TOP_NS = (0, 1, 5, 20)
NEW_COMBOS = list(itertools.product(REPS, FREQS, PRESS, MIN_PS, TOP_NS))
HISTORIES = ("none", "empty", "one", "big", "both", "argmax")
N_TOP = 20
JUNK = 0x1234

# (V, B, dtype, generator seed). Seeds were picked on the CPU, with the
# reference alone, so that no row of a case is undecided
# (tests/test_sampler_ext.py::test_case_seeds_leave_rows_decided).
SHAPES = [
    (100, 3, torch.bfloat16, 1),
    (1001, 3, torch.bfloat16, 10),
    (1024, 5, torch.float32, 3),
    (32064, 2, torch.bfloat16, 1),
    (151936, 2, torch.bfloat16, 2),
]
MAX_UNDECIDED_SHARE = sc.MAX_UNDECIDED_SHARE


def row_plan(V, shape_index):
    """[(T, k, p, rep, freq, pres, min_p, top_n, history)] of one shape."""
    rows = []
    if V <= 1024:
        for i, new in enumerate(NEW_COMBOS):
            tkp = sc.COMBOS[(i + i // 6) % 36]
            rows.append(tkp + new + (HISTORIES[(i + i // 6) % 6],))
    else:
        for i, tkp in enumerate(sc.COMBOS):
            new = NEW_COMBOS[(7 * i + 31 * shape_index) % len(NEW_COMBOS)]
            rows.append(tkp + new + (HISTORIES[(i + i // 6) % 6],))
    return rows


def history(kind, logits_row, g):
    """(prompt ids, output ids) of one row."""
    V = logits_row.shape[0]

    def rnd(n):
        return torch.randint(0, V, (n,), generator=g).tolist()

    if kind in ("none", "empty"):
        return [], []
    if kind == "one":
        return [], rnd(1)
    if kind == "big":
        a = rnd(1)[0]
        pairs = [t for j in rnd(50) for t in (j & ~1, (j & ~1) + 1)
                 if (j & ~1) + 1 < V]
        out = [a] * 600 + pairs
        perm = torch.randperm(len(out), generator=g).tolist()
        return [], [out[i] for i in perm]
    if kind == "both":
        t = rnd(1)[0]
        return rnd(5) + [t], [t] + rnd(4) + [t]
    top2 = torch.topk(logits_row.float(), 2).indices.tolist()
    return [top2[1]], [top2[0]] * 3


class Launch:
    def __init__(self, logits, plan, g):
        B, V = logits.shape
        f32, i32 = torch.float32, torch.int32
        col = lambda j, dt: torch.tensor([p[j] for p in plan], dtype=dt)
        self.logits = logits
        self.plan = plan
        self.temperature, self.top_k, self.top_p = (
            col(0, f32), col(1, i32), col(2, f32))
        self.rep, self.freq, self.pres, self.min_p, self.top_n = (
            col(3, f32), col(4, f32), col(5, f32), col(6, f32), col(7, i32))
        self.seed = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g,
                                  dtype=torch.int64)
        self.pos = torch.randint(0, 4096, (B,), generator=g, dtype=i32)
        self.state_row = torch.tensor(
            [-1 if p[8] == "none" else B - r for r, p in enumerate(plan)],
            dtype=i32)
        state = ref.token_state_alloc(B + 1, V, "cpu")
        state[0] = JUNK
        state[:, V:] = JUNK                 # padding: never read or written
        self.histories = [history(p[8], logits[r], g)
                          for r, p in enumerate(plan)]
        used = [r for r in range(B) if plan[r][8] != "none"]
        toks, offs, n_p = [], [0], []
        for r in used:
            pr, out = self.histories[r]
            toks += pr + out
            offs.append(len(toks))
            n_p.append(len(pr))
        self.fill_args = (self.state_row[used].contiguous(),
                          torch.tensor(toks, dtype=i32),
                          torch.tensor(offs, dtype=torch.int64),
                          torch.tensor(n_p, dtype=i32), V)
        ref.token_state_fill(state, *self.fill_args)
        self.state_before = state
        self.state_after = state.clone()
        (self.tokens, self.logprobs, self.n_kept, self.threshold,
         self.top_tokens, self.top_logprobs, self.details) = ref.sample_ext(
            *self._args(self.state_after), n_top=N_TOP, details=True)
        self.token_undecided = [
            d["score_gap"] < 16 * sc.ulp32(max(32.0, d["max_abs_z"]))
            for d in self.details]
        self.kept_undecided = [
            d["mass_margin"] < sc.MASS_MARGIN or
            d["minp_margin"] < 16 * sc.ulp32(max(32.0, d["max_abs_z"]))
            for d in self.details]

    def _args(self, state):
        return (self.logits, self.temperature, self.top_k, self.top_p,
                self.seed, self.pos, self.rep, self.pres, self.freq,
                self.min_p, self.top_n, self.state_row, state)

    def args(self, device):
        """Arguments of sample_ext on `device`, with a fresh copy of the
        state as it is before the call (the last element)."""
        return tuple(t.to(device) for t in
                     self._args(self.state_before.clone()))


@functools.lru_cache(maxsize=None)
def make_case(V, B, dtype, gen_seed):
    g = torch.Generator().manual_seed(gen_seed)
    si = [s[0] for s in SHAPES].index(V)
    plan = row_plan(V, si)
    plan = plan + plan[:(-len(plan)) % B]
    launches = []
    for i in range(0, len(plan), B):
        logits = (torch.randn(B, V, generator=g) * 4).to(dtype)
        launches.append(Launch(logits, plan[i:i + B], g))
    return launches


def undecided_share(launches) -> float:
    return sc.undecided_share(launches)
