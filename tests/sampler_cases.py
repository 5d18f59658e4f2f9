"""Inputs of the sampler tests, shared by the CPU and the GPU tier
(DEVELOPMENT.md "Sampling").

A case is one logits shape [B, V] run over every combination of
T in {0, 0.3, 1.0, 1.5}, k in {0, 1, 50} and p in {1.0, 0.9, 0.5}: 36 rows,
B per launch, fresh `randn * 4` logits rounded to the dtype for every launch
(so bf16 rows are full of ties), a different seed and position per row. The
reference runs once per case and is cached.

Rows on which fp32 rounding decides the answer are named here, from the
reference alone:
  * token: the two best perturbed scores differ by less than
    16 * ulp32(max(32, max|z|)). logf is good to about 1 ulp and |g| stays
    under about 17, so the error of g is a few 1e-6; the margin is roughly
    ten times that.
  * kept set: the cumulative mass on either side of the chosen top-p
    boundary is within 1e-4 * W of p * W. Masses are summed exactly (2^-32
    fixed point); what differs between two implementations is expf.
"""
import functools
import itertools
import math

import torch

from llm_d_inference_scheduler_amd.ops import ref

TEMPS = (0.0, 0.3, 1.0, 1.5)
TOP_KS = (0, 1, 50)
TOP_PS = (1.0, 0.9, 0.5)
COMBOS = list(itertools.product(TEMPS, TOP_KS, TOP_PS))

# (V, B, dtype, generator seed). Seeds were picked on the CPU, with the
# reference alone, so that no row of a case is undecided
# (tests/test_sampler.py::test_case_seeds_leave_rows_decided).
SHAPES = [
    (100, 3, torch.bfloat16, 11),
    (1001, 3, torch.bfloat16, 11),
    (1024, 5, torch.float32, 13),
    (32064, 2, torch.bfloat16, 21),
    (151936, 2, torch.bfloat16, 14),
]
MAX_UNDECIDED_SHARE = 0.02
MASS_MARGIN = 1e-4


def ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23)


class Launch:
    def __init__(self, logits, temperature, top_k, top_p, seed, pos):
        self.logits = logits
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        self.seed, self.pos = seed, pos
        (self.tokens, self.logprobs, self.n_kept, self.threshold,
         self.details) = ref.sample(logits, temperature, top_k, top_p, seed,
                                    pos, details=True)
        self.token_undecided = [
            d["score_gap"] < 16 * ulp32(max(32.0, d["max_abs_z"]))
            for d in self.details]
        self.kept_undecided = [d["mass_margin"] < MASS_MARGIN
                               for d in self.details]

    def args(self, device):
        return tuple(t.to(device) for t in (
            self.logits, self.temperature, self.top_k, self.top_p,
            self.seed, self.pos))


@functools.lru_cache(maxsize=None)
def make_case(V, B, dtype, gen_seed):
    """The launches of one shape: ceil(36 / B) of them, B rows each."""
    g = torch.Generator().manual_seed(gen_seed)
    launches = []
    combos = COMBOS + COMBOS[:(-len(COMBOS)) % B]
    for i in range(0, len(combos), B):
        rows = combos[i:i + B]
        logits = (torch.randn(B, V, generator=g) * 4).to(dtype)
        launches.append(Launch(
            logits,
            torch.tensor([c[0] for c in rows], dtype=torch.float32),
            torch.tensor([c[1] for c in rows], dtype=torch.int32),
            torch.tensor([c[2] for c in rows], dtype=torch.float32),
            torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g,
                          dtype=torch.int64),
            torch.randint(0, 4096, (B,), generator=g, dtype=torch.int32)))
    return launches


def undecided_share(launches) -> float:
    rows = sum(len(l.details) for l in launches)
    und = sum(a or b for l in launches
              for a, b in zip(l.token_undecided, l.kept_undecided))
    return und / rows
