"""Inputs, the float64 reference, a rounding emulation and its mutants for
the batched LoRA kernels (ops.lora_add; DEVELOPMENT.md "LoRA adapters").

Plain CPU Python, shared by tests/test_lora_cases.py (CPU proof) and
tests/test_gpu_lora.py (GPU tier), in the manner of kernel_cases.py.

Inputs: `in` = 256 and `out` = 512 unless a case says otherwise. x rows with
no adapter and every slot no row uses hold NaN, so a kernel that reads either
shows it. y starts as randn. A is randn / sqrt(in) and B is randn * 4 /
sqrt(rank), so an adapter's update has elements of about N(0, 4^2) next to a
y of N(0, 1): a dropped, misplaced or half-summed update is an O(1) relative
error of the update. perm is shuffled inside each slot group, which the work
list allows and which tells a gather through perm from contiguous rows.

Metric: per adapter row, relative L2 of (y_after - y_before) against the
float64 update computed from the bf16-rounded inputs. The limit of a case is
4x the worst row of the rounding emulation (fp32 accumulation, the
intermediate rounded to bf16, bf16 read-add-round of y), never below 2^-8.
"""
import dataclasses
import functools
from typing import List, Optional

import torch

from llm_d_inference_scheduler_amd.ops import ref

FLOOR = 2.0 ** -8
MARGIN = 4.0
MUTANT_FACTOR = 10.0
KCHUNK = 1024      # LORA_KCHUNK of csrc/hip/launchers.h: `in` columns per split
NBLOCK = 256       # LORA_NBLOCK: `out` columns per expand workgroup
BF16 = torch.bfloat16


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    T: int
    row_slot: tuple            # per row: slot, -1 = no adapter
    S: int
    R: int = 16
    rank: int = 16             # the adapters' own rank, zero-padded to R
    n_in: int = 256
    n_out: int = 512


def _pattern(T):
    base = [2, -1, 0, 0, 2, 1]
    return tuple(base[i % len(base)] for i in range(T))


SPECS = [
    Spec("a_T1", 1, (0,), S=2),
    Spec("b_T17", 17, (0,) * 17, S=2),
    Spec("c_T40_mixed", 40, _pattern(40), S=4),
    Spec("d_longK", 3, (1, 1, 1), S=2, n_in=14336, n_out=4096),
    Spec("e_out48", 5, (0, -1, 0, 0, -1), S=2, n_out=48),
    Spec("f_rank8_R16", 6, (1, 0, -1, 1, 0, 0), S=3, R=16, rank=8),
    Spec("f_rank64_R64", 19, (0,) * 10 + (-1,) + (1,) * 8, S=3, R=64,
         rank=64),
]
NAMES = [s.name for s in SPECS]


@dataclasses.dataclass
class Case:
    spec: Spec
    x: torch.Tensor        # [T, in] bf16, NaN rows where no adapter
    y0: torch.Tensor       # [T, out] bf16
    A: torch.Tensor        # [S, R, in] bf16, NaN in unused slots
    B: torch.Tensor        # [S, out, R] bf16
    perm: torch.Tensor     # int32
    tiles: torch.Tensor    # [n, 3] int32
    delta64: torch.Tensor  # [T, out] float64, zero outside perm
    limit: float
    emu_worst: float


def row_slot_of(perm, tiles, T) -> List[int]:
    rs = [-1] * T
    for start, count, slot in tiles.tolist():
        for r in perm[start:start + count].tolist():
            rs[r] = slot
    return rs


def _shuffle_groups(perm, tiles, gen):
    """Shuffle the rows of each slot group of perm: tiles stay as they are."""
    perm = perm.clone()
    t = tiles.tolist()
    i = 0
    while i < len(t):
        j = i
        while j < len(t) and t[j][2] == t[i][2]:
            j += 1
        lo, hi = t[i][0], t[j - 1][0] + t[j - 1][1]
        perm[lo:hi] = perm[lo:hi][torch.randperm(hi - lo, generator=gen)]
        i = j
    return perm


def reference64(x, A, B, perm, tiles, T):
    """The exact update of every adapter row, from the stored tensors."""
    out = torch.zeros(T, B.shape[1], dtype=torch.float64)
    for start, count, slot in tiles.tolist():
        rows = perm[start:start + count].long()
        out[rows] = (x[rows].double() @ A[slot].double().T) \
            @ B[slot].double().T
    return out


def row_errors(y_after, case) -> torch.Tensor:
    """Relative L2 of the applied update per adapter row (float64); a
    non-finite row counts as infinitely wrong."""
    rows = case.perm.long()
    d = (y_after.double() - case.y0.double())[rows]
    want = case.delta64[rows]
    err = (d - want).norm(dim=1) / want.norm(dim=1)
    return torch.where(torch.isfinite(d).all(dim=1), err,
                       torch.full_like(err, float("inf")))


MUTANTS = ["neighbour_slot", "perm_ignored", "tail_row_dropped",
           "last_split_dropped", "upper_R_dropped", "column_block_shifted"]


def emulate(c, mutant: Optional[str] = None) -> Optional[torch.Tensor]:
    """y after the kernels' rounding points on the CPU. With `mutant`, one
    fault is built in; None is returned where that fault changes nothing on
    this case (then the case cannot tell it apart, and does not claim to)."""
    sp = c.spec
    y = c.y0.clone()
    tiles = c.tiles.tolist()
    if mutant == "perm_ignored" and torch.equal(
            c.perm, torch.arange(len(c.perm), dtype=torch.int32)):
        return None
    if mutant == "upper_R_dropped" and sp.rank <= sp.R // 2:
        return None
    if mutant == "tail_row_dropped" and all(t[1] == 16 for t in tiles):
        return None
    k_end = sp.n_in
    if mutant == "last_split_dropped":
        k_end = (sp.n_in - 1) // KCHUNK * KCHUNK
    r_end = sp.R // 2 if mutant == "upper_R_dropped" else sp.R
    first = True
    for start, count, slot in tiles:
        rows = c.perm[start:start + count].long()
        src = rows
        if mutant == "perm_ignored":
            src = torch.arange(start, start + count)
        if mutant == "tail_row_dropped" and count < 16:
            rows, src = rows[:-1], src[:-1]
        xs = c.x[src].float()
        delta = torch.zeros(len(rows), sp.n_out)
        for i in range(len(rows)):
            s = slot
            if mutant == "neighbour_slot" and first and i == 0:
                s = (slot + 1) % sp.S
            tmp = xs[i, :k_end] @ c.A[s].float()[:, :k_end].T
            tmp = tmp.to(BF16).float()
            delta[i] = tmp[:r_end] @ c.B[s].float()[:, :r_end].T
        first = False
        if mutant == "column_block_shifted":
            delta = torch.roll(delta, NBLOCK if sp.n_out > NBLOCK else 16, 1)
        y[rows] = (y[rows].float() + delta).to(BF16)
    return y


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    sp = SPECS[NAMES.index(name)]
    gen = torch.Generator().manual_seed(1000 + NAMES.index(name))
    nan = float("nan")
    x = torch.randn(sp.T, sp.n_in, generator=gen)
    y0 = torch.randn(sp.T, sp.n_out, generator=gen).to(BF16)
    A = torch.randn(sp.S, sp.R, sp.n_in, generator=gen) / sp.n_in ** 0.5
    B = torch.randn(sp.S, sp.n_out, sp.R, generator=gen) * 4 / sp.rank ** 0.5
    A[:, sp.rank:] = 0.0
    B[:, :, sp.rank:] = 0.0
    used = {s for s in sp.row_slot if s >= 0}
    for s in range(sp.S):
        if s not in used:
            A[s], B[s] = nan, nan
    for r, s in enumerate(sp.row_slot):
        if s < 0:
            x[r] = nan
    x, A, B = x.to(BF16), A.to(BF16), B.to(BF16)
    perm, tiles = ref.lora_worklist(sp.row_slot)
    perm = _shuffle_groups(perm, tiles, gen)
    assert row_slot_of(perm, tiles, sp.T) == list(sp.row_slot)
    c = Case(sp, x, y0, A, B, perm, tiles,
             reference64(x, A, B, perm, tiles, sp.T), 0.0, 0.0)
    c.emu_worst = float(row_errors(emulate(c), c).max())
    c.limit = max(FLOOR, MARGIN * c.emu_worst)
    return c


def single_row(c: Case, row: int):
    """The T = 1 launch of one adapter row of c at row index 0: (x, y0, perm,
    tiles) with c's pools."""
    slot = row_slot_of(c.perm, c.tiles, c.spec.T)[row]
    return (c.x[row:row + 1].clone(), c.y0[row:row + 1].clone(),
            torch.zeros(1, dtype=torch.int32),
            torch.tensor([[0, 1, slot]], dtype=torch.int32))
