"""Inputs, float64 references and the error metric for the kernel edge tests.

Plain CPU Python, shared by tests/test_kernel_cases.py (CPU tier) and
tests/test_gpu_kernel_edges.py (GPU tier). Independent of ops/ref.py, so the
project's own fp32 reference is cross-checked against this module once.

Needle inputs: K rows are randn; a needle query row is 1.5 * k_j for one
target token j, so at D=128 the target logit is about 17 against N(0, 1.5^2)
for every other token and the output row is essentially v_j. A wrong, missing,
duplicated or stale token gives an O(1) row error instead of an O(1/S) one.

Poisoned pool: every cache row the operation may not read (block 0, blocks in
no table, rows at or beyond ctx in a last block) holds NaN (bf16) or 448
(fp8 e4m3 max); block-table columns beyond a sequence's blocks point at the
poisoned block 0.

Metric: per-row relative L2 error against float64 over every output row. The
limit of a case is 4x the worst row error of a rounding emulation of the
kernel on that case (fp32 accumulation, P rounded to bf16 before P.V for the
flash kernels, bf16 output), never below 2^-8 (one bf16 output rounding step).
"""
import dataclasses
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

D = 128
BS = 16
TILE = 32                    # KV tile of the glds flash kernel
FLOOR = 2.0 ** -8            # one bf16 output rounding step
MARGIN = 4.0                 # accumulation order + __expf
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0

# (chunk, prior) of the flash-prefill launch; see DEVELOPMENT.md
PREFILL_SEQS = [(1, 300), (5, 0), (32, 0), (64, 0), (96, 0), (97, 31),
                (33, 95), (600, 171), (257, 1500)]
DECODE_SEQS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025, 2049]


def split_seqs(np_: int, part: int) -> List[int]:
    return [1, part, part + 1, 2 * part - 1, 2 * part + 1, np_ * part]


# ---------------------------------------------------------------------------
# quantisation and the poisoned pool
# ---------------------------------------------------------------------------

def quantise(x: torch.Tensor, kv_dtype: str) -> torch.Tensor:
    """fp32 tensor holding only values representable in the cache dtype."""
    if kv_dtype == "bf16":
        return x.bfloat16().float()
    return x.clamp(-FP8_MAX, FP8_MAX).to(FP8).float()


def to_cache(xf: torch.Tensor, kv_dtype: str) -> torch.Tensor:
    return xf.bfloat16() if kv_dtype == "bf16" else xf.to(FP8)


def cache_to_f64(c: torch.Tensor) -> torch.Tensor:
    return c.float().double()


def poison_value(kv_dtype: str) -> float:
    return float("nan") if kv_dtype == "bf16" else FP8_MAX


def _build_pool(gen, n_tokens: List[int], kvh: int, kv_dtype: str,
                spare: int = 3):
    """Shuffled block table + clean fp32 K/V pools + the [NB, BS] mask of
    rows the operation may read."""
    nbs = [(n + BS - 1) // BS for n in n_tokens]
    NB = 1 + sum(nbs) + spare
    perm = torch.randperm(NB - 1, generator=gen) + 1
    bt = torch.zeros(len(n_tokens), max(max(nbs), 1), dtype=torch.int32)
    valid = torch.zeros(NB, BS, dtype=torch.bool)
    k = 0
    for i, (n, nb) in enumerate(zip(n_tokens, nbs)):
        ids = perm[k:k + nb]
        k += nb
        bt[i, :nb] = ids.to(torch.int32)
        valid[ids] = (torch.arange(nb * BS) < n).view(nb, BS)
    kf = quantise(torch.randn(NB, kvh, BS, D, generator=gen), kv_dtype)
    vf = quantise(torch.randn(NB, kvh, BS, D, generator=gen), kv_dtype)
    assert not valid[0].any(), "block 0 must stay out of every table"
    return bt, valid, kf, vf


def _poisoned_cache(xf: torch.Tensor, valid: torch.Tensor, kv_dtype: str):
    x = xf.clone()
    x.permute(0, 2, 1, 3)[~valid] = poison_value(kv_dtype)
    return to_cache(x, kv_dtype)


def gather_tokens(cache_f: torch.Tensor, bt_row: torch.Tensor, n: int):
    """[NB, KVH, BS, D] -> the first n tokens of one sequence, [KVH, n, D]."""
    nb = (n + BS - 1) // BS
    blocks = bt_row[:nb].long()
    kvh = cache_f.shape[1]
    return cache_f[blocks].permute(1, 0, 2, 3).reshape(kvh, nb * BS, -1)[:, :n]


# ---------------------------------------------------------------------------
# the attention maths: float64, or the kernels' rounding points in fp32
# ---------------------------------------------------------------------------

def attend(q, k, v, prior: int, scale: float, *, emulate: Optional[str] = None,
           mask_shift: int = 0, drop: Optional[torch.Tensor] = None):
    """Causal attention of q [KVH, G, C, D] over k, v [KVH, S, D]: row t sees
    keys s <= prior + t + mask_shift, minus the columns flagged in drop [S].
    emulate=None is float64; "flash" and "decode" are fp32 accumulation with
    bf16 output, "flash" also rounding P to bf16 before P.V. A row that sees
    nothing gives zeros (the kernels' l == 0 case). Returns float64."""
    dt = torch.float64 if emulate is None else torch.float32
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    C, S = q.shape[2], k.shape[1]
    s = torch.einsum("hgtd,hsd->hgts", q, k) * scale
    hidden = (torch.arange(S).view(1, -1) >
              torch.arange(C).view(-1, 1) + prior + mask_shift)
    if drop is not None:
        hidden = hidden | drop.view(1, -1)
    s = s.masked_fill(hidden.view(1, 1, C, S), float("-inf"))
    m = s.amax(dim=-1, keepdim=True) if S else s.new_zeros(*s.shape[:3], 1)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    if emulate == "flash":
        p = p.bfloat16().float()
    o = torch.einsum("hgts,hsd->hgtd", p, v)
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    if emulate is not None:
        o = o.bfloat16()
    return o.double()


def row_rel_err(out: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """||out_r - ref_r|| / ||ref_r|| per row of [..., D]; a non-finite output
    row counts as infinitely wrong. A reference row that is exactly zero is
    judged by exact equality (error 0 or inf)."""
    out, ref = out.double(), ref.double()
    num = (out - ref).norm(dim=-1)
    den = ref.norm(dim=-1)
    err = num / den
    err = torch.where(den == 0, torch.where(num == 0, 0.0, math.inf), err)
    return torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))


def limit_from(emul: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(limit, worst emulation row error) of one case."""
    worst = float(row_rel_err(emul, ref).max())
    assert math.isfinite(worst), "the emulation itself must be finite"
    return max(MARGIN * worst, FLOOR), worst


# ---------------------------------------------------------------------------
# flash prefill cases
# ---------------------------------------------------------------------------

def _is_diffuse(p: int, g: int, qpg: int) -> bool:
    """Every fourth virtual row v = p*QPG + g stays randn. Where QPG is a
    multiple of 4 the phase moves with p, so no q-head is diffuse throughout."""
    v = p * qpg + g
    return (v + (p if qpg % 4 == 0 else 0)) % 4 == 3


def _take(pool: List[int], vis: int) -> Optional[int]:
    """Largest entry <= vis of a descending list, removed from it."""
    for i, t in enumerate(pool):
        if t <= vis:
            return pool.pop(i)
    return None


def prefill_targets(chunk: int, prior: int, qpg: int, kvh: int, rng):
    """Needle target per (position, q-head), -1 for diffuse rows.

    Needle rows alternate between own position, own position - 1 and a
    wanted token: first the last token of every 32-token tile no row aims at
    yet, then the other tile lasts, the tile firsts (token 0 among them), the
    first and last row of every 16-token block, then random visible tokens.
    Wanted tokens are handed out from the last row backwards, each row taking
    the largest one it may see. Returns (targets [chunk, QH], uncovered tiles).
    """
    ctx = chunk + prior
    n_tiles = (ctx + TILE - 1) // TILE
    tgt = torch.full((chunk, kvh * qpg), -1, dtype=torch.int64)
    rows = [(p, g, kh) for p in range(chunk) for g in range(qpg)
            for kh in range(kvh) if not _is_diffuse(p, g, qpg)]
    assert rows, "a sequence needs at least one needle row"
    hit, free = set(), []
    # a sequence short of rows (one new token after a long prior) keeps one
    # row each for own position and own position - 1, the rest go to tiles
    scarce = len(rows) < 4 * n_tiles
    for c, (p, g, kh) in enumerate(rows):
        own = prior + p
        if c % 4 == 0 and (c == 0 or not scarce):
            t = own
        elif c % 4 == 1 and (c == 1 or not scarce):
            t = max(own - 1, 0)
        else:
            free.append((p, g, kh))
            continue
        tgt[p, kh * qpg + g] = t
        hit.add(t)
    own_tiles = {t // TILE for t in hit}
    tile_last = [min(TILE * n + TILE - 1, ctx - 1) for n in range(n_tiles)]
    tile_first = [TILE * n for n in range(n_tiles)]
    edges = {e for b in range((ctx + BS - 1) // BS)
             for e in (BS * b, min(BS * b + BS - 1, ctx - 1))}
    pools = [
        [t for t in tile_last if t // TILE not in own_tiles],
        [t for t in tile_last if t // TILE in own_tiles and t not in hit],
        [t for t in tile_first if t not in hit and t not in tile_last],
        [t for t in edges if t not in hit and t not in tile_last
         and t not in tile_first],
    ]
    pools = [sorted(set(pl), reverse=True) for pl in pools]
    n_needed = len(pools[0])
    for (p, g, kh) in reversed(free):
        vis = prior + p
        t = None
        for pl in pools:
            t = _take(pl, vis)
            if t is not None:
                break
        if t is None:
            t = int(rng.integers(0, vis + 1))
        tgt[p, kh * qpg + g] = t
        hit.add(t)
    covered = {t // TILE for t in hit}
    uncovered = [n for n in range(n_tiles) if n not in covered]
    # coverage: every tile of [0, ctx) is some needle's target, unless the
    # sequence has fewer free needle rows than tiles still wanting one
    assert not uncovered or len(free) < n_needed, (
        f"(chunk={chunk}, prior={prior}, qpg={qpg}): tiles {uncovered} have "
        f"no needle although {len(free)} rows were free for {n_needed}")
    # a needle never aims past its own causal horizon
    vis_all = prior + torch.arange(chunk).view(-1, 1)
    assert bool(((tgt <= vis_all) | (tgt < 0)).all())
    return tgt, uncovered


@dataclasses.dataclass
class PrefillCase:
    qpg: int
    kvh: int
    kv_dtype: str
    seqs: List[Tuple[int, int]]
    q: torch.Tensor                 # [T, QH, D] bf16
    k_cache: torch.Tensor           # [NB, KVH, BS, D] bf16 | fp8, poisoned
    v_cache: torch.Tensor
    block_tables: torch.Tensor      # [n_seqs, W] int32
    metas: List[Tuple[int, int, int]]   # (start, chunk, prior)
    tiles: List[Tuple[int, int]]        # (seq, first virtual row)
    scale: float
    targets: List[torch.Tensor]
    uncovered: dict
    _cache: dict = dataclasses.field(default_factory=dict)

    def widened(self, width: int) -> torch.Tensor:
        """The block table zero-padded to `width` columns; the padding
        points at the poisoned block 0."""
        bt = torch.zeros(len(self.seqs), width, dtype=torch.int32)
        bt[:, :self.block_tables.shape[1]] = self.block_tables
        return bt

    def reference(self):
        if "ref" not in self._cache:
            self._cache["ref"] = prefill_reference(self)
        return self._cache["ref"]

    def limit(self):
        if "limit" not in self._cache:
            self._cache["limit"] = limit_from(
                prefill_reference(self, emulate="flash"), self.reference())
        return self._cache["limit"]


def make_prefill_case(qpg: int, seqs=None, kvh: int = 2,
                      kv_dtype: str = "bf16", seed: int = 0,
                      needle: bool = True) -> PrefillCase:
    seqs = list(PREFILL_SEQS if seqs is None else seqs)
    gen = torch.Generator().manual_seed(1000 * seed + qpg)
    rng = np.random.default_rng(1000 * seed + qpg)
    QH = kvh * qpg
    ctxs = [c + p for c, p in seqs]
    bt, valid, kf, vf = _build_pool(gen, ctxs, kvh, kv_dtype)
    head_kh = torch.arange(QH) // qpg
    qs, metas, tiles, targets, uncovered = [], [], [], [], {}
    start = 0
    for i, (chunk, prior) in enumerate(seqs):
        qi = torch.randn(chunk, QH, D, generator=gen)
        if needle:
            tgt, unc = prefill_targets(chunk, prior, qpg, kvh, rng)
            kk = gather_tokens(kf, bt[i], ctxs[i])          # [KVH, ctx, D]
            aimed = 1.5 * kk[head_kh.view(1, -1), tgt.clamp(min=0)]
            qi = torch.where((tgt >= 0).unsqueeze(-1), aimed, qi)
        else:
            tgt = torch.full((chunk, QH), -1, dtype=torch.int64)
            unc = []
        if unc:
            uncovered[(chunk, prior)] = unc
        targets.append(tgt)
        qs.append(qi)
        metas.append((start, chunk, prior))
        tiles += [(i, v0) for v0 in range(0, chunk * qpg, 128)]
        start += chunk
    poison = _poisoned_cache if needle else (
        lambda xf, _valid, dt: to_cache(xf, dt))
    return PrefillCase(
        qpg=qpg, kvh=kvh, kv_dtype=kv_dtype, seqs=seqs,
        q=torch.cat(qs).bfloat16(), k_cache=poison(kf, valid, kv_dtype),
        v_cache=poison(vf, valid, kv_dtype), block_tables=bt, metas=metas,
        tiles=tiles, scale=D ** -0.5, targets=targets, uncovered=uncovered)


PREFILL_MUTANTS = ["skip_third_tile", "skip_last_full_tile",
                   "skip_partial_tile", "ring_alias", "mask_plus_one",
                   "mask_minus_one", "prior_ignored", "bt_swap"]


def prefill_reference(case: PrefillCase, emulate: Optional[str] = None,
                      mutant: Optional[str] = None) -> torch.Tensor:
    """[T, QH, D] float64: the float64 reference, the rounding emulation, or
    a deliberately wrong variant of the float64 reference (`mutant`)."""
    assert mutant is None or mutant in PREFILL_MUTANTS
    kc, vc = cache_to_f64(case.k_cache), cache_to_f64(case.v_cache)
    qf = case.q.double()
    QH = case.kvh * case.qpg
    out = torch.empty(qf.shape, dtype=torch.float64)
    for i, (start, chunk, prior) in enumerate(case.metas):
        ctx = chunk + prior
        n_tiles = (ctx + TILE - 1) // TILE
        bt_row = case.block_tables[i].clone()
        nb = (ctx + BS - 1) // BS
        shift, drop = 0, None
        if mutant == "bt_swap" and nb >= 3:
            bt_row[[nb - 3, nb - 2]] = bt_row[[nb - 2, nb - 3]]
        kk = gather_tokens(kc, bt_row, ctx).clone()
        vv = gather_tokens(vc, bt_row, ctx).clone()
        skip = None
        if mutant == "skip_third_tile" and n_tiles >= 3:
            skip = 2
        elif mutant == "skip_last_full_tile" and ctx >= TILE:
            skip = ctx // TILE - 1
        elif mutant == "skip_partial_tile" and ctx % TILE:
            skip = ctx // TILE
        if skip is not None:
            drop = torch.zeros(ctx, dtype=torch.bool)
            drop[skip * TILE:(skip + 1) * TILE] = True
        if mutant == "ring_alias" and n_tiles >= 4:
            n = n_tiles - 1
            w = ctx - n * TILE
            kk[:, n * TILE:] = kk[:, (n - 3) * TILE:(n - 3) * TILE + w]
            vv[:, n * TILE:] = vv[:, (n - 3) * TILE:(n - 3) * TILE + w]
        if mutant == "mask_plus_one":
            shift = 1
        elif mutant == "mask_minus_one":
            shift = -1
        if mutant == "prior_ignored":
            kk, vv, prior = kk[:, :chunk], vv[:, :chunk], 0
        qi = qf[start:start + chunk].view(chunk, case.kvh, case.qpg,
                                          D).permute(1, 2, 0, 3)
        o = attend(qi, kk, vv, prior, case.scale, emulate=emulate,
                   mask_shift=shift, drop=drop)
        out[start:start + chunk] = o.permute(2, 0, 1, 3).reshape(chunk, QH, D)
    return out


# ---------------------------------------------------------------------------
# paged decode cases
# ---------------------------------------------------------------------------

def decode_targets(S: int, n_heads: int, part_tokens: Optional[int], rng):
    """Targets of one sequence's heads, by priority: S-1, 0, S-2, then both
    sides of every multiple < S of part_tokens, 512, 256 and 16 (largest
    multiple first), then random fill."""
    wanted = [S - 1, 0, S - 2]
    for m in (part_tokens, 512, 256, 16):
        if not m:
            continue
        for b in range((S - 1) // m * m, 0, -m):
            if b < S:
                wanted += [b - 1, b]
    seen, order = set(), []
    for t in wanted:
        if 0 <= t < S and t not in seen:
            seen.add(t)
            order.append(t)
    tg = order[:n_heads]
    assert tg == order[:len(tg)] and tg[0] == S - 1
    while len(tg) < n_heads:
        tg.append(int(rng.integers(0, S)))
    return tg


@dataclasses.dataclass
class DecodeCase:
    qpg: int
    kvh: int
    kv_dtype: str
    seq_lens: List[int]             # the last one is the diffuse extra
    part_tokens: Optional[int]
    q: torch.Tensor                 # [B, QH, D] bf16
    k_cache: torch.Tensor
    v_cache: torch.Tensor
    block_tables: torch.Tensor      # [B, W] int32
    scale: float
    targets: torch.Tensor           # [B, QH], -1 = diffuse
    _cache: dict = dataclasses.field(default_factory=dict)

    def reference(self):
        if "ref" not in self._cache:
            self._cache["ref"] = decode_reference(self)
        return self._cache["ref"]

    def limit(self):
        if "limit" not in self._cache:
            self._cache["limit"] = limit_from(
                decode_reference(self, emulate="decode"), self.reference())
        return self._cache["limit"]


def make_decode_case(qpg: int, seq_lens, part_tokens: Optional[int] = None,
                     kvh: int = 2, kv_dtype: str = "bf16", seed: int = 0,
                     needle: bool = True,
                     diffuse_extra: bool = True) -> DecodeCase:
    """One launch: `seq_lens` with needle heads, plus (diffuse_extra) one
    fully diffuse sequence as long as the longest."""
    n_needle = len(seq_lens) if needle else 0
    seq_lens = list(seq_lens) + ([max(seq_lens)]
                                 if needle and diffuse_extra else [])
    gen = torch.Generator().manual_seed(7000 + 1000 * seed + qpg)
    rng = np.random.default_rng(7000 + 1000 * seed + qpg)
    QH = kvh * qpg
    B = len(seq_lens)
    bt, valid, kf, vf = _build_pool(gen, seq_lens, kvh, kv_dtype)
    head_kh = torch.arange(QH) // qpg
    q = torch.randn(B, QH, D, generator=gen)
    targets = torch.full((B, QH), -1, dtype=torch.int64)
    for b, S in enumerate(seq_lens[:n_needle]):
        if S == 0:
            continue
        tg = torch.tensor(decode_targets(S, QH, part_tokens, rng))
        targets[b] = tg
        kk = gather_tokens(kf, bt[b], S)
        q[b] = 1.5 * kk[head_kh, tg]
        # the last token of every sequence is some head's target
        assert S - 1 in tg.tolist()
    poison = _poisoned_cache if needle else (
        lambda xf, _valid, dt: to_cache(xf, dt))
    return DecodeCase(
        qpg=qpg, kvh=kvh, kv_dtype=kv_dtype, seq_lens=seq_lens,
        part_tokens=part_tokens, q=q.bfloat16(),
        k_cache=poison(kf, valid, kv_dtype),
        v_cache=poison(vf, valid, kv_dtype), block_tables=bt,
        scale=D ** -0.5, targets=targets)


DECODE_MUTANTS = ["drop_last_token", "drop_last_partition", "m_unadjusted",
                  "drop_chunk_tail", "row_off_by_one"]


def decode_reference(case: DecodeCase, emulate: Optional[str] = None,
                     mutant: Optional[str] = None) -> torch.Tensor:
    """[B, QH, D] float64; see prefill_reference. The partition mutants need
    case.part_tokens."""
    assert mutant is None or mutant in DECODE_MUTANTS
    kc, vc = cache_to_f64(case.k_cache), cache_to_f64(case.v_cache)
    if mutant == "row_off_by_one":
        kc, vc = kc.roll(-1, dims=2), vc.roll(-1, dims=2)
    qf = case.q.double()
    QH = case.kvh * case.qpg
    part = case.part_tokens
    out = torch.zeros(qf.shape, dtype=torch.float64)
    for b, S in enumerate(case.seq_lens):
        if S == 0:
            continue
        kk = gather_tokens(kc, case.block_tables[b], S)
        vv = gather_tokens(vc, case.block_tables[b], S)
        qb = qf[b].view(case.kvh, case.qpg, 1, D)
        drop = torch.zeros(S, dtype=torch.bool)
        if mutant == "drop_last_token":
            drop[S - 1] = True
        elif mutant == "drop_last_partition":
            drop[(S - 1) // part * part:] = True
        elif mutant == "drop_chunk_tail":
            drop = (torch.arange(S) % 512) >= 256
        if mutant == "m_unadjusted":
            # partials merged as if every partition had the same running max
            s = torch.einsum("hgtd,hsd->hgts", qb, kk) * case.scale
            o = torch.zeros(case.kvh, case.qpg, 1, D, dtype=torch.float64)
            l = torch.zeros(case.kvh, case.qpg, 1, 1, dtype=torch.float64)
            for t0 in range(0, S, part):
                sp = s[..., t0:t0 + part]
                e = torch.exp(sp - sp.amax(dim=-1, keepdim=True))
                o += torch.einsum("hgts,hsd->hgtd", e, vv[:, t0:t0 + part])
                l += e.sum(dim=-1, keepdim=True)
            o = o / l
        else:
            o = attend(qb, kk, vv, S - 1, case.scale, emulate=emulate,
                       drop=drop)
        out[b] = o.reshape(QH, D)
    return out


# ---------------------------------------------------------------------------
# elementwise / row kernels, float64
# ---------------------------------------------------------------------------

RMS_CACHED_ELEMS = 256 * 8 * 8   # threads * cached chunks * elements


def rmsnorm_ref64(x, w, eps: float, residual=None):
    """Returns (y float64, updated residual bf16 | None).

    With a residual the kernel sums x + r in fp32, writes bf16(x + r) back
    and keeps the fp32 sum of the first 16384 elements of a row in
    registers; elements beyond that are re-read from the updated bf16
    residual. The mean of squares uses the unrounded sum throughout. The
    reference follows this per element: unrounded sum below
    RMS_CACHED_ELEMS, bf16-rounded sum from there on."""
    src = x.double()
    new_res = None
    if residual is not None:
        new_res = (x.float() + residual.float()).bfloat16()
        src = src + residual.double()
    var = src.pow(2).mean(dim=-1, keepdim=True)
    if residual is not None and x.shape[-1] > RMS_CACHED_ELEMS:
        src = torch.cat([src[..., :RMS_CACHED_ELEMS],
                         new_res.double()[..., RMS_CACHED_ELEMS:]], dim=-1)
    return src / torch.sqrt(var + eps) * w.double(), new_res


def rope_ref64(x, table, positions):
    """NeoX rotate-half of x [T, H, D] in float64 with the fp32 table."""
    half = x.shape[-1] // 2
    cs = table.double()[positions.long()]
    c, s = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    xf = x.double()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_ref32(x, table, positions, fused: bool = False):
    """The same rotation evaluated in fp32 and rounded to bf16: both
    products rounded (fused=False), or the way a compiler contracts
    x1*c - x2*s into fma(x1, c, -(x2*s)), with only the second product
    rounded (fused=True; a bf16 times an fp32 is exact in float64)."""
    half = x.shape[-1] // 2
    cs = table[positions.long()]
    c, s = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    if fused:
        xf, c, s = x.double(), c.double(), s.double()
        x1, x2 = xf[..., :half], xf[..., half:]
        o1 = x1 * c - (x2 * s).float().double()
        o2 = x2 * c + (x1 * s).float().double()
        return torch.cat([o1, o2], dim=-1).float().bfloat16()
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).bfloat16()


def silu_mul_ref64(gate_up):
    inter = gate_up.shape[-1] // 2
    g = gate_up[..., :inter].double()
    u = gate_up[..., inter:].double()
    return g / (1.0 + torch.exp(-g)) * u


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |ref| (float64), the subnormal spacing at least."""
    e = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126)))
    return torch.pow(2.0, e - 7)
