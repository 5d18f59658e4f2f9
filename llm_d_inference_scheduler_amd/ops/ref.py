"""Reference torch implementations of the gfx950 kernels.

Used (a) as the CPU execution path (tiny configs in tests / gloo multi-proc
runs) and (b) as the fp32 ground truth the GPU numerics tests compare the
HIP kernels against (tests/test_gpu_kernels.py). Math is fp32 regardless of
input dtype, mirroring the kernels' internal precision.
"""
from typing import Optional

import numpy as np
import torch

FP8_E4M3_MAX = 448.0


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float,
            residual: torch.Tensor = None):
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
        residual.copy_(xf.to(residual.dtype))
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    y = xf * torch.rsqrt(var + eps) * w.float()
    return y.to(x.dtype)


def rope_table(max_pos: int, head_dim: int, theta: float,
               device="cpu") -> torch.Tensor:
    """cos/sin table [max_pos, head_dim/2, 2] fp32 (host-precomputed)."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half, dtype=torch.float64) / half))
    pos = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(pos, inv_freq)
    table = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
    return table.to(torch.float32).contiguous().to(device)


def rope(q: torch.Tensor, k: torch.Tensor, cos_sin: torch.Tensor,
         positions: torch.Tensor) -> None:
    """In-place NeoX rotate-half RoPE. q: [T, QH, D], k: [T, KVH, D]."""
    half = q.shape[-1] // 2
    cs = cos_sin[positions.long()]          # [T, half, 2]
    cos = cs[..., 0].unsqueeze(1)           # [T, 1, half]
    sin = cs[..., 1].unsqueeze(1)
    for t in (q, k):
        tf = t.float()
        x1, x2 = tf[..., :half], tf[..., half:]
        o1 = x1 * cos - x2 * sin
        o2 = x2 * cos + x1 * sin
        t.copy_(torch.cat([o1, o2], dim=-1).to(t.dtype))


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    inter = gate_up.shape[-1] // 2
    g = gate_up[..., :inter].float()
    u = gate_up[..., inter:].float()
    return (g * torch.sigmoid(g) * u).to(gate_up.dtype)


def reshape_and_cache(k_new: torch.Tensor, v_new: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor,
                      slots: torch.Tensor, k_inv_scale: torch.Tensor = None,
                      v_inv_scale: torch.Tensor = None) -> None:
    """k_new/v_new: [T, KVH, D]; caches: [NB, KVH, BS, D]; slots: [T].
    With an inverse scale [KVH] (scaled fp8 cache) the stored element is
    clamp(float(x) * inv_scale[h], -448, 448) cast to the cache dtype."""
    bs = k_cache.shape[2]

    def quant(x, inv):
        if inv is None:
            return x
        return (x.float() * inv.float().view(-1, 1)).clamp(
            -FP8_E4M3_MAX, FP8_E4M3_MAX).to(k_cache.dtype)

    for t in range(k_new.shape[0]):
        s = int(slots[t])
        if s < 0:
            continue
        blk, row = s // bs, s % bs
        k_cache[blk, :, row, :] = quant(k_new[t], k_inv_scale)
        v_cache[blk, :, row, :] = quant(v_new[t], v_inv_scale)


def dequant(cache: torch.Tensor, scale: torch.Tensor = None) -> torch.Tensor:
    """fp32 values of cache elements [..., KVH, n, D] (KVH third from the
    end) under an optional per-head scale [KVH]: cache.float() * scale."""
    cf = cache.float()
    if scale is None:
        return cf
    return cf * scale.float().view(-1, 1, 1)


def paged_attention(q: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, block_tables: torch.Tensor,
                    seq_lens: torch.Tensor, scale: float,
                    k_scale: torch.Tensor = None,
                    v_scale: torch.Tensor = None) -> torch.Tensor:
    """Decode GQA attention. q: [B, QH, D] -> out [B, QH, D]. k_scale /
    v_scale [KVH]: a cache element c of head h means float(c) * scale[h]."""
    B, QH, D = q.shape
    KVH, BS = k_cache.shape[1], k_cache.shape[2]
    qpg = QH // KVH
    out = torch.empty_like(q)
    for b in range(B):
        S = int(seq_lens[b])
        nb = (S + BS - 1) // BS
        blocks = block_tables[b, :nb].long()
        k = k_cache[blocks]                # [nb, KVH, BS, D]
        v = v_cache[blocks]
        k = dequant(k.permute(1, 0, 2, 3).reshape(KVH, nb * BS, D)[:, :S],
                    k_scale)
        v = dequant(v.permute(1, 0, 2, 3).reshape(KVH, nb * BS, D)[:, :S],
                    v_scale)
        qb = q[b].float().view(KVH, qpg, D)
        scores = torch.einsum("hgd,hsd->hgs", qb, k) * scale
        p = torch.softmax(scores, dim=-1)
        o = torch.einsum("hgs,hsd->hgd", p, v)
        out[b] = o.reshape(QH, D).to(q.dtype)
    return out


def gather_prefix(k_cache: torch.Tensor, v_cache: torch.Tensor,
                  block_table: torch.Tensor, seq_len: int):
    """Gather one sequence's K/V [S, KVH, D] from the paged pool."""
    BS = k_cache.shape[2]
    nb = (seq_len + BS - 1) // BS
    blocks = block_table[:nb].long()
    k = k_cache[blocks].permute(0, 2, 1, 3)   # [nb, BS, KVH, D]
    v = v_cache[blocks].permute(0, 2, 1, 3)
    S = nb * BS
    k = k.reshape(S, k.shape[2], k.shape[3])[:seq_len]
    v = v.reshape(S, v.shape[2], v.shape[3])[:seq_len]
    return k, v


# ---- sampler (contract: DEVELOPMENT.md "Sampling") -------------------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF
_MASS_SCALE = 4294967296.0          # masses are summed in 2^-32 fixed point
_U_MAX = 1.0 - 2.0 ** -24           # largest fp32 below 1


def philox4x32_10(counter: torch.Tensor, key) -> torch.Tensor:
    """Philox4x32-10 over a batch of counters. counter: [..., 4] int64 holding
    32-bit words; key: (k0, k1) python ints. Returns [..., 4] int64 words.
    32x32->64 products wrap in int64, which keeps their bit pattern."""
    c0, c1, c2, c3 = (counter[..., i] & _M32 for i in range(4))
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(10):
        p0 = c0 * _PHILOX_M0
        p1 = c2 * _PHILOX_M1
        n0 = ((p1 >> 32) & _M32) ^ c1 ^ k0
        n2 = ((p0 >> 32) & _M32) ^ c3 ^ k1
        c1, c3 = p1 & _M32, p0 & _M32
        c0, c2 = n0, n2
        k0 = (k0 + _PHILOX_W0) & _M32
        k1 = (k1 + _PHILOX_W1) & _M32
    return torch.stack([c0, c1, c2, c3], dim=-1)


def gumbel_noise(idx: torch.Tensor, seed: int, pos: int) -> torch.Tensor:
    """g_i of the sampling contract for vocabulary indices idx (int64)."""
    ctr = torch.zeros((idx.shape[0], 4), dtype=torch.int64)
    ctr[:, 0] = idx >> 2
    ctr[:, 1] = int(pos) & _M32
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10(ctr, (seed & _M32, seed >> 32))
    x = words.gather(1, (idx & 3).unsqueeze(1)).squeeze(1)
    u = ((x >> 8).to(torch.float32) + 0.5) * torch.tensor(
        2.0 ** -24, dtype=torch.float32)
    u = u.clamp(max=_U_MAX)
    return -torch.log(-torch.log(u))


def _sample_row(l: torch.Tensor, T: float, k: int, p: float, seed: int,
                pos: int, x: Optional[torch.Tensor] = None,
                min_p: float = 0.0, minp_base=None):
    """One row of sample() / sample_ext(); l is fp32 [V], x the penalised
    logits of step 0 (None: x = l). minp_base(z, l * inv) gives the value
    min_p is measured from (None: max z). Returns (token, logprob, n_kept,
    threshold, detail)."""
    V = l.shape[0]
    f32 = torch.float32
    M = l.max()
    lse = M + torch.log(torch.exp(l - M).sum(dtype=f32))
    detail = {"score_gap": float("inf"), "max_abs_z": 0.0,
              "mass_margin": float("inf"), "minp_margin": float("inf"),
              "lse": lse}
    if x is None:
        x = l
    T32 = torch.tensor(T, dtype=f32)
    if not T32 > 0:
        tok = int(torch.nonzero(x == x.max())[0])
        return tok, float(l[tok] - lse), V, float("-inf"), detail
    inv = torch.tensor(1.0, dtype=f32) / T32
    z = x * inv
    m = z.max()
    tau = torch.tensor(float("-inf"), dtype=f32)
    if 0 < k < V:
        tau = torch.topk(z, k).values[-1]
    p32 = torch.tensor(p, dtype=f32)
    if p32 < 1:
        kept_k = torch.nonzero(z >= tau).squeeze(1)
        zk = z[kept_k]
        w = torch.exp(zk - m)
        q = torch.round(w * _MASS_SCALE).to(torch.int64)
        order = torch.argsort(zk, descending=True, stable=True)
        zs, cum = zk[order], torch.cumsum(q[order], dim=0)
        W = cum[-1]
        target = p32.double() * W.double()
        # a value's mass counts every element tied with it: the cumulative
        # sum at the last element of each run of equal z
        ends = torch.nonzero(torch.cat(
            [zs[1:] != zs[:-1], torch.tensor([True])])).squeeze(1)
        cum_end = cum[ends].double()
        g = int(torch.nonzero(cum_end >= target)[0])
        tau_p = zs[ends[g]]
        margin = abs(float(cum_end[g] - target))
        if g > 0:
            margin = min(margin, abs(float(target - cum_end[g - 1])))
        detail["mass_margin"] = margin / float(W)
        tau = torch.maximum(tau, tau_p)
    mp32 = torch.tensor(min_p, dtype=f32)
    if mp32 > 0:
        base = m if minp_base is None else minp_base(z, l * inv)
        # log(min_p) correctly rounded to fp32: through float64
        tau_m = base + torch.log(mp32.double()).to(f32)
        detail["minp_margin"] = float((z - tau_m).abs().min())
        tau = torch.maximum(tau, tau_m)
    kept = torch.nonzero(z >= tau).squeeze(1)
    score = z[kept] + gumbel_noise(kept, seed, pos)
    best = int(torch.argmax(score))         # first maximum = lowest index
    if score.shape[0] > 1:
        top2 = torch.topk(score, 2).values
        detail["score_gap"] = float(top2[0] - top2[1])
    detail["max_abs_z"] = float(z.abs().max())
    tok = int(kept[best])
    return (tok, float(l[tok] - lse), int(kept.shape[0]), float(tau * T32),
            detail)


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
           pos: torch.Tensor, details: bool = False):
    """Temperature / top-k / top-p / seeded Gumbel-max sampling with the
    sampled token's logprob. logits [B, V] bf16|fp32; temperature, top_p [B]
    fp32; top_k, pos [B] int32; seed [B] int64 (the bits of a u64).
    Returns (tokens i64, logprobs f32, n_kept i32, threshold f32), plus a
    list of per-row dicts with details=True: the gap between the two best
    perturbed scores, max |z| over the row, and how far (as a share of
    W) the top-p mass at the boundary is from p*W on either side."""
    B = logits.shape[0]
    lf = logits.detach().to("cpu", torch.float32)
    toks, lps, nks, ths, dets = [], [], [], [], []
    for r in range(B):
        tok, lp, nk, th, det = _sample_row(
            lf[r], float(temperature[r]), int(top_k[r]), float(top_p[r]),
            int(seed[r]), int(pos[r]))
        toks.append(tok); lps.append(lp); nks.append(nk); ths.append(th)
        dets.append(det)
    dev = logits.device
    out = (torch.tensor(toks, dtype=torch.int64, device=dev),
           torch.tensor(lps, dtype=torch.float32, device=dev),
           torch.tensor(nks, dtype=torch.int32, device=dev),
           torch.tensor(ths, dtype=torch.float32, device=dev))
    return out + (dets,) if details else out


# ---- sample_ext: penalties, min_p, top-N, token state -----------------------

STATE_COUNT_MASK = 0x3FFF           # c: occurrences in the output, saturating
STATE_PROMPT_BIT = 0x4000           # bit 14: the token occurs in the prompt
TOPN_MAX = 20


def token_state_alloc(rows: int, V: int, device) -> torch.Tensor:
    """A zeroed token state: int16 [rows, Vs], Vs = V rounded up to a
    multiple of 8 (rows stay 16-byte aligned; columns >= V are padding)."""
    return torch.zeros((rows, (V + 7) // 8 * 8), dtype=torch.int16,
                       device=device)


class SamplerExtModel:
    """sample_ext / token_state_fill on CPU tensors, with the extension's
    signatures. The small methods are the places where an implementation
    can go wrong; tests/test_sampler_ext.py overrides them one at a time to
    prove that the test cases notice."""

    # -- step 0 --
    def rep_mask(self, s):
        """Elements the repetition penalty applies to (s: int32 state)."""
        return s != 0

    def rep_apply(self, x, rep):
        return torch.where(x > 0, x / rep, x * rep)

    def freq_count(self, s):
        return (s & STATE_COUNT_MASK).to(torch.float32)

    def pres_mask(self, s):
        return (s & STATE_COUNT_MASK) > 0

    def penalise(self, l, s, rep, pres, freq):
        """x of step 0 for raw fp32 logits l and int32 state s, each torch
        op one rounded fp32 operation."""
        f32 = torch.float32
        rep, pres, freq = (torch.tensor(v, dtype=f32)
                           for v in (rep, pres, freq))
        x = torch.where(self.rep_mask(s), self.rep_apply(l, rep), l)
        x = x - freq * self.freq_count(s)
        return x - torch.where(self.pres_mask(s), pres,
                               torch.zeros((), dtype=f32))

    # -- min_p --
    def minp_base(self, z, z_raw):
        return z.max()

    # -- top-N --
    def topn_values(self, l, x):
        return l

    def topn_pick(self, v, n):
        """Indices of the n largest of v by (value descending, index
        ascending)."""
        return torch.argsort(v, descending=True, stable=True)[:n]

    # -- state --
    def bump(self, s: int) -> int:
        """State element after one more occurrence in the output."""
        return s if (s & STATE_COUNT_MASK) == STATE_COUNT_MASK else s + 1

    def update_state(self, row, tok: int) -> None:
        row[tok] = self.bump(int(row[tok]))

    def sample_ext(self, logits, temperature, top_k, top_p, seed, pos, rep,
                   pres, freq, min_p, top_n, state_row, state=None,
                   n_top: int = 0, details: bool = False):
        """sample() with the per-row extensions of DEVELOPMENT.md
        "Sampling": rep / pres / freq / min_p [B] fp32, top_n / state_row
        [B] int32, state the int16 token state [R, Vs] or None (updated in
        place), n_top the width of the top-N outputs. Returns (tokens,
        logprobs, n_kept, threshold, top_tokens [B, n_top] i64, top_logprobs
        [B, n_top] f32), plus the per-row details with details=True."""
        _req(0 <= n_top <= TOPN_MAX, "n_top must be in [0, 20]")
        B, V = logits.shape
        if state is not None:
            _req(state.dtype == torch.int16 and state.dim() == 2 and
                 state.shape[1] == (V + 7) // 8 * 8,
                 "state must be int16 [R, Vs]")
        lf = logits.detach().to("cpu", torch.float32)
        toks, lps, nks, ths, dets = [], [], [], [], []
        top_tok = torch.full((B, n_top), -1, dtype=torch.int64)
        top_lp = torch.full((B, n_top), float("-inf"), dtype=torch.float32)
        for r in range(B):
            l = lf[r]
            sr = int(state_row[r])
            has = state is not None and 0 <= sr < state.shape[0]
            s = state[sr, :V].to(torch.int32) if has else \
                torch.zeros(V, dtype=torch.int32)
            x = self.penalise(l, s, float(rep[r]), float(pres[r]),
                              float(freq[r]))
            tok, lp, nk, th, det = _sample_row(
                l, float(temperature[r]), int(top_k[r]), float(top_p[r]),
                int(seed[r]), int(pos[r]), x=x, min_p=float(min_p[r]),
                minp_base=self.minp_base)
            n = max(0, min(int(top_n[r]), n_top, V))
            if n:
                idx = self.topn_pick(self.topn_values(l, x) + 0.0, n)
                top_tok[r, :n] = idx
                top_lp[r, :n] = l[idx] - det["lse"]
            if has:
                self.update_state(state[sr], tok)
            toks.append(tok); lps.append(lp); nks.append(nk); ths.append(th)
            dets.append(det)
        dev = logits.device
        out = (torch.tensor(toks, dtype=torch.int64, device=dev),
               torch.tensor(lps, dtype=torch.float32, device=dev),
               torch.tensor(nks, dtype=torch.int32, device=dev),
               torch.tensor(ths, dtype=torch.float32, device=dev),
               top_tok.to(dev), top_lp.to(dev))
        return out + (dets,) if details else out

    def token_state_fill(self, state, rows, tokens, offsets, n_prompt,
                         V: int) -> None:
        """For each q: clear columns [0, V) of state row rows[q], set the
        prompt bit for tokens[offsets[q] : offsets[q] + n_prompt[q]] and
        count tokens[offsets[q] + n_prompt[q] : offsets[q + 1]], saturating.
        Rows and ids out of range are skipped."""
        _req(state.dtype == torch.int16 and state.dim() == 2 and
             state.shape[1] == (V + 7) // 8 * 8,
             "state must be int16 [R, Vs]")
        _req(rows.dtype == torch.int32 and tokens.dtype == torch.int32 and
             n_prompt.dtype == torch.int32,
             "rows, tokens and n_prompt must be int32")
        _req(offsets.dtype == torch.int64, "offsets must be int64")
        _req(n_prompt.numel() == rows.numel() and
             offsets.numel() == rows.numel() + 1,
             "n_prompt must hold one value per row and offsets one more")
        toks = tokens.tolist()
        off = offsets.tolist()
        for q, sr in enumerate(rows.tolist()):
            if not 0 <= sr < state.shape[0]:
                continue
            beg = min(max(off[q], 0), len(toks))
            end = min(max(off[q + 1], beg), len(toks))
            n_p = min(max(int(n_prompt[q]), 0), end - beg)
            vals = [0] * V
            for t in toks[beg:beg + n_p]:
                if 0 <= t < V:
                    vals[t] |= STATE_PROMPT_BIT
            for t in toks[beg + n_p:end]:
                if 0 <= t < V:
                    vals[t] = self.bump(vals[t])
            state[sr, :V] = torch.tensor(vals, dtype=torch.int16)


_SAMPLER_EXT = SamplerExtModel()
sample_ext = _SAMPLER_EXT.sample_ext
token_state_fill = _SAMPLER_EXT.token_state_fill


# ---- prefix-cache kernels (contract: DEVELOPMENT.md "Prefix-cache tests") --
#
# A second implementation of csrc/common/xxhash64.h and of the device table
# in csrc/hip/prefix_kernels.hip, in Python integers masked to 64 bits. It
# shares no code with the C++ core (`_router_core.hash_tokens`), so the two
# check each other. PrefixModel's small methods are the places where the
# kernels can go wrong; tests/test_prefix_cases.py overrides them one at a
# time to prove that the test cases notice.

_M64 = 0xFFFFFFFFFFFFFFFF
_XP1 = 0x9E3779B185EBCA87
_XP2 = 0xC2B2AE3D27D4EB4F
_XP3 = 0x165667B19E3779F9
_XP4 = 0x85EBCA77C2B2AE63
_XP5 = 0x27D4EB2F165667C5


def _rotl64(x: int, r: int) -> int:
    return ((x << r) | (x >> (64 - r))) & _M64


def _xxh_round(acc: int, inp: int) -> int:
    return (_rotl64((acc + inp * _XP2) & _M64, 31) * _XP1) & _M64


def _xxh_merge(acc: int, val: int) -> int:
    return ((acc ^ _xxh_round(0, val)) * _XP1 + _XP4) & _M64


def xxh64(data: bytes, seed: int) -> int:
    """XXH64 of `data` from the xxHash specification."""
    n, p = len(data), 0
    seed &= _M64

    def rd(k):
        return int.from_bytes(data[p:p + k], "little")

    if n >= 32:
        v = [(seed + _XP1 + _XP2) & _M64, (seed + _XP2) & _M64, seed,
             (seed - _XP1) & _M64]
        while p + 32 <= n:
            for i in range(4):
                v[i] = _xxh_round(v[i], rd(8))
                p += 8
        h = (_rotl64(v[0], 1) + _rotl64(v[1], 7) + _rotl64(v[2], 12) +
             _rotl64(v[3], 18)) & _M64
        for x in v:
            h = _xxh_merge(h, x)
    else:
        h = (seed + _XP5) & _M64
    h = (h + n) & _M64
    while p + 8 <= n:
        h ^= _xxh_round(0, rd(8))
        h = (_rotl64(h, 27) * _XP1 + _XP4) & _M64
        p += 8
    if p + 4 <= n:
        h ^= (rd(4) * _XP1) & _M64
        h = (_rotl64(h, 23) * _XP2 + _XP3) & _M64
        p += 4
    while p < n:
        h ^= (data[p] * _XP5) & _M64
        h = (_rotl64(h, 11) * _XP1) & _M64
        p += 1
    h ^= h >> 33
    h = (h * _XP2) & _M64
    h ^= h >> 29
    h = (h * _XP3) & _M64
    h ^= h >> 32
    return h


def _req(cond: bool, msg: str) -> None:
    # the extension rejects bad arguments with TORCH_CHECK -> RuntimeError
    if not cond:
        raise RuntimeError(msg)


class PrefixModel:
    """hash_prompts / table_update / match_longest with the extension's
    signatures and tensor layouts, on CPU tensors.

    Device table: keys[cap] and masks[cap] uint64, cap = 2^k. Key 0 means
    empty, so hash 0 is stored as 1 (hashes 0 and 1 share one entry). The
    home slot is key & (cap-1); probing is linear and wraps; a removed key
    keeps its slot with mask 0; an insert that finds no slot in cap probes
    is dropped and counted."""

    # -- hashing: the chain of csrc/common/xxhash64.h --
    def content_hash(self, block: bytes, seed0: int) -> int:
        return xxh64(block, seed0)

    def chain_start(self, seed0: int) -> int:
        return seed0

    def chain_hash(self, content: int, prev: int) -> int:
        return xxh64(content.to_bytes(8, "little") + prev.to_bytes(8, "little"),
                     0)

    def hash_prompts(self, tokens, offsets, block_tokens, max_blocks, seed0):
        _req(tokens.dtype == torch.int32 and offsets.dtype == torch.int64,
             "tokens must be int32 and offsets int64")
        _req(block_tokens >= 1, "block_tokens must be >= 1")
        _req(max_blocks >= 1, "max_blocks must be >= 1")
        _req(offsets.numel() >= 1, "offsets must hold R+1 >= 1 values")
        import numpy as np
        tok = tokens.numpy().astype("<i4")
        off = offsets.numpy()
        seed0 = int(seed0) & _M64
        R = off.shape[0] - 1
        out = np.zeros((R, max_blocks), dtype=np.uint64)
        counts = np.zeros(R, dtype=np.int32)
        for r in range(R):
            beg, end = int(off[r]), int(off[r + 1])
            n = max(0, min((end - beg) // block_tokens, max_blocks))
            counts[r] = n
            prev = self.chain_start(seed0)
            for b in range(n):
                lo = beg + b * block_tokens
                c = self.content_hash(tok[lo:lo + block_tokens].tobytes(),
                                      seed0)
                prev = self.chain_hash(c, prev)
                out[r, b] = prev
        return torch.from_numpy(out), torch.from_numpy(counts)

    # -- table --
    def norm_key(self, h: int) -> int:
        return h if h else 1

    def lookup_key(self, h: int) -> int:
        return self.norm_key(h)

    def next_slot(self, slot: int, cap: int):
        """Slot probed after `slot`; None ends the probe."""
        return (slot + 1) & (cap - 1)

    def same_key(self, stored: int, key: int) -> bool:
        """Whether an insert of `key` shares the slot holding `stored`."""
        return stored == key

    def lookup_stops_at(self, stored: int, mask: int) -> bool:
        """Whether a lookup gives up at a slot holding another key."""
        return False

    @staticmethod
    def _check_table(keys, masks, hashes):
        for t in (keys, masks, hashes):
            _req(t.dtype == torch.uint64, "keys, masks, hashes must be uint64")
        _req(keys.numel() == masks.numel(),
             "table keys and masks must be equally long")
        cap = keys.numel()
        _req(cap >= 1 and cap & (cap - 1) == 0, "table cap must be 2^k")

    def table_update(self, keys, masks, hashes, endpoint, is_remove,
                     dropped=None):
        self._check_table(keys, masks, hashes)
        _req(0 <= endpoint < 64, "endpoint must be in [0, 64)")
        k, m = keys.numpy(), masks.numpy()      # views: updated in place
        cap = k.shape[0]
        bit = 1 << endpoint
        for h in hashes.numpy().reshape(-1).tolist():
            key = self.norm_key(h)
            slot = key & (cap - 1)
            for _ in range(cap):
                stored = int(k[slot])
                if is_remove:
                    if stored == 0:
                        break
                    if stored == key:
                        m[slot] = int(m[slot]) & ~bit & _M64
                        break
                elif stored == 0 or self.same_key(stored, key):
                    k[slot] = key
                    m[slot] = int(m[slot]) | bit
                    break
                slot = self.next_slot(slot, cap)
                if slot is None:
                    slot = -1
                    break
            else:
                slot = -1
            if slot < 0 and not is_remove and dropped is not None:
                dropped += 1

    def lookup(self, k, m, h: int) -> int:
        cap = k.shape[0]
        key = self.lookup_key(h)
        slot = key & (cap - 1)
        for _ in range(cap):
            stored = int(k[slot])
            if stored == 0:
                return 0
            if stored == key:
                return int(m[slot])
            if self.lookup_stops_at(stored, int(m[slot])):
                return 0
            slot = self.next_slot(slot, cap)
            if slot is None:
                return 0
        return 0

    # -- match --
    def row_blocks(self, count: int, width: int) -> int:
        return max(0, min(count, width))

    def next_active(self, active: int, survivors: int, block: int,
                    full: int) -> int:
        """Endpoints still matching after `block`."""
        return survivors

    def match_longest(self, keys, masks, hashes, counts, n_endpoints):
        self._check_table(keys, masks, hashes)
        _req(hashes.dim() == 2, "hashes must be [R, max_blocks]")
        _req(counts.dtype == torch.int32 and
             counts.numel() == hashes.shape[0],
             "counts must hold one int32 per hashes row")
        _req(1 <= n_endpoints <= 64, "n_endpoints must be in [1, 64]")
        import numpy as np
        k, m = keys.numpy(), masks.numpy()
        hs, cs = hashes.numpy(), counts.numpy()
        R, width = hs.shape
        full = (1 << n_endpoints) - 1
        out = np.zeros((R, n_endpoints), dtype=np.int32)
        for r in range(R):
            active = full
            for b in range(self.row_blocks(int(cs[r]), width)):
                if not active:
                    break
                surv = active & self.lookup(k, m, int(hs[r, b]))
                for e in range(n_endpoints):
                    if surv >> e & 1:
                        out[r, e] = b + 1
                active = self.next_active(active, surv, b, full)
        return torch.from_numpy(out)


LORA_TILE = 16     # rows of one work-list tile (one MFMA row block)


def lora_worklist(row_slot):
    """The LoRA work list of a batch (DEVELOPMENT.md "LoRA adapters"):
    row_slot holds each row's adapter slot, -1 for none. Returns (perm,
    tiles) as CPU int32 tensors: perm lists the adapter rows grouped by slot
    (rows of one slot in ascending order), tiles [n, 3] holds (start in perm,
    count <= 16, slot). Rows with no adapter appear in neither."""
    rs = np.asarray(row_slot, dtype=np.int64).reshape(-1)
    rows = np.nonzero(rs >= 0)[0]
    rows = rows[np.argsort(rs[rows], kind="stable")]
    slots, starts, counts = np.unique(rs[rows], return_index=True,
                                      return_counts=True)
    tiles = [(start + i, min(LORA_TILE, count - i), slot)
             for slot, start, count in zip(slots.tolist(), starts.tolist(),
                                           counts.tolist())
             for i in range(0, count, LORA_TILE)]
    return (torch.from_numpy(rows.astype(np.int32)),
            torch.tensor(tiles, dtype=torch.int32).reshape(-1, 3))


def lora_add(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
             B: torch.Tensor, perm: torch.Tensor, tiles: torch.Tensor) -> None:
    """y[row] += (x[row] · A[slot]ᵀ) · B[slot]ᵀ in place for the rows of
    perm, the slot taken from the row's tile. x [T, in], y [T, out];
    A [S, R, in], B [S, out, R]. fp32 maths, the intermediate rounded to
    x's dtype as the kernel does; rows outside perm are not touched."""
    for start, count, slot in tiles.tolist():
        rows = perm[start:start + count].long()
        tmp = (x[rows].float() @ A[slot].float().T).to(x.dtype).float()
        y[rows] = (y[rows].float() + tmp @ B[slot].float().T).to(y.dtype)


# ---- fp8 weights (DEVELOPMENT.md "fp8 weights") ---------------------------

FP8_E4M3_MAX = 448.0


def quantize_weight_fp8(W: torch.Tensor):
    """W [in, out], applied as x @ W -> (wq [out, in] float8_e4m3fn, scale
    [out] fp32): scale[n] = absmax(W[:, n]) / 448 (1 for an all-zero column)
    and wq[n, k] = W[k, n] / scale[n] rounded to e4m3. Plain torch on W's
    device; fp32 division and round-to-nearest-even on either device, so a
    CPU and a GPU worker hold the same bytes."""
    wt = W.detach().float().t()
    amax = wt.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    wq = (wt / scale[:, None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return wq.to(torch.float8_e4m3fn).contiguous(), scale.contiguous()


def dequant_fp8_weight(wq: torch.Tensor, scale: torch.Tensor,
                       out: Optional[torch.Tensor] = None,
                       dtype=torch.bfloat16) -> torch.Tensor:
    """The dense [in, out] weight of an fp8 pair, float(wq[n, k]) * scale[n]
    in fp32 rounded once to `dtype` (out's, if out is given and filled)."""
    if out is not None:
        dtype = out.dtype
    W = (wq.float() * scale[:, None]).to(dtype).t()
    if out is None:
        return W.contiguous()
    out.copy_(W)
    return out


def linear_fp8(x: torch.Tensor, wq: torch.Tensor,
               scale: torch.Tensor) -> torch.Tensor:
    """x [T, in] against an fp8 weight -> [T, out] in x's dtype."""
    return (x.float() @ (wq.float() * scale[:, None]).t()).to(x.dtype)


# ---- fp8 activations (DEVELOPMENT.md "fp8 activations") --------------------

def quantize_rows_fp8(x: torch.Tensor):
    """x [T, K] -> (xq [T, K] float8_e4m3fn, sx [T] fp32), one dynamic scale
    per row: sx[m] = absmax(x[m, :]) / 448 (1 for an all-zero row) and
    xq[m, k] = x[m, k] / sx[m] rounded to e4m3. quantize_weight_fp8 per row
    instead of per column: fp32 division and round-to-nearest-even, so a
    CPU and a GPU worker hold the same bytes."""
    xf = x.detach().float()
    amax = xf.abs().amax(dim=1)
    sx = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    xq = (xf / sx[:, None]).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return xq.to(torch.float8_e4m3fn).contiguous(), sx.contiguous()


def linear_fp8_a8(x: torch.Tensor, wq: torch.Tensor,
                  scale: torch.Tensor) -> torch.Tensor:
    """x [T, in], quantised per row by quantize_rows_fp8, against an fp8
    weight -> [T, out] in x's dtype: y[m, n] = sx[m] * scale[n] * sum_k
    float(xq[m, k]) * float(wq[n, k]), fp32 sums, sx applied first."""
    xq, sx = quantize_rows_fp8(x)
    acc = xq.float() @ wq.float().t()
    return (acc * sx[:, None] * scale[None, :]).to(x.dtype)


# ---- fp8 block scales (DEVELOPMENT.md "fp8 block scales") ------------------

FP8_BLOCK = 128   # edge of a weight block and width of an activation group


def _fp8_block_scale(amax: torch.Tensor) -> torch.Tensor:
    return torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))


def quantize_weight_fp8_block(W: torch.Tensor):
    """W [in, out], applied as x @ W -> (wq [out, in] float8_e4m3fn, scale
    [ceil(out / 128), ceil(in / 128)] fp32), the recipe of the public
    block-scaled fp8 checkpoints: scale[b, g] = absmax of the 128 x 128 block
    (b, g) of Wᵀ / 448 (1 for an all-zero block), wq = Wᵀ / scale rounded to
    e4m3. Edge blocks are ragged. fp32 division and round-to-nearest-even on
    either device, so a CPU and a GPU worker hold the same bytes."""
    wt = W.detach().float().t()
    n_out, n_in = wt.shape
    nb, ng = -(-n_out // FP8_BLOCK), -(-n_in // FP8_BLOCK)
    pad = torch.zeros(nb * FP8_BLOCK, ng * FP8_BLOCK, device=wt.device)
    pad[:n_out, :n_in] = wt
    amax = pad.view(nb, FP8_BLOCK, ng, FP8_BLOCK).abs().amax(dim=(1, 3))
    scale = _fp8_block_scale(amax)
    wq = (wt / expand_fp8_block_scale(scale, n_out, n_in)).clamp_(
        -FP8_E4M3_MAX, FP8_E4M3_MAX)
    return wq.to(torch.float8_e4m3fn).contiguous(), scale.contiguous()


def expand_fp8_block_scale(scale: torch.Tensor, n_out: int,
                           n_in: int) -> torch.Tensor:
    """scale [NBk, G] -> [out, in]: every element's block scale."""
    return scale.repeat_interleave(FP8_BLOCK, 0)[:n_out] \
        .repeat_interleave(FP8_BLOCK, 1)[:, :n_in]


def quantize_groups_fp8(x: torch.Tensor):
    """x [T, K] -> (xq [T, K] float8_e4m3fn, sx [T, ceil(K / 128)] fp32), one
    dynamic scale per row and 128-wide group of K (the last group may be
    narrower): sx[m, g] = absmax of the group / 448 (1 for a zero group) and
    xq = x / sx rounded to e4m3. quantize_rows_fp8 per group: fp32 division
    and round-to-nearest-even, so a CPU and a GPU worker hold the same
    bytes."""
    xf = x.detach().float()
    T, K = xf.shape
    ng = -(-K // FP8_BLOCK)
    pad = torch.zeros(T, ng * FP8_BLOCK, device=xf.device)
    pad[:, :K] = xf
    sx = _fp8_block_scale(pad.view(T, ng, FP8_BLOCK).abs().amax(dim=2))
    xq = (xf / sx.repeat_interleave(FP8_BLOCK, 1)[:, :K]).clamp_(
        -FP8_E4M3_MAX, FP8_E4M3_MAX)
    return xq.to(torch.float8_e4m3fn).contiguous(), sx.contiguous()


def linear_fp8_block(x: torch.Tensor, wq: torch.Tensor,
                     scale: torch.Tensor) -> torch.Tensor:
    """x [T, in], quantised per group by quantize_groups_fp8, against a
    block-scaled fp8 weight -> [T, out] in x's dtype: y[m, n] = sum_g
    sx[m, g] * scale[n // 128, g] * sum_{k in g} float(xq[m, k]) *
    float(wq[n, k]), fp32 sums, groups in order."""
    xq, sx = quantize_groups_fp8(x)
    xf, wf = xq.float(), wq.float()
    n_out, n_in = wf.shape
    col = scale.repeat_interleave(FP8_BLOCK, 0)[:n_out]      # [out, G]
    y = torch.zeros(xf.shape[0], n_out, device=x.device)
    for g in range(sx.shape[1]):
        k = slice(g * FP8_BLOCK, min((g + 1) * FP8_BLOCK, n_in))
        y += (xf[:, k] @ wf[:, k].t()) * (sx[:, g, None] * col[None, :, g])
    return y.to(x.dtype)


# ---- MXFP4 weights (DEVELOPMENT.md "MXFP4 weights") -----------------------

MXFP4_GROUP = 32
# the magnitudes of the e2m1 codes 0..7; bit 3 of a code is the sign
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _exp2_f32(biased: torch.Tensor) -> torch.Tensor:
    """2^(biased - 127) in fp32 for integer biased in [1, 254]: the value is
    placed in the exponent field, so the power is exact on any device."""
    return (biased.to(torch.int32) << 23).view(torch.float32)


def quantize_weight_mxfp4(W: torch.Tensor):
    """W [in, out], applied as x @ W -> (wq [out, in / 2] uint8, scale
    [out, in / 32] uint8), OCP Microscaling FP4. Group g of row n covers
    k in [32g, 32g + 32) and shares the exponent X = floor(log2(absmax)) - 2,
    stored as e8m0 X + 127 clamped to [2, 252] (127 for an all-zero group).
    Elements are W[k, n] / 2^X rounded to the nearest e2m1 value, ties to the
    even code, saturating at 6; byte j of a row holds k = 2j in its low
    nibble and k = 2j + 1 in its high nibble. Plain torch on W's device; the
    exponent comes from frexp and the power of two from bits, so a CPU and a
    GPU worker hold the same bytes. in % 32 == 0."""
    wt = W.detach().float().t().contiguous()
    n_out, n_in = wt.shape
    grp = wt.view(n_out, n_in // MXFP4_GROUP, MXFP4_GROUP)
    amax = grp.abs().amax(dim=2)
    # amax = m * 2^e with m in [0.5, 1): floor(log2(amax)) = e - 1
    _, e = torch.frexp(amax)
    biased = torch.where(amax > 0, (e - 3 + 127).clamp(2, 252),
                         torch.full_like(e, 127))
    a = (grp * _exp2_f32(254 - biased)[:, :, None]).abs()
    # midpoints between neighbouring values; a tie goes to the even code
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) +
            (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    # the sign survives rounding to zero (code 8 is -0), as in a hardware cast
    code = (code + 8 * (grp < 0)).to(torch.uint8)
    code = code.view(n_out, n_in // 2, 2)
    wq = code[:, :, 0] | (code[:, :, 1] << 4)
    return wq.contiguous(), biased.to(torch.uint8).contiguous()


def _mxfp4_dense_f32(wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """[out, in] fp32, exact: e2m1(code) * 2^(scale - 127)."""
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES),
                       dtype=torch.float32, device=wq.device)
    codes = torch.stack((wq & 15, wq >> 4), dim=2).view(wq.shape[0], -1)
    sc = _exp2_f32(scale).repeat_interleave(MXFP4_GROUP, dim=1)
    return lut[codes.long()] * sc


def dequant_mxfp4_weight(wq: torch.Tensor, scale: torch.Tensor,
                         out: Optional[torch.Tensor] = None,
                         dtype=torch.bfloat16) -> torch.Tensor:
    """The dense [in, out] weight of an MXFP4 pair in `dtype` (out's, if out
    is given and filled). Every value is zero or a normal bf16, so bf16 and
    wider types hold it exactly."""
    if out is not None:
        dtype = out.dtype
    W = _mxfp4_dense_f32(wq, scale).to(dtype).t()
    if out is None:
        return W.contiguous()
    out.copy_(W)
    return out


def linear_mxfp4(x: torch.Tensor, wq: torch.Tensor,
                 scale: torch.Tensor) -> torch.Tensor:
    """x [T, in] against an MXFP4 weight -> [T, out] in x's dtype."""
    return (x.float() @ _mxfp4_dense_f32(wq, scale).t()).to(x.dtype)


# ---- mixture of experts (DEVELOPMENT.md "Mixture of experts") --------------

def moe_route(x: torch.Tensor, router: torch.Tensor, k: int, renorm: bool):
    """x [T, H], router [E, H] -> (ids [T, k] int32, w [T, k] fp32): fp32
    logits, softmax over all E, the k largest (value descending, ties to the
    lower index), divided by their sum with renorm."""
    p = torch.softmax(x.float() @ router.float().t(), dim=-1)
    order = torch.sort(p, dim=-1, descending=True, stable=True).indices[:, :k]
    w = torch.gather(p, 1, order)
    if renorm:
        w = w / w.sum(dim=-1, keepdim=True)
    return order.to(torch.int32), w


def moe_ffn(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
            ids: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [T, H], w13 [E, 2 I, H] (gate rows, then up rows), w2 [E, H, I],
    ids / w [T, k] -> y [T, H] in x's dtype: y[t] = sum_j w[t, j] *
    (act(x[t], e) · w2[e]ᵀ) with e = ids[t, j], act = silu(x · Wgᵀ) *
    (x · Wuᵀ) rounded once to x's dtype, fp32 sums, j in slot order, one final
    rounding."""
    T, H = x.shape
    I, k = w13.shape[1] // 2, ids.shape[1]
    xf = x.float()
    y2 = torch.zeros(T, k, H, dtype=torch.float32, device=x.device)
    for e in range(w13.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        g, u = (xf[t] @ w13[e].float().t()).split(I, dim=-1)
        act = (g * torch.sigmoid(g) * u).to(x.dtype).float()
        y2[t, j] = (act @ w2[e].float().t()) * w[t, j].float()[:, None]
    y = y2[:, 0]
    for j in range(1, k):
        y = y + y2[:, j]
    return y.to(x.dtype)


def quantize_experts_mxfp4(W: torch.Tensor):
    """W [E, out, in] -> (wq [E, out, in / 2] uint8, scale [E, out, in / 32]
    uint8): quantize_weight_mxfp4 expert by expert, so the peak is one
    expert's fp32 copy."""
    pairs = [quantize_weight_mxfp4(W[e].t()) for e in range(W.shape[0])]
    return (torch.stack([p[0] for p in pairs]),
            torch.stack([p[1] for p in pairs]))


def dequant_experts_mxfp4(wq: torch.Tensor, scale: torch.Tensor,
                          dtype=torch.float32) -> torch.Tensor:
    """[E, out, in] in `dtype`, exact: every value is zero or a normal bf16."""
    E, n_out = wq.shape[:2]
    return _mxfp4_dense_f32(wq.flatten(0, 1), scale.flatten(0, 1)).to(
        dtype).view(E, n_out, -1)


def moe_ffn_mxfp4(x: torch.Tensor, w13q: torch.Tensor, w13s: torch.Tensor,
                  w2q: torch.Tensor, w2s: torch.Tensor, ids: torch.Tensor,
                  w: torch.Tensor) -> torch.Tensor:
    """moe_ffn on the exactly dequantised experts of MXFP4 pairs w13q
    [E, 2 I, H / 2], w13s [E, 2 I, H / 32], w2q [E, H, I / 2], w2s
    [E, H, I / 32]."""
    return moe_ffn(x, dequant_experts_mxfp4(w13q, w13s),
                   dequant_experts_mxfp4(w2q, w2s), ids, w)


def quantize_experts_fp8(W: torch.Tensor):
    """W [E, out, in] -> (wq [E, out, in] float8_e4m3fn, scale [E, out]
    fp32): quantize_weight_fp8 expert by expert, so the peak is one expert's
    fp32 copy."""
    pairs = [quantize_weight_fp8(W[e].t()) for e in range(W.shape[0])]
    return (torch.stack([p[0] for p in pairs]),
            torch.stack([p[1] for p in pairs]))


def dequant_experts_fp8(wq: torch.Tensor, scale: torch.Tensor,
                        dtype=torch.float32) -> torch.Tensor:
    """[E, out, in] in `dtype`: float(wq) * scale[e, n] in fp32. Not a bf16
    in general: the kernels multiply the fp32 sums by the scale instead."""
    return (wq.float() * scale[..., None]).to(dtype)


def moe_ffn_fp8(x: torch.Tensor, w13q: torch.Tensor, w13s: torch.Tensor,
                w2q: torch.Tensor, w2s: torch.Tensor, ids: torch.Tensor,
                w: torch.Tensor) -> torch.Tensor:
    """moe_ffn on the dequantised experts of fp8 pairs w13q [E, 2 I, H],
    w13s [E, 2 I], w2q [E, H, I], w2s [E, H]."""
    return moe_ffn(x, dequant_experts_fp8(w13q, w13s),
                   dequant_experts_fp8(w2q, w2s), ids, w)


def moe_ffn_fp8_a8(x: torch.Tensor, w13q: torch.Tensor, w13s: torch.Tensor,
                   w2q: torch.Tensor, w2s: torch.Tensor, ids: torch.Tensor,
                   w: torch.Tensor,
                   act_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moe_ffn_fp8 with both activations quantised per row by
    quantize_rows_fp8: the fp32 sums of codes times the row scale, then the
    channel scale. act = bf16(silu(g) * u) is quantised per (token, slot)
    pair; act_out [T k, I], if given, receives it at row t k + j."""
    T, H = x.shape
    I, k = w13q.shape[1] // 2, ids.shape[1]
    xq, sx = quantize_rows_fp8(x)
    xf = xq.float()
    y2 = torch.zeros(T, k, H, dtype=torch.float32, device=x.device)
    for e in range(w13q.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        gu = (xf[t] @ w13q[e].float().t()) * sx[t][:, None] * w13s[e][None, :]
        g, u = gu.split(I, dim=-1)
        act = (g * torch.sigmoid(g) * u).to(x.dtype)
        if act_out is not None:
            act_out[t * k + j] = act.to(act_out.dtype)
        aq, sa = quantize_rows_fp8(act)
        y2[t, j] = (aq.float() @ w2q[e].float().t()) * sa[:, None] * \
            w2s[e][None, :] * w[t, j].float()[:, None]
    y = y2[:, 0]
    for j in range(1, k):
        y = y + y2[:, j]
    return y.to(x.dtype)


def quantize_experts_fp8_block(W: torch.Tensor, halves: int = 1):
    """W [E, out, in] -> (wq [E, out, in] float8_e4m3fn, scale [E, halves *
    ceil((out / halves) / 128), ceil(in / 128)] fp32), expert by expert: each
    of the `halves` row ranges is a matrix of its own to
    quantize_weight_fp8_block, with a grid of 128-row blocks that starts at
    its first row. w13 takes halves=2, the gate rows [0, I) and the up rows
    [I, 2 I) as the checkpoints store gate_proj and up_proj (with I % 128 !=
    0 this is not the blocking of the merged [2 I, H] matrix); w2 takes 1."""
    rows = W.shape[1] // halves
    wq, scale = [], []
    for e in range(W.shape[0]):
        pairs = [quantize_weight_fp8_block(W[e, h * rows:(h + 1) * rows].t())
                 for h in range(halves)]
        wq.append(torch.cat([p[0] for p in pairs]))
        scale.append(torch.cat([p[1] for p in pairs]))
    return torch.stack(wq), torch.stack(scale)


def _expand_experts_fp8_block(scale: torch.Tensor, n_out: int, n_in: int,
                              halves: int) -> torch.Tensor:
    """scale [E, halves * NBk, G] -> [E, out, in]: every element's scale."""
    E, rows = scale.shape[0], n_out // halves
    nb = scale.shape[1] // halves
    s = scale.reshape(E * halves, nb, -1).repeat_interleave(FP8_BLOCK, 1)
    s = s[:, :rows].repeat_interleave(FP8_BLOCK, 2)[:, :, :n_in]
    return s.reshape(E, n_out, n_in)


def dequant_experts_fp8_block(wq: torch.Tensor, scale: torch.Tensor,
                              halves: int = 1,
                              dtype=torch.float32) -> torch.Tensor:
    """[E, out, in] in `dtype`: float(wq) * its block's scale in fp32."""
    return (wq.float() * _expand_experts_fp8_block(
        scale, wq.shape[1], wq.shape[2], halves)).to(dtype)


def _grouped_fp8_block(xq: torch.Tensor, sx: torch.Tensor, wq: torch.Tensor,
                       col: torch.Tensor) -> torch.Tensor:
    """sum_g sx[m, g] * col[n, g] * sum_{k in g} xq[m, k] wq[n, k] as
    linear_fp8_block sums it: fp32, groups in order."""
    xf, wf = xq.float(), wq.float()
    y = torch.zeros(xf.shape[0], wf.shape[0], device=xq.device)
    for g in range(sx.shape[1]):
        k = slice(g * FP8_BLOCK, min((g + 1) * FP8_BLOCK, wf.shape[1]))
        y += (xf[:, k] @ wf[:, k].t()) * (sx[:, g, None] * col[None, :, g])
    return y


def moe_ffn_fp8_block(x: torch.Tensor, w13q: torch.Tensor,
                      w13s: torch.Tensor, w2q: torch.Tensor,
                      w2s: torch.Tensor, ids: torch.Tensor, w: torch.Tensor,
                      act_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moe_ffn_fp8_a8 on block-scaled experts (quantize_experts_fp8_block,
    w13 with halves=2): both activations quantised by quantize_groups_fp8,
    both GEMMs summed as linear_fp8_block sums them. act = bf16(silu(g) * u)
    is quantised per (token, slot) pair and 128-wide group of I; act_out
    [T k, I], if given, receives it at row t k + j."""
    T, H = x.shape
    I, k = w13q.shape[1] // 2, ids.shape[1]
    xq, sx = quantize_groups_fp8(x)
    # every output row's scales over the groups of K: [E, out, G]
    rows = lambda s, n, halves: s.reshape(
        s.shape[0] * halves, -1, s.shape[2]).repeat_interleave(
            FP8_BLOCK, 1)[:, :n // halves].reshape(s.shape[0], n, -1)
    col13, col2 = rows(w13s, 2 * I, 2), rows(w2s, H, 1)
    y2 = torch.zeros(T, k, H, dtype=torch.float32, device=x.device)
    for e in range(w13q.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        g, u = _grouped_fp8_block(xq[t], sx[t], w13q[e], col13[e]).split(
            I, dim=-1)
        act = (g * torch.sigmoid(g) * u).to(x.dtype)
        if act_out is not None:
            act_out[t * k + j] = act.to(act_out.dtype)
        aq, sa = quantize_groups_fp8(act)
        y2[t, j] = _grouped_fp8_block(aq, sa, w2q[e], col2[e]) * \
            w[t, j].float()[:, None]
    y = y2[:, 0]
    for j in range(1, k):
        y = y + y2[:, j]
    return y.to(x.dtype)


_PREFIX_MODEL = PrefixModel()
hash_prompts = _PREFIX_MODEL.hash_prompts
table_update = _PREFIX_MODEL.table_update
match_longest = _PREFIX_MODEL.match_longest
