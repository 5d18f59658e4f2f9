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


_PREFIX_MODEL = PrefixModel()
hash_prompts = _PREFIX_MODEL.hash_prompts
table_update = _PREFIX_MODEL.table_update
match_longest = _PREFIX_MODEL.match_longest
