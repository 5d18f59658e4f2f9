"""Cases for the prefix-cache kernels (hash_prompts, table_update,
match_longest) and for GpuPrefixIndex on top of them.

Every case is a function `case(impl, device)` that raises AssertionError.
`impl` is anything with the extension's three functions: the `_hip_ops`
module on a GPU (tests/test_gpu_prefix.py), `ops.ref` on the CPU, or a
mutant of `ref.PrefixModel` (tests/test_prefix_cases.py, which proves that
these cases can fail). Expected values come from `ops.ref`, computed once
per case and shared, and the hashes are cross-checked against the C++ core's
`hash_tokens`, an implementation that shares no code with `ops.ref`.

Where a key lands under collisions depends on thread order on the device, so
tables are never compared slot by slot. Two things are compared instead: the
sorted list of (key, mask) over occupied slots, which must equal the model's
(a list, so a key stored twice shows), and the probe-chain invariant: every
occupied key is reachable from its home slot without crossing an empty slot.

All cases are tiny: tables of 16-2048 slots, prompts of at most 1105 tokens.
"""
import numpy as np
import torch

from llm_d_inference_scheduler_amd import _router_core as rc
from llm_d_inference_scheduler_amd.ops import ref
from llm_d_inference_scheduler_amd.ops.prefix import (GpuPrefixIndex, _i64,
                                                      batch_match)

M64 = (1 << 64) - 1
SEED_PLAIN = rc.model_seed("llama-3-8b", "") & ~(1 << 63) & M64
SEED_BIT63 = rc.model_seed("llama-3-8b", "salt") | (1 << 63)

_expected = {}          # case name -> reference result, computed once


def _once(name, fn):
    if name not in _expected:
        _expected[name] = fn()
    return _expected[name]


def u64(values, device):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return torch.from_numpy(a).to(device)


def as_np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# hashing
# ---------------------------------------------------------------------------

def _hash_inputs(lens, seed, lo=-2**31, hi=2**31 - 1):
    rng = np.random.default_rng(seed)
    toks = [rng.integers(lo, hi, size=n, endpoint=True).astype(np.int32)
            for n in lens]
    flat = np.concatenate(toks) if toks else np.zeros(0, np.int32)
    offsets = np.zeros(len(lens) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    return toks, flat, offsets


def _hash_case(name, lens, block_tokens, max_blocks, seed0, rng_seed=0):
    def case(impl, device):
        toks, flat, offsets = _hash_inputs(lens, rng_seed)

        def expect():
            h, c = ref.hash_prompts(torch.from_numpy(flat),
                                    torch.from_numpy(offsets), block_tokens,
                                    max_blocks, _i64(seed0))
            h, c = h.numpy(), c.numpy()
            # the two independent implementations agree with each other
            for r, t in enumerate(toks):
                cpu = rc.hash_tokens(t, block_tokens, max_blocks, seed0)
                assert c[r] == len(cpu) == min(len(t) // block_tokens,
                                               max_blocks)
                assert (h[r, :len(cpu)] == cpu).all(), (name, r)
            return h, c

        eh, ec = _once(name, expect)
        h, c = impl.hash_prompts(torch.from_numpy(flat).to(device),
                                 torch.from_numpy(offsets).to(device),
                                 block_tokens, max_blocks, _i64(seed0))
        assert tuple(h.shape) == (len(lens), max_blocks)
        assert h.dtype == torch.uint64 and c.dtype == torch.int32
        h, c = as_np(h), as_np(c)
        assert (c == ec).all(), (name, c, ec)
        # bitwise, and the unused tail of each row stays 0
        bad = np.argwhere(h != eh)
        assert not len(bad), (name, "first mismatch (row, block)", bad[0])
    case.__name__ = name
    return case


def _hash_cases():
    out = []
    for i, bt in enumerate((1, 3, 7, 8, 9, 16, 17)):
        # empty, under one block, one block, one block and a partial one,
        # 64 and 65 blocks (lane stride) with and without a partial tail
        lens = [0, bt - 1, bt, 2 * bt - 1, 64 * bt, 65 * bt,
                65 * bt + bt - 1, 63 * bt]
        out.append(_hash_case(f"hash_bt{bt}", lens, bt, 80,
                              SEED_BIT63 if i % 2 else SEED_PLAIN,
                              rng_seed=bt))
    # second and third pass of the 512-block staging buffer; 1105 clamps
    out.append(_hash_case("hash_passes", [513, 1030, 512, 1105, 0, 1024],
                          1, 1100, SEED_PLAIN, rng_seed=100))
    out.append(_hash_case("hash_passes_bt3", [3 * 513 + 2, 3 * 511], 3, 600,
                          SEED_BIT63, rng_seed=101))
    out.append(_hash_case("hash_clamp", [160, 64, 65, 16], 16, 4,
                          SEED_PLAIN, rng_seed=102))
    out.append(_hash_case("hash_seed_bit63", [48, 100], 16, 8, SEED_BIT63,
                          rng_seed=103))
    out.append(_hash_case("hash_seed_all_ones", [33], 8, 8, M64,
                          rng_seed=104))
    out.append(_hash_case("hash_rows_0", [], 16, 8, SEED_PLAIN))
    out.append(_hash_case("hash_rows_70", [(7 * r) % 40 for r in range(70)],
                          3, 16, SEED_PLAIN, rng_seed=105))
    return out


def hash_negative_tokens(impl, device):
    """Token ids are hashed as their little-endian two's-complement bytes."""
    toks = np.array([-1, -2**31, 2**31 - 1, 0, -7, 5, -1, -1], np.int32)
    offsets = np.array([0, 8], np.int64)

    def expect():
        h = rc.hash_tokens(toks, 4, 4, SEED_PLAIN)
        e, _ = ref.hash_prompts(torch.from_numpy(toks),
                                torch.from_numpy(offsets), 4, 4,
                                _i64(SEED_PLAIN))
        assert (e.numpy()[0, :2] == h).all()
        return h

    eh = _once("hash_negative_tokens", expect)
    h, c = impl.hash_prompts(torch.from_numpy(toks).to(device),
                             torch.from_numpy(offsets).to(device), 4, 4,
                             _i64(SEED_PLAIN))
    assert int(c[0]) == 2
    want = np.zeros(4, dtype=np.uint64)
    want[:2] = eh
    assert (as_np(h)[0] == want).all()


HASH_CASES = _hash_cases() + [hash_negative_tokens]


# ---------------------------------------------------------------------------
# table
# ---------------------------------------------------------------------------

class Table:
    """keys/masks/dropped on `device`, driven through `impl`, next to the
    same history applied to the model on the CPU."""

    def __init__(self, impl, device, cap):
        self.impl, self.device, self.cap = impl, device, cap
        self.keys = torch.zeros(cap, dtype=torch.uint64, device=device)
        self.masks = torch.zeros(cap, dtype=torch.uint64, device=device)
        self.dropped = torch.zeros(1, dtype=torch.int32, device=device)
        self.mk = torch.zeros(cap, dtype=torch.uint64)
        self.mm = torch.zeros(cap, dtype=torch.uint64)
        self.md = torch.zeros(1, dtype=torch.int32)

    def update(self, hashes, endpoint, remove=False):
        self.impl.table_update(self.keys, self.masks,
                               u64(hashes, self.device), endpoint, remove,
                               self.dropped)
        ref.table_update(self.mk, self.mm, u64(hashes, "cpu"), endpoint,
                         remove, self.md)

    @staticmethod
    def entries(keys, masks):
        k, m = as_np(keys), as_np(masks)
        occ = k != 0
        assert not m[~occ].any(), "mask set on an empty slot"
        return sorted(zip(k[occ].tolist(), m[occ].tolist()))

    def check(self):
        """Same (key, mask) list as the model, probe chains unbroken, same
        drop count."""
        got = self.entries(self.keys, self.masks)
        want = self.entries(self.mk, self.mm)
        assert got == want, (got, want)
        k = as_np(self.keys)
        for slot in np.flatnonzero(k):
            s = int(k[slot]) & (self.cap - 1)
            while s != slot:
                assert k[s] != 0, ("key unreachable from its home slot",
                                   hex(int(k[slot])), int(slot), s)
                s = (s + 1) & (self.cap - 1)
        assert int(self.dropped.item()) == int(self.md.item())
        return got

    def lookup(self, hashes, n_endpoints=64):
        """Mask of each hash as the match kernel sees it: one row per hash,
        one block per row -> out[r, e] == 1 iff bit e is set."""
        h = u64(hashes, self.device).view(-1, 1)
        counts = torch.ones(h.shape[0], dtype=torch.int32, device=self.device)
        out = as_np(self.impl.match_longest(self.keys, self.masks, h, counts,
                                            n_endpoints))
        assert set(np.unique(out)) <= {0, 1}
        return [sum(1 << int(e) for e in np.flatnonzero(row)) for row in out]


def _rand_keys(n, seed, low_bits=None, cap=None):
    rng = np.random.default_rng(seed)
    k = rng.integers(2, M64, size=n, dtype=np.uint64, endpoint=True)
    assert len(set(k.tolist())) == n
    if low_bits is not None:
        k = (k & np.uint64(M64 ^ (cap - 1))) | np.uint64(low_bits)
    return k


def table_48_in_64(impl, device):
    """Load 0.75: most keys collide and probe."""
    t = Table(impl, device, 64)
    keys = _rand_keys(48, 1)
    t.update(keys, 3)
    got = t.check()
    assert got == sorted((int(k), 1 << 3) for k in keys)
    assert t.lookup(keys) == [1 << 3] * 48
    assert t.lookup(_rand_keys(20, 2)) == [0] * 20
    assert int(t.dropped.item()) == 0


def table_wrap(impl, device):
    """Eight keys whose home is the last slot: seven of them wrap to the
    front of the table."""
    t = Table(impl, device, 16)
    keys = _rand_keys(8, 3, low_bits=15, cap=16)
    t.update(keys, 1)
    got = t.check()
    assert len(got) == 8
    k = as_np(t.keys)
    assert k[15] != 0 and (k[:7] != 0).all() and not k[7:15].any()
    assert t.lookup(keys) == [2] * 8
    t.update(keys[2:5], 1, remove=True)
    t.check()
    assert t.lookup(keys) == [2, 2, 0, 0, 0, 2, 2, 2]


def table_same_key_600(impl, device):
    """One hash 600 times in one call: more than one workgroup racing on
    one key (the `prev == key` arm of the CAS). Exactly one slot."""
    t = Table(impl, device, 64)
    key = 0xDEADBEEFCAFEF00D
    t.update(np.full(600, key, dtype=np.uint64), 5)
    assert t.check() == [(key, 1 << 5)]
    # and among other keys sharing its home slot
    others = _rand_keys(6, 4, low_bits=key & 63, cap=64)
    mixed = np.concatenate([others, np.full(300, key, np.uint64), others])
    t.update(mixed, 6)
    got = t.check()
    assert len(got) == 7 and (key, (1 << 5) | (1 << 6)) in got
    assert int(t.dropped.item()) == 0


def table_keys_0_1(impl, device):
    """Key 0 marks an empty slot, so hash 0 is stored as 1: hashes 0 and 1
    share one entry. That is by design (a chain hash of exactly 0 or 1 has
    probability 2^-63); this pins it."""
    t = Table(impl, device, 16)
    t.update([0], 0)
    assert t.check() == [(1, 1)]
    assert t.lookup([0, 1, 2]) == [1, 1, 0]
    t.update([1], 1)
    assert t.check() == [(1, 3)]
    assert t.lookup([0, 1]) == [3, 3]
    t.update([0], 1, remove=True)
    assert t.check() == [(1, 1)]
    assert t.lookup([0, 1]) == [1, 1]


def table_endpoint_63(impl, device):
    """The highest endpoint bit survives insert, lookup and removal."""
    t = Table(impl, device, 32)
    keys = _rand_keys(5, 5)
    t.update(keys, 63)
    t.update(keys[:2], 0)
    got = t.check()
    assert sorted(m for _, m in got) == [1 << 63] * 3 + [(1 << 63) | 1] * 2
    assert t.lookup(keys) == [(1 << 63) | 1] * 2 + [1 << 63] * 3
    assert t.lookup(keys, n_endpoints=63) == [1, 1, 0, 0, 0]
    t.update(keys, 63, remove=True)
    t.check()
    assert t.lookup(keys) == [1, 1, 0, 0, 0]


def table_remove_reinsert(impl, device):
    """A removed key keeps its slot with mask 0 and is found again by a
    later insert instead of taking a second slot."""
    t = Table(impl, device, 16)
    key = int(_rand_keys(1, 6)[0])
    t.update([key], 2)
    slot = int(np.flatnonzero(as_np(t.keys))[0])
    t.update([key], 2, remove=True)
    assert t.check() == [(key, 0)]
    assert t.lookup([key]) == [0]
    t.update([key], 4)
    assert t.check() == [(key, 1 << 4)]
    assert int(np.flatnonzero(as_np(t.keys))[0]) == slot
    assert t.lookup([key]) == [1 << 4]
    t.update([key], 9, remove=True)         # a bit that was never set
    assert t.check() == [(key, 1 << 4)]


def table_dead_key_chain(impl, device):
    """A, B, C share a home slot (inserted one call each, so A, B, C sit in
    a row). A is removed and leaves a dead key; removing B must probe past
    it, and C behind both must still be found."""
    t = Table(impl, device, 16)
    a, b, c = (int(x) for x in _rand_keys(3, 7, low_bits=5, cap=16))
    for key in (a, b, c):
        t.update([key], 0)
    assert as_np(t.keys)[5:8].tolist() == [a, b, c]
    t.update([a], 0, remove=True)
    assert t.lookup([a, b, c]) == [0, 1, 1]
    t.update([b], 0, remove=True)
    assert t.check() == sorted([(a, 0), (b, 0), (c, 1)])
    assert t.lookup([a, b, c]) == [0, 0, 1]
    # a new key with the same home goes behind the dead keys, not into them
    d = int(_rand_keys(1, 8, low_bits=5, cap=16)[0])
    t.update([d], 1)
    t.check()
    assert as_np(t.keys)[8] == d
    assert t.lookup([a, b, c, d]) == [0, 0, 1, 2]


def table_full_drop(impl, device):
    """16 keys fill 16 slots; the 17th finds no slot in cap probes, is
    dropped and counted, and its lookup misses. Every loop is bounded by
    cap, so insert, remove and lookup all return on a full table."""
    t = Table(impl, device, 16)
    keys = _rand_keys(17, 9)
    t.update(keys[:16], 0)
    assert len(t.check()) == 16 and int(t.dropped.item()) == 0
    t.update(keys[16:], 0)
    got = t.check()
    assert len(got) == 16 and int(t.dropped.item()) == 1
    assert int(keys[16]) not in [k for k, _ in got]
    assert t.lookup(keys) == [1] * 16 + [0]
    t.update(keys[16:], 0, remove=True)     # absent key, full table
    t.update(keys[:1], 1)                   # present key still updates
    t.check()
    assert t.lookup(keys) == [3] + [1] * 15 + [0]
    assert int(t.dropped.item()) == 1


TABLE_CASES = [table_48_in_64, table_wrap, table_same_key_600, table_keys_0_1,
               table_endpoint_63, table_remove_reinsert, table_dead_key_chain,
               table_full_drop]


# ---------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------

def _match(impl, device, t, rows, counts, n_endpoints):
    h = u64(np.stack(rows), device)
    c = torch.tensor(counts, dtype=torch.int32, device=device)
    out = impl.match_longest(t.keys, t.masks, h, c, n_endpoints)
    assert out.dtype == torch.int32
    assert tuple(out.shape) == (len(rows), n_endpoints)

    def expect():
        return ref.match_longest(t.mk, t.mm, torch.from_numpy(np.stack(rows)),
                                 torch.tensor(counts, dtype=torch.int32),
                                 n_endpoints).numpy()
    return as_np(out), expect


def match_counts(impl, device):
    """Rows with different counts against one table. Endpoint 0 holds the
    whole 20-block chain, endpoint 1 its first 10 blocks, endpoint 2 blocks
    0-4 and 6-19 (a gap at 5)."""
    t = Table(impl, device, 256)
    chain = _rand_keys(20, 10)
    t.update(chain, 0)
    t.update(chain[:10], 1)
    t.update(np.concatenate([chain[:5], chain[6:]]), 2)
    t.check()
    unknown = _rand_keys(1, 11)
    rows = [chain,                                   # 0: full
            chain,                                   # 1: counts 7 < present
            chain,                                   # 2: counts 0
            chain,                                   # 3: counts > width
            np.concatenate([unknown, chain[1:]]),    # 4: first block unknown
            np.concatenate([chain[:12], unknown, chain[13:]])]  # 5: gap at 12
    counts = [20, 7, 0, 25, 20, 20]
    want3 = [[20, 10, 5], [7, 7, 5], [0, 0, 0], [20, 10, 5], [0, 0, 0],
             [12, 10, 5]]
    for n_eps in (3, 1, 64):
        out, expect = _match(impl, device, t, rows, counts, n_eps)
        want = np.zeros((6, n_eps), dtype=np.int32)
        w = min(3, n_eps)
        want[:, :w] = np.array(want3)[:, :w]
        assert (_once(f"match_counts_{n_eps}", expect) == want).all()
        assert (out == want).all(), (n_eps, out[:, :3].tolist())


def match_endpoint_63(impl, device):
    """n_endpoints 64 with the top bit in use."""
    t = Table(impl, device, 64)
    chain = _rand_keys(6, 12)
    t.update(chain, 63)
    t.update(chain[:2], 62)
    out, _ = _match(impl, device, t, [chain], [6], 64)
    want = np.zeros((1, 64), dtype=np.int32)
    want[0, 63], want[0, 62] = 6, 2
    assert (out == want).all()


def match_cross_512(impl, device):
    """Rows long enough to cross the 512-block staging pass. Endpoint 0
    holds all 600 blocks; endpoint 1 everything but block 300, so it must
    stay at 300 although it holds blocks 512-599; endpoint 2 blocks 0-514,
    which ends three blocks into the second pass."""
    t = Table(impl, device, 2048)
    chain = _rand_keys(600, 13)
    t.update(chain, 0)
    t.update(np.concatenate([chain[:300], chain[301:]]), 1)
    t.update(chain[:515], 2)
    t.check()
    rows = [chain, chain, chain, chain]
    counts = [600, 512, 513, 511]
    out, expect = _match(impl, device, t, rows, counts, 3)
    want = [[600, 300, 515], [512, 300, 512], [513, 300, 513],
            [511, 300, 511]]
    assert _once("match_cross_512", expect).tolist() == want
    assert out.tolist() == want, out.tolist()


def match_rows_0(impl, device):
    t = Table(impl, device, 16)
    h = torch.zeros((0, 4), dtype=torch.uint64, device=device)
    c = torch.zeros(0, dtype=torch.int32, device=device)
    out = impl.match_longest(t.keys, t.masks, h, c, 4)
    assert tuple(out.shape) == (0, 4)


MATCH_CASES = [match_counts, match_endpoint_63, match_cross_512, match_rows_0]

KERNEL_CASES = HASH_CASES + TABLE_CASES + MATCH_CASES
CASES_BY_NAME = {c.__name__: c for c in KERNEL_CASES}
assert len(CASES_BY_NAME) == len(KERNEL_CASES)


# ---------------------------------------------------------------------------
# GpuPrefixIndex: random histories against the host index, mixed models
# ---------------------------------------------------------------------------

HIST_ENDPOINTS = 4
HIST_LRU = 8
HIST_TABLE = 64
HIST_WIDTH = 10


def history_chains(seed, n_chains=400):
    """Hash chains of 2-10 blocks; a third of them extend a prefix of an
    earlier one, so endpoints share leading blocks."""
    rng = np.random.default_rng(seed)
    fresh = iter(_rand_keys(n_chains * HIST_WIDTH, seed + 1).tolist())
    chains = []
    for i in range(n_chains):
        n = int(rng.integers(2, HIST_WIDTH + 1))
        head = []
        if i and rng.random() < 0.33:
            src = chains[int(rng.integers(0, i))]
            head = src[:int(rng.integers(1, len(src) + 1))][:n - 1]
        chains.append(head + [next(fresh) for _ in range(n - len(head))])
    return [np.array(c, dtype=np.uint64) for c in chains]


def run_history(device, steps=300, seed=0):
    """Drive add / remove_endpoint / capacity changes through a
    GpuPrefixIndex on `device` (64-slot table, LRU capacity 8, 4
    endpoints). After every step the batched match must equal the host
    index's answer for every query and nothing may have been dropped.
    Returns (index, distinct hashes added)."""
    rng = np.random.default_rng(seed)
    chains = history_chains(seed)
    idx = GpuPrefixIndex(device, capacity_pow2=HIST_TABLE,
                         lru_capacity_per_endpoint=HIST_LRU)
    seen, recent = set(), []
    for step in range(steps):
        r = rng.random()
        if r < 0.80:
            c = chains[int(rng.integers(0, len(chains)))]
            idx.add(int(rng.integers(0, HIST_ENDPOINTS)), c)
            seen.update(c.tolist())
            recent = (recent + [c])[-8:]
        elif r < 0.90:
            idx.remove_endpoint(int(rng.integers(0, HIST_ENDPOINTS)))
        else:
            idx.set_capacity(int(rng.choice([3, 5, HIST_LRU, HIST_LRU])))
        queries = recent + [chains[int(i)] for i in
                            rng.integers(0, len(chains), size=4)]
        rows = np.zeros((len(queries), HIST_WIDTH), dtype=np.uint64)
        for i, q in enumerate(queries):
            rows[i, :len(q)] = q
        counts = torch.tensor([len(q) for q in queries], dtype=torch.int32)
        got = as_np(idx.match_batch(u64(rows, idx.device),
                                    counts.to(idx.device), HIST_ENDPOINTS))
        for i, q in enumerate(queries):
            want = idx.host.match_longest(q, HIST_ENDPOINTS)
            assert got[i].tolist() == list(want), (step, i, got[i], want)
        assert idx.dropped() == 0, step
        occ, live = idx.occupancy()
        assert live <= HIST_ENDPOINTS * idx.host.capacity()
        assert occ <= idx.capacity // 2, (step, occ, idx.capacity)
    return idx, len(seen)


def check_history(device, steps=300, seed=0):
    idx, distinct = run_history(device, steps, seed)
    # enough churn that the table would have filled with dead keys many
    # times over, so rebuild() ran repeatedly
    assert distinct >= 10 * HIST_TABLE, distinct
    assert distinct >= 2 * idx.capacity
    assert idx.rebuilds >= 3, idx.rebuilds
    return idx


def check_mixed_models(device):
    """batch_match on a batch of two models hashes every row with its own
    model's seed: equal to per-request host results."""
    rng = np.random.default_rng(21)
    seeds = {"a": rc.model_seed("model-a", ""),
             "b": rc.model_seed("model-b", "") | (1 << 63)}
    bt, mb, n_eps = 4, 16, 3
    idx = GpuPrefixIndex(device, capacity_pow2=256,
                         lru_capacity_per_endpoint=64)
    prompts = [rng.integers(0, 1000, size=int(n)).astype(np.int32)
               for n in (40, 17, 64, 3, 33, 0, 64, 25)]
    models = ["a", "b", "b", "a", "b", "a", "a", "b"]
    for e, i in enumerate((0, 1, 2, 6)):
        idx.add(e % n_eps, rc.hash_tokens(prompts[i], bt, mb,
                                          seeds[models[i]]))
    # the same tokens under the other model must not match
    prompts.append(prompts[0])
    models.append("b")
    match, counts, hashes = batch_match(
        idx, [p.tolist() for p in prompts], [seeds[m] for m in models], bt,
        mb, n_eps)
    hits = 0
    for i, p in enumerate(prompts):
        h = rc.hash_tokens(p, bt, mb, seeds[models[i]])
        assert counts[i] == len(h)
        assert (hashes[i, :len(h)] == h).all(), i
        want = list(idx.host.match_longest(h, n_eps))
        assert match[i].tolist() == want, (i, match[i], want)
        hits += sum(want)
    assert hits and match[-1].tolist() == [0] * n_eps
    # one model only: the single-launch path gives the same rows
    only_a = [i for i, m in enumerate(models) if m == "a"]
    m1, c1, h1 = batch_match(idx, [prompts[i].tolist() for i in only_a],
                             [seeds["a"]] * len(only_a), bt, mb, n_eps)
    assert (m1 == match[only_a]).all() and (c1 == counts[only_a]).all()
    assert (h1 == hashes[only_a]).all()
