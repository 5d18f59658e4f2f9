"""CPU tier of the prefix-cache tests (DEVELOPMENT.md "Prefix-cache tests").

1. The model in ops.ref passes every case of tests/prefix_cases.py, so the
   cases are consistent with the written contract (and, for the hashes,
   with the C++ core, a second implementation).
2. The cases can fail: each mutant below breaks the model in one way a
   kernel could be broken, and the named case must reject it.
3. GpuPrefixIndex on a CPU device (the same code the router runs, with the
   model in place of the kernels) stays equal to the host index through
   random histories, rebuilds its table, and handles mixed-model batches.
"""
import numpy as np
import pytest
import torch

import prefix_cases as pc
from llm_d_inference_scheduler_amd import _router_core as rc
from llm_d_inference_scheduler_amd.ops import ref
from llm_d_inference_scheduler_amd.ops.prefix import GpuPrefixIndex


@pytest.mark.parametrize("case", pc.KERNEL_CASES, ids=lambda c: c.__name__)
def test_model_passes(case):
    case(ref, "cpu")


# ---- mutants ---------------------------------------------------------------

class NoWrap(ref.PrefixModel):
    """The probe runs off the end of the table instead of wrapping."""
    def next_slot(self, slot, cap):
        return slot + 1 if slot + 1 < cap else None


class LookupStopsAtDeadKey(ref.PrefixModel):
    """A lookup treats a removed key (mask 0) like an empty slot."""
    def lookup_stops_at(self, stored, mask):
        return mask == 0


class NoRemapOnLookup(ref.PrefixModel):
    """Hash 0 is stored as 1 but looked up as 0."""
    def lookup_key(self, h):
        return h


class DuplicateTakesSecondSlot(ref.PrefixModel):
    """The insert ignores `prev == key`: a present key is inserted again."""
    def same_key(self, stored, key):
        return False


class ActiveNotCarried(ref.PrefixModel):
    """Every block starts from all endpoints."""
    def next_active(self, active, survivors, block, full):
        return full


class CountsIgnored(ref.PrefixModel):
    """Rows are matched over the whole width of `hashes`."""
    def row_blocks(self, count, width):
        return width


class ActiveResetAt512(ref.PrefixModel):
    """`active` is not carried from the first staging pass to the second."""
    def next_active(self, active, survivors, block, full):
        return full if block == 511 else survivors


class ChainSeededWith0(ref.PrefixModel):
    def chain_start(self, seed0):
        return 0


class ContentSeededWith0(ref.PrefixModel):
    def content_hash(self, block, seed0):
        return ref.xxh64(block, 0)


MUTANTS = [
    (NoWrap, "table_wrap"),
    (LookupStopsAtDeadKey, "table_dead_key_chain"),
    (NoRemapOnLookup, "table_keys_0_1"),
    (DuplicateTakesSecondSlot, "table_same_key_600"),
    (DuplicateTakesSecondSlot, "table_remove_reinsert"),
    (ActiveNotCarried, "match_counts"),
    (CountsIgnored, "match_counts"),
    (ActiveResetAt512, "match_cross_512"),
    (ChainSeededWith0, "hash_bt16"),
    (ChainSeededWith0, "hash_passes"),
    (ContentSeededWith0, "hash_bt1"),
    (ContentSeededWith0, "hash_negative_tokens"),
]


@pytest.mark.parametrize("mutant,case", MUTANTS,
                         ids=[f"{m.__name__}-{c}" for m, c in MUTANTS])
def test_case_rejects_mutant(mutant, case):
    with pytest.raises(AssertionError):
        pc.CASES_BY_NAME[case](mutant(), "cpu")


def test_every_mutant_is_listed():
    listed = {m for m, _ in MUTANTS}
    defined = {c for c in globals().values() if isinstance(c, type) and
               issubclass(c, ref.PrefixModel) and c is not ref.PrefixModel}
    assert listed == defined


def test_mutants_only_fail_where_they_should():
    """A mutant that failed everywhere would prove nothing about the named
    case: table mutants leave the hash cases alone and the other way
    round."""
    for case in pc.HASH_CASES:
        case(NoWrap(), "cpu")
        case(ActiveNotCarried(), "cpu")
    for case in pc.TABLE_CASES + pc.MATCH_CASES:
        case(ChainSeededWith0(), "cpu")


# ---- the model's argument checks mirror the binding's -----------------------

def test_model_rejects_bad_arguments():
    k = torch.zeros(16, dtype=torch.uint64)
    m = torch.zeros(16, dtype=torch.uint64)
    h = torch.zeros((2, 4), dtype=torch.uint64)
    c = torch.zeros(2, dtype=torch.int32)
    tok = torch.zeros(8, dtype=torch.int32)
    off = torch.tensor([0, 8])
    bad = [
        lambda: ref.table_update(k, m, h, -1, False),
        lambda: ref.table_update(k, m, h, 64, False),
        lambda: ref.table_update(k, m[:8], h, 0, False),
        lambda: ref.table_update(k, m, h.view(torch.int64), 0, False),
        lambda: ref.table_update(k[:12], m[:12], h, 0, False),
        lambda: ref.match_longest(k, m, h, c, 0),
        lambda: ref.match_longest(k, m, h, c, 65),
        lambda: ref.match_longest(k, m, h, c[:1], 4),
        lambda: ref.match_longest(k, m, h.view(-1), c, 4),
        lambda: ref.hash_prompts(tok, off, 0, 4, 0),
        lambda: ref.hash_prompts(tok, off, 4, 0, 0),
        lambda: ref.hash_prompts(tok, off[:0], 4, 4, 0),
    ]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()


# ---- GpuPrefixIndex on the CPU ---------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_history_matches_host_index(seed):
    pc.check_history("cpu", seed=seed)


def test_mixed_model_batch():
    pc.check_mixed_models("cpu")


def test_rebuild_keeps_live_entries_and_drops_dead_keys():
    idx = GpuPrefixIndex("cpu", capacity_pow2=64,
                         lru_capacity_per_endpoint=100)
    keys = pc._rand_keys(12, 30)
    idx.add(0, keys)
    idx.add(63, keys[:6])
    idx.remove_endpoint(0)
    before = pc.Table.entries(idx.keys, idx.masks)
    assert idx.occupancy() == (12, 6)
    idx.rebuild()
    assert idx.occupancy() == (6, 6) and idx.capacity == 64
    assert pc.Table.entries(idx.keys, idx.masks) == \
        [(k, m) for k, m in before if m]
    assert idx.rebuilds == 1 and idx.dropped() == 0
    # 17 live keys are more than a quarter of 64 slots: the table grows to
    # the next power of two >= 4 x 17
    idx.add(1, pc._rand_keys(11, 31))
    idx.rebuild()
    assert idx.occupancy() == (17, 17) and idx.capacity == 128


def test_add_larger_than_table_grows_instead_of_dropping():
    idx = GpuPrefixIndex("cpu", capacity_pow2=16,
                         lru_capacity_per_endpoint=1000)
    keys = pc._rand_keys(100, 32)
    idx.add(2, keys)
    assert idx.dropped() == 0 and idx.capacity >= 400
    rows = pc.u64(keys.reshape(100, 1), "cpu")
    out = idx.match_batch(rows, torch.ones(100, dtype=torch.int32), 3)
    assert out.numpy().tolist() == [[0, 0, 1]] * 100


def test_add_evicting_more_than_the_lru_holds():
    """One add with more distinct hashes than the LRU capacity: the hashes
    evicted by the same call must end up removed from the table."""
    idx = GpuPrefixIndex("cpu", capacity_pow2=64, lru_capacity_per_endpoint=4)
    keys = pc._rand_keys(10, 33)
    idx.add(0, keys)
    live = set(idx.host.endpoint_hashes(0).tolist())
    assert len(live) == 4
    got = {k for k, m in pc.Table.entries(idx.keys, idx.masks) if m}
    assert got == live


def test_adopt_host_reloads_the_table():
    host = rc.PrefixIndex(50)
    a, b = pc._rand_keys(5, 34), pc._rand_keys(7, 35)
    host.add(0, a)
    host.add(3, b)
    host.add(3, a[:2])
    idx = GpuPrefixIndex("cpu", capacity_pow2=64)
    idx.add(1, pc._rand_keys(3, 36))        # forgotten on adoption
    idx.adopt_host(host)
    assert idx.host is host
    want = sorted([(int(k), 1 | 8) for k in a[:2]] +
                  [(int(k), 1) for k in a[2:]] + [(int(k), 8) for k in b])
    assert pc.Table.entries(idx.keys, idx.masks) == want


def test_producer_changes_go_through_the_attached_index():
    """ApproxPrefixCacheProducer with an attached index: pre_request,
    remove_endpoint and auto-tune reach the host index and the table."""
    from types import SimpleNamespace as NS
    from llm_d_inference_scheduler_amd.plugins.producers import \
        ApproxPrefixCacheProducer
    p = ApproxPrefixCacheProducer("p", lruCapacityPerServer=6)
    idx = GpuPrefixIndex("cpu", capacity_pow2=64)
    p.attach_gpu_index(idx)
    assert idx.host is p.index

    def table():
        return {(k, m) for k, m in pc.Table.entries(idx.keys, idx.masks) if m}

    def host():
        out = {}
        for e in range(64):
            for h in p.index.endpoint_hashes(e).tolist():
                out[h] = out.get(h, 0) | (1 << e)
        return set(out.items())

    eps = [NS(index=0, name="gpu0"), NS(index=2, name="gpu2")]
    result = NS(all_endpoints=lambda: eps)
    for seed in (40, 41, 42):
        ctx = NS(state={"prefix_hashes": pc._rand_keys(4, seed)})
        p.pre_request(ctx, result, None)
        assert table() == host() and len(host()) <= 6
    assert len(host()) == 6                 # 12 added, LRU capacity 6
    p.remove_endpoint(eps[0])
    assert p.index.endpoint_size(0) == 0 and table() == host()
    tuned = NS(metrics=NS(cache_num_blocks=2, cache_block_size=16))
    p._auto_tune([tuned])
    assert p.index.endpoint_size(2) == 2 and table() == host()
    assert idx.dropped() == 0
