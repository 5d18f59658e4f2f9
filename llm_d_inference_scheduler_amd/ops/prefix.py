"""GPU prefix-cache index — device-resident hash table driven by the gfx950
kernels (csrc/hip/prefix_kernels.hip), kept equal to one C++ PrefixIndex.

The host C++ index is the source of truth for LRU/eviction bookkeeping
(cheap, and eviction policy is inherently sequential). Every change goes
through this wrapper, which applies it to the host index first and then to
the device table: inserts, the evictions the host reports for them
(`add_evicting`), endpoint removal and capacity changes. The batched
admission-queue match then runs entirely on-GPU and scores a request exactly
as `host.match_longest` would: one `hash_prompts` launch per model seed
hashes every queued request, one `match_longest` launch probes the table for
all of them (SURVEY.md §2.6 MI355X mapping).

The device table never deletes a key (a removal only clears mask bits, so
probe chains stay intact); `rebuild()` reclaims the dead keys. On a GPU
device the kernels of `_hip_ops` run; on a CPU device the same calls go to
the model in `ops.ref`, like the other ops (ops/dispatch.py).

Known aliasing: the table stores hash 0 as key 1, so hashes 0 and 1 share
one device entry while the host index keeps them apart.
"""
import threading
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _router_core as rc
from . import ref
from .dispatch import hip_ops


def _i64(u: int) -> int:
    """Reinterpret a python uint64 as the int64 the binding expects."""
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >= (1 << 63) else u


def _pow2_at_least(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


class GpuPrefixIndex:
    def __init__(self, device, capacity_pow2: int = 1 << 21,
                 lru_capacity_per_endpoint: int = 131072,
                 host: Optional["rc.PrefixIndex"] = None):
        assert capacity_pow2 & (capacity_pow2 - 1) == 0
        self.device = torch.device(device)
        self.ext = hip_ops() if self.device.type == "cuda" else ref
        self._alloc(capacity_pow2)
        self._dropped = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.rebuilds = 0
        self._lock = threading.RLock()
        # LRU decisions are the host index's; it is either handed over
        # (adopt_host: the producer's own index) or private to this object
        self.host = host if host is not None else \
            rc.PrefixIndex(lru_capacity_per_endpoint)
        if host is not None:
            self._load_from_host()

    # ---- table storage ----

    def _alloc(self, cap: int) -> None:
        self.keys = torch.zeros(cap, dtype=torch.uint64, device=self.device)
        self.masks = torch.zeros(cap, dtype=torch.uint64, device=self.device)
        # upper bound on occupied slots (live or dead) since the last
        # rebuild, kept on the host so the common add() needs no sync
        self._occupied_bound = 0

    @property
    def capacity(self) -> int:
        return self.keys.numel()

    def _update(self, endpoint: int, hashes: np.ndarray, remove: bool) -> None:
        if not len(hashes):
            return
        h = torch.from_numpy(np.ascontiguousarray(hashes, dtype=np.uint64))
        self.ext.table_update(self.keys, self.masks, h.to(self.device),
                              endpoint, remove, self._dropped)

    def occupancy(self):
        """(occupied slots, slots with a live mask). Syncs with the device."""
        occ = int((self.keys.view(torch.int64) != 0).sum())
        live = int((self.masks.view(torch.int64) != 0).sum())
        return occ, live

    def rebuild(self, incoming: int = 0) -> None:
        """Drop dead keys: collect the slots whose mask is not 0, clear the
        table and insert them again, one table_update launch per endpoint
        bit in use. Grows the table to the next power of two >= 4 x (live
        keys + `incoming` about to be inserted) when that count is more
        than a quarter of it."""
        with self._lock:
            sel = self.masks.view(torch.int64) != 0
            k = self.keys.view(torch.int64)[sel].cpu().numpy().view(np.uint64)
            m = self.masks.view(torch.int64)[sel].cpu().numpy().view(np.uint64)
            need = len(k) + int(incoming)
            cap = self.capacity
            if need > cap // 4:
                cap = max(cap, _pow2_at_least(4 * need))
            if cap != self.capacity:
                self._alloc(cap)
            else:
                self.keys.zero_()
                self.masks.zero_()
            for e in range(64):
                part = k[((m >> np.uint64(e)) & np.uint64(1)) != 0]
                self._update(e, part, False)
            self._occupied_bound = len(k)
            self.rebuilds += 1

    def _reserve(self, n: int) -> None:
        """Keep the table at most half full once `n` more hashes are in.
        Linear probing's expected miss cost grows fast beyond half load
        (about (1 + 1/(1-a)^2)/2 probes at load a); the bound is reasoned,
        not measured (DEVELOPMENT.md "Prefix-cache tests")."""
        half = self.capacity // 2
        if self._occupied_bound + n > half:
            occ, _ = self.occupancy()        # one sync, rare
            self._occupied_bound = occ
            if occ + n > half:
                self.rebuild(incoming=n)
        self._occupied_bound += n

    def _load_from_host(self) -> None:
        self.keys.zero_()
        self.masks.zero_()
        self._occupied_bound = 0
        for e in range(64):
            h = self.host.endpoint_hashes(e)
            if len(h):
                self._reserve(len(h))
                self._update(e, h, False)

    def adopt_host(self, host) -> None:
        """Mirror `host` from now on (the producer hands over its index);
        the table is reloaded from what `host` holds."""
        with self._lock:
            self.host = host
            self._load_from_host()

    # ---- changes: host first, then the device table ----

    def add(self, endpoint: int, hashes: np.ndarray) -> None:
        if not 0 <= endpoint < 64:
            return                      # the host index ignores these too
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1)
        if not len(h):
            return
        with self._lock:
            evicted = self.host.add_evicting(endpoint, h)
            self._reserve(len(h))
            self._update(endpoint, h, False)
            # after the inserts: a hash added and evicted by the same call
            # (more distinct hashes than the LRU holds) must end up removed
            self._update(endpoint, evicted, True)

    def remove_endpoint(self, endpoint: int) -> None:
        if not 0 <= endpoint < 64:
            return
        with self._lock:
            self._update(endpoint, self.host.endpoint_hashes(endpoint), True)
            self.host.remove_endpoint(endpoint)

    def set_capacity(self, lru_capacity_per_endpoint: int) -> None:
        with self._lock:
            for e, evicted in self.host.set_capacity(
                    lru_capacity_per_endpoint):
                self._update(e, evicted, True)

    def dropped(self) -> int:
        """Inserts the device table had no slot for (0 unless the rebuild
        policy failed). Syncs with the device."""
        return int(self._dropped.item())

    # ---- queries ----

    def hash_prompts_batch(self, token_lists, block_tokens: int,
                           max_blocks: int, seed0: int):
        """Hash a whole admission batch in one launch.
        Returns (hashes [R, max_blocks] uint64 on device, counts [R])."""
        lens = [len(t) for t in token_lists]
        flat = np.concatenate([np.asarray(t, dtype=np.int32)
                               for t in token_lists]) if token_lists else \
            np.zeros(0, dtype=np.int32)
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        return self.ext.hash_prompts(
            torch.from_numpy(flat).to(self.device),
            torch.from_numpy(offsets).to(self.device),
            block_tokens, max_blocks, _i64(seed0))

    def match_batch(self, hashes: torch.Tensor, counts: torch.Tensor,
                    n_endpoints: int) -> torch.Tensor:
        """[R, n_endpoints] consecutive matched blocks, one launch."""
        with self._lock:
            return self.ext.match_longest(self.keys, self.masks, hashes,
                                          counts, n_endpoints)


def batch_match(index: GpuPrefixIndex, prompts: Sequence[Sequence[int]],
                seeds: Sequence[int], block_tokens: int, max_blocks: int,
                n_endpoints: int):
    """Hash and match a batch whose rows may belong to different models:
    one hash launch per distinct seed (rows grouped by seed), then one match
    launch for all rows. Returns numpy arrays (match [R, n_endpoints] int32,
    counts [R] int32, hashes [R, max_blocks] uint64), rows in input order."""
    assert len(prompts) == len(seeds)
    groups = {}
    for i, s in enumerate(seeds):
        groups.setdefault(int(s) & ((1 << 64) - 1), []).append(i)
    if len(groups) == 1:
        (seed, _), = groups.items()
        hashes, counts = index.hash_prompts_batch(prompts, block_tokens,
                                                  max_blocks, seed)
    else:
        R = len(prompts)
        hashes = torch.zeros((R, max_blocks), dtype=torch.uint64,
                             device=index.device)
        counts = torch.zeros(R, dtype=torch.int32, device=index.device)
        for seed, rows in groups.items():
            h, c = index.hash_prompts_batch([prompts[i] for i in rows],
                                            block_tokens, max_blocks, seed)
            at = torch.tensor(rows, dtype=torch.int64, device=index.device)
            hashes.view(torch.int64)[at] = h.view(torch.int64)
            counts[at] = c
    match = index.match_batch(hashes, counts, n_endpoints)
    return (match.cpu().numpy(), counts.cpu().numpy(),
            hashes.cpu().numpy().astype(np.uint64, copy=False))
