"""LoRA adapters of the worker engine (DEVELOPMENT.md "LoRA adapters").

LoraAdapter is the host-side adapter: per layer and target the CPU tensors
A [r, in] and B [out, r] of y += (alpha / r) * (x · Aᵀ) · Bᵀ. The four
targets are the fused matrices as LlamaRunner holds them.

LoraSlots is the device side: one slot pool per layer and target,
A [S, R, in] and B [S, out, R] in the model dtype, read by ops.lora_add. A
registered adapter is resident when it occupies a slot; a slot is reloaded
only when no request uses it.
"""
import hashlib
import struct
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from ..models.configs import ModelConfig
from ..models.llama import LORA_TARGETS

# block_hashes' default seed: what a request with no adapter hashes with
BASE_HASH_SEED = 0x9E3779B97F4A7C15


def adapter_hash_seed(adapter: str) -> int:
    """The block_hashes seed of a request under `adapter` ("" = base model).
    KV computed under one adapter must never be reused under another or under
    none, so the adapter's name is part of every block's content hash. Every
    place that hashes prompt blocks derives the seed here."""
    if not adapter:
        return BASE_HASH_SEED
    digest = hashlib.sha256(adapter.encode("utf-8")).digest()
    return BASE_HASH_SEED ^ int.from_bytes(digest[:8], "little")


def target_dims(cfg: ModelConfig) -> Dict[str, Tuple[int, int]]:
    """(in, out) of each target's fused matrix."""
    return {"wqkv": (cfg.hidden_size, cfg.q_size + 2 * cfg.kv_size),
            "wo": (cfg.q_size, cfg.hidden_size),
            "wgate_up": (cfg.hidden_size, 2 * cfg.intermediate_size),
            "wdown": (cfg.intermediate_size, cfg.hidden_size)}


class LoraAdapter:
    def __init__(self, name: str, rank: int, alpha: float,
                 weights: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]):
        """weights: per layer, target -> (A [rank, in], B [out, rank]), fp32
        on the CPU."""
        self.name = name
        self.rank = int(rank)
        self.alpha = float(alpha)
        self.weights = [
            {t: (A.detach().to("cpu", torch.float32).contiguous(),
                 B.detach().to("cpu", torch.float32).contiguous())
             for t, (A, B) in layer.items()} for layer in weights]
        for layer in self.weights:
            for t, (A, B) in layer.items():
                if t not in LORA_TARGETS or A.shape[0] != self.rank or \
                        B.shape[1] != self.rank:
                    raise ValueError(f"adapter {name}: bad tensor for {t}")
        self._content_id: Optional[str] = None

    @property
    def content_id(self) -> str:
        """Hash of what the adapter computes: rank, alpha and every tensor's
        bytes. Not the name: two ranks may know one adapter by two paths."""
        if self._content_id is None:
            h = hashlib.sha256(struct.pack("<id", self.rank, self.alpha))
            for li, layer in enumerate(self.weights):
                for t in LORA_TARGETS:
                    if t in layer:
                        h.update(f"{li}/{t}".encode())
                        for m in layer[t]:
                            h.update(m.numpy().tobytes())
            self._content_id = h.hexdigest()[:16]
        return self._content_id

    @classmethod
    def random(cls, cfg: ModelConfig, rank: int, seed: int, std: float = 0.02,
               name: str = "", alpha: Optional[float] = None
               ) -> "LoraAdapter":
        """A and B ~ N(0, std^2) on every layer and target, from a CPU
        generator: the same arguments give the same adapter anywhere."""
        gen = torch.Generator(device="cpu").manual_seed(seed)
        dims = target_dims(cfg)
        weights = []
        for _ in range(cfg.num_layers):
            layer = {}
            for t in LORA_TARGETS:
                n_in, n_out = dims[t]
                layer[t] = (
                    torch.empty(rank, n_in).normal_(0.0, std, generator=gen),
                    torch.empty(n_out, rank).normal_(0.0, std, generator=gen))
            weights.append(layer)
        return cls(name or f"random-r{rank}-s{seed}", rank,
                   float(rank) if alpha is None else alpha, weights)

    def save(self, path: str) -> None:
        torch.save({"name": self.name, "rank": self.rank, "alpha": self.alpha,
                    "weights": [{t: [A, B] for t, (A, B) in layer.items()}
                                for layer in self.weights]}, path)

    @classmethod
    def load(cls, path: str, name: str = "") -> "LoraAdapter":
        d = torch.load(path, map_location="cpu", weights_only=True)
        return cls(name or d["name"], d["rank"], d["alpha"],
                   [{t: (ab[0], ab[1]) for t, ab in layer.items()}
                    for layer in d["weights"]])

    def pool_tensors(self, cfg: ModelConfig, R: int, dtype: torch.dtype
                     ) -> List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]:
        """What a slot holds for this adapter: per layer and target
        (A [R, in], B [out, R]) in `dtype` on the CPU, zero-padded from rank
        to R (exact), alpha / rank folded into B in fp32 before the rounding.
        A target the adapter lacks is all zeros."""
        if self.rank > R:
            raise ValueError(f"adapter {self.name}: rank {self.rank} exceeds "
                             f"the pool rank {R}")
        if len(self.weights) != cfg.num_layers:
            raise ValueError(f"adapter {self.name}: {len(self.weights)} "
                             f"layers, the model has {cfg.num_layers}")
        dims = target_dims(cfg)
        out = []
        for layer in self.weights:
            slot = {}
            for t in LORA_TARGETS:
                n_in, n_out = dims[t]
                A = torch.zeros(R, n_in)
                B = torch.zeros(n_out, R)
                if t in layer:
                    a, b = layer[t]
                    if a.shape[1] != n_in or b.shape[0] != n_out:
                        raise ValueError(
                            f"adapter {self.name}: {t} does not fit the model")
                    A[:self.rank] = a
                    B[:, :self.rank] = b * (self.alpha / self.rank)
                slot[t] = (A.to(dtype), B.to(dtype))
            out.append(slot)
        return out


def adapter_from_spec(name: str, spec: str, cfg: ModelConfig) -> LoraAdapter:
    """An adapter from a NodeConfig.lora_adapters value: the path of a
    LoraAdapter.save file, or "random:rank=8,seed=1[,std=0.02][,alpha=8]"
    (LoraAdapter.random; every rank that reads the same spec holds the same
    adapter)."""
    if not spec.startswith("random:"):
        return LoraAdapter.load(spec, name=name)
    kw = dict(item.split("=", 1) for item in spec[len("random:"):].split(",")
              if item)
    unknown = set(kw) - {"rank", "seed", "std", "alpha"}
    if unknown or "rank" not in kw:
        raise ValueError(f"bad adapter spec for {name}: {spec}")
    return LoraAdapter.random(
        cfg, int(kw["rank"]), int(kw.get("seed", 0)),
        float(kw.get("std", 0.02)), name=name,
        alpha=float(kw["alpha"]) if "alpha" in kw else None)


class LoraSlots:
    """The slot pools of one worker and who lives in them."""

    def __init__(self, cfg: ModelConfig, max_loras: int, rank: int,
                 device: torch.device, dtype: torch.dtype):
        if rank % 16 or not 16 <= rank <= 64:
            raise ValueError("max_lora_rank must round to a multiple of 16 "
                             f"in 16..64, got {rank}")
        self.cfg, self.S, self.R = cfg, max_loras, rank
        self.device, self.dtype = device, dtype
        dims = target_dims(cfg)
        self.pools = [
            {t: (torch.zeros(self.S, rank, dims[t][0], dtype=dtype,
                             device=device),
                 torch.zeros(self.S, dims[t][1], rank, dtype=dtype,
                             device=device)) for t in LORA_TARGETS}
            for _ in range(cfg.num_layers)]
        self.resident: List[str] = [""] * self.S       # slot -> adapter name
        self.slot_of: Dict[str, int] = {}
        self._used_at = [0] * self.S
        self._tick = 0
        self.loads = 0

    def touch(self, name: str) -> int:
        self._tick += 1
        slot = self.slot_of[name]
        self._used_at[slot] = self._tick
        return slot

    def victim(self, in_use: Iterable[str]) -> Optional[int]:
        """A free slot, else the least recently used one whose adapter is
        not in `in_use`, else None."""
        busy = set(in_use)
        best = None
        for s in range(self.S):
            if not self.resident[s]:
                return s
            if self.resident[s] not in busy and (
                    best is None or self._used_at[s] < self._used_at[best]):
                best = s
        return best

    def host_tensors(self, adapter: LoraAdapter):
        """The adapter as a slot holds it (LoraAdapter.pool_tensors), built
        once at registration and pinned where the pools are on a GPU, so a
        reload is only its H2D copies."""
        tensors = adapter.pool_tensors(self.cfg, self.R, self.dtype)
        if self.device.type == "cuda":
            tensors = [{t: (A.pin_memory(), B.pin_memory())
                        for t, (A, B) in layer.items()} for layer in tensors]
        return tensors

    def load(self, slot: int, name: str, tensors) -> None:
        """H2D copies of host_tensors() into `slot`, on the current
        stream."""
        old = self.resident[slot]
        if old:
            del self.slot_of[old]
        for pool, layer in zip(self.pools, tensors):
            for t in LORA_TARGETS:
                pool[t][0][slot].copy_(layer[t][0], non_blocking=True)
                pool[t][1][slot].copy_(layer[t][1], non_blocking=True)
        self.resident[slot] = name
        self.slot_of[name] = slot
        self.loads += 1
        self.touch(name)

    def drop(self, name: str) -> None:
        slot = self.slot_of.pop(name, None)
        if slot is not None:
            self.resident[slot] = ""
