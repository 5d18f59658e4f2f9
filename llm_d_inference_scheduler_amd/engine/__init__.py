from .kvcache import BlockManager, KVPool  # noqa: F401
from .lora import LoraAdapter, adapter_hash_seed  # noqa: F401
from .worker import EngineRequest, EngineWorker, RequestOutput  # noqa: F401
