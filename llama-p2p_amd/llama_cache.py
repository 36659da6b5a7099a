"""Prompt caches, with llama-cpp-python's names and constructor signatures (``llama_cpp.llama_cache``):
``llm.set_cache(LlamaRAMCache())`` keeps the KV state of earlier prompts, and a later prompt starts from the
longest matching prefix.

llama_cpp is not installed here, so the contract is pinned as read from its 0.3 source: ``BaseLlamaCache(
capacity_bytes=2 << 30)``, ``LlamaRAMCache(capacity_bytes=2 << 30)``, ``LlamaCache = LlamaRAMCache`` and
``LlamaDiskCache(cache_dir=".cache/llama_cache", capacity_bytes=2 << 30)``.

Here the cache is the device's own KV slots: ``Llama.set_cache`` with a ``BaseLlamaCache``
switches the engine's prefix sharing on -- a prompt whose prefix any slot holds, or another request of the same
round evaluates, receives those positions by a device copy -- and ``None`` switches it off.  Nothing is kept
in host RAM, so ``capacity_bytes`` is accepted and not used: the capacity is the engine's ``n_seq_max`` slots of
``n_ctx`` positions, reused in the scheduler's order.  ``LlamaDiskCache`` raises ``NotImplementedError`` (when
constructed, and in ``set_cache``): no state leaves the device.  The classes hold no ``LlamaState``; indexing one raises
``KeyError`` as an empty upstream cache does.
"""
from __future__ import annotations

from typing import Sequence


class BaseLlamaCache:
    """Base of the prompt caches ``Llama.set_cache`` takes."""

    def __init__(self, capacity_bytes: int = (2 << 30)):
        self.capacity_bytes = capacity_bytes

    @property
    def cache_size(self) -> int:
        return 0  # host bytes held: the state lives in the device's KV slots

    def __contains__(self, key: Sequence[int]) -> bool:
        return False

    def __getitem__(self, key: Sequence[int]):
        raise KeyError("Key not found")

    def __setitem__(self, key: Sequence[int], value) -> None:
        raise NotImplementedError("the KV state stays in the device's slots: there is no LlamaState to store")


class LlamaRAMCache(BaseLlamaCache):
    """``Llama.set_cache(LlamaRAMCache())``: prefix sharing across the engine's KV slots."""

    def __init__(self, capacity_bytes: int = (2 << 30)):
        super().__init__(capacity_bytes)


LlamaCache = LlamaRAMCache  # llama-cpp-python's alias, kept for its callers


class LlamaDiskCache(BaseLlamaCache):
    """The name and signature only: constructing one raises ``NotImplementedError`` (no KV state is written to
    disk), and so does ``Llama.set_cache`` for a subclass that got past the constructor."""

    def __init__(self, cache_dir: str = ".cache/llama_cache", capacity_bytes: int = (2 << 30)):
        raise NotImplementedError("LlamaDiskCache is not supported: the prompt cache is the device's KV slots "
                                  "(use LlamaRAMCache)")
