"""Prompt caches, with llama-cpp-python's names and constructor signatures (``llama_cpp.llama_cache``):
``llm.set_cache(LlamaRAMCache())`` keeps the KV state of earlier prompts, and a later prompt starts from the
longest matching prefix.

llama_cpp is not installed here, so the contract is pinned as read from its 0.3 source: ``BaseLlamaCache(
capacity_bytes=2 << 30)``, ``LlamaRAMCache(capacity_bytes=2 << 30)``, ``LlamaCache = LlamaRAMCache`` and
``LlamaDiskCache(cache_dir=".cache/llama_cache", capacity_bytes=2 << 30)``.

Here the cache is the device's own KV slots with a host-RAM tier behind them (§14):
``Llama.set_cache`` with a ``BaseLlamaCache`` switches the engine's prefix sharing on -- a prompt whose prefix any
slot holds, or another request of the same round evaluates, receives those positions by a device copy -- and
``None`` switches it off.  ``capacity_bytes`` is the budget of the host tier: when a slot is handed to a prompt
that does not match what it holds, its K/V first go to pinned host memory, least recently used entries leaving
when the budget is full, and a later prompt that matches an entry gets those positions back by one transfer
instead of a prefill.  ``cache_size`` is the host bytes held by the engine the cache is bound to (0 for a cache no
``Llama`` uses).  ``LlamaDiskCache`` raises ``NotImplementedError`` (when constructed, and in ``set_cache``): no
state goes to disk.  The classes hold no ``LlamaState``; indexing one raises ``KeyError`` as an empty upstream
cache does.
"""
from __future__ import annotations

from typing import Sequence


class BaseLlamaCache:
    """Base of the prompt caches ``Llama.set_cache`` takes."""

    def __init__(self, capacity_bytes: int = (2 << 30)):
        self.capacity_bytes = capacity_bytes
        self._engine = None

    def _bind(self, engine) -> None:
        """``Llama.set_cache``: the engine whose host tier this object stands for (None: none any more)."""
        self._engine = engine

    @property
    def cache_size(self) -> int:
        """Host bytes held for this cache: the engine's host tier; 0 while no ``Llama`` uses the object."""
        eng = getattr(self, "_engine", None)
        return int(eng.host_cache_stats()["bytes"]) if eng is not None else 0

    def __contains__(self, key: Sequence[int]) -> bool:
        return False

    def __getitem__(self, key: Sequence[int]):
        raise KeyError("Key not found")

    def __setitem__(self, key: Sequence[int], value) -> None:
        raise NotImplementedError("the KV state stays in the device's slots: there is no LlamaState to store")


class LlamaRAMCache(BaseLlamaCache):
    """``Llama.set_cache(LlamaRAMCache(capacity_bytes))``: prefix sharing across the engine's KV slots, and up to
    ``capacity_bytes`` of evicted slots' K/V kept in host RAM."""

    def __init__(self, capacity_bytes: int = (2 << 30)):
        super().__init__(capacity_bytes)


LlamaCache = LlamaRAMCache  # llama-cpp-python's alias, kept for its callers


class LlamaDiskCache(BaseLlamaCache):
    """The name and signature only: constructing one raises ``NotImplementedError`` (no KV state is written to
    disk), and so does ``Llama.set_cache`` for a subclass that got past the constructor."""

    def __init__(self, cache_dir: str = ".cache/llama_cache", capacity_bytes: int = (2 << 30)):
        raise NotImplementedError("LlamaDiskCache is not supported: the prompt cache is the device's KV slots "
                                  "(use LlamaRAMCache)")
