"""Llama.set_cache / Llama.cache and llama_cache.py on the CPU, over a stand-in engine with Engine's
prefix-sharing surface (set_prefix_sharing(on) and supports_prefix_sharing): llama-cpp-python 0.3's names and
constructor signatures as llama_cache.py's docstring pins them, the switch reaching the engine with True / False,
and the two refusals -- LlamaDiskCache, and a front without supports_prefix_sharing (the pipeline server's).
"""
import inspect

import pytest

from llama_p2p_amd import llama_cache as C
from llama_p2p_amd.llama import Llama

MODEL = "synthetic:test-tiny:seed=0"


class SharingEngine:
    supports_prefix_sharing = True

    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd, self.calls = n_vocab, 8, []

    def set_prefix_sharing(self, on):
        self.calls.append(on)


class PlainEngine:
    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd = n_vocab, 8


def make(eng):
    return Llama.from_engine(MODEL, eng, n_ctx=64)


def test_set_cache_switches_the_engine_and_keeps_the_object():
    eng = SharingEngine()
    llm = make(eng)
    assert llm.cache is None and eng.calls == []
    cache = C.LlamaRAMCache()
    llm.set_cache(cache)
    assert eng.calls == [True] and llm.cache is cache
    llm.set_cache(None)
    assert eng.calls == [True, False] and llm.cache is None
    base = C.BaseLlamaCache(capacity_bytes=1 << 20)  # any BaseLlamaCache switches it on
    llm.set_cache(base)
    assert eng.calls == [True, False, True] and llm.cache is base


def test_names_and_aliases():
    assert C.LlamaCache is C.LlamaRAMCache
    assert issubclass(C.LlamaRAMCache, C.BaseLlamaCache) and issubclass(C.LlamaDiskCache, C.BaseLlamaCache)


def params(cls):
    return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]


def test_constructor_signatures_follow_llama_cpp_python():
    assert params(C.BaseLlamaCache) == [("capacity_bytes", 2 << 30)]
    assert params(C.LlamaRAMCache) == [("capacity_bytes", 2 << 30)]
    assert params(C.LlamaDiskCache) == [("cache_dir", ".cache/llama_cache"), ("capacity_bytes", 2 << 30)]
    assert C.LlamaRAMCache().capacity_bytes == 2 << 30
    assert C.LlamaRAMCache(capacity_bytes=123).capacity_bytes == 123  # accepted, not used
    assert C.LlamaRAMCache().cache_size == 0  # nothing is held on the host


def test_disk_cache_is_refused():
    with pytest.raises(NotImplementedError):
        C.LlamaDiskCache()

    class Disk(C.LlamaDiskCache):  # past the constructor: set_cache still refuses it
        def __init__(self):
            C.BaseLlamaCache.__init__(self)

    eng = SharingEngine()
    llm = make(eng)
    with pytest.raises(NotImplementedError):
        llm.set_cache(Disk())
    assert eng.calls == [] and llm.cache is None


def test_front_without_prefix_sharing_is_refused():
    llm = make(PlainEngine())
    with pytest.raises(NotImplementedError):
        llm.set_cache(C.LlamaRAMCache())
    assert llm.cache is None


def test_not_a_cache_is_a_type_error():
    eng = SharingEngine()
    llm = make(eng)
    with pytest.raises(TypeError):
        llm.set_cache(object())
    assert eng.calls == []


def test_engine_binding_declares_the_surface():
    from llama_p2p_amd import engine as E

    assert E.Engine.supports_prefix_sharing is True
    assert inspect.signature(E.Engine.__init__).parameters["prefix_sharing"].default is False
    for name in ("mx_engine_set_prefix_sharing", "mx_prefix_sharing_stats", "mx_kv_copy_probe"):
        assert name in E.EXPORTS
