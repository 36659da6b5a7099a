"""The host-RAM tier's host side on the CPU: Llama.set_cache over a stand-in engine with Engine's
prefix-sharing and host-cache surface, llama_cache.py's cache_size, the names the binding declares, and the
packed-layout helper of the GPU test (tests/kv_pack_ref.py) against a brute-force loop.
"""
import inspect
import os

import numpy as np
import pytest

import kv_layout as L
import kv_pack_ref as P
from llama_p2p_amd import llama_cache as C
from llama_p2p_amd.llama import Llama

MODEL = "synthetic:test-tiny:seed=0"
NAMES = ("mx_engine_set_host_cache", "mx_host_cache_stats", "mx_kv_pack_probe")


class HostEngine:
    supports_prefix_sharing = True
    supports_host_cache = True

    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd, self.calls, self.bytes = n_vocab, 8, [], 0

    def set_prefix_sharing(self, on):
        self.calls.append(("sharing", on))

    def set_host_cache(self, n):
        self.calls.append(("host", n))
        if n == 0:
            self.bytes = 0

    def host_cache_stats(self):
        return {"entries": 1 if self.bytes else 0, "bytes": self.bytes}


def make(eng):
    return Llama.from_engine(MODEL, eng, n_ctx=64)


def test_set_cache_sets_sharing_then_the_capacity():
    eng = HostEngine()
    llm = make(eng)
    cache = C.LlamaRAMCache(capacity_bytes=1 << 20)
    llm.set_cache(cache)
    assert eng.calls == [("sharing", True), ("host", 1 << 20)] and llm.cache is cache
    eng.calls.clear()
    llm.set_cache(None)
    assert eng.calls == [("sharing", False), ("host", 0)] and llm.cache is None


def test_cache_size_follows_the_engine():
    eng = HostEngine()
    llm = make(eng)
    cache = C.LlamaRAMCache(capacity_bytes=1 << 20)
    assert cache.cache_size == 0  # unbound
    eng.bytes = 12345
    assert cache.cache_size == 0  # still unbound: no Llama uses it
    llm.set_cache(cache)
    assert cache.cache_size == 12345
    eng.bytes = 777
    assert cache.cache_size == 777
    llm.set_cache(None)
    assert cache.cache_size == 0 and eng.bytes == 0
    eng.bytes = 5  # the object no longer stands for the engine
    assert cache.cache_size == 0
    assert C.LlamaRAMCache().cache_size == 0


def test_replacing_a_cache_unbinds_the_old_one():
    eng = HostEngine()
    llm = make(eng)
    a, b = C.LlamaRAMCache(capacity_bytes=100), C.LlamaRAMCache(capacity_bytes=200)
    llm.set_cache(a)
    llm.set_cache(b)
    eng.bytes = 64
    assert a.cache_size == 0 and b.cache_size == 64
    assert eng.calls[-1] == ("host", 200)


def test_engine_binding_declares_the_surface():
    from llama_p2p_amd import engine as E

    assert E.Engine.supports_host_cache is True
    assert inspect.signature(E.Engine.__init__).parameters["host_cache_bytes"].default == 0
    assert inspect.signature(E.Engine.__init__).parameters["prefix_sharing"].default is False
    lib = E.lib()
    for name in NAMES:
        assert name in E.EXPORTS
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert [n for n, _ in E.MxHostCacheCounts._fields_] == [
        "entries", "bytes", "capacity_bytes", "spills", "spilled_bytes", "restores", "restored_prompt_tokens",
        "restored_bytes", "evictions", "skipped"]
    assert callable(E.kv_pack_probe) and callable(E.Engine.set_host_cache) and callable(E.Engine.host_cache_stats)


def test_pack_kernels_have_no_packed_fp32_and_do_not_spill():
    """tests/test_isa_guards.py's two guards for the translation unit the tier adds (csrc/kvpack.hip)."""
    import test_isa_guards as G

    obj = os.path.join(G.BUILD, "kvpack.hip.o")
    if not os.path.exists(obj) or not os.path.exists(G.LLVM):
        pytest.skip("device objects not built (run __graft_entry__.build())")
    import isa_scan

    per = isa_scan.scan(isa_scan.device_asm(obj))
    assert not {f: v[0] for f, v in per.items() if v[0]}
    spills = G._spills(obj)
    assert len(spills) == 2 and all("kv_pack_kernel" in k or "kv_unpack_kernel" in k for k in spills), spills
    assert not any(spills.values()), spills


@pytest.mark.parametrize("D", [64, 128])
def test_packed_layout_helper_against_a_brute_force_loop(D):
    n_layer, n_slots, H, S = 2, 3, 2, 128
    rng = np.random.default_rng(D)
    k = rng.integers(0, 1 << 16, (n_layer, n_slots, H, S, D), dtype=np.uint16)
    v = rng.integers(0, 1 << 16, (n_layer, n_slots, H, S, D), dtype=np.uint16)
    kt, vt = L.tile_k(k), L.tile_v(v)  # [layer][slot][head][S * D]: the regions as the device holds them
    for slot, n_pos in ((0, 1), (1, 33), (2, 128), (1, 100)):
        got = P.pack_entry(k, v, slot, n_pos)
        tiles = P.ceil32(n_pos) // 32
        assert got.size == tiles * P.tile_elems(n_layer, H, D) and P.tile_words(n_layer, H, D) * 8 == got.size // tiles
        exp = np.zeros_like(got)
        seen = np.zeros(got.size, dtype=bool)
        for t in range(tiles):
            for layer in range(n_layer):
                for kv, reg in ((0, kt), (1, vt)):
                    for head in range(H):
                        for e in range(0, 32 * D, 8):  # one 16-byte word at a time
                            i = P.packed_index(t, layer, kv, head, e, n_layer, H, D)
                            assert not seen[i:i + 8].any()
                            seen[i:i + 8] = True
                            # the region's elements, verbatim
                            exp[i:i + 8] = reg[layer, slot, head, 32 * t * D + e:32 * t * D + e + 8]
        assert seen.all() and np.array_equal(got, exp)
        # a shorter prefix of the entry is a prefix of its bytes
        for fewer in range(1, tiles):
            assert np.array_equal(P.pack_entry(k, v, slot, 32 * fewer), got[:fewer * P.tile_elems(n_layer, H, D)])
