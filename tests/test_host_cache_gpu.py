"""The host-RAM tier behind the KV slots through the scheduler (Engine(host_cache_bytes=...)).

bf16 models test-tiny (D 64) and test-d128, greedy with ignore_eos.  The reference of every request is the same
request run alone on a fresh engine without the tier (computed once per request, shared, never modified): a
request fed by a restore must return its tokens bitwise -- the spill and the restore move K/V bits unchanged, and
DESIGN.md §1 item 10 (batch invariance) makes a prompt row's arithmetic independent of its chunk-mates.

n_seq_max = 1 unless said otherwise, so every admission that does not match the slot's record destroys it.  A
request of max_tokens = 1 leaves exactly its prompt as the slot's record (the last generated token is never fed
back); one of max_tokens = 8 leaves prompt + 7 tokens.
"""
import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

MODELS = ["test-tiny", "test-d128"]
HOST_MIN = 32
GREEDY = dict(temperature=0.0, ignore_eos=True)
BIG = 1 << 26


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def model(name, q8=False):
    return f"synthetic:{name}:seed=0" + (":q8_0" if q8 else "")


def vocab(name):
    from llama_p2p_amd import synth

    return synth.SHAPES[name].n_vocab


def toks(name, n, seed, first=None):
    """n random token ids (never BOS / EOS); `first` fixes the first one."""
    t = [int(x) for x in np.random.default_rng(seed).integers(3, vocab(name), n)]
    if first is not None:
        t[0] = first
    return t


def lcp(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def other_first(*avoid):
    t = 3
    while t in avoid:
        t += 1
    return t


_alone = {}


def alone(mx, name, prompt, max_tokens, n_ctx=256, **kw):
    key = (name, tuple(prompt), max_tokens, n_ctx, tuple(sorted(kw.items())))
    if key not in _alone:
        eng = mx.Engine(model(name), n_ctx=n_ctx, n_seq_max=2)
        _alone[key] = tuple(eng.generate(prompt, max_tokens, **GREEDY, **kw)[0])
        eng.close()
    return list(_alone[key])


def pos_bytes(eng):
    i = eng.info
    return i.n_layer * 2 * i.n_head_kv * i.head_dim * 2


def gen(eng, prompt, n=1, **kw):
    return eng.generate(prompt, n, **GREEDY, **kw)[0]


def read_slot0(eng, n_ctx=256):
    """K and V of slot 0 of a one-slot engine, untiled: [layer][kv head][position][d] uint16 each."""
    i = eng.info
    S = L.ctx_stride(n_ctx)
    nbytes = i.n_layer * i.n_head_kv * S * i.head_dim * 2
    shape = (i.n_layer, i.n_head_kv, S * i.head_dim)
    k = L.untile_k(eng.debug_read("kcache", nbytes).view(np.uint16).reshape(shape), i.head_dim)
    v = L.untile_v(eng.debug_read("vcache", nbytes).view(np.uint16).reshape(shape), i.head_dim)
    return k, v


def abc(name):
    A = [1] + toks(name, 69, 11)
    B = toks(name, 40, 12, first=7)
    return A, B


_evict = {}


def evict_and_restore(mx, name, capacity=BIG, keyword=True):
    """A (70 tokens, 8 generated), unrelated B (40 tokens), then C = A + a 12-token tail, on one slot."""
    key = (name, capacity, keyword)
    if key in _evict:
        return _evict[key]
    kw = dict(host_cache_bytes=capacity) if keyword else {}
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, **kw)
    A, B = abc(name)
    tA = gen(eng, A, 8)
    after_a = eng.host_cache_stats()
    tB = gen(eng, B, 4)
    after_b, st_b = eng.host_cache_stats(), eng.stats()
    C = A + toks(name, 12, 13, first=other_first(tA[0]))
    tC = gen(eng, C, 8)
    k, v = read_slot0(eng)
    _evict[key] = dict(A=A, B=B, C=C, tA=tA, tB=tB, tC=tC, after_a=after_a, after_b=after_b, st_b=st_b,
                       host=eng.host_cache_stats(), stats=eng.stats(), sharing=eng.sharing_stats(), k=k, v=v,
                       pos_bytes=pos_bytes(eng))
    eng.close()
    return _evict[key]


@pytest.mark.parametrize("name", MODELS)
def test_evict_and_restore(mx, name):
    r = evict_and_restore(mx, name)
    pb = r["pos_bytes"]
    assert lcp(r["C"], r["A"] + r["tA"][:7]) == 70 and lcp(r["B"], r["A"]) == 0
    assert r["after_a"]["spills"] == 0 and r["after_a"]["entries"] == 0
    hb = r["after_b"]  # A's record, 77 tokens, left as 96 positions
    assert hb["spills"] == 1 and hb["entries"] == 1 and hb["bytes"] == 96 * pb and hb["spilled_bytes"] == 96 * pb, hb
    assert hb["restores"] == 0 and hb["capacity_bytes"] == BIG
    h = r["host"]
    assert h["restores"] == 1 and h["restored_prompt_tokens"] == 70 and h["restored_bytes"] == 96 * pb, h
    assert h["spills"] == 2 and h["entries"] == 2 and h["evictions"] == 0 and h["skipped"] == 0, h  # B's record too
    assert r["stats"]["reused_prompt_tokens"] == r["st_b"]["reused_prompt_tokens"] == 0, r["stats"]
    assert r["sharing"] == dict.fromkeys(r["sharing"], 0)
    assert r["tA"] == alone(mx, name, r["A"], 8) and r["tB"] == alone(mx, name, r["B"], 4)
    assert r["tC"] == alone(mx, name, r["C"], 8), "the request fed by a restore differs from the fresh engine"


@pytest.mark.parametrize("name", MODELS)
def test_restore_leaves_identical_kv_bits(mx, name):
    r = evict_and_restore(mx, name)
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1)
    assert gen(eng, r["C"], 8) == r["tC"]
    k, v = read_slot0(eng)
    eng.close()
    for what, got, ref in (("K", r["k"], k), ("V", r["v"], v)):  # [layer][kv head][position][d]
        assert ref[:, :, :70].any(axis=(1, 2, 3)).all(), f"{what}: a layer of the reference is empty"
        assert np.array_equal(got[:, :, :70], ref[:, :, :70]), f"{what}: [0, 70) is not what a fresh engine computes"


def test_off_means_off(mx):
    name = "test-d128"
    off, plain = evict_and_restore(mx, name, capacity=0), evict_and_restore(mx, name, keyword=False)
    for r in (off, plain):
        assert r["host"] == dict.fromkeys(r["host"], 0), r["host"]
    for key in ("stats", "sharing", "tA", "tB", "tC"):
        assert off[key] == plain[key], key
    assert off["tC"] == alone(mx, name, off["C"], 8)
    # switched on and off again before any request: nothing is kept either
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1)
    eng.set_host_cache(BIG)
    eng.set_host_cache(0)
    A, B = abc(name)
    gen(eng, A), gen(eng, B), gen(eng, A)
    h, st = eng.host_cache_stats(), eng.stats()
    eng.close()
    assert h == dict.fromkeys(h, 0) and st["reused_prompt_tokens"] == 0


def test_spill_threshold(mx):
    name = "test-tiny"
    for n_prompt, spills in ((HOST_MIN - 8, 0), (HOST_MIN - 7, 1)):  # records of 31 and of 32 tokens
        eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
        gen(eng, [1] + toks(name, n_prompt - 1, 21), 8)
        gen(eng, toks(name, 40, 22, first=7))
        h = eng.host_cache_stats()
        eng.close()
        assert h["spills"] == spills and h["entries"] == spills, (n_prompt, h)


def test_restore_threshold(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    A, B = abc(name)
    firsts = [other_first(A[6], A[37], A[38]) + i for i in range(8)]
    firsts = [f for f in firsts if f not in (A[6], A[37], A[38])]
    gen(eng, A), gen(eng, B)
    assert eng.host_cache_stats()["entries"] == 1
    for round_, longer in ((0, 37), (1, 38)):  # a host match of cur + 31, then of cur + 32, with cur = 6
        s1 = A[:6] + toks(name, 30, 30 + round_, first=firsts[2 * round_])
        s2 = A[:longer] + toks(name, 10, 40 + round_, first=firsts[2 * round_ + 1])
        assert gen(eng, s1) == alone(mx, name, s1, 1)
        assert eng.host_cache_stats()["restores"] == 0  # 6 positions on the host, 0 in the slot
        reused = eng.stats()["reused_prompt_tokens"]
        t2 = gen(eng, s2)
        h = eng.host_cache_stats()
        assert eng.stats()["reused_prompt_tokens"] == reused + 6
        assert t2 == alone(mx, name, s2, 1)
        if round_ == 0:
            assert h["restores"] == 0 and h["restored_prompt_tokens"] == 0, h
            gen(eng, toks(name, 40, 50, first=8))  # the slot matches nothing again
        else:
            assert h["restores"] == 1 and h["restored_prompt_tokens"] == 32, h
            assert h["restored_bytes"] == 64 * pos_bytes(eng), h  # 38 positions travel as two tiles
    eng.close()


def test_record_covered_by_another_slot_is_not_spilled(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=2, host_cache_bytes=BIG)
    head = [1] + toks(name, 59, 61)
    X, Y = head + toks(name, 20, 62, first=5), head + toks(name, 10, 63, first=6)
    for r in eng.submit_many([X, Y], 1, **GREEDY):
        eng.wait(r)
    # both slots are free; whichever the next request takes, the other covers its record to within 20 / 10
    gen(eng, toks(name, 40, 64, first=7))
    h = eng.host_cache_stats()
    assert h["spills"] == 0 and h["entries"] == 0, h
    # two more take both slots: the 40-token record and the one that now stands alone both leave
    for r in eng.submit_many([toks(name, 40, 65, first=8), toks(name, 40, 66, first=9)], 1, **GREEDY):
        eng.wait(r)
    h = eng.host_cache_stats()
    eng.close()
    assert h["spills"] == 2 and h["entries"] == 2, h


def test_record_a_host_entry_covers_is_not_spilled_again_and_counts_as_used(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    A = [1] + toks(name, 69, 11)
    B, C, D = (toks(name, 70, 70 + i, first=7 + i) for i in range(3))
    gen(eng, A), gen(eng, B), gen(eng, C)  # entries A, B, in that order of use
    req = eng.submit(A, 1, logprobs=0, prompt_logprobs=True, **GREEDY)  # evaluates A whole: no restore; C leaves
    eng.wait(req)
    h = eng.host_cache_stats()
    assert h["spills"] == 3 and h["entries"] == 3 and h["restores"] == 0, h
    gen(eng, D)  # the slot's record is A again, and entry A holds it: nothing is written, entry A is the newest
    h = eng.host_cache_stats()
    assert h["spills"] == 3 and h["entries"] == 3, h
    entry = 96 * pos_bytes(eng)
    assert h["bytes"] == 3 * entry
    eng.set_host_cache(2 * entry)  # the least recently used goes: B, not A
    h = eng.host_cache_stats()
    assert h["entries"] == 2 and h["evictions"] == 1 and h["bytes"] == 2 * entry, h
    A2 = A + toks(name, 5, 80, first=3)
    assert gen(eng, A2) == alone(mx, name, A2, 1)
    h = eng.host_cache_stats()
    eng.close()
    assert h["restores"] == 1 and h["restored_prompt_tokens"] == 70, h


def test_budget(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1)
    entry = 96 * pos_bytes(eng)
    eng.set_host_cache(2 * entry)
    P = [[1] + toks(name, 69, 90 + i, first=10 + i) for i in range(4)]
    for p in P:
        gen(eng, p)  # three evictions: entries 0, 1, 2 in turn; the third pushes entry 0 out
    h = eng.host_cache_stats()
    assert h["spills"] == 3 and h["entries"] == 2 and h["evictions"] == 1 and h["bytes"] == 2 * entry, h
    assert h["capacity_bytes"] == 2 * entry and h["skipped"] == 0
    gone = P[0] + toks(name, 5, 95, first=3)
    assert gen(eng, gone) == alone(mx, name, gone, 1)
    h = eng.host_cache_stats()
    assert h["restores"] == 0 and h["entries"] == 2, h  # (entry 3 came in, entry 1 went)
    kept = P[2] + toks(name, 5, 96, first=3)
    assert gen(eng, kept) == alone(mx, name, kept, 1)
    h = eng.host_cache_stats()
    # 70 positions come back; the slot's own match with `gone`'s record is the BOS, which counts as reused in place
    assert h["restores"] == 1 and h["restored_prompt_tokens"] == 70 - 1 and h["bytes"] <= 2 * entry, h
    assert h["restored_bytes"] == entry
    # lowering the capacity evicts at once
    ev = h["evictions"]
    eng.set_host_cache(entry)
    h = eng.host_cache_stats()
    assert h["entries"] == 1 and h["bytes"] == entry and h["evictions"] == ev + 1 and h["capacity_bytes"] == entry, h
    # an entry larger than the capacity is not stored
    eng.set_host_cache(entry - 16)
    assert eng.host_cache_stats()["entries"] == 0
    gen(eng, P[3])
    h = eng.host_cache_stats()
    assert h["skipped"] == 1 and h["entries"] == 0 and h["bytes"] == 0, h
    # ... and capacity 0 empties the store and switches the tier off
    eng.set_host_cache(BIG)
    gen(eng, P[0]), gen(eng, P[1])
    assert eng.host_cache_stats()["entries"] == 2
    eng.set_host_cache(0)
    h = eng.host_cache_stats()
    assert h["entries"] == 0 and h["bytes"] == 0 and h["capacity_bytes"] == 0, h
    sp = h["spills"]
    assert gen(eng, P[2]) == alone(mx, name, P[2], 1)
    h = eng.host_cache_stats()
    eng.close()
    assert h["spills"] == sp and h["entries"] == 0


def test_subsumption(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    A = [1] + toks(name, 69, 11)
    gen(eng, A)
    gen(eng, toks(name, 20, 100, first=7))  # a record too short to be kept itself
    pb = pos_bytes(eng)
    h = eng.host_cache_stats()
    assert h["entries"] == 1 and h["bytes"] == 96 * pb, h
    C = A + toks(name, 40, 101, first=3)
    assert gen(eng, C) == alone(mx, name, C, 1)
    assert eng.host_cache_stats()["restores"] == 1
    gen(eng, toks(name, 20, 102, first=8))  # C's record (110 tokens) leaves: entry A is a prefix of it and goes
    h = eng.host_cache_stats()
    eng.close()
    assert h["entries"] == 1 and h["bytes"] == 128 * pb and h["spills"] == 2 and h["evictions"] == 0, h


@pytest.mark.parametrize("name", MODELS)
def test_with_sharing_on(mx, name):
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=4, prefix_sharing=True, host_cache_bytes=BIG)
    first = [toks(name, 70, 110 + i, first=10 + i) for i in range(4)]  # no common first token: every match is 0
    A, U = first[0], first[1]
    for r in eng.submit_many(first, 1, **GREEDY):
        eng.wait(r)
    for r in eng.submit_many([toks(name, 40, 120 + i, first=20 + i) for i in range(4)], 1, **GREEDY):
        eng.wait(r)
    h = eng.host_cache_stats()
    assert h["spills"] == 4 and h["entries"] == 4 and h["restores"] == 0, h
    assert gen(eng, A) == alone(mx, name, A, 1)  # A comes back from the host into a free slot
    h, sh = eng.host_cache_stats(), eng.sharing_stats()
    assert h["restores"] == 1 and h["restored_prompt_tokens"] == 69 and sh["copies"] == 0, (h, sh)
    # a device source of equal length wins: one takes A's slot in place, the other copies from it
    C1, C2 = A + toks(name, 12, 130, first=3), A + toks(name, 9, 131, first=4)
    t1, t2 = (eng.wait(r)[0] for r in eng.submit_many([C1, C2], 8, **GREEDY))
    h2, sh2 = eng.host_cache_stats(), eng.sharing_stats()
    assert sh2["copies"] == 1 and sh2["shared_prompt_tokens"] == 70 and h2["restores"] == 1, (h2, sh2)
    assert t1 == alone(mx, name, C1, 8) and t2 == alone(mx, name, C2, 8)
    # U is on the host only: the first request gets it back and leads the second, which shares 20 tokens more
    both = U + toks(name, 20, 132, first=3)
    F1, F2 = both + toks(name, 6, 133, first=5), both + toks(name, 11, 134, first=6)
    t1, t2 = (eng.wait(r)[0] for r in eng.submit_many([F1, F2], 8, **GREEDY))
    h3, sh3 = eng.host_cache_stats(), eng.sharing_stats()
    eng.close()
    assert h3["restores"] == 2 and h3["restored_prompt_tokens"] == 69 + 70, h3
    assert sh3["follower_requests"] == 1 and sh3["copies"] == 2 and sh3["shared_prompt_tokens"] == 70 + 90, sh3
    assert t1 == alone(mx, name, F1, 8) and t2 == alone(mx, name, F2, 8)


def test_not_served(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    A, B = abc(name)
    gen(eng, A), gen(eng, B)
    assert eng.host_cache_stats()["spills"] == 1
    # prompt log-probabilities: the whole prompt is evaluated, nothing comes from the host
    P = A + toks(name, 40, 140, first=3)
    req = eng.submit(P, 4, logprobs=0, prompt_logprobs=True, **GREEDY)
    tP, _ = eng.wait(req)
    h = eng.host_cache_stats()
    assert h["restores"] == 0 and h["spills"] == 2, h  # (B's record left)
    assert tP == alone(mx, name, P, 4, logprobs=0, prompt_logprobs=True)
    gen(eng, toks(name, 40, 141, first=8))
    assert eng.host_cache_stats()["spills"] == 3  # its slot's record is spilled like any other
    # an embedding request
    E = A + toks(name, 40, 142, first=4)
    eng.embed([E], pooling=mx.POOL_MEAN)
    h = eng.host_cache_stats()
    assert h["restores"] == 0 and h["spills"] == 4, h
    gen(eng, toks(name, 40, 143, first=9))
    h = eng.host_cache_stats()
    assert h["restores"] == 0 and h["spills"] == 5, h
    # ... and what they left serves a completion
    E2 = E + toks(name, 3, 144, first=3)
    assert gen(eng, E2, 4) == alone(mx, name, E2, 4)
    h = eng.host_cache_stats()
    eng.close()
    assert h["restores"] == 1 and h["restored_prompt_tokens"] == len(E), h


def test_q8_restore_equals_in_place_reuse(mx):
    """Q8_0 rows are not batch invariant, so the comparison keeps every launch the same: A is evaluated alone in
    its chunk both times, and C = A + a tail starts from those 70 positions -- still in the slot, or evicted by B
    and restored -- with the same prefill rows and the same one-row decode steps."""
    name = "test-tiny"
    A, B = abc(name)
    got = {}
    for restore in (False, True):
        eng = mx.Engine(model(name, q8=True), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG if restore else 0)
        tA = gen(eng, A)
        if restore:
            gen(eng, B)
        C = A + toks(name, 12, 150, first=other_first(tA[0]))
        got[restore] = gen(eng, C, 8)
        h, st = eng.host_cache_stats(), eng.stats()
        eng.close()
        if restore:
            assert h["restores"] == 1 and h["restored_prompt_tokens"] == 70 and st["reused_prompt_tokens"] == 0, (h, st)
        else:
            assert h["restores"] == 0 and st["reused_prompt_tokens"] == 70, (h, st)
    assert len(got[True]) == 8 and got[True] == got[False]


def test_teardown_and_stage_engines(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    A, B = abc(name)
    gen(eng, A)
    gen(eng, B)  # this round queued a spill: its transfer may still be in flight
    eng.close()
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=1, host_cache_bytes=BIG)
    gen(eng, A)
    eng.submit(B, 64, **GREEDY)  # ... and with the request still running
    eng.close()
    stage = mx.Engine(model(name), n_ctx=64, n_seq_max=2, layer_end=1)
    with pytest.raises(mx.MxError) as ei:
        stage.set_host_cache(1 << 20)
    assert ei.value.code == mx.MX_ERR_STATE
    stage.close()
    with pytest.raises(mx.MxError) as ei:
        mx.Engine(model(name), n_ctx=64, n_seq_max=2, layer_begin=1, host_cache_bytes=1 << 20)
    assert ei.value.code == mx.MX_ERR_STATE


def test_through_llama(mx):
    from llama_p2p_amd.llama import Llama
    from llama_p2p_amd.llama_cache import LlamaRAMCache

    name = "test-tiny"
    llm = Llama(model(name), n_ctx=256, n_seq_max=1, verbose=False)
    cache = LlamaRAMCache(capacity_bytes=1 << 20)
    assert cache.cache_size == 0
    llm.set_cache(cache)
    P1, P2 = [1] + toks(name, 69, 160), [1] + toks(name, 50, 161, first=9)
    first = llm.create_completion(P1, max_tokens=8, temperature=0.0)["choices"][0]["text"]
    llm.create_completion(P2, max_tokens=8, temperature=0.0)
    assert cache.cache_size > 0 and cache.cache_size == llm._engine.host_cache_stats()["bytes"]
    again = llm.create_completion(P1, max_tokens=8, temperature=0.0)["choices"][0]["text"]
    h = llm._engine.host_cache_stats()
    assert again == first and h["restores"] == 1, h
    llm.set_cache(None)
    assert cache.cache_size == 0 and llm._engine.host_cache_stats()["entries"] == 0
    llm.close()
