"""Prefix sharing across KV slots through the scheduler (Engine(prefix_sharing=True)).

bf16 models test-tiny (D 64) and test-d128, greedy with ignore_eos.  The reference of every request is the same
request run alone on a fresh engine with sharing off (computed once per request, shared, never modified): a
request fed by a copy must return its tokens bitwise -- DESIGN.md §1 item 10 (batch invariance) says a prompt
row's arithmetic does not depend on which rows share its chunk or where its 16-row blocks start, and the copy
moves K/V bits unchanged.

Slot numbers: a fresh engine hands out slot 0 first, then 1, ...; a finished request's slot is the most recently
freed one.  The K/V comparison below relies on that (slots 0 and 1).
"""
import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

MODELS = ["test-tiny", "test-d128"]
SHARE_MIN = 16
GREEDY = dict(temperature=0.0, ignore_eos=True)


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
    """n random token ids (never BOS / EOS); `first` fixes the first one (so two tails differ where they start)."""
    t = [int(x) for x in np.random.default_rng(seed).integers(3, vocab(name), n)]
    if first is not None:
        t[0] = first
    return t


def lcp(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


_alone = {}


def alone(mx, name, prompt, max_tokens, n_ctx=256, q8=False, **kw):
    key = (name, tuple(prompt), max_tokens, n_ctx, q8, tuple(sorted(kw.items())))
    if key not in _alone:
        eng = mx.Engine(model(name, q8), n_ctx=n_ctx, n_seq_max=2)
        _alone[key] = tuple(eng.generate(prompt, max_tokens, **GREEDY, **kw)[0])
        eng.close()
    return list(_alone[key])


def other_first(name, *avoid):
    """A token id that is none of `avoid` (tails that must not continue a recorded sequence by chance)."""
    t = 3
    while t in avoid:
        t += 1
    return t


_two = {}


def two_on_one_slot(mx, name):
    """A (70 tokens) runs to completion; then B and C, both A + a tail of their own, in one submit_batch.  Returns
    what the tests below read: prompts, tokens, counters and the raw caches after the round."""
    if name in _two:
        return _two[name]
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=4, prefix_sharing=True)
    A = [1] + toks(name, 69, 11)
    tA, _ = eng.generate(A, 8, **GREEDY)
    rec = A + tA[:7]  # what A's slot holds K/V for
    fb = other_first(name, tA[0])
    B = A + toks(name, 12, 12, first=fb)
    C = A + toks(name, 9, 13, first=other_first(name, tA[0], fb))
    after_a = (eng.stats(), eng.sharing_stats())
    reqs = eng.submit_many([B, C], 8, **GREEDY)
    tB, tC = (eng.wait(r)[0] for r in reqs)
    info = eng.info
    S = L.ctx_stride(256)
    nbytes = info.n_layer * 4 * info.n_head_kv * S * info.head_dim * 2
    shape = (info.n_layer, 4, info.n_head_kv, S * info.head_dim)
    kc = L.untile_k(eng.debug_read("kcache", nbytes).view(np.uint16).reshape(shape), info.head_dim)
    vc = L.untile_v(eng.debug_read("vcache", nbytes).view(np.uint16).reshape(shape), info.head_dim)
    _two[name] = dict(A=A, B=B, C=C, rec=rec, tA=tA, tB=tB, tC=tC, after_a=after_a, stats=eng.stats(),
                      sharing=eng.sharing_stats(), kc=kc, vc=vc)
    eng.close()
    return _two[name]


@pytest.mark.parametrize("name", MODELS)
def test_two_requests_matching_one_free_slot(mx, name):
    r = two_on_one_slot(mx, name)
    assert lcp(r["B"], r["rec"]) == 70 and lcp(r["C"], r["rec"]) == 70 and lcp(r["B"], r["C"]) == 70
    st0, sh0 = r["after_a"]
    assert st0["reused_prompt_tokens"] == 0 and sh0 == dict.fromkeys(sh0, 0)
    # B takes A's slot in place; C gets its common prefix with A's valid record by one copy
    assert r["stats"]["reused_prompt_tokens"] == 70, r["stats"]
    sh = r["sharing"]
    assert sh["shared_prompt_tokens"] == 70 and sh["copies"] == 1 and sh["follower_requests"] == 0, sh
    info_bytes = sh["copied_bytes"]
    assert info_bytes > 0 and info_bytes % (96 * 2) == 0, sh  # 70 positions travel as 96 (three 32-position tiles)
    assert r["stats"]["prompt_tokens"] == len(r["A"]) + len(r["B"]) + len(r["C"])
    assert r["tA"] == alone(mx, name, r["A"], 8)
    assert r["tB"] == alone(mx, name, r["B"], 8), "in-place reuse differs from the fresh engine"
    assert r["tC"] == alone(mx, name, r["C"], 8), "the request fed by a copy differs from the fresh engine"


@pytest.mark.parametrize("name", MODELS)
def test_copy_leaves_identical_kv_bits(mx, name):
    r = two_on_one_slot(mx, name)
    for what, c in (("K", r["kc"]), ("V", r["vc"])):  # [layer][slot][kv head][position][d]
        src, dst = c[:, 0, :, :70], c[:, 1, :, :70]
        assert src.any(axis=(1, 2, 3)).all(), f"{what}: a layer of the source slot is empty"
        assert np.array_equal(src, dst), f"{what}: slot 1 [0, 70) is not slot 0's"
        assert not c[:, 2:].any(), f"{what}: a slot no request used was written"


@pytest.mark.parametrize("name", MODELS)
def test_busy_source(mx, name):
    eng = mx.Engine(model(name), n_ctx=512, n_seq_max=4, prefix_sharing=True)
    A = [1] + toks(name, 59, 21)
    rA = eng.submit(A, 512, **GREEDY)  # runs to the end of n_ctx
    first, done = eng.poll(rA, 0)
    assert len(first) >= 1 and not done
    B = A + toks(name, 20, 22, first=other_first(name, first[0]))
    tB, _ = eng.wait(eng.submit(B, 8, **GREEDY))
    sh = eng.sharing_stats()
    tA, finA = eng.wait(rA)
    eng.close()
    assert sh["copies"] == 1 and sh["shared_prompt_tokens"] >= len(A) - 1, sh
    assert sh["shared_prompt_tokens"] == len(A), sh  # B leaves A's sequence at its first own token
    assert tB == alone(mx, name, B, 8, n_ctx=512)
    assert finA == mx.FINISH_LENGTH and len(tA) > 400  # it ran to the end of n_ctx, long after B had gone
    assert tA == alone(mx, name, A, 512, n_ctx=512), "the source's own tokens changed"


def header_batch(name, n_header, tails=(5, 12, 16, 23, 31, 40)):
    head = [1] + toks(name, n_header - 1, 31)
    return [head + toks(name, n, 40 + i, first=3 + i) for i, n in enumerate(tails)]


@pytest.mark.parametrize("name", MODELS)
def test_same_round_followers(mx, name):
    prompts = header_batch(name, 100)
    out = {}
    for on in (False, True):
        eng = mx.Engine(model(name), n_ctx=256, n_seq_max=8, prefix_sharing=on)
        out[on] = [eng.wait(r)[0] for r in eng.submit_many(prompts, 8, **GREEDY)]
        st, sh = eng.stats(), eng.sharing_stats()
        eng.close()
        assert st["prompt_tokens"] == sum(len(p) for p in prompts) and st["reused_prompt_tokens"] == 0, st
        if on:
            assert sh["follower_requests"] == 5 and sh["copies"] == 5 and sh["shared_prompt_tokens"] == 500, sh
        else:
            assert sh == dict.fromkeys(sh, 0), sh
    assert out[True] == out[False], "followers differ from the same batch with sharing off"
    for p, t in zip(prompts, out[True]):
        assert t == alone(mx, name, p, 8)


def test_header_shorter_than_share_min_makes_no_copy(mx):
    name = "test-tiny"
    prompts = header_batch(name, SHARE_MIN - 1)
    assert all(lcp(prompts[0], p) == SHARE_MIN - 1 for p in prompts[1:])
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=8, prefix_sharing=True)
    got = [eng.wait(r)[0] for r in eng.submit_many(prompts, 4, **GREEDY)]
    sh = eng.sharing_stats()
    eng.close()
    assert sh == dict.fromkeys(sh, 0), sh
    assert got[0] == alone(mx, name, prompts[0], 4)
    # ... and a header of exactly SHARE_MIN tokens does
    prompts = header_batch(name, SHARE_MIN)
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=8, prefix_sharing=True)
    got = [eng.wait(r)[0] for r in eng.submit_many(prompts, 4, **GREEDY)]
    sh = eng.sharing_stats()
    eng.close()
    assert sh["follower_requests"] == 5 and sh["shared_prompt_tokens"] == 5 * SHARE_MIN, sh
    for p, t in zip(prompts, got):
        assert t == alone(mx, name, p, 4)


def test_switch_off_counts_as_before(mx):
    """The arithmetic of test_engine_gpu.test_prefix_kv_reuse, exact, with the switch never on, and on then off."""
    name = "test-d128"
    for flip in (False, True):
        eng = mx.Engine(model(name), n_ctx=256, n_seq_max=4)
        if flip:
            eng.set_prefix_sharing(True)
            eng.set_prefix_sharing(False)
        p1 = [1] + toks(name, 39, 61)
        t1, _ = eng.generate(p1, 8, **GREEDY)
        rec1 = p1 + t1[:7]
        p2 = rec1 + toks(name, 11, 62, first=other_first(name, t1[7]))
        t2, _ = eng.generate(p2, 8, **GREEDY)
        assert eng.stats()["reused_prompt_tokens"] == 40 + 7  # prompt 1 + its fed-back tokens, in place
        rec2 = p2 + t2[:7]
        p3 = [1] + toks(name, 29, 63)
        t3, _ = eng.generate(p3, 4, **GREEDY)
        st, sh = eng.stats(), eng.sharing_stats()
        eng.close()
        assert st["reused_prompt_tokens"] == 47 + lcp(p3, rec2) and lcp(p3, rec2) < SHARE_MIN, st
        assert st["prompt_tokens"] == len(p1) + len(p2) + len(p3)
        assert sh == dict.fromkeys(sh, 0), sh
        assert t2 == alone(mx, name, p2, 8) and t3 == alone(mx, name, p3, 4)


@pytest.mark.parametrize("name", MODELS)
def test_speculating_source(mx, name):
    """A live speculating request: the K/V of its rejected drafts lie past its kept position and must not be
    shared -- B continues A's kept output and then leaves it."""
    block = toks(name, 12, 100)
    A = [1] + block + block  # the lookup has something to find
    eng = mx.Engine(model(name), n_ctx=512, n_seq_max=4, prefix_sharing=True)
    rA = eng.submit(A, 512, draft=(4, 2), **GREEDY)
    seen, done = [], False
    while len(seen) < 12 and not done:
        seen, done = eng.poll(rA, len(seen))
    assert not done
    k = len(seen) - 1  # tokens whose K/V A's slot holds for sure
    B = A + seen[:k] + toks(name, 10, 101, first=other_first(name, seen[k]))
    tB, _ = eng.wait(eng.submit(B, 8, **GREEDY))
    sh = eng.sharing_stats()
    spec = eng.spec_stats(rA)
    tA, _ = eng.wait(rA)
    eng.close()
    assert spec["steps"] > 0 and spec["drafted"] > spec["accepted"], spec  # drafts were rejected
    assert sh["copies"] == 1 and sh["shared_prompt_tokens"] == len(A) + k, sh
    assert tB == alone(mx, name, B, 8, n_ctx=512)
    assert tA == alone(mx, name, A, 512, n_ctx=512)


def test_embedding_source_and_prompt_logprobs(mx):
    name = "test-tiny"
    eng = mx.Engine(model(name), n_ctx=256, n_seq_max=4, prefix_sharing=True)
    E = [1] + toks(name, 59, 71)
    eng.embed([E], pooling=mx.POOL_MEAN)
    assert eng.sharing_stats()["copies"] == 0
    B, C = E + toks(name, 7, 72, first=5), E + toks(name, 19, 73, first=6)
    tB, tC = (eng.wait(r)[0] for r in eng.submit_many([B, C], 8, **GREEDY))
    sh = eng.sharing_stats()
    assert eng.stats()["reused_prompt_tokens"] == 60 and sh["copies"] == 1 and sh["shared_prompt_tokens"] == 60, sh
    assert tB == alone(mx, name, B, 8) and tC == alone(mx, name, C, 8)
    # a request with prompt log-probabilities evaluates its whole prompt: no reuse, no copy
    # (B's and C's slots both hold E: whichever P takes, the other could have been the source of 60 positions)
    P = E + toks(name, 30, 74, first=7)
    before = (eng.stats()["reused_prompt_tokens"], eng.sharing_stats())
    req = eng.submit(P, 8, logprobs=0, prompt_logprobs=True, **GREEDY)
    assert len(eng.poll(req, 7)[0]) == 8
    assert len(eng.logprobs(req)[0]) == len(P) - 1 + 8  # every prompt position >= 1, then the 8 tokens
    tP, _ = eng.wait(req)
    assert (eng.stats()["reused_prompt_tokens"], eng.sharing_stats()) == before
    assert tP == alone(mx, name, P, 8, logprobs=0, prompt_logprobs=True)
    # ... and its slot serves as a source afterwards: Q takes it in place (90), R holds E (60) and copies up to 90
    fq = other_first(name, tP[0])
    Q, R = P + toks(name, 5, 75, first=fq), P + toks(name, 6, 76, first=other_first(name, tP[0], fq))
    tQ, tR = (eng.wait(r)[0] for r in eng.submit_many([Q, R], 4, **GREEDY))
    st2, sh2 = eng.stats(), eng.sharing_stats()
    eng.close()
    assert sh2["copies"] == 2 and sh2["shared_prompt_tokens"] == 60 + 30, sh2
    assert st2["reused_prompt_tokens"] == before[0] + 90 + 60, st2
    assert tQ == alone(mx, name, Q, 4) and tR == alone(mx, name, R, 4)


def test_q8_copy_equals_in_place_reuse(mx):
    """Q8_0 rows are not batch invariant, so the comparison keeps every launch the same: a long request L = A
    keeps its slot busy and decodes next to C both times; C = A + a tail starts from 70 positions evaluated by the
    same launches (A alone in its chunk) -- held by C's own slot (sharing off, in place) or copied from L's."""
    name = "test-tiny"
    A = [1] + toks(name, 69, 81)
    got = {}
    for share in (False, True):
        eng = mx.Engine(model(name, q8=True), n_ctx=1024, n_seq_max=4)
        rL = eng.submit(A, 1024, **GREEDY)
        first, done = eng.poll(rL, 0)
        assert not done
        C = A + toks(name, 12, 82, first=other_first(name, first[0]))
        if share:
            eng.set_prefix_sharing(True)
        else:
            assert eng.generate(A, 1, **GREEDY)[0] == first[:1]  # a free slot that holds A, evaluated alone
        rC = eng.submit(C, 8, **GREEDY)
        got[share], _ = eng.wait(rC)
        _, still = eng.poll(rL, 0)
        st, sh = eng.stats(), eng.sharing_stats()
        eng.cancel(rL)
        eng.wait(rL)
        eng.close()
        assert not still, "L finished before C: the two runs did not decode the same batch"
        if share:
            assert sh["copies"] == 1 and sh["shared_prompt_tokens"] == 70 and st["reused_prompt_tokens"] == 0, (st, sh)
        else:
            assert sh["copies"] == 0 and st["reused_prompt_tokens"] == 70, (st, sh)
    assert len(got[True]) == 8 and got[True] == got[False]


def test_pipeline_stage_engine_refuses(mx):
    stage = mx.Engine(model("test-tiny"), n_ctx=64, n_seq_max=2, layer_end=1)
    with pytest.raises(mx.MxError) as ei:
        stage.set_prefix_sharing(True)
    assert ei.value.code == mx.MX_ERR_STATE
    stage.close()
    with pytest.raises(mx.MxError) as ei:
        mx.Engine(model("test-tiny"), n_ctx=64, n_seq_max=2, layer_begin=1, prefix_sharing=True)
    assert ei.value.code == mx.MX_ERR_STATE
