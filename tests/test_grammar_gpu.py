"""Grammar-constrained sampling through the engine: create_completion(grammar=) and
Engine.submit(grammar=) on the device -- the language of the text, every token against the reference's allowed set
(tests/grammar_ref.py), the device picks against the host sampler (a fresh engine with MX_NO_DEV_TOPK), greedy
against the argmax over the allowed set of the row a second engine computes, mixed rounds, log-probabilities, a
draft model, dead ends and the Llama front."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grammar_ref import BOUNDED, RefGrammar  # noqa: E402  BOUNDED: root ::= ("yes" | "no") " " [a-z]{3,5} "."

pytestmark = pytest.mark.gpu

MODEL = "synthetic:test-tiny:seed=0"  # V = 512
BIG = "synthetic:test-8b-v128k:seed=0"  # the real vocabulary width
LANG = re.compile(r"(yes|no) [a-z]{3,5}\.")
WORDS = 'root ::= ([a-z]{1,6} " "){4,6} "."\n'  # at most 6 x 7 + 1 tokens, then the end-of-generation token
MAXT = 24  # "yes" / "no" and the letters one piece each at worst: 3 + 1 + 5 + 1, then the end-of-generation token
PROMPTS = [[1, 17, 99, 5, 23], [1, 400, 401, 402], [1, 7] * 9]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def spm(n):
    from llama_p2p_amd.gguf import synthetic_spm_vocab
    from llama_p2p_amd.tokenizer import Tokenizer

    toks, scores, types = synthetic_spm_vocab(n)
    tk = Tokenizer(toks, scores, types, "llama", bos_id=1, eos_id=2)
    return [tk.token_to_piece(t) for t in range(n)], [t for t in range(n) if tk.is_eog(t)]


@pytest.fixture(scope="module")
def tiny(mx):
    pieces, eog = spm(512)
    return pieces, eog, mx.GrammarVocab(pieces, eog)


def text_of(pieces, eog, toks):
    return b"".join(pieces[t] for t in toks if t not in eog)


def check_allowed(ref, pieces, eog, toks, what=""):
    """Every token is in the reference's allowed set at its step."""
    gen = b""
    for k, t in enumerate(toks):
        assert ref.allows(pieces[t], t in eog, gen), f"{what}: step {k} token {t} {pieces[t]!r} after {gen!r}"
        if t not in eog:
            gen += pieces[t]


def test_completions_match_the_language(mx):
    """Fails without the feature: grammar= used to be swallowed and the text was unconstrained."""
    from llama_p2p_amd.llama import Llama
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    llm = Llama(model_path=MODEL, n_ctx=128, verbose=False, n_seq_max=2)
    g = LlamaGrammar.from_string(BOUNDED)
    for kw in (dict(temperature=0.0), dict(temperature=0.8, seed=3), dict(temperature=1.0, top_k=0, seed=4)):
        out = llm("The quick brown fox", max_tokens=MAXT, grammar=g, **kw)
        text, why = out["choices"][0]["text"], out["choices"][0]["finish_reason"]
        assert LANG.fullmatch(text), (kw, text)
        assert why == "stop", (kw, why)
        free = llm("The quick brown fox", max_tokens=MAXT, **kw)["choices"][0]["text"]
        assert free != text and not LANG.fullmatch(free)
    assert len(g._compiled) == 1  # compiled once for this Llama
    llm.close()


def test_every_token_is_in_the_reference_allowed_set(mx, tiny):
    pieces, eog, gv = tiny
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    for text in (BOUNDED, WORDS):
        g, ref = mx.CompiledGrammar(gv, text), RefGrammar(text)
        for i, kw in enumerate((dict(temperature=0.0), dict(temperature=0.8, top_k=40), dict(temperature=1.0, top_k=0))):
            toks, fin = eng.generate(PROMPTS[i], 64, grammar=g, seed=11 + i, **kw)
            check_allowed(ref, pieces, eog, toks, f"{text!r} {kw}")
            assert fin == mx.FINISH_STOP and toks[-1] in eog and ref.may_end(text_of(pieces, eog, toks))
    eng.close()


def settings(pieces):
    banned = pieces.index(b"Q")  # no capital letter is ever allowed by BOUNDED
    return banned, [dict(temperature=0.0),
                    dict(temperature=0.8, top_k=40),
                    dict(temperature=0.8, top_k=0),
                    dict(temperature=1.0, mirostat_mode=2, mirostat_tau=3.0, mirostat_eta=0.2),
                    dict(temperature=0.8, top_k=40, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1,
                         repeat_last_n=32, logit_bias={banned: 100.0})]


def run_all(eng, g, kws):
    out = []
    for kw in kws:
        before = eng.sampler_stats()
        alone = [eng.generate(p, MAXT, seed=1000 + i, grammar=g, **kw) for i, p in enumerate(PROMPTS)]
        mid = eng.sampler_stats()
        # three at once: behind a plain request that holds the engine for some rounds, so that the scheduler finds
        # all three waiting when it next admits (submit() queues one request per call)
        hold = eng.submit([1, 9, 8, 7], 64, ignore_eos=True)
        reqs = [eng.submit(p, MAXT, seed=1000 + i, grammar=g, **kw) for i, p in enumerate(PROMPTS)]
        many = [eng.wait(r) for r in reqs]
        eng.cancel(hold)
        eng.wait(hold)
        after = eng.sampler_stats()
        st = {k: mid[k] - before[k] for k in after}
        st["alone_rounds"] = mid["rounds"] - before["rounds"]
        st["many_rounds"] = after["rounds"] - mid["rounds"]
        out.append((alone, many, st))
    return out


def test_device_picks_equal_host_sampler(mx, tiny, monkeypatch):
    pieces, eog, gv = tiny
    banned, kws = settings(pieces)
    g, ref = mx.CompiledGrammar(gv, BOUNDED), RefGrammar(BOUNDED)
    dev = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    got = run_all(dev, g, kws)
    dev.close()
    monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    host = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    want = run_all(host, g, kws)
    host.close()
    for kw, (alone, many, st), (h_alone, h_many, hst) in zip(kws, got, want):
        print(kw, st, [len(t) for t, _ in alone])
        assert alone == h_alone, kw
        assert many == h_many, kw
        assert [t for t, _ in many] == [t for t, _ in alone], kw  # batch invariance of the bf16 path
        for toks, fin in alone + many:
            assert fin == mx.FINISH_STOP and LANG.fullmatch(text_of(pieces, eog, toks).decode()), (kw, toks)
            assert banned not in toks
            check_allowed(ref, pieces, eog, toks, str(kw))
        assert st["host_steps"] == 0, kw
        assert st["rounds"] == st["device_steps"] > 0, kw  # a round with a grammar row runs one step
        # the three at once shared rounds (M > 1): one after another they take alone_rounds, and the plain request
        # beside them adds one or two rounds of its own before they arrive
        assert st["many_rounds"] < st["alone_rounds"], (kw, st)
        if kw["temperature"] > 0 or "logit_bias" in kw:
            assert hst["device_steps"] == 0 and hst["host_steps"] == hst["rounds"] > 0, kw


def test_greedy_is_the_argmax_over_the_allowed_set(mx, tiny):
    """Against rows a second engine computes for the same contexts with forward_logits (prefill rows, where the
    request decoded): equal wherever the two best allowed logits differ by more than the decode-versus-prefill
    tolerance the project's tests use (2 x conftest.logit_tol), and at most 5 % of the steps are not judged.  The
    contexts are grammar_ref.GREEDY_CASES; tests/test_grammar_host.py shows on the CPU oracle that they are decided."""
    import grammar_ref as R

    pieces, eog, gv = tiny
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=2)
    other = mx.Engine(MODEL, n_ctx=128, n_seq_max=2)
    judged = skipped = 0
    for text, seed in R.GREEDY_CASES:
        g, ref, p = mx.CompiledGrammar(gv, text), RefGrammar(text), R.greedy_prompt(seed)
        toks, fin = eng.generate(p, R.GREEDY_MAX_TOKENS, grammar=g)
        assert fin == mx.FINISH_STOP
        rows = other.forward_logits(p + toks[:-1])[len(p) - 1:]
        gen = b""
        for k, t in enumerate(toks):
            ok = np.array(ref.allowed(pieces, eog, gen), dtype=bool)
            best, gap = R.masked_top2(rows[k], ok)
            print(f"case {seed} step {k}: token {t} best {best} gap {gap:.4f} tol {R.greedy_tol(rows[k]):.4f}")
            assert ok[t]
            if gap > R.greedy_tol(rows[k]):
                judged += 1
                assert t == best, f"case {seed} step {k}: picked {t} ({rows[k][t]:.4f}), allowed argmax {best} ({rows[k][best]:.4f})"
            else:
                skipped += 1
            if t not in eog:
                gen += pieces[t]
    eng.close()
    other.close()
    print(f"judged {judged} skipped {skipped}")
    assert judged >= 60 and skipped <= 0.05 * (judged + skipped)


def test_mixed_round(mx, tiny):
    pieces, eog, gv = tiny
    G = 64
    g = mx.CompiledGrammar(gv, BOUNDED)
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    per = [dict(temperature=0.0), dict(temperature=0.8, top_k=40),
           dict(temperature=1.0, mirostat_mode=2, mirostat_tau=1.0, mirostat_eta=0.5)]
    gkw = dict(temperature=0.8, top_k=40, seed=53, grammar=g)
    alone = [eng.generate(p, G, seed=50 + i, ignore_eos=True, **kw)[0] for i, (p, kw) in enumerate(zip(PROMPTS, per))]
    g_alone = eng.generate([1, 33, 34], MAXT, **gkw)[0]
    before = eng.sampler_stats()
    plain = eng.submit_many(PROMPTS, G, seeds=[50, 51, 52], ignore_eos=True, per_request=per)
    gr = eng.submit([1, 33, 34], MAXT, **gkw)
    g_many = eng.wait(gr)[0]
    # the plain requests were running while the grammar request lived: all four rows shared its rounds
    state = [eng.poll(r, 0) for r in plain]
    many = [eng.wait(r)[0] for r in plain]
    after = eng.sampler_stats()
    eng.close()
    assert all(not done and 0 < len(t) < G for t, done in state), [(len(t), done) for t, done in state]
    assert many == alone and g_many == g_alone
    assert len(g_many) < MAXT and all(len(t) == G for t in many)
    assert after["host_steps"] == before["host_steps"] == 0
    # once the grammar request has ended the rounds run several steps again
    assert after["rounds"] - before["rounds"] < after["device_steps"] - before["device_steps"]


def test_logprobs_report_the_raw_row(mx, tiny, monkeypatch):
    pieces, eog, gv = tiny
    g = mx.CompiledGrammar(gv, BOUNDED)

    def run_lp(eng, **kw):
        r = eng.submit(PROMPTS[0], MAXT, seed=7, logprobs=3, grammar=g, **kw)
        n, done = 0, False
        while not done:
            toks, done = eng.poll(r, n)
            n = len(toks)
        lp = eng.logprobs(r)
        return eng.wait(r)[0], lp

    for kw in (dict(temperature=0.0), dict(temperature=0.8, top_k=40)):
        monkeypatch.delenv("MX_NO_DEV_TOPK", raising=False)
        dev = mx.Engine(MODEL, n_ctx=128, n_seq_max=2)
        toks, (tok_lp, top_lp, top_idx) = run_lp(dev, **kw)
        free = dev.submit(PROMPTS[0], 1, logprobs=3, **kw)
        while not dev.poll(free, 0)[1]:
            pass
        f_top = dev.logprobs(free)
        dev.wait(free)
        assert dev.sampler_stats()["host_steps"] == 0
        dev.close()
        monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
        host = mx.Engine(MODEL, n_ctx=128, n_seq_max=2)
        h_toks, (h_tok_lp, h_top_lp, h_top_idx) = run_lp(host, **kw)
        host.close()
        assert toks == h_toks and tok_lp.shape == (len(toks),)
        print(kw, "chosen-token log-probs, device against host engine: max |d|", np.abs(tok_lp - h_tok_lp).max())
        assert tok_lp.tobytes() == h_tok_lp.tobytes()
        assert top_lp.tobytes() == h_top_lp.tobytes() and top_idx.tobytes() == h_top_idx.tobytes()
        assert np.isfinite(tok_lp).all() and (tok_lp <= 0).all()
        # the first entry is the raw row's: what the same prompt reports without a grammar, banned tokens included
        assert top_idx[0].tolist() == f_top[2][0].tolist() and top_lp[0].tobytes() == f_top[1][0].tobytes()


def test_grammar_request_never_speculates(mx, tiny):
    pieces, eog, gv = tiny
    g = mx.CompiledGrammar(gv, WORDS)
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=2)
    prompt = [1] + [40, 41, 42, 43] * 6
    plain = eng.generate(prompt, 32, grammar=g)
    r = eng.submit(prompt, 32, grammar=g, draft=(4, 2))
    while not eng.poll(r, 10 ** 6)[1]:  # until it is done; its counters live until wait() releases it
        pass
    st = eng.spec_stats(r)
    assert eng.wait(r) == plain
    assert st == {"steps": 0, "drafted": 0, "accepted": 0}
    from llama_p2p_amd.llama import Llama
    from llama_p2p_amd.llama_grammar import LlamaGrammar
    from llama_p2p_amd.speculative import LlamaPromptLookupDecoding

    eng.close()
    lg = LlamaGrammar.from_string(WORDS)
    a = Llama(model_path=MODEL, n_ctx=128, verbose=False, n_seq_max=2)
    b = Llama(model_path=MODEL, n_ctx=128, verbose=False, n_seq_max=2, draft_model=LlamaPromptLookupDecoding())
    ta = a("a b a b a b a b", max_tokens=32, temperature=0.0, grammar=lg)["choices"][0]
    tb = b("a b a b a b a b", max_tokens=32, temperature=0.0, grammar=lg)["choices"][0]
    assert ta == tb and b._engine.spec_stats()["steps"] == 0
    a.close()
    b.close()


def test_dead_end_ends_one_request_only(mx, tiny):
    pieces, eog, gv = tiny
    mute = [b"" if 3 <= t < 259 else p for t, p in enumerate(pieces)]  # no byte tokens: nothing spells '#'
    mv = mx.GrammarVocab(mute, eog)
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    want = eng.generate(PROMPTS[1], 16, ignore_eos=True)
    for text, n_before in (('root ::= "a" "#"\n', 1), ('root ::= "#"\n', 0)):  # in a decode round / in the prefill
        g = mx.CompiledGrammar(mv, text)
        dead = eng.submit(PROMPTS[0], 16, grammar=g)
        plain = eng.submit(PROMPTS[1], 16, ignore_eos=True)
        toks, done = eng.poll(dead, 10 ** 6)
        assert done and len(toks) == n_before
        with pytest.raises(mx.MxError, match="grammar: dead end") as ei:
            eng.wait(dead)
        assert ei.value.code == mx.MX_ERR_STATE and isinstance(ei.value, RuntimeError)
        assert eng.wait(plain) == want
        assert eng.generate(PROMPTS[1], 16, ignore_eos=True) == want
    with pytest.raises(mx.MxError, match="vocabulary has 3 tokens"):
        eng.submit(PROMPTS[0], 4, grammar=mx.CompiledGrammar(mx.GrammarVocab([b"a", b"b", b""], [2]), 'root ::= "a"\n'))
    eng.close()


def test_llama_front(mx):
    from llama_p2p_amd.llama import Llama
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    llm = Llama(model_path=MODEL, n_ctx=128, verbose=False, n_seq_max=2)
    g = LlamaGrammar.from_string(BOUNDED)
    chunks = list(llm("Answer:", max_tokens=MAXT, temperature=0.8, seed=5, grammar=g, stream=True))
    text = "".join(c["choices"][0]["text"] for c in chunks)
    assert LANG.fullmatch(text) and chunks[-1]["choices"][0]["finish_reason"] == "stop"
    whole = llm("Answer:", max_tokens=MAXT, temperature=0.8, seed=5, grammar=g)["choices"][0]["text"]
    assert whole == text
    cut = llm("Answer:", max_tokens=MAXT, temperature=0.8, seed=5, grammar=g, stop=[" "])["choices"][0]
    assert cut["text"] in ("yes", "no") and cut["finish_reason"] == "stop"
    lp = llm("Answer:", max_tokens=MAXT, temperature=0.8, seed=5, grammar=g, logprobs=2)["choices"][0]
    assert lp["text"] == text and len(lp["logprobs"]["tokens"]) > 0
    with pytest.raises(TypeError):
        llm("Answer:", max_tokens=4, grammar=BOUNDED)
    # a dead end raises RuntimeError, streamed or not: a vocabulary without byte tokens cannot spell '#'
    pieces, eog = spm(512)
    llm._gvocab = mx.GrammarVocab([b"" if 3 <= t < 259 else p for t, p in enumerate(pieces)], eog)
    dead = LlamaGrammar.from_string('root ::= "a" "#"\n')
    with pytest.raises(RuntimeError, match="grammar: dead end"):
        llm("Answer:", max_tokens=8, grammar=dead)
    chunks = []
    with pytest.raises(RuntimeError, match="grammar: dead end"):
        for c in llm("Answer:", max_tokens=8, grammar=dead, stream=True):
            chunks.append(c["choices"][0]["text"])
    assert "".join(chunks) == "a"  # what was generated before the dead end was streamed
    assert LANG.fullmatch(llm("Answer:", max_tokens=MAXT, temperature=0.8, seed=5, grammar=g)["choices"][0]["text"])

    class PipelineFront:  # what pipeserve's rank-0 front offers: no supports_grammar
        n_vocab, n_embd = 512, 256

    front = Llama.from_engine(MODEL, PipelineFront(), n_ctx=128, verbose=False)
    with pytest.raises(NotImplementedError):
        front("Answer:", max_tokens=4, grammar=g)
    llm.close()


def test_shared_grammar_and_close_order(mx, tiny):
    pieces, eog, gv = tiny
    g = mx.CompiledGrammar(gv, BOUNDED)
    eng = mx.Engine(MODEL, n_ctx=128, n_seq_max=4)
    alone = [eng.generate(p, MAXT, temperature=0.8, seed=i, grammar=g) for i, p in enumerate(PROMPTS[:2])]
    reqs = [eng.submit(p, MAXT, temperature=0.8, seed=i, grammar=g) for i, p in enumerate(PROMPTS[:2])]
    assert [eng.wait(r) for r in reqs] == alone and alone[0] != alone[1]
    r = eng.submit(PROMPTS[2], MAXT, grammar=g)
    g.close()  # the request keeps the grammar
    toks, fin = eng.wait(r)
    assert fin == mx.FINISH_STOP and LANG.fullmatch(text_of(pieces, eog, toks).decode())
    g2 = mx.CompiledGrammar(gv, WORDS)
    eng.generate(PROMPTS[0], 8, grammar=g2)
    eng.close()
    assert g2.cache_stats()["misses"] > 0  # still alive after the engine
    g2.close()


def test_real_vocabulary_width(mx):
    pieces, eog = spm(128256)
    gv = mx.GrammarVocab(pieces, eog)
    g, ref = mx.CompiledGrammar(gv, BOUNDED), RefGrammar(BOUNDED)
    eng = mx.Engine(BIG, n_ctx=64, n_seq_max=2)
    for kw in (dict(temperature=0.0), dict(temperature=0.8, top_k=40, seed=2), dict(temperature=1.0, top_k=0, seed=3)):
        toks, fin = eng.generate(PROMPTS[0], MAXT, grammar=g, **kw)
        assert fin == mx.FINISH_STOP and LANG.fullmatch(text_of(pieces, eog, toks).decode()), (kw, toks)
        check_allowed(ref, pieces, eog, toks, str(kw))
    assert eng.sampler_stats()["host_steps"] == 0
    eng.close()
