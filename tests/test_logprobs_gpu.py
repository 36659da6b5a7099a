"""Per-token log-probabilities through the engine: the parity hook (mx_forward_logprobs), the request path
(mx_submit_lp / mx_request_logprobs: greedy multi-step rounds, penalties on the device chain and the host
sampler, prompt log-probs, co-batching) and Llama.create_completion(logprobs=k).

Tight checks use float64 numpy over the engine's own f32 logits, 1e-4 absolute (derivation in
test_logprobs_kernel_gpu.py), ids exact against np.lexsort((ids, -vals)).  Checks against teacher-forced
logits of another forward (or the CPU oracle) use the project's bf16 bar, 2 * logit_tol(ref).max()
(test_request_gpu.py): the two forwards run different kernels (1 row vs many), so their logits agree
only to that bar.  A step misalignment in the history moves a chosen token's value by ~0.9, the bar is
~0.04, so an off-by-one fails.
"""
import numpy as np
import pytest

from conftest import logit_tol

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def log_softmax64(lg):
    x = np.asarray(lg, np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def topk_ids(row, k):
    return np.lexsort((np.arange(len(row)), -np.asarray(row, np.float64)))[:k]


def std_prompt(V):
    return [1] + [int(t) for t in np.random.default_rng(11).integers(3, V, 12)]


# ------------------------------------------------------------------ test 2: the hook on its own logits
@pytest.mark.parametrize("model,oracle_shape", [("synthetic:test-tiny:seed=0", "test-tiny"),
                                                ("synthetic:test-tiny-ffn:seed=0", "test-tiny-ffn"),
                                                ("synthetic:test-8b-v128k:seed=0", None),
                                                ("synthetic:test-tiny:seed=0:q8_0", None)])
def test_hook_vs_own_logits(mx, oracle_mod, model, oracle_shape):
    from llama_p2p_amd import synth

    eng = mx.Engine(model, n_ctx=128, n_seq_max=2)
    V, k = eng.n_vocab, 5
    rng = np.random.default_rng(3)
    ids = np.concatenate([[1], rng.integers(3, V, 63)]).astype(np.int32)
    targets = rng.integers(0, V, 64).astype(np.int32)
    targets[0], targets[1] = 0, V - 1
    ref_lg = None
    if oracle_shape:
        octx = oracle_mod.OracleModel(synth.SHAPES[oracle_shape], seed=0).context(128)
        ref_lg = octx.eval(ids, 0, all_logits=True)
    for n in (1, 17, 64):
        slots, pos = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
        tgt, top, idx, lg = eng.forward_logprobs(slots, pos, ids[:n], targets[:n], k, want_logits=True)
        assert lg.shape == (n, V) and top.shape == idx.shape == (n, k)
        ref = log_softmax64(lg)
        for i in range(n):
            assert abs(tgt[i] - ref[i, targets[i]]) <= TOL, f"{model} n={n} row {i}: {tgt[i]} vs {ref[i, targets[i]]}"
            want = topk_ids(lg[i], k)
            assert idx[i].tolist() == want.tolist(), f"{model} n={n} row {i}: top ids"
            assert np.abs(top[i] - ref[i, want]).max() <= TOL
        # the rows the statistics were computed from are the rows forward_rows returns
        again = eng.forward_rows(slots, pos, ids[:n])
        assert again.tobytes() == lg.tobytes(), f"{model} n={n}: logits_out differs from forward_rows"
        if ref_lg is not None:
            oref = log_softmax64(ref_lg[:n])
            tol = 2 * logit_tol(ref_lg[:n]).max()
            d = np.abs(tgt - oref[np.arange(n), targets[:n]])
            assert d.max() <= tol, f"{model} n={n}: target log-probs vs oracle, max |d| {d.max():.4g} > {tol:.4g}"
    eng.close()


# ------------------------------------------------------------------ tests 3 / 4: the request path
def teacher_forced(eng, prompt, toks):
    """Raw logits rows that produced toks[0..]: prompt + toks[:-1] through the parity hook in slot 1."""
    return eng.forward_logits(prompt + toks[:-1], 0, slot=1)[len(prompt) - 1:]


def run_lp(eng, prompt, G, k, **kw):
    """Submit with logprobs=k; checks after every poll that each returned token has its entry."""
    r = eng.submit(prompt, G, ignore_eos=True, logprobs=k, **kw)
    n, done = 0, False
    while not done:
        toks, done = eng.poll(r, n)
        n = len(toks)
        assert len(eng.logprobs(r)[0]) >= n, "a polled token has no log-prob entry yet"
    lp = eng.logprobs(r)
    toks, fin = eng.wait(r)
    with pytest.raises(Exception):
        eng.logprobs(r)  # released by wait
    return toks, lp


def test_request_greedy_multistep(mx):
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=2)
    prompt, G, k = std_prompt(eng.n_vocab), 24, 5
    plain, _ = eng.generate(prompt, G, temperature=0.0, ignore_eos=True)
    toks, (tok_lp, top_lp, top_idx) = run_lp(eng, prompt, G, k, temperature=0.0)
    assert toks == plain and len(toks) == G  # prefill + three 8-step rounds (the last one 7 steps)
    assert tok_lp.shape == (G,) and top_lp.shape == top_idx.shape == (G, k)
    lg = teacher_forced(eng, prompt, toks)
    ref = log_softmax64(lg)
    for i, t in enumerate(toks):
        # argmax and top-k break ties the same way: the greedy token is the first top entry, bit for bit
        assert top_idx[i, 0] == t and tok_lp[i] == top_lp[i, 0], f"step {i}"
        tol = 2 * logit_tol(lg[i]).max()
        assert abs(tok_lp[i] - ref[i, t]) <= tol, f"step {i}: {tok_lp[i]} vs teacher-forced {ref[i, t]} (tol {tol})"
        assert np.abs(top_lp[i] - ref[i, top_idx[i]]).max() <= tol, f"step {i}: top log-probs"
        fifth = np.sort(ref[i])[-k]
        assert (ref[i, top_idx[i]] >= fifth - tol).all(), f"step {i}: a returned id is not among the top {k}"
        assert len(set(top_idx[i].tolist())) == k
    # a request without log-probabilities has none to read
    r = eng.submit(prompt, 4, temperature=0.0, ignore_eos=True)
    with pytest.raises(mx.MxError):
        eng.logprobs(r)
    eng.wait(r)
    for bad in (-1, 65):
        with pytest.raises(mx.MxError):
            eng.submit(prompt, 4, logprobs=bad)
    eng.close()


@pytest.mark.parametrize("host_sampler", [False, True])
@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=0.8, seed=7)])
def test_penalised_picks_report_raw_logprobs(mx, monkeypatch, host_sampler, kw):
    """presence_penalty = -1 boosts every token of the window by 1.0, so picks fall inside it and the
    penalised logit of such a pick differs from the raw one by 1.0 -- 25x the tolerance.  The reported
    log-prob must be that of the raw logits row, on the device chain (penalty_kernel's side table) and on
    the host sampler (MX_NO_DEV_TOPK).  Every run asserts that a pick was in its window (the unpenalised
    greedy chain already repeats a token nine times in a row), so the raw / penalised difference is live."""
    if host_sampler:
        monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=2)
    prompt, G, k = std_prompt(eng.n_vocab), 24, 5
    pen = dict(presence_penalty=-1.0, repeat_last_n=64, **kw)
    toks, (tok_lp, top_lp, top_idx) = run_lp(eng, prompt, G, k, **pen)
    assert len(toks) == G and tok_lp.shape == (G,)
    assert toks == eng.generate(prompt, G, ignore_eos=True, **pen)[0]  # same tokens without logprobs
    lg = teacher_forced(eng, prompt, toks)
    ref = log_softmax64(lg)
    in_window = 0
    for i, t in enumerate(toks):
        tol = 2 * logit_tol(lg[i]).max()
        assert abs(tok_lp[i] - ref[i, t]) <= tol, (f"step {i}: token {t} reported {tok_lp[i]:.4f}, raw teacher-forced "
                                                   f"{ref[i, t]:.4f} (tol {tol:.3f})")
        assert np.abs(top_lp[i] - ref[i, top_idx[i]]).max() <= tol, f"step {i}: top log-probs are not the raw row's"
        in_window += int(t in (prompt + toks[:i])[-64:])
    print(f"host_sampler={host_sampler} {kw}: {in_window} of {G} picks inside their penalty window")
    assert in_window >= 1
    eng.close()


# ------------------------------------------------------------------ test 5: prompt log-probs
def test_prompt_logprobs(mx):
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=256, n_seq_max=2)
    V, G, k = eng.n_vocab, 8, 5
    prompt = [1] + [int(t) for t in np.random.default_rng(5).integers(3, V, 149)]  # 150: > 64 rows, not % 16
    plain, _ = eng.generate(prompt, G, temperature=0.0, ignore_eos=True)

    def run():
        r = eng.submit(prompt, G, temperature=0.0, ignore_eos=True, logprobs=k, prompt_logprobs=True)
        toks, done = [], False
        while not done:
            toks, done = eng.poll(r, len(toks))
        lp = eng.logprobs(r)
        return eng.wait(r)[0], lp

    toks, (tok_lp, top_lp, top_idx) = run()
    assert toks == plain
    assert tok_lp.shape == (149 + G,) and top_lp.shape == top_idx.shape == (149 + G, k)
    lg = eng.forward_logits(prompt + toks[:-1], 0, slot=1)
    ref = log_softmax64(lg)
    seq = prompt + toks
    for e in range(149 + G):  # entry e: log-prob of seq[e + 1] given seq[:e + 1]
        tol = 2 * logit_tol(lg[e]).max()
        assert abs(tok_lp[e] - ref[e, seq[e + 1]]) <= tol, f"entry {e}: {tok_lp[e]} vs {ref[e, seq[e + 1]]}"
        assert np.abs(top_lp[e] - ref[e, top_idx[e]]).max() <= tol, f"entry {e}: top log-probs"
        assert (ref[e, top_idx[e]] >= np.sort(ref[e])[-k] - tol).all()
    # a second request with the same prompt (its prefix is now cached in a slot): the same entries
    toks2, lp2 = run()
    assert toks2 == toks
    for a, b in zip((tok_lp, top_lp, top_idx), lp2):
        assert a.tobytes() == b.tobytes()
    eng.close()


# ------------------------------------------------------------------ test 6: co-batching
def test_logprobs_do_not_depend_on_batch_mates(mx):
    eng = mx.Engine("synthetic:tinyllama-1.1b:seed=0", n_ctx=128, n_seq_max=8)
    rng = np.random.default_rng(21)
    prompt = [1] + [int(t) for t in rng.integers(3, eng.n_vocab, 9)]
    others = [[1] + [int(t) for t in rng.integers(3, eng.n_vocab, 5 + i)] for i in range(7)]
    alone_t, alone_lp = run_lp(eng, prompt, 16, 5, temperature=0.0)
    reqs = eng.submit_many(others, 64, temperature=0.0, ignore_eos=True)
    both_t, both_lp = run_lp(eng, prompt, 16, 5, temperature=0.0)
    left = [len(eng.wait(r)[0]) for r in reqs]
    assert left == [64] * 7
    assert both_t == alone_t and len(alone_t) == 16
    for a, b in zip(alone_lp, both_lp):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    eng.close()


# ------------------------------------------------------------------ test 7: Llama
def test_llama_create_completion_logprobs():
    from llama_p2p_amd.llama import Llama

    llm = Llama(model_path="synthetic:test-tiny:seed=0", n_ctx=128, verbose=False, n_seq_max=2)
    prompt, k = "hello world once", 3
    n_prompt = len(llm.tokenize(prompt.encode()))
    plain = llm(prompt, max_tokens=12, temperature=0.0)
    out = llm(prompt, max_tokens=12, temperature=0.0, logprobs=k)
    ch, lp = out["choices"][0], out["choices"][0]["logprobs"]
    assert ch["text"] == plain["choices"][0]["text"] and out["usage"] == plain["usage"]
    n = out["usage"]["completion_tokens"]
    assert set(lp) == {"tokens", "text_offset", "token_logprobs", "top_logprobs"}
    assert len(lp["tokens"]) == len(lp["text_offset"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == n
    assert "".join(lp["tokens"]) == ch["text"]
    for tok, off, v, top in zip(lp["tokens"], lp["text_offset"], lp["token_logprobs"], lp["top_logprobs"]):
        assert ch["text"][off - len(prompt):].startswith(tok)
        assert v <= 0.0 and top[tok] == v and 1 <= len(top) <= k + 1
        assert max(top.values()) >= v
    # echo: the prompt tokens (BOS skipped) first, the first entry without log-probs
    eo = llm(prompt, max_tokens=12, temperature=0.0, logprobs=k, echo=True)
    ech, elp = eo["choices"][0], eo["choices"][0]["logprobs"]
    assert eo["usage"] == out["usage"] and ech["text"].endswith(ch["text"])
    m = n_prompt - 1 + n
    assert len(elp["tokens"]) == len(elp["text_offset"]) == len(elp["token_logprobs"]) == len(elp["top_logprobs"]) == m
    assert elp["token_logprobs"][0] is None and elp["top_logprobs"][0] is None
    assert all(v is not None and v <= 0.0 for v in elp["token_logprobs"][1:])
    assert "".join(elp["tokens"]) == ech["text"]
    for tok, off, v, top in zip(elp["tokens"], elp["text_offset"], elp["token_logprobs"], elp["top_logprobs"]):
        assert ech["text"][off:].startswith(tok)
        assert top is None or top[tok] == v
    # the completion's entries are the same with and without echo (the prompt pass changes no token)
    assert elp["tokens"][-n:] == lp["tokens"]
    for bad in (65, -1):
        with pytest.raises(ValueError):
            llm(prompt, max_tokens=4, logprobs=bad)
    with pytest.raises(NotImplementedError):
        llm(prompt, max_tokens=4, logprobs=k, stream=True)
    llm.close()
