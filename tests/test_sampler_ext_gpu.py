"""The extended sampler chain through the engine: typical_p, tfs_z, logit_bias and Mirostat v2
requests in the scheduler's multi-step device rounds, against the host sampler (MX_NO_DEV_TOPK), the numpy
restatement of sampler_ext_ref.py teacher-forced over the engine's own logits, and the raw log-probabilities.
"""
import math

import numpy as np
import pytest

import sampler_ext_ref as R
from conftest import logit_tol

pytestmark = pytest.mark.gpu

G = 24
PROMPTS = [[1, 17, 99, 5, 23], [1, 400, 401, 402], [1, 7] * 9]
BIAS = {5: 4.0, 17: -math.inf, 99: -3.0, 400: 2.5, 7: -math.inf, 23: 6.0}


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def log_softmax64(row):
    x = row.astype(np.float64)
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum())


def replay_rows(eng, prompt, toks, slot=0):
    """The logits rows the request's decode steps saw, recomputed one row at a time in the request's own slot
    (its K/V is still there): row i >= 1 is the forward of toks[i - 1] at its position, the one-row decode path
    the scheduler ran.  Row 0 (the last prompt row, a prefill row in the request) is recomputed last, so that
    its rewritten K/V cannot touch the others."""
    n = len(prompt)
    rows = [None] * len(toks)
    for i in list(range(1, len(toks))) + [0]:
        t = prompt[-1] if i == 0 else toks[i - 1]
        rows[i] = eng.forward_rows([slot], [n - 1 + i], [t])[0]
    return rows


@pytest.mark.parametrize("kw", [dict(temperature=0.9, typical_p=0.5),
                                dict(temperature=0.9, tfs_z=0.9, top_k=20),
                                dict(temperature=0.8, logit_bias=BIAS, repeat_penalty=1.2)])
def test_device_round_equals_host_sampler(mx, monkeypatch, kw):
    """Alone and as three requests of one submit_many: the same tokens per seed from the device rounds and from
    the host sampler (a fresh engine with MX_NO_DEV_TOPK), which share samp_pick and the counter-based draws."""
    def run(eng):
        alone = [eng.generate(p, G, seed=1000 + i, ignore_eos=True, **kw)[0] for i, p in enumerate(PROMPTS)]
        reqs = eng.submit_many(PROMPTS, G, seeds=[1000, 1001, 1002], ignore_eos=True, **kw)
        return alone, [eng.wait(r)[0] for r in reqs]

    dev = mx.Engine("synthetic:test-d128:seed=0", n_ctx=128, n_seq_max=4)
    dev_alone, dev_many = run(dev)
    dev.close()
    monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    host = mx.Engine("synthetic:test-d128:seed=0", n_ctx=128, n_seq_max=4)
    host_alone, host_many = run(host)
    host.close()
    assert all(len(t) == G for t in dev_alone + dev_many)
    assert dev_alone == host_alone
    assert dev_many == host_many
    if "logit_bias" in kw:
        banned = {t for t, b in BIAS.items() if b == -math.inf}
        assert not banned & {t for ts in dev_alone + dev_many for t in ts}


def test_logit_bias_bans_and_forces(mx):
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=2)
    prompt = [1, 17, 99, 5, 23]
    plain, _ = eng.generate(prompt, G, temperature=0.0, ignore_eos=True)
    ban = {t: -math.inf for t in set(plain)}
    got, _ = eng.generate(prompt, G, temperature=0.0, ignore_eos=True, logit_bias=ban)
    assert len(got) == G and not set(got) & set(plain)
    forced = next(t for t in range(3, eng.n_vocab) if t not in plain)
    for temp in (0.0, 1.0):
        got, _ = eng.generate(prompt, G, temperature=temp, seed=3, ignore_eos=True, logit_bias={forced: 100.0})
        assert got == [forced] * G, f"temperature {temp}"
    eng.close()


def test_biased_greedy_vs_numpy_restatement(mx):
    """Teacher-forced as test_penalised_greedy_vs_numpy_restatement: every pick is the maximum of the numpy
    rewrite (bias, then penalties) of the engine's own row, within the bf16 bar."""
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=2)
    rng = np.random.default_rng(11)
    prompt = [1] + [int(t) for t in rng.integers(3, eng.n_vocab, 12)]
    bias = {int(t): float(b) for t, b in zip(rng.choice(eng.n_vocab, 200, replace=False), rng.normal(size=200) * 3)}
    bias.update({int(t): -math.inf for t in rng.choice(eng.n_vocab, 20, replace=False)})
    s = dict(temperature=0.0, repeat_penalty=1.15, repeat_last_n=16, frequency_penalty=0.2, presence_penalty=0.3,
             logit_bias=bias)
    toks, _ = eng.generate(prompt, G, ignore_eos=True, **s)
    assert len(toks) == G
    lg = eng.forward_logits(prompt + toks[:-1], 0, slot=1)[len(prompt) - 1:]
    plain = 0
    for k, t in enumerate(toks):
        p = R.rewrite(lg[k], s, prompt + toks[:k])
        tol = 2 * logit_tol(lg[k]).max()
        assert p.max() - p[t] <= tol, f"step {k}: picked {t}, rewritten max {p.max():.4f} at {int(p.argmax())}"
        assert bias.get(t, 0.0) != -math.inf
        plain += int(t == int(np.argmax(lg[k])))
    assert plain < G, "the biased chain equals plain greedy at every step"
    eng.close()


@pytest.mark.parametrize("temp", [0.0, 1.0])
def test_logprobs_stay_raw_under_bias(mx, temp):
    """logprobs=3 with a +100 bias: every chosen token is the biased one, far outside the raw top 3, and its
    reported log-prob is the raw row's -- the value from before the bias rewrite (bias_kernel's side table)."""
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=1)
    prompt = [1, 17, 99, 5, 23]
    forced = 77
    r = eng.submit(prompt, G, temperature=temp, seed=5, ignore_eos=True, logprobs=3, logit_bias={forced: 100.0},
                   presence_penalty=0.5)
    n, done = 0, False
    while not done:
        toks, done = eng.poll(r, n)
        n = len(toks)
    tok_lp, top_lp, top_idx = eng.logprobs(r)
    toks, _ = eng.wait(r)
    assert toks == [forced] * G and tok_lp.shape == (G,)
    rows = replay_rows(eng, prompt, toks)
    worst = 0.0
    for i, t in enumerate(toks):
        ref = log_softmax64(rows[i])
        d = abs(float(tok_lp[i]) - ref[t])
        worst = max(worst, d)
        print(f"step {i}: reported {tok_lp[i]:.6f} raw {ref[t]:.6f} biased would be ~0")
        assert d <= 1e-4, f"step {i}: reported {tok_lp[i]}, raw log-softmax {ref[t]}"
        assert np.abs(top_lp[i] - np.sort(ref)[::-1][:3]).max() <= 1e-4
    print(f"temperature {temp}: worst |reported - raw| = {worst:.3g}")
    eng.close()


# a flat model keeps nothing at mu = 2 tau for a dozen steps (mu climbs eta tau a step); the bias table sharpens
# the rows of the second case, so that its kept sets change from the first step on
SHARP = {t: 8.0 - 0.5 * j for j, t in enumerate(range(40, 52))}


@pytest.mark.parametrize("model,seed,extra", [("test-d128", 7, {}), ("test-tiny", 4242, dict(logit_bias=SHARP))])
def test_mirostat_carries_mu_across_steps_and_rounds(mx, model, seed, extra):
    """tau 1, eta 0.5, temperature 1, 24 tokens (more than one round of device steps).  The numpy reference is
    teacher-forced along the engine's tokens over the engine's own rows, its mu updated from the engine's token
    each step.  A pick is asserted when its margins exceed what the bf16 bar d = 2 logit_tol(row).max() can move:
    2 d / ln 2 bits of surprise (the logit and the log-sum each move by at most d) and e^(2d) - 1 of mass.  Every
    asserted pick lies in the reference's kept set and is its draw.  From the reference alone: in at least 6 steps
    the kept set differs from the one mu = 2 tau gives, so an engine that forgets mu would be told apart."""
    eng = mx.Engine(f"synthetic:{model}:seed=0", n_ctx=128, n_seq_max=1)
    prompt = [1, 17, 99, 5, 23]
    s = dict(temperature=1.0, mirostat_mode=2, mirostat_tau=1.0, mirostat_eta=0.5, **extra)
    toks, _ = eng.generate(prompt, G, seed=seed, ignore_eos=True, **s)
    assert len(toks) == G
    rows = replay_rows(eng, prompt, toks)
    mu, differs, asserted, tight, decided = 2.0, 0, 0, 0, 0
    for i, t in enumerate(toks):
        x = R.rewrite(rows[i], s, prompt + toks[:i])
        u = R.samp_u01(seed, i)
        res = R.chain(x, s, u, mu)
        start = R.chain(x, s, u, 2.0)
        differs += int(not np.array_equal(res["kept"], start["kept"]))
        d = 2 * float(logit_tol(rows[i]).max())
        bound = {R.BITS_MARGIN: 2 * d / math.log(2), R.MASS_MARGIN: math.exp(2 * d) - 1}
        decided += int(R.decided(res))
        tight += int(R.decided(res) and res["tok"] == t)
        if all(m >= bound[lim] for m, lim in res["margins"]):
            asserted += 1
            assert res["kept"][t] or not res["kept"].any(), f"step {i}: token {t} outside the kept set (mu {mu})"
            assert t == res["tok"], f"step {i}: token {t}, reference {res['tok']} at mu {mu}"
        # the reference follows the engine's token: p' of that token over the reference's kept set
        kept = res["kept"] if res["kept"].any() else (np.arange(len(x)) == int(np.argmax(x)))
        lp = log_softmax64(x)
        pp = math.exp(lp[t]) / np.exp(lp[kept]).sum() if kept[t] else 1.0
        mu = mu - s["mirostat_eta"] * (-math.log2(pp) - s["mirostat_tau"])
    print(f"{asserted} of {G} picks asserted at the bf16 bar, {tight} of {decided} decided at the reference's own margins equal it, "
          f"kept set differs from mu = 2 tau in {differs} steps")
    assert differs >= 6
    # the rows are the decode path's own (replay_rows), so the reference's own margins decide as well
    assert tight == decided, f"{decided - tight} picks decided at the reference's margins differ from it"
    eng.close()


def test_earlier_requests_are_unchanged_after_the_new_settings_ran(mx):
    from llama_p2p_amd.speculative import LlamaPromptLookupDecoding  # noqa: F401  (the draft= keyword's source)

    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=128, n_seq_max=4)
    prompt = [1, 7] * 9
    def old():
        a = eng.generate(prompt, G, temperature=0.8, seed=9, ignore_eos=True)[0]
        b = eng.generate(prompt, G, temperature=0.0, ignore_eos=True, draft=(4, 2))[0]
        return a, b
    before = old()
    eng.generate(prompt, G, temperature=0.9, seed=1, ignore_eos=True, typical_p=0.5, tfs_z=0.9, logit_bias={7: -1.0})
    eng.generate(prompt, G, temperature=1.0, seed=2, ignore_eos=True, mirostat_mode=2, mirostat_tau=1.0)
    assert old() == before
    eng.close()
