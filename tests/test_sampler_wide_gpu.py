"""Requests with more than 64 candidates (top_k = 0, top_k = 100) through the engine: sampled on the
device by the wide kernel inside the scheduler's multi-step rounds, token for token what the host sampler (a fresh
engine with MX_NO_DEV_TOPK) draws from the same counter-based streams; mixed rounds, log-probabilities, the Llama
front and the settings that still go to the host.

Both engines run the same forwards, so their logits are the same bits and the two samplers differ only in the
order of their f64 sums (~1e-13 of mass against draw boundaries): the seeds below are plain fixed seeds, none had
to be replaced for meeting an undecided case.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 24
PROMPTS = [[1, 17, 99, 5, 23], [1, 400, 401, 402], [1, 7] * 9]
MODELS = ["synthetic:test-d128:seed=0", "synthetic:test-8b-v128k:seed=0"]  # V 2048 (one slice) and V 128256
SETTINGS = [dict(temperature=0.8, top_k=0, top_p=0.95, min_p=0.05),
            dict(temperature=1.0, top_k=100, top_p=1.0, min_p=0.0),
            dict(temperature=0.8, top_k=0, repeat_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.2,
                 repeat_last_n=32, logit_bias={5: 4.0, 17: -np.inf, 99: -3.0, 400: 2.5, 7: -np.inf, 23: 6.0})]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def run(eng, kw):
    alone = [eng.generate(p, G, seed=1000 + i, ignore_eos=True, **kw)[0] for i, p in enumerate(PROMPTS)]
    reqs = eng.submit_many(PROMPTS, G, seeds=[1000, 1001, 1002], ignore_eos=True, **kw)
    return alone, [eng.wait(r)[0] for r in reqs]


@pytest.mark.parametrize("model", MODELS)
def test_device_rounds_equal_host_sampler(mx, monkeypatch, model):
    dev = mx.Engine(model, n_ctx=128, n_seq_max=4)
    got, stats = [], []
    for kw in SETTINGS:
        before = dev.sampler_stats()
        got.append(run(dev, kw))
        after = dev.sampler_stats()
        stats.append({k: after[k] - before[k] for k in after})
    dev.close()
    monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    host = mx.Engine(model, n_ctx=128, n_seq_max=4)
    want = [run(host, kw) for kw in SETTINGS]
    hs = host.sampler_stats()
    host.close()
    for kw, (alone, many), (h_alone, h_many), st in zip(SETTINGS, got, want, stats):
        assert all(len(t) == G for t in alone + many), kw
        assert alone == h_alone, kw
        assert many == h_many, kw
        print(kw, st)
        assert st["host_steps"] == 0
        assert st["wide_rows"] == 6 * G  # every token of the six requests, the first ones from the prefill
        assert st["device_steps"] == 4 * (G - 1)  # three requests alone, then three in one batch
        assert st["rounds"] < st["device_steps"]
    assert hs["wide_rows"] == 0 and hs["device_steps"] == 0 and hs["host_steps"] == hs["rounds"] > 0


def test_mixed_round(mx):
    """Greedy, top_k = 40, top_k = 0 and Mirostat v2 requests in one round: each gets the tokens it gets alone."""
    eng = mx.Engine(MODELS[0], n_ctx=128, n_seq_max=4)
    prompts = PROMPTS + [[1, 33, 34]]
    per = [dict(temperature=0.0), dict(temperature=0.8, top_k=40), dict(temperature=0.8, top_k=0),
           dict(temperature=1.0, mirostat_mode=2, mirostat_tau=1.0, mirostat_eta=0.5)]
    alone = [eng.generate(p, G, seed=50 + i, ignore_eos=True, **kw)[0] for i, (p, kw) in enumerate(zip(prompts, per))]
    before = eng.sampler_stats()
    reqs = eng.submit_many(prompts, G, seeds=[50, 51, 52, 53], ignore_eos=True, per_request=per)
    many = [eng.wait(r)[0] for r in reqs]
    after = eng.sampler_stats()
    eng.close()
    assert many == alone
    assert after["host_steps"] == before["host_steps"] == 0
    assert after["wide_rows"] - before["wide_rows"] == G
    assert after["rounds"] - before["rounds"] < G - 1


def test_logprobs_with_whole_vocabulary_candidates(mx, monkeypatch):
    """logprobs=3 with top_k = 0: the wide kernel leaves the logits alone, so the entries are the host-sampled
    engine's (the same kernels over the same rows; its chosen token's entry is formed on the host from the copied
    row by the same formula, hence the 1e-5 instead of equality)."""
    def run_lp(eng):
        r = eng.submit(PROMPTS[0], G, temperature=0.8, top_k=0, seed=7, ignore_eos=True, logprobs=3)
        n, done = 0, False
        while not done:
            toks, done = eng.poll(r, n)
            n = len(toks)
        lp = eng.logprobs(r)
        return eng.wait(r)[0], lp

    dev = mx.Engine(MODELS[0], n_ctx=128, n_seq_max=2)
    toks, (tok_lp, top_lp, top_idx) = run_lp(dev)
    assert dev.sampler_stats()["host_steps"] == 0
    dev.close()
    monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    host = mx.Engine(MODELS[0], n_ctx=128, n_seq_max=2)
    h_toks, (h_tok_lp, h_top_lp, h_top_idx) = run_lp(host)
    host.close()
    assert toks == h_toks and tok_lp.shape == (G,)
    assert np.abs(tok_lp - h_tok_lp).max() <= 1e-5
    assert top_lp.tobytes() == h_top_lp.tobytes() and top_idx.tobytes() == h_top_idx.tobytes()


def test_llama_front(monkeypatch):
    from llama_p2p_amd.llama import Llama

    def text():
        llm = Llama(model_path="synthetic:test-tiny:seed=0", n_ctx=128, verbose=False, n_seq_max=2)
        out = llm("The quick brown fox", max_tokens=16, temperature=0.8, top_k=0, seed=7)
        return out["choices"][0]["text"], out["usage"]["completion_tokens"]

    dev = text()
    monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    assert dev == text() and dev[1] > 0


def test_tail_free_over_the_whole_vocabulary_still_completes_on_the_host(mx):
    eng = mx.Engine(MODELS[0], n_ctx=128, n_seq_max=2)
    assert mx.sample_plan(dict(temperature=0.8, top_k=0, tfs_z=0.9), eng.n_vocab) == mx.MX_PICK_HOST
    toks, _ = eng.generate(PROMPTS[0], G, temperature=0.8, top_k=0, tfs_z=0.9, seed=3, ignore_eos=True)
    st = eng.sampler_stats()
    eng.close()
    assert len(toks) == G and st["host_steps"] == G - 1 and st["wide_rows"] == 0
