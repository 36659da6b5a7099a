"""Llama.create_completion(logprobs=k) on the CPU: the llama-cpp-python structure in
choices[0]["logprobs"] ({"tokens", "text_offset", "token_logprobs", "top_logprobs"}), built from a
stand-in engine that returns canned tokens and log-probabilities through Engine's request API (submit
with logprobs= / prompt_logprobs=, poll, logprobs, cancel, wait).  Covered: offsets, echo with the BOS
skipped and the first entry's None, stop-string trimming, the argument checks, and a front without
supports_logprobs (the pipeline server's) which keeps raising NotImplementedError.
"""
import numpy as np
import pytest

from llama_p2p_amd import engine as E
from llama_p2p_amd.llama import Llama

K_ENGINE = 4  # the stand-in records this many top entries whatever is asked (>= k: the dict takes the first k)


class CannedEngine:
    """Generates `stream` in rounds of 8; entry e (prompt position e + 1 when prompt_logprobs, then the
    generated tokens) has tok_lp = -(e + 1) / 8, top ids 300 + e + j and top values -j / 16 - 0.01 (j < K_ENGINE)."""
    supports_logprobs = True
    ROUND = 8

    def __init__(self, stream, n_vocab=512):
        self.stream, self.n_vocab, self.n_embd = list(stream), n_vocab, 64
        self.reqs, self.next, self.cancelled, self.submits = {}, 1, [], []

    def submit(self, ids, max_tokens, logprobs=None, prompt_logprobs=False, **kw):
        r = self.next
        self.next += 1
        self.submits.append({"logprobs": logprobs, "prompt_logprobs": prompt_logprobs})
        self.reqs[r] = {"max": max_tokens, "out": [], "cancel": False, "done": False, "fin": None,
                        "n_prompt": len(ids) - 1 if prompt_logprobs else 0, "lp": logprobs}
        return r

    def _round(self, r):
        q = self.reqs[r]
        if q["done"]:
            return
        if q["cancel"]:
            q["done"], q["fin"] = True, E.FINISH_STOP
            return
        for _ in range(self.ROUND):
            if len(q["out"]) >= min(q["max"], len(self.stream)):
                q["done"], q["fin"] = True, E.FINISH_LENGTH
                return
            q["out"].append(self.stream[len(q["out"])])

    def poll(self, r, n_have=0):
        q = self.reqs[r]
        while len(q["out"]) <= n_have and not q["done"]:
            self._round(r)
        return list(q["out"]), q["done"]

    def cancel(self, r):
        self.cancelled.append(r)
        self.reqs[r]["cancel"] = True

    def logprobs(self, r):
        q = self.reqs[r]
        assert q["lp"] is not None
        n = q["n_prompt"] + len(q["out"])
        tok = -(np.arange(n, dtype=np.float32) + 1) / 8
        top = np.tile(-np.arange(K_ENGINE, dtype=np.float32) / 16, (n, 1)) - 0.01
        idx = (300 + np.arange(n)[:, None] + np.arange(K_ENGINE)[None, :]).astype(np.int32) % self.n_vocab
        return tok, top, idx

    def wait(self, r, cap=None):
        q = self.reqs[r]
        self._round(r)
        while not q["done"]:
            self._round(r)
        del self.reqs[r]
        return list(q["out"]), q["fin"]


MODEL = "synthetic:test-tiny:seed=0"


def make(stream, eng_cls=CannedEngine):
    eng = eng_cls(stream)
    return Llama.from_engine(MODEL, eng, n_ctx=512), eng


def words(text):
    return make([])[0].tokenize(text.encode(), add_bos=False)


def test_completion_logprobs_offsets_and_values():
    stream = words(" alpha beta, gamma delta")
    llm, eng = make(stream)
    prompt = "the model said"
    out = llm(prompt, max_tokens=len(stream), temperature=0.0, logprobs=2)
    assert eng.submits == [{"logprobs": 2, "prompt_logprobs": False}] and not eng.reqs
    ch = out["choices"][0]
    lp = ch["logprobs"]
    n = len(stream)
    assert out["usage"]["completion_tokens"] == n
    assert [len(lp[key]) for key in ("tokens", "text_offset", "token_logprobs", "top_logprobs")] == [n] * 4
    full = llm.detokenize(stream, prev_tokens=llm.tokenize(prompt.encode())).decode()
    assert "".join(lp["tokens"]) == ch["text"] == full and "alpha beta, gamma delta" in full
    off = len(prompt)
    for i, tok in enumerate(lp["tokens"]):
        assert lp["text_offset"][i] == off  # offset in the returned text, shifted by len(prompt)
        assert ch["text"][off - len(prompt):].startswith(tok)
        off += len(tok)
        assert lp["token_logprobs"][i] == pytest.approx(-(i + 1) / 8)
        top = lp["top_logprobs"][i]
        # the first k = 2 of the engine's entries, plus the chosen token's own
        ctx = llm.tokenize(prompt.encode()) + stream[:i]
        want = {llm.detokenize([(300 + i + j) % 512], prev_tokens=ctx).decode("utf-8", errors="ignore"):
                pytest.approx(-j / 16 - 0.01) for j in range(2)}
        want[tok] = pytest.approx(-(i + 1) / 8)
        assert top == want


def test_echo_lists_the_prompt_without_bos_and_a_none_first_entry():
    stream = words(" node peer")
    llm, eng = make(stream)
    prompt = "hello world"
    ptoks = llm.tokenize(prompt.encode())
    assert ptoks[0] == llm.token_bos()
    out = llm(prompt, max_tokens=len(stream), temperature=0.0, logprobs=1, echo=True)
    assert eng.submits == [{"logprobs": 1, "prompt_logprobs": True}]
    ch = out["choices"][0]
    lp = ch["logprobs"]
    n = len(ptoks) - 1 + len(stream)
    assert [len(lp[key]) for key in ("tokens", "text_offset", "token_logprobs", "top_logprobs")] == [n] * 4
    full = prompt + llm.detokenize(stream, prev_tokens=ptoks).decode()
    assert ch["text"] == full and "".join(lp["tokens"]) == full and full.endswith("node peer")
    assert lp["text_offset"][0] == 0 and lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    off = 0
    for i, tok in enumerate(lp["tokens"]):
        assert lp["text_offset"][i] == off
        off += len(tok)
    # listed token i > 0 is prompt position i + 1 -> engine entry i (entry e: position e + 1), then the completion
    for i in range(1, n):
        assert lp["token_logprobs"][i] == pytest.approx(-(i + 1) / 8)
        assert lp["top_logprobs"][i][lp["tokens"][i]] == pytest.approx(-(i + 1) / 8)
    assert out["usage"] == {"prompt_tokens": len(ptoks), "completion_tokens": len(stream),
                            "total_tokens": len(ptoks) + len(stream)}


def test_echo_with_a_token_prompt_that_has_no_bos():
    stream = words(" peer")
    llm, eng = make(stream)
    ptoks = words("hello world")
    out = llm(ptoks, max_tokens=len(stream), temperature=0.0, logprobs=0, echo=True)
    lp = out["choices"][0]["logprobs"]
    n = len(ptoks) + len(stream)  # nothing skipped; position 0 has no entry either way
    assert len(lp["tokens"]) == n and lp["token_logprobs"][0] is None
    assert [v for v in lp["token_logprobs"][1:]] == [pytest.approx(-(e + 1) / 8) for e in range(n - 1)]
    assert all(len(t) == 1 for t in lp["top_logprobs"][1:])  # k = 0: only the chosen token's own entry


def test_stop_string_trims_the_lists_with_the_usage_count():
    stream = words(" alpha beta gamma delta epsilon zeta eta theta iota kappa lambda")
    llm, eng = make(stream)
    out = llm("p", max_tokens=64, stop=["delta"], temperature=0.0, logprobs=2)
    ch = out["choices"][0]
    n = out["usage"]["completion_tokens"]
    assert ch["finish_reason"] == "stop" and ch["text"].endswith("alpha beta gamma ") and 0 < n < len(stream)
    lp = ch["logprobs"]
    assert [len(lp[key]) for key in ("tokens", "text_offset", "token_logprobs", "top_logprobs")] == [n] * 4
    joined = "".join(lp["tokens"])
    assert joined.startswith(ch["text"]) and "delta" in joined  # up to the token completing the stop string
    assert lp["token_logprobs"] == [pytest.approx(-(i + 1) / 8) for i in range(n)]
    assert eng.cancelled and not eng.reqs


def test_eog_token_is_not_listed():
    stream = words(" alpha beta") + [2]

    class Eos(CannedEngine):
        def _round(self, r):
            super()._round(r)
            q = self.reqs[r]
            if q["out"] and q["out"][-1] == 2:  # the engine stops at an end-of-generation token
                q["done"], q["fin"] = True, E.FINISH_STOP

    llm, eng = make(stream, Eos)
    out = llm("p", max_tokens=16, temperature=0.0, logprobs=1)
    n = len(stream) - 1
    assert out["choices"][0]["finish_reason"] == "stop" and out["usage"]["completion_tokens"] == n
    assert len(out["choices"][0]["logprobs"]["tokens"]) == n


def test_argument_checks():
    llm, eng = make([5, 6, 7])
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="64"):
            llm("p", max_tokens=3, logprobs=bad)
    with pytest.raises(NotImplementedError):
        llm("p", max_tokens=3, logprobs=2, stream=True)
    assert not eng.submits
    assert llm("p", max_tokens=3, temperature=0.0)["choices"][0]["logprobs"] is None


def test_front_without_logprob_support_keeps_raising():
    class Plain(CannedEngine):
        supports_logprobs = False

    class Bare:  # the pipeline server's front has no such attribute at all
        n_vocab, n_embd = 512, 64

    for eng in (Plain([5, 6]), Bare()):
        llm = Llama.from_engine(MODEL, eng, n_ctx=512)
        with pytest.raises(NotImplementedError):
            llm("p", max_tokens=2, logprobs=1)


def test_engine_binding_declares_the_feature():
    assert E.Engine.supports_logprobs is True and E.TOPK_MAX == 64
    for name in ("mx_submit_lp", "mx_request_logprobs", "mx_forward_logprobs", "mx_logprob_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
