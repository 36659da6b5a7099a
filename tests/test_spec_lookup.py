"""Prompt-lookup speculative decoding on the CPU: LlamaPromptLookupDecoding.__call__ (the host restatement
of the device's draft kernel, llama-cpp-python's find_candidate_pred_tokens) against hand-written cases, and
Llama(draft_model=...) over a stand-in engine: the two numbers reach Engine.submit(draft=) only when a draft
model is given, any other draft model and num_pred_tokens > 15 are refused.
"""
import types

import numpy as np
import pytest

from llama_p2p_amd import engine as E
from llama_p2p_amd.llama import Llama
from llama_p2p_amd.speculative import LlamaDraftModel, LlamaPromptLookupDecoding


def draft(seq, ng=2, d=10):
    out = LlamaPromptLookupDecoding(max_ngram_size=ng, num_pred_tokens=d)(np.asarray(seq, dtype=np.intc))
    assert isinstance(out, np.ndarray) and out.ndim == 1
    return out.tolist()


def test_no_match():
    assert draft([5, 6, 7, 8, 9]) == []
    assert draft([5]) == [] and draft([]) == []


def test_match_only_at_size_one():
    # the last 2-gram (9, 7) occurs nowhere earlier; the last token 7 does, at index 1
    assert draft([5, 7, 8, 9, 7], ng=2, d=3) == [8, 9, 7]
    assert draft([5, 7, 8, 9, 7], ng=2, d=2) == [8, 9]


def test_larger_ngram_wins_over_an_earlier_smaller_one():
    # size 1 alone would match index 0 (-> 1, 2); the 2-gram (4, 3) matches at index 3 and is tried first
    assert draft([3, 1, 2, 4, 3, 8, 9, 4, 3], ng=2, d=2) == [8, 9]
    assert draft([3, 1, 2, 4, 3, 8, 9, 4, 3], ng=1, d=2) == [1, 2]


def test_earliest_of_several_matches():
    # (1, 2) at 0, 4 and 8 (the key itself): the lowest index wins
    assert draft([1, 2, 30, 31, 1, 2, 40, 41, 1, 2], ng=2, d=2) == [30, 31]


def test_match_at_the_very_end_is_skipped():
    # the only window equal to the key is the key itself (empty continuation) at size 2; size 1 finds index 0
    assert draft([7, 9, 8, 7], ng=2, d=4) == [9, 8, 7]
    # all tokens equal: window 0 matches the 1-gram, window len-1 is the key and never a candidate
    assert draft([4, 4], ng=1, d=5) == [4]
    assert draft([4, 4], ng=2, d=5) == [4]


def test_continuation_shorter_than_d():
    assert draft([1, 2, 3, 1, 2], ng=2, d=10) == [3, 1, 2]
    assert draft([1, 2, 3, 1, 2], ng=2, d=1) == [3]


def test_length_at_most_ngram():
    # len <= NG: the n-gram sizes start at len - 1
    assert draft([6, 6, 6], ng=3, d=4) == [6]      # size 2: (6, 6) at 0 -> [6]
    assert draft([6, 6, 6], ng=8, d=4) == [6]
    assert draft([1, 2], ng=5, d=4) == []
    assert draft([2, 2], ng=5, d=4) == [2]


def test_result_is_a_copy_and_static_form_agrees():
    seq = np.array([1, 2, 3, 1, 2], dtype=np.intc)
    out = LlamaPromptLookupDecoding.find_candidate_pred_tokens(seq, 2, 10)
    out[0] = 99
    assert seq.tolist() == [1, 2, 3, 1, 2]
    assert issubclass(LlamaPromptLookupDecoding, LlamaDraftModel)
    with pytest.raises(TypeError):
        LlamaDraftModel()


class CannedEngine:
    """Engine's request API over a fixed token stream; records the keywords of every submit."""
    supports_draft = True

    def __init__(self, stream, n_vocab=512):
        self.stream, self.n_vocab, self.n_embd, self.submits = list(stream), n_vocab, 64, []
        self.info = types.SimpleNamespace(n_vocab=n_vocab)

    def submit(self, ids, max_tokens, **kw):
        self.submits.append(kw)
        self.max = max_tokens
        return 1

    def poll(self, r, n_have=0):
        return self.stream[:self.max], True

    def cancel(self, r):
        pass

    def wait(self, r, cap=None):
        return self.stream[:self.max], E.FINISH_LENGTH


def llama_over(engine, monkeypatch, **kw):
    monkeypatch.setattr(E, "Engine", lambda *a, **k: engine)
    return Llama("synthetic:test-tiny", **kw)


def test_llama_forwards_draft_only_when_given(monkeypatch):
    eng = CannedEngine([10, 11, 12, 13])
    llm = llama_over(eng, monkeypatch, draft_model=LlamaPromptLookupDecoding())
    out = llm([1, 5, 6], max_tokens=3, temperature=0.0)
    assert out["usage"]["completion_tokens"] == 3
    assert eng.submits[-1]["draft"] == (10, 2)  # (num_pred_tokens, max_ngram_size), llama-cpp-python's defaults
    llm._engine = None

    eng2 = CannedEngine([10, 11, 12, 13])
    llm2 = llama_over(eng2, monkeypatch, draft_model=LlamaPromptLookupDecoding(max_ngram_size=3, num_pred_tokens=15))
    llm2([1, 5, 6], max_tokens=2, temperature=0.0)
    assert eng2.submits[-1]["draft"] == (15, 3)
    llm2._engine = None

    eng3 = CannedEngine([10, 11, 12, 13])
    llm3 = llama_over(eng3, monkeypatch)
    plain = llm3([1, 5, 6], max_tokens=3, temperature=0.0)
    assert "draft" not in eng3.submits[-1]
    assert plain["choices"][0]["text"] == out["choices"][0]["text"]
    llm3._engine = None


def test_llama_refuses_other_draft_models_and_too_many_tokens(monkeypatch):
    class Other(LlamaDraftModel):
        def __call__(self, input_ids, /, **kwargs):
            return np.array([], dtype=np.intc)

    with pytest.raises(NotImplementedError):
        llama_over(CannedEngine([1]), monkeypatch, draft_model=Other())
    with pytest.raises(ValueError):
        llama_over(CannedEngine([1]), monkeypatch, draft_model=LlamaPromptLookupDecoding(num_pred_tokens=16))
    with pytest.raises(ValueError):
        llama_over(CannedEngine([1]), monkeypatch, draft_model=LlamaPromptLookupDecoding(num_pred_tokens=0))
    with pytest.raises(ValueError):
        llama_over(CannedEngine([1]), monkeypatch, draft_model=LlamaPromptLookupDecoding(max_ngram_size=0))


def test_binding_declares_the_new_entries():
    assert E.Engine.supports_draft is True and E.SPEC_MAX_DRAFT == 15
    for name in ("mx_submit_spec", "mx_spec_stats", "mx_draft_probe", "mx_accept_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
