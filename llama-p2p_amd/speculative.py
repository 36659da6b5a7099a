"""Draft models for speculative decoding, with llama-cpp-python's names and contract
(``llama_cpp.llama_speculative``): ``Llama(..., draft_model=LlamaPromptLookupDecoding(...))``.

The engine runs the prompt lookup itself, on the device, inside the decode step (spec_draft_kernel,
DESIGN.md §10); ``Llama`` only hands it the two numbers.  ``__call__`` here is the host restatement of
that kernel -- the reference its tests compare with, and what llama-cpp-python's callers get when they
call a draft model directly.
"""
from __future__ import annotations

import abc
from typing import Any

import numpy as np


class LlamaDraftModel(abc.ABC):
    @abc.abstractmethod
    def __call__(self, input_ids: np.ndarray, /, **kwargs: Any) -> np.ndarray:
        raise NotImplementedError()


class LlamaPromptLookupDecoding(LlamaDraftModel):
    """Propose the tokens that followed the earliest earlier occurrence of the sequence's last n-gram
    (n = max_ngram_size down to 1), at most num_pred_tokens of them."""

    def __init__(self, max_ngram_size: int = 2, num_pred_tokens: int = 10):
        self.max_ngram_size = max_ngram_size
        self.num_pred_tokens = num_pred_tokens

    @staticmethod
    def find_candidate_pred_tokens(input_ids: np.ndarray, max_ngram_size: int, num_pred_tokens: int) -> np.ndarray:
        ids = np.asarray(input_ids, dtype=np.intc).reshape(-1)
        n = ids.shape[0]
        for g in range(min(max_ngram_size, n - 1), 0, -1):
            key = ids[n - g:]
            # windows [i, i + g) for i < n - g: the key's own window has no continuation
            hit = np.ones(n - g, dtype=bool)
            for k in range(g):
                hit &= ids[k:n - g + k] == key[k]
            idx = np.nonzero(hit)[0]
            if idx.size:
                start = int(idx[0]) + g
                return ids[start:min(start + num_pred_tokens, n)].copy()
        return np.array([], dtype=np.intc)

    def __call__(self, input_ids: np.ndarray, /, **kwargs: Any) -> np.ndarray:
        return self.find_candidate_pred_tokens(input_ids, self.max_ngram_size, self.num_pred_tokens)
