"""Qwen3 on the CPU: the NumPy reference in the engine's form (permuted rows and norm weights, per-head
RMS_NORM before adjacent-pair RoPE) against transformers' Qwen3ForCausalLM goldens."""
import functools

import numpy as np
import pytest
from conftest import logit_tol

import qwen3_ref as Q


@functools.lru_cache(maxsize=None)
def _both(name):
    ids, lg = Q.golden(name)
    w = Q.weights(name)
    return lg, Q.forward(name, ids, "exact", t=w), Q.forward(name, ids, "ggml", t=w)


@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_exact_reference_reproduces_hf(name):
    """Within 1e-5 of the logit scale of HF's forward on the file-order rows: test_qwen2_host.py's bound."""
    lg, ex, _ = _both(name)
    d = np.abs(ex - lg).max() / np.abs(lg).max()
    print(f"{name}: exact vs HF {d:.3g} of max|logit| {np.abs(lg).max():.3f}")
    assert d <= 1e-5


@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_ggml_reference_within_bf16_tolerance(name):
    lg, _, gg = _both(name)
    r = (np.abs(gg - lg) / logit_tol(lg)).max()
    print(f"{name}: ggml vs HF {r:.3f} of the tolerance")
    assert r <= 1.0
