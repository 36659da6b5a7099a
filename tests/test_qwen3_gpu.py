"""Qwen3 on the GPU: the per-head q/k RMS_NORM inside the decode attention's FIN path and in
qkn_finish_kernel, whole models in every row regime of tests/test_qwen2_gpu.py (its helpers, tolerances and
StopOnHipError habit).  "one" and "slots24" reach the FIN path with one and with several slabs, "chunk5" / "chunk16"
the finish kernel behind the GEMVs, "prefill144" the finish kernel behind the GEMM.  The reference is
tests/qwen3_ref.py, checked against transformers in tests/test_qwen3_host.py."""
import functools

import numpy as np
import pytest
from conftest import assert_logits_close, assert_tokens_match

import qwen3_ref as Q
from test_qwen2_gpu import N_CTX, REGIMES, mx, open_engine, run_regime, tmp  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name, ones=False):
    ids, _ = Q.golden(name)
    ref = Q.forward(name, ids, "ggml", t=Q.weights(name, ones=ones)).astype(np.float32)
    ref.setflags(write=False)
    return ids, ref


def check(eng, ids, ref, regimes, what):
    out = {}
    for regime in regimes:
        rows, got = run_regime(eng, ids, regime)
        print(f"{what} {regime}: max |d| {np.abs(got - ref[rows]).max():.4g} of max|ref| {np.abs(ref[rows]).max():.4g}")
        assert_logits_close(got, ref[rows], f"{what} {regime}")
        assert_tokens_match(got, ref[rows], f"{what} {regime}")
        out[regime] = got
    return out


@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_bf16_logits_every_regime(mx, tmp, name):
    ids, ref = reference(name)
    eng = open_engine(mx, Q.write_gguf(str(tmp / f"{name}.gguf"), name))
    try:
        check(eng, ids, ref, REGIMES, name)
    finally:
        eng.close()


def quant_vs_own_bf16(mx, tmp, tag, wtype, **kw):
    """test_qwen2_gpu.quant_vs_own_bf16 on q3-g4-d128 in regimes one and slots24."""
    ids, _ = Q.golden("q3-g4-d128")
    pq = Q.write_gguf(str(tmp / f"{tag}_{wtype}.gguf"), "q3-g4-d128", wtype=wtype, **kw)
    pb = Q.write_gguf(str(tmp / f"{tag}_{wtype}_bf16.gguf"), "q3-g4-d128", dequant_from=pq, **kw)
    res = []
    for path in (pq, pb):
        eng = open_engine(mx, path)
        try:
            res.append([run_regime(eng, ids[:12] if r == "one" else ids, r)[1] for r in ("one", "slots24")])
        finally:
            eng.close()
    assert all(not np.isnan(a).any() for a in res[0])
    return max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(*res))


@pytest.mark.parametrize("wtype", ["q8_0", "q4_k_m"])
def test_quantised_model(mx, tmp, wtype):
    """Q8_0, and Q4_K with attn_v Q6_K, against this engine on the same file rewritten as BF16; the bar of the Qwen2
    quantised test: twice what the llama twin of the shape (no norm weights: code from before them) shows."""
    twin = quant_vs_own_bf16(mx, tmp, "twin", wtype, arch="llama", qk_norm=None)
    q3 = quant_vs_own_bf16(mx, tmp, "q3", wtype)
    print(f"q3-g4-d128 {wtype}: quantised vs its own BF16, worst |d| / max|ref|: llama twin {twin:.4g}, qwen3 {q3:.4g}")
    assert twin > 0
    assert q3 <= 2 * twin, f"{wtype}: qwen3 {q3:.4g} > 2 x llama twin {twin:.4g}"


def test_norm_weights_are_applied(mx, tmp):
    """All-ones and non-trivial norm weights: different logits, each matching its own reference."""
    got = []
    for ones in (True, False):
        ids, ref = reference("q3-tiny", ones)
        eng = open_engine(mx, Q.write_gguf(str(tmp / f"ones{int(ones)}.gguf"), "q3-tiny", ones=ones))
        try:
            got.append(check(eng, ids, ref, ("one", "chunk16"), f"q3-tiny ones={ones}"))
        finally:
            eng.close()
    for r in got[0]:
        assert np.abs(got[0][r] - got[1][r]).max() > 0.1 * np.abs(got[1][r]).max(), r


def test_llama_front_on_a_qwen3_file(mx, tmp):
    from llama_p2p_amd.llama import Llama

    path = Q.write_gguf(str(tmp / "front.gguf"), "q3-g5")
    ids = [int(t) for t in Q.golden("q3-g5")[0][:12]]
    llm = Llama(path, n_ctx=N_CTX, n_seq_max=4, device=0, verbose=False)
    try:
        assert llm.metadata["general.architecture"] == "qwen3"
        text = llm.create_completion(ids, max_tokens=6, temperature=0.0)["choices"][0]["text"]
    finally:
        llm.close()
    eng = open_engine(mx, path)
    try:
        lg = eng.forward_rows([0] * len(ids), list(range(len(ids))), ids)[-1]
        toks = []
        for p in range(len(ids), len(ids) + 6):  # teacher-forced: each greedy token fed back as a one-row step
            if int(lg.argmax()) == eng.info.eos_id:
                break
            toks.append(int(lg.argmax()))
            lg = eng.forward_rows([0], [p], [toks[-1]])[0]
    finally:
        eng.close()
    assert len(toks) >= 3 and text == llm.tokenizer_.detokenize(toks, prev_tokens=ids).decode("utf-8", errors="ignore")


def test_refusals(mx, tmp):
    cases = {"key_length": (dict(key_length=32), "key_length"),
             "norm weights beside a bias": (dict(qkv_bias=0.3), "bias"),
             "qwen3 without norm weights": (dict(qk_norm=None), "required")}
    for what, (kw, msg) in cases.items():
        path = Q.write_gguf(str(tmp / f"bad_{len(what)}.gguf"), "q3-tiny", **kw)
        with pytest.raises(mx.MxError) as ei:
            mx.Engine(path, n_ctx=N_CTX, n_seq_max=2, device=0)
        assert ei.value.code == mx.MX_ERR_MODEL and msg in str(ei.value), f"{what}: {ei.value}"
