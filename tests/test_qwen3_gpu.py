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
from test_qwen2_gpu import N_CTX, REGIMES, StopOnHipError, mx, open_engine, run_regime, tmp  # noqa: F401  (fixtures)

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


def quant_vs_own_bf16(mx, tmp, tag, wtype, name="q3-g4-d128", **kw):
    """test_qwen2_gpu.quant_vs_own_bf16 on `name` in every regime -> {regime: worst |d| / max|ref|}."""
    ids = Q.golden(name)[0] if name in Q.SHAPES else Q.seeded_ids(name)
    pq = Q.write_gguf(str(tmp / f"{tag}_{name}_{wtype}.gguf"), name, wtype=wtype, **kw)
    pb = Q.write_gguf(str(tmp / f"{tag}_{name}_{wtype}_bf16.gguf"), name, dequant_from=pq, **kw)
    res = []
    for path in (pq, pb):
        eng = open_engine(mx, path)
        try:
            res.append({r: run_regime(eng, ids[:12] if r == "one" else ids, r)[1] for r in REGIMES})
        finally:
            eng.close()
    assert all(not np.isnan(a).any() for a in res[0].values())
    return {r: float(np.abs(res[0][r] - res[1][r]).max() / np.abs(res[1][r]).max()) for r in REGIMES}


def quantised_within_twice_the_twin(mx, tmp, wtype, name):
    twin = quant_vs_own_bf16(mx, tmp, "twin", wtype, name, arch="llama", qk_norm=None)
    q3 = quant_vs_own_bf16(mx, tmp, "q3", wtype, name)
    for r in REGIMES:
        print(f"{name} {wtype} {r}: quantised vs its own BF16, worst |d| / max|ref|: llama twin {twin[r]:.4g}, qwen3 "
              f"{q3[r]:.4g} (ratio {q3[r] / twin[r] if twin[r] else float('inf'):.3f})")
    t, q = max(twin.values()), max(q3.values())
    assert t > 0
    assert q <= 2 * t, f"{wtype}: qwen3 {q:.4g} > 2 x llama twin {t:.4g}"


@pytest.mark.parametrize("wtype", ["q8_0", "q4_k_m"])
def test_quantised_model(mx, tmp, wtype):
    """Q8_0, and Q4_K with attn_v Q6_K, against this engine on the same file rewritten as BF16, in every regime; the bar
    of the Qwen2 quantised test: twice what the llama twin of the shape (no norm weights: code from before them) shows,
    worst regime against worst regime as before.  "chunk5" / "chunk16" reach qkn_finish_kernel behind the quantised
    GEMVs (shared-slot rows, an EPI_F32 GEMV's sums as one slab), "prefill144" Q8_0's route of more than 64 rows into
    the GEMM's slab space and the K-quant model's dequantised GEMM, whose split finish leaves q|k|v raw."""
    quantised_within_twice_the_twin(mx, tmp, wtype, "q3-g4-d128")


def test_bf16_width_448_every_regime(mx, tmp):
    """q3-g7 (n_embd 448 = 7 heads x 64, one kv head, n_ff 512): no multiple of 128, so no launch_mm_wide and no
    prefill GEMM.  "slots24" runs the FIN path with the norm behind launch_mm's 17..64-row raw q|k|v epilogue,
    "prefill144" the GEMV route with qkn_finish_kernel.  The reference is qwen3_ref.forward(..., "ggml"), validated
    against transformers on the four golden shapes; the ids come from a seeded generator, so no new transformers
    golden is needed."""
    ids = Q.seeded_ids("q3-g7")
    ref = Q.forward("q3-g7", ids, "ggml").astype(np.float32)
    eng = open_engine(mx, Q.write_gguf(str(tmp / "q3-g7.gguf"), "q3-g7"))
    try:
        assert (eng.info.n_head, eng.info.n_head_kv, eng.info.head_dim) == (7, 1, 64)
        check(eng, ids, ref, REGIMES, "q3-g7")
    finally:
        eng.close()


def test_q8_0_without_gemm_slab_space(mx, tmp):
    """A Q8_0 model with q/k norm weights whose shapes the prefill GEMM does not take (q3-g7) has no slab space for the
    raw q|k|v sums of more than 64 rows: its prompts are taken in 64-row chunks (engine.cpp qkn_raw_fits).  Before
    that, a prompt chunk above 64 rows was refused ("no slab space") and Llama.create_completion failed on any
    prompt above 64 tokens.  Every regime ("prefill144": 144 rows in one call) against the llama twin's bar, and a
    100-token prompt through the Llama front against the engine's own 16-row chunks."""
    from llama_p2p_amd.llama import Llama

    quantised_within_twice_the_twin(mx, tmp, "q8_0", "q3-g7")
    path = Q.write_gguf(str(tmp / "front_q3-g7_q8_0.gguf"), "q3-g7", wtype="q8_0")
    ids = [int(t) for t in Q.seeded_ids("q3-g7", 100)]
    llm = Llama(path, n_ctx=128, n_seq_max=2, device=0, verbose=False)
    try:
        text = llm.create_completion(ids, max_tokens=1, temperature=0.0)["choices"][0]["text"]
    finally:
        llm.close()
    try:
        eng = StopOnHipError(mx.Engine(path, n_ctx=128, n_seq_max=2, device=0), mx)
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:
            pytest.exit(f"{path}: {e}", returncode=3)
        raise
    try:
        eos = eng.info.eos_id
        for i in range(0, 100, 16):
            lg = eng.forward_rows([0] * len(ids[i:i + 16]), list(range(i, min(i + 16, 100))), ids[i:i + 16])[-1]
    finally:
        eng.close()
    tok = int(lg.argmax())
    assert text == ("" if tok == eos else llm.tokenizer_.detokenize([tok], prev_tokens=ids).decode("utf-8", errors="ignore"))


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
