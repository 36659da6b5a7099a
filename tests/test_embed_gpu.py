"""Embeddings through the engine (mx_submit_embed / mx_wait_embed, Engine.embed, Llama.embed).

Against the oracle: the residual stream after the last layer (OracleContext.layers over all layers), then the
final RMS_NORM + MUL and the pooling in float64 with the model's output_norm.weight -- every pooling, both
normalize values, prompts of 1, 5, 16, 17 and 70 tokens in one call (one block, a padded block, more than
MAX_ROWS; n_ctx = 72, so the 70-token prompt is padded with copies of its last row).  Tolerance: the bf16
tolerance tests/test_engine_gpu.py applies to logits, per vector |d| <= 1e-2 |ref| + 2e-2 max|ref|; the Q8_0 case
adds tests/test_q8_gpu.py's bound by the oracle's own deviation under 1e-6 input noise.

Bitwise on a bf16 model: an input embedded alone equals its vectors from a call with seven others.  With
completions: greedy tokens do not change while another thread embeds on the same engine, and a completion right
after embed() of the same text reuses the embedding's K/V and still gives a fresh engine's tokens.
"""
import ctypes
import threading

import numpy as np
import pytest

from conftest import logit_tol

pytestmark = pytest.mark.gpu

N_CTX = 72
LENGTHS = [1, 5, 16, 17, 70]
NONE, MEAN, CLS, LAST = 0, 1, 2, 3


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def _prompt(shape, n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[1], rng.integers(3, shape.n_vocab, n - 1)]).astype(np.int32)


def _pool64(x, w, eps, pooling, normalize):
    """float64 reference of the tail on the oracle's f32 hidden states x [T][h]."""
    x = x.astype(np.float64)
    y = x * (1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)) * w.astype(np.float64)
    v = {NONE: y, MEAN: y.mean(axis=0, keepdims=True), CLS: y[:1], LAST: y[-1:]}[pooling]
    if normalize:
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v


def _assert_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    for r in range(len(ref)):
        tol = logit_tol(ref[r])
        err = np.abs(got[r] - ref[r])
        assert (err <= tol).all(), (f"{what} row {r}: {(err > tol).sum()} values out of tolerance, max |d| "
                                    f"{err.max():.4g} vs max|ref| {np.abs(ref[r]).max():.4g}")


@pytest.mark.parametrize("name", ["test-tiny", "test-gqa8", "test-d128", "test-h4096"])
def test_embeddings_vs_oracle(mx, oracle_mod, name):
    from llama_p2p_amd import synth

    shape = synth.SHAPES[name]
    w = synth.synth_norm_f32(0, synth.TID_OUT_NORM, shape.n_embd)
    prompts = [_prompt(shape, n, 40 + n) for n in LENGTHS]
    om = oracle_mod.OracleModel(shape, seed=0)
    hidden = [om.context(N_CTX).layers(None, 0, 0, shape.n_layer, ids=p) for p in prompts]
    eng = mx.Engine(f"synthetic:{name}:seed=0", n_ctx=N_CTX, n_seq_max=8)
    try:
        worst = 0.0
        for pooling in (NONE, MEAN, CLS, LAST):
            for normalize in (False, True):
                got = eng.embed(prompts, pooling=pooling, normalize=normalize)
                assert len(got) == len(prompts)
                for p, g, x in zip(prompts, got, hidden):
                    assert g.dtype == np.float32 and g.shape == ((len(p) if pooling == NONE else 1), shape.n_embd)
                    ref = _pool64(x, w, shape.eps, pooling, normalize)
                    _assert_close(g, ref, f"{name} pooling={pooling} normalize={normalize} T={len(p)}")
                    worst = max(worst, float((np.abs(g - ref) / np.array([logit_tol(r) for r in ref])).max()))
                    if normalize:
                        assert np.abs(np.linalg.norm(g.astype(np.float64), axis=1) - 1).max() < 1e-6
        print({"model": name, "worst_err_over_tol": round(worst, 4)})
    finally:
        eng.close()


def test_q8_embeddings_vs_oracle(mx, oracle_mod):
    from llama_p2p_amd import synth

    name = "test-tiny"
    shape = synth.SHAPES[name]
    w = synth.synth_norm_f32(0, synth.TID_OUT_NORM, shape.n_embd)
    p = _prompt(shape, 70, 11)

    def oracle_rows():
        om = oracle_mod.OracleModel(shape, seed=0)
        om.quantize_q8()
        return _pool64(om.context(N_CTX).layers(None, 0, 0, shape.n_layer, ids=p), w, shape.eps, NONE, False)

    ref = oracle_rows()
    oracle_mod.q8_jitter(1e-6)
    try:
        jit = oracle_rows()
    finally:
        oracle_mod.q8_jitter(0.0)
    eng = mx.Engine(f"synthetic:{name}:seed=0:q8_0", n_ctx=N_CTX, n_seq_max=2)
    try:
        got = eng.embed([p], pooling=NONE)[0]
    finally:
        eng.close()
    _assert_close(got, ref, "test-tiny q8_0 embeddings")
    err, self_dev = np.abs(got - ref).max(), np.abs(jit - ref).max()
    print({"q8_err": float(err), "oracle_self_dev": float(self_dev)})
    assert err <= 2 * self_dev + 1e-4 * np.abs(ref).max(), (err, self_dev)


@pytest.mark.parametrize("pooling", [NONE, MEAN])
def test_batch_invariance_bitwise(mx, pooling):
    from llama_p2p_amd import synth

    shape = synth.SHAPES["test-h4096"]
    prompts = [_prompt(shape, n, 70 + i) for i, n in enumerate([70, 1, 5, 16, 17, 33, 70, 9])]
    eng = mx.Engine("synthetic:test-h4096:seed=0", n_ctx=N_CTX, n_seq_max=8)
    try:
        together = eng.embed(prompts, pooling=pooling, normalize=True)
        for i, p in enumerate(prompts):
            alone = eng.embed([p], pooling=pooling, normalize=True)[0]
            assert np.isfinite(alone).all() and alone.std() > 0
            d = np.flatnonzero(alone.view(np.uint32) != together[i].view(np.uint32))
            assert d.size == 0, f"input {i} ({len(p)} tokens): {d.size} values differ alone vs in the 8-input call"
    finally:
        eng.close()


def test_completions_unchanged_while_embedding(mx):
    from llama_p2p_amd import synth

    name = "test-tiny"
    shape = synth.SHAPES[name]
    prompts = [_prompt(shape, n, 5 + n).tolist() for n in (9, 21, 40)]
    texts = [_prompt(shape, n, 90 + n) for n in (3, 17, 30)]
    T = 24
    fresh = mx.Engine(f"synthetic:{name}:seed=0", n_ctx=128, n_seq_max=8)
    try:
        want = [fresh.wait(r)[0] for r in fresh.submit_many(prompts, T, ignore_eos=True)]
    finally:
        fresh.close()
    eng = mx.Engine(f"synthetic:{name}:seed=0", n_ctx=128, n_seq_max=8)
    try:
        first = eng.embed(texts, pooling=MEAN, normalize=True)
        stop, done, errors = threading.Event(), [], []

        def embedder():
            try:
                while True:
                    out = eng.embed(texts, pooling=MEAN, normalize=True)
                    done.append(all(np.array_equal(a, b) for a, b in zip(out, first)))
                    if stop.is_set():
                        return
            except Exception as ex:  # surfaced below
                errors.append(ex)

        th = threading.Thread(target=embedder)
        th.start()
        try:
            got = [eng.wait(r)[0] for r in eng.submit_many(prompts, T, ignore_eos=True)]
        finally:
            stop.set()
            th.join()
        assert not errors, errors
        assert done and all(done), "embeddings changed while completions ran"
        assert got == want
        assert all(len(g) == T for g in got)
    finally:
        eng.close()


def test_completion_after_embed_reuses_its_kv():
    from llama_p2p_amd.llama import LLAMA_POOLING_TYPE_MEAN, Llama

    model = "synthetic:test-tiny:seed=0"
    text = "the quick brown fox jumps over the lazy dog and runs far away"
    fresh = Llama(model, n_ctx=128, n_seq_max=2, verbose=False)
    try:
        want = fresh(text, max_tokens=12, temperature=0.0)
    finally:
        fresh.close()
    llm = Llama(model, n_ctx=128, n_seq_max=2, verbose=False, embedding=True, pooling_type=LLAMA_POOLING_TYPE_MEAN)
    try:
        n = len(llm.tokenize(text.encode()))
        assert n % 16 not in (0, 1) and n > 16  # the embedding's pass wrote K/V at padded positions past the text
        vec = llm.embed(text, normalize=True)
        assert len(vec) == llm.n_embd() and abs(np.linalg.norm(vec) - 1) < 1e-6
        before = llm._engine.stats()["reused_prompt_tokens"]
        got = llm(text, max_tokens=12, temperature=0.0)
        assert llm._engine.stats()["reused_prompt_tokens"] - before == n - 1  # all but the last prompt token
        assert got["choices"][0]["text"] == want["choices"][0]["text"]
        assert got["usage"] == want["usage"]
        # and an embedding after the completion is what it was before it
        assert llm.embed(text, normalize=True) == vec
    finally:
        llm.close()


def test_refusals(mx):
    from llama_p2p_amd import synth

    shape = synth.SHAPES["test-tiny"]
    L = mx.lib()
    eng = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=N_CTX, n_seq_max=4)
    try:
        for bad in ([], [[]], [_prompt(shape, 5, 1), []]):
            with pytest.raises(mx.MxError) as ei:
                eng.embed(bad)
            assert ei.value.code == mx.MX_ERR_ARG
        with pytest.raises(mx.MxError) as ei:
            eng.embed([_prompt(shape, N_CTX + 1, 2)])
        assert ei.value.code == mx.MX_ERR_CTX
        for pooling in (-1, 4):
            with pytest.raises(mx.MxError) as ei:
                eng.embed([_prompt(shape, 5, 1)], pooling=pooling)
            assert ei.value.code == mx.MX_ERR_ARG
        with pytest.raises(mx.MxError) as ei:
            eng.embed([[1, shape.n_vocab]])
        assert ei.value.code == mx.MX_ERR_ARG
        full = eng.embed([_prompt(shape, N_CTX, 3)], pooling=LAST)[0]  # exactly n_ctx tokens fit
        assert full.shape == (1, shape.n_embd) and np.isfinite(full).all()

        # the wrong wait for each kind of request; too small a buffer keeps the request
        ids = _prompt(shape, 5, 1)
        ptrs = (ctypes.c_void_p * 1)(ids.ctypes.data)
        lens = np.array([5], np.int32)
        req = (ctypes.c_uint64 * 1)()
        assert L.mx_submit_embed(eng._h, 1, ptrs, lens.ctypes.data, NONE, 0, req) == 0
        n, fin = ctypes.c_int32(), ctypes.c_int32()
        toks = np.zeros(8, np.int32)
        assert L.mx_wait(eng._h, req[0], toks.ctypes.data, 8, ctypes.byref(n), ctypes.byref(fin)) == mx.MX_ERR_ARG
        assert L.mx_poll(eng._h, req[0], 0, toks.ctypes.data, 8, ctypes.byref(n), ctypes.byref(fin)) == mx.MX_ERR_ARG
        assert L.mx_request_logprobs(eng._h, req[0], None, None, None, 0, ctypes.byref(n),
                                     ctypes.byref(fin)) == mx.MX_ERR_ARG
        out = np.zeros((5, shape.n_embd), np.float32)
        rows = ctypes.c_int32()
        assert L.mx_wait_embed(eng._h, req[0], out.ctypes.data, out.size - 1, ctypes.byref(rows)) == mx.MX_ERR_ARG
        assert rows.value == 5 and (out == 0).all()
        assert L.mx_wait_embed(eng._h, req[0], out.ctypes.data, out.size, ctypes.byref(rows)) == 0
        assert rows.value == 5 and np.array_equal(out, eng.embed([ids])[0])
        assert L.mx_wait_embed(eng._h, req[0], out.ctypes.data, out.size, ctypes.byref(rows)) == mx.MX_ERR_NOTFOUND

        r = eng.submit(ids, 4, ignore_eos=True)
        assert L.mx_wait_embed(eng._h, r, out.ctypes.data, out.size, ctypes.byref(rows)) == mx.MX_ERR_ARG
        assert len(eng.wait(r)[0]) == 4
    finally:
        eng.close()
    stage = mx.Engine("synthetic:test-tiny:seed=0", n_ctx=N_CTX, n_seq_max=2, layer_end=1)
    try:
        assert not stage.info.has_head
        with pytest.raises(mx.MxError) as ei:
            stage.embed([_prompt(shape, 5, 1)])
        assert ei.value.code == mx.MX_ERR_STATE
    finally:
        stage.close()


def test_gguf_pooling_type_metadata(tmp_path):
    from llama_p2p_amd import gguf, synth
    from llama_p2p_amd.llama import LLAMA_POOLING_TYPE_MEAN, LLAMA_POOLING_TYPE_NONE, Llama

    shape = synth.SHAPES["test-tiny"]
    path = str(tmp_path / "tiny_mean.gguf")
    gguf.write_synthetic_gguf(path, shape, seed=0, pooling_type=1)
    llm = Llama(path, n_ctx=64, n_seq_max=2, verbose=False, embedding=True)
    try:
        assert llm.pooling_type() == LLAMA_POOLING_TYPE_MEAN
        vec = llm.embed("x")
        assert isinstance(vec, list) and len(vec) == shape.n_embd and all(isinstance(v, float) for v in vec)
        assert np.isfinite(vec).all() and np.std(vec) > 0
    finally:
        llm.close()
    llm = Llama(path, n_ctx=64, n_seq_max=2, verbose=False, embedding=True, pooling_type=LLAMA_POOLING_TYPE_NONE)
    try:
        assert llm.pooling_type() == LLAMA_POOLING_TYPE_NONE
        rows = llm.embed("x")
        n = len(llm.tokenize(b"x"))
        assert len(rows) == n and all(len(r) == shape.n_embd for r in rows)
        # the mean of the per-token rows is the pooled vector (f32 sum in position order on the device)
        assert np.allclose(np.mean(rows, axis=0), vec, rtol=1e-5, atol=1e-6)
        d = llm.create_embedding(["x", "y z"])
        assert [e["index"] for e in d["data"]] == [0, 1] and d["usage"]["prompt_tokens"] == n + len(llm.tokenize(b"y z"))
    finally:
        llm.close()
