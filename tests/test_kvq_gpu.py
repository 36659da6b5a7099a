"""The Q8_0 KV cache in the engine (kv_type 8): the cache a forward leaves, the logits it gives, the
llama-cpp-python front and a context past the split threshold."""
import threading

import numpy as np
import pytest

import kv_layout as L
import kvq_layout as Q
from llama_p2p_amd import gguf, synth
from llama_p2p_amd.gguf import quantize_q8_0

pytestmark = pytest.mark.gpu

N_CTX, N_SLOTS = 192, 32


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def ids_for(shape, n, seed=0):
    return np.random.default_rng(seed).integers(3, shape.n_vocab, n).astype(np.int32)


# the four writer routes: <= 16 rows (GEMV epilogues), 17..64 rows (unfused: slabs, then launch_qkv_finish) and a
# prompt of 144 rows (the GEMM epilogue, blocked prefill attention).  (slots, positions) of each forward.
FORWARDS = {
    "one": ([0], [0]),
    "rows16": (list(range(1, 17)), [0] * 16),
    "slots24": (list(range(1, 25)), [1] * 24),
    "prompt144": ([30] * 144, list(range(144))),
}


@pytest.mark.parametrize("name", ["test-tiny", "test-gqa8"])
def test_layer0_cache_is_the_quantised_f16_cache(mx, name):
    """After the same forwards, layer 0 of the Q8_0 caches equals quantize_q8_0 of layer 0 of the f16 caches, bitwise
    (layer 0's K / V do not depend on attention; never-written positions are zero blocks on both sides)."""
    shape = synth.SHAPES[name]
    D, H = shape.n_embd // shape.n_head, shape.n_head_kv
    S = L.ctx_stride(N_CTX)
    layer = {}
    for kv in (1, 8):
        eng = mx.Engine(f"synthetic:{name}:seed=3", n_ctx=N_CTX, n_seq_max=N_SLOTS, device=0, kv_type=kv)
        try:
            for i, (slots, pos) in enumerate(FORWARDS.values()):
                eng.forward_rows(slots, pos, ids_for(shape, len(pos), i), want_logits=len(pos) <= 64)
            n = N_SLOTS * H * (S * D * 2 if kv == 1 else Q.region_bytes(S, D))
            layer[kv] = [eng.debug_read(b, n) for b in ("kcache", "vcache")]
        finally:
            eng.close()
    for which, untile16, untile8 in ((0, L.untile_k, Q.untile_k), (1, L.untile_v, Q.untile_v)):
        f16 = untile16(layer[1][which].view(np.float16).reshape(N_SLOTS, H, S * D), D)
        want = quantize_q8_0(f16.astype(np.float32))
        got = untile8(layer[8][which].reshape(N_SLOTS, H, -1), D)
        assert np.abs(f16[30, :, :144]).max() > 0 and np.array_equal(got, want), "KV"[which]


def prompt_and_decode(eng, ids):
    """Logits of a 48-token prompt's last row, then of 8 teacher-forced decode steps."""
    out = [eng.forward_rows([0] * 48, list(range(48)), ids[:48])[-1:]]
    for t in range(8):
        out.append(eng.forward_rows([0], [48 + t], ids[48 + t:49 + t]))
    return np.concatenate(out)


def worst_rel(a, b):
    assert np.isfinite(a).all()
    return float(np.abs(a - b).max() / np.abs(b).max())


def twins(mx, tmp_path, name, n_ctx, run):
    """(weights, kvq): worst |d| / max|ref| of run(engine) for the shape's Q8_0-weights GGUF against its own BF16
    rewrite (existing code on both sides), and for that BF16 file with kv_type 8 against kv_type 1."""
    shape = synth.SHAPES[name]
    pq = gguf.write_synthetic_gguf(str(tmp_path / "q8.gguf"), shape, seed=5, wtype="q8_0")
    pb = gguf.write_synthetic_gguf(str(tmp_path / "bf16.gguf"), shape, seed=5, dequant_from=pq)
    res = {}
    for tag, path, kv in (("w8", pq, 1), ("bf16", pb, 1), ("kv8", pb, 8)):
        eng = mx.Engine(path, n_ctx=n_ctx, n_seq_max=2, device=0, kv_type=kv)
        try:
            res[tag] = run(eng)
        finally:
            eng.close()
    return worst_rel(res["w8"], res["bf16"]), worst_rel(res["kv8"], res["bf16"])


@pytest.mark.parametrize("name", ["test-tiny", "test-gqa8"])
def test_logits_against_the_weight_quantisation_yardstick(mx, name, tmp_path):
    """Worst |logits(kv 8) - logits(kv 1)| / max|logits(kv 1)| over a 48-token prompt and 8 decode steps is at most
    twice the same measure of the shape's Q8_0-weights GGUF against its own BF16 rewrite: that model quantises every
    matrix and activation row with the block format the cache applies to K and V alone, and 2 is the margin this
    suite gives such twin comparisons."""
    ids = ids_for(synth.SHAPES[name], 56, 7)
    weights, kvq = twins(mx, tmp_path, name, N_CTX, lambda eng: prompt_and_decode(eng, ids))
    print(f"{name}: worst |d| / max|ref|: Q8_0 weights vs own BF16 {weights:.4g}, Q8_0 KV cache vs f16 cache {kvq:.4g}")
    assert 0 < kvq <= 2 * weights


def test_llama_front(mx):
    """Llama(type_k=8, type_v=8) completes; a prompt alone and among 8 concurrent requests gives the same tokens;
    set_cache is refused."""
    from llama_p2p_amd.llama import Llama
    from llama_p2p_amd.llama_cache import LlamaRAMCache

    llm = Llama("synthetic:test-tiny", type_k=8, type_v=8, flash_attn=True, n_ctx=128, verbose=False)
    assert llm._engine.kv_type == 8
    prompts = [[1] + ids_for(synth.SHAPES["test-tiny"], 5 + 3 * i, i).tolist() for i in range(8)]
    run = lambda p: llm.create_completion(p, max_tokens=12, temperature=0.0)["choices"][0]["text"]  # noqa: E731
    alone = run(prompts[0])
    got = [None] * 8
    ts = [threading.Thread(target=lambda i=i: got.__setitem__(i, run(prompts[i]))) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert got[0] == alone and all(g is not None for g in got)
    with pytest.raises(NotImplementedError):
        llm.set_cache(LlamaRAMCache())


def test_position_past_the_split_threshold(mx, tmp_path):
    """One request at n_ctx above the threshold decodes past it (the split + merge launches on the Q8_0 cache), held
    to the same yardstick as the short test, measured at these positions."""
    T = mx.attention_split_plan(1)["threshold"]
    n = T + 40
    ids = ids_for(synth.SHAPES["test-tiny"], n + 4, 11)

    def run(eng):
        eng.forward_rows([0] * n, list(range(n)), ids[:n], want_logits=False)
        return np.concatenate([eng.forward_rows([0], [n + t], ids[n + t:n + t + 1]) for t in range(4)])

    weights, kvq = twins(mx, tmp_path, "test-tiny", T + 128, run)
    print(f"pos {n}..{n + 3}: worst |d| / max|ref|: Q8_0 weights {weights:.4g}, Q8_0 KV cache {kvq:.4g}")
    assert 0 < kvq <= 2 * weights
