"""What the engine's q|k|v epilogues store is the layout the attention kernels read (Engine.debug_read).

tests/test_attention_kernel_gpu.py proves that the kernels read the documented tile layout; this proves that
the epilogues write it.  One-layer engines (synthetic:test-h4096: D 128, G 4; test-tiny with layer_end=1: D 64,
G 2), n_ctx 128:
  * prefill 100 tokens of one sequence without logits -- one GEMM chunk, rows blocked, attn_prefill_kernel,
    a partial last block; dump q, kcache, vcache, attn_out, pos, slot, de-tile K / V with tests/kv_layout.py:
    every row's attn_out lies inside the random-family bound of test_attention_kernel_gpu.py in its bf16 form
    (2^-10 A + 2^-8 |ref|) of kv_layout.ref_attention on the dumped q / K / V;
  * a 5-row decode step at positions {100, 33, 32, 31, 1} in five slots prefilled to those lengths (the
    <= 16-row path, whose q buffer is final): the same check;
  * the de-tiled K / V of every position beyond a slot's length is all zero (the creation memset): nothing
    writes past pos.
"""
import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

N_CTX, N_SLOTS = 128, 6


def dump(eng, shape, rows):
    H, NKV, D, h = shape.n_head, shape.n_head_kv, shape.n_embd // shape.n_head, shape.n_embd
    S = L.ctx_stride(N_CTX)
    q = eng.debug_read("q", rows * h * 4).view(np.float32).reshape(rows, H, D)
    ao = eng.debug_read("attn_out", rows * h * 2).view(np.uint16).reshape(rows, H, D)
    ao = (ao.astype(np.uint32) << 16).view(np.float32)
    n = N_SLOTS * NKV * S * D
    K = L.untile_k(eng.debug_read("kcache", n * 2).view(np.uint16).reshape(N_SLOTS, NKV, S * D), D).view(np.float16)
    V = L.untile_v(eng.debug_read("vcache", n * 2).view(np.uint16).reshape(N_SLOTS, NKV, S * D), D).view(np.float16)
    pos = eng.debug_read("pos", rows * 4).view(np.int32)
    slot = eng.debug_read("slot", rows * 4).view(np.int32)
    return q, ao, K, V, pos, slot


def check_rows(what, q, ao, K, V, pos, slot, G):
    D = q.shape[2]
    worst = spread_max = 0.0
    for i in range(len(pos)):
        for kvh in range(K.shape[1]):
            hs = slice(kvh * G, (kvh + 1) * G)
            ref, A, spread = L.ref_attention(q[i, hs], K[slot[i], kvh], V[slot[i], kvh], pos[i], 1.0 / np.sqrt(D), N_CTX)
            tol = 2.0 ** -10 * A + 2.0 ** -8 * np.abs(ref)
            ratio = float((np.abs(ao[i, hs] - ref) / tol).max())
            assert ratio <= 1.0, (f"{what}: row {i} (slot {slot[i]}, pos {pos[i]}) kv head {kvh}: "
                                  f"|attn_out - ref| = {ratio:.3g} x tolerance")
            worst, spread_max = max(worst, ratio), max(spread_max, float(spread.max()))
    print(f"{what}: worst |attn_out - ref| / tolerance = {worst:.3f}, largest score spread {spread_max:.2f}")


def check_zero_beyond(what, K, V, lengths):
    for s in range(N_SLOTS):
        n = lengths.get(s, 0)
        for name, c in (("K", K), ("V", V)):
            tail = c[s, :, n:].view(np.uint16)
            assert not tail.any(), (f"{what}: {name} cache of slot {s} holds non-zero bits at positions "
                                    f"{sorted(set((n + np.nonzero(tail.any(axis=(0, 2)))[0]).tolist()))[:8]} >= {n}")


@pytest.mark.parametrize("name,layer_end", [("test-h4096", -1), ("test-tiny", 1)])
def test_epilogues_store_what_the_attention_reads(name, layer_end):
    from llama_p2p_amd import synth
    from llama_p2p_amd.engine import Engine

    shape = synth.SHAPES[name]
    G = shape.n_head // shape.n_head_kv
    rng = np.random.default_rng(7)
    eng = Engine(f"synthetic:{name}:seed=3", n_ctx=N_CTX, n_seq_max=N_SLOTS, layer_end=layer_end, device=0)
    try:
        ids = rng.integers(3, shape.n_vocab, 100).astype(np.int32)
        eng.stage_rows_pick([0] * 100, list(range(100)), ids)  # any row count, also on a one-layer stage of test-tiny
        q, ao, K, V, pos, slot = dump(eng, shape, 100)
        assert pos.tolist() == list(range(100)) and not slot.any()
        check_zero_beyond(f"{name} prefill", K, V, {0: 100})
        check_rows(f"{name} prefill of 100 rows", q, ao, K, V, pos, slot, G)

        lengths = {0: 100, 1: 33, 2: 32, 3: 31, 4: 1}
        for s in (1, 2, 3, 4):
            n = lengths[s]
            eng.stage_rows([s] * n, list(range(n)), rng.integers(3, shape.n_vocab, n).astype(np.int32))
        eng.stage_rows([0, 1, 2, 3, 4], [lengths[s] for s in range(5)], rng.integers(3, shape.n_vocab, 5).astype(np.int32))
        q, ao, K, V, pos, slot = dump(eng, shape, 5)
        assert pos.tolist() == [100, 33, 32, 31, 1] and slot.tolist() == [0, 1, 2, 3, 4]
        check_zero_beyond(f"{name} decode", K, V, {s: n + 1 for s, n in lengths.items()})
        check_rows(f"{name} 5-row decode step", q, ao, K, V, pos, slot, G)
    finally:
        eng.close()
