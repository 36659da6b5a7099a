"""kv_quant_kernel and the Q8_0-cache attention kernels through mx_attention_kvq_probe -- no model.

Caches are built in numpy (kvq_layout); every position past a slot's used length holds 0xFF bytes (NaN scales) and the
probe pre-fills outputs and the split workspace with 0xFF, so a key read past ctx or an element never written shows.

Bound of the attention tests, per element: |out - ref| <= 2^-10 A, A = sum_j p_j |v_j|, plus 2^-8 |ref| for bf16
output.  Derivation (the f16 kernels', tests/test_attention_kernel_gpu.py): the reference quantises q, K and V by the
same rule and forms the scores from the same exact integers, so what is left is P.V.  Each term's A operand
f16(p d_v) is rounded once (2^-11 relative; V's integers widen to f16 exactly), which sums to 2^-11 A; the same again
covers the f32 accumulation, the f32 score sums and v_exp_f32.  No second f16 rounding exists in this design.  The
reference also asserts that the terms whose f16(e d_v) would be subnormal are negligible (kvq_layout.ref_attention).
"""
import functools

import numpy as np
import pytest

import kv_layout as L
import kvq_layout as Q
from llama_p2p_amd.gguf import quantize_q8_0

pytestmark = pytest.mark.gpu

CTXS = (1, 31, 32, 33, 64, 65, 257)
N_CTX = 300  # ctx_stride 320: positions 257..319 are never written


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def raw_caches(Kb, Vb, used, D):
    """Q8_0 rows [slots][kvh][S][D/32*34] -> the probe's raw caches, 0xFF past used[slot] positions."""
    k, v = Q.tile_k(Kb, D), Q.tile_v(Vb, D)
    S = Kb.shape[-2]
    for s, n in enumerate(used):
        live = np.zeros((S, D // 32 * 34), np.uint8)
        live[:n] = 1
        k[s][:, Q.tile_k(live, D) == 0] = 0xFF
        v[s][:, Q.tile_v(live, D) == 0] = 0xFF
    return k, v


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n_ctx", [100, 64])
def test_kv_quant_bitwise(mx, D, n_ctx):
    """Mode 0: the named rows' blocks equal gguf.quantize_q8_0 of the f16 rows, every other byte stays 0xFF."""
    S, H = L.ctx_stride(n_ctx), 2
    rng = np.random.default_rng(D + n_ctx)
    K = rng.standard_normal((2, H, S, D)).astype(np.float16)
    V = (3 * rng.standard_normal((2, H, S, D))).astype(np.float16)
    K[:, :, :, :32][:, :, ::2] = 0  # a block of zeros
    V[:, 0, :, 32:64] = -np.abs(V[:, 0, :, 32:64])  # amax reached by a negative value
    V[:, 1, :, 3], K[:, 1, :, 40] = 65504, -65504
    poss = [0, 15, 16, 31, 32, n_ctx - 1, n_ctx]
    pos = np.array(poss + poss[:-1])
    slot = np.array([0] * len(poss) + [1] * (len(poss) - 1))
    kq, vq = mx.attention_kvq_probe(0, 2 * H, H, D, n_ctx, 2, pos, slot, kcache=L.tile_k(K.view(np.uint16)),
                                    vcache=L.tile_v(V.view(np.uint16)))
    for got, X, untile in ((kq, K, Q.untile_k), (vq, V, Q.untile_v)):
        want = np.full((2, H, S, D // 32 * 34), 0xFF, np.uint8)
        for p, s in zip(pos, slot):
            if p < n_ctx:
                want[s, :, p] = quantize_q8_0(X[s, :, p].astype(np.float32))
        assert np.array_equal(untile(got.reshape(2, H, -1), D), want)


@functools.lru_cache(maxsize=None)
def bank(D, G):
    """Random caches of two slots (one kv head) used up to 257 positions, q rows and the float64 references."""
    rng = np.random.default_rng(1000 * D + G)
    S = L.ctx_stride(N_CTX)
    Kb = quantize_q8_0((0.5 * rng.standard_normal((2, 1, S, D))).astype(np.float32))
    Vb = quantize_q8_0(rng.standard_normal((2, 1, S, D)).astype(np.float32))
    kq, vq = raw_caches(Kb, Vb, (257, 257), D)
    rows = [(c - 1, i % 2) for i, c in enumerate(CTXS)]  # (pos, slot)
    q = rng.standard_normal((len(rows), G, D)).astype(np.float32)
    refs = [Q.ref_attention(q[i], Kb[s, 0], Vb[s, 0], p, D ** -0.5) for i, (p, s) in enumerate(rows)]
    for _, A, spread, sub in refs:
        assert spread.max() <= 9 and (sub <= 2.0 ** -13 * A).all()
    return Kb, Vb, kq, vq, rows, q, refs


def check(out, ref, A, out_f32, what):
    tol = 2.0 ** -10 * A + (0 if out_f32 else 2.0 ** -8 * np.abs(ref))
    assert np.isfinite(out).all(), what
    err = np.abs(out - ref)
    ratio = (err[tol > 0] / tol[tol > 0]).max(initial=0)  # tol == 0: a quantised V element of 0 at ctx 1, exact
    print(f"{what}: worst |err| / tol = {ratio:.3f}")
    assert (err <= tol).all(), what


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [1, 16, 17, 64, 128])
@pytest.mark.parametrize("D,G", [(64, 1), (128, 4), (64, 7), (128, 7), (128, 1), (64, 4)])
def test_decode_vs_float64(mx, D, G, M, out_f32):
    """Mode 1 at every chunk, tile and wave-assignment edge of ctx; M cycles the rows (128: the 4-wave form)."""
    _, _, kq, vq, rows, q, refs = bank(D, G)
    idx = [(i + M) % len(rows) for i in range(M)]
    out, guard = mx.attention_kvq_probe(1, G, 1, D, N_CTX, 2, [rows[i][0] for i in idx], [rows[i][1] for i in idx],
                                        kq=kq, vq=vq, q=q[idx], out_f32=out_f32)
    assert (guard == 0xFF).all()
    for r, i in enumerate(idx):
        check(out[r].reshape(G, D), refs[i][0], refs[i][1], out_f32, f"row {r} ctx {rows[i][0] + 1}")


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,G", [(64, 1), (128, 4), (64, 7), (128, 7)])
def test_prefill_vs_float64(mx, D, G, out_f32):
    """Mode 3: blocks starting at 0 and 48, a block padded with copies of its last row, M no multiple of 16."""
    Kb, Vb, kq, vq, _, _, _ = bank(D, G)
    pos = list(range(16)) + list(range(48, 64)) + list(range(16, 27)) + [26] * 5 + list(range(64, 69))
    slot = [0] * 16 + [1] * 16 + [0] * 16 + [1] * 5
    q = np.random.default_rng(D * G).standard_normal((len(pos), G, D)).astype(np.float32)
    out, guard = mx.attention_kvq_probe(3, G, 1, D, N_CTX, 2, pos, slot, kq=kq, vq=vq, q=q, out_f32=out_f32)
    assert (guard == 0xFF).all()
    for r, (p, s) in enumerate(zip(pos, slot)):
        ref, A, spread, sub = Q.ref_attention(q[r], Kb[s, 0], Vb[s, 0], p, D ** -0.5)
        assert spread.max() <= 9 and (sub <= 2.0 ** -13 * A).all()
        check(out[r].reshape(G, D), ref, A, out_f32, f"row {r} pos {p}")


@pytest.mark.parametrize("D,G,out_f32", [(128, 4, True), (64, 7, False), (64, 1, True)])
def test_split_vs_float64(mx, D, G, out_f32):
    """Mode 2 just below, at and above the threshold (T + 1: a last segment of one position) and at a ragged
    longer context; rows M..63 of out stay 0xFF."""
    T = mx.attention_split_plan(1)["threshold"]
    ctxs = [T - 1, T, T + 1, T + 611]
    n_ctx = T + 700
    assert mx.attention_split_plan(T + 611)["nseg"] > 1 and (T + 611) % mx.attention_split_plan(T + 611)["seg_len"]
    rng = np.random.default_rng(D + G)
    S = L.ctx_stride(n_ctx)
    Kb = quantize_q8_0((0.5 * rng.standard_normal((2, 1, S, D))).astype(np.float32))
    Vb = quantize_q8_0(rng.standard_normal((2, 1, S, D)).astype(np.float32))
    kq, vq = raw_caches(Kb, Vb, (T + 611, T + 611), D)
    q = rng.standard_normal((len(ctxs), G, D)).astype(np.float32)
    slot = [i % 2 for i in range(len(ctxs))]
    out, guard = mx.attention_kvq_probe(2, G, 1, D, n_ctx, 2, [c - 1 for c in ctxs], slot, kq=kq, vq=vq, q=q,
                                        out_f32=out_f32)
    assert guard.shape[0] == 64 - len(ctxs) and (guard == 0xFF).all()
    for r, c in enumerate(ctxs):
        ref, A, spread, sub = Q.ref_attention(q[r], Kb[slot[r], 0], Vb[slot[r], 0], c - 1, D ** -0.5)
        assert spread.max() <= 9 and (sub <= 2.0 ** -13 * A).all()
        check(out[r].reshape(G, D), ref, A, out_f32, f"ctx {c}")


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("D,G", [(64, 4), (128, 2)])
def test_placement_codes(mx, mode, D, G):
    """V[p][0:4] = (p // 64, p % 64, slot, kv head) and one dominant key per row (q . k = 400, every other K row is
    zero: the rest of the softmax weighs < 1e-12): the output's first four elements are the key's codes.  The codes
    are exact after Q8_0: element 4 of the block is 127, so d_v = 1 and the integers are the codes themselves, and
    the dominant term's A operand is f16(1 * 1).  The check stays at 1e-6."""
    H, T = 2, mx.attention_split_plan(1)["threshold"]
    n_ctx = T + 200 if mode == 2 else 200
    S = L.ctx_stride(n_ctx)
    K = np.zeros((2, H, S, D), np.float32)
    V = np.zeros((2, H, S, D), np.float32)
    p_, s_, h_ = np.meshgrid(np.arange(S), np.arange(2), np.arange(H), indexing="ij")
    V[s_, h_, p_, 0], V[s_, h_, p_, 1], V[s_, h_, p_, 2], V[s_, h_, p_, 3] = p_ // 64, p_ % 64, s_, h_
    V[..., 4] = 127
    if mode == 3:
        pos, slot = list(range(16, 32)) + list(range(96, 101)), [1] * 16 + [0] * 5
    else:
        pos = [0, 17, 33, 70, 199] + ([T + 150] if mode == 2 else [])
        slot = [i % 2 for i in range(len(pos))]
    rng = np.random.default_rng(mode)
    key = [[int(rng.integers(0, p + 1)) for _ in range(H)] for p in pos]  # the dominant key of (row, kv head)
    q = np.zeros((len(pos), H, G, D), np.float32)
    for r, s in enumerate(slot):
        for h in range(H):
            dim = 5 + (r * H + h) % (D - 5)  # rows of one slot that share a key position still differ in direction
            K[s, h, key[r][h], dim] = 20
            q[r, h, :, dim] = 20
    kq, vq = raw_caches(quantize_q8_0(K), quantize_q8_0(V), (S, S), D)
    out, guard = mx.attention_kvq_probe(mode, H * G, H, D, n_ctx, 2, pos, slot, kq=kq, vq=vq, q=q)
    assert (guard == 0xFF).all()
    out = out.reshape(len(pos), H, G, D)
    for r, s in enumerate(slot):
        for h in range(H):
            want = np.array([key[r][h] // 64, key[r][h] % 64, s, h], np.float64)
            assert np.abs(out[r, h, :, :4] - want).max() <= 1e-6 * max(1, want.max()), (r, h, out[r, h, 0, :5], want)


@pytest.mark.parametrize("D,G", [(128, 4), (64, 1)])
def test_batch_invariance(mx, D, G):
    """Mode 1: a row alone and the same row among 16 give the same bits."""
    _, _, kq, vq, rows, q, _ = bank(D, G)
    idx = [i % len(rows) for i in range(16)]
    many, _ = mx.attention_kvq_probe(1, G, 1, D, N_CTX, 2, [rows[i][0] for i in idx], [rows[i][1] for i in idx],
                                     kq=kq, vq=vq, q=q[idx])
    for r in (0, 6, 15):
        one, _ = mx.attention_kvq_probe(1, G, 1, D, N_CTX, 2, [rows[idx[r]][0]], [rows[idx[r]][1]], kq=kq, vq=vq,
                                        q=q[idx[r]][None])
        assert np.array_equal(one[0].view(np.uint32), many[r].view(np.uint32))
