"""The Q8_0 KV-cache layout and a float64 attention reference, in plain numpy (test helper, no engine).

Written from DESIGN.md §22: per (slot, kv head) a region of ctx_stride positions, one Q8_0 block per position and
32 consecutive head-dim elements, as an int8 plane of ctx_stride * D bytes followed by the f16 scale plane:

    K int8:   tile (pos/16, d/64), 1 KiB: lane = pos%16 + 16*((d%32)/8) holds 16 bytes, d%8 of block 2j then of 2j+1
    K scales: [pos][D/32] f16
    V int8:   tile (pos/32, d/32), 1 KiB: lane = d%16 + 16*((pos%32)/8) holds 16 bytes, pos%8 of dim d%16 then 16+d%16
    V scales: [pos/8][D/32][8] f16

tile_* take ggml Q8_0 rows (gguf.quantize_q8_0: [..., S, D/32*34] uint8) and return [..., region bytes] uint8;
untile_* invert them.  Every leading axis (slot, kv head) is kept.
"""
import numpy as np

from llama_p2p_amd.gguf import quantize_q8_0

from kv_layout import ctx_stride  # noqa: F401  (re-exported)


def region_bytes(S, D):
    return S * D + S * (D // 32) * 2


def _split(blocks, D):
    """ggml rows [..., S, D/32*34] -> (q uint8 [..., S, D], d uint8 [..., S, D/32, 2])."""
    b = np.asarray(blocks, dtype=np.uint8)
    b = b.reshape(*b.shape[:-1], D // 32, 34)
    return np.ascontiguousarray(b[..., 2:]).reshape(*b.shape[:-2], D), np.ascontiguousarray(b[..., :2])


def _join(q, d):
    *lead, S, D = q.shape
    b = np.empty((*lead, S, D // 32, 34), np.uint8)
    b[..., :2], b[..., 2:] = d, q.reshape(*lead, S, D // 32, 32)
    return b.reshape(*lead, S, D // 32 * 34)


def tile_k(blocks, D):
    q, d = _split(blocks, D)
    *lead, S, _ = q.shape
    n = len(lead)
    t = q.reshape(*lead, S // 16, 16, D // 64, 2, 4, 8)  # pt pl jt blk dg e
    t = t.transpose(*range(n), n, n + 2, n + 4, n + 1, n + 3, n + 5)  # pt jt dg pl blk e
    return np.concatenate([t.reshape(*lead, S * D), d.reshape(*lead, -1)], axis=-1)


def untile_k(flat, D):
    flat = np.asarray(flat, dtype=np.uint8)
    *lead, R = flat.shape
    S = R // (D + D // 16)
    n = len(lead)
    t = flat[..., :S * D].reshape(*lead, S // 16, D // 64, 4, 16, 2, 8)  # pt jt dg pl blk e
    q = t.transpose(*range(n), n, n + 3, n + 1, n + 4, n + 2, n + 5).reshape(*lead, S, D)
    return _join(q, flat[..., S * D:].reshape(*lead, S, D // 32, 2))


def tile_v(blocks, D):
    q, d = _split(blocks, D)
    *lead, S, _ = q.shape
    n = len(lead)
    t = q.reshape(*lead, S // 32, 4, 8, D // 32, 2, 16)  # pt pg e b half dl
    t = t.transpose(*range(n), n, n + 3, n + 1, n + 5, n + 4, n + 2)  # pt b pg dl half e
    s = d.reshape(*lead, S // 8, 8, D // 32, 2).transpose(*range(n), n, n + 2, n + 1, n + 3)  # p8 b e byte
    return np.concatenate([t.reshape(*lead, S * D), s.reshape(*lead, -1)], axis=-1)


def untile_v(flat, D):
    flat = np.asarray(flat, dtype=np.uint8)
    *lead, R = flat.shape
    S = R // (D + D // 16)
    n = len(lead)
    t = flat[..., :S * D].reshape(*lead, S // 32, D // 32, 4, 16, 2, 8)  # pt b pg dl half e
    q = t.transpose(*range(n), n, n + 2, n + 5, n + 1, n + 4, n + 3).reshape(*lead, S, D)
    s = flat[..., S * D:].reshape(*lead, S // 8, D // 32, 8, 2).transpose(*range(n), n, n + 2, n + 1, n + 3)
    return _join(q, s.reshape(*lead, S, D // 32, 2))


def dequant(blocks, D):
    """ggml rows -> (integers [..., S, D/32, 32] float64, scales [..., S, D/32] float64)."""
    q, d = _split(blocks, D)
    qi = q.view(np.int8).astype(np.float64).reshape(*q.shape[:-1], D // 32, 32)
    return qi, d.view(np.float16)[..., 0].astype(np.float64)


def ref_attention(q, Kb, Vb, pos, scale, n_ctx=None):
    """float64 attention of query heads q [G][D] (f32) at `pos` over keys 0..min(pos, n_ctx-1) of the Q8_0 rows Kb,
    Vb [>= n_ctx][D/32*34]: q is quantised to Q8_0 by the same rule, scores = sum over blocks of d_q d_k (exact
    integer dot) * scale, a plain softmax, out = P . (d_v q_v).  Returns (out, A, spread, sub): A = sum_j p_j
    |v_j|, spread = max - min score per head, sub = per output element the error budget of the terms whose p_j d_v
    falls below f16's smallest normal in the kernels' unnormalised form (2^-25 |q_v| / sum e each)."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    D = q.shape[-1]
    n_ctx = Kb.shape[0] if n_ctx is None else n_ctx
    n = min(int(pos), n_ctx - 1) + 1
    qi, qd = dequant(quantize_q8_0(q), D)  # [G][B][32], [G][B]
    ki, kd = dequant(Kb[:n], D)
    vi, vd = dequant(Vb[:n], D)
    s = np.einsum("gbe,nbe,gb,nb->gn", qi, ki, qd, kd) * float(scale)
    spread = s.max(axis=1) - s.min(axis=1)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    v = (vi * vd[..., None]).reshape(n, D)
    # The kernels form the A operand from the unnormalised e_j = exp(s_j - max) <= 1 and divide by L = sum e at the
    # end.  A term whose f16(e_j d_v) is subnormal carries an absolute error of up to 2^-25 |q_v| / L, not a relative one.
    e = p / p.max(axis=1, keepdims=True)
    tiny = (e[:, :, None] * vd[None] < 2.0 ** -14).astype(np.float64)  # [G][n][B]
    sub = 2.0 ** -25 * np.einsum("gnb,nbe->gbe", tiny, np.abs(vi)).reshape(len(q), D) / e.sum(axis=1)[:, None]
    return p @ v, p @ np.abs(v), spread, sub
