"""The KV-cache tile layout and a float64 attention reference, in plain numpy (test helper, no engine).

Written from the sentence of DESIGN.md §3, not from the device code: per (slot, kv head) a region of
ctx_stride x D f16 in 1 KiB tiles (512 elements: 64 lanes x 8 elements),

    K: tile (pos/16, d/32) = 16 positions x 32 dims, lane = pos%16 + 16*((d%32)/8), element d%8
    V: tile (pos/32, d/16) = 32 positions x 16 dims, lane = d%16 + 16*((pos%32)/8), element pos%8

tiles position-major (all d tiles of one position tile are adjacent).  The tilers take [..., ctx_stride, D]
arrays of any dtype and return [..., ctx_stride * D]; every leading axis (slot, kv head) is kept.
"""
import numpy as np

KV_POS_ALIGN = 64


def ctx_stride(n_ctx):
    return (n_ctx + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN


def tile_k(K):
    K = np.asarray(K)
    *lead, S, D = K.shape
    assert S % 16 == 0 and D % 32 == 0
    n = len(lead)
    # position = 16*pt + pl; dim = 32*dt + 8*dg + e; lane = pl + 16*dg -> within a tile [dg][pl][e]
    t = K.reshape(*lead, S // 16, 16, D // 32, 4, 8)  # pt pl dt dg e
    t = t.transpose(*range(n), n, n + 2, n + 3, n + 1, n + 4)  # pt dt dg pl e
    return np.ascontiguousarray(t).reshape(*lead, S * D)


def untile_k(flat, D):
    flat = np.asarray(flat)
    *lead, SD = flat.shape
    S = SD // D
    n = len(lead)
    t = flat.reshape(*lead, S // 16, D // 32, 4, 16, 8)  # pt dt dg pl e
    t = t.transpose(*range(n), n, n + 3, n + 1, n + 2, n + 4)  # pt pl dt dg e
    return np.ascontiguousarray(t).reshape(*lead, S, D)


def tile_v(V):
    V = np.asarray(V)
    *lead, S, D = V.shape
    assert S % 32 == 0 and D % 16 == 0
    n = len(lead)
    # position = 32*pt + 8*pg + e; dim = 16*dt + dl; lane = dl + 16*pg -> within a tile [pg][dl][e]
    t = V.reshape(*lead, S // 32, 4, 8, D // 16, 16)  # pt pg e dt dl
    t = t.transpose(*range(n), n, n + 3, n + 1, n + 4, n + 2)  # pt dt pg dl e
    return np.ascontiguousarray(t).reshape(*lead, S * D)


def untile_v(flat, D):
    flat = np.asarray(flat)
    *lead, SD = flat.shape
    S = SD // D
    n = len(lead)
    t = flat.reshape(*lead, S // 32, D // 16, 4, 16, 8)  # pt dt pg dl e
    t = t.transpose(*range(n), n, n + 2, n + 4, n + 1, n + 3)  # pt pg e dt dl
    return np.ascontiguousarray(t).reshape(*lead, S, D)


def ref_attention(q, K, V, pos, scale, n_ctx=None):
    """float64 attention of query head(s) q [D] or [G][D] at `pos` over keys 0..min(pos, n_ctx-1) of K, V
    [>= n_ctx][D] (f16 as given): q is rounded to f16 first, scores q.k*scale, a plain softmax, out = P.V.
    Returns (out, A, spread): A = sum_j p_j |v_j| per output element (the scale of the rounding errors of
    P.V) and spread = max - min score (per head).  Keys past the last attended one are never touched."""
    q = np.asarray(q)
    one = q.ndim == 1
    n_ctx = K.shape[0] if n_ctx is None else n_ctx
    n = min(int(pos), n_ctx - 1) + 1
    q64 = np.atleast_2d(q).astype(np.float16).astype(np.float64)
    k64 = np.asarray(K[:n]).astype(np.float64)
    v64 = np.asarray(V[:n]).astype(np.float64)
    s = (q64 @ k64.T) * float(scale)  # [G][n]
    spread = s.max(axis=1) - s.min(axis=1)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    out, A = p @ v64, p @ np.abs(v64)
    return (out[0], A[0], spread[0]) if one else (out, A, spread)
