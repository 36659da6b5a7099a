"""The bf16 weight tiling and the references of the matmul kernel tests, in plain numpy (test helper, no engine).

Written from the layout sentence of kernels.h, not from the device code:

    tile (nt, kt) holds rows [16nt, 16nt+16) x cols [32kt, 32kt+32) of W[N][K] ... element (lane, j) of tile =
    W[16nt + (lane&15)][32kt + 8(lane>>4) + j], 1 KiB per tile (64 lanes x 8 elements), tiles nt-major

and, for ffn_gate / ffn_up (one matrix of 2 n_ff rows): each 16-row tile holds 8 gate rows, then the matching
8 up rows -- tile t = gate rows [8t, 8t+8) followed by up rows [8t, 8t+8).

References: exact integer matmul, SwiGLU / RoPE split / RMS-norm / per-16 sums of squares in float64.
"""
import numpy as np

import kv_layout

TILE_N, TILE_K = 16, 32


# ---- bf16 <-> f32 -------------------------------------------------------------------------------------------
def bf16_bits(a, exact=False):
    """f32 values -> bf16 bits (uint16), round to nearest even.  exact: assert nothing was rounded away."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    if exact:
        assert not (u & 0xFFFF).any(), "value not representable in bf16"
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def bf16_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(a):
    """f32 / f64 values rounded to bf16, as f32 (the input passes through f32 first, as on the device)."""
    return bf16_f32(bf16_bits(np.asarray(a, dtype=np.float32)))


def bf16_ulp(v):
    """Spacing of bf16 numbers at |v| (normal range): 2^(floor(log2 |v|) - 7)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


# ---- tiling -------------------------------------------------------------------------------------------------
def pack_tiles(W):
    """W [N][K] -> flat [N*K] in tile order (any dtype)."""
    W = np.asarray(W)
    N, K = W.shape
    assert N % TILE_N == 0 and K % TILE_K == 0
    # row = 16 nt + r, col = 32 kt + 8 g + j, lane = r + 16 g -> [nt][kt][g][r][j]
    t = W.reshape(N // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)
    return np.ascontiguousarray(t).reshape(-1)


def unpack_tiles(flat, N, K):
    flat = np.asarray(flat)
    t = flat.reshape(N // 16, K // 32, 4, 16, 8).transpose(0, 3, 1, 2, 4)  # nt r kt g j
    return np.ascontiguousarray(t).reshape(N, K)


def interleave_gate_up(gate, up):
    """gate, up [F][K] -> [2F][K]: per 16-row tile, 8 gate rows then the matching 8 up rows."""
    gate, up = np.asarray(gate), np.asarray(up)
    F, K = gate.shape
    assert up.shape == (F, K) and F % 8 == 0
    t = np.stack([gate.reshape(F // 8, 8, K), up.reshape(F // 8, 8, K)], axis=1)  # [tile][gate | up][8][K]
    return np.ascontiguousarray(t).reshape(2 * F, K)


def pack_swiglu(W):
    """Logical [N][K] with rows [0, N/2) gate and [N/2, N) up -> flat packed tiles."""
    W = np.asarray(W)
    F = W.shape[0] // 2
    return pack_tiles(interleave_gate_up(W[:F], W[F:]))


# ---- references ---------------------------------------------------------------------------------------------
def int_matmul(W, X):
    """Exact X [M][K] . W [N][K]^T for small-integer operands, int64 [M][N].  Runs in f32 BLAS by row blocks;
    exact because every partial sum is an integer below 2^24 (asserted from the operands' magnitudes)."""
    W, X = np.asarray(W), np.asarray(X)
    K = W.shape[1]
    assert X.shape[1] == K
    bound = int(np.abs(W).max(initial=0)) * int(np.abs(X).max(initial=0)) * K
    assert bound < 2 ** 24, "partial sums could leave f32's exact integers"
    Xt = np.ascontiguousarray(X.T, dtype=np.float32)
    out = np.empty((X.shape[0], W.shape[0]), dtype=np.int64)
    step = max(1, (1 << 25) // K)
    for r in range(0, W.shape[0], step):
        out[:, r:r + step] = np.rint(W[r:r + step].astype(np.float32) @ Xt).T.astype(np.int64)
    return out


def swiglu_ref(g, u):
    """silu(g) * u in float64."""
    g, u = np.asarray(g, dtype=np.float64), np.asarray(u, dtype=np.float64)
    return g / (1.0 + np.exp(-g)) * u


def rope_ref(s, D, pos, rope_cs):
    """RoPE (adjacent pairs) of rows s [M][H*D] at pos [M] with rope_cs [n_ctx][D/2][cos, sin], float64."""
    s = np.asarray(s, dtype=np.float64)
    M, n = s.shape
    cs = np.asarray(rope_cs, dtype=np.float64)[np.asarray(pos)]  # [M][D/2][2]
    p = s.reshape(M, n // D, D // 2, 2)
    c, sn = cs[:, None, :, 0], cs[:, None, :, 1]
    o = np.stack([p[..., 0] * c - p[..., 1] * sn, p[..., 0] * sn + p[..., 1] * c], axis=-1)
    return o.reshape(M, n)


def qkv_ref(s, n_head, n_head_kv, D, pos, rope_cs):
    """The q|k|v product s [M][(n_head + 2 n_head_kv) D] -> (q [M][n_q] and k [M][n_kv] after RoPE, v [M][n_kv])."""
    s = np.asarray(s, dtype=np.float64)
    nq, nkv = n_head * D, n_head_kv * D
    return (rope_ref(s[:, :nq], D, pos, rope_cs), rope_ref(s[:, nq:nq + nkv], D, pos, rope_cs), s[:, nq + nkv:])


def untile_caches(kc, vc, n_slots, n_head_kv, ctx_stride, D):
    """Raw cache bits -> (K, V) [slot][kv head][position][D] through tests/kv_layout.py."""
    K = kv_layout.untile_k(np.asarray(kc).reshape(n_slots, n_head_kv, ctx_stride * D), D)
    V = kv_layout.untile_v(np.asarray(vc).reshape(n_slots, n_head_kv, ctx_stride * D), D)
    return K, V


def rmsnorm_ref(x, w, eps):
    """x / sqrt(mean(x^2) + eps) * w per row, float64."""
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * np.asarray(w, dtype=np.float64)


def ssq16_ref(x):
    """Sums of squares of each 16 consecutive elements of every row, float64 [rows][n/16]."""
    x = np.asarray(x, dtype=np.float64)
    return (x * x).reshape(x.shape[0], -1, 16).sum(axis=-1)
