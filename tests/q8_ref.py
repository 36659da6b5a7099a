"""The Q8_0 / Q4_0 path in plain numpy (test helper, no engine): ggml's activation quantiser, the k permutation
of the activation rows, both packed tile layouts, the tile dequantisation, the RMS_NORM scale and the exact block
matmul.  Every float32 operation is one numpy float32 operation (one rounding each), as in ggml's C.

Written from the comments of kernels.h, not from the device code:

    Q8 tile = 16 rows x 64 k, 1088 bytes: [0,1024) lane l = row l&15 holds 8 bytes of block 0 (k 8(l>>4)..+8) then
    8 bytes of block 1 (k 32+8(l>>4)..+8); [1024,1088) f16 block scales, row group g = rows 4g..4g+3: [block 0 x 4
    rows][block 1 x 4 rows].  Tiles nt-major.
    Q4 tile = 16 rows x 64 k, 576 bytes: [0,512) lane l = row l&15 holds 4 bytes of block 0 then 4 of block 1, its
    8 values k 8(l>>4)..+8 as low nibbles (first 4) and high nibbles (last 4) of those bytes; [512,576) the scales
    as in a Q8 tile.
    activation rows: within each 64-k group, lane group g reads 16 bytes = k 8g..8g+7 (block 0) then k
    32+8g..32+8g+7 (block 1).
"""
import numpy as np

import mm_layout as L

Q8_TILE_BYTES, Q4_TILE_BYTES = 1088, 576
F32 = np.float32


# ---- activation quantiser (ggml quantize_row_q8_0, the AVX2 / NEON rounding) ---------------------------------------
def quantize_act(x):
    """x f32 [..., n] (n % 32 == 0) -> (q int8 [..., n], d f32 [..., n/32] holding f16 values).
    d = amax / 127, id = d ? 1 / d : 0, q = rint(v * id) (half to even), d kept as its f16 value."""
    x = np.asarray(x, dtype=F32)
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(b).max(axis=-1)
    d = amax / F32(127.0)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, F32(1.0) / d, F32(0.0)).astype(F32)
    q = np.rint(b * idv[..., None]).astype(np.int32)
    assert np.abs(q).max(initial=0) <= 127
    with np.errstate(over="ignore"):
        d16 = d.astype(np.float16).astype(F32)
    return q.astype(np.int8).reshape(x.shape), d16


# ---- q8_perm --------------------------------------------------------------------------------------------------------
def q8_perm(k):
    """Byte position of logical k in an activation row: 64-k group kept, then [k bits 3..4][k bit 5][k bits 0..2]."""
    k = np.asarray(k)
    return (k & ~63) | (((k >> 3) & 3) << 4) | (((k >> 5) & 1) << 3) | (k & 7)


def q8_perm_inv(p):
    """Logical k of byte position p."""
    p = np.asarray(p)
    return (p & ~63) | (((p >> 3) & 1) << 5) | (((p >> 4) & 3) << 3) | (p & 7)


def perm_rows(q):
    """Logical rows [..., n] -> device order."""
    q = np.asarray(q)
    out = np.empty_like(q)
    out[..., q8_perm(np.arange(q.shape[-1]))] = q
    return out


def unperm_rows(p):
    """Device rows [..., n] -> logical order."""
    p = np.asarray(p)
    return p[..., q8_perm(np.arange(p.shape[-1]))]


# ---- GGUF blocks ------------------------------------------------------------------------------------------------------
def f16_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16)


def q8_blocks(dbits, q):
    """block_q8_0 {f16 d; int8 qs[32]}: dbits uint16 [N][nb], q int8 [N][32 nb] -> uint8 [N][34 nb]."""
    dbits, q = np.asarray(dbits, dtype=np.uint16), np.asarray(q, dtype=np.int8)
    N, nb = dbits.shape
    out = np.empty((N, nb, 34), dtype=np.uint8)
    out[..., 0], out[..., 1] = dbits & 0xFF, dbits >> 8
    out[..., 2:] = q.reshape(N, nb, 32).view(np.uint8)
    return out.reshape(N, nb * 34)


def q4_blocks(dbits, nib):
    """block_q4_0 {f16 d; uint8 qs[16]}, qs[j] = weight j | weight (j + 16) << 4: nib uint8 [N][32 nb] in 0..15."""
    dbits, nib = np.asarray(dbits, dtype=np.uint16), np.asarray(nib, dtype=np.uint8)
    assert nib.max(initial=0) <= 15
    N, nb = dbits.shape
    v = nib.reshape(N, nb, 2, 16)
    out = np.empty((N, nb, 18), dtype=np.uint8)
    out[..., 0], out[..., 1] = dbits & 0xFF, dbits >> 8
    out[..., 2:] = v[:, :, 0] | (v[:, :, 1] << 4)
    return out.reshape(N, nb * 18)


# ---- packed tiles -----------------------------------------------------------------------------------------------------
def _scales(dbits):
    N, nb = dbits.shape  # [nt][row group][row in group][kt][half] -> [nt][kt][row group][half][row in group]
    return np.asarray(dbits, dtype=np.uint16).reshape(N // 16, 4, 4, nb // 2, 2).transpose(0, 3, 1, 4, 2)


def pack_q8_tiles(dbits, q):
    """dbits uint16 [N][K/32], q int8 [N][K] -> the packed matrix, uint8 flat (N % 16 == 0, K % 64 == 0)."""
    q = np.asarray(q, dtype=np.int8)
    N, K = q.shape
    assert N % 16 == 0 and K % 64 == 0
    # row = 16 nt + r, k = 64 kt + 32 half + 8 g + j, lane = r + 16 g: lane's 16 bytes = [half][j]
    body = q.reshape(N // 16, 16, K // 64, 2, 4, 8).transpose(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 1024)
    sc = np.ascontiguousarray(_scales(dbits)).reshape(N // 16, K // 64, 32).view(np.uint8).reshape(N // 16, K // 64, 64)
    return np.concatenate([body.view(np.uint8), sc], axis=-1).reshape(-1)


def unpack_q8_tiles(flat, N, K):
    t = np.asarray(flat, dtype=np.uint8).reshape(N // 16, K // 64, Q8_TILE_BYTES)
    q = t[..., :1024].view(np.int8).reshape(N // 16, K // 64, 4, 16, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(N, K)
    sc = np.ascontiguousarray(t[..., 1024:]).view(np.uint16).reshape(N // 16, K // 64, 4, 2, 4)
    return np.ascontiguousarray(sc.transpose(0, 2, 4, 1, 3)).reshape(N, K // 32), np.ascontiguousarray(q)


def pack_q4_tiles(dbits, nib):
    """dbits uint16 [N][K/32], nib uint8 [N][K] in 0..15 -> the packed matrix, uint8 flat."""
    nib = np.asarray(nib, dtype=np.uint8)
    N, K = nib.shape
    assert N % 16 == 0 and K % 64 == 0 and nib.max(initial=0) <= 15
    # k = 64 kt + 32 half + 8 g + 4 hl + j: byte j of the lane's 4 = value (hl 0) | value (hl 1) << 4
    v = nib.reshape(N // 16, 16, K // 64, 2, 4, 2, 4).transpose(0, 2, 4, 1, 3, 5, 6)  # nt kt g r half hl j
    body = (v[..., 0, :] | (v[..., 1, :] << 4)).reshape(N // 16, K // 64, 512)
    sc = np.ascontiguousarray(_scales(dbits)).reshape(N // 16, K // 64, 32).view(np.uint8).reshape(N // 16, K // 64, 64)
    return np.concatenate([body, sc], axis=-1).reshape(-1)


def unpack_q4_tiles(flat, N, K):
    t = np.asarray(flat, dtype=np.uint8).reshape(N // 16, K // 64, Q4_TILE_BYTES)
    b = t[..., :512].reshape(N // 16, K // 64, 4, 16, 2, 1, 4)
    v = np.concatenate([b & 15, b >> 4], axis=5)  # nt kt g r half hl j
    nib = v.transpose(0, 3, 1, 4, 2, 5, 6).reshape(N, K)
    sc = np.ascontiguousarray(t[..., 512:]).view(np.uint16).reshape(N // 16, K // 64, 4, 2, 4)
    return np.ascontiguousarray(sc.transpose(0, 2, 4, 1, 3)).reshape(N, K // 32), np.ascontiguousarray(nib)


def gate_up(a):
    """Logical rows [0, N/2) gate, [N/2, N) up -> the packed row order (8 gate rows then their 8 up rows)."""
    a = np.asarray(a)
    F = a.shape[0] // 2
    return L.interleave_gate_up(a[:F], a[F:])


def dequant_q8_bf16_tiles(dbits, q):
    """The packed bf16 tiles of f32(d) * f32(q) rounded to bf16 (tests/mm_layout.py's tile order), uint16 flat."""
    d = np.asarray(dbits, dtype=np.uint16).view(np.float16).astype(F32)
    v = np.repeat(d, 32, axis=1) * np.asarray(q).astype(F32)
    return L.pack_tiles(L.bf16_bits(v))


# ---- RMS_NORM ---------------------------------------------------------------------------------------------------------
def rms_scale(x, eps, nudge=0, partials=False):
    """1.0f / sqrtf((float)(sum / n) + eps) per row, sum = the double sum of the f32 squares.  nudge -1 / +1: the
    f32 neighbour of the scale (a different order of the double sum may move (float)(sum / n) by one ulp).
    partials: sum = the double sum of the per-16-element partials, each the double sum of its f32 squares rounded
    to f32 -- what a quantise-on-load GEMV reads (launch_ssq / the RESID epilogues write them)."""
    x = np.asarray(x, dtype=F32)
    sq = (x * x).astype(np.float64)
    if partials:
        sq = sq.reshape(sq.shape[:-1] + (-1, 16)).sum(axis=-1).astype(F32).astype(np.float64)
    mean = (sq.sum(axis=-1) / x.shape[-1]).astype(F32)
    s = F32(1.0) / np.sqrt(mean + F32(eps), dtype=F32)
    if nudge:
        s = np.nextafter(s, F32(np.inf if nudge > 0 else -np.inf), dtype=F32)
    return s.astype(F32)


def norm_rows(x, w, eps, nudge=0, partials=False):
    """(x * scale) * w in f32, the rows the quantiser then takes."""
    x = np.asarray(x, dtype=F32)
    return (x * rms_scale(x, eps, nudge, partials)[..., None]) * np.asarray(w, dtype=F32)


# ---- the exact block matmul -------------------------------------------------------------------------------------------
def block_isums(wq, xq, chunk=64):
    """isum[m][n][b] = sum over block b of wq[n][k] * xq[m][k], int64 [M][N][K/32] (yielded in chunks of blocks
    as (b0, [M][N][nb_chunk]) to bound memory)."""
    wq, xq = np.asarray(wq), np.asarray(xq)
    N, K = wq.shape
    M = xq.shape[0]
    nb = K // 32
    wf = wq.reshape(N, nb, 32).transpose(1, 2, 0).astype(np.float64)  # [b][32][N]
    xf = xq.reshape(M, nb, 32).transpose(1, 0, 2).astype(np.float64)  # [b][M][32]
    for b0 in range(0, nb, chunk):
        yield b0, np.rint(np.matmul(xf[b0:b0 + chunk], wf[b0:b0 + chunk])).astype(np.int64).transpose(1, 2, 0)


def scaled_block_sum(wq, dw, xq, dx):
    """(sum_b dw[n][b] dx[m][b] isum[m][n][b], sum_b |dw dx isum|) in float64; dw [N][nb], dx [M][nb] float64."""
    dw, dx = np.asarray(dw, dtype=np.float64), np.asarray(dx, dtype=np.float64)
    tot = np.zeros((xq.shape[0], wq.shape[0]))
    mag = np.zeros_like(tot)
    for b0, isum in block_isums(wq, xq):
        nbc = isum.shape[-1]
        t = isum * (dx[:, None, b0:b0 + nbc] * dw[None, :, b0:b0 + nbc])
        tot += t.sum(axis=-1)
        mag += np.abs(t).sum(axis=-1)
    return tot, mag
