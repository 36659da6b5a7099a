"""GGUF IQ4_XS (type 23) weights x Q8_K activations in plain numpy (test helper, no engine), beside tests/kq_ref.py:

    block_iq4_xs, 136 bytes per 256 weights: f16 d | u16 scales_h (bits 2j..2j+1: high 2 bits of sub-block j's scale)
    | u8 scales_l[4] (nibble j & 1 of byte j >> 1: its low 4 bits) | u8 qs[128] (sub-block j = bytes 16 j .. 16 j + 15,
    value k < 16 the low nibble of byte k, value 16 + k the high nibble);
    w[32 j + k] = f16(d) (ls_j - 32) KV[index], KV = ggml's kvalues_iq4nl;
    super-block integer S = sum_j (ls_j - 32) (KV[index] . q_x over sub-block j), acc += (f16(d) d_x) S: no mins;
    packed tile, 2208 bytes per 16 rows x 256 k: [0, 2048) Q4_K's QS plane holding the indices; byte 2048 + 32 q + 4 c
    + i the int8 ls - 32 of row 4 q + i, sub-block c; 2176 + 2 r the f16 d of row r.
"""
import numpy as np

import kq_ref as R

IQ4_XS, BLOCK_BYTES, TILE_BYTES, SC, DD = 23, 136, 2208, 2048, 2176
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int64)
F32 = np.float32


def blocks(dbits, ls, idx):
    """GGUF blocks uint8 [N][136 SB] from dbits uint16 [N][SB], ls [N][SB][8] in 0..63, idx [N][256 SB] in 0..15."""
    dbits, ls, idx = np.asarray(dbits, np.uint16), np.asarray(ls, np.int64), np.asarray(idx, np.uint8)
    N, SB = dbits.shape
    assert ls.shape == (N, SB, 8) and 0 <= ls.min() and ls.max() <= 63 and idx.shape == (N, 256 * SB) and idx.max() <= 15
    out = np.empty((N, SB, BLOCK_BYTES), np.uint8)
    out[..., 0], out[..., 1] = dbits & 0xFF, dbits >> 8
    sh = ((ls >> 4) << (2 * np.arange(8))).sum(axis=-1)
    out[..., 2], out[..., 3] = sh & 0xFF, sh >> 8
    out[..., 4:8] = (ls[..., 0::2] & 15) | ((ls[..., 1::2] & 15) << 4)
    v = idx.reshape(N, SB, 8, 2, 16)
    out[..., 8:] = (v[..., 0, :] | (v[..., 1, :] << 4)).reshape(N, SB, 128)
    return out.reshape(N, -1)


def fields(b):
    """The inverse of blocks(), read field by field: dict(d uint16 [N][SB], ls int64 [N][SB][8], idx uint8 [N][K])."""
    b = np.asarray(b, np.uint8)
    N = b.shape[0]
    b = b.reshape(N, -1, BLOCK_BYTES)
    sh = b[..., 2].astype(np.int64) | (b[..., 3].astype(np.int64) << 8)
    ls = np.stack([((b[..., 4 + j // 2] >> (4 * (j & 1))) & 15) | (((sh >> (2 * j)) & 3) << 4) for j in range(8)], axis=-1)
    qs = b[..., 8:].reshape(N, -1, 8, 16)
    idx = np.stack([qs & 15, qs >> 4], axis=3).reshape(N, -1)
    return dict(d=b[..., 0].astype(np.uint16) | (b[..., 1].astype(np.uint16) << 8), ls=ls, idx=idx)


def superblock_ints(f, xq):
    """S int64 [M][N][SB] = sum over the super-block of (ls - 32) KV[index] q_x; xq int [M][K] in k order."""
    w = (np.repeat((f["ls"].reshape(f["ls"].shape[0], -1) - 32).astype(np.int32), 32, axis=1) * KV.astype(np.int32)[f["idx"]]).astype(np.float64)
    xq = np.asarray(xq).astype(np.float64)  # |w| <= 4064, |q| <= 127, 256 terms: exact in float64
    M, N, SB = xq.shape[0], w.shape[0], w.shape[1] // 256
    S = np.matmul(xq.reshape(M, SB, 256).transpose(1, 0, 2), w.reshape(N, SB, 256).transpose(1, 2, 0))
    return np.rint(S).transpose(1, 2, 0).astype(np.int64)


def product(f, xq, xd):
    """(sum_s (d d_x) S, sum_s |.|) in float64 [M][N]; xd [M][SB]."""
    a = R.f16_f32(f["d"]).astype(np.float64)[None] * np.asarray(xd, np.float64)[:, None, :] * superblock_ints(f, xq)
    return a.sum(axis=-1), np.abs(a).sum(axis=-1)


def dequant_f32(f):
    """ggml dequantize_row_iq4_xs in f32, one rounding per product: (d (ls - 32)) KV[index], [N][K]."""
    with np.errstate(over="ignore", invalid="ignore"):
        dl = (R.f16_f32(f["d"])[..., None] * (f["ls"] - 32).astype(F32)).astype(F32)
        return (np.repeat(dl.reshape(dl.shape[0], -1), 32, axis=1) * KV[f["idx"]].astype(F32)).astype(F32)


def pack_tiles(b, mode=0, offset=0):
    """The packed matrix, uint8 flat, rows placed as kq_ref.pack_tiles places them (0xFF where nothing is written).
    The QS plane is that of a Q4_K block holding the indices as its values."""
    f = fields(b)
    N, SB = f["d"].shape
    z8 = np.zeros((N, SB, 8), np.uint8)
    q4 = R.pack_tiles(R.Q4_K, R.kq_blocks(R.Q4_K, f["d"], f["idx"], z8, f["d"], z8), mode, offset)
    q4 = q4.reshape(-1, SB, R.TILE_BYTES[R.Q4_K])
    out = np.full((q4.shape[0], SB, TILE_BYTES), 0xFF, np.uint8)
    out[..., :2048] = q4[..., :2048]
    P = np.arange(N) + offset if mode == 0 else 16 * (np.arange(N) >> 3) + (np.arange(N) & 7) + (8 if mode == 2 else 0)
    for n in range(N):
        T, r = out[P[n] >> 4], P[n] & 15
        for c in range(8):
            T[:, SC + 32 * (r >> 2) + 4 * c + (r & 3)] = (f["ls"][n, :, c] - 32).astype(np.int8).view(np.uint8)
        T[:, DD + 2 * r], T[:, DD + 2 * r + 1] = f["d"][n] & 0xFF, f["d"][n] >> 8
    return out.reshape(-1)
