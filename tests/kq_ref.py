"""The K-quant path (GGUF Q4_K 12, Q5_K 13, Q6_K 14 weights x Q8_K activations) in plain numpy (test helper, no
engine): block builders and their inverse, ggml's quantize_row_q8_K, the permuted activation row and its sub-block
sum slots, the packed tile layout, the per-super-block integers S and Mn with the float64 product, and the f32
dequantisation.  Every float32 operation is one numpy float32 operation (one rounding each), as in ggml's C.

Written from the comments of csrc/kquant.hip and from the loop transcriptions in tests/test_kquants.py, not from
the device code:

    blocks (ggml-common.h): block_q4_K {f16 d, f16 dmin, scales[12], qs[128]}, block_q5_K {d, dmin, scales[12],
    qh[32], qs[128]}, block_q6_K {ql[128], qh[64], int8 scales[16], f16 d}; 256 weights each.
    super-block integers: Q4_K / Q5_K  S = sum_j sc_j (q_w . q_x over 32-value sub-block j), Mn = sum_j m_j bsum32_j;
    Q6_K  S = sum_g sc_g (q_w . q_x over 16-value group g), q_w = 6-bit value - 32;
    acc += (f16(d) d_x) S - (f16(dmin) d_x) Mn.
    Q8_K rows: xq int8 [M][K], within super-block s logical k = 256 s + 32 j + 8 g + e sits at 256 s + 64 g + 8 j + e;
    xd f32 [M][K/256] (d = 1 / iscale); xb f32 [M][K/32]: the sum of the 32 q of sub-block j at 8 s + 2 (j & 3) +
    (j >> 2).
    packed tile, per 16 rows x 256 k:
      [0, 2048) QS: lane l (row r = l & 15, k-slice g = l >> 4) owns 8 dwords D[0..7], D[j] holding the low 4 bits of
        value (j, e) -- k = 32 j + 8 g + e -- in byte e & 3, nibble e >> 2; D[0..3] at 16 l, D[4..7] at 1024 + 16 l
      Q5_K [2048, 2560): lane l's 2 dwords at 2048 + 8 l: bit 4 of value (j, e) at bit 8 (e & 3) + (u & 7) of dword
        u >> 3, u = 2 j + (e >> 2)
      Q6_K [2048, 3072): lane l's 4 dwords at 2048 + 16 l: bits 4-5 of value (j, e) at bits 8 (e & 3) + 2 (u & 3) of
        dword u >> 2
      scales, row r = 4 q + i: byte SC + 64 q + 4 c + i is column c of row r.  Q4_K / Q5_K at SC = 2048 / 2560:
        column c < 8 the 6-bit scale of sub-block c, c >= 8 the 6-bit min of sub-block c - 8; SC + 256 + 16 q + 2 i:
        f16 d of row r, SC + 264 + 16 q + 2 i: f16 dmin.  Q6_K at SC = 3072: column c the int8 scale of 16-value
        group c; SC + 256 + 2 r: f16 d of row r.
      Tiles [row tile][super-block]; bytes 2368 / 2880 / 3360.
"""
import numpy as np

import mm_layout as L

Q4_K, Q5_K, Q6_K = 12, 13, 14
TYPES = (Q4_K, Q5_K, Q6_K)
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}
TILE_BYTES = {Q4_K: 2368, Q5_K: 2880, Q6_K: 3360}
TILE_SC = {Q4_K: 2048, Q5_K: 2560, Q6_K: 3072}
VMAX = {Q4_K: 15, Q5_K: 31, Q6_K: 63}
F32 = np.float32


def f16_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16)


def f16_f32(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(F32)


# ---- GGUF blocks ------------------------------------------------------------------------------------------------------
def _scales12(sc, mn):
    """get_scale_min_k4's 12 bytes from 6-bit scales / mins [..., 8]."""
    sc, mn = np.asarray(sc, dtype=np.uint8), np.asarray(mn, dtype=np.uint8)
    assert sc.max(initial=0) <= 63 and mn.max(initial=0) <= 63
    q = np.empty(sc.shape[:-1] + (12,), dtype=np.uint8)
    q[..., 0:4] = sc[..., 0:4] | ((sc[..., 4:8] >> 4) << 6)
    q[..., 4:8] = mn[..., 0:4] | ((mn[..., 4:8] >> 4) << 6)
    q[..., 8:12] = (sc[..., 4:8] & 15) | ((mn[..., 4:8] & 15) << 4)
    return q


def _unscales12(q):
    q = np.asarray(q, dtype=np.uint8)
    sc = np.empty(q.shape[:-1] + (8,), dtype=np.uint8)
    mn = np.empty_like(sc)
    sc[..., 0:4], mn[..., 0:4] = q[..., 0:4] & 63, q[..., 4:8] & 63
    sc[..., 4:8] = (q[..., 8:12] & 15) | ((q[..., 0:4] >> 6) << 4)
    mn[..., 4:8] = (q[..., 8:12] >> 4) | ((q[..., 4:8] >> 6) << 4)
    return sc, mn


def kq_blocks(t, dbits, vals, sc, mbits=None, mn=None):
    """GGUF blocks uint8 [N][SB * block bytes] from dbits uint16 [N][SB], vals [N][256 SB] in 0..VMAX[t], and for
    Q4_K / Q5_K the 6-bit sc / mn uint8 [N][SB][8] with mbits (dmin) uint16 [N][SB]; Q6_K: sc int8 [N][SB][16]."""
    dbits, vals = np.asarray(dbits, dtype=np.uint16), np.asarray(vals, dtype=np.uint8)
    N, SB = dbits.shape
    assert vals.shape == (N, 256 * SB) and vals.max(initial=0) <= VMAX[t]
    out = np.empty((N, SB, BLOCK_BYTES[t]), dtype=np.uint8)
    if t == Q6_K:
        sc = np.asarray(sc, dtype=np.int8)
        assert sc.shape == (N, SB, 16)
        v = vals.reshape(N, SB, 2, 4, 32)  # k = 128 h + 32 i + l
        out[..., 0:128] = np.stack([(v[:, :, :, 0] & 15) | ((v[:, :, :, 2] & 15) << 4),
                                    (v[:, :, :, 1] & 15) | ((v[:, :, :, 3] & 15) << 4)], axis=3).reshape(N, SB, 128)
        hi = (v >> 4) & 3
        out[..., 128:192] = (hi[:, :, :, 0] | (hi[:, :, :, 1] << 2) | (hi[:, :, :, 2] << 4) | (hi[:, :, :, 3] << 6)).reshape(N, SB, 64)
        out[..., 192:208] = sc.view(np.uint8)
        out[..., 208], out[..., 209] = dbits & 0xFF, dbits >> 8
        return out.reshape(N, -1)
    mbits = np.asarray(mbits, dtype=np.uint16)
    assert np.asarray(sc).shape == (N, SB, 8) and np.asarray(mn).shape == (N, SB, 8) and mbits.shape == (N, SB)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = dbits & 0xFF, dbits >> 8, mbits & 0xFF, mbits >> 8
    out[..., 4:16] = _scales12(sc, mn)
    v = vals.reshape(N, SB, 4, 2, 32)  # k = 64 g + 32 hi + l
    qs = ((v[:, :, :, 0] & 15) | ((v[:, :, :, 1] & 15) << 4)).reshape(N, SB, 128)
    if t == Q5_K:
        b4 = (v >> 4) & 1
        qh = np.zeros((N, SB, 32), dtype=np.uint8)
        for g in range(4):
            qh |= (b4[:, :, g, 0] << (2 * g)) | (b4[:, :, g, 1] << (2 * g + 1))
        out[..., 16:48], out[..., 48:176] = qh, qs
    else:
        out[..., 16:144] = qs
    return out.reshape(N, -1)


def kq_fields(t, blocks):
    """The inverse of kq_blocks: dict(d, dmin: uint16 [N][SB]; sc, mn [N][SB][8] uint8 or sc int8 [N][SB][16];
    vals uint8 [N][256 SB])."""
    blocks = np.asarray(blocks, dtype=np.uint8)
    N = blocks.shape[0]
    b = blocks.reshape(N, -1, BLOCK_BYTES[t])
    SB = b.shape[1]
    u16 = lambda o: b[..., o].astype(np.uint16) | (b[..., o + 1].astype(np.uint16) << 8)
    if t == Q6_K:
        ql, qh = b[..., 0:128].reshape(N, SB, 2, 2, 32), b[..., 128:192].reshape(N, SB, 2, 32)
        v = np.empty((N, SB, 2, 4, 32), dtype=np.uint8)
        for i in range(4):
            lo = ql[:, :, :, i & 1]
            v[:, :, :, i] = ((lo & 15) if i < 2 else (lo >> 4)) | (((qh >> (2 * i)) & 3) << 4)
        return dict(d=u16(208), dmin=None, sc=b[..., 192:208].copy().view(np.int8), mn=None, vals=v.reshape(N, -1))
    sc, mn = _unscales12(b[..., 4:16])
    qs = (b[..., 48:176] if t == Q5_K else b[..., 16:144]).reshape(N, SB, 4, 32)
    v = np.stack([qs & 15, qs >> 4], axis=3)  # [N][SB][g][hi][l]
    if t == Q5_K:
        qh = b[..., 16:48]
        for g in range(4):
            v[:, :, g, 0] |= ((qh >> (2 * g)) & 1) << 4
            v[:, :, g, 1] |= ((qh >> (2 * g + 1)) & 1) << 4
    return dict(d=u16(0), dmin=u16(2), sc=sc, mn=mn, vals=v.reshape(N, -1))


def kq_ints(t, f):
    """The integer weight of every k (Q6_K: value - 32), int16 [N][K]."""
    return f["vals"].astype(np.int16) - (32 if t == Q6_K else 0)


# ---- Q8_K activations (ggml quantize_row_q8_K_ref) -----------------------------------------------------------------------
def nearest_int(v):
    """ggml nearest_int of f32 values with |v| <= 2^22: the magic-number addition, i.e. round half to even."""
    val = (np.asarray(v, dtype=F32) + F32(12582912.0)).astype(F32)
    return (val.view(np.int32) & 0x007FFFFF) - 0x00400000


def quantize_q8k(x):
    """x f32 [..., n] (n % 256 == 0) -> (q int8 [..., n] in k order, d f32 [..., n/256], bsums int32 [..., n/16]).
    max = the signed value of the FIRST element with |x| == amax; iscale = -127 / max; q = min(127,
    nearest_int(iscale x)); d = 1 / iscale; an all-zero super-block: d = 0, q = 0."""
    x = np.asarray(x, dtype=F32)
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // 256, 256))
    first = np.abs(b).argmax(axis=-1)  # the first occurrence of the maximum
    mx = np.take_along_axis(b, first[..., None], axis=-1)[..., 0]
    zero = mx == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = np.where(zero, F32(0), F32(-127.0) / mx).astype(F32)
        q = np.minimum(127, nearest_int((iscale[..., None] * b).astype(F32)))
        d = np.where(zero, F32(0), F32(1.0) / iscale).astype(F32)
    q = np.where(zero[..., None], 0, q)
    assert q.min(initial=0) >= -128
    bs = q.reshape(q.shape[:-1] + (16, 16)).sum(axis=-1)
    return q.astype(np.int8).reshape(x.shape), d, bs.reshape(x.shape[:-1] + (-1,)).astype(np.int32)


def xq_perm(k):
    """Byte position of logical k in a Q8_K device row: k = 256 s + 32 j + 8 g + e -> 256 s + 64 g + 8 j + e."""
    k = np.asarray(k)
    return (k & ~255) | (((k >> 3) & 3) << 6) | (((k >> 5) & 7) << 3) | (k & 7)


def perm_rows(q):
    """Logical rows [..., n] -> device order."""
    q = np.asarray(q)
    out = np.empty_like(q)
    out[..., xq_perm(np.arange(q.shape[-1]))] = q
    return out


def unperm_rows(p):
    """Device rows [..., n] -> logical order."""
    p = np.asarray(p)
    return p[..., xq_perm(np.arange(p.shape[-1]))]


def xb_slot(s, j):
    """Slot of sub-block j of super-block s in a device xb row."""
    return 8 * s + 2 * (j & 3) + (j >> 2)


def xb_rows(bsums):
    """bsums int [..., n/16] -> the device's xb f32 [..., n/32]: sub-block sums in slot order."""
    bsums = np.asarray(bsums)
    b32 = bsums.reshape(bsums.shape[:-1] + (-1, 2)).sum(axis=-1)
    n32 = b32.shape[-1]
    s, j = np.arange(n32) // 8, np.arange(n32) % 8
    out = np.empty(b32.shape, dtype=F32)
    out[..., xb_slot(s, j)] = b32
    return out


def bsum32_of_xb(xb):
    """Device xb [..., n/32] -> sub-block sums in k order, int64."""
    xb = np.asarray(xb)
    n32 = xb.shape[-1]
    s, j = np.arange(n32) // 8, np.arange(n32) % 8
    v = xb[..., xb_slot(s, j)]
    assert np.array_equal(v, np.rint(v))
    return v.astype(np.int64)


# ---- packed tiles -----------------------------------------------------------------------------------------------------
def pack_tiles(t, blocks, mode=0, offset=0):
    """blocks uint8 [N][SB * block bytes] (N % 16 == 0 after placement) -> the packed matrix, uint8 flat.  mode 0:
    logical row r at packed row r + offset (rows below offset: 0xFF); mode 1 / 2 (gate / up): row r at packed row
    16 (r >> 3) + (r & 7) (+ 8 for up) of a 2 N-row matrix, the other half 0xFF."""
    f = kq_fields(t, blocks)
    N, SB = f["d"].shape
    rows = N + offset if mode == 0 else 2 * N
    assert rows % 16 == 0
    P = np.arange(N) + offset if mode == 0 else 16 * (np.arange(N) >> 3) + (np.arange(N) & 7) + (8 if mode == 2 else 0)
    nt = rows // 16
    out = np.full((nt, SB, TILE_BYTES[t]), 0xFF, dtype=np.uint8)
    tile, r = P >> 4, P & 15
    SC = TILE_SC[t]
    v = f["vals"].reshape(N, SB, 2, 4, 4, 2, 4)  # [n][sb][jhi][jlo][g][h][b]: k = 32 (4 jhi + jlo) + 8 g + 4 h + b
    for n in range(N):
        T = out[tile[n]]  # [SB][bytes] view
        vv = v[n]
        # QS: offset 1024 jhi + 16 (r + 16 g) + 4 jlo + b
        qs = ((vv[..., 0, :] & 15) | ((vv[..., 1, :] & 15) << 4)).transpose(0, 1, 3, 2, 4)  # [sb][jhi][g][jlo][b]
        for g in range(4):
            lane = r[n] + 16 * g
            for jhi in range(2):
                T[:, 1024 * jhi + 16 * lane:1024 * jhi + 16 * lane + 16] = qs[:, jhi, g].reshape(SB, 16)
        if t == Q5_K:
            b4 = (vv >> 4) & 1  # [sb][c = jhi][jj = jlo][g][h][b] -> bit 2 jj + h of byte 8 lane + 4 c + b
            by = np.zeros((SB, 2, 4, 4), dtype=np.uint8)  # [sb][c][g][b]
            for jj in range(4):
                for h in range(2):
                    by |= b4[:, :, jj, :, h, :] << (2 * jj + h)
            for g in range(4):
                lane = r[n] + 16 * g
                T[:, 2048 + 8 * lane:2048 + 8 * lane + 8] = by[:, :, g, :].reshape(SB, 8)
        if t == Q6_K:
            two = ((vv >> 4) & 3).reshape(SB, 2, 2, 2, 4, 2, 4)  # [sb][jhi][jl1][jj][g][h][b], dword c = 2 jhi + jl1
            by = np.zeros((SB, 2, 2, 4, 4), dtype=np.uint8)  # [sb][jhi][jl1][g][b]
            for jj in range(2):
                for h in range(2):
                    by |= two[:, :, :, jj, :, h, :] << (2 * (2 * jj + h))
            for g in range(4):
                lane = r[n] + 16 * g
                T[:, 2048 + 16 * lane:2048 + 16 * lane + 16] = by[:, :, :, g, :].reshape(SB, 16)
        q, i = r[n] >> 2, r[n] & 3
        if t == Q6_K:
            for c in range(16):
                T[:, SC + 64 * q + 4 * c + i] = f["sc"][n, :, c].view(np.uint8)
            T[:, SC + 256 + 2 * r[n]], T[:, SC + 256 + 2 * r[n] + 1] = f["d"][n] & 0xFF, f["d"][n] >> 8
        else:
            for c in range(8):
                T[:, SC + 64 * q + 4 * c + i] = f["sc"][n, :, c]
                T[:, SC + 64 * q + 4 * (8 + c) + i] = f["mn"][n, :, c]
            o = SC + 256 + 16 * q + 2 * i
            T[:, o], T[:, o + 1] = f["d"][n] & 0xFF, f["d"][n] >> 8
            T[:, o + 8], T[:, o + 9] = f["dmin"][n] & 0xFF, f["dmin"][n] >> 8
    return out.reshape(-1)


# ---- the exact product ------------------------------------------------------------------------------------------------
def sub_scales(t, f):
    """The integer scale of every k: Q4_K / Q5_K sc of its 32-value sub-block, Q6_K of its 16-value group; int16
    [N][K]."""
    if t == Q6_K:
        return np.repeat(f["sc"].astype(np.int16).reshape(f["sc"].shape[0], -1), 16, axis=1)
    return np.repeat(f["sc"].astype(np.int16).reshape(f["sc"].shape[0], -1), 32, axis=1)


def superblock_ints(t, f, xq, bs32=None):
    """(S, Mn) int64 [M][N][SB]: S = sum over the super-block of sc_k w_k q_k, Mn = sum_j m_j bsum32_j (Q6_K: 0).
    xq int [M][K] in k order; bs32 [M][K/32] (default: the sums of xq)."""
    xq = np.asarray(xq).astype(np.float64)
    M, K = xq.shape
    SB = K // 256
    w = (kq_ints(t, f).astype(np.int32) * sub_scales(t, f)).astype(np.float64)  # |.| <= 4096: products exact
    N = w.shape[0]
    S = np.rint(np.matmul(xq.reshape(M, SB, 256).transpose(1, 0, 2), w.reshape(N, SB, 256).transpose(1, 2, 0)))
    S = S.transpose(1, 2, 0).astype(np.int64)
    if t == Q6_K:
        return S, np.zeros_like(S)
    if bs32 is None:
        bs32 = xq.reshape(M, K // 32, 32).sum(axis=-1)
    b = np.asarray(bs32, dtype=np.float64).reshape(M, SB, 8).transpose(1, 0, 2)
    Mn = np.rint(np.matmul(b, f["mn"].astype(np.float64).transpose(1, 2, 0))).transpose(1, 2, 0).astype(np.int64)
    return S, Mn


def product(t, f, xq, xd, bs32=None):
    """(sum_s (d d_x) S - (dmin d_x) Mn, sum_s |.| + |.|) in float64 [M][N]; xd [M][SB]."""
    S, Mn = superblock_ints(t, f, xq, bs32)
    dx = np.asarray(xd, dtype=np.float64)[:, None, :]
    a = f16_f32(f["d"]).astype(np.float64)[None] * dx * S
    if t == Q6_K:
        return a.sum(axis=-1), np.abs(a).sum(axis=-1)
    b = f16_f32(f["dmin"]).astype(np.float64)[None] * dx * Mn
    return (a - b).sum(axis=-1), (np.abs(a) + np.abs(b)).sum(axis=-1)


# ---- dequantisation (ggml dequantize_row_q{4,5,6}_K, f32, one rounding per operation) ------------------------------------
def dequant_f32(t, f):
    """f32 [N][K]: Q4_K / Q5_K (d sc) q - dmin m; Q6_K (d sc) (q - 32)."""
    d = f16_f32(f["d"])
    with np.errstate(over="ignore", invalid="ignore"):
        if t == Q6_K:
            ds = (d[..., None] * f["sc"].astype(F32)).astype(F32)  # [N][SB][16]
            return (np.repeat(ds.reshape(ds.shape[0], -1), 16, axis=1) * kq_ints(t, f).astype(F32)).astype(F32)
        d1 = (d[..., None] * f["sc"].astype(F32)).astype(F32)
        m1 = (f16_f32(f["dmin"])[..., None] * f["mn"].astype(F32)).astype(F32)
        d1, m1 = np.repeat(d1.reshape(d1.shape[0], -1), 32, axis=1), np.repeat(m1.reshape(m1.shape[0], -1), 32, axis=1)
        return ((d1 * f["vals"].astype(F32)).astype(F32) - m1).astype(F32)


def dequant_bf16_tiles(t, f):
    """The packed bf16 tiles (tests/mm_layout.py's order) of dequant_f32 rounded to nearest even, uint16 flat."""
    return L.pack_tiles(L.bf16_bits(dequant_f32(t, f)))
