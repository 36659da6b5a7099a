"""References and inputs for the dequantise-at-load, residual-stream boundary and argmax kernels
(tests/test_glue_kernel_gpu.py); pinned on the host by tests/test_glue_ref.py.

  bf16_rne     f32 -> bf16 bits, round to nearest even, a NaN -> (u >> 16) | 0x40 (ggml_compute_fp32_to_bf16)
  ssq16_emul   the device's ssq16 (csrc/device_common.h) bit for bit
  argmax_ref   launch_argmax's rule as a plain loop
  SPECIALS     every 16-bit upper half x six lower halves: 393 216 f32 bit patterns
  blocks_*     raw GGUF blocks of Q4_0 / Q8_0 / Q4_K / Q5_K / Q6_K: (a) random, (b) field edges, (c) one-hot, (d) a
               distinct d per block
"""
import functools

import numpy as np

F32, F16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 2, 8, 12, 13, 14
BLOCKS = {Q4_0: (32, 18), Q8_0: (32, 34), Q4_K: (256, 144), Q5_K: (256, 176), Q6_K: (256, 210)}
QUANT = [Q4_0, Q8_0, Q4_K, Q5_K, Q6_K]
TNAME = {F32: "f32", F16: "f16", Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4k", Q5_K: "q5k", Q6_K: "q6k"}
D_OFF = {Q4_0: 0, Q8_0: 0, Q4_K: 0, Q5_K: 0, Q6_K: 208}  # byte offset of the f16 d

LOWS = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
SPECIALS = ((np.arange(65536, dtype=np.uint32)[:, None] << 16) | LOWS[None, :]).reshape(-1)
SPECIALS.setflags(write=False)
# d: 0, -0, the smallest f16 subnormal, 65504, +inf, a quiet NaN; and -inf, a signalling NaN, -65504
D_EDGES = np.array([0x0000, 0x8000, 0x0001, 0x7BFF, 0x7C00, 0x7E00, 0xFC00, 0x7C01, 0xFBFF], dtype=np.uint16)


def is_nan_bits32(u):
    return (np.asarray(u, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000


def is_nan_bits16(h):
    return (np.asarray(h, dtype=np.uint16) & 0x7FFF) > 0x7F80


def bf16_rne(x):
    """bf16 bits (uint16) of f32 values (or of uint32 bit patterns): (u + 0x7fff + ((u >> 16) & 1)) >> 16, and for a
    NaN (u >> 16) | 0x40 -- sign and top payload bits kept, made quiet."""
    a = np.ascontiguousarray(x)
    u = a if a.dtype == np.uint32 else a.astype(np.float32, copy=False).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return np.where(is_nan_bits32(u), (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint16)


def ssq16_emul(x):
    """ssq16 of every 16 consecutive elements of each row, f32 [rows][n/16]: squares rounded to f32, summed in double
    sequentially inside each group of 4, the group sums combined as (g0 + g1) + (g2 + g3), rounded to f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sq = (x * x).astype(np.float64).reshape(x.shape[0], -1, 4, 4)
    g = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    return ((g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])).astype(np.float32)


def argmax_ref(row, V):
    """The greedy pick: a larger value wins, among equal values (+0 == -0) the lowest id, NaN never; all NaN -> 0."""
    best, bv = -1, 0.0
    for i, v in enumerate(np.asarray(row[:V], dtype=np.float32).tolist()):
        if v != v:
            continue
        if best < 0 or v > bv:
            best, bv = i, v
    return max(best, 0)


# ---- block builders ---------------------------------------------------------------------------------------------------
def rand_f16_bits(rng, size, emin=1, emax=30):
    """Random finite normal f16 bit patterns: any sign, exponent field in [emin, emax], all 10 mantissa bits random."""
    return (rng.integers(0, 2, size=size) << 15 | rng.integers(emin, emax + 1, size=size) << 10 |
            rng.integers(0, 1024, size=size)).astype(np.uint16)


def put_f16(b, off, bits):
    b[:, off:off + 2] = np.ascontiguousarray(bits, dtype=np.uint16).reshape(-1, 1).view(np.uint8)


def pack_scales_k4(s, m):
    """The 12 scale bytes of Q4_K / Q5_K from 6-bit scales s [nb][8] and mins m [nb][8] (get_scale_min_k4 inverted)."""
    s, m = np.asarray(s, dtype=np.int64), np.asarray(m, dtype=np.int64)
    sc = np.zeros(s.shape[:-1] + (12,), np.int64)
    sc[..., 0:4] = (s[..., 0:4] & 63) | ((s[..., 4:8] >> 4) << 6)
    sc[..., 4:8] = (m[..., 0:4] & 63) | ((m[..., 4:8] >> 4) << 6)
    sc[..., 8:12] = (s[..., 4:8] & 15) | ((m[..., 4:8] & 15) << 4)
    return sc.astype(np.uint8)


def blocks_random(t, nb, seed=0):
    """(a) every byte random; d and dmin random full-mantissa f16.  Q4_K / Q5_K: d's exponent field in [8, 20] and
    dmin's 3 above it, so that d sc q and dmin m are of one magnitude and the subtraction often cancels: the low
    bits of both terms reach the bf16 result."""
    rng = np.random.default_rng(100 * t + seed)
    b = rng.integers(0, 256, size=(nb, BLOCKS[t][1]), dtype=np.uint8)
    if t in (Q4_K, Q5_K):
        e = rng.integers(8, 21, size=nb)
        put_f16(b, 0, (e << 10 | rng.integers(0, 1024, size=nb)).astype(np.uint16))
        put_f16(b, 2, ((e + 3) << 10 | rng.integers(0, 1024, size=nb)).astype(np.uint16))
    else:
        put_f16(b, D_OFF[t], rand_f16_bits(rng, nb))
    return b


def blocks_edges(t, seed=1):
    """(b) field edges: the quantised fields at both ends of their range (Q4_K / Q5_K scales and mins at 0 and 63 in
    each of the 8 sub-blocks, Q6_K scales at -128 and 127 in each of the 16), then every D_EDGES value as d (and as
    dmin) over random fields."""
    rng = np.random.default_rng(100 * t + seed)
    bb = BLOCKS[t][1]
    out = []
    if t == Q4_0:
        for v in (0x00, 0xFF, 0x0F, 0xF0):
            b = blocks_random(t, 1, seed + v)
            b[:, 2:] = v
            out.append(b)
    elif t == Q8_0:
        for v in (0x80, 0x7F):
            b = blocks_random(t, 1, seed + v)
            b[:, 2:] = v
            out.append(b)
        b = blocks_random(t, 1, seed + 2)
        b[:, 2:] = np.where(np.arange(32) % 2, 0x80, 0x7F)
        out.append(b)
    elif t in (Q4_K, Q5_K):
        for j in range(8):
            for sv, mv in ((0, 63), (63, 0), (63, 63), (0, 0)):
                b = blocks_random(t, 1, seed + 10 * j + sv + mv // 63)
                s, m = rng.integers(1, 63, size=(1, 8)), rng.integers(1, 63, size=(1, 8))
                s[0, j], m[0, j] = sv, mv
                b[:, 4:16] = pack_scales_k4(s, m)
                out.append(b)
    else:
        for j in range(16):
            for v in (-128, 127):
                b = blocks_random(t, 1, seed + 10 * j + (v & 1))
                sc = rng.integers(-100, 100, size=16)
                sc[j] = v
                b[0, 192:208] = sc.astype(np.int8).view(np.uint8)
                out.append(b)
    for off in ([0, 2] if t in (Q4_K, Q5_K) else [D_OFF[t]]):
        b = blocks_random(t, len(D_EDGES), seed + 50 + off)
        put_f16(b, off, D_EDGES)
        out.append(b)
    b = np.concatenate(out)
    assert b.shape[1] == bb
    return b


def one_hot_positions(t):
    """[(field, byte offset of the field, byte, bit or nibble, value)] of the one-hot blocks of type t."""
    pos = []
    if t == Q5_K:
        pos += [("qh", 16, i, k, 1 << k) for i in range(32) for k in range(8)]
        pos += [("qs", 48, i, k, (1 + (i + k) % 15) << (4 * k)) for i in range(128) for k in range(2)]
    elif t == Q6_K:
        pos += [("qh", 128, i, k, 1 << k) for i in range(64) for k in range(8)]
        pos += [("ql", 0, i, k, (1 + (i + k) % 15) << (4 * k)) for i in range(128) for k in range(2)]
    elif t == Q4_K:
        pos += [("qs", 16, i, k, (1 + (i + k) % 15) << (4 * k)) for i in range(128) for k in range(2)]
    return pos


def blocks_one_hot(t):
    """(c) per block exactly one qh bit or one nibble set, over every position; d = 1, every scale 1 (Q4_K / Q5_K:
    dmin = 1, mins 0), so the one element that differs from the rest names the (g, l) that was read."""
    pos = one_hot_positions(t)
    b = np.zeros((len(pos), BLOCKS[t][1]), dtype=np.uint8)
    one = np.array([0x3C00], dtype=np.uint16)
    put_f16(b, D_OFF[t], np.repeat(one, len(pos)))
    if t == Q6_K:
        b[:, 192:208] = 1
    else:
        put_f16(b, 2, np.repeat(one, len(pos)))
        b[:, 4:16] = pack_scales_k4(np.ones((1, 8)), np.zeros((1, 8)))
    for r, (_, off, i, _, v) in enumerate(pos):
        b[r, off + i] = v
    return b


def blocks_distinct_d(t, nb, seed=3):
    """(d) random blocks whose d differs from block to block: f16 bits 0x0400 + 5 i (normal, positive, increasing)."""
    b = blocks_random(t, nb, seed)
    bits = 0x0400 + 5 * np.arange(nb)
    assert bits.max() < 0x7800
    put_f16(b, D_OFF[t], bits.astype(np.uint16))
    return b


CASES = ("random", "edges", "one_hot", "distinct_d")


@functools.lru_cache(maxsize=None)
def blocks_case(t, case, nb):
    """nb blocks of the case (uint8 [nb][block bytes]); the fixed sets (edges, one-hot) repeat cyclically."""
    if case == "random":
        b = blocks_random(t, nb)
    elif case == "distinct_d":
        b = blocks_distinct_d(t, nb)
    else:
        src = blocks_edges(t) if case == "edges" else blocks_one_hot(t)
        b = src[np.arange(nb) % len(src)]
    b.setflags(write=False)
    return b


def has_case(t, case):
    return case != "one_hot" or t in (Q4_K, Q5_K, Q6_K)


def k4_terms(t, blocks):
    """(d1 f32 [nb][8], m1 f32 [nb][8], q f32 [nb][8][32]) of Q4_K / Q5_K blocks: y = d1 q - m1."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCKS[t][1])
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)
    sc = b[:, 4:16].astype(np.int32)
    s, m = np.empty((len(b), 8), np.int32), np.empty((len(b), 8), np.int32)
    s[:, :4], m[:, :4] = sc[:, 0:4] & 63, sc[:, 4:8] & 63
    s[:, 4:] = (sc[:, 8:12] & 0xF) | ((sc[:, 0:4] >> 6) << 4)
    m[:, 4:] = (sc[:, 8:12] >> 4) | ((sc[:, 4:8] >> 6) << 4)
    qs = b[:, (48 if t == Q5_K else 16):].reshape(-1, 4, 32).astype(np.int32)
    q = np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 8, 32)
    if t == Q5_K:
        qh = b[:, 16:48].astype(np.int32)
        q = q + 16 * ((qh[:, None, :] >> np.arange(8)[None, :, None]) & 1)
    return (d * s.astype(np.float32)).astype(np.float32), (dmin * m.astype(np.float32)).astype(np.float32), q.astype(np.float32)


def order_tile():
    """16 values (bf16-exact) whose ssq16 depends on the order of the four group sums: g0 = 2^53, g1 = 2^29 (an f32
    tie), g2 = g3 = 1.  (g0 + g1) + (g2 + g3) = 2^53 + 2^29 + 2 rounds up to 2^53 + 2^30; ((g0 + g1) + g2) + g3 loses
    each 1 in double (ulp 2) and the tie rounds to even, 2^53."""
    y = np.zeros(16, np.float32)
    y[0] = y[1] = 2.0 ** 26
    y[4] = y[5] = 2.0 ** 14
    y[8] = y[12] = 1.0
    return y
