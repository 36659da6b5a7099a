"""tests/kq_ref.py pinned bit for bit (no GPU): to the loop transcriptions of ggml-quants.c in tests/test_kquants.py
(ref_quantize_q8_k, _kq_ints, ref_vec_dot, REFS), to the C oracle (kq_quantize_q8k, kq_dequant, kq_vec_dot), to
gguf.py's dequantisers, and -- for the packed tile -- to a scalar reading of kquant.hip's layout comment.  Also
mx_kq_matmul_plan for the Llama-3-8B and TinyLlama matrices against plans worked out by hand from the launchers'
conditions."""
import numpy as np
import pytest

import kq_ref as R
import test_kquants as TK
from llama_p2p_amd import gguf, synth

F32 = np.float32


def rand_fields(t, N, SB, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-2, 2, size=(N, SB)).astype(np.float16).view(np.uint16)
    vals = rng.integers(0, R.VMAX[t] + 1, size=(N, 256 * SB), dtype=np.uint8)
    if t == R.Q6_K:
        return dict(dbits=d, vals=vals, sc=rng.integers(-128, 128, size=(N, SB, 16)).astype(np.int8))
    return dict(dbits=d, vals=vals, sc=rng.integers(0, 64, size=(N, SB, 8), dtype=np.uint8),
                mbits=rng.uniform(-2, 2, size=(N, SB)).astype(np.float16).view(np.uint16),
                mn=rng.integers(0, 64, size=(N, SB, 8), dtype=np.uint8))


def blocks_of(t, N, SB, seed):
    kw = rand_fields(t, N, SB, seed)
    return R.kq_blocks(t, **kw), kw


@pytest.mark.parametrize("t", R.TYPES)
def test_block_builders_and_their_inverse(t):
    blocks, kw = blocks_of(t, 5, 3, 10 + t)
    assert blocks.shape == (5, 3 * R.BLOCK_BYTES[t]) == (5, 3 * gguf.BLOCKS[t][1])
    f = R.kq_fields(t, blocks)
    assert np.array_equal(f["d"], kw["dbits"]) and np.array_equal(f["vals"], kw["vals"]) and np.array_equal(f["sc"], kw["sc"])
    if t != R.Q6_K:
        assert np.array_equal(f["dmin"], kw["mbits"]) and np.array_equal(f["mn"], kw["mn"])
    # every byte is a field: any random block survives fields -> blocks
    raw = np.random.default_rng(t).integers(0, 256, size=(4, 2 * R.BLOCK_BYTES[t]), dtype=np.uint8)
    g = R.kq_fields(t, raw)
    back = R.kq_blocks(t, g["d"], g["vals"], g["sc"], g["dmin"], g["mn"])
    assert np.array_equal(back, raw)
    # ... and its integers and scales are those of the ggml loops
    for n in range(4):
        for s in range(2):
            b = [int(c) for c in raw[n, s * R.BLOCK_BYTES[t]:(s + 1) * R.BLOCK_BYTES[t]]]
            assert R.kq_ints(t, g)[n, 256 * s:256 * s + 256].tolist() == TK._kq_ints(t, b)
            if t != R.Q6_K:
                scm = [TK.get_scale_min_k4(j, b[4:16]) for j in range(8)]
                assert g["sc"][n, s].tolist() == [a for a, _ in scm] and g["mn"][n, s].tolist() == [m for _, m in scm]


def crafted_rows():
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1.3, size=(4, 1024)).astype(F32)
    x[0, 256:512] = 0.0                                # an all-zero super-block
    x[0, 600], x[0, 700] = -9.0, 9.0                   # tie in |x|, the first negative
    x[1, 10], x[1, 5] = -7.5, 7.5                      # tie, the first positive
    x[1, 256:512] = 0.0
    x[1, 300] = -3.0                                   # the only non-zero element is the maximum
    x[2, 0:256] = np.float32(-0.0)
    x[2, 512:768] = (np.arange(256) - 128).astype(F32) / 2  # halves: ties to even after scaling by 127 / 64
    x[2, 512] = 63.5
    x[3, 768:1024] = 127.0 * 2.0 ** -5
    x[3, 768 + 15], x[3, 768 + 16] = -127.0 * 2.0 ** -5, 2.0 ** -5 * 2.5
    return x


def test_quantize_q8k_matches_ggml_loop_and_oracle(oracle_mod):
    x = crafted_rows()
    q, d, bs = R.quantize_q8k(x)
    for r in range(x.shape[0]):
        oq, od, ob = oracle_mod.kq_quantize_q8k(x[r])
        assert np.array_equal(q[r], np.asarray(oq).astype(np.int8)) and np.array_equal(bs[r], np.asarray(ob))
        assert np.array_equal(d[r].view(np.uint32), np.asarray(od, dtype=F32).view(np.uint32))
        for i, (rd, rq, rb) in enumerate(TK.ref_quantize_q8_k(x[r])):
            assert F32(rd).view(np.uint32) == d[r, i].view(np.uint32)
            assert q[r, 256 * i:256 * i + 256].tolist() == rq and bs[r, 16 * i:16 * i + 16].tolist() == rb
    assert d[0, 1] == 0 and not q[0, 256:512].any() and d[0, 2] > 0 and d[1, 0] < 0
    assert q[1, 300] == -127 and np.count_nonzero(q[1, 256:512]) == 1
    assert d[2, 0] == 0 and q[3, 768] == -127 and q[3, 768 + 15] == 127


def test_nearest_int_is_round_half_even():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -127.5, 3.49999, -0.0], dtype=F32)
    assert R.nearest_int(v).tolist() == [TK.ref_nearest_int(a) for a in v] == [0, 2, 2, 0, -2, -2, 126, 128, -128, 3, 0]


def test_activation_row_order():
    for k in range(512):
        s, j, g, e = k // 256, (k % 256) // 32, (k % 32) // 8, k % 8
        assert R.xq_perm(k) == 256 * s + 64 * g + 8 * j + e
    q = np.arange(512, dtype=np.int16)[None]
    assert np.array_equal(R.unperm_rows(R.perm_rows(q)), q)
    bs = np.arange(32)[None]  # bsums of 16: sub-block j of super-block s = bs[16 s + 2 j] + bs[16 s + 2 j + 1]
    xb = R.xb_rows(bs)
    for s in range(2):
        for j in range(8):
            assert xb[0, 8 * s + 2 * (j & 3) + (j >> 2)] == bs[0, 16 * s + 2 * j] + bs[0, 16 * s + 2 * j + 1]
    assert np.array_equal(R.bsum32_of_xb(xb), bs.reshape(1, 16, 2).sum(axis=-1))


def pow2_blocks(t, SB, seed):
    """One row of blocks with d, dmin powers of two: the ggml loop's f32 result is then exact."""
    kw = rand_fields(t, 1, SB, seed)
    rng = np.random.default_rng(seed)
    kw["dbits"] = R.f16_bits(2.0 ** rng.integers(-8, -5, size=(1, SB)))
    if t != R.Q6_K:
        kw["mbits"] = R.f16_bits(2.0 ** rng.integers(-8, -5, size=(1, SB)))
    return R.kq_blocks(t, **kw)


@pytest.mark.parametrize("t", R.TYPES)
def test_superblock_integers_match_vec_dot(oracle_mod, t):
    SB = 3
    blocks = pow2_blocks(t, SB, 40 + t)
    rng = np.random.default_rng(t)
    xi = rng.integers(-6, 7, size=(1, 256 * SB))
    xi[0, [3, 300, 767]] = [127, -127, 127]
    e = np.array([[2, 3, 4]])
    x = (xi * np.repeat(2.0 ** -e, 256, axis=1)).astype(F32)
    q, d, bs = R.quantize_q8k(x)
    # iscale = -127 / max: a positive maximum gives d = -2^-e and the negated integers
    sign = -np.sign(xi[0, [3, 300, 767]])[None]
    assert np.array_equal(d, (sign * 2.0 ** -e).astype(F32)) and np.array_equal(q, xi * np.repeat(sign, 256, axis=1))
    f = R.kq_fields(t, blocks)
    want, mag = R.product(t, f, q, d)
    assert mag.max() / 2.0 ** (-8 - 4) < 2 ** 24  # every partial sum exact in f32
    loop = TK.ref_vec_dot(t, blocks.reshape(-1), x[0])
    assert float(loop) == want[0, 0]
    assert float(oracle_mod.kq_vec_dot(t, blocks.reshape(-1), x[0])) == want[0, 0]
    # the integers themselves: the scalar sums over sub-blocks
    S, Mn = R.superblock_ints(t, f, q, R.bsum32_of_xb(R.xb_rows(bs)))
    w = R.kq_ints(t, f)[0].astype(int)
    for s in range(SB):
        if t == R.Q6_K:
            ref = sum(int(f["sc"][0, s, g]) * int(np.dot(w[256 * s + 16 * g:][:16], q[0, 256 * s + 16 * g:][:16])) for g in range(16))
            assert Mn[0, 0, s] == 0
        else:
            ref = sum(int(f["sc"][0, s, j]) * int(np.dot(w[256 * s + 32 * j:][:32], q[0, 256 * s + 32 * j:][:32])) for j in range(8))
            assert Mn[0, 0, s] == sum(int(f["mn"][0, s, j]) * int(q[0, 256 * s + 32 * j:][:32].astype(int).sum()) for j in range(8))
        assert S[0, 0, s] == ref


@pytest.mark.parametrize("t", R.TYPES)
def test_product_close_to_vec_dot_on_real_scales(oracle_mod, t):
    blocks = synth.kq_blocks(t, 3, seed=4, tid=77).reshape(1, -1)
    x = np.random.default_rng(t).normal(0, 1.0, 768).astype(F32)
    q, d, _ = R.quantize_q8k(x[None])
    want, mag = R.product(t, R.kq_fields(t, blocks), q, d)
    got = float(oracle_mod.kq_vec_dot(t, blocks.reshape(-1), x))
    assert abs(got - want[0, 0]) <= 16 * 2.0 ** -24 * mag[0, 0]


@pytest.mark.parametrize("t", R.TYPES)
def test_dequant_matches_ggml_loop_oracle_and_gguf(oracle_mod, t):
    raw = np.random.default_rng(t).integers(0, 256, size=(3, 2 * R.BLOCK_BYTES[t]), dtype=np.uint8)
    for o in ([208] if t == R.Q6_K else [0, 2]):  # finite f16 fields, one subnormal, one zero, one negative
        for s in range(2):
            vals = np.array([0.75, -1.5, 3e-7 if s else 0.0], np.float16) if o != 2 else np.array([0.5, -0.25, 6e-8], np.float16)
            raw[:, s * R.BLOCK_BYTES[t] + o:s * R.BLOCK_BYTES[t] + o + 2] = vals.view(np.uint8).reshape(3, 2)
    syn = synth.kq_blocks(t, 6, seed=1, tid=5).reshape(3, -1)
    for blocks in (raw, syn):
        f = R.kq_fields(t, blocks)
        y = R.dequant_f32(t, f)
        loop = np.array([[v for s in range(2) for v in TK.REFS[t]([int(c) for c in b[s * R.BLOCK_BYTES[t]:(s + 1) * R.BLOCK_BYTES[t]]])]
                         for b in blocks], dtype=F32)
        assert np.array_equal(y.view(np.uint32), loop.view(np.uint32))
        assert np.array_equal(y.view(np.uint32), gguf.dequantize(t, blocks, (3, 512)).view(np.uint32))
        fn = {R.Q4_K: gguf.dequantize_q4_k, R.Q5_K: gguf.dequantize_q5_k, R.Q6_K: gguf.dequantize_q6_k}[t]
        assert np.array_equal(np.asarray(fn(blocks.reshape(-1, R.BLOCK_BYTES[t]), 256), dtype=F32).reshape(3, 512).view(np.uint32),
                              y.view(np.uint32))
        for n in range(3):
            o = oracle_mod.kq_dequant(t, blocks[n], 512)
            assert np.array_equal(np.asarray(o, dtype=F32).view(np.uint32), y[n].view(np.uint32))


def tile_value(t, tile, r, k):
    """Value k of row r read from one packed tile by the layout comment, scalar."""
    j, g, e = k // 32, (k % 32) // 8, k % 8
    lane = r + 16 * g
    D = int.from_bytes(bytes(tile[(j >> 2) * 1024 + 16 * lane + 4 * (j & 3):][:4]), "little")
    v = (D >> (8 * (e & 3) + 4 * (e >> 2))) & 15
    u = 2 * j + (e >> 2)
    if t == R.Q5_K:
        H = int.from_bytes(bytes(tile[2048 + 8 * lane + 4 * (u >> 3):][:4]), "little")
        v |= ((H >> (8 * (e & 3) + (u & 7))) & 1) << 4
    if t == R.Q6_K:
        H = int.from_bytes(bytes(tile[2048 + 16 * lane + 4 * (u >> 2):][:4]), "little")
        v |= ((H >> (8 * (e & 3) + 2 * (u & 3))) & 3) << 4
    return v


@pytest.mark.parametrize("mode,offset", [(0, 0), (0, 16), (1, 0), (2, 0)])
@pytest.mark.parametrize("t", R.TYPES)
def test_packed_tile_layout(t, mode, offset):
    N, SB = 32, 2
    blocks, kw = blocks_of(t, N, SB, 70 + t)
    flat = R.pack_tiles(t, blocks, mode, offset)
    rows = N + offset if mode == 0 else 2 * N
    assert flat.size == rows // 16 * SB * R.TILE_BYTES[t]
    tiles = flat.reshape(rows // 16, SB, R.TILE_BYTES[t])
    SC = R.TILE_SC[t]
    written = np.zeros(rows, bool)
    rng = np.random.default_rng(5)
    for n in range(N):
        P = n + offset if mode == 0 else 16 * (n >> 3) + (n & 7) + (8 if mode == 2 else 0)
        written[P] = True
        r, q, i = P & 15, (P & 15) >> 2, P & 3
        for s in range(SB):
            T = tiles[P >> 4, s]
            for k in list(rng.integers(0, 256, 24)) + [0, 7, 8, 31, 32, 255]:
                assert tile_value(t, T, r, int(k)) == kw["vals"][n, 256 * s + k]
            if t == R.Q6_K:
                assert [int(np.int8(T[SC + 64 * q + 4 * c + i])) for c in range(16)] == kw["sc"][n, s].tolist()
                assert int(T[SC + 256 + 2 * r]) | int(T[SC + 257 + 2 * r]) << 8 == kw["dbits"][n, s]
            else:
                assert [int(T[SC + 64 * q + 4 * c + i]) for c in range(8)] == kw["sc"][n, s].tolist()
                assert [int(T[SC + 64 * q + 4 * (8 + c) + i]) for c in range(8)] == kw["mn"][n, s].tolist()
                o = SC + 256 + 16 * q + 2 * i
                assert int(T[o]) | int(T[o + 1]) << 8 == kw["dbits"][n, s]
                assert int(T[o + 8]) | int(T[o + 9]) << 8 == kw["mbits"][n, s]
    # rows the mode leaves to another launch hold no byte of this one: whole tiles, or (gate / up) the other half's lanes
    for P in np.nonzero(~written)[0]:
        r = P & 15
        for s in range(SB):
            T = tiles[P >> 4, s]
            assert all((T[1024 * h + 16 * (r + 16 * g):][:16] == 0xFF).all() for g in range(4) for h in range(2))
            assert (T[SC + 64 * (r >> 2) + (r & 3):SC + 64 * (r >> 2) + 64:4] == 0xFF).all()


# ---- mx_kq_matmul_plan: the Llama-3-8B and TinyLlama matrices ---------------------------------------------------------------
F32E, RESID, QKV, SWIGLU = 0, 1, 2, 3
L3 = dict(qkv=(QKV, 6144, 4096, [(12, 320), (14, 384)]), o=(RESID, 4096, 4096, 12), gu=(SWIGLU, 28672, 4096, 12),
          down=(RESID, 4096, 14336, 14), head=(F32E, 128256, 4096, 14))
TL = dict(qkv=(QKV, 2560, 2048, [(12, 144), (14, 160)]), o=(RESID, 2048, 2048, 12), gu=(SWIGLU, 11264, 2048, 12),
          down=(RESID, 2048, 5632, 14), head=(F32E, 32000, 2048, 14))
GEMV = dict(kind="mkq", ks=8, tpw=1, w=0)
# (model, matrix, M, on_load, norm, flags) -> the fields worked out from launch_mkq's conditions
PLANS = [
    # one token, quantised on load (the decode): K 4096 q|k|v with even segment ends -> mkq_pers_seg_kernel
    (L3, "qkv", 1, 1, 1, 0, dict(kind="qkv_pers", t=0, ks=8, nkw=2, tpw=2, u=4, bd=1, ql=1, grid_x=192)),
    (L3, "o", 1, 1, 0, 0, dict(GEMV, nkw=2, u=2, bd=1, ql=1, nb=1, grid_x=256, grid_y=1)),         # 16 / 8 = 2 per wave
    (L3, "gu", 1, 1, 1, 0, dict(kind="bd_tile", t=12, w=7, nkw=16, tpw=1, u=8, grid_x=256)),      # 1792 <= 1792
    (L3, "down", 1, 1, 0, 0, dict(GEMV, nkw=7, u=7, bd=1, ql=1, grid_x=256)),                      # 56 / 8 = 7
    (L3, "head", 1, 1, 1, 0, dict(kind="bd_tile", t=14, w=8, nkw=16, tpw=4, u=8, grid_x=251)),    # 8016 tiles / 32
    (L3, "gu", 1, 1, 1, 1, dict(kind="pers", t=12, ks=8, nkw=2, tpw=7, u=4, bd=1, ql=1, grid_x=256)),  # MX_NO_KQ_BD_TILE
    (L3, "head", 1, 1, 1, 1, dict(kind="pers", t=14, ks=8, nkw=2, tpw=8, u=4, bd=1, ql=1, grid_x=1002)),
    (L3, "gu", 1, 1, 1, 2, dict(GEMV, nkw=2, u=2, bd=1, ql=1, grid_x=1792)),                       # MX_NO_KQ_PERS
    # 4 sequences, pre-quantised rows
    (L3, "qkv", 4, 0, 0, 0, dict(GEMV, nkw=2, u=2, bd=0, ql=0, nb=1, grid_x=384)),
    (L3, "gu", 4, 0, 0, 0, dict(kind="pers", t=12, ks=8, nkw=2, tpw=7, u=2, bd=0, ql=0, nb=1, grid_x=256)),
    (L3, "head", 4, 0, 0, 0, dict(kind="pers", t=14, ks=8, nkw=2, tpw=8, u=2, bd=0, grid_x=1002)),
    (L3, "head", 1, 0, 0, 0, dict(kind="pers", t=14, ks=8, nkw=2, tpw=8, u=4, bd=1, ql=0, grid_x=1002)),
    (L3, "down", 16, 0, 0, 0, dict(GEMV, nkw=7, u=2, bd=0, nb=1, grid_x=256, slab_ks=-1)),
    # 32 sequences: the LDS-shared form and the split-K slabs
    (L3, "gu", 32, 0, 0, 0, dict(kind="wide", t=12, w=7, nb=2, u=4, grid_x=256, grid_y=1)),       # 1792 = 7 x 256
    (L3, "head", 32, 0, 0, 0, dict(kind="wide", t=14, w=8, nb=2, u=2, grid_x=1002)),               # 8016 = 8 x 1002
    (L3, "qkv", 32, 0, 0, 0, dict(GEMV, nb=2, u=1, grid_x=384, grid_y=1, qkv_slab_ks=2)),          # 96 groups x 2
    (L3, "o", 17, 0, 0, 0, dict(GEMV, nb=2, u=1, slab_ks=4)),                                      # 64 groups x 4
    (L3, "down", 32, 0, 0, 0, dict(GEMV, nb=2, u=1, slab_ks=4)),
    (L3, "gu", 32, 0, 0, 4, dict(GEMV, nb=2, u=1, grid_x=1792, slab_ks=-1)),                       # MX_NO_KQ_WIDE
    (L3, "o", 32, 0, 0, 4, dict(GEMV, slab_ks=-1, qkv_slab_ks=-1)),
    (L3, "gu", 33, 0, 0, 0, dict(GEMV, nb=2, u=1, grid_x=1792, grid_y=2, slab_ks=-1)),
    (L3, "gu", 64, 0, 0, 0, dict(GEMV, nb=2, u=1, grid_y=2)),
    # TinyLlama
    (TL, "qkv", 1, 1, 1, 0, dict(GEMV, nkw=1, u=1, bd=1, ql=1, grid_x=160)),                       # K 2048: no q|k|v form
    (TL, "gu", 1, 1, 1, 0, dict(kind="bd_tile", t=12, w=3, nkw=8, tpw=1, u=8, grid_x=235)),       # ceil(704 / 3)
    (TL, "down", 1, 1, 0, 0, dict(GEMV, nkw=3, u=4, bd=1, ql=1, grid_x=128)),                      # ceil(22 / 8) = 3
    (TL, "head", 1, 1, 1, 0, dict(kind="bd_tile", t=14, w=8, nkw=8, tpw=1, u=8, grid_x=250)),
    (TL, "gu", 1, 1, 1, 1, dict(kind="pers", t=12, ks=8, nkw=1, tpw=3, u=3, bd=1, ql=1, grid_x=235)),
    (TL, "head", 1, 1, 1, 1, dict(kind="pers", t=14, ks=8, nkw=1, tpw=8, u=4, bd=1, ql=1, grid_x=250)),
    (TL, "gu", 8, 0, 0, 0, dict(kind="pers", t=12, ks=8, nkw=1, tpw=3, u=2, bd=0, grid_x=235)),
    (TL, "gu", 32, 0, 0, 0, dict(kind="wide", t=12, w=4, nb=2, u=4, grid_x=176)),                  # 704 % 7, 88 < 200
    (TL, "head", 32, 0, 0, 0, dict(kind="wide", t=14, w=8, u=2, grid_x=250)),                      # 2000 = 8 x 250
    (TL, "o", 32, 0, 0, 0, dict(GEMV, nb=2, slab_ks=2)),                                           # 8 / 4 < 4 super-blocks
    (TL, "down", 32, 0, 0, 0, dict(GEMV, nb=2, slab_ks=4)),                                        # 22 / 8 < 4
    (TL, "qkv", 32, 0, 0, 0, dict(GEMV, nb=2, qkv_slab_ks=2)),
]


@pytest.mark.parametrize("case", PLANS, ids=[f"{'L3' if c[0] is L3 else 'TL'}-{c[1]}-M{c[2]}-ql{c[3]}-f{c[5]}" for c in PLANS])
def test_plans_of_the_llama_matrices(case):
    from llama_p2p_amd import engine

    model, name, M, on_load, norm, flags, want = case
    epi, N, K, segs = model[name]
    p = engine.kq_matmul_plan(epi, M, N, K, segs, on_load=bool(on_load), norm=bool(norm), flags=flags)
    got = {k: p[k] for k in want}
    assert got == want, p
    assert p["can_on_load"] == (M == 1)


def test_plan_edges():
    from llama_p2p_amd import engine as E

    plan = E.kq_matmul_plan
    assert plan(F32E, 1, 64, 16384, 12, on_load=True)["u"] == 8 and plan(F32E, 1, 64, 16640, 12, on_load=True)["kind"] == "none"
    assert plan(F32E, 1, 64, 8192, 12, on_load=True, norm=True)["kind"] == "mkq"
    assert plan(F32E, 1, 64, 8448, 12, on_load=True, norm=True)["kind"] == "none"  # more than 512 partials
    assert plan(F32E, 1, 64, 16640, 12)["u"] == 2 and plan(F32E, 1, 64, 14336, 12)["u"] == 2  # pre-quantised: ring 2
    # q|k|v: an odd segment end or another K leaves mkq_kernel
    assert plan(QKV, 1, 256, 4096, [(12, 11), (14, 16)], on_load=True)["kind"] == "mkq"
    assert plan(QKV, 1, 256, 4096, [(12, 12), (14, 16)], on_load=True)["kind"] == "qkv_pers"
    assert plan(QKV, 1, 256, 4352, [(12, 12), (14, 16)], on_load=True)["kind"] == "mkq"
    # the persistent kernel's exact tile counts
    assert plan(SWIGLU, 2, 16 * 704, 2048, 13)["kind"] == "pers" and plan(SWIGLU, 2, 16 * 706, 2048, 13)["kind"] == "mkq"
    assert plan(F32E, 2, 16 * 1025, 2048, 12)["kind"] == "pers" and plan(F32E, 2, 16 * 1024, 2048, 12)["kind"] == "mkq"
    assert plan(F32E, 2, 16 * 2049, 4096, 12)["kind"] == "pers" and plan(F32E, 2, 16 * 2048, 4096, 12)["kind"] == "mkq"
    assert plan(F32E, 17, 16 * 2049, 4096, 12)["kind"] == "mkq"  # 2049 tiles: no W divides them
    # segments: a bad type, ends that do not reach N, more than one type under a single-type kernel
    assert plan(F32E, 1, 64, 256, [(11, 4)])["kind"] == "none" and plan(F32E, 1, 64, 256, [(12, 3)])["kind"] == "none"
    assert plan(F32E, 32, 64, 1024, [(12, 2), (14, 4)])["kind"] == "mkq"
    # slabs: K 1024 has too few super-blocks to split, N 16384 already fills the target
    assert plan(RESID, 32, 64, 1024, 12)["slab_ks"] == -1 and plan(RESID, 32, 16384, 4096, 12)["slab_ks"] == -1
    assert [plan(RESID, 32, 64, k, 12)["slab_ks"] for k in (2048, 2304, 4096, 4352, 8192)] == [2, 2, 4, 4, 8]
    assert plan(RESID, 32, 4096, 4096, 12)["slab_ks"] == 4 and plan(RESID, 32, 8192, 4096, 12)["slab_ks"] == 2
    assert plan(QKV, 32, 256, 1024, [(12, 12), (14, 16)])["qkv_slab_ks"] == 1
    assert plan(QKV, 32, 256, 4096, [(12, 10), (14, 16)])["qkv_slab_ks"] == -1
    assert plan(RESID, 16, 64, 4096, 12)["slab_ks"] == -1 and plan(RESID, 33, 64, 4096, 12)["slab_ks"] == -1
