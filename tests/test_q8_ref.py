"""tests/q8_ref.py pinned on the CPU: the activation quantiser against known answers and ties (ggml's
quantize_row_q8_0 with the AVX2 / NEON rounding: half to even; the oracle's C exposes its Q8_0 activation
quantiser only inside orc_q4_0_vec_dot, which is used here as a second witness), q8_perm as a bijection with the
lane-group property kernels.h states, both tile layouts by round trip and by direct element addressing, the
dequantisation, the RMS_NORM scale and the block matmul; and mx_q8_matmul_plan for the Llama-3-8B matrices."""
import numpy as np
import pytest

import mm_layout as L
import q8_ref as R


def test_quantiser_known_answers_and_ties():
    x = np.zeros((1, 64), np.float32)
    x[0, 0] = 127.0                       # amax 127: d = 1, id = 1
    x[0, 1:5] = [0.5, 1.5, 2.5, -2.5]     # ties go to even: 0, 2, 2, -2 (roundf would give 1, 2, 3, -3)
    x[0, 5:8] = [0.49999997, 3.4999998, -126.5]
    q, d = R.quantize_act(x)
    assert d.tolist() == [[1.0, 0.0]]
    assert q[0, :8].tolist() == [127, 0, 2, 2, -2, 0, 3, -126]
    assert not q[0, 32:].any()            # an all-zero block: d = 0, id = 0, q = 0
    # amax held by a negative value
    y = np.zeros((1, 32), np.float32)
    y[0, 3], y[0, 4] = -12.7, 0.1
    q, d = R.quantize_act(y)
    d32 = np.float32(12.7) / np.float32(127)
    assert d[0, 0] == np.float32(np.float16(d32)) and q[0, 3] == -127
    assert q[0, 4] == int(np.rint(np.float32(0.1) * (np.float32(1) / d32)))
    # amax so small that d rounds to 0 in f16 while the q are nonzero
    z = np.zeros((1, 32), np.float32)
    z[0, 0], z[0, 1] = 1e-9, -5e-10
    q, d = R.quantize_act(z)
    assert d[0, 0] == 0.0 and q[0, :2].tolist() == [127, -64]  # 63.5 -> 64 (even)
    # integers n * 2^-e with one +-127 * 2^-e element per block come back exactly (e 0..14)
    rng = np.random.default_rng(0)
    for e in range(15):
        xi = rng.integers(-4, 5, size=(8, 256))
        xi[:, ::32] = 127 * (1 - 2 * rng.integers(0, 2, size=(8, 8)))
        q, d = R.quantize_act((xi * 2.0 ** -e).astype(np.float32))
        assert np.array_equal(q, xi) and (d == np.float32(2.0 ** -e)).all()


def test_quantiser_against_the_oracle_vec_dot(oracle_mod):
    """ggml_vec_dot_q4_0_q8_0 in the oracle quantises x with its own C quantiser: the dot product from the numpy
    quantiser's q and d agrees with it to f32 rounding of a 8-block sum -- a q off by one or a d off by an f16 ulp
    would move it by far more (the operands are chosen with large, distinct block contributions)."""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(256) * 3).astype(np.float32)
    wrow = (rng.standard_normal(256)).astype(np.float32)
    blocks = oracle_mod.q4_0_quantize_row(wrow)
    got = oracle_mod.q4_0_vec_dot(blocks, x)
    b = blocks.reshape(8, 18)
    dw = b[:, :2].copy().view(np.float16).astype(np.float64)[:, 0]
    nib = np.concatenate([b[:, 2:] & 15, b[:, 2:] >> 4], axis=1).astype(np.int64) - 8
    q, d = R.quantize_act(x[None])
    isum = (nib * q.reshape(8, 32).astype(np.int64)).sum(axis=1)
    want = float((isum * dw * d[0].astype(np.float64)).sum())
    mag = float(np.abs(isum * dw * d[0]).sum())
    assert abs(got - want) <= 10 * 2.0 ** -24 * mag
    # sensitivity of this check: one q off by one moves the sum by at least |nib| * dw * d of that block
    assert (np.abs(nib).max(axis=1) * np.abs(dw) * d[0]).min() > 100 * 2.0 ** -24 * mag


def test_perm_is_a_bijection_with_the_lane_group_property():
    k = np.arange(256)
    p = R.q8_perm(k)
    assert sorted(p[:64].tolist()) == list(range(64)) and np.array_equal(p[64:128], p[:64] + 64)
    assert np.array_equal(R.q8_perm_inv(p), k)
    for g in range(4):  # lane group g's 16 bytes: k 8g..8g+7 then 32+8g..32+8g+7
        assert R.q8_perm_inv(np.arange(16 * g, 16 * g + 16)).tolist() == list(range(8 * g, 8 * g + 8)) + list(range(32 + 8 * g, 40 + 8 * g))
    rows = np.random.default_rng(2).integers(-128, 128, size=(3, 192)).astype(np.int8)
    assert np.array_equal(R.unperm_rows(R.perm_rows(rows)), rows)
    assert R.perm_rows(rows)[1, 16 * 2 + 8 + 3] == rows[1, 32 + 8 * 2 + 3]


@pytest.mark.parametrize("N,K", [(16, 64), (96, 192)])
def test_tile_layouts_round_trip_and_address(N, K):
    rng = np.random.default_rng(N + K)
    dbits = rng.integers(0, 0x7C00, size=(N, K // 32)).astype(np.uint16)
    q = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
    nib = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
    p8, p4 = R.pack_q8_tiles(dbits, q), R.pack_q4_tiles(dbits, nib)
    assert p8.size == N // 16 * (K // 64) * 1088 and p4.size == N // 16 * (K // 64) * 576
    d2, q2 = R.unpack_q8_tiles(p8, N, K)
    assert np.array_equal(d2, dbits) and np.array_equal(q2, q)
    d3, n3 = R.unpack_q4_tiles(p4, N, K)
    assert np.array_equal(d3, dbits) and np.array_equal(n3, nib)
    # direct addressing of single elements, from the sentences of kernels.h
    for row, k in [(0, 0), (N - 1, K - 1), (N - 11, 37), (5, K - 40)]:
        nt, r, kt, half, g, j = row // 16, row % 16, k // 64, (k % 64) // 32, (k % 32) // 8, k % 8
        t8 = p8[(nt * (K // 64) + kt) * 1088:][:1088]
        assert t8[16 * (r + 16 * g) + 8 * half + j] == q[row, k].view(np.uint8)
        sc = t8[1024 + 16 * (r // 4) + 8 * half + 2 * (r % 4):][:2]
        assert int(sc[0]) | (int(sc[1]) << 8) == dbits[row, k // 32]
        t4 = p4[(nt * (K // 64) + kt) * 576:][:576]
        byte = t4[8 * (r + 16 * g) + 4 * half + j % 4]
        assert (byte >> 4 if j >= 4 else byte & 15) == nib[row, k]
        sc = t4[512 + 16 * (r // 4) + 8 * half + 2 * (r % 4):][:2]
        assert int(sc[0]) | (int(sc[1]) << 8) == dbits[row, k // 32]


def test_blocks_dequant_and_gate_up():
    rng = np.random.default_rng(5)
    N, K = 32, 64
    d = (2.0 ** rng.integers(-6, -3, size=(N, 2))).astype(np.float16)
    q = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
    b = R.q8_blocks(d.view(np.uint16), q)
    assert b.shape == (N, 68) and b[3, 34:36].view(np.float16)[0] == d[3, 1] and b[3, 36].view(np.int8) == q[3, 32]
    nib = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
    b4 = R.q4_blocks(d.view(np.uint16), nib)
    assert b4.shape == (N, 36) and b4[2, 18 + 2 + 5] == nib[2, 32 + 5] | (nib[2, 32 + 21] << 4)
    tiles = R.dequant_q8_bf16_tiles(d.view(np.uint16), q)
    vals = L.bf16_f32(L.unpack_tiles(tiles, N, K))
    assert np.array_equal(vals, L.bf16_round(np.repeat(d.astype(np.float32), 32, axis=1) * q.astype(np.float32)))
    gu = R.gate_up(np.arange(32)[:, None])
    assert gu[:, 0].tolist() == list(range(8)) + list(range(16, 24)) + list(range(8, 16)) + list(range(24, 32))


def test_rms_scale_and_block_matmul():
    x = np.ones((2, 64), np.float32)
    x[1] *= 2
    assert R.rms_scale(x, 0.0).tolist() == [1.0, 0.5]
    assert R.rms_scale(x, 0.0, +1)[0] == np.nextafter(np.float32(1), np.float32(2))
    rng = np.random.default_rng(6)
    y = rng.standard_normal((4, 256)).astype(np.float32)
    s64 = 1 / np.sqrt((y.astype(np.float64) ** 2).mean(axis=1) + 1e-5)
    assert (np.abs(R.rms_scale(y, 1e-5) - s64) <= 4 * 2.0 ** -24 * s64).all()
    wq = rng.integers(-128, 128, size=(8, 128))
    xq = rng.integers(-127, 128, size=(3, 128))
    dw, dx = 2.0 ** rng.integers(-3, 0, size=(8, 4)), 2.0 ** rng.integers(-5, -2, size=(3, 4))
    tot, mag = R.scaled_block_sum(wq, dw, xq, dx)
    deq = (xq * np.repeat(dx, 32, axis=1)) @ (wq * np.repeat(dw, 32, axis=1)).T
    assert np.array_equal(tot, deq) and (mag >= np.abs(tot)).all()
    (b0, isum), = list(R.block_isums(wq, xq))
    assert b0 == 0 and isum.shape == (3, 8, 4) and isum[2, 5, 1] == int((wq[5, 32:64] * xq[2, 32:64]).sum())


def test_plan_of_llama3_8b_shapes():
    """mx_q8_matmul_plan (no GPU) for the Llama-3-8B matrices, worked out by hand from the launchers' conditions as
    they stood before they were moved into mq8_plan: the dispatch the whole-model tests run must not move."""
    from llama_p2p_amd import engine

    F32, RESID, QKV, SWIGLU = 0, 1, 2, 3
    plan = engine.q8_matmul_plan

    def has(p, **want):
        assert {k: p[k] for k in want} == want, p

    # one token, quantise on load with norm: gate/up 1792 tiles = 256 groups of 7; q|k|v 384 tiles: Q4_0 only
    has(plan(SWIGLU, 1, 28672, 4096, on_load=True, norm=True), kind="pers_ql", tpw=7)
    has(plan(SWIGLU, 1, 28672, 4096, wq4=True, on_load=True, norm=True), kind="pers_ql", tpw=7)
    has(plan(QKV, 1, 6144, 4096, on_load=True, norm=True), kind="ql", qp=2, qm=1, bd=1)
    has(plan(QKV, 1, 6144, 4096, wq4=True, on_load=True, norm=True), kind="pers_ql", tpw=2)
    has(plan(SWIGLU, 2, 28672, 4096, on_load=True, norm=True), kind="ql", qp=2, qm=2, bd=0)
    # ffn_down: K 14336 = 224 tiles, 28 per wave = 1792 k: 8 float4 per lane; 3 tokens in the 4-slot image
    has(plan(RESID, 3, 4096, 14336, on_load=True), kind="ql", qp=8, qm=4, bd=0)
    has(plan(F32, 4, 128256, 4096, on_load=True, norm=True), kind="ql", qp=2, qm=4)
    assert plan(F32, 5, 128256, 4096, on_load=True, norm=True)["kind"] == "none"
    # pre-quantised rows
    has(plan(RESID, 16, 4096, 4096), kind="mq8", ks=8, rt=1, nb=1, bd=0, slab_ks=-1)
    has(plan(SWIGLU, 32, 28672, 4096), kind="wide", w=7)            # 1792 = 7 x 256
    has(plan(SWIGLU, 32, 28672, 4096, wq4=True), kind="wsw", w=7)
    has(plan(F32, 17, 128256, 4096), kind="wide", w=8)              # 8016 tiles: not 7 x, 8 x 1002
    has(plan(RESID, 32, 4096, 4096), kind="mq8", ks=8, rt=1, nb=2, slab_ks=4)
    has(plan(RESID, 32, 4096, 14336), kind="mq8", slab_ks=4)
    has(plan(QKV, 32, 6144, 4096), kind="mq8", ks=8, rt=2, nb=2, slab_ks=2)
    has(plan(QKV, 64, 6144, 4096), kind="mq8", ks=8, rt=1, nb=4, grid_y=1, slab_ks=-1)
    has(plan(RESID, 256, 4096, 4096), kind="mq8", nb=4, grid_y=4)   # 16 x 2 = 32 work-groups: below QG_MIN_GRID
    has(plan(SWIGLU, 256, 28672, 4096), kind="gemm", grid=224)
    has(plan(RESID, 4096, 4096, 14336), kind="gemm", grid=512)
