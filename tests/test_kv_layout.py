"""tests/kv_layout.py against the layout sentence of DESIGN.md §3 (CPU only), and the probe's binding."""
import numpy as np
import pytest

import kv_layout as L


def offsets(tiler, S, D):
    """offs[p][d] = where element (p, d) lands in the tiled region."""
    idx = np.arange(S * D, dtype=np.int64).reshape(S, D)
    flat = tiler(idx)
    offs = np.empty(S * D, dtype=np.int64)
    offs[flat] = np.arange(S * D)
    return flat, offs.reshape(S, D)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [64, 128, 512])
def test_tilers_are_bijections(S, D):
    for tiler in (L.tile_k, L.tile_v):
        flat, _ = offsets(tiler, S, D)
        assert flat.shape == (S * D,)
        assert np.array_equal(np.sort(flat), np.arange(S * D))


@pytest.mark.parametrize("D", [64, 128])
def test_k_tiles_hold_16_positions_by_32_dims(D):
    S = 128
    _, offs = offsets(L.tile_k, S, D)
    for pt in range(S // 16):
        for dt in range(D // 32):
            blk = offs[16 * pt:16 * pt + 16, 32 * dt:32 * dt + 32]
            t = pt * (D // 32) + dt  # position-major tile order
            assert np.array_equal(np.sort(blk.ravel()), np.arange(512 * t, 512 * t + 512))
            p, d = np.meshgrid(np.arange(16), np.arange(32), indexing="ij")
            lane, elem = (blk - 512 * t) // 8, (blk - 512 * t) % 8
            assert np.array_equal(lane, p + 16 * (d // 8)) and np.array_equal(elem, d % 8)


@pytest.mark.parametrize("D", [64, 128])
def test_v_tiles_hold_32_positions_by_16_dims(D):
    S = 128
    _, offs = offsets(L.tile_v, S, D)
    for pt in range(S // 32):
        for dt in range(D // 16):
            blk = offs[32 * pt:32 * pt + 32, 16 * dt:16 * dt + 16]
            t = pt * (D // 16) + dt
            assert np.array_equal(np.sort(blk.ravel()), np.arange(512 * t, 512 * t + 512))
            p, d = np.meshgrid(np.arange(32), np.arange(16), indexing="ij")
            lane, elem = (blk - 512 * t) // 8, (blk - 512 * t) % 8
            assert np.array_equal(lane, d + 16 * (p // 8)) and np.array_equal(elem, p % 8)


def test_hand_computed_entries():
    # (tile index * 64 + lane) * 8 + element, worked out by hand from the sentence
    _, k64 = offsets(L.tile_k, 64, 64)
    assert k64[0, 0] == 0
    assert k64[15, 31] == (0 * 64 + 63) * 8 + 7  # last lane, last element of tile (0, 0)
    assert k64[0, 32] == 512  # tile (0, 1) follows tile (0, 0)
    assert k64[16, 0] == 2 * 512  # tile (1, 0) = third tile when D / 32 = 2
    assert k64[3, 9] == (0 * 64 + 3 + 16 * 1) * 8 + 1
    _, k128 = offsets(L.tile_k, 64, 128)
    assert k128[37, 77] == ((2 * 4 + 2) * 64 + 5 + 16 * 1) * 8 + 5 == 5293
    _, v64 = offsets(L.tile_v, 64, 64)
    assert v64[0, 0] == 0
    assert v64[31, 15] == (0 * 64 + 63) * 8 + 7
    assert v64[0, 16] == 512  # tile (0, 1)
    assert v64[32, 0] == 4 * 512  # tile (1, 0) = fifth tile when D / 16 = 4
    assert v64[8, 0] == (0 * 64 + 16) * 8 + 0  # position group 1 -> lane 16
    assert v64[9, 3] == (0 * 64 + 3 + 16 * 1) * 8 + 1
    _, v128 = offsets(L.tile_v, 64, 128)
    assert v128[37, 77] == ((1 * 8 + 4) * 64 + 13 + 16 * 0) * 8 + 5 == 6253


@pytest.mark.parametrize("D", [64, 128])
def test_round_trip_with_leading_axes(D):
    rng = np.random.default_rng(D)
    x = rng.standard_normal((3, 2, 128, D)).astype(np.float16)
    for tile, untile in ((L.tile_k, L.untile_k), (L.tile_v, L.untile_v)):
        flat = tile(x)
        assert flat.shape == (3, 2, 128 * D)
        assert np.array_equal(untile(flat, D), x)
        assert np.array_equal(tile(x[1, 0]), flat[1, 0])  # leading axes are independent regions
        assert np.array_equal(tile(untile(flat, D)), flat)


def test_ref_attention_small_cases():
    D = 64
    K = np.zeros((64, D), np.float16)
    V = np.zeros((64, D), np.float16)
    V[:, 0] = np.arange(64)
    K[10:] = np.nan  # past pos: never touched
    V[10:] = np.nan
    out, A, spread = L.ref_attention(np.zeros(D, np.float32), K, V, 9, 0.125)
    assert abs(out[0] - 4.5) < 1e-12 and abs(A[0] - 4.5) < 1e-12 and spread == 0 and out[1] == 0
    # pos beyond n_ctx attends keys [0, n_ctx)
    out2, _, _ = L.ref_attention(np.zeros(D, np.float32), K, V, 10, 0.125, n_ctx=10)
    assert np.array_equal(out, out2)
    # one dominant key; q is rounded to f16 (1 + 2^-12 -> 1)
    K[:10] = 0
    K[3, 5] = 32
    q = np.zeros((2, D), np.float32)
    q[0, 5], q[1, 5] = 16 * (1 + 2.0 ** -12), -16
    out, A, spread = L.ref_attention(q, K, V, 9, 0.125)
    assert spread[0] == 64.0 and abs(out[0, 0] - 3.0) < 1e-20 + 9 * np.exp(-64) * 9
    assert abs(out[1, 0] - (45 - 3) / 9) < 1e-12  # the -64 key drops out, the other 9 weigh equally


def test_engine_binding_declares_the_probe():
    from llama_p2p_amd import engine as E

    assert "mx_attention_probe" in E.EXPORTS and hasattr(E.lib(), "mx_attention_probe")
    assert E.KV_POS_ALIGN == L.KV_POS_ALIGN
