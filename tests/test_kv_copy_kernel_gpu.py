"""kv_copy_kernel through mx_kv_copy_probe -- no model (prefix sharing).

The caches are built here in logical order [layer][slot][kv head][position][d] and tiled in numpy with
tests/kv_layout.py (written from the layout sentence of DESIGN.md §3, not from the device's offset functions);
the expectation is made the same way: in logical order, positions [0, P) of each destination become the
source's, P = n_pos rounded up to 32, and the result is tiled.  Every element is a 16-bit pattern of its own
(cache, layer, slot, head, position, d), so a word taken from or written to any other place shows.  The
comparison is bitwise over the whole of both caches: positions >= P of a destination, every other slot and the
sources must come back as they went in.

One launch per case: 16 slots, slots 0..3 each feed three destinations (4..15), the twelve destinations take the
twelve n_pos values {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, n_ctx - 1, n_ctx}.  Cases: D in {64, 128} x
n_head_kv in {1, 2, 8} x n_layer in {1, 3} x n_ctx in {100 (ctx_stride 128), 512}.
"""
import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

N_SLOTS = 16
CASES = [(D, H, NL, C) for D in (64, 128) for H in (1, 2, 8) for NL in (1, 3) for C in (100, 512)]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def logical(cache, n_layer, n_slots, H, S, D):
    """uint16 [layer][slot][head][pos][d]: pos * D + d is unique within a region (S * D <= 2^16); the other
    terms shift regions against each other, so no two slots, heads, layers or caches agree at one (pos, d)."""
    pd = (np.arange(S, dtype=np.uint32)[:, None] * D + np.arange(D, dtype=np.uint32)[None, :])
    lay = np.arange(n_layer, dtype=np.uint32)[:, None, None, None, None] * 3307
    slot = np.arange(n_slots, dtype=np.uint32)[None, :, None, None, None] * 977
    head = np.arange(H, dtype=np.uint32)[None, None, :, None, None] * 5573
    return ((pd[None, None, None] + lay + slot + head + 29 * cache) & 0xFFFF).astype(np.uint16)


def table(n_ctx):
    n_pos = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, n_ctx - 1, n_ctx]
    return [(i % 4, 4 + i, n) for i, n in enumerate(n_pos)]


def expected(x, copies, S):
    y = x.copy()
    for s, d, n in copies:
        P = min((n + 31) // 32 * 32, S)
        y[:, d, :, :P, :] = x[:, s, :, :P, :]
    return y


@pytest.mark.parametrize("D,H,NL,n_ctx", CASES, ids=[f"D{D}-kv{H}-L{NL}-ctx{C}" for D, H, NL, C in CASES])
def test_copy_moves_the_prefix_and_nothing_else(mx, D, H, NL, n_ctx):
    S = L.ctx_stride(n_ctx)
    copies = table(n_ctx)
    k, v = logical(0, NL, N_SLOTS, H, S, D), logical(1, NL, N_SLOTS, H, S, D)
    kt, vt = L.tile_k(k).reshape(-1), L.tile_v(v).reshape(-1)
    ko, vo = mx.kv_copy_probe(NL, N_SLOTS, H, D, n_ctx, copies, kt, vt)
    ke, ve = L.tile_k(expected(k, copies, S)).reshape(-1), L.tile_v(expected(v, copies, S)).reshape(-1)
    assert not np.array_equal(ke, kt) and not np.array_equal(ve, vt)  # the table does move something
    for name, got, exp in (("K", ko, ke), ("V", vo, ve)):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{name}: {bad.size} elements differ, first at flat index {bad[0]}"


REFUSED = {
    "src == dst": [(1, 1, 5)],
    "src below range": [(-1, 1, 5)],
    "src above range": [(4, 1, 5)],
    "dst below range": [(0, -1, 5)],
    "dst above range": [(0, 4, 5)],
    "n_pos 0": [(0, 1, 0)],
    "n_pos negative": [(0, 1, -3)],
    "n_pos above n_ctx": [(0, 1, 101)],
    "a destination twice": [(0, 1, 5), (2, 1, 5)],
    "a destination then a source": [(0, 1, 5), (1, 2, 5)],
    "a source then a destination": [(0, 1, 5), (2, 0, 5)],
    "a good copy before a bad one": [(0, 1, 40), (2, 2, 5)],
    "no copies": [],
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_tables_launch_nothing(mx, what):
    NL, n_slots, H, D, n_ctx = 2, 4, 2, 64, 100
    S = L.ctx_stride(n_ctx)
    kt = L.tile_k(logical(0, NL, n_slots, H, S, D)).reshape(-1)
    vt = L.tile_v(logical(1, NL, n_slots, H, S, D)).reshape(-1)
    k0, v0 = kt.copy(), vt.copy()
    with pytest.raises(mx.MxError) as ei:
        mx.kv_copy_probe(NL, n_slots, H, D, n_ctx, REFUSED[what], kt, vt, inplace=True)
    assert ei.value.code == mx.MX_ERR_ARG
    assert np.array_equal(kt, k0) and np.array_equal(vt, v0)
