"""kv_pack_kernel / kv_unpack_kernel through mx_kv_pack_probe -- no model (host-RAM tier).

The caches are random 16-bit patterns (NaNs and infinities included) in logical order [layer][slot][kv head]
[position][d], tiled in numpy with tests/kv_layout.py; the packed expectation comes from tests/kv_pack_ref.py
(the layout sentence: packed[t][layer][K|V][kv head][32 * D], each block the region's bytes of positions
[32t, 32t + 32)).  Every comparison is bitwise and covers everything the call returns: the whole packed buffer
with its gaps and its guard, and the whole of both caches.

One launch per case and direction: nine entries, one per n_pos of {1, 31, 32, 33, 63, 64, 65, n_ctx - 1, n_ctx}.
Cases: D in {64, 128} x n_head_kv in {1, 2, 8} x n_layer in {1, 3} x n_ctx in {100 (ctx_stride 128), 512}.
"""
import numpy as np
import pytest

import kv_layout as L
import kv_pack_ref as P

pytestmark = pytest.mark.gpu

N_SLOTS = 10
CASES = [(D, H, NL, C) for D in (64, 128) for H in (1, 2, 8) for NL in (1, 3) for C in (100, 512)]
IDS = [f"D{D}-kv{H}-L{NL}-ctx{C}" for D, H, NL, C in CASES]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def n_pos_list(n_ctx):
    return [1, 31, 32, 33, 63, 64, 65, n_ctx - 1, n_ctx]


_caches = {}


def caches(D, H, NL, n_ctx, n_slots=N_SLOTS):
    """Logical k, v and their tiled flat forms, made once per geometry and never modified."""
    key = (D, H, NL, n_ctx, n_slots)
    if key not in _caches:
        S = L.ctx_stride(n_ctx)
        rng = np.random.default_rng(hash(key) & 0xFFFF)
        k = rng.integers(0, 1 << 16, (NL, n_slots, H, S, D), dtype=np.uint16)
        v = rng.integers(0, 1 << 16, (NL, n_slots, H, S, D), dtype=np.uint16)
        k[0, 0, 0, :4, :4] = [[0x7E00, 0xFE00, 0x7C00, 0xFC01]] * 4  # NaN / inf patterns, whatever the draw gave
        kt, vt = L.tile_k(k).reshape(-1), L.tile_v(v).reshape(-1)
        for a in (k, v, kt, vt):
            a.setflags(write=False)
        _caches[key] = (k, v, kt, vt)
    return _caches[key]


def differ(name, got, exp):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{name}: {bad.size} elements differ, first at flat index {bad[0]}"


@pytest.mark.parametrize("D,H,NL,n_ctx", CASES, ids=IDS)
def test_pack(mx, D, H, NL, n_ctx):
    k, v, kt, vt = caches(D, H, NL, n_ctx)
    tw = P.tile_words(NL, H, D)
    entries, off, exp = [], 0, []
    for slot, n in enumerate(n_pos_list(n_ctx)):  # back to back, slot i at n_pos i
        entries.append((slot, n, off))
        e = P.pack_entry(k, v, slot, n)
        exp.append(e)
        off += e.size // 8
    nbytes = off * 16
    assert off % tw == 0
    got, ko, vo = mx.kv_pack_probe(0, NL, N_SLOTS, H, D, n_ctx, entries, kt, vt, packed_bytes=nbytes)
    differ("packed", got[:nbytes].view(np.uint16), np.concatenate(exp))
    assert got.size == nbytes + mx.KV_PACK_GUARD_BYTES and (got[nbytes:] == 0xFF).all(), "the guard was written"
    differ("K", ko, kt)
    differ("V", vo, vt)


@pytest.mark.parametrize("D,H,NL,n_ctx", CASES, ids=IDS)
def test_unpack_prefixes_of_longer_entries(mx, D, H, NL, n_ctx):
    """The packed buffer holds nine whole-slot entries (of slots 1..9, 0); entry i gives only its first
    ceil32(n_pos_i) positions to slot i: nothing at or past that position may change."""
    k, v, kt, vt = caches(D, H, NL, n_ctx)
    S = L.ctx_stride(n_ctx)
    whole = [P.pack_entry(k, v, (i + 1) % N_SLOTS, n_ctx) for i in range(9)]
    assert all(w.size == whole[0].size for w in whole)
    packed = np.concatenate(whole).view(np.uint8)
    entries = [(i, n, i * (whole[0].size // 8)) for i, n in enumerate(n_pos_list(n_ctx))]
    ko, vo = mx.kv_pack_probe(1, NL, N_SLOTS, H, D, n_ctx, entries, kt, vt, packed=packed)
    ke, ve = k.copy(), v.copy()
    for dst, n, _ in entries:
        Pn = min(P.ceil32(n), S)
        ke[:, dst, :, :Pn] = k[:, (dst + 1) % N_SLOTS, :, :Pn]
        ve[:, dst, :, :Pn] = v[:, (dst + 1) % N_SLOTS, :, :Pn]
    assert not np.array_equal(ke, k)
    differ("K", ko, L.tile_k(ke).reshape(-1))
    differ("V", vo, L.tile_v(ve).reshape(-1))


def test_three_entries_at_distinct_offsets(mx):
    D, H, NL, n_ctx = 64, 2, 3, 100
    k, v, kt, vt = caches(D, H, NL, n_ctx)
    tw = P.tile_words(NL, H, D)
    entries = [(7, 40, 5 * tw), (2, 100, 0), (7, 1, 9 * tw)]  # out of order, gaps between them, a slot read twice
    nbytes = 11 * tw * 16
    got, ko, vo = mx.kv_pack_probe(0, NL, N_SLOTS, H, D, n_ctx, entries, kt, vt, packed_bytes=nbytes)
    exp = np.full((nbytes + mx.KV_PACK_GUARD_BYTES) // 2, 0xFFFF, dtype=np.uint16)
    for slot, n, off in entries:
        e = P.pack_entry(k, v, slot, n)
        exp[off * 8:off * 8 + e.size] = e
    differ("packed, gaps and guard", got.view(np.uint16), exp)
    differ("K", ko, kt)
    differ("V", vo, vt)
    # ... and back, into three other slots, from the buffer the device wrote
    back = [(0, 40, 5 * tw), (1, 100, 0), (3, 1, 9 * tw)]
    ko, vo = mx.kv_pack_probe(1, NL, N_SLOTS, H, D, n_ctx, back, kt, vt, packed=got[:nbytes])
    ke, ve = k.copy(), v.copy()
    for (dst, n, _), (src, _, _) in zip(back, entries):
        Pn = P.ceil32(n)
        ke[:, dst, :, :Pn], ve[:, dst, :, :Pn] = k[:, src, :, :Pn], v[:, src, :, :Pn]
    differ("K", ko, L.tile_k(ke).reshape(-1))
    differ("V", vo, L.tile_v(ve).reshape(-1))


@pytest.mark.parametrize("D", [64, 128])
def test_pack_then_unpack_equals_the_device_copy(mx, D):
    H, NL, n_ctx = 2, 3, 100
    k, v, kt, vt = caches(D, H, NL, n_ctx)
    tw = P.tile_words(NL, H, D)
    moves = [(0, 4, 70), (1, 5, 1), (2, 6, 100)]
    table, off = [], 0
    for src, _, n in moves:
        table.append((src, n, off))
        off += P.ceil32(n) // 32 * tw
    packed, _, _ = mx.kv_pack_probe(0, NL, N_SLOTS, H, D, n_ctx, table, kt, vt, packed_bytes=off * 16)
    ko, vo = mx.kv_pack_probe(1, NL, N_SLOTS, H, D, n_ctx, [(dst, n, o) for (_, dst, n), (_, _, o) in zip(moves, table)],
                              kt, vt, packed=packed[:off * 16])
    kc, vc = mx.kv_copy_probe(NL, N_SLOTS, H, D, n_ctx, moves, kt, vt)
    assert not np.array_equal(kc, kt)
    differ("K", ko, kc)
    differ("V", vo, vc)


def refused(tw):
    good = (0, 40, 0)  # two tiles
    return {
        "slot below range": (None, [(-1, 5, 0)]),
        "slot above range": (None, [(4, 5, 0)]),
        "n_pos 0": (None, [(0, 0, 0)]),
        "n_pos negative": (None, [(0, -3, 0)]),
        "n_pos above n_ctx": (None, [(0, 101, 0)]),
        "an offset off a tile": (None, [(0, 5, 1)]),
        "an offset half a tile on": (None, [(0, 5, tw // 2)]),
        "an entry past the buffer": (None, [(0, 100, 5 * tw)]),  # four tiles from tile 5 of 8
        "an offset past the buffer": (None, [(0, 5, 8 * tw)]),
        "overlapping ranges": (None, [good, (1, 5, tw)]),
        "the same range twice": (None, [good, (1, 40, 0)]),
        "a good entry before a bad one": (None, [good, (1, 0, 4 * tw)]),
        "no entries": (None, []),
        "a slot a destination twice": (1, [good, (0, 5, 4 * tw)]),
    }


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("what", list(refused(8)))
def test_refused_tables_launch_nothing(mx, what, direction):
    NL, n_slots, H, D, n_ctx = 2, 4, 2, 64, 100
    k, v, kt, vt = caches(D, H, NL, n_ctx, n_slots)
    tw = P.tile_words(NL, H, D)
    only, entries = refused(tw)[what]
    nbytes = 8 * tw * 16
    kc, vc = kt.copy(), vt.copy()
    if direction == 0:
        packed = np.full(nbytes + mx.KV_PACK_GUARD_BYTES, 0x5A, dtype=np.uint8)
    else:
        packed = np.random.default_rng(3).integers(0, 256, nbytes, dtype=np.uint8)
    p0 = packed.copy()

    def call():
        return mx.kv_pack_probe(direction, NL, n_slots, H, D, n_ctx, entries, kc, vc, packed=packed,
                                packed_bytes=nbytes, inplace=True)

    if only is not None and only != direction:  # packing may read a slot twice
        call()
        assert np.array_equal(kc, kt) and np.array_equal(vc, vt)
        return
    with pytest.raises(mx.MxError) as ei:
        call()
    assert ei.value.code == mx.MX_ERR_ARG
    assert np.array_equal(kc, kt) and np.array_equal(vc, vt) and np.array_equal(packed, p0)
