"""grammar_mask_kernel alone (csrc/grammar.hip) through mx_grammar_mask_probe: the output equals
numpy's where(bit, x, -inf) bit for bit -- every vocabulary width around a mask word, a 16-byte group and a
work-group, rows that start on a 16-byte boundary and rows that do not (ldl = V + 7), guard columns, rows that are
off, and NaN / inf / -0.0 inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = [1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 4097, 128256]
KINDS = ["all_set", "all_clear", "bit0", "last", "alternating", "random"]
GUARD_BITS = 0xDEADBEEF


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def make_mask(kind, V, rng):
    nw = (V + 31) // 32
    if kind == "all_set":
        return np.full(nw, 0xFFFFFFFF, dtype=np.uint32)
    if kind == "all_clear":
        return np.zeros(nw, dtype=np.uint32)
    if kind == "alternating":
        return np.full(nw, 0x55555555, dtype=np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
    w = np.zeros(nw, dtype=np.uint32)
    t = 0 if kind == "bit0" else V - 1
    w[t >> 5] = np.uint32(1) << np.uint32(t & 31)
    return w


def make_rows(M, V, ldl, rng):
    x = rng.standard_normal((M, ldl)).astype(np.float32) * 8
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=np.float32)
    hit = rng.random((M, ldl)) < 0.1
    x[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    x[:, :min(V, 5)] = special[:min(V, 5)]  # the first columns hold every special value whatever the draw
    g = x[:, V:].view(np.uint32)
    g[:, 0::2] = 0x7FC00001  # a NaN with a payload
    g[:, 1::2] = GUARD_BITS
    return x


def expected(x, masks, on, V):
    bits = np.unpackbits(masks.view(np.uint8).reshape(len(masks), -1), axis=1, bitorder="little")[:, :V].astype(bool)
    out = x.copy()
    body = out[:, :V]
    body[...] = np.where(bits | (on == 0)[:, None], body, np.float32(-np.inf))
    return out


def check(mx, V, ldl, kinds, on, seed):
    rng = np.random.default_rng(seed)
    M = len(kinds)
    x = make_rows(M, V, ldl, rng)
    masks = np.stack([make_mask(k, V, rng) for k in kinds])
    on = np.asarray(on, dtype=np.uint32)
    got = mx.grammar_mask_probe(x, masks, on, V=V)
    want = expected(x, masks, on, V)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, (f"V {V} ldl {ldl} kinds {kinds[:6]} on {on[:6].tolist()}: {len(bad)} words differ, first "
                           f"(row, col) {bad[0].tolist()}: got {gb[tuple(bad[0])]:#x} want {wb[tuple(bad[0])]:#x}")
    # said once more for what must never change: guard columns, rows that are off, allowed columns
    assert (gb[:, V:] == x.view(np.uint32)[:, V:]).all()
    assert (gb[on == 0] == x.view(np.uint32)[on == 0]).all()


@pytest.mark.parametrize("V", VS)
def test_mask_kernel_bitwise(mx, V):
    for ldl in (V, V + 7):
        for i, k in enumerate(KINDS):  # M = 1: every mask alone, and once switched off
            check(mx, V, ldl, [k], [1], 10 + i)
        check(mx, V, ldl, ["random"], [0], 17)
        check(mx, V, ldl, KINDS[:3], [1, 1, 1], 20)  # M = 3
        check(mx, V, ldl, KINDS[3:], [1, 0, 1], 21)
        kinds = [KINDS[r % 6] for r in range(64)]  # M = 64: every mask on and off (garbage words in the off rows)
        on = [0 if (r // 6) % 2 else 1 + r for r in range(64)]
        check(mx, V, ldl, kinds, on, 22)


def test_probe_refuses_bad_shapes(mx):
    x = np.zeros((1, 8), dtype=np.float32)
    m = np.zeros((1, 1), dtype=np.uint32)
    with pytest.raises(mx.MxError):
        mx.grammar_mask_probe(np.zeros((65, 8), dtype=np.float32), np.zeros((65, 1), dtype=np.uint32), np.ones(65), V=8)
    with pytest.raises(mx.MxError):
        mx._check(mx.lib().mx_grammar_mask_probe(0, x.ctypes.data, 1, 9, 8, m.ctypes.data, m.ctypes.data, x.ctypes.data))
    with pytest.raises(ValueError):
        mx.grammar_mask_probe(x, np.zeros((1, 2), dtype=np.uint32), np.ones(1), V=8)
