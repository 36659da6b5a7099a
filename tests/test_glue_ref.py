"""tests/glue_ref.py pinned on the host: bf16_rne against torch's CPU conversion, ssq16_emul against the float64 sums,
argmax_ref on hand-made rows, what the block builders promise (on the inputs alone), and the refusals of
mx_glue_probe that need no GPU."""
import numpy as np
import pytest
import torch

import glue_ref as G
import mm_layout as L
from llama_p2p_amd import gguf


def torch_bf16_bits(u):
    f = torch.from_numpy(np.ascontiguousarray(u, dtype=np.uint32).view(np.float32).copy())
    return f.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_specials_cover_the_classes():
    s = G.SPECIALS
    assert s.size == 393216 and len(np.unique(s)) == s.size
    for u in (0x7F800001, 0x7F808000, 0x7FFF8000, 0x7FFFFFFF, 0xFFFFFFFF,   # the NaNs f2bf's carry loses
              0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x00000001, 0x807FFFFF,  # inf, overflow to inf, denormals
              0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001):  # tie to even, tie to odd, just below, just above
        assert u in s


def test_bf16_rne_equals_torch_on_every_non_nan():
    rng = np.random.default_rng(0)
    for u in (G.SPECIALS, rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)):
        keep = u[~G.is_nan_bits32(u)]
        assert keep.size > 0.98 * u.size
        got, want = G.bf16_rne(keep), torch_bf16_bits(keep)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"f32 {keep[bad[0]]:#010x}: {got[bad[0]]:#06x}, torch {want[bad[0]]:#06x}"
    # f32 arrays and uint32 bit patterns are the same input
    assert np.array_equal(G.bf16_rne(G.SPECIALS.view(np.float32)), G.bf16_rne(G.SPECIALS))


def test_bf16_rne_keeps_a_nan():
    u = G.SPECIALS[G.is_nan_bits32(G.SPECIALS)]
    assert u.size == 2 * 127 * 6 + 2 * 5  # exponent all ones: 127 upper halves with payload x 6, and 0x7F80 x 5, per sign
    got = G.bf16_rne(u)
    assert np.array_equal(got, ((u >> 16) | 0x40).astype(np.uint16))
    assert G.is_nan_bits16(got).all()
    for x, want in ((0x7F800001, 0x7FC0), (0x7F808000, 0x7FC0), (0x7FFF8000, 0x7FFF), (0x7FFFFFFF, 0x7FFF),
                    (0xFFFFFFFF, 0xFFFF), (0xFF800001, 0xFFC0)):
        assert G.bf16_rne(np.array([x], dtype=np.uint32))[0] == want
    # the formula without the NaN branch (f2bf, synth.f32_to_bf16_bits) loses exactly the classes the issue names
    plain = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert not G.is_nan_bits16(plain).all()


def test_ssq16_emul_against_float64():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((64, 8192)) * np.exp2(rng.integers(-8, 9, size=(64, 8192)))).astype(np.float32)
    got, want = G.ssq16_emul(x).astype(np.float64), L.ssq16_ref(x)
    assert got.shape == (64, 512)
    assert (np.abs(got - want) <= 2.0 ** -22 * want).all()
    # integers times 2^-e: exact, in any order
    xi = (rng.integers(-8, 9, size=(17, 4160)) * np.exp2(-rng.integers(0, 4, size=(17, 1)))).astype(np.float32)
    assert np.array_equal(G.ssq16_emul(xi).astype(np.float64), L.ssq16_ref(xi))
    # the order matters: a sum whose groups round differently when taken ((g0 + g1) + g2) + g3
    y = np.zeros((1, 16), np.float32)
    # g0 = 2^53, g1 = 2^29 (an f32 tie that rounds down), g2 = g3 = 1: (g2 + g3) = 2 lifts the sum over the tie,
    # while 1 and 1 added one after the other are each lost in double (ulp 2) and the tie rounds to even
    y[0, 0] = y[0, 1] = 2.0 ** 26
    y[0, 4] = y[0, 5] = 2.0 ** 14
    y[0, 8] = y[0, 12] = 1.0
    assert G.ssq16_emul(y)[0, 0] == np.float32(2.0 ** 53 + 2.0 ** 30)
    g = [2.0 ** 53, 2.0 ** 29, 1.0, 1.0]
    assert np.float32(((g[0] + g[1]) + g[2]) + g[3]) == np.float32(2.0 ** 53)


def test_argmax_ref_rules():
    nan, inf = float("nan"), float("inf")
    assert G.argmax_ref(np.array([1, 3, 2], np.float32), 3) == 1
    assert G.argmax_ref(np.array([1, 3, 3, 9], np.float32), 3) == 1      # ties -> lowest id; V bounds the row
    assert G.argmax_ref(np.array([-0.0, 0.0], np.float32), 2) == 0 and G.argmax_ref(np.array([0.0, -0.0], np.float32), 2) == 0
    assert G.argmax_ref(np.array([-inf, -inf], np.float32), 2) == 0
    assert G.argmax_ref(np.array([nan, nan], np.float32), 2) == 0
    assert G.argmax_ref(np.array([nan, nan, -5, nan], np.float32), 4) == 2
    assert G.argmax_ref(np.array([nan, inf, nan], np.float32), 3) == 1
    assert G.argmax_ref(np.array([nan, -inf], np.float32), 2) == 1       # -inf is a value, NaN is not


@pytest.mark.parametrize("t", G.QUANT, ids=[G.TNAME[t] for t in G.QUANT])
def test_builders_make_what_they_promise(t):
    be, bb = G.BLOCKS[t]
    assert gguf.BLOCKS[t] == (be, bb)
    a = G.blocks_case(t, "random", 4099)
    d = a[:, G.D_OFF[t]:G.D_OFF[t] + 2].copy().view(np.uint16)[:, 0]
    assert np.isfinite(d.view(np.float16)).all() and len(np.unique(d & 0x3FF)) > 900  # full mantissas, not one constant
    e = G.blocks_edges(t)
    de = e[:, G.D_OFF[t]:G.D_OFF[t] + 2].copy().view(np.uint16)[:, 0]
    assert set(G.D_EDGES.tolist()) <= set(de.tolist())
    if t == G.Q4_0:
        assert {0x00, 0xFF} <= set(e[:, 2:].reshape(-1).tolist())
    elif t == G.Q8_0:
        assert {0x80, 0x7F} <= set(e[:, 2:].reshape(-1).tolist())
    elif t in (G.Q4_K, G.Q5_K):
        s, m = gguf._scale_min_k4(e[:, 4:16])
        for j in range(8):  # both packings (j < 4, j >= 4), both fields, both ends
            assert {0, 63} <= set(s[:, j].tolist()) and {0, 63} <= set(m[:, j].tolist())
        rs, rm = np.random.default_rng(5).integers(0, 64, size=(2, 50, 8))
        assert [x.tolist() for x in gguf._scale_min_k4(G.pack_scales_k4(rs, rm))] == [rs.tolist(), rm.tolist()]
        assert set(G.D_EDGES.tolist()) <= set(e[:, 2:4].copy().view(np.uint16)[:, 0].tolist())  # dmin too
    else:
        sc = e[:, 192:208].view(np.int8)
        for j in range(16):
            assert {-128, 127} <= set(sc[:, j].tolist())
    dd = G.blocks_case(t, "distinct_d", 4099)
    dbits = dd[:, G.D_OFF[t]:G.D_OFF[t] + 2].copy().view(np.uint16)[:, 0]
    assert len(np.unique(dbits)) == 4099 and np.isfinite(dbits.view(np.float16)).all()
    # the decoder reads every builder's blocks without a complaint, and the one-hot blocks differ in one element
    for case in G.CASES:
        if G.has_case(t, case):
            y = gguf.dequantize(t, G.blocks_case(t, case, 257), (257, be))
            assert y.shape == (257, be) and y.dtype == np.float32


@pytest.mark.parametrize("t", [G.Q4_K, G.Q5_K, G.Q6_K], ids=["q4k", "q5k", "q6k"])
def test_one_hot_covers_every_position(t):
    pos = G.one_hot_positions(t)
    b = G.blocks_one_hot(t)
    nqh = {G.Q4_K: 0, G.Q5_K: 32, G.Q6_K: 64}[t]
    assert {(i, k) for f, _, i, k, _ in pos if f == "qh"} == {(i, k) for i in range(nqh) for k in range(8)}
    assert {(i, k) for f, _, i, k, _ in pos if f != "qh"} == {(i, k) for i in range(128) for k in range(2)}
    y = gguf.dequantize(t, b, (len(b), 256))
    base = -32.0 if t == G.Q6_K else 0.0
    hit = y != base
    assert (hit.sum(axis=1) == 1).all()          # one element per block answers
    where = hit.argmax(axis=1)
    what = y[np.arange(len(b)), where]
    for f in ("qh", "qs", "ql"):  # within a field no two positions give the same answer (Q6_K's qh: two bits, 16 and
        rows = [r for r, p in enumerate(pos) if p[0] == f]  # 32, per element; a nibble: one element each)
        assert len(set(zip(where[rows].tolist(), what[rows].tolist()))) == len(rows)
        if f != "qh" or t == G.Q5_K:
            assert len(set(where[rows].tolist())) == len(rows)


@pytest.mark.parametrize("t", [G.Q4_K, G.Q5_K], ids=["q4k", "q5k"])
def test_k4_product_is_exact_so_a_fused_multiply_subtract_cannot_show(t):
    """One would want case (a) to make the fused value f32(double(d1) q - double(m1)) differ from the two-rounding
    value in a good share of the elements, so that a contracted multiply-subtract in the kernel could not pass.  No
    valid block can do that: d is an f16 (11 significant bits), sc < 64 (6
    bits), q < 32 (5 bits), so d1 = d sc and d1 q hold at most 22 significant bits and are exact in f32; the only
    rounding is the subtraction's, which a fused multiply-subtract performs on the same exact value.  (Q6_K: 11 + 8 +
    6 bits with |sc| = 128 a power of two, at most 24; Q4_0 / Q8_0: 11 + 8.)  What is asserted here, on the inputs
    alone, is that fact: fused and unfused agree bit for bit on every element of cases (a) and (b) -- contraction in
    dequant_bf16_kernel is an equivalent mutant, reported as such in tests/test_glue_kernel_gpu.py."""
    for case in ("random", "edges"):
        blocks = G.blocks_case(t, case, 4099)
        d1, m1, q = G.k4_terms(t, blocks)
        with np.errstate(invalid="ignore", over="ignore"):
            prod = d1[:, :, None] * q
            two = prod - m1[:, :, None]
            fused = (d1.astype(np.float64)[:, :, None] * q.astype(np.float64) - m1.astype(np.float64)[:, :, None]).astype(np.float32)
            ref = gguf.dequantize(t, blocks, (4099, 256))
        fin = np.isfinite(two)
        assert fin.mean() > 0.5
        assert np.array_equal(prod.astype(np.float64)[fin], (d1.astype(np.float64)[:, :, None] * q.astype(np.float64))[fin])
        assert np.array_equal(two.view(np.uint32)[fin], fused.view(np.uint32)[fin])
        # k4_terms is the decoder's own arithmetic: sub-block s of a block is elements [32 s, 32 s + 32)
        assert np.array_equal(two.reshape(4099, 256).view(np.uint32)[fin.reshape(4099, 256)],
                              ref.view(np.uint32)[fin.reshape(4099, 256)])


# ---- mx_glue_probe: the refusals that are decided before any device call -------------------------------------------
@pytest.fixture(scope="module")
def E():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def refused(E, fn, *a, **kw):
    with pytest.raises(E.MxError) as err:
        fn(*a, **kw)
    assert err.value.code == E.MX_ERR_ARG and "mx_glue_probe" in str(err.value)


def test_probe_is_exported_and_refuses(E):
    assert "mx_glue_probe" in E.EXPORTS and hasattr(E.lib(), "mx_glue_probe")
    x = np.zeros((4, 128), np.float32)
    h = np.zeros((4, 128), np.uint16)
    for mode, src in ((1, h), (2, x), (3, x), (4, h)):
        kw = {"ids": [0, 1]} if mode == 1 else {}
        refused(E, E.glue_rows_probe, mode, src, n=96, **kw)      # n % 64
        refused(E, E.glue_rows_probe, mode, src, n=0, **kw)
        refused(E, E.glue_rows_probe, mode, src, M=0, **kw)
        refused(E, E.glue_rows_probe, mode, src, M=4097, **kw)
    refused(E, E.glue_rows_probe, 1, h, ids=[0, 4])                 # an id outside the table
    refused(E, E.glue_rows_probe, 1, h, ids=[-1])
    for mode in (5, 6):
        refused(E, E.glue_flat_probe, mode, np.zeros(8, np.float32), 6)   # n % 4
        refused(E, E.glue_flat_probe, mode, np.zeros(8, np.float32), 0)
    refused(E, E.glue_flat_probe, 0, np.zeros(18, np.uint8), 64, type=G.Q4_0)  # fewer bytes than 64 elements
    lg = np.zeros((2, 32), np.float32)
    refused(E, E.argmax_probe, lg, 32, [0, 0], [0, 0], 4, 4, M=0)
    refused(E, E.argmax_probe, lg, 0, [0, 0], [0, 0], 4, 4)
    refused(E, E.argmax_probe, lg, 33, [0, 0], [0, 0], 4, 4)         # ldl < V
    refused(E, E.argmax_probe, lg, 32, [0, 0], [0, 0], 4, 5)         # max_hist > hist_stride: a write past the row
    refused(E, E.argmax_probe, lg, 32, [0, 0], [0, -1], 4, 4)        # a negative count: a write before the row
