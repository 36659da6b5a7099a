"""The dequantise-at-load, residual-stream boundary and greedy-pick kernels alone (dequant_bf16_kernel, embed_kernel,
ssq_kernel, f32_in_kernel, bf16_to_f32_kernel, f32_to_bf16_kernel, f32_copy_kernel, argmax_stage1 + argmax_stage2)
through mx_glue_probe, which calls the production launchers -- no model, no engine.

Every comparison is bitwise on the uint16 / uint32 views, against tests/glue_ref.py (pinned on the host by
tests/test_glue_ref.py): bf16_rne(gguf.dequantize(...)), the widened or copied source bits, ssq16_emul, argmax_ref.
One exception: where the reference is a NaN that arithmetic made (inf * 0, NaN * q from an infinite or NaN d) only
NaN-ness is asserted -- the sign and payload of a generated NaN differ between x86 and the GPU.  NaNs that come from
F32 / F16 source bits are pinned exactly ((u >> 16) | 0x40; hardware quieting sets the same bit).  Every test checks
that the guard behind each output is still all-ones bits; "nothing left unwritten" is part of the bitwise comparison
(a legitimate output can itself be 0xFFFF: the bf16 of the f32 NaN 0xFFFFxxxx, so the poison is not searched for).

Branches and the case that reaches each:
  dequant_bf16_kernel F32 / F16 ........ test_dequant_f32_specials (393 216 patterns), test_dequant_f16_all (65 536:
                                         subnormals, both infinities, every NaN)
  Q4_0, Q8_0, Q4_K, Q5_K, Q6_K ......... test_dequant_blocks[type-case]: random / edges / one_hot / distinct_d at
                                         1, 255, 256, 257, 4099 blocks (one thread, a ragged and a full work-group)
  scale_min_k4 j < 4 and j >= 4 ........ the edges case: scale and min 0 and 63 in each of the 8 sub-blocks
  Q5_K qh bit 2g / 2g + 1, Q6_K qh
  pairs and the sc index l/16 + 2i ..... the one_hot case (Q6_K's scales are all 1 there) and the edges case (one
                                         scale at -128 / 127 among random others)
  the grid-stride second pass .......... test_dequant_stride (8192 * 256 + 257 Q4_0 blocks), test_flat[stride]
                                         (f32_to_bf16 / f32_copy: 1024 * 256 + 259 float4)
  launch_dequant_bf16's refusals ....... test_dequant_refusals (types 30, 3, 15; a count that is no block multiple)
  embed / f32_in / bf16_to_f32 / ssq:
  one tile per thread, 4 threads with
  two, every thread with two ........... test_rows[mode-n-M], n 64 (4 tiles), 4160 (260), 8192 (512)
  ssq requested / not requested ........ test_rows (pattern inputs: ssq withheld, the buffer returns all-ones)
  ssq16's summation shape .............. test_rows (order tiles, glue_ref.order_tile, in the first and last tile)
  f2bf_nan's NaN branch ................ test_dequant_f32_specials, test_dequant_f16_all, test_flat[specials] (mode 5)
  argmax: chunks of per = ceil(V / 64),
  empty chunks, lanes / waves / the
  256 stride / chunks in ties .......... test_argmax[V-pad]: V 1 .. 128256 (per 1 .. 2004), M 1, 3, 64
  stage 2's writes, NULL pointers,
  history full ......................... test_argmax (state checked on every call), test_argmax_null_pointers

Measured on MI355X: the 107 tests of this file take 3.1 s together (1.5 s of it loading the library); the slowest,
test_dequant_f32_specials, 0.24 s; test_dequant_stride (38 MB in, 134 MB out) 0.10 s.

Mutations tried on scratch copies (none committed), each run against this file, with the first test that failed:
  Q5_K's 2 << (2g) taken as 1 << (2g) -> test_dequant_blocks[q5k-random] (1 block: element 32 = g 0, high half, l 0);
  Q6_K's scale index without + 2 * i -> test_dequant_blocks[q6k-random] (block 0 element 32: i = 1);
  scale_min_k4's j >= 4 branch taking q[j] for q[j - 4] -> test_dequant_blocks[q4k-random] (block 0 element 128: the
    first element of sub-block 4);
  dequant_bf16_kernel's loop replaced by a single pass -> test_dequant_stride (block 2 097 152, the first of the
    second pass, still 0xFFFF);
  f32_to_bf16_kernel's loop replaced by a single pass -> test_flat[f32_to_bf16-stride] (element 1 048 576);
  bf16_to_f32_kernel writing ssq[... + (t & 255)] -> test_rows[bf16_to_f32-4160-1] (tiles 0-3 overwritten by tiles
    256-259, which stay unwritten);
  ssq16 summed as ((g0 + g1) + g2) + g3 -> test_rows[embed-64-1] (the order tile: 0x5a000000 for 0x5a000001; no
    random tile in this file tells the two orders apart);
  better's i < bi taken as i > bi -> test_argmax[2-ldl=V] ("tie 0 = 1" gives 1);
  per computed with floor division -> test_argmax[2-ldl=V] (per = 0: nothing is read, "max at 1" gives 0; at V
    16385 the last element is never read);
  argmax_stage2 without the n < max_hist test -> test_argmax[1-ldl=V] (row 2, count 5 = max_hist: slot 5 of the
    slack written);
  f2bf_nan taken back to f2bf -> test_dequant_f32_specials (12 of SPECIALS' NaNs stop being NaN: 0x7f800001,
    0x7f807fff, 0x7f808000 -> +inf, 0x7fff8000, 0x7fff8001, 0x7fffffff -> -0, 0xff800001 ... -> -inf, 0xffffxxxx ->
    +0); run without -x, also test_dequant_f16_all (F16 0x7fff -> f32 0x7fffe000 -> -0), test_flat[f32_to_bf16-specials]
    (the same 12 classes) and every other test_flat[f32_to_bf16-*] (their inputs carry members of SPECIALS): 12 of the
    107 tests fail;
  the fp contract(off) pragma removed from dequant_bf16_kernel: every test passes, and no test can fail -- an
    equivalent mutant.  d (f16, 11 significant bits) times a 6-bit scale times a 5-bit value holds at most 22 bits, so
    d1 q is exact in f32 and a fused multiply-subtract rounds the same exact difference once (Q6_K: 11 + 8 + 6 bits
    with -128 a power of two, at most 24; Q4_0 / Q8_0: 19).  tests/test_glue_ref.py asserts that fact on the inputs;
    the pragma stays as a statement of intent.
"""
import functools

import numpy as np
import pytest

import glue_ref as G
import test_matmul_kernel_gpu as B
from llama_p2p_amd import gguf
from test_matmul_kernel_gpu import all_ones

pytestmark = pytest.mark.gpu

NBLOCKS = [1, 255, 256, 257, 4099]
ROW_N = [64, 4160, 8192]
ROW_M = [1, 17, 64]
ROW_MODE = {1: "embed", 2: "ssq", 3: "f32_in", 4: "bf16_to_f32"}


class StopOnHipError(B.StopOnHipError):
    def glue_flat_probe(self, *a, **kw):
        return self._call(self._e.glue_flat_probe, *a, **kw)

    def glue_rows_probe(self, *a, **kw):
        return self._call(self._e.glue_rows_probe, *a, **kw)

    def argmax_probe(self, *a, **kw):
        return self._call(self._e.argmax_probe, *a, **kw)


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return StopOnHipError(engine)


def same_bits(got, want, what, name=None):
    """Bitwise equality of two integer views; a failure names the first element and both bit patterns."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        where = name(i) if name else f"element {i}"
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {where}: got {int(got[i]):#x}, "
                             f"want {int(want[i]):#x}")


# ---- mode 0: dequantise at load ---------------------------------------------------------------------------------------
def check_dequant(got, guard, ref, what, arithmetic_nan, name=None):
    """got uint16 against bf16_rne(ref f32).  arithmetic_nan: where ref is a NaN only NaN-ness is asserted."""
    assert all_ones(guard), f"{what}: wrote past the output"
    want = G.bf16_rne(ref.reshape(-1))
    if arithmetic_nan:
        nan = np.isnan(ref.reshape(-1))
        assert G.is_nan_bits16(got[nan]).all(), f"{what}: a NaN of the reference is not a NaN on the device"
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    same_bits(got, want, what, name)


def nan_classes(u, got):
    """The source patterns (hex) of the NaNs that did not stay NaN, for the failure message."""
    lost = G.is_nan_bits32(u) & ~G.is_nan_bits16(got)
    return ", ".join(f"{int(x):#010x}->{int(g):#06x}" for x, g in list(zip(u[lost], got[lost]))[:8]), int(lost.sum())


def test_dequant_f32_specials(mx):
    u = G.SPECIALS
    got, guard = mx.glue_flat_probe(0, u, u.size, type=G.F32)
    names, lost = nan_classes(u, got)
    assert lost == 0, f"F32 at load: {lost} NaN patterns stopped being NaN: {names}"
    check_dequant(got, guard, gguf.dequantize(G.F32, u.view(np.float32), (u.size,)), "F32 SPECIALS", False,
                  lambda i: f"f32 {int(u[i]):#010x}")


def test_dequant_f16_all(mx):
    h = np.arange(65536, dtype=np.uint16)
    got, guard = mx.glue_flat_probe(0, h, h.size, type=G.F16)
    ref = gguf.dequantize(G.F16, h.view(np.float16), (h.size,))
    sub = (h & 0x7C00) == 0
    assert ((got[sub & ((h & 0x3FF) != 0)] & 0x7FFF) != 0).all(), "an F16 subnormal was flushed to zero"
    assert G.is_nan_bits16(got[np.isnan(ref)]).all(), "an F16 NaN stopped being NaN"
    check_dequant(got, guard, ref, "F16, every pattern", False, lambda i: f"f16 {i:#06x}")


@functools.lru_cache(maxsize=None)
def dequant_ref(t, case):
    """(blocks uint8 [4099][bb], f32 [4099][be]) of a case, decoded once: the smaller counts are its leading blocks."""
    blocks = G.blocks_case(t, case, NBLOCKS[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        ref = gguf.dequantize(t, blocks, (NBLOCKS[-1], G.BLOCKS[t][0]))
    ref.setflags(write=False)
    return blocks, ref


@pytest.mark.parametrize("t,case", [(t, c) for t in G.QUANT for c in G.CASES if G.has_case(t, c)],
                         ids=[f"{G.TNAME[t]}-{c}" for t in G.QUANT for c in G.CASES if G.has_case(t, c)])
def test_dequant_blocks(mx, t, case):
    be = G.BLOCKS[t][0]
    blocks, ref = dequant_ref(t, case)
    pos = G.one_hot_positions(t) if case == "one_hot" else None

    def name(i):
        b, e = divmod(i, be)
        s = f"block {b} element {e}"
        if be == 256:
            s += f" (g {e // 64}, half {e // 32 % 2}, l {e % 32})"
        if pos:
            f, _, byte, k, _ = pos[b % len(pos)]
            s += f"; the block's only set field is {f}[{byte}] bit/nibble {k}"
        return s

    for nb in NBLOCKS:
        got, guard = mx.glue_flat_probe(0, blocks[:nb], nb * be, type=t)
        check_dequant(got, guard, ref[:nb], f"{G.TNAME[t]} {case} {nb} blocks", True, name)


def test_dequant_stride(mx):
    """More blocks than fill_grid's 8192 x 256 threads: the grid-stride second pass, with a ragged end.  The blocks
    tile a 4099-block pattern (4099 is prime: a second-pass block never sits on its first-pass pattern index)."""
    t, nb = G.Q4_0, 8192 * 256 + 257
    pat = np.concatenate([G.blocks_case(t, "edges", 99), G.blocks_case(t, "distinct_d", 2000),
                          G.blocks_case(t, "random", 2000)])
    assert len(pat) == 4099
    with np.errstate(invalid="ignore", over="ignore"):
        ref = gguf.dequantize(t, pat, (4099, 32))
    idx = np.arange(nb) % 4099
    got, guard = mx.glue_flat_probe(0, pat[idx], nb * 32, type=t)
    assert all_ones(guard), "Q4_0 stride: wrote past the output"
    want, nan = G.bf16_rne(ref)[idx].reshape(-1), np.isnan(ref)[idx].reshape(-1)  # tiled from the one decoding
    assert G.is_nan_bits16(got[nan]).all()
    got[nan] = want[nan]
    same_bits(got, want, "Q4_0 stride", lambda i: f"block {i // 32} (pattern {i // 32 % 4099}) element {i % 32}")


def test_dequant_refusals(mx):
    src = np.zeros(4096, np.uint8)
    for t, count in ((30, 256), (3, 256), (15, 256), (G.Q4_0, 48), (G.Q6_K, 384), (G.F32, 31)):
        with pytest.raises(mx.MxError) as err:
            mx.glue_flat_probe(0, src, count, type=t)
        assert err.value.code == mx.MX_ERR_ARG and "launch_dequant_bf16 refused" in str(err.value), str(err.value)


# ---- modes 1-4: the residual-stream boundary ------------------------------------------------------------------------
def pattern16(rows, n, salt=0):
    """bf16 bits that encode (row, col): distinct along a row, between tiles 256 apart and between rows; finite."""
    r, c = np.indices((rows, n), dtype=np.uint32)
    h = ((r + salt) * 40503 + c * 7 + (c >> 4)) & 0xFFFF
    return np.where((h & 0x7F80) == 0x7F80, h ^ 0x4000, h).astype(np.uint16)


def pattern32(rows, n):
    r, c = np.indices((rows, n), dtype=np.uint32)
    u = (r * np.uint32(2654435761) + c * np.uint32(40503) + (c >> 4)).astype(np.uint32)
    return np.where((u & 0x7F800000) == 0x7F800000, u ^ 0x40000000, u).astype(np.uint32)


def ssq_inputs(rows, n, bf16, seed):
    """Two f32 [rows][n] sets: small integers times 2^-e (any summation order is exact), and random full-mantissa
    values with glue_ref.order_tile() as the first tile of row 0 and the last tile of the last row (bf16: values
    with 8 significant bits, exact in both formats)."""
    rng = np.random.default_rng(seed)
    ints = (rng.integers(-8, 9, size=(rows, n)) * np.exp2(-rng.integers(0, 4, size=(rows, 1)))).astype(np.float32)
    rnd = (rng.uniform(1.0, 2.0, size=(rows, n)) * np.exp2(rng.integers(-8, 9, size=(rows, n))) *
           rng.choice([-1.0, 1.0], size=(rows, n))).astype(np.float32)
    if bf16:
        rnd = (rnd.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    rnd[0, :16] = G.order_tile()
    rnd[-1, -16:] = G.order_tile()
    return ints, rnd


def tile_name(n):
    return lambda i: f"row {i // (n // 16)} tile {i % (n // 16)}"


@pytest.mark.parametrize("M", ROW_M)
@pytest.mark.parametrize("n", ROW_N)
@pytest.mark.parametrize("mode", sorted(ROW_MODE), ids=[ROW_MODE[m] for m in sorted(ROW_MODE)])
def test_rows(mx, mode, n, M):
    bf16, what = mode in (1, 4), f"{ROW_MODE[mode]} M={M} n={n}"
    N = 97  # the embedding table's rows
    ids = (np.arange(M) * 37 + 5) % N
    ids[0], ids[-1] = N - 1, 0
    if M > 2:
        ids[1], ids[2] = 0, N - 1  # repeats
    srows = N if mode == 1 else M

    def run(src_f32_or_bits, want_ssq):
        kw = {"ids": ids} if mode == 1 else {}
        return mx.glue_rows_probe(mode, src_f32_or_bits, want_ssq=want_ssq, **kw)

    def rows_of(a):
        return a[ids] if mode == 1 else a

    # x: bit patterns that name their (row, col); the partials are withheld and the buffer must come back untouched
    if mode != 2:
        bits = pattern16(srows, n) if bf16 else pattern32(srows, n)
        x, xg, ssq, sg = run(bits if bf16 else bits.view(np.float32), False)
        want = rows_of(bits).astype(np.uint32) << (16 if bf16 else 0)
        same_bits(x, want, what + " x", lambda i: f"row {i // n} col {i % n}")
        assert all_ones(xg), what + ": wrote past x"
        assert all_ones(ssq) and all_ones(sg), what + ": ssq written though not requested"
    # ssq: exact integers, then full mantissas against the emulation of ssq16
    for k, vals in enumerate(ssq_inputs(srows, n, bf16, 7 * n + M + mode)):
        src = (vals.view(np.uint32) >> 16).astype(np.uint16) if bf16 else vals
        x, xg, ssq, sg = run(src, True)
        v = rows_of(vals)
        if mode != 2:
            same_bits(x, v.view(np.uint32), f"{what} x (ssq set {k})", lambda i: f"row {i // n} col {i % n}")
            assert all_ones(xg), what + ": wrote past x"
        assert all_ones(sg), what + ": wrote past ssq"
        emul = G.ssq16_emul(v)
        if k == 0:
            exact = (v.astype(np.float64) ** 2).reshape(M, -1, 16).sum(axis=-1)
            assert np.array_equal(emul.astype(np.float64), exact)
        same_bits(ssq, emul.view(np.uint32), f"{what} ssq (set {k})", tile_name(n))


def test_bf16_to_f32_every_pattern(mx):
    h = np.arange(65536, dtype=np.uint16).reshape(16, 4096)
    x, xg, ssq, sg = mx.glue_rows_probe(4, h, want_ssq=False)
    same_bits(x, h.astype(np.uint32) << 16, "bf16_to_f32, every pattern", lambda i: f"bf16 {i:#06x}")
    assert all_ones(xg) and all_ones(ssq) and all_ones(sg)


# ---- modes 5 / 6: the flat hand-off ------------------------------------------------------------------------------
def flat_input(name):
    if name == "specials":
        return G.SPECIALS
    rng = np.random.default_rng(len(name))
    count = 4 * (1024 * 256 + 259) if name == "stride" else int(name)
    u = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    u[::1001] = G.SPECIALS[rng.integers(0, G.SPECIALS.size, size=len(u[::1001]))]
    return u


@pytest.mark.parametrize("name", ["specials", "stride"] + sorted({str(M * n) for M in ROW_M for n in ROW_N}, key=int))
@pytest.mark.parametrize("mode", [5, 6], ids=["f32_to_bf16", "f32_copy"])
def test_flat(mx, mode, name):
    u = flat_input(name)
    got, guard = mx.glue_flat_probe(mode, u.view(np.float32), u.size)
    what = f"{'f32_to_bf16' if mode == 5 else 'f32_copy'} {name} ({u.size} floats)"
    assert all_ones(guard), what + ": wrote past the output"
    if mode == 5:
        names, lost = nan_classes(u, got)
        assert lost == 0, f"{what}: {lost} NaN patterns stopped being NaN: {names}"
    same_bits(got, G.bf16_rne(u) if mode == 5 else u, what, lambda i: f"element {i}, f32 {int(u[i]):#010x}")


# ---- mode 7: the greedy pick ----------------------------------------------------------------------------------------
ARGMAX_V = [1, 2, 63, 64, 65, 255, 16384, 16385, 32000, 128256]
MAX_HIST, HIST_STRIDE = 5, 8


@functools.lru_cache(maxsize=None)
def argmax_rows(V):
    """([name], f32 [rows][V], expected ids by argmax_ref) -- the catalogue of rows for a vocabulary of V."""
    rng = np.random.default_rng(V)
    per = -(-V // 64)
    nan, inf = np.float32("nan"), np.float32("inf")
    names, rows = [], []

    def add(name, row):
        names.append(name)
        rows.append(row.astype(np.float32))

    def base():
        return rng.uniform(-1.0, 1.0, size=V).astype(np.float32)

    for p in sorted({0, per - 1, min(per, V - 1), V - 1, (V - 1) // per * per}):  # a unique maximum
        r = base()
        r[p] = 2.0
        add(f"max at {p}", r)
    pairs = {(0, 1), (1, 256), (63, 64), (255, 256), (0, 256), (per - 1, per), (per, per + 1), (V - 2, V - 1),
             ((V - 1) // per * per - 1, (V - 1) // per * per), (per + 63, per + 64), (per + 255, per + 256)}
    for i, j in sorted(p for p in pairs if 0 <= p[0] < p[1] < V):  # equal maxima: the lower id wins
        r = base()
        r[i] = r[j] = 2.0
        add(f"tie {i} = {j}", r)
    add("all equal", np.full(V, 1.5))
    add("all -inf", np.full(V, -inf))
    add("all NaN", np.full(V, nan))
    if V >= 2:
        k = V // 2 if V > 2 else 0
        for a, b, nm in ((-0.0, 0.0, "-0 before +0"), (0.0, -0.0, "+0 before -0")):
            r = -1.0 - base() ** 2
            r[k], r[k + 1] = a, b
            add(nm, r)
        r = np.full(V, nan)
        r[V - 1 - k] = -3.0
        add("NaN but one", r)
        for a, b, nm in ((nan, inf, "NaN then +inf"), (inf, nan, "+inf then NaN")):
            r = base()
            r[k], r[k + 1] = a, b
            add(nm, r)
    rows = np.stack(rows)
    want = np.array([G.argmax_ref(r, V) for r in rows], dtype=np.int32)
    rows.setflags(write=False)
    return names, rows, want


def run_argmax(mx, V, pad, pick, null_mask=0):
    """Rows `pick` of the catalogue in one call; checks tok, ids_next, pos_next, history, counts, slack and guards."""
    names, rows, want = argmax_rows(V)
    M, ldl = len(pick), V + pad
    lg = np.full((M, ldl), np.inf, dtype=np.float32)  # the padding past V would win if it were read
    lg[:, :V] = rows[pick]
    pos = (np.arange(M) * 7 + 3).astype(np.int32)
    hc = np.array([(0, MAX_HIST - 1, MAX_HIST, 2)[(i + len(pick)) % 4] for i in range(M)], dtype=np.int32)
    r = mx.argmax_probe(lg, V, pos, hc, HIST_STRIDE, MAX_HIST, null_mask=null_mask)
    what = f"V={V} ldl={ldl} M={M} null_mask={null_mask}"
    tok = want[pick]
    label = lambda i: f"row {i} ({names[pick[i]]})"
    untouched = np.full(M, -1, dtype=np.int32)
    same_bits(r.tok, untouched if null_mask & 1 else tok, what + " tok_out", label)
    same_bits(r.ids_next, untouched if null_mask & 2 else tok, what + " ids_next", label)
    same_bits(r.pos_next, pos if null_mask & 4 else pos + 1, what + " pos_next", label)
    hist = np.full((M, HIST_STRIDE), -1, dtype=np.int32)  # slack past max_hist stays all-ones
    if not null_mask & 8:
        for i in range(M):
            if hc[i] < MAX_HIST:
                hist[i, hc[i]] = tok[i]
    same_bits(r.hist, hist, what + " hist", lambda i: f"row {i // HIST_STRIDE} slot {i % HIST_STRIDE}")
    same_bits(r.hist_count, hc if null_mask & 8 else hc + 1, what + " hist_count", label)
    for g in (r.tok_guard, r.ids_next_guard, r.pos_next_guard, r.hist_count_guard, r.hist_guard):
        assert all_ones(g), what + ": wrote past an output"
    return r


@pytest.mark.parametrize("pad", [0, 16], ids=["ldl=V", "ldl=V+16"])
@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax(mx, V, pad):
    names, rows, want = argmax_rows(V)
    n = len(names)
    assert n <= 64
    run_argmax(mx, V, pad, [i % n for i in range(64)])          # M 64: the whole catalogue
    for i in range(n):                                          # M 1: every row alone gives the same id
        run_argmax(mx, V, pad, [i])
    for i in range(0, n, 3):                                    # M 3
        run_argmax(mx, V, pad, [(i + k) % n for k in range(3)])


@pytest.mark.parametrize("null_mask", [1, 2, 4, 8, 14, 15])
def test_argmax_null_pointers(mx, null_mask):
    """Each optional pointer NULL in turn; 14: the engine's own call for a first token (tok_out only)."""
    for V in (65, 16385):
        run_argmax(mx, V, 16, [0, 1, 2], null_mask=null_mask)
