"""The K-quant kernels alone (mkq_kernel in its block-diagonal, ring, quantise-on-load and two-column-tile forms,
mkq_bd_tile_kernel, mkq_pers_kernel, mkq_pers_seg_kernel, mkq_wide_kernel with its EPI_SLAB split-K form,
mkq_wide_seg_kernel, q8k_kernel, pack_kq_kernel, dequant_kq_kernel, embed_kq_kernel) against exact integer
references, through mx_kq_matmul_probe / mx_kq_side_probe -- no model.

Why bitwise: a K-quant x Q8_K product is a sum over super-blocks of exact int32 S and Mn, each times d d_x or
dmin d_x.  Here d and dmin are 2^j (at most 3 consecutive exponents per matrix) and every activation super-block
holds integers in a small range times 2^-e (at most 3 consecutive e per case) with exactly one element +-127 2^-e, so
the device's quantiser returns d_x = -+2^-e and those integers (negated under a positive maximum; checked on the
returned xq / xd / xb), (d d_x) S and (dmin d_x) Mn are exact, and every partial sum is a multiple of the unit
2^(j_min - e_max) below 2^24 units (asserted in the builder from sum_s |terms| of the actual operands) -- exact in
f32 in ANY summation order.  Large K narrows the exponent spreads and the integer range (narrow()) to keep that
assertion.  The reference is the float64 product of tests/kq_ref.py (pinned to ggml's loops by tests/test_kq_ref.py).
Comparisons are by value (==): bit equality except for the sign of a zero, and a NaN (the probe's 0xFF poison in
outputs, slabs, xq / xd / xb rows >= M) never compares equal.

Branches and the case that reaches each (every case asserts its kernel through mx_kq_matmul_plan):
  mkq_kernel<8,1,1,BD> (M 1, pre-quantised), super-blocks per wave (SB w) / 8: K 256 (7 of 8 waves empty), 1792 (0 |
    1), 2048 (1), 2304 (1 | 2), 4096 (2), 4352 (2 | 3), 8192 (4), 8448 (4 | 5: ring of 2 with a tail), 16384 (8),
    16640 (8 | 9): U 1, 2, 4 and the 2-deep ring: test_exact_gemv.
  mkq_kernel<8,1,1> ring U 2 (M 2, 15, 16) and <8,1,2> U 1 (M 17, 31, 32 where the wide form refuses: 3 or 6 tiles;
    grid.y at M 33, 64, 65, 100): the same K list, N 48 / 96; N 16 and 304, and QKV at K 256 .. 8448:
    test_exact_gemv, test_exact_gemv_rows, test_exact_gemv_qkv, test_mixed_segments.
  launch_mkq_bd<QL>, every U: K 256 (U 1), 2304, 4096 (2), 4352, 8192 (4), 8448, 14336 (7), 16384 (8), with norm
    to 8192, RESID with ssq partials and F32 over three segment types: test_exact_on_load.
  mkq_bd_tile_kernel: SWIGLU <7,16,1> 2, 8, 14 tiles; <3,8,1> 2, 4, 768; F32 <8,16,4> 1, 32, 33, 40; <8,8,1> 1, 9;
    with and without norm: test_bd_tile.
  mkq_pers_seg_kernel: K 4096, N 256, q|k Q4_K + v Q6_K and Q4_K | Q5_K | Q6_K: test_qkv_pers.
  mkq_pers_kernel: SWIGLU 704 tiles / SB 8, F32 1025 / SB 8, SWIGLU 1792 / SB 16, F32 2049 / SB 16 (the last two
    Q4_K and Q6_K), M 1 (BD) and 2, 16 (ring): test_pers; quantising on load under MX_NO_KQ_BD_TILE=1 in one child
    process, the same bits as mkq_bd_tile_kernel on the same operands at the same tile counts: test_pers_on_load.
  mkq_wide_kernel (Q4_K: kq_compute_fold): W 4 at 4 and 12 tiles, SB 4, 8, 12; W 7 at 1400, W 8 at 1600 tiles
    (SB 4); M 17, 31, 32: test_exact_wide.
  launch_mkq_slab: N 64 ks 2 (K 2048, 2304: 4 + 5), 4 (4096, 4352: 4, 4, 4, 5), 8 (8192); N 256 (ks 8) and 4096 (ks
    4) folded by q8k_kernel<true,true>; N 8192 (ks 2) folded by launch_resid_norm; refusals K 1024, N 16384:
    test_exact_slab_resid, test_slab_refusals.
  launch_mkq_qkv_slab (mkq_wide_seg_kernel) through launch_qkv_finish: ks 4 (K 4096), 2 (2304), 1 (1024); refusal
    on a segment end that is no multiple of 4: test_exact_slab_qkv.
  q8k_kernel<false,false> / <true,false> / <true,true>: test_quantize_q8k, test_norm_q8k, test_norm_q8k_fold;
    ql_build: the on-load cases above.
  Unreachable in production: mkq_pers_kernel<QL> (shadowed by mkq_bd_tile_kernel for every shape it has, unless
  MX_NO_KQ_BD_TILE); launch_mkq_bd<false> with U 7 / 8 (pre-quantised slices above 4 ring 2 deep).

Measured on MI355X over all cases of this file (the tests print each case's figure):
  f32 SwiGLU (actf) worst relative error vs float64 ....... 1.92e-7 (asserted at the bf16 file's ACTF_BAR, 7.0e-7:
    the same epi_store<EPI_SWIGLU>)
  real scales: worst |err| / bound ........................ 0.086
  norm rows matching only a neighbouring f32 scale ........ 0 of 475

Mutations tried on scratch copies of kquant.hip (arithmetic and layout only, none committed), each run against this
file, with the first test that failed:
  kq_compute's Q5_K high-bit shift (2 j + 1) & 7 taken as (2 j) & 7 -> test_exact_gemv[q5k-0-256] (F32, M 2);
  kq_compute's Q6_K lane zeroing g < 2 taken as g < 1 -> test_exact_gemv[q6k-0-256] (F32, M 2);
  kq_load_w's mins dwords of sub-blocks g and g + 4 swapped -> test_exact_gemv[q4k-0-256] (F32, M 2);
  q8k_row's xb slot 2 (j & 3) + (j >> 2) taken as j -> test_exact_gemv[q4k-0-256] (the returned xb, M 1);
  q8k_row's first-maximum search run upwards (the last maximum of a lane wins) -> test_extremes[q4k] (every |x|
    equal, signs mixed: the returned xq);
  kq_compute_fold's S = Cl + 8 Ch taken as Cl + 4 Ch -> test_exact_wide[q4k-4x1024] (F32, M 17);
  mkq_body's ring tail loop stopping one super-block early -> test_exact_gemv[q4k-0-256] (M 2: K 256 is tail only);
  mkq_wide_body's K range taken from (blockIdx.y + 1) % gridDim.y, the slab still blockIdx.y: every test passes --
    each range keeps its own length, so the slabs are permuted and their sum is unchanged; which slab holds which
    range is not pinned by this file (an equivalent mutant, as in the Q8 file).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kq_ref as R
import mm_layout as L
import q8_ref as R8
import test_matmul_kernel_gpu as B
from test_matmul_kernel_gpu import ACTF_BAR, GEOM, N_CTX, all_ones, check_qkv, check_ssq, qkv_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, RESID, QKV, SWIGLU = 0, 1, 2, 3
EPI_NAME = B.EPI_NAME
TYPES = [12, 13, 14]
TNAME = {12: "q4k", 13: "q5k", 14: "q6k"}
JW0 = -8          # d, dmin = 2^-8 .. 2^-6: normal f16
MEASURED = {"actf": 0.0, "real": 0.0, "nudged": 0, "rows": 0}


class StopOnHipError(B.StopOnHipError):
    def kq_matmul_probe(self, *a, **kw):
        return self._call(self._e.kq_matmul_probe, *a, **kw)

    def kq_pack_probe(self, *a, **kw):
        return self._call(self._e.kq_pack_probe, *a, **kw)

    def kq_dequant_probe(self, *a, **kw):
        return self._call(self._e.kq_dequant_probe, *a, **kw)

    def kq_embed_probe(self, *a, **kw):
        return self._call(self._e.kq_embed_probe, *a, **kw)

    def q8k_probe(self, *a, **kw):
        return self._call(self._e.q8k_probe, *a, **kw)


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return StopOnHipError(engine)


def one(t, N):
    return ((t, N // 16),)


def plan_is(mx, epi, M, N, K, segs, on_load=False, norm=False, **want):
    p = mx.kq_matmul_plan(epi, M, N, K, list(segs), on_load=on_load, norm=norm)
    got = {k: p[k] for k in want}
    assert got == want, f"plan of {EPI_NAME[epi]} M={M} N={N} K={K} {segs}: {p}"
    return p


# ---- operands -------------------------------------------------------------------------------------------------------
def narrow(K, t):
    """(activation integer range, e spread, j spread) that keeps sum |terms| < 2^24 units: per super-block the one
    +-127 element alone contributes up to 127 x 31 x 63 units times 2^(j - j_min) 2^(e_max - e), so K above 2304
    (and Q6_K, whose int8 scales reach -128, at every K) takes two exponents each, K above 4352 smaller integers and
    K above 8448 one e.  Q6_K's scales are drawn from [-32, 32) with one group in 16 at -128 or 127 (wcase) for the
    same reason."""
    if K <= 2304 and t != 14:
        return 4, 3, 3
    return (4, 2, 2) if K <= 4352 else (2, 2, 2) if K <= 8448 else (1, 1, 2)


@functools.lru_cache(maxsize=6)
def wcase(N, K, t, seed=0):
    """(GGUF blocks uint8 [N][SB bb], fields): d, dmin = 2^j, random 6-bit scales / mins (Q6_K: int8 scales) and values;
    column n % 8 of the scales walks through the values whose low or high 3 bits are 0 or 7 (kq_compute_fold)."""
    rng = np.random.default_rng(1000 + N + K + t + seed)
    SB = K // 256
    js = narrow(K, t)[2]
    dbits = R.f16_bits(2.0 ** rng.integers(JW0, JW0 + js, size=(N, SB)))
    vals = rng.integers(0, R.VMAX[t] + 1, size=(N, K), dtype=np.uint8)
    if t == 14:
        sc = rng.integers(-32, 32, size=(N, SB, 16))
        n_i, s_i = np.indices((N, SB))
        sc[n_i, s_i, (n_i + 5 * s_i) % 16] = np.where((n_i + s_i) % 2, -128, 127)
        blocks = R.kq_blocks(t, dbits, vals, sc.astype(np.int8))
    else:
        sc = rng.integers(0, 64, size=(N, SB, 8), dtype=np.uint8)
        edge = np.array([0, 7, 56, 63, 8, 15, 57, 62], dtype=np.uint8)
        n_i, s_i = np.indices((N, SB))
        sc[n_i, s_i, n_i % 8] = edge[(n_i // 8 + s_i) % 8]
        blocks = R.kq_blocks(t, dbits, vals, sc, R.f16_bits(2.0 ** rng.integers(JW0, JW0 + js, size=(N, SB))),
                             rng.integers(0, 64, size=(N, SB, 8), dtype=np.uint8))
    f = R.kq_fields(t, blocks)
    blocks.setflags(write=False)
    return blocks, f


@functools.lru_cache(maxsize=4)
def xcase(K, rows, t):
    """(integers [rows][K], relative e [rows][SB]): integers in the narrow range, one +-127 per super-block."""
    rng = np.random.default_rng(2000 + K + rows)
    xr, es, _ = narrow(K, t)
    SB = K // 256
    xi = rng.integers(-xr, xr + 1, size=(rows, SB, 256)).astype(np.int16)
    at = rng.integers(0, 256, size=(rows, SB))
    r_i, b_i = np.indices((rows, SB))
    xi[r_i, b_i, at] = 127 * (1 - 2 * rng.integers(0, 2, size=(rows, SB)))
    xi[0, 0, at[0, 0]], xi[min(1, rows - 1), SB - 1, at[min(1, rows - 1), SB - 1]] = 127, -127  # both signs, always
    e = rng.integers(0, es, size=(rows, SB))
    xi = xi.reshape(rows, K)
    for a in (xi, e):
        a.setflags(write=False)
    return xi, e


def exact_product(segs, K, fields, xi, e):
    """float64 [M][N] product (d_x = 2^-e) over the row segments, asserted exact in f32 in any order; (s, j_min)."""
    out, jmin = [], 0
    for (t, _), f in zip(segs, fields):
        d = [f["d"]] + ([] if t == 14 else [f["dmin"]])
        jmin = min([jmin] + [int(np.log2(R.f16_f32(b).min())) for b in d])
    unit = 2.0 ** (jmin - int(e.max()))
    for (t, _), f in zip(segs, fields):
        N = f["d"].shape[0]
        step = max(16, (1 << 22) // K * 16)
        for n0 in range(0, N, step):  # row blocks of W: the float64 copies stay small
            g = {k: (v[n0:n0 + step] if v is not None else None) for k, v in f.items()}
            s, mag = R.product(t, g, xi, 2.0 ** -e.astype(np.float64))
            assert mag.max() / unit < 2 ** 24, f"partial sums could leave f32's exact range: 2^{np.log2(mag.max() / unit):.1f} units"
            out.append(s)
    return np.concatenate(out, axis=1), unit


@functools.lru_cache(maxsize=3)
def case(segs, K, rows, swiglu=False):
    """(blocks flat, fields per segment, xf f32 [rows][K], xi, e, s [rows][N] float64, unit).  e0 (the common
    exponent of the activations) puts the largest |output| at 32..64: SWIGLU's gate stays inside expf's range."""
    t0, parts, fields = 0, [], []
    for i, (t, te) in enumerate(segs):
        b, f = wcase(16 * (te - t0), K, t, seed=i)
        parts.append(b.reshape(-1))
        fields.append(f)
        t0 = te
    xi, er = xcase(K, rows, max(t for t, _ in segs))
    s_rel, unit_rel = exact_product(segs, K, fields, xi, er)
    peak = np.abs(s_rel[:, :s_rel.shape[1] // 2] if swiglu else s_rel).max()
    e0 = max(0, int(np.ceil(np.log2(max(peak, 1) / 64))))
    e = er + e0
    xf = (xi * np.repeat(2.0 ** -e, 256, axis=1)).astype(np.float32)
    s = s_rel * 2.0 ** -e0
    for a in (xf, s):
        a.setflags(write=False)
    return np.concatenate(parts), fields, xf, xi, e, s, unit_rel * 2.0 ** -e0


def device_rows(xi, e):
    """What quantize_row_q8_K makes of integers x 2^-e with one +-127 per super-block: iscale = -127 / max, so a
    positive maximum negates the integers and d: (q [M][K], d [M][SB])."""
    M, K = xi.shape
    b = xi.reshape(M, K // 256, 256)
    sign = -np.sign(np.take_along_axis(b, np.abs(b).argmax(axis=-1)[..., None], axis=-1)[..., 0])
    return (b * sign[..., None]).reshape(M, K), (sign * 2.0 ** -e).astype(np.float32)


def check_operand(r, xi, e, M, what):
    q, d = device_rows(xi[:M], e[:M])
    assert (d > 0).any() and (d < 0).any() or M * d.shape[1] < 2, f"{what}: both signs of the maximum"
    assert np.array_equal(R.unperm_rows(r.xq), q), f"{what}: the device's xq is not the intended integers"
    assert np.array_equal(r.xd, d), f"{what}: the device's xd"
    assert np.array_equal(r.xb, R.xb_rows(q.reshape(M, -1, 16).sum(axis=-1))), f"{what}: the device's xb"
    assert all_ones(r.xq_guard) and all_ones(r.xd_guard) and all_ones(r.xb_guard), f"{what}: xq / xd / xb rows >= M written"


def check_out(r, epi, s, M, N, what, qa=None, resid_i=None, unit=None):
    final = None
    if epi == F32:
        assert np.array_equal(r.out, s.astype(np.float32)), what
    elif epi == RESID:
        final = s + resid_i * unit
        assert np.abs(final).max() < 2 ** 24 * unit
        assert np.array_equal(r.out, final.astype(np.float32)), what
    elif epi == QKV:
        check_qkv(r, qa, s, what)
    else:
        F = N // 2
        g, u = s[:, :F], s[:, F:]
        assert np.abs(g).max() <= 80, what
        want = L.swiglu_ref(g, u)
        got = r.out.astype(np.float64)
        nz = want != 0
        assert (got[~nz] == 0).all(), what
        rel = float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()) if nz.any() else 0.0
        MEASURED["actf"] = max(MEASURED["actf"], rel)
        print(f"actf worst relative error: {what} {rel:.3e}; so far {MEASURED['actf']:.3e}")
        assert rel <= ACTF_BAR, what
    assert all_ones(r.guard), f"{what}: guard rows written"
    if r.ssq_guard is not None:
        assert all_ones(r.ssq_guard), f"{what}: ssq partials written for rows >= M"
    r.final = final
    return r


def resid_ints(M, N):
    return np.random.default_rng(3000 + M + N).integers(-16, 17, size=(M, N)).astype(np.int64)


def normed(xi_row, e_row):
    """RMS_NORM operands whose normalised row is exactly xi 2^-e: x = +-1 (mean square 1, scale 1.0f), w = |xi| 2^-e."""
    x = np.where(xi_row < 0, -1.0, 1.0).astype(np.float32)
    return x, (np.abs(xi_row) * np.repeat(2.0 ** -e_row, 256)).astype(np.float32)


def run_exact(mx, path, epi, segs, K, M, *, rows=32, rope="id", want_ssq=False, act=0, norm=False, ssq_in=False):
    """Rows of the shared integer case through path 0 / 1 / 2: act 0 pre-quantised by launch_quantize_q8k, act 2 one
    token quantised on load (norm: through RMS_NORM with an exact scale)."""
    N = 16 * segs[-1][1]
    blocks, fields, xf, xi, e, s, unit = case(segs, K, rows, epi == SWIGLU)
    s = s[:M]
    what = f"path {path} {'|'.join(TNAME[t] for t, _ in segs)} {EPI_NAME[epi]} M={M} N={N} K={K} act {act} norm {norm}"
    kw, qa, ri = dict(want_slabs=path >= 1), None, None
    if epi == RESID:
        ri = resid_ints(M, N)
        kw.update(resid=(ri * unit).astype(np.float32), want_ssq=want_ssq)
        if path == 1:
            kw["fold_w"] = np.ones(N, np.float32)
    if epi == QKV:
        qa = kw["qkv"] = qkv_args(M, GEOM[N], rope)
    x = xf[:M]
    if norm:
        assert M == 1
        x1, w = normed(xi[0], e[0])
        x, kw["norm_w"] = x1[None], w
        if ssq_in:
            kw["ssq_in"] = np.full(K // 16, 16.0, np.float32)
    r = mx.kq_matmul_probe(path, epi, blocks, x, list(segs), N=N, K=K, act=act, **kw)
    if act != 2:
        check_operand(r, xi, e, M, what)
    check_out(r, epi, s, M, N, what + (f" rope {rope}" if epi == QKV else ""), qa, ri, unit)
    if path >= 1:
        p = mx.kq_matmul_plan(epi, M, N, K, list(segs))
        ks = p["slab_ks"] if path == 1 else p["qkv_slab_ks"]
        assert r.split == ks and r.slabs.shape == (ks, M, N), f"{what}: split {r.split}, plan {ks}"
        assert not (r.slabs.view(np.uint32) == 0xFFFFFFFF).any(), f"{what}: slab element never written"
        assert np.array_equal(r.slabs.astype(np.float64).sum(axis=0), s), f"{what}: slabs do not sum to the product"
    return r


def per_wave(K):
    return (K // 256 + 7) // 8


def bd_u(K, ql):
    p = per_wave(K)
    return 1 if p <= 1 else 2 if p <= 2 else 4 if p <= 4 else 7 if ql and p <= 7 else 8 if ql and p <= 8 else 2


# ---- exact: mkq_kernel on pre-quantised rows ------------------------------------------------------------------------------
GEMV_K = [256, 1792, 2048, 2304, 4096, 4352, 8192, 8448, 16384, 16640]


@pytest.mark.parametrize("K", GEMV_K)
@pytest.mark.parametrize("epi", [F32, RESID, SWIGLU])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_gemv(mx, t, epi, K):
    N = 96 if epi == SWIGLU else 48  # 6 / 3 tiles: the wide form refuses (ntiles % 4), and so does SB % 4 at most K
    segs = one(t, N)
    for M in [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 100]:
        want = dict(kind="mkq", ks=8, nkw=per_wave(K), grid_x=N // 16)
        if M == 1:
            want.update(bd=1, ql=0, nb=1, u=bd_u(K, False))
        elif M <= 16:
            want.update(bd=0, nb=1, u=2, grid_y=1)
        else:
            want.update(bd=0, nb=2, u=1, grid_y=1 if M <= 32 else (M + 31) // 32)
        plan_is(mx, epi, M, N, K, segs, **want)
        r = run_exact(mx, 0, epi, segs, K, M, rows=100, want_ssq=epi == RESID)
        if epi == RESID:
            check_ssq(r, f"mkq RESID ssq M={M} K={K}")


@pytest.mark.parametrize("N", [16, 304])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_gemv_rows(mx, t, N):
    """One tile, and 19 tiles (a few hundred rows; 19 % 4: the wide form refuses), F32 and RESID, short and long K."""
    for K in (256, 2304, 8448):
        for M in (1, 2, 16, 17, 32, 33):
            for epi in (F32, RESID):
                plan_is(mx, epi, M, N, K, one(t, N), kind="mkq", grid_x=N // 16, nb=1 if M <= 16 else 2)
                run_exact(mx, 0, epi, one(t, N), K, M, rows=33)


@pytest.mark.parametrize("K", [256, 2304, 4352, 8448])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_gemv_qkv(mx, t, K):
    for M in [1, 5, 16, 17, 33, 100]:
        for rope in ("id", "quarter", "mixed"):
            plan_is(mx, QKV, M, 192, K, one(t, 192), kind="mkq", nb=1 if M <= 16 else 2)
            run_exact(mx, 0, QKV, one(t, 192), K, M, rows=100, rope=rope)


def test_mixed_segments(mx):
    """One tile each of Q4_K | Q5_K | Q6_K under F32 and q|k Q4_K + v Q6_K under QKV: the segment walk of mkq_kernel."""
    for K in (256, 2304):
        for M in (1, 2, 16, 17, 33):
            segs = ((12, 1), (13, 2), (14, 3))
            plan_is(mx, F32, M, 48, K, segs, kind="mkq", t=0)
            run_exact(mx, 0, F32, segs, K, M, rows=33)
            segs = ((12, 8), (14, 12))
            plan_is(mx, QKV, M, 192, K, segs, kind="mkq")
            run_exact(mx, 0, QKV, segs, K, M, rows=33, rope="mixed")


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_norm_rows(mx, t):
    """Rows through launch_rmsnorm_q8k (q8k_kernel<true, false>) with a row_map, then mkq_kernel: x = +-1 and
    w = |xi| 2^-e make the normalised rows exactly sign-flipped copies of one integer row."""
    N, K, M = 48, 2304, 3
    blocks, fields, _, xi, e, _, _ = case(one(t, N), K, 100)
    signs = np.where(np.random.default_rng(t).integers(0, 2, size=(5, K)) > 0, 1, -1)
    signs[:, np.abs(xi[0]) == 127] = 1  # the maximum keeps its sign: d_x as in the shared case
    _, w = normed(xi[0], e[0])
    x = (signs * np.where(xi[0] < 0, -1, 1)[None]).astype(np.float32)
    rmap = [4, 0, 2]
    plan_is(mx, F32, M, N, K, one(t, N), kind="mkq", nb=1, u=2, bd=0)
    r = mx.kq_matmul_probe(0, F32, blocks, x, list(one(t, N)), N=N, K=K, act=1, norm_w=w, row_map=rmap)
    rows = signs[rmap] * xi[0][None]
    check_operand(r, rows, np.repeat(e[:1], M, axis=0), M, f"norm rows {TNAME[t]}")
    s, _ = exact_product(one(t, N), K, fields, rows, np.repeat(e[:1], M, axis=0))
    assert np.array_equal(r.out, s.astype(np.float32)) and all_ones(r.guard)


# ---- exact: one token quantised on load -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 2304, 4096, 4352, 8192, 8448, 14336, 16384])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_on_load(mx, t, K):
    """launch_mkq_bd<EPI, true>: RESID (no bd_tile form) with ssq partials, and F32 over three segment types."""
    mixed = tuple((ty, i + 1) for i, ty in enumerate([t] + [x for x in TYPES if x != t]))
    for norm in ([False, True] if K <= 8192 else [False]):
        for epi, segs in ((RESID, one(t, 48)), (F32, mixed)):
            plan_is(mx, epi, 1, 48, K, segs, on_load=True, norm=norm, kind="mkq", bd=1, ql=1, u=bd_u(K, True),
                    nkw=per_wave(K))
            for ssq_in in ([False, True] if norm else [False]):
                ssq = epi == RESID and not norm  # (MMArgs has one ssq pointer: partials are read or written)
                r = run_exact(mx, 0, epi, segs, K, 1, rows=33 if epi == F32 else 100, act=2, norm=norm, ssq_in=ssq_in,
                              want_ssq=ssq)
                if ssq:
                    check_ssq(r, f"on load RESID ssq K={K}")


def test_on_load_refusals(mx):
    b, _ = wcase(16, 256, 12)
    for K, norm in ((16640, False), (8448, True)):
        assert not mx.kq_matmul_plan(F32, 1, 16, K, 12, on_load=True, norm=norm)["can_on_load"]
        with pytest.raises(mx.MxError, match="mkq_can_quantize_on_load"):
            mx.kq_matmul_probe(0, F32, np.zeros(16 * K // 256 * 144, np.uint8), np.ones((1, K), np.float32), 12, N=16, act=2,
                               norm_w=np.ones(K, np.float32) if norm else None)


BD_TILE = ([(SWIGLU, 4096, nt, dict(w=7, nkw=16, tpw=1)) for nt in (2, 8, 14)] +
           [(SWIGLU, 2048, nt, dict(w=3, nkw=8, tpw=1)) for nt in (2, 4, 768)] +
           [(F32, 4096, nt, dict(w=8, nkw=16, tpw=4)) for nt in (1, 32, 33, 40)] +
           [(F32, 2048, nt, dict(w=8, nkw=8, tpw=1)) for nt in (1, 9)])


@pytest.mark.parametrize("epi,K,ntiles,cfg", BD_TILE, ids=[f"{EPI_NAME[e]}-{k}-{n}" for e, k, n, _ in BD_TILE])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_bd_tile(mx, t, epi, K, ntiles, cfg):
    """mkq_bd_tile_kernel: tile counts that leave phantom tiles in the last work-group (and none)."""
    N = 16 * ntiles
    for norm in (False, True):
        plan_is(mx, epi, 1, N, K, one(t, N), on_load=True, norm=norm, kind="bd_tile", t=t, u=8,
                grid_x=-(-ntiles // (cfg["w"] * cfg["tpw"])), **cfg)
        run_exact(mx, 0, epi, one(t, N), K, 1, rows=2, act=2, norm=norm)


QKV_PERS = [((12, 12), (14, 16)), ((12, 8), (13, 12), (14, 16))]


@pytest.mark.parametrize("segs", QKV_PERS, ids=["q4k|q6k", "q4k|q5k|q6k"])
def test_qkv_pers(mx, segs):
    """mkq_pers_seg_kernel: K 4096, one normed token, N 256 (head_dim 64): 2 contiguous tiles per work-group."""
    for norm in (True, False):
        plan_is(mx, QKV, 1, 256, 4096, segs, on_load=True, norm=norm, kind="qkv_pers", ks=8, nkw=2, tpw=2, u=4, grid_x=8)
        for rope in ("id", "mixed"):
            run_exact(mx, 0, QKV, segs, 4096, 1, rows=2, act=2, norm=norm, rope=rope)
    odd = ((12, 11), (14, 16))  # a segment end that is odd: mkq_kernel instead
    plan_is(mx, QKV, 1, 256, 4096, odd, on_load=True, norm=True, kind="mkq", u=2)
    run_exact(mx, 0, QKV, odd, 4096, 1, rows=2, act=2, norm=True, rope="mixed")


PERS = [(SWIGLU, 2048, 704, TYPES, dict(nkw=1, tpw=3), 3), (F32, 2048, 1025, TYPES, dict(nkw=1, tpw=8), 4),
        (SWIGLU, 4096, 1792, [12, 14], dict(nkw=2, tpw=7), 4), (F32, 4096, 2049, [12, 14], dict(nkw=2, tpw=8), 4)]


@pytest.mark.parametrize("epi,K,ntiles,types,cfg,ub", PERS, ids=[f"{EPI_NAME[e]}-{k}-{n}" for e, k, n, *_ in PERS])
def test_pers(mx, epi, K, ntiles, types, cfg, ub):
    """mkq_pers_kernel on pre-quantised rows: M 1 block-diagonal, M 2 / 16 the ring; 1025 and 2049 tiles leave the last
    work-group one real tile and seven phantom ones."""
    N = 16 * ntiles
    for t in types:
        for M in (1, 2, 16):
            plan_is(mx, epi, M, N, K, one(t, N), kind="pers", t=t, ks=8, bd=int(M == 1), ql=0, u=ub if M == 1 else 2,
                    grid_x=-(-ntiles // cfg["tpw"]), **cfg)
            run_exact(mx, 0, epi, one(t, N), K, M, rows=16)


def on_load_cases():
    return [(epi, K, ntiles, t, norm, cfg, ub) for epi, K, ntiles, types, cfg, ub in PERS for t in types for norm in (False, True)]


def child_pers_on_load(out_path):
    """The child of test_pers_on_load (MX_NO_KQ_BD_TILE=1 is read once per process): mkq_pers_kernel<QL> on the exact
    operands, each output checked by value and its bits saved for the parent."""
    from llama_p2p_amd import engine

    mx = StopOnHipError(engine)
    res = {}
    for epi, K, ntiles, t, norm, cfg, ub in on_load_cases():
        N = 16 * ntiles
        plan_is(mx, epi, 1, N, K, one(t, N), on_load=True, norm=norm, kind="pers", t=t, ks=8, bd=1, ql=1, u=ub, **cfg)
        r = run_exact(mx, 0, epi, one(t, N), K, 1, rows=16, act=2, norm=norm)
        res[f"{epi}/{K}/{ntiles}/{t}/{int(norm)}"] = r.out.view(np.uint32)
    np.savez(out_path, **res)
    print("child ok")


@pytest.fixture(scope="module")
def pers_on_load_form(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kq") / "pers_on_load.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            f"import test_kq_kernel_gpu as T\nT.child_pers_on_load({out!r})\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MX_NO_KQ_BD_TILE="1"),
                       capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode == 3 or "mx error -2" in r.stderr + r.stdout:
        pytest.exit(f"the child met a GPU error, nothing more is launched: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("epi,K,ntiles,types,cfg,ub", PERS, ids=[f"{EPI_NAME[e]}-{k}-{n}" for e, k, n, *_ in PERS])
def test_pers_on_load(mx, pers_on_load_form, epi, K, ntiles, types, cfg, ub):
    """The quantise-on-load forms of mkq_pers_kernel are shadowed by mkq_bd_tile_kernel: they run in one child
    process under MX_NO_KQ_BD_TILE=1.  Here the same exact operands go through mkq_bd_tile_kernel at the same tile
    counts (704, 1025, 1792, 2049), and the two kernels' outputs must be the same bits, F32 and the SwiGLU act."""
    N = 16 * ntiles
    w, tp = {(SWIGLU, 2048): (3, 1), (SWIGLU, 4096): (7, 1), (F32, 2048): (8, 1), (F32, 4096): (8, 4)}[(epi, K)]
    for t in types:
        for norm in (False, True):
            plan_is(mx, epi, 1, N, K, one(t, N), on_load=True, norm=norm, kind="bd_tile", t=t, w=w, tpw=tp, nkw=K // 256,
                    grid_x=-(-ntiles // (w * tp)))
            r = run_exact(mx, 0, epi, one(t, N), K, 1, rows=16, act=2, norm=norm)
            child = pers_on_load_form[f"{epi}/{K}/{ntiles}/{t}/{int(norm)}"]
            assert np.array_equal(r.out.view(np.uint32), child), \
                f"{TNAME[t]} {EPI_NAME[epi]} {ntiles} tiles norm {norm}: mkq_pers_kernel<QL> and mkq_bd_tile_kernel differ in bits"


# ---- exact: the LDS-shared forms --------------------------------------------------------------------------------------------
WIDE = [(4, 4, 1024), (12, 4, 1024), (4, 4, 2048), (12, 4, 3072), (1400, 7, 1024), (1600, 8, 1024)]


@pytest.mark.parametrize("ntiles,W,K", WIDE, ids=[f"{n}x{k}" for n, _, k in WIDE])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_wide(mx, t, ntiles, W, K):
    """mkq_wide_kernel: SB 4 / 8 / 12 = one, two, three turns of the 4-deep ring (Q6_K: 2-deep); Q4_K: kq_compute_fold."""
    for epi in (F32, SWIGLU):
        N = 16 * ntiles * (2 if epi == SWIGLU and ntiles < 100 else 1)
        Wn = W if N == 16 * ntiles else 4
        for M in ((17, 31, 32) if ntiles < 100 else (31,)):
            plan_is(mx, epi, M, N, K, one(t, N), kind="wide", t=t, w=Wn, nb=2, u=2 if t == 14 else 4, grid_x=N // 16 // Wn)
            run_exact(mx, 0, epi, one(t, N), K, M, rows=32)


SLAB = [(64, 2048, 2), (64, 2304, 2), (64, 4096, 4), (64, 4352, 4), (64, 8192, 8), (256, 8192, 8), (4096, 4096, 4),
        (8192, 4096, 2)]


@pytest.mark.parametrize("N,K,ks", SLAB, ids=[f"{n}x{k}" for n, k, _ in SLAB])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_exact_slab_resid(mx, t, N, K, ks):
    """launch_mkq_slab's partials: every slab fully written for rows < M, summing to the product, folded into x by
    the next launch_rmsnorm_q8k (q8k_kernel<true, true>, N % 256 == 0, N <= 4096) or by launch_resid_norm (N 64, and
    N 8192 where the fused fold has no form: the width at which the engine has to fold first)."""
    for M in ((17, 31, 32) if N <= 256 else (31,)):
        assert plan_is(mx, RESID, M, N, K, one(t, N))["slab_ks"] == ks
        r = run_exact(mx, 1, RESID, one(t, N), K, M, rows=32)
        if N % 256 == 0 and N <= 4096:
            check_q8k_rows(r.nxq, r.nxd, r.nxb, r.out, np.ones(N, np.float32), 0.0, f"slab fold norm N={N} K={K} M={M}")
            assert all_ones(r.nxq_guard) and all_ones(r.nxd_guard) and all_ones(r.nxb_guard)


def test_slab_refusals(mx):
    for N, K in ((64, 1024), (16384, 2048)):
        assert plan_is(mx, RESID, 32, N, K, one(12, N))["slab_ks"] == -1
        b = np.zeros(N * (K // 256) * 144, np.uint8)
        with pytest.raises(mx.MxError, match="launch_mkq_slab refused"):
            mx.kq_matmul_probe(1, RESID, b, np.ones((32, K), np.float32), 12, N=N, resid=np.zeros((32, N), np.float32),
                               fold_w=np.ones(N, np.float32))
    for M in (16, 33):
        with pytest.raises(mx.MxError, match="launch_mkq_slab refused"):
            mx.kq_matmul_probe(1, RESID, np.zeros(64 * 16 * 144, np.uint8), np.ones((M, 4096), np.float32), 12, N=64,
                               resid=np.zeros((M, 64), np.float32), fold_w=np.ones(64, np.float32))


SLAB_QKV = [(4096, 4), (2304, 2), (1024, 1)]


@pytest.mark.parametrize("K,ks", SLAB_QKV, ids=[str(k) for k, _ in SLAB_QKV])
def test_exact_slab_qkv(mx, K, ks):
    """launch_mkq_qkv_slab (mkq_wide_seg_kernel over mixed segments) finished by launch_qkv_finish; K 1024: ks stays 1."""
    for segs in (((12, 12), (14, 16)), ((12, 8), (13, 12), (14, 16))):
        for M in (17, 31, 32):
            assert plan_is(mx, QKV, M, 256, K, segs)["qkv_slab_ks"] == ks
            run_exact(mx, 2, QKV, segs, K, M, rows=32, rope="mixed")
    bad = ((12, 10), (14, 16))
    assert plan_is(mx, QKV, 32, 256, K, bad)["qkv_slab_ks"] == -1
    blocks = case(bad, K, 32)[0]
    with pytest.raises(mx.MxError, match="launch_mkq_qkv_slab refused"):
        mx.kq_matmul_probe(2, QKV, blocks, np.ones((32, K), np.float32), list(bad), N=256, qkv=qkv_args(32, GEOM[256], "id"))


# ---- extremes and one-hot: K 256, one super-block in one wave ---------------------------------------------------------------
def extreme_blocks(t, N, which):
    """Every field at an end of its range: values max (Q6_K: 0 or 63), scales / mins 63 (Q6_K: -128 or 127)."""
    d = R.f16_bits(np.full((N, 1), 2.0 ** JW0))
    if t == 14:
        vals = np.full((N, 256), 0 if which & 1 else 63, np.uint8)
        return R.kq_blocks(t, d, vals, np.full((N, 1, 16), -128 if which & 2 else 127, np.int8))
    return R.kq_blocks(t, d, np.full((N, 256), R.VMAX[t], np.uint8), np.full((N, 1, 8), 63, np.uint8), d,
                       np.full((N, 1, 8), 63, np.uint8))


def run_one_sb(mx, t, blocks, xf, N, M, s0=0, act=0, norm=False, kind=None):
    """Activations that are zero outside super-block s0: every other super-block contributes exactly 0 (d_x = 0), and
    the result is fl(fl(S) d d_x - Mn dmin d_x) whatever the contraction and the summation order (d d_x and dmin d_x
    powers of two here, Mn below 2^24; S may exceed 2^24: its conversion to f32 is the one rounding every kernel
    makes) -- so still compared by value."""
    K = xf.shape[1]
    f = R.kq_fields(t, blocks)
    q, d, bs = R.quantize_q8k(xf[:M])
    assert not q[:, :256 * s0].any() and not q[:, 256 * (s0 + 1):].any()
    g = dict(d=f["d"][:, s0:s0 + 1], dmin=None if t == 14 else f["dmin"][:, s0:s0 + 1], sc=f["sc"][:, s0:s0 + 1],
             mn=None if t == 14 else f["mn"][:, s0:s0 + 1], vals=f["vals"][:, 256 * s0:256 * (s0 + 1)])
    S, Mn = R.superblock_ints(t, g, q[:, 256 * s0:256 * (s0 + 1)])
    dx = d[:, s0].astype(np.float64)[:, None]
    ref = S[..., 0].astype(np.float32).astype(np.float64) * (R.f16_f32(g["d"][:, 0]).astype(np.float64)[None] * dx)
    if t != 14:
        assert np.abs(Mn).max() < 2 ** 24
        ref = ref - Mn[..., 0] * (R.f16_f32(g["dmin"][:, 0]).astype(np.float64)[None] * dx)
    ref = ref.astype(np.float32)
    kw = {}
    x = xf[:M]
    if norm:
        xi = np.rint(xf[0].astype(np.float64) * 2.0 ** 6).astype(np.int64)
        assert np.array_equal(xi * 2.0 ** -6, xf[0])
        x1, w = normed(xi, np.full(K // 256, 6))
        x, kw["norm_w"] = x1[None], w
    what = f"{TNAME[t]} N={N} K={K} M={M} s0={s0} act {act} norm {norm}"
    if kind:
        plan_is(mx, F32, M, N, K, one(t, N), on_load=act == 2, norm=norm, kind=kind)
    r = mx.kq_matmul_probe(0, F32, blocks, x, t, N=N, K=K, act=act, **kw)
    if act != 2:
        assert np.array_equal(R.unperm_rows(r.xq), q) and np.array_equal(r.xd, d) and np.array_equal(r.xb, R.xb_rows(bs)), what
    assert np.array_equal(r.out, ref), what
    assert all_ones(r.guard), what


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_extremes(mx, t):
    """Every weight value, scale and min at its maximum against every q_x at +-127: Q5_K's sub-block product
    |P| = 32 x 31 x 127 = 125 984, just under the 2^17 that __mul24's comment states.  K 256 through mkq_kernel (BD,
    ring, two column tiles, grid.y, quantise on load with and without norm); one extreme super-block among zero
    ones through mkq_bd_tile_kernel (K 2048) and mkq_wide_kernel (K 1024; Q4_K: kq_compute_fold)."""
    rng = np.random.default_rng(t)
    for which in ((0, 1, 2, 3) if t == 14 else (0,)):
        for sign in ("+", "-", "mixed"):
            x = np.full((33, 256), 127.0 * 2.0 ** -6, np.float32)
            if sign == "-":
                x = -x
            if sign == "mixed":
                x *= (rng.integers(0, 2, size=x.shape) * 2 - 1).astype(np.float32)
            b = extreme_blocks(t, 64, which)
            for M in (1, 2, 16, 17, 32, 33):
                run_one_sb(mx, t, b, x, 64, M, kind="mkq")
            run_one_sb(mx, t, b, x, 64, 1, act=2, kind="mkq")
            run_one_sb(mx, t, b, x, 64, 1, act=2, norm=True, kind="mkq")
            for K, M, act, kind in ((2048, 1, 2, "bd_tile"), (1024, 17, 0, "wide"), (1024, 32, 0, "wide")):
                SB = K // 256
                for s0 in (0, SB - 1, SB // 2):
                    xx = np.zeros((33, K), np.float32)
                    xx[:, 256 * s0:256 * (s0 + 1)] = x
                    run_one_sb(mx, t, np.tile(b, (1, SB)), xx, 64, M, s0=s0, act=act, kind=kind)
                    if act == 2:
                        run_one_sb(mx, t, np.tile(b, (1, SB)), xx, 64, M, s0=s0, act=act, norm=True, kind=kind)


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_onehot(mx, t):
    """A single non-zero weight value at each (row in tile, k) class against a single non-zero activation: names the
    misplaced lane or byte when a layout is wrong.  Scales 1 except the one-hot sub-block's (5), mins 0 except one."""
    N, K = 16, 256
    rng = np.random.default_rng(50 + t)
    ks = sorted(set([0, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 160, 224, 255] + rng.integers(0, 256, 16).tolist()))
    for M, act in ((1, 0), (1, 2), (2, 0), (17, 0)):
        for k in ks:
            vals = np.zeros((N, K), np.uint8) + (32 if t == 14 else 0)  # Q6_K: 32 is the zero weight
            rows = np.arange(N)
            kk = (k + 17 * rows) % 256  # every row its own k: a row mix-up shows
            vals[rows, kk] = (rows % (R.VMAX[t])) + 1
            d = R.f16_bits(np.full((N, 1), 2.0 ** JW0))
            if t == 14:
                sc = np.ones((N, 1, 16), np.int8)
                sc[rows, 0, kk // 16] = 5
                b = R.kq_blocks(t, d, vals, sc)
            else:
                sc, mn = np.ones((N, 1, 8), np.uint8), np.zeros((N, 1, 8), np.uint8)
                sc[rows, 0, kk // 32] = 5
                mn[rows, 0, (kk // 32 + 3) % 8] = 9
                b = R.kq_blocks(t, d, vals, sc, d, mn)
            x = np.zeros((M, K), np.float32)
            x[:, k] = 127 * 2.0 ** -6                      # the maximum sits on the probed k ...
            x[:, (k + 17 * 5) % 256] = -3 * 2.0 ** -6      # ... and row 5's weight meets a second value
            run_one_sb(mx, t, b, x, N, M, act=act, kind="mkq")


# ---- the Q8_K quantiser -----------------------------------------------------------------------------------------------------
def crafted(n):
    """Rows with ties in |x| of opposite sign (in one lane and across lanes, at k 0, 15, 16, 255), an all-zero
    super-block, -0.0, exact .5 after scaling and a super-block whose only non-zero element is the maximum."""
    rng = np.random.default_rng(n)
    x = rng.normal(0, 1.0, size=(6, n)).astype(np.float32)
    SB = n // 256
    for s in range(SB):
        o = 256 * s
        a, b = [(0, 15), (16, 255), (15, 16), (0, 255), (3, 9), (255, 0)][s % 6]
        x[0, o + a], x[0, o + b] = -8.0, 8.0            # tie: the first (lower k) decides the sign
        x[1, o + a], x[1, o + b] = 8.0, -8.0
    x[2, :256] = 0.0
    x[2, n - 256:] = np.float32(-0.0)
    x[3, :256] = (np.arange(256) - 128) / 2.0           # iscale = -127 / 63.5 = -2: every odd k lands on .5
    x[3, 0] = 63.5
    x[4, :] = 0.0
    x[4, 7::256] = -3.0                                 # only the maximum is non-zero
    x[5, :256] = np.float32(-0.0)
    x[5, 100] = 2.0 ** -120                             # a tiny maximum: iscale overflows nothing, d tiny
    return x


def check_q8k(r, q, d, bs, what):
    assert np.array_equal(R.unperm_rows(r.xq), q), f"{what}: xq"
    assert np.array_equal(r.xd.view(np.uint32), d.view(np.uint32)), f"{what}: xd"
    assert np.array_equal(r.xb, R.xb_rows(bs)), f"{what}: xb"
    assert all_ones(r.xq_guard) and all_ones(r.xd_guard) and all_ones(r.xb_guard), f"{what}: rows >= M written"


Q8K_N = [256, 3840, 4096, 4352, 8448]


@pytest.mark.parametrize("n", Q8K_N)
def test_quantize_q8k(mx, n):
    """q8k_kernel<false, false> against ggml's quantize_row_q8_K: bit for bit, ld > n, M 1 and more."""
    x = crafted(n)
    q, d, bs = R.quantize_q8k(x)
    for M, ld in ((1, n), (3, n), (6, n + 64), (6, n)):
        xx = np.full((M, ld), np.nan, np.float32)
        xx[:, :n] = x[:M] if M > 1 else x[3:4] if n == 256 else x[:1]
        sel = slice(0, M) if M > 1 else (slice(3, 4) if n == 256 else slice(0, 1))
        r = mx.q8k_probe(xx, n=n)
        check_q8k(r, q[sel], d[sel], bs[sel], f"quantize n={n} M={M} ld={ld}")
        assert np.array_equal(r.x.view(np.uint32), xx.view(np.uint32)) and all_ones(r.x_guard)


def check_q8k_rows(xq, xd, xb, x, w, eps, what):
    """Device Q8_K rows of RMS_NORM(x) * w: the device's steps imitated (f32 squares, double sum, f32 cast, + eps,
    sqrtf, reciprocal) with the nominal f32 scale or one of its two neighbours (a different order of the double sum
    may move (float)(sum / n) by an ulp); at most 1 % of rows via a neighbour, counted and printed."""
    nudged = 0
    for m in range(x.shape[0]):
        for nudge in (0, -1, 1):
            q, d, bs = R.quantize_q8k(R8.norm_rows(x[m:m + 1], w, eps, nudge))
            if (np.array_equal(R.unperm_rows(xq[m:m + 1]), q) and np.array_equal(xd[m:m + 1].view(np.uint32), d.view(np.uint32))
                    and np.array_equal(xb[m:m + 1], R.xb_rows(bs))):
                nudged += nudge != 0
                break
        else:
            raise AssertionError(f"{what}: row {m} matches no scale within one ulp of the nominal one")
    MEASURED["nudged"] += nudged
    MEASURED["rows"] += x.shape[0]
    print(f"norm rows via a neighbouring scale: {what} {nudged} of {x.shape[0]}; so far {MEASURED['nudged']} of {MEASURED['rows']}")
    assert MEASURED["nudged"] <= 0.01 * MEASURED["rows"] + 1, what


@pytest.mark.parametrize("n", Q8K_N)
def test_norm_q8k(mx, n):
    """q8k_kernel<true, false>: random rows of different RMS, crafted rows, eps 1e-5, with and without row_map."""
    rng = np.random.default_rng(n)
    x = np.concatenate([crafted(n)[:4], rng.normal(0, 1, size=(5, n)).astype(np.float32) * np.float32([[0.01], [0.3], [1], [7], [90]])])
    w = (1 + 0.25 * rng.standard_normal(n)).astype(np.float32)
    r = mx.q8k_probe(x, w=w, eps=1e-5)
    check_q8k_rows(r.xq, r.xd, r.xb, x, w, 1e-5, f"norm n={n}")
    assert all_ones(r.xq_guard) and all_ones(r.xd_guard) and all_ones(r.xb_guard)
    assert np.array_equal(r.x.view(np.uint32), x.view(np.uint32)), "x written without slabs"
    rmap = [8, 0, 0, 5, 2]
    r = mx.q8k_probe(x, w=w, eps=1e-5, row_map=rmap)
    check_q8k_rows(r.xq, r.xd, r.xb, x[rmap], w, 1e-5, f"norm row_map n={n}")
    assert all_ones(r.xq_guard) and all_ones(r.xd_guard) and all_ones(r.xb_guard)


@pytest.mark.parametrize("nslab", range(1, 9))
def test_norm_q8k_fold(mx, nslab):
    """q8k_kernel<true, true>: x + (s0 + s1 + ...) pinned bitwise on rows where another order differs, the folded x
    returned, then the norm rows of the folded x."""
    for n in (256, 3840, 4096):
        rng = np.random.default_rng(100 * nslab + n)
        M = 3
        x = rng.normal(0, 1, size=(M, n)).astype(np.float32)
        slabs = (rng.normal(0, 1, size=(nslab, M, n)) * 2.0 ** rng.integers(-12, 4, size=(nslab, M, n))).astype(np.float32)
        t = slabs[0].copy()
        for k in range(1, nslab):
            t = (t + slabs[k]).astype(np.float32)
        want = (x + t).astype(np.float32)
        if nslab >= 2:
            other = x.copy()
            for k in range(nslab):
                other = (other + slabs[k]).astype(np.float32)
            assert (other != want).any(), "the operands do not tell the two orders apart"
        w = (1 + 0.25 * rng.standard_normal(n)).astype(np.float32)
        r = mx.q8k_probe(x, w=w, eps=1e-5, slabs=slabs)
        assert np.array_equal(r.x.view(np.uint32), want.view(np.uint32)), f"fold order nslab={nslab} n={n}"
        assert all_ones(r.x_guard)
        check_q8k_rows(r.xq, r.xd, r.xb, want, w, 1e-5, f"fold nslab={nslab} n={n}")


def test_norm_q8k_refusals(mx):
    x, w = np.ones((2, 4352), np.float32), np.ones(4352, np.float32)
    with pytest.raises(mx.MxError, match="launch_rmsnorm_q8k refused"):
        mx.q8k_probe(x, w=w, slabs=np.zeros((2, 2, 4352), np.float32))         # n > 4096
    with pytest.raises(mx.MxError, match="launch_rmsnorm_q8k refused"):
        mx.q8k_probe(x[:, :256], w=w[:256], slabs=np.zeros((1, 2, 256), np.float32), row_map=[1, 0])
    with pytest.raises(mx.MxError):
        mx.q8k_probe(np.ones((2, 320), np.float32))                              # n % 256


# ---- real scales --------------------------------------------------------------------------------------------------------------
REAL = [(F32, 48, 2304, 1, dict(kind="mkq", bd=1, ql=0)), (F32, 48, 2304, 16, dict(kind="mkq", nb=1, u=2)),
        (F32, 48, 4096, 33, dict(kind="mkq", nb=2, grid_y=2)), (F32, 64, 2048, 32, dict(kind="wide", w=4)),
        (RESID, 64, 4352, 31, dict(slab_ks=4)), (F32, 16 * 9, 2048, 1, dict(kind="bd_tile", w=8, tpw=1)),
        (F32, 256, 4096, 1, dict(kind="bd_tile", w=8, tpw=4))]


@pytest.mark.parametrize("epi,N,K,M,want", REAL, ids=[f"{EPI_NAME[e]}-{n}x{k}-M{m}" for e, n, k, m, _ in REAL])
@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_real_scales(mx, t, epi, N, K, M, want):
    """Synthetic blocks (synth.kq_blocks: random f16 scales) and Gaussian rows.  The integers S and Mn are recomputed
    from the returned xq, so the only freedom left is f32 rounding: each of the 2 SB terms (d d_x) S, (dmin d_x) Mn
    is formed with at most 3 roundings (the scale product, the int -> f32 conversion of |S| >= 2^24, the product)
    and joins a running sum of at most 2 SB + 8 additions (ring, LDS reduction over 8 waves or slabs, fold), each
    rounding by at most 2^-24 of a partial sum that never exceeds sum |terms|:
        |err| <= (3 + 2 SB + 8) 2^-24 sum_s (|d d_x S| + |dmin d_x Mn|).
    The two on-load cases (mkq_bd_tile_kernel) return no xq: there S and Mn come from the host quantiser, which the
    quantiser tests pin to the device's bit for bit."""
    from llama_p2p_amd import synth

    blocks = synth.kq_blocks(t, N * K // 256, seed=11, tid=900 + t).reshape(N, -1)
    f = R.kq_fields(t, blocks)
    x = (np.random.default_rng(K + M).standard_normal((M, K)) * 1.5).astype(np.float32)
    on_load = M == 1 and N != 48
    path = 1 if epi == RESID else 0
    plan_is(mx, epi, M, N, K, one(t, N), on_load=on_load, **want)
    kw = dict(resid=np.zeros((M, N), np.float32), fold_w=np.ones(N, np.float32)) if epi == RESID else {}
    r = mx.kq_matmul_probe(path, epi, blocks, x, t, N=N, K=K, act=2 if on_load else 0, **kw)
    if on_load:
        q, d, bs = R.quantize_q8k(x)
    else:
        q, d, bs = R.quantize_q8k(x)
        check_q8k(r, q, d, bs, f"real scales {TNAME[t]} K={K} M={M}")
        q, d = R.unperm_rows(r.xq), r.xd
    want, mag = R.product(t, f, q, d, R.bsum32_of_xb(r.xb) if not on_load else None)
    bound = (3 + 2 * (K // 256) + 8) * 2.0 ** -24 * mag
    err = np.abs(r.out.astype(np.float64) - want)
    frac = float((err / bound).max())
    MEASURED["real"] = max(MEASURED["real"], frac)
    print(f"real scales worst |err| / bound: {TNAME[t]} {EPI_NAME[epi]} N={N} K={K} M={M} {frac:.3f}; so far {MEASURED['real']:.3f}")
    assert frac <= 1.0
    assert all_ones(r.guard)


# ---- layout and side kernels ----------------------------------------------------------------------------------------------------
def edge_blocks(t, N, SB, seed):
    """Random blocks whose f16 fields are finite, among them a subnormal d, d = 0 and a negative d."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(N, SB, R.BLOCK_BYTES[t]), dtype=np.uint8)
    for o in ([208] if t == 14 else [0, 2]):
        v = rng.uniform(-2, 2, size=(N, SB)).astype(np.float16)
        v[0, 0], v[1, 0], v[2, 0] = np.float16(3e-7), np.float16(0.0), np.float16(-1.25)
        b[..., o], b[..., o + 1] = v.view(np.uint16) & 0xFF, v.view(np.uint16) >> 8
    return b.reshape(N, -1)


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_packer_matches_layout(mx, t):
    """pack_kq_kernel's bytes equal tests/kq_ref.py's for the three pack modes (and a row offset), nothing else written."""
    N, K = 32, 768
    blocks = edge_blocks(t, N, K // 256, 7 + t)
    for mode, off in ((0, 0), (0, 16), (1, 0), (2, 0)):
        got, guard = mx.kq_pack_probe(blocks, t, N, K, pack=mode, offset=off)
        want = R.pack_tiles(t, blocks, mode, off)
        assert np.array_equal(got, want), f"{TNAME[t]} pack mode {mode} offset {off}"
        assert all_ones(guard)
    with pytest.raises(mx.MxError, match="launch_pack_kq refused|mode 0"):
        mx.kq_pack_probe(blocks, 11, N, K)


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_dequant_tiles(mx, t):
    """dequant_kq_kernel's bf16 tiles, bitwise the f32 one-rounding-per-operation values rounded to nearest even; one
    segment and three (segment offsets)."""
    K = 768
    others = [x for x in TYPES if x != t]
    for segs in (((t, 3),), ((others[0], 1), (t, 3), (others[1], 4))):
        parts, want, t0 = [], [], 0
        for i, (ty, te) in enumerate(segs):
            b = edge_blocks(ty, 16 * (te - t0), K // 256, 20 + ty + i)
            parts.append(b.reshape(-1))
            want.append(R.dequant_f32(ty, R.kq_fields(ty, b)))
            t0 = te
        N = 16 * t0
        got, guard = mx.kq_dequant_probe(np.concatenate(parts), list(segs), N, K)
        ref = L.pack_tiles(L.bf16_bits(np.concatenate(want, axis=0)))
        assert np.array_equal(got, ref), f"dequant {segs}"
        assert all_ones(guard)


@pytest.mark.parametrize("t", TYPES, ids=TNAME.values())
def test_embed(mx, t):
    """embed_kq_kernel's rows bitwise dequantize_row_q*_K's, its ssq partials within check_ssq's bar."""
    N, K = 40, 1024
    blocks = edge_blocks(t, N, K // 256, 30 + t)
    ids = [39, 0, 2, 1, 7, 39, 13]
    want = R.dequant_f32(t, R.kq_fields(t, blocks))[ids]
    x, xg, ssq, sg = mx.kq_embed_probe(blocks, t, N, K, ids)
    assert np.array_equal(x.view(np.uint32), want.view(np.uint32))
    assert all_ones(xg) and all_ones(sg)

    class Rr:
        pass
    rr = Rr()
    rr.final, rr.ssq = want.astype(np.float64), ssq
    check_ssq(rr, f"embed {TNAME[t]}")
    x2, xg2, ssq2, _ = mx.kq_embed_probe(blocks, t, N, K, ids, want_ssq=False)
    assert np.array_equal(x2.view(np.uint32), want.view(np.uint32)) and ssq2 is None


# ---- refusals: an error and nothing launched ----------------------------------------------------------------------------------
def test_refusals(mx):
    b = np.zeros(64 * 144, np.uint8)
    x = np.ones((1, 256), np.float32)
    bad = [dict(K=320, xf=np.ones((1, 320), np.float32)), dict(N=24), dict(segs=[(12, 3)]), dict(segs=[(11, 4)]), dict(segs=[(12, 2), (14, 2)]), dict(M=0),
           dict(M=4097, xf=np.ones((4097, 256), np.float32)), dict(ldx=260, K=256, xf=np.ones((1, 260), np.float32), norm_w=np.ones(256, np.float32)),
           dict(act=1), dict(act=2, M=2, xf=np.ones((2, 256), np.float32)), dict(epi=SWIGLU, N=48, segs=[(12, 3)]),
           dict(epi=RESID), dict(epi=QKV), dict(epi=4), dict(path=3), dict(path=1, epi=F32),
           dict(epi=RESID, act=2, norm_w=np.ones(256, np.float32), resid=np.zeros((1, 64), np.float32), want_ssq=True),
           dict(epi=QKV, qkv=dict(qkv_args(1, GEOM[192], "id"), slot=[7]), N=192, segs=[(12, 12)], w=np.zeros(192 * 144, np.uint8))]
    for kw in bad:
        a = dict(path=0, epi=F32, w=b, xf=x, segs=[(12, 4)], N=64, K=256)
        a.update(kw)
        path, epi, w, xf, segs = (a.pop(k) for k in ("path", "epi", "w", "xf", "segs"))
        with pytest.raises(mx.MxError):  # the probe's own check, not the wrapper's
            mx.kq_matmul_probe(path, epi, w, xf, segs, **a)
    r = mx.kq_matmul_probe(0, F32, b, x, [(12, 4)], N=64, K=256)  # ... and the good call next to them runs
    assert (r.out == 0).all() and all_ones(r.guard)


# ---- the engine at a width whose slabs the fused fold cannot take -----------------------------------------------------------
def test_engine_h8192_rows_17_to_32(mx, oracle_mod):
    """Found by this file's plan and quantiser cases: at n_embd 8192 (Llama-3-70B's width) launch_mkq_slab splits
    attn_output / ffn_down of 17..32 rows (ks 2) while launch_rmsnorm_q8k refuses to fold slabs into rows longer than
    4096, so such a forward ended in MX_ERR_ARG.  The engine now folds them with launch_resid_norm first.  20 rows of
    one sequence and 20 sequences of one row against the oracle's K-quant forward, the tolerance of
    tests/test_kquants_gpu.py."""
    from conftest import assert_logits_close, assert_tokens_match
    from llama_p2p_amd import synth

    shape = synth.SHAPES["test-h8192"]
    assert mx.kq_matmul_plan(RESID, 20, shape.n_embd, shape.n_embd, 12)["slab_ks"] == 2
    om = oracle_mod.OracleModel(shape, seed=0)
    om.kq_synthetic("q4_k_m", 0)
    rng = np.random.default_rng(20)
    seq = np.concatenate([[1], rng.integers(3, shape.n_vocab, 19)]).astype(np.int32)
    eng = mx.Engine("synthetic:test-h8192:seed=0:q4_k_m", n_ctx=64, n_seq_max=20)
    got = eng.forward_logits(seq, 0, slot=0)
    ref = om.context(64).eval(seq, 0, all_logits=True)
    assert_logits_close(got, ref, "h 8192, 20 rows of one sequence")
    assert_tokens_match(got, ref, "h 8192, 20 rows of one sequence")
    firsts = [int(t) for t in rng.integers(3, shape.n_vocab, 20)]
    rows = eng.forward_rows(list(range(20)), [0] * 20, firsts)
    eng.close()
    want = np.stack([om.context(64).eval(np.array([t], np.int32), 0)[0] for t in firsts])
    assert_logits_close(rows, want, "h 8192, 20 sequences")
