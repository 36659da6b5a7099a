"""The Q8_0 / Q4_0 kernels alone (mq8_kernel in its block-diagonal, quantise-on-load and 17..32-row forms,
mq8_pers_ql_kernel, mq8_wide_kernel with its EPI_SLAB split-K form, mq8_wsw_kernel, q8gemm_kernel, quantize_q8_kernel,
norm_q8_kernel, norm_q8_fold_kernel, pack_q8_kernel, pack_q4_kernel, dequant_q8_tiles_kernel, embed_q8_kernel)
against exact integer references, through mx_q8_matmul_probe / mx_q8_side_probe -- no model.

Why bitwise: a Q8_0 x Q8_0 product is a sum of exact int32 block products, each times d_w * d_x.  Here every weight
scale is 2^j (3 consecutive exponents per matrix) and every activation block holds integers in [-4, 4] times 2^-e (3
consecutive e per case) with exactly one element +-127 * 2^-e, so the device's quantiser returns d_x = 2^-e and those
integers (checked on the returned xq / xd), d_w * d_x is exact, and every partial sum is a multiple of the unit
2^(j_min - e_max) below 2^24 units (asserted in the builder from sum_k |w x|) -- exact in f32 in ANY summation
order.  The reference is the float64 product of the dequantised operands (exact: tests/test_q8_ref.py pins it to the
int64 block sums).  Comparisons are by value (==): bit equality except for the sign of a zero, and a NaN (the probe's
0xFF poison in outputs, slabs, xq / xd rows >= M and f32 source rows >= M) never compares equal.

Families: exact (xq / xd, F32 / RESID / QKV bitwise, SWIGLU's f32 act within ACTF_BAR of float64 -- the Q8 kernels go
through the same epi_store<EPI_SWIGLU> as the bf16 ones, so that file's bar is used --, slabs fully written and
summing to the product, guards), extremes, onehot, quantisers, real scales, norm on load on random rows, layout
and side kernels, refusals.

Branches and the case that reaches each (every case asserts its kernel through mx_q8_matmul_plan):
  mq8_kernel<8,1,1,BD> (M 1), tiles per wave = the (KT w) / 8 split of KT = K / 64: K 64 (0 | 1: 7 of 8 waves
    empty), 448 (0 | 1), 512 (1), 576 (1 | 2), 1536 (3), 2048 (4), 2112 (4 | 5), 3584 (7), 4096 (8), 4608 (9),
    8192 (16): test_exact_gemv.
  mq8_kernel<8,1,1> (M 2, 15, 16), ring U 4: the same K list = 0, 1, < U, U, U + tail, k U, k U + tail tiles.
  mq8_kernel 17..32 rows where wide / slab refuse (K 320): cfg 1 <8,2,2> QKV 256; cfg 3 <4,4,2> F32 / SWIGLU 64;
    cfg 0 <8,1,2> 48 (odd tile count) and RESID 96 (N % 64): test_exact_mid.
  mq8_kernel<8,1,4>: M 33, 64, and 65, 100, 255 (grid.y 2, 2, 4, ragged last group): test_exact_gemv.
  quantise on load: M 1..4 (QM 1 / 2 / 4; M 3 in a 4-slot image), QP 2 / 4 / 8 at K 512, 4096 | 4160, 8192 |
    16384, with and without norm (norm: K <= 8192), RESID with ssq partials: test_exact_on_load.  Random rows of
    different RMS, eps 1e-5, random norm_w, M 1..4 at K 512 / 4160 / 8192: test_norm_on_load_random.
  mq8_pers_ql_kernel: SWIGLU 14 and 1792 tiles, Q4 QKV 384 (24 tiles), K 4096, M 1, norm: test_pers_ql (exact,
    and bit-identity to the one-tile form under MX_NO_Q8_PERS_QL=1 in a child process on random operands),
    test_extremes_pers_ql, test_onehot_pers_ql, and its real-scale cases in test_norm_on_load_random.
  mq8_wide_kernel (Q8) / mq8_wsw_kernel (Q4): W 4 at 4 and 12 tiles, W 7 at 1400, W 8 at 1600, K 256; W 4 at
    K 256 * {1..5}; M 17, 31, 32: test_exact_wide.
  launch_mq8_slab: ks 1 (K 256, 1792), 2 (2048, 2304: 4 + 5 chunks), 4 (4096, 4352), 8 (8192, 8448) at N 64; N 4096
    (ks <= 4) and the launch_resid_norm fallback at N 8192; RESID through norm_q8_fold_kernel<1|2|4|8>, QKV through
    launch_qkv_finish: test_exact_slab_resid, test_exact_slab_qkv.
  q8gemm_kernel: N 5632 M 257 (grid 66), N 512 M 4096 (grid 64), K 64 / 256 / 320, all epilogues (QKV: 6144, M 257),
    and M 3968 x N 512 (grid 62): the GEMVs, same results: test_exact_gemm.
  launch_rmsnorm_q8: nslab 0 norm_q8_kernel; 1, 2, 4, 8 norm_q8_fold_kernel; 3, 5, 6, 7, a row_map or n > 4096
    fold first (launch_resid_norm): test_norm_q8.

Measured on MI355X over all cases of this file (the tests print each case's figure):
  f32 SwiGLU (actf) worst relative error vs float64 ....... 1.99e-7 (asserted at the bf16 file's ACTF_BAR, 7.0e-7:
    the same epi_store<EPI_SWIGLU>)
  real scales: worst |err| / bound ........................ 0.41
  norm rows matching only a neighbouring f32 scale ........ 0 of 2293
  norm on load, random rows: worst |err| / bound .......... 0.10; rows needing a neighbouring scale: 0 of 76

Mutations tried on scratch copies of kernels.hip (none committed), each run against this file, with the first test
that failed:
  mq8_kernel's tail loop dropped -> test_exact_gemv[q8-0-64] (F32, M 2: K 64 is tail only);
  q8_perm's bit 5 and bits 3..4 swapped back on the quantiser side -> test_exact_gemv[q8-0-64] (the returned xq);
  q4_operand's high nibbles without the subtraction of 8 in one byte -> test_exact_gemv[q4-0-64];
  QG_MAGIC's subtraction constant 12582913 -> test_exact_wide[q8-4x256];
  norm_q8_fold_kernel adding the slabs to x one by one -> test_norm_q8_fold_order[2];
  mq8_pers_ql_kernel's load_dw(i + 1) reading tile i -> test_exact_on_load[q4-2-4096] (QKV, one normed token: the
    12-tile q|k|v reaches mq8_pers_ql_kernel<2>; test_pers_ql fails too).
  The BD form's `tt < ke` zeroing removed: every test passes -- the MFMAs of a k-tile past the slice are already
    skipped by the wave-uniform `kt < ke`, so that block's C column stays 0 whatever x holds, and 0 times the
    (finite, clamped) d_w d_x adds nothing: the zeroing is redundant, the mutant equivalent.
  q8gemm's tokd clamp removed: every test passes -- a padded token's d_x (the probe's NaN rows past M) feeds only
    that token's own outputs, which are dropped; the clamp guards the end of the xd buffer (as the bf16 file's
    column clamp).
  launch_mq8_slab's chunk range cb from blockIdx.y + 1: as written the last range starts at the end of K and reads
    past the buffers, so it was run wrapped inside K (cb = NCHT ((y + 1) % ks) / ks, each range keeping its own
    length, which never exceeds the last range's) -> test_exact_slab_resid[q8-64x2304] (4 + 5 chunks: chunk 4 read
    twice, chunk 8 never).  Where K splits evenly the wrapped form only permutes the slabs, whose sum is unchanged;
    which slab holds which range is not pinned by this file.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mm_layout as L
import q8_ref as R
import test_matmul_kernel_gpu as B
from test_matmul_kernel_gpu import ACTF_BAR, GEOM, N_CTX, all_ones, check_qkv, check_ssq, qkv_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, RESID, QKV, SWIGLU = 0, 1, 2, 3
EPI_NAME = B.EPI_NAME
FMT = [False, True]
FMT_ID = ["q8", "q4"]
JW0 = -6          # weight scales 2^-6, 2^-5, 2^-4: normal f16
MEASURED = {"actf": 0.0, "real": 0.0, "nudged": 0, "rows": 0}


class StopOnHipError(B.StopOnHipError):
    def q8_matmul_probe(self, *a, **kw):
        return self._call(self._e.q8_matmul_probe, *a, **kw)

    def q8_dequant_tiles_probe(self, *a, **kw):
        return self._call(self._e.q8_dequant_tiles_probe, *a, **kw)

    def q8_embed_probe(self, *a, **kw):
        return self._call(self._e.q8_embed_probe, *a, **kw)


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return StopOnHipError(engine)


def plan_is(mx, epi, M, N, K, q4, on_load=False, norm=False, **want):
    p = mx.q8_matmul_plan(epi, M, N, K, wq4=q4, on_load=on_load, norm=norm)
    got = {k: p[k] for k in want}
    assert got == want, f"plan of {EPI_NAME[epi]} M={M} N={N} K={K} q4={q4}: {p}"
    return p


# ---- operands -------------------------------------------------------------------------------------------------------
def act_exp(K, q4):
    """e0 with the sums of order 2: a block's product has sigma ~ 2600 (Q4: 4700) units 2^(JW0 - e); the rare
    -128 / 127 blocks make the tails long, and SWIGLU's gate must stay far inside expf's range (|g| <= 80)."""
    sig = (4700 if q4 else 2600) * np.sqrt(K / 32)
    return int(np.clip(round(np.log2(sig / 2)) + JW0, 0, 12))


@functools.lru_cache(maxsize=3)
def wcase(N, K, q4, kind="int"):
    """(GGUF blocks uint8 [N][...], integer weights [N][K] (Q4: nibble - 8), exponents j [N][K/32]).
    kind int: Q8 q in [-4, 4] with about one block in 8 carrying a -128 and a 127, Q4 nibbles over 0..15."""
    rng = np.random.default_rng(1000 + N + K + q4)
    nb = K // 32
    jw = rng.integers(JW0, JW0 + 3, size=(N, nb))
    dbits = R.f16_bits(2.0 ** jw)
    if q4:
        nib = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
        blocks, wv = R.q4_blocks(dbits, nib), nib.astype(np.int16) - 8
    else:
        q = rng.integers(-4, 5, size=(N, K), dtype=np.int16).reshape(N, nb, 32)
        big = rng.random((N, nb)) < 0.125
        pos = rng.integers(0, 32, size=(N, nb, 2))
        pos[..., 1] = (pos[..., 0] + 1 + pos[..., 1] % 31) % 32  # two distinct places
        n_i, b_i = np.nonzero(big)
        q[n_i, b_i, pos[n_i, b_i, 0]] = -128
        q[n_i, b_i, pos[n_i, b_i, 1]] = 127
        wv = q.reshape(N, K)
        blocks = R.q8_blocks(dbits, wv.astype(np.int8))
    for a in (blocks, wv, jw):
        a.setflags(write=False)
    return blocks, wv, jw


@functools.lru_cache(maxsize=4)
def xcase(K, rows, e0):
    """(xf f32 [rows][K], integers [rows][K], e [rows][K/32]): integers in [-4, 4] times 2^-e, one +-127 per block."""
    rng = np.random.default_rng(2000 + K + rows)
    nb = K // 32
    xi = rng.integers(-4, 5, size=(rows, nb, 32)).astype(np.int16)
    at = rng.integers(0, 32, size=(rows, nb))
    r_i, b_i = np.indices((rows, nb))
    xi[r_i, b_i, at] = 127 * (1 - 2 * rng.integers(0, 2, size=(rows, nb)))
    e = rng.integers(e0, e0 + 3, size=(rows, nb))
    xf = (xi * 2.0 ** -e[..., None]).astype(np.float32).reshape(rows, K)
    xi = xi.reshape(rows, K)
    for a in (xf, xi, e):
        a.setflags(write=False)
    return xf, xi, e


def exact_product(wv, jw, xv, sx, e_max):
    """float64 [M][N] product of the dequantised operands, asserted exact in f32 in any order."""
    X = xv.astype(np.float64) * np.repeat(sx, 32, axis=1)
    unit = 2.0 ** (jw.min() - e_max)
    out = np.empty((xv.shape[0], wv.shape[0]))
    step = max(16, (1 << 24) // wv.shape[1])
    for n0 in range(0, wv.shape[0], step):  # row blocks of W: the float64 copies stay small
        W = wv[n0:n0 + step].astype(np.float64) * np.repeat(2.0 ** jw[n0:n0 + step], 32, axis=1)
        bound = float((np.abs(X) @ np.abs(W).T).max()) / unit
        assert bound < 2 ** 24, f"partial sums could leave f32's exact range: 2^{np.log2(bound):.1f} units"
        out[:, n0:n0 + step] = X @ W.T
    return out, unit


@functools.lru_cache(maxsize=2)
def case(N, K, q4, rows):
    blocks, wv, jw = wcase(N, K, q4)
    e0 = act_exp(K, q4)
    xf, xi, e = xcase(K, rows, e0)
    s, unit = exact_product(wv, jw, xi, 2.0 ** -e, e0 + 2)
    s.setflags(write=False)
    return blocks, xf, xi, e, s, unit


def check_operand(r, xi, e, M, what):
    assert np.array_equal(R.unperm_rows(r.xq), xi[:M]), f"{what}: the device's xq is not the intended integers"
    assert np.array_equal(r.xd, (2.0 ** -e[:M]).astype(np.float32)), f"{what}: the device's xd"
    assert all_ones(r.xq_guard) and all_ones(r.xd_guard), f"{what}: xq / xd rows >= M written"


def check_out(mx, r, epi, s, M, N, what, qa=None, resid_i=None, unit=None):
    """One launch's outputs against the exact product s [M][N]; returns the exact final residual for RESID."""
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


def run_exact(mx, path, epi, N, K, M, q4, *, rows=64, rope="id", want_ssq=False):
    """Pre-quantised rows (launch_quantize_q8) through path 0 / 1 on the shared integer case."""
    blocks, xf, xi, e, s, unit = case(N, K, q4, rows)
    s = s[:M]
    what = f"path {path} {FMT_ID[q4]} {EPI_NAME[epi]} M={M} N={N} K={K}"
    kw, qa, ri = dict(wq4=q4, want_slabs=path == 1), None, None
    if epi == RESID:
        ri = resid_ints(M, N)
        kw.update(resid=(ri * unit).astype(np.float32), want_ssq=want_ssq)
        if path == 1:
            kw["fold_w"] = np.ones(N, np.float32)
    if epi == QKV:
        qa = kw["qkv"] = qkv_args(M, GEOM[N], rope)
    r = mx.q8_matmul_probe(path, epi, blocks, xf[:M], **kw)
    check_operand(r, xi, e, M, what)
    check_out(mx, r, epi, s, M, N, what + (f" rope {rope}" if epi == QKV else ""), qa, ri, unit)
    if path == 1:
        ks = mx.q8_matmul_plan(epi, M, N, K, wq4=q4)["slab_ks"]
        assert r.split == ks and r.slabs.shape == (ks, M, N), f"{what}: split {r.split}, plan {ks}"
        assert not (r.slabs.view(np.uint32) == 0xFFFFFFFF).any(), f"{what}: slab element never written"
        assert np.array_equal(r.slabs.astype(np.float64).sum(axis=0), s), f"{what}: slabs do not sum to the product"
    return r


# ---- exact: mq8_kernel on pre-quantised rows ----------------------------------------------------------------------------
GEMV_K = [64, 448, 512, 576, 1536, 2048, 2112, 3584, 4096, 4608, 8192]
GEMV_M = [1, 2, 15, 16, 33, 64, 65, 100, 255]


@pytest.mark.parametrize("K", GEMV_K)
@pytest.mark.parametrize("epi", [F32, RESID, SWIGLU])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_gemv(mx, q4, epi, K):
    N = 96 if epi == SWIGLU else 48
    for M in GEMV_M if K <= 4096 else [1, 2, 16, 33]:
        plan_is(mx, epi, M, N, K, q4, kind="mq8", ks=8, rt=1, nb=1 if M <= 16 else 4, bd=int(M == 1),
                grid_y=1 if M <= 16 else (M + 63) // 64)
        r = run_exact(mx, 0, epi, N, K, M, q4, rows=255, want_ssq=epi == RESID)
        if epi == RESID:
            check_ssq(r, f"mq8 RESID ssq M={M} K={K}")


@pytest.mark.parametrize("K", [64, 2112])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_gemv_qkv(mx, q4, K):
    for M in [1, 5, 16, 33, 100]:
        for rope in ("id", "quarter", "mixed"):
            plan_is(mx, QKV, M, 192, K, q4, kind="mq8", nb=1 if M <= 16 else 4)
            run_exact(mx, 0, QKV, 192, K, M, q4, rows=100, rope=rope)


MID = [(QKV, 256, dict(ks=8, rt=2, nb=2)), (F32, 64, dict(ks=4, rt=4, nb=2)), (SWIGLU, 128, dict(ks=4, rt=4, nb=2)),
       (F32, 48, dict(ks=8, rt=1, nb=2)), (SWIGLU, 96, dict(ks=8, rt=1, nb=2)), (RESID, 96, dict(ks=8, rt=1, nb=2)),
       (RESID, 64, dict(ks=8, rt=1, nb=2))]


@pytest.mark.parametrize("epi,N,cfg", MID, ids=[f"{EPI_NAME[e]}-{n}" for e, n, _ in MID])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_mid(mx, q4, epi, N, cfg):
    """17..32 rows at K 320 (K % 256: the LDS-shared forms and the slabs refuse): mq8_kernel's three configurations."""
    for K in (320, 2112):
        for M in (17, 31, 32):
            assert plan_is(mx, epi, M, N, K, q4, kind="mq8", **cfg)["slab_ks"] == -1
            run_exact(mx, 0, epi, N, K, M, q4, rows=32, rope="mixed")


# ---- exact: the LDS-shared forms ------------------------------------------------------------------------------------------
WIDE = [(4, 4, 256), (12, 4, 256), (1400, 7, 256), (1600, 8, 256), (4, 4, 512), (4, 4, 768), (4, 4, 1024), (4, 4, 1280)]


@pytest.mark.parametrize("ntiles,W,K", WIDE, ids=[f"{t}x{k}" for t, _, k in WIDE])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_wide(mx, q4, ntiles, W, K):
    for epi in (F32, SWIGLU):
        for M in (17, 31, 32):
            plan_is(mx, epi, M, 16 * ntiles, K, q4, kind="wsw" if q4 else "wide", w=W)
            run_exact(mx, 0, epi, 16 * ntiles, K, M, q4, rows=32)


SLAB = [(64, 256, 1), (64, 1792, 1), (64, 2048, 2), (64, 2304, 2), (64, 4096, 4), (64, 4352, 4), (64, 8192, 8),
        (64, 8448, 8), (4096, 256, 1), (4096, 2048, 2), (4096, 4096, 4), (8192, 256, 1)]


@pytest.mark.parametrize("N,K,ks", SLAB, ids=[f"{n}x{k}" for n, k, _ in SLAB])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_slab_resid(mx, q4, N, K, ks):
    """launch_mq8_slab's partials folded by the next launch_rmsnorm_q8 (norm_q8_fold_kernel<ks>; N 8192:
    launch_resid_norm first): slabs, the folded x, and that norm's Q8_0 rows against tests/q8_ref.py."""
    for M in ((17, 31, 32) if N == 64 else (31,)):
        assert plan_is(mx, RESID, M, N, K, q4)["slab_ks"] == ks
        r = run_exact(mx, 1, RESID, N, K, M, q4, rows=32)
        check_norm_rows(r.nxq, r.nxd, r.out, np.ones(N, np.float32), 0.0, f"slab fold norm N={N} K={K} M={M}")
        assert all_ones(r.nxq_guard) and all_ones(r.nxd_guard)


@pytest.mark.parametrize("N,K,ks", [(192, 256, 1), (192, 2304, 2), (320, 4352, 4), (192, 8448, 8), (6144, 256, 1)])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_slab_qkv(mx, q4, N, K, ks):
    for M in (17, 32):
        for rope in ("quarter", "mixed"):
            assert plan_is(mx, QKV, M, N, K, q4)["slab_ks"] == ks
            run_exact(mx, 1, QKV, N, K, M, q4, rows=32, rope=rope)


# ---- exact: q8gemm_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 256, 320])
@pytest.mark.parametrize("epi,N,M,grid", [(F32, 5632, 257, 66), (RESID, 5632, 257, 66), (SWIGLU, 5632, 257, 66),
                                          (F32, 512, 4096, 64), (RESID, 512, 4096, 64), (SWIGLU, 512, 4096, 64),
                                          (QKV, 6144, 257, 72)],
                         ids=lambda v: EPI_NAME[v] if isinstance(v, int) and v < 4 else str(v))
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_gemm(mx, q4, epi, N, M, grid, K):
    plan_is(mx, epi, M, N, K, q4, kind="gemm", grid=grid)
    run_exact(mx, 0, epi, N, K, M, q4, rows=M, rope="mixed")


@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_gemm_threshold_falls_back_to_the_gemvs(mx, q4):
    """Grid 62 < 64 (N 512, M 3968): mq8_kernel<8,1,4>, and the same bits as the GEMM gives those rows at M 4096."""
    N, K = 512, 64
    plan_is(mx, F32, 3968, N, K, q4, kind="mq8", nb=4, grid_y=62)
    a = run_exact(mx, 0, F32, N, K, 3968, q4, rows=4096)
    b = run_exact(mx, 0, F32, N, K, 4096, q4, rows=4096)
    assert np.array_equal(a.out.view(np.uint32), b.out[:3968].view(np.uint32))


# ---- exact: quantise on load ------------------------------------------------------------------------------------------------
def on_load_operands(K, M, e0, norm):
    """xf [M][K], norm_w [K] or None, and the operand's integers / scales.  norm: xf = +-1 (mean square exactly 1,
    1.0f / sqrtf(1.0f + 0) exactly 1), norm_w = {1, 2, 4, one 127 per block} * 2^-e: (x * 1) * w = +-w exactly."""
    if not norm:
        xf, xi, e = xcase(K, 4, e0)
        return xf[:M], None, xi[:M], 2.0 ** -e[:M]
    rng = np.random.default_rng(4000 + K)
    nb = K // 32
    sign = (rng.integers(0, 2, size=(M, K)) * 2 - 1).astype(np.int16)
    m = (2 ** rng.integers(0, 3, size=(nb, 32))).astype(np.int16)
    m[np.arange(nb), rng.integers(0, 32, size=nb)] = 127
    e = rng.integers(e0, e0 + 3, size=nb)
    w = (m * 2.0 ** -e[:, None]).astype(np.float32).reshape(K)
    return sign.astype(np.float32), w, sign * m.reshape(K)[None, :], np.broadcast_to(2.0 ** -e, (M, nb))


ON_LOAD = [(512, 2), (4096, 2), (4160, 4), (8192, 4), (16384, 8)]


@pytest.mark.parametrize("K,qp", ON_LOAD, ids=[str(k) for k, _ in ON_LOAD])
@pytest.mark.parametrize("epi", [F32, RESID, QKV, SWIGLU])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_exact_on_load(mx, q4, epi, K, qp):
    N = {F32: 48, RESID: 48, QKV: 192, SWIGLU: 96}[epi]
    blocks, wv, jw = wcase(N, K, q4)
    e0 = act_exp(K, q4)
    for norm in ((False, True) if K <= 8192 else (False,)):
        if norm and epi == RESID:
            continue  # the engine's RESID GEMVs (attn_output, ffn_down) take un-normed rows
        for M in (1, 2, 3, 4):
            # (Q4 q|k|v of 12 tiles at K 4096, one normed token: mq8_pers_ql_kernel<2>, as test_pers_ql's 24 tiles)
            pers = q4 and epi == QKV and M == 1 and K == 4096 and norm
            pl = plan_is(mx, epi, M, N, K, q4, on_load=True, norm=norm, kind="pers_ql" if pers else "ql", qp=qp,
                         qm=(1, 2, 4, 4)[M - 1], bd=int(M == 1), tpw=2 if pers else 0)
            assert pl["can_on_load"]
            xf, nw, xi, sx = on_load_operands(K, M, e0, norm)
            s, unit = exact_product(wv, jw, xi, sx, e0 + 2)
            what = f"on load {FMT_ID[q4]} {EPI_NAME[epi]} M={M} K={K} norm={norm}"
            kw, qa, ri = dict(wq4=q4, act=2, norm_w=nw), None, None
            if epi == RESID:
                ri = resid_ints(M, N)
                kw.update(resid=(ri * unit).astype(np.float32), want_ssq=True)
            if epi == QKV:
                qa = kw["qkv"] = qkv_args(M, GEOM[N], "quarter")
            r = mx.q8_matmul_probe(0, epi, blocks, xf, **kw)
            check_out(mx, r, epi, s, M, N, what, qa, ri, unit)
            if epi == RESID:
                check_ssq(r, what)


# ---- mq8_pers_ql_kernel -----------------------------------------------------------------------------------------------------
PERS = [(SWIGLU, 16 * 14, False), (SWIGLU, 16 * 14, True), (SWIGLU, 16 * 1792, False), (SWIGLU, 16 * 1792, True),
        (QKV, 384, True)]
PERS_ID = [f"{FMT_ID[q]}-{EPI_NAME[e]}-{n}" for e, n, q in PERS]


def pers_random(epi, N, q4):
    """Random f16 scales, full-range q and random rows: the order of the block sums changes the rounding."""
    rng = np.random.default_rng(50 + N)
    K, nb = 4096, 128
    dbits = R.f16_bits((0.5 + rng.random((N, nb))) * 2.0 ** -7)
    blocks = (R.q4_blocks(dbits, rng.integers(0, 16, size=(N, K), dtype=np.uint8)) if q4
              else R.q8_blocks(dbits, rng.integers(-127, 128, size=(N, K), dtype=np.int8)))
    xf = rng.standard_normal((1, K)).astype(np.float32)
    nw = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    kw = dict(wq4=q4, act=2, norm_w=nw, eps=1e-5)
    if epi == QKV:
        kw["qkv"] = qkv_args(1, GEOM[N], "mixed")
    return blocks, xf, kw


def pers_random_bits(eng, epi, N, q4):
    blocks, xf, kw = pers_random(epi, N, q4)
    r = eng.q8_matmul_probe(0, epi, blocks, xf, **kw)
    assert not np.isnan(r.out).any()
    return [r.out.view(np.uint32)] + ([r.kcache, r.vcache] if epi == QKV else [])


def child_no_pers_ql(out_path):  # the child of test_pers_ql: MX_NO_Q8_PERS_QL is read once per process
    from llama_p2p_amd import engine

    engine.lib()
    res = {}
    for (epi, N, q4), name in zip(PERS, PERS_ID):
        assert engine.q8_matmul_plan(epi, 1, N, 4096, wq4=q4, on_load=True, norm=True)["kind"] == "ql"
        for i, a in enumerate(pers_random_bits(engine, epi, N, q4)):
            res[f"{name}/{i}"] = a
    np.savez(out_path, **res)
    print("child ok")


@pytest.fixture(scope="module")
def one_tile_form(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("q8") / "no_pers.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            f"import test_q8_kernel_gpu as T\nT.child_no_pers_ql({out!r})\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MX_NO_Q8_PERS_QL="1"),
                       capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or "mx error -2" in r.stderr:
        pytest.exit(f"the child met a GPU error, nothing more is launched: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("epi,N,q4", PERS, ids=PERS_ID)
def test_pers_ql(mx, one_tile_form, epi, N, q4):
    """exact: the norm form of test_exact_on_load at K 4096, M 1.  equal: 'per tile the arithmetic and summation
    order are mq8_kernel<8,1,1,EPI,4,2,1,Q4,true>'s, so the results are bit-identical' (comment above the kernel)
    -- random operands, against the one-tile form run in a child under MX_NO_Q8_PERS_QL=1."""
    K = 4096
    plan_is(mx, epi, 1, N, K, q4, on_load=True, norm=True, kind="pers_ql", tpw=7 if epi == SWIGLU else 2)
    blocks, wv, jw = wcase(N, K, q4)
    e0 = act_exp(K, q4)
    xf, nw, xi, sx = on_load_operands(K, 1, e0, True)
    s, unit = exact_product(wv, jw, xi, sx, e0 + 2)
    kw, qa = dict(wq4=q4, act=2, norm_w=nw), None
    if epi == QKV:
        qa = kw["qkv"] = qkv_args(1, GEOM[N], "quarter")
    what = f"pers_ql {FMT_ID[q4]} {EPI_NAME[epi]} N={N}"
    check_out(mx, mx.q8_matmul_probe(0, epi, blocks, xf, **kw), epi, s, 1, N, what, qa)
    name = PERS_ID[PERS.index((epi, N, q4))]
    for i, a in enumerate(pers_random_bits(mx, epi, N, q4)):
        assert np.array_equal(a, one_tile_form[f"{name}/{i}"]), f"{what}: differs from the one-tile form (output {i})"


# ---- extremes -----------------------------------------------------------------------------------------------------------------
FAMILY = [  # (name, path, epi, M, N, K of the extremes, K of onehot / real scales, on_load, plan)
    ("bd", 0, F32, 1, 48, 64, 576, False, dict(kind="mq8", bd=1)),
    ("gemv16", 0, F32, 16, 48, 128, 576, False, dict(kind="mq8", nb=1, bd=0)),
    ("mid", 0, F32, 17, 48, 64, 576, False, dict(kind="mq8", nb=2)),
    ("gemv64", 0, F32, 64, 48, 128, 576, False, dict(kind="mq8", nb=4)),
    ("ql", 0, F32, 3, 48, 256, 512, True, dict(kind="ql", qm=4)),
    ("ql1", 0, F32, 1, 48, 256, 512, True, dict(kind="ql", bd=1)),
    ("wide", 0, F32, 17, 64, 256, 512, False, dict(w=4)),
    ("slab", 1, RESID, 17, 64, 256, 512, False, dict(slab_ks=1)),
    ("gemm", 0, F32, 4096, 512, 64, 320, False, dict(kind="gemm")),
]


@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_extremes(mx, q4, fam):
    """Every |isum| at its largest, 32 * 128 * 127 = 520192 (Q4: 32 * 8 * 127): weights all -128 (Q4: nibble 0 in
    even blocks, 15 in odd ones) against activations all +-127 (one sign per block) -- where QG_MAGIC and
    q4_operand16 lose exactness if their bounds are wrong; plus a zero activation block (d = 0, id = 0) and a zero
    d_w block per row.  (mq8_pers_ql_kernel: test_extremes_pers_ql.)"""
    name, path, epi, M, N, K, _, on_load, want = fam
    plan_is(mx, epi, M, N, K, q4, on_load=on_load, **want)
    rng = np.random.default_rng(7)
    nb = K // 32
    UNIT = 2.0 ** (JW0 - 1)  # two exponents each side: 8 blocks of 520192 * 4 units stay below 2^24
    jw = rng.integers(JW0, JW0 + 2, size=(N, nb))
    dw = 2.0 ** jw
    dw[np.arange(N), np.arange(N) % nb] = 0.0  # a zero d_w (the q stay at their extreme)
    if q4:
        nib = np.where(np.arange(nb) % 2, 15, 0).astype(np.uint8)
        nib = np.broadcast_to(np.repeat(nib, 32), (N, K))
        blocks, wv = R.q4_blocks(R.f16_bits(dw), nib), nib.astype(np.int16) - 8
    else:
        wv = np.full((N, K), -128, np.int16)
        blocks = R.q8_blocks(R.f16_bits(dw), wv.astype(np.int8))
    sign = 1 - 2 * rng.integers(0, 2, size=(M, nb))
    e = rng.integers(0, 2, size=(M, nb))
    xi = np.repeat(127 * sign, 32, axis=1)
    zero = (np.arange(M) + 1) % nb
    xi.reshape(M, nb, 32)[np.arange(M), zero] = 0  # an all-zero activation block per row
    sx = 2.0 ** -e
    sx_dev = sx.copy()
    sx_dev[np.arange(M), zero] = 0.0
    xf = (xi * np.repeat(sx, 32, axis=1)).astype(np.float32)
    W = wv * np.repeat(dw, 32, axis=1)
    s = (xi * np.repeat(sx, 32, axis=1)) @ W.T
    assert float((np.abs(xf.astype(np.float64)) @ np.abs(W).T).max()) / UNIT + 16 < 2 ** 24
    what = f"extremes {name} {FMT_ID[q4]}"
    kw = dict(wq4=q4, act=2 if on_load else 0, want_slabs=path == 1)
    ri = None
    if epi == RESID:
        ri = resid_ints(M, N)
        kw.update(resid=(ri * UNIT).astype(np.float32), fold_w=np.ones(N, np.float32))
    r = mx.q8_matmul_probe(path, epi, blocks, xf, **kw)
    if not on_load:
        assert np.array_equal(R.unperm_rows(r.xq), xi) and np.array_equal(r.xd, sx_dev.astype(np.float32)), what
    check_out(mx, r, epi, s, M, N, what, None, ri, UNIT)


@pytest.mark.parametrize("epi,N,q4", [(SWIGLU, 224, False), (SWIGLU, 224, True), (QKV, 384, True)],
                         ids=["q8-SWIGLU-224", "q4-SWIGLU-224", "q4-QKV-384"])
def test_extremes_pers_ql(mx, epi, N, q4):
    """The same extremes through mq8_pers_ql_kernel (K 4096, one normed token): xf = +-1 and norm_w = 127 * 2^-e on 8
    blocks (every |isum| there 520192; 8 x 520192 x 4 units < 2^24), 0 on the other 120 (all-zero activation blocks,
    d = 0), a zero d_w per row on one of the 8."""
    K, nb, e0 = 4096, 128, 11  # e0: SWIGLU's gate stays below 80
    plan_is(mx, epi, 1, N, K, q4, on_load=True, norm=True, kind="pers_ql")
    rng = np.random.default_rng(8)
    UNIT = 2.0 ** (JW0 - 1 - e0)
    active = np.array([0, 1, 17, 40, 63, 64, 99, 127])
    dw = 2.0 ** rng.integers(JW0, JW0 + 2, size=(N, nb))
    dw[np.arange(N), active[np.arange(N) % 8]] = 0.0
    if q4:
        nib = np.broadcast_to(np.repeat(np.where(np.arange(nb) % 2, 15, 0).astype(np.uint8), 32), (N, K))
        blocks, wv = R.q4_blocks(R.f16_bits(dw), nib), nib.astype(np.int16) - 8
    else:
        wv = np.full((N, K), -128, np.int16)
        blocks = R.q8_blocks(R.f16_bits(dw), wv.astype(np.int8))
    sign = 1 - 2 * rng.integers(0, 2, size=nb)
    sx = np.zeros(nb)
    sx[active] = 2.0 ** -(e0 + rng.integers(0, 2, size=8))
    xf = np.repeat(sign, 32).astype(np.float32)[None, :]
    nw = np.repeat(127 * sx, 32).astype(np.float32)
    X = (xf.astype(np.float64) * nw)
    W = wv * np.repeat(dw, 32, axis=1)
    assert float((np.abs(X) @ np.abs(W).T).max()) / UNIT < 2 ** 24
    q, d = R.quantize_act(R.norm_rows(xf, nw, 0.0))  # the form is exact: q = +-127 on the 8 blocks, d = 2^-e
    assert np.array_equal(q[0], (np.repeat(sign * (sx > 0), 32) * 127)) and np.array_equal(d[0], sx.astype(np.float32))
    kw, qa = dict(wq4=q4, act=2, norm_w=nw), None
    if epi == QKV:
        qa = kw["qkv"] = qkv_args(1, GEOM[N], "quarter")
    r = mx.q8_matmul_probe(0, epi, blocks, xf, **kw)
    check_out(mx, r, epi, X @ W.T, 1, N, f"extremes pers_ql {FMT_ID[q4]} {EPI_NAME[epi]}", qa)


# ---- onehot: a mismatch names the (n, k-block) that was read ---------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_onehot(mx, q4, fam):
    name, path, epi, M, N, _, K, on_load, want = fam
    plan_is(mx, epi, M, N, K, q4, on_load=on_load, **want)
    nb = K // 32
    n, b = np.arange(N)[:, None], np.arange(nb)[None, :]
    code = ((n * 5 + b * 3) % 16 - 8) if q4 else ((n * 131 + b * 7) % 251 - 125)
    dbits = R.f16_bits(np.ones((N, nb)))
    wv = np.repeat(code, 32, axis=1)
    blocks = R.q4_blocks(dbits, (wv + 8).astype(np.uint8)) if q4 else R.q8_blocks(dbits, wv.astype(np.int8))
    hot = (np.arange(M) * 5 + 3) % nb  # row c's one nonzero block
    xf = np.zeros((M, K), np.float32)
    xf[np.arange(M), 32 * hot + (np.arange(M) * 11) % 32] = 127.0  # d = 1, q = 127 at one place of the block
    kw = dict(wq4=q4, act=2 if on_load else 0)
    if epi == RESID:
        kw.update(resid=np.zeros((M, N), np.float32), fold_w=np.ones(N, np.float32))
    r = mx.q8_matmul_probe(path, epi, blocks, xf, **kw)
    want_out = (127 * code[:, hot].T).astype(np.float32)
    bad = np.argwhere(r.out != want_out)
    if len(bad):
        c, nn = bad[0]
        v = r.out[c, nn]
        src = np.argwhere(127 * code == v)[:4].tolist()
        pytest.fail(f"{len(bad)} wrong: row {c} output {nn} should be 127 * code[{nn}][block {hot[c]}] = "
                    f"{want_out[c, nn]}, got {v} (the code of (n, block) in {src} ...)")


# ---- quantisers ---------------------------------------------------------------------------------------------------------------
def check_norm_rows(xq, xd, x, w, eps, what):
    """Each device row equals, bit for bit over the whole row, the reference made with the nominal f32 scale or one
    of its two f32 neighbours (the order of the double sum may move (float)(sum / n) by one ulp)."""
    got_q, got_d = R.unperm_rows(xq), xd
    for c in range(x.shape[0]):
        for nudge in (0, -1, 1):
            q, d = R.quantize_act(R.norm_rows(x[c:c + 1], w, eps, nudge))
            if np.array_equal(q[0], got_q[c]) and np.array_equal(d[0], got_d[c]):
                break
        else:
            q, d = R.quantize_act(R.norm_rows(x[c:c + 1], w, eps))
            nq, ndd = int((q[0] != got_q[c]).sum()), int((d[0] != got_d[c]).sum())
            pytest.fail(f"{what}: row {c} matches no scale: {nq} q and {ndd} d differ from the nominal reference")
        MEASURED["rows"] += 1
        MEASURED["nudged"] += int(nudge != 0)
    # the cap over the file so far (expected: zero; see the module docstring), checked wherever rows are counted
    assert MEASURED["nudged"] <= 0.01 * MEASURED["rows"], f"{what}: {MEASURED['nudged']} of {MEASURED['rows']} rows"


@pytest.mark.parametrize("n", [32, 64, 992, 1024, 1056, 1088, 4096, 14336])
def test_quantize(mx, n):
    """quantize_q8_kernel on random rows, bit for bit on q and d, M 1, 17, 64, also with ld > n.  A row whose n is
    an odd multiple of 32 has no Q8_0 image: q8_perm places the last block's k 8..31 at bytes n - 16 .. n + 23,
    inside the next row (the engine demands n_embd and n_ff multiples of 64), so the probe refuses n = 32, 992 and
    1056 and the bitwise check runs on their neighbours 64, 1024 and 1088."""
    rng = np.random.default_rng(n)
    if n % 64:
        with pytest.raises(mx.MxError) as ei:
            mx.q8_matmul_probe(-1, 0, None, np.ones((1, n), np.float32), K=n)
        assert ei.value.code == mx.MX_ERR_ARG
        return
    for M in (1, 17, 64):
        for ld in (n, n + 68):
            src = (rng.standard_normal((M, ld)) * np.exp(rng.standard_normal((M, 1)) * 3)).astype(np.float32)
            r = mx.q8_matmul_probe(-1, 0, None, src, K=n, ldx=ld if ld != n else 0)
            q, d = R.quantize_act(src[:, :n])
            assert np.array_equal(R.unperm_rows(r.xq), q), f"quantize n={n} M={M} ld={ld}: q"
            assert np.array_equal(r.xd, d), f"quantize n={n} M={M} ld={ld}: d"
            assert all_ones(r.xq_guard) and all_ones(r.xd_guard)


def test_quantize_hand_made_blocks(mx):
    x = np.zeros((2, 128), np.float32)
    x[0, 0], x[0, 1:5] = 127.0, [0.5, 1.5, 2.5, -2.5]   # ties to even: 0, 2, 2, -2
    x[0, 32 + 7], x[0, 32 + 9] = -12.7, 0.1             # amax held by a negative value
    x[0, 64], x[0, 65] = 1e-9, -5e-10                   # d rounds to 0 in f16, q nonzero
    x[1, 96:128] = np.linspace(-3, 3, 32)               # (block 3 of row 0 and blocks 0..2 of row 1: all zero)
    r = mx.q8_matmul_probe(-1, 0, None, x)
    q, d = R.quantize_act(x)
    got = R.unperm_rows(r.xq)
    assert got[0, :5].tolist() == [127, 0, 2, 2, -2] and got[0, 32 + 7] == -127
    assert r.xd[0, 2] == 0.0 and got[0, 64:66].tolist() == [127, -64]
    assert not got[0, 96:].any() and r.xd[0, 3] == 0.0 and not got[1, :96].any()
    assert np.array_equal(got, q) and np.array_equal(r.xd, d)


@pytest.mark.parametrize("n", [64, 2048, 4096, 5632, 8192])
def test_norm_q8(mx, n):
    """launch_rmsnorm_q8: nslab 0..8 (3, 5, 6, 7 and n > 4096 fold first), the folded x exact from integer slabs."""
    M = 17
    rng = np.random.default_rng(n)
    e = 3
    fin_i = rng.integers(-64, 65, size=(M, n)).astype(np.int64)
    fin = (fin_i * 2.0 ** -e).astype(np.float32)
    w = (1 + 0.25 * rng.standard_normal(n)).astype(np.float32)
    sl_i = rng.integers(-16, 17, size=(8, M, n)).astype(np.int64)
    first = None
    for ns in range(9):
        x0 = ((fin_i - sl_i[:ns].sum(axis=0)) * 2.0 ** -e).astype(np.float32)
        slabs = (sl_i[:ns] * 2.0 ** -e).astype(np.float32) if ns else None
        r = mx.q8_matmul_probe(-1, 0, None, x0, act=1, norm_w=w, eps=1e-5, fold_slabs=slabs)
        what = f"norm_q8 n={n} nslab={ns}"
        assert np.array_equal(r.x, fin), f"{what}: folded x"
        check_norm_rows(r.xq, r.xd, fin, w, 1e-5, what)
        assert all_ones(r.xq_guard) and all_ones(r.xd_guard), what
        if first is None:
            first = (r.xq.copy(), r.xd.copy())
        assert np.array_equal(r.xq, first[0]) and np.array_equal(r.xd, first[1]), f"{what}: differs from nslab 0's"
    # a row_map, out of order and with a repeat
    row_map = [16, 3, 3, 0, 7, 11, 5]
    r = mx.q8_matmul_probe(-1, 0, None, fin, act=1, norm_w=w, eps=1e-5, row_map=row_map)
    assert np.array_equal(r.x, fin)
    assert np.array_equal(r.xq, first[0][row_map]) and np.array_equal(r.xd, first[1][row_map])
    print(f"norm rows matching only a neighbouring scale: {MEASURED['nudged']} of {MEASURED['rows']} so far")
    assert MEASURED["nudged"] <= 0.01 * MEASURED["rows"]


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 8])
def test_norm_q8_fold_order(mx, ns):
    """Random slabs: x + (s0 + s1 + ...) in f32, not ((x + s0) + s1) + ..."""
    M, n = 5, 2048
    rng = np.random.default_rng(ns)
    x = rng.standard_normal((M, n)).astype(np.float32)
    sl = rng.standard_normal((ns, M, n)).astype(np.float32)
    w = np.ones(n, np.float32)
    t = sl[0]
    for k in range(1, ns):
        t = t + sl[k]
    want = x + t
    r = mx.q8_matmul_probe(-1, 0, None, x, act=1, norm_w=w, eps=1e-5, fold_slabs=sl)
    assert np.array_equal(r.x.view(np.uint32), want.view(np.uint32)), f"fold order nslab={ns}"
    check_norm_rows(r.xq, r.xd, want, w, 1e-5, f"fold order nslab={ns}")
    assert MEASURED["nudged"] <= 0.01 * MEASURED["rows"]


# ---- real scales (order-sensitive) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY, ids=[f[0] for f in FAMILY])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_real_scales(mx, q4, fam):
    """Random f16 d_w, random f32 rows: float64 sum_b d_w d_x isum_b over the device's own xq / xd (on load: the
    reference quantiser's, which test_quantize pins to the device's), per output within (nblocks + 2) 2^-24 sum_b
    |d_w d_x isum_b|: one rounding of d_w * d_x and a chain of nblocks fma roundings."""
    name, path, epi, M, N, _, K, on_load, want = fam
    plan_is(mx, epi, M, N, K, q4, on_load=on_load, **want)
    rng = np.random.default_rng(90 + N + K)
    nb = K // 32
    dw16 = ((0.5 + rng.random((N, nb))) * 2.0 ** -6).astype(np.float16)
    if q4:
        nib = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
        blocks, wv = R.q4_blocks(dw16.view(np.uint16), nib), nib.astype(np.int64) - 8
    else:
        wv = rng.integers(-127, 128, size=(N, K))
        blocks = R.q8_blocks(dw16.view(np.uint16), wv.astype(np.int8))
    xf = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, nb)).repeat(32, axis=1))).astype(np.float32)
    kw = dict(wq4=q4, act=2 if on_load else 0)
    x0 = None
    if epi == RESID:
        x0 = np.zeros((M, N), np.float32)
        kw.update(resid=x0, fold_w=np.ones(N, np.float32))
    r = mx.q8_matmul_probe(path, epi, blocks, xf, **kw)
    xq, xd = (R.quantize_act(xf) if on_load else (R.unperm_rows(r.xq), r.xd))
    tot, mag = R.scaled_block_sum(wv, dw16.astype(np.float64), xq.astype(np.int64), xd.astype(np.float64))
    bound = (nb + 2) * 2.0 ** -24 * mag
    err = np.abs(r.out.astype(np.float64) - tot)
    assert not np.isnan(r.out).any()
    frac = float((err / np.maximum(bound, 1e-300)).max())
    MEASURED["real"] = max(MEASURED["real"], frac)
    print(f"real scales {name} {FMT_ID[q4]}: worst err / bound {frac:.3f}; so far {MEASURED['real']:.3f}")
    assert frac <= 1.0


# ---- norm on load, random rows (order-sensitive) ------------------------------------------------------------------------------
def real_weights(N, K, q4, seed, scale=2.0 ** -6):
    """Random f16 d_w in [0.5, 1.5) * scale and full-range q: (blocks, integer weights [N][K], d_w float64)."""
    rng = np.random.default_rng(seed)
    dw16 = ((0.5 + rng.random((N, K // 32))) * scale).astype(np.float16)
    if q4:
        nib = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
        return R.q4_blocks(dw16.view(np.uint16), nib), nib.astype(np.int64) - 8, dw16.astype(np.float64)
    wv = rng.integers(-127, 128, size=(N, K), dtype=np.int8)
    return R.q8_blocks(dw16.view(np.uint16), wv), wv.astype(np.int64), dw16.astype(np.float64)


NOL = [("ql", F32, 48, 512, (1, 2, 3, 4)), ("ql", F32, 48, 4160, (1, 2, 3, 4)), ("ql", F32, 48, 8192, (1, 2, 3, 4)),
       ("ql", QKV, 192, 512, (2, 4)), ("pers_ql", SWIGLU, 224, 4096, (1,)), ("pers_ql", QKV, 384, 4096, (1,))]


@pytest.mark.parametrize("kind,epi,N,K,Ms", NOL, ids=[f"{k}-{EPI_NAME[e]}-{n}x{kk}" for k, e, n, kk, _ in NOL])
@pytest.mark.parametrize("q4", FMT, ids=FMT_ID)
def test_norm_on_load_random(mx, q4, kind, epi, N, K, Ms):
    """Quantise on load with RMS_NORM on random rows of clearly different RMS (0.01, 30, 1, 7: at 0.01 eps = 1e-5 is a
    tenth of the mean square), a random norm_w and random f16 d_w.  The device returns no image, so the image is
    checked through the product: the reference is R.quantize_act(R.norm_rows(...)) with the scale made as the
    kernel's comment says (the double sum of the f32 per-16 partials launch_ssq writes), nominal or one of its two
    f32 neighbours, then float64 sum_b d_w d_x isum_b, bounded as test_real_scales; a row must meet the bound with
    one of the three scales.  One q off by one moves an output by d_w d_x |w|, about 2^-7 / sqrt(nblocks) of
    sum_b |d_w d_x isum_b| -- thousands of bounds.  SWIGLU: the bound on g and u carried through silu(g) u
    (|silu'| <= 1.1) plus ACTF_BAR of the value."""
    if kind == "pers_ql" and epi == QKV and not q4:
        kind = "ql"  # Q8_0 q|k|v of one token keeps the one-tile form: checked the same way
    blocks, wv, dw = real_weights(N, K, q4, 70 + N + K, 2.0 ** -11 if epi == SWIGLU else 2.0 ** -6)
    nb = K // 32
    rng = np.random.default_rng(71 + K)
    rows = (rng.standard_normal((4, K)) * np.exp(0.5 * rng.standard_normal((4, nb)).repeat(32, axis=1)) *
            np.array([0.01, 30.0, 1.0, 7.0])[:, None]).astype(np.float32)
    nw = (1 + 0.25 * rng.standard_normal(K)).astype(np.float32)
    eps = 1e-5
    for M in Ms:
        xf = rows[:M]  # M 1: the rms 0.01 row, where eps counts; M 2: 0.01 beside 30
        plan_is(mx, epi, M, N, K, q4, on_load=True, norm=True, kind=kind)
        kw, qa = dict(wq4=q4, act=2, norm_w=nw, eps=eps), None
        if epi == QKV:
            qa = kw["qkv"] = qkv_args(M, GEOM[N], "id")
        r = mx.q8_matmul_probe(0, epi, blocks, xf, **kw)
        assert all_ones(r.guard) and not np.isnan(r.out).any()
        got = r.out.astype(np.float64)
        for c in range(M):
            fracs = []
            for nudge in (0, -1, 1):
                q, d = R.quantize_act(R.norm_rows(xf[c:c + 1], nw, eps, nudge, partials=True))
                tot, mag = R.scaled_block_sum(wv, dw, q.astype(np.int64), d.astype(np.float64))
                bound = (nb + 2) * 2.0 ** -24 * mag[0]
                if epi == SWIGLU:
                    F = N // 2
                    g, u, bg, bu = tot[0, :F], tot[0, F:], bound[:F], bound[F:]
                    want = L.swiglu_ref(g, u)
                    bar = 1.1 * np.abs(u) * bg + np.abs(L.swiglu_ref(g, 1.0)) * bu + 1.1 * bg * bu + ACTF_BAR * np.abs(want)
                    fracs.append(float((np.abs(got[c] - want) / np.maximum(bar, 1e-300)).max()))
                else:
                    ncol = got.shape[1]  # QKV under the identity table: the q rows are the first n_q sums
                    fracs.append(float((np.abs(got[c] - tot[0, :ncol]) / np.maximum(bound[:ncol], 1e-300)).max()))
                if fracs[-1] <= 1.0:
                    break
            MEASURED["nol_rows"] = MEASURED.get("nol_rows", 0) + 1
            MEASURED["nol_nudged"] = MEASURED.get("nol_nudged", 0) + int(len(fracs) > 1)
            MEASURED["nol"] = max(MEASURED.get("nol", 0.0), min(fracs))
            print(f"norm on load {kind} {FMT_ID[q4]} {EPI_NAME[epi]} K={K} M={M} row {c}: err / bound {fracs} "
                  f"(worst so far {MEASURED['nol']:.3f}; {MEASURED['nol_nudged']} of {MEASURED['nol_rows']} rows nudged)")
            assert min(fracs) <= 1.0, f"row {c} of M={M}: err / bound {fracs} with the nominal scale and its neighbours"
        # the partials' double sum has at most 512 terms: its order cannot move the f32 scale but with a probability
        # of order 1e-9 per row, as for the norm kernels: the same 1% cap, expected zero
        assert MEASURED["nol_nudged"] <= 0.01 * MEASURED["nol_rows"]


# ---- mq8_pers_ql_kernel: onehot (its real-scale cases are test_norm_on_load_random's) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("epi,N,q4", [(SWIGLU, 224, False), (SWIGLU, 224, True), (QKV, 384, True)],
                         ids=["q8-SWIGLU-224", "q4-SWIGLU-224", "q4-QKV-384"])
def test_onehot_pers_ql(mx, epi, N, q4):
    """xf = +-1 (mean square exactly 1, eps 0: scale 1) and norm_w = 127 at one element of one block, 0 elsewhere:
    the image is q = +-127 there, d = 1; the weights carry a per-(n, block) code and d_w = 2^-10 (SWIGLU's gate
    stays small).  A mismatch names the blocks whose code gives the value read."""
    K, nb = 4096, 128
    plan_is(mx, epi, 1, N, K, q4, on_load=True, norm=True, kind="pers_ql")
    n, b = np.arange(N)[:, None], np.arange(nb)[None, :]
    code = ((n * 5 + b * 3) % 16 - 8) if q4 else ((n * 131 + b * 7) % 251 - 125)
    dwv = 2.0 ** -10
    dbits = R.f16_bits(np.full((N, nb), dwv))
    wv = np.repeat(code, 32, axis=1)
    blocks = R.q4_blocks(dbits, (wv + 8).astype(np.uint8)) if q4 else R.q8_blocks(dbits, wv.astype(np.int8))
    rng = np.random.default_rng(9)
    for hot in (0, 15, 16, 67, 127):
        xf = (rng.integers(0, 2, size=(1, K)) * 2 - 1).astype(np.float32)
        at = 32 * hot + (hot * 11) % 32
        nw = np.zeros(K, np.float32)
        nw[at] = 127.0
        sums = 127.0 * xf[0, at] * code * dwv  # [N][nb]: the product if block b were the one read
        kw, qa = dict(wq4=q4, act=2, norm_w=nw), None
        if epi == QKV:
            qa = kw["qkv"] = qkv_args(1, GEOM[N], "id")
        r = mx.q8_matmul_probe(0, epi, blocks, xf, **kw)
        if epi == SWIGLU:
            F = N // 2
            table = L.swiglu_ref(sums[:F], sums[F:])          # [F][nb]
            got = r.out[0].astype(np.float64)
            bar = ACTF_BAR * np.abs(table)
        else:
            table = sums[:r.out.shape[1]]
            got, bar = r.out[0].astype(np.float64), np.zeros_like(table)
        bad = np.nonzero(np.abs(got - table[:, hot]) > bar[:, hot])[0]
        if len(bad):
            nn = bad[0]
            src = np.nonzero(np.abs(got[nn] - table[nn]) <= bar[nn])[0][:6].tolist()
            pytest.fail(f"{len(bad)} wrong with block {hot} hot: output {nn} should be {table[nn, hot]}, got {got[nn]} "
                        f"(what blocks {src} of that row would give)")
        assert all_ones(r.guard)
        if epi == QKV:
            check_qkv(r, qa, sums[:, hot][None, :], f"onehot pers_ql block {hot}")


# ---- layout and side kernels ----------------------------------------------------------------------------------------------------
def test_packers_match_layout(mx):
    N, K = 96, 192
    rng = np.random.default_rng(3)
    dbits = rng.integers(0, 0x7C00, size=(N, K // 32)).astype(np.uint16)
    q = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
    nib = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
    xf = np.ones((1, K), np.float32)
    for q4, blocks, pack, v in ((False, R.q8_blocks(dbits, q), R.pack_q8_tiles, q),
                                (True, R.q4_blocks(dbits, nib), R.pack_q4_tiles, nib)):
        r = mx.q8_matmul_probe(0, F32, blocks, xf, wq4=q4, want_packed=True)
        assert np.array_equal(r.packed, pack(dbits, v)), f"PACK_ROWS q4={q4}"
        r = mx.q8_matmul_probe(0, SWIGLU, blocks, xf, wq4=q4, want_packed=True)
        assert np.array_equal(r.packed, pack(R.gate_up(dbits), R.gate_up(v))), f"PACK_GATE / PACK_UP q4={q4}"


def test_dequant_q8_tiles(mx):
    N, K = 96, 192
    rng = np.random.default_rng(4)
    d16 = ((0.5 + rng.random((N, K // 32))) * 2.0 ** rng.integers(-12, 3, size=(N, K // 32))).astype(np.float16)
    q = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
    tiles, guard = mx.q8_dequant_tiles_probe(R.q8_blocks(d16.view(np.uint16), q))
    assert np.array_equal(tiles, R.dequant_q8_bf16_tiles(d16.view(np.uint16), q))
    assert all_ones(guard)


def test_embed_q8(mx):
    V, n = 50, 2048
    rng = np.random.default_rng(5)
    d16 = ((0.5 + rng.random((V, n // 32))) * 2.0 ** -5).astype(np.float16)
    q = rng.integers(-128, 128, size=(V, n)).astype(np.int8)
    ids = [0, V - 1, 7, 7, 31]
    x, xg, ssq, sg = mx.q8_embed_probe(R.q8_blocks(d16.view(np.uint16), q), ids)
    want = q[ids].astype(np.float32) * np.repeat(d16[ids].astype(np.float32), 32, axis=1)
    assert np.array_equal(x, want) and all_ones(xg) and all_ones(sg)
    ref = L.ssq16_ref(want)
    assert (np.abs(ssq.astype(np.float64) - ref) <= 2.0 ** -22 * ref).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(mx):
    """Every invalid argument and every shape a launcher refuses gives MX_ERR_ARG with the output untouched."""
    blocks, xf = case(64, 256, False, 64)[:2]
    b4 = wcase(64, 256, True)[0]
    b192 = wcase(192, 256, False)[0]
    sentinel = np.full(4200 * 256, 0x5A5A5A5A, dtype=np.uint32)
    res = np.zeros((64, 64), np.float32)
    ones = np.ones(64, np.float32)
    qa = lambda M, **over: {**qkv_args(M, (1, 1, 64), "id"), **over}

    def refused(*a, **kw):
        out = sentinel.copy()
        with pytest.raises(mx.MxError) as ei:
            mx.q8_matmul_probe(*a, out=out.view(np.float32), **kw)
        assert ei.value.code == mx.MX_ERR_ARG, (a, ei.value)
        assert np.array_equal(out, sentinel), "a refused call wrote its output"
        return str(ei.value)

    refused(2, F32, blocks, xf[:4])                                   # path
    refused(0, 4, blocks, xf[:4])                                     # epilogue
    refused(0, F32, blocks, xf[:4], act=3)
    refused(0, F32, blocks, xf[:4], M=0)                              # M = 0
    refused(0, F32, blocks, xf[:4], M=4097)                           # M above the limit
    refused(0, F32, blocks[:, :7 * 34], xf[:4, :224])                 # K % 64
    refused(0, F32, blocks[:24], xf[:4])                              # N % 16
    refused(0, SWIGLU, blocks[:48], xf[:4])                           # SWIGLU N % 32
    refused(1, RESID, blocks, xf[:16], resid=res[:16], fold_w=ones)   # slabs outside 17..32 rows
    refused(1, RESID, blocks, xf[:33], resid=res[:33], fold_w=ones)
    refused(1, F32, blocks, xf[:17])                                  # slabs are RESID's and QKV's
    refused(1, RESID, blocks, xf[:17], resid=res[:17])                # no fold_w
    refused(0, RESID, blocks, xf[:4])                                 # RESID without resid
    refused(0, F32, blocks, xf[:5], act=2)                            # quantise on load at M 5
    big = np.zeros((64, 16448 // 32 * 34), np.uint8)
    refused(0, F32, big, np.ones((1, 16448), np.float32), act=2)      # K beyond mq8_can_quantize_on_load
    big = np.zeros((64, 8256 // 32 * 34), np.uint8)
    refused(0, F32, big, np.ones((1, 8256), np.float32), act=2, norm_w=np.ones(8256, np.float32))  # norm: K / 16 > 512
    refused(0, F32, blocks, xf[:4], act=1)                            # act 1 without norm_w
    refused(0, F32, blocks, xf[:4], act=1, norm_w=np.ones(256, np.float32), row_map=[0, 4])
    refused(0, F32, blocks, xf[:4], act=1, norm_w=np.ones(256, np.float32), row_map=[-1])
    refused(0, F32, blocks, xf[:4], act=1, norm_w=np.ones(256, np.float32), fold_slabs=np.zeros((9, 4, 256), np.float32))
    refused(0, F32, blocks, xf[:4], want_ssq=True)                    # want_ssq is RESID's
    refused(0, QKV, b192, xf[:4])                                     # QKV without its operands
    refused(0, QKV, b192, xf[:4], qkv=qa(4, rope_cs=None))
    refused(0, QKV, b192, xf[:4], qkv=qa(4, n_head=2))                # geometry does not give N
    refused(0, QKV, blocks, xf[:4], qkv={**qkv_args(4, (2, 1, 16), "id")})  # head_dim
    refused(0, QKV, b192, xf[:4], qkv=qa(4, pos=np.array([0, 1, N_CTX + 1, 2])))
    refused(0, QKV, b192, xf[:4], qkv=qa(4, pos=np.array([0, -1, 1, 2])))
    refused(0, QKV, b192, xf[:4], qkv=qa(4, slot=np.array([0, 1, 3, 2])))
    # shapes the launchers themselves refuse: reported with the launcher's name
    assert "launch_mq8 " in refused(0, SWIGLU, blocks, xf[:4], act_f32=False)            # SWIGLU without actf
    assert "launch_mq8 " in refused(0, SWIGLU, b4, xf[:4], wq4=True, act_f32=False)
    assert "launch_mq8_slab" in refused(1, RESID, wcase(64, 320, False)[0], case(64, 320, False, 32)[1][:17],
                                        resid=res[:17], fold_w=ones)                     # K % 256
    assert "launch_mq8 " in refused(0, F32, blocks, xf[:2], act=2, norm_w=np.ones(256, np.float32), np_partials=8)  # np * 16 != K
    refused(0, F32, blocks, xf[:2], act=2, norm_w=np.ones(256, np.float32), np_partials=16)   # (the probe's own range)
    refused(0, F32, blocks, xf[:2], act=2, np_partials=8)
    assert mx.q8_matmul_plan(F32, 5, 64, 256, on_load=True)["kind"] == "none"
    with pytest.raises(mx.MxError):
        mx.q8_matmul_plan(F32, 1, 64, 96)
