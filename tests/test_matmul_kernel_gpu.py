"""The bf16 matmul kernels alone (mm_kernel, mm_pers_kernel, mm_wide_kernel, gemm_kernel with its split-K form,
qkv_finish_kernel, swiglu_finish_kernel, norm_kernel, norm_generic_kernel) against exact integer references,
through mx_matmul_probe / mx_norm_probe -- no model.

Why bitwise: W holds integers in [-4, 4] and X integers in [-4, 4] times 2^-e, so every product and every
partial sum is an integer times 2^-e below 2^24 in magnitude (asserted in the builders) -- exact in f32 in ANY
summation order.  The reference is an integer matmul (tests/mm_layout.py); any element dropped, doubled or
read from the wrong place moves a result.  Comparisons are by value (==): that is bit equality except for
the sign of a zero, and a NaN (the probe's 0xFF poison, or a padded activation row leaking in) never
compares equal.  The probe fills outputs and slabs with 0xFF, appends 64 guard rows, and pads the
activation buffer with bf16 NaN rows.

Families: exact (F32 / RESID / QKV bitwise; slabs, split and guard on the split paths), onehot (names the
(n, k) read), swiglu (bf16 act within 2^-8 |ref|; f32 act within ACTF_BAR), norm_on_load, resid_ssq, norm,
refusals, cross-path equality with random (order-sensitive) operands.

Branches and the case that reaches each (kernels.hip):
  launch_mm nb=1 <16,1,*,4>: M 1/15/16, every epilogue; K 32 (15 of 16 waves empty), 96 (uneven), 512 (one tile
    per wave, tail only), 2080 (ring + tail), 4096 (full ring).  nb=2: F32 <8,4> tiles 4 / <8,1> tiles 1,2,3,6;
    RESID <4,1>; QKV <8,2> (tiles always even: head_dim 64 / 128 make q|k|v a multiple of 4 tiles, so <8,1,QKV>
    and <4,1,QKV> are unreachable with a valid geometry); SWIGLU <4,4> tiles 4 / <4,1> tiles 1,2,3,6.  nb=3,4:
    <4,2> even / <4,1> odd tiles for F32 and SWIGLU, <4,2,QKV>, <4,1,RESID>.  Norm on load: K 512 / 2048 / 8192.
  launch_mm_pers: SWIGLU tiles 1026 / 1376 / 1537 (5, 6, 7 per group, phantom tiles), 1792, 704 (K 2048), 3584
    (K 8192); RESID (4096,4096) (4096,14336) (2048,2048) (2048,5632); QKV 384 / 768 / 160 / 640 tiles.
  launch_mm_wide F32 tiles 6 <3,2>, 4 <4,1>, 2 <2,1>, 2048 <4,2>, 4096 <8,2>; SWIGLU 3, 5, 770 (<3,1> / <4,1>
    ragged), 1030 <6,1>, 1540 <7,1>, 1541 <8,1>, 2048 <4,2>; QKV / RESID wide_split cfg 0..4, splits 1, 2, 4, 8,
    RG at K 2176 / 8320 / 11008, all again with full_chain.
  launch_gemm_split: unsplit (target 0) and split (target 256) forms of all four epilogues, the slab cap, and
    gemm_rw heights 1 (small shapes), 2, 3, 4 (the heuristic's own picks) and 2..4 through MX_GEMM_RW.
  launch_norm_impl: nslab 0, 1, 2, 4, 8 (16 at n 4096) -> norm_kernel<NS, 1 | 2>; everything else generic.

Measured on MI355X over all cases of this file (the tests print each case's figure):
  f32 SwiGLU (actf) worst relative error vs float64 ....... 1.75e-7 = 2^-22.45; asserted at 4x = 7.0e-7
  norm on load, random operands: worst |err| / bar ......... 1.1e-3
  norm y: worst distance from float64 in bf16 ulps ......... 0.5000

Mutations tried on scratch copies of kernels.hip / device_common.h (none committed), each run against this
file, with the first test that failed: mm_body's last K tile dropped -> test_exact_mm[F32, 1 tile, K 32];
packed_row PACK_UP offset 8 -> 0 -> test_exact_mm[SWIGLU]; launch_wide_cfg's RG branch taking the non-RG kernel
-> test_exact_wide_split[QKV-320x8320]; kfold skipping group 1 -> test_exact_mm[RESID, K 4096];
launch_norm_impl case 8 -> <4> -> test_exact_wide_split[RESID-4096x11008] (the fold); gemm_split's finish
kernels given S - 1 -> test_exact_gemm[QKV-256-512]; qkv_cs pair index + 1 -> test_exact_mm_qkv (the mixed
table).  mm_body's column clamp removed: every test passes -- a padded column feeds only its own outputs,
which are dropped, so the NaN rows cannot reach a stored value; the clamp guards the end of the buffer.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mm_layout as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, RESID, QKV, SWIGLU = 0, 1, 2, 3
EPI_NAME = {F32: "F32", RESID: "RESID", QKV: "QKV", SWIGLU: "SWIGLU"}
ACTF_WORST = 1.75e-7          # = 2^-22.45, measured (test_swiglu_f32 prints each case's)
ACTF_BAR = 4 * ACTF_WORST     # 7.0e-7 = 2^-20.4
NOL_WORST_FRACTION = 1.1e-3   # measured (test_norm_on_load_random prints each case's)
NORM_WORST_ULP = 0.5000       # measured (test_norm prints the running worst): never past the half-ulp tie
MEASURED = {"actf": 0.0, "nol": 0.0, "norm_ulp": 0.0}


class StopOnHipError:
    """The engine binding with probes that end the session on a HIP runtime error: after a GPU fault nothing
    more is launched."""

    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        return getattr(self._e, name)

    def _call(self, fn, *a, **kw):
        try:
            return fn(*a, **kw)
        except self._e.MxError as err:
            if err.code == self._e.MX_ERR_HIP:
                pytest.exit(f"HIP error, nothing more is launched: {err}", returncode=3)
            raise

    def matmul_probe(self, *a, **kw):
        return self._call(self._e.matmul_probe, *a, **kw)

    def norm_probe(self, *a, **kw):
        return self._call(self._e.norm_probe, *a, **kw)


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return StopOnHipError(engine)


# ---- inputs ---------------------------------------------------------------------------------------------------
BF_INT = L.bf16_bits(np.arange(-4, 5, dtype=np.float32), exact=True)  # bf16 bits of -4..4


def xexp(K, extra=0):
    """e with sums of K products of two uniform [-4, 4] integers (sigma = 6.7 sqrt(K)) times 2^-e of order 8."""
    return max(0, int(round(np.log2(6.7 * np.sqrt(K) / 8)))) + extra


def int_w(N, K, seed):
    wi = np.random.default_rng(seed).integers(-4, 5, size=(N, K), dtype=np.int8)
    return wi, BF_INT[wi + 4]


def int_x(M, K, e, seed):
    """(integers [M][K], bf16 bits of integers * 2^-e); 16 K < 2^24 keeps every partial sum exact in f32."""
    assert 16 * K < 2 ** 24
    xi = np.random.default_rng(seed).integers(-4, 5, size=(M, K), dtype=np.int8)
    return xi, L.bf16_bits(xi.astype(np.float32) * np.float32(2.0 ** -e), exact=True)


def int_f32(shape, e, seed, lo=-4, hi=4):
    v = np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.int64)
    return v, (v * 2.0 ** -e).astype(np.float32)


def rand_bf16(shape, seed):
    """Random bf16 bits: random sign and mantissa, exponents 2^-7 .. 2^0 -- sums whose rounding depends on order."""
    r = np.random.default_rng(seed).integers(0, 1 << 16, size=shape, dtype=np.uint16)
    return (r & np.uint16(0x83FF)) | np.uint16(0x3C00)


@functools.lru_cache(maxsize=2)
def case(N, K, mrows=64, extra=0):
    """Integer W [N][K], X [mrows][K] and the exact product [mrows][N] (int64, in units of 2^-e), made once."""
    e = xexp(K, extra)
    wi, wb = int_w(N, K, 1000 + N + K)
    xi, xb = int_x(mrows, K, e, 2000 + N + K)
    ref = L.int_matmul(wi, xi)
    assert np.abs(ref).max() < 2 ** 24
    for a in (wb, xb, ref, wi):
        a.setflags(write=False)
    return wb, xb, ref, e, wi


def all_ones(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


# ---- q|k|v geometry ---------------------------------------------------------------------------------------------
N_CTX = 40


def n_slots_for(M):
    return 3 if M <= 64 else 16  # 40 positions each: room for 120 / 640 rows


def qkv_rows(M):
    i, ns = np.arange(M), n_slots_for(M)
    slot, pos = i % ns, (7 * (i // ns) + 3) % N_CTX  # every row its own (slot, position)
    assert len(set(zip(slot.tolist(), pos.tolist()))) == M
    if M >= 5:
        pos[2] = N_CTX  # a row at n_ctx stores nothing
    return pos.astype(np.int32), slot.astype(np.int32)


def rope_table(D, kind):
    cs = np.zeros((N_CTX, D // 2, 2), dtype=np.float32)
    if kind == "id":
        cs[..., 0] = 1
    elif kind == "quarter":
        cs[..., 1] = 1
    else:  # mixed: identity or quarter turn by (position + pair) parity: pins the table's position and pair index
        par = (np.arange(N_CTX)[:, None] + np.arange(D // 2)[None, :]) % 2
        cs[..., 0], cs[..., 1] = 1 - par, par
    return cs


def qkv_args(M, geom, kind):
    nh, nkv, D = geom
    pos, slot = qkv_rows(M)
    S = L.kv_layout.ctx_stride(N_CTX)
    elems = n_slots_for(M) * nkv * S * D
    init = ((np.arange(elems, dtype=np.int64) * 37) % 2001 - 1000).astype(np.float16).view(np.uint16)
    return dict(n_head=nh, n_head_kv=nkv, head_dim=D, n_ctx=N_CTX, n_slots=n_slots_for(M), pos=pos, slot=slot,
                rope_cs=rope_table(D, kind), kcache=init, vcache=init[::-1].copy())


def check_qkv(r, qa, s, what):
    """q rows and both caches against the float64 split of the exact product s [M][N]."""
    nh, nkv, D = qa["n_head"], qa["n_head_kv"], qa["head_dim"]
    pos, slot = qa["pos"], qa["slot"]
    M = len(pos)
    stored = pos < N_CTX
    q, k, v = L.qkv_ref(s, nh, nkv, D, np.minimum(pos, N_CTX - 1), qa["rope_cs"])
    assert np.array_equal(r.out[stored], q[stored].astype(np.float32)), f"{what}: q"
    assert all_ones(r.out[~stored]), f"{what}: q of a row at n_ctx was written"
    S = L.kv_layout.ctx_stride(N_CTX)
    K0, V0 = L.untile_caches(qa["kcache"], qa["vcache"], qa["n_slots"], nkv, S, D)
    K0, V0 = K0.view(np.float16).copy(), V0.view(np.float16).copy()
    for i in range(M):
        if stored[i]:
            K0[slot[i], :, pos[i], :] = k[i].reshape(nkv, D).astype(np.float16)
            V0[slot[i], :, pos[i], :] = v[i].reshape(nkv, D).astype(np.float16)
    K1, V1 = L.untile_caches(r.kcache, r.vcache, qa["n_slots"], nkv, S, D)
    assert np.array_equal(K1.view(np.float16), K0), f"{what}: K cache (stores, or an element that was not this row's)"
    assert np.array_equal(V1.view(np.float16), V0), f"{what}: V cache"


GEOM = {192: (1, 1, 64), 256: (2, 1, 64), 320: (3, 1, 64), 384: (1, 1, 128), 512: (4, 2, 64), 768: (4, 4, 64),
        6144: (32, 8, 128), 12288: (32, 32, 128), 2560: (32, 4, 64), 10240: (64, 8, 128)}


# ---- one exact run ----------------------------------------------------------------------------------------------
def run_exact(mx, path, epi, N, K, M, *, rope="id", want_ssq=False, mrows=64, target=0, slab_floats=0):
    """Launch (path, epi) on the shared integer case and compare with the integer reference.  Returns the
    probe result (and the exact final residual for RESID)."""
    wb, xb, ref, e, _ = case(N, K, mrows, 1 if epi == SWIGLU else 0)
    s = ref[:M] * 2.0 ** -e  # float64, exact
    what = f"path {path} {EPI_NAME[epi]} M={M} N={N} K={K}"
    kw = dict(want_slabs=path >= 2 and epi != F32, target=target, slab_floats=slab_floats)
    final = None
    if epi == F32:
        r = mx.matmul_probe(path, F32, wb, xb[:M], **kw)
        assert np.array_equal(r.out, s.astype(np.float32)), what
    elif epi == RESID:
        x0i, x0 = int_f32((M, N), e, 3000 + M + N)
        r = mx.matmul_probe(path, RESID, wb, xb[:M], resid=x0, want_ssq=want_ssq, **kw)
        final = (x0i + ref[:M]) * 2.0 ** -e
        assert np.array_equal(r.out, final.astype(np.float32)), what
    elif epi == QKV:
        qa = qkv_args(M, GEOM[N], rope)
        r = mx.matmul_probe(path, QKV, wb, xb[:M], qkv=qa, **kw)
        check_qkv(r, qa, s, f"{what} rope {rope}")
    else:
        F = N // 2
        g, u = s[:, :F], s[:, F:]
        assert np.abs(g).max() <= 32
        want = L.swiglu_ref(g, u)
        r = mx.matmul_probe(path, SWIGLU, wb, xb[:M], **kw)
        got = L.bf16_f32(r.out).astype(np.float64)
        assert (np.abs(got - want) <= 2.0 ** -8 * np.abs(want)).all(), f"{what}: bf16 act"
    assert all_ones(r.guard), f"{what}: guard rows written"
    if path in (2, 3) and epi in (QKV, RESID):
        kg = mx.matmul_plan(epi, M, N, K)["kgroups"]
        assert r.split == (1 if path == 3 else kg), f"{what}: split {r.split}, canon_kgroups {kg}"
        assert r.slabs.shape == (r.split, M, N)
        assert not (r.slabs.view(np.uint32) == 0xFFFFFFFF).any(), f"{what}: slab element never written"
        assert np.array_equal(r.slabs.astype(np.float64).sum(axis=0), s), f"{what}: slabs do not sum to the product"
    r.final = final
    return r


# ---- exact: launch_mm ---------------------------------------------------------------------------------------------
MM_M = [1, 15, 16, 17, 32, 33, 48, 49, 64]
MM_K = [32, 96, 512, 2080, 4096]


@pytest.mark.parametrize("K", MM_K)
@pytest.mark.parametrize("ntiles", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("epi", [F32, RESID, SWIGLU])
def test_exact_mm(mx, epi, ntiles, K):
    for M in MM_M:
        run_exact(mx, 0, epi, 16 * ntiles, K, M)


@pytest.mark.parametrize("K", MM_K)
@pytest.mark.parametrize("N", [192, 320, 384])
def test_exact_mm_qkv(mx, N, K):
    for M in MM_M:
        for rope in ("id", "quarter", "mixed"):
            run_exact(mx, 0, QKV, N, K, M, rope=rope)


# ---- exact: launch_mm_pers (the full-size matrices its instantiations are keyed to) ---------------------------------
PERS = ([(SWIGLU, 16 * nt, 4096) for nt in (1026, 1376, 1537, 1792)] + [(SWIGLU, 16 * 704, 2048), (SWIGLU, 16 * 3584, 8192)] +
        [(RESID, 4096, 4096), (RESID, 4096, 14336), (RESID, 2048, 2048), (RESID, 2048, 5632)] +
        [(QKV, 6144, 4096), (QKV, 12288, 4096), (QKV, 2560, 2048), (QKV, 10240, 8192)])
PERS_M = [1, 4, 5, 16]


@pytest.mark.parametrize("epi,N,K", PERS, ids=[f"{EPI_NAME[e]}-{n}x{k}" for e, n, k in PERS])
def test_pers(mx, epi, N, K):
    """One test per shape so that its weights (up to 0.9 GB for the 57344 x 8192 gate/up: a few seconds of
    numpy on the host, not of GPU) are built once.
    exact: integer operands, bitwise against the reference (SWIGLU: the bf16 bar), RESID with and without ssq.
    equal: 'the same summation order per tile as mm_kernel, so results are bit-identical' (comment above
    mm_pers_kernel) -- integer weights with random bf16 activations, where the order of the K slices changes
    the rounding; launch_mm and launch_mm_pers must agree bitwise.
    norm on load (not RESID): the exact form of test_norm_on_load_exact at M 1..4."""
    assert mx.matmul_plan(epi, 1, N, K)["pers_ok"]
    for M in PERS_M:
        if epi == QKV:
            for rope in ("id", "quarter"):
                run_exact(mx, 1, QKV, N, K, M, rope=rope, mrows=16)
        elif epi == RESID:
            for ssq in (False, True):
                r = run_exact(mx, 1, RESID, N, K, M, want_ssq=ssq, mrows=16)
                if ssq:
                    check_ssq(r, f"pers RESID M={M} N={N} K={K}")
        else:
            run_exact(mx, 1, SWIGLU, N, K, M, mrows=16)
    wb = case(N, K, 16, 1 if epi == SWIGLU else 0)[0]
    for M in PERS_M:
        xb = rand_bf16((M, K), 77 + M)
        kw = {}
        if epi == RESID:
            kw["resid"] = np.random.default_rng(5).standard_normal((M, N)).astype(np.float32)
            kw["want_ssq"] = True
        if epi == QKV:
            kw["qkv"] = qkv_args(M, GEOM[N], "mixed")
        a, b = mx.matmul_probe(0, epi, wb, xb, **kw), mx.matmul_probe(1, epi, wb, xb, **kw)
        same_result(a, b, epi, f"pers vs mm {EPI_NAME[epi]} M={M} N={N} K={K}")
        if epi == RESID:
            assert np.array_equal(a.ssq.view(np.uint32), b.ssq.view(np.uint32))
    if epi != RESID:
        nol_exact(mx, 1, epi, N, K, 16)


def same_result(a, b, epi, what):
    assert np.array_equal(a.out.view(np.uint32 if a.out.dtype == np.float32 else np.uint16),
                          b.out.view(np.uint32 if b.out.dtype == np.float32 else np.uint16)), what
    if epi == QKV:
        assert np.array_equal(a.kcache, b.kcache) and np.array_equal(a.vcache, b.vcache), f"{what}: caches"
    if epi != QKV:
        assert not np.isnan(a.out.astype(np.float32) if a.out.dtype == np.float32 else L.bf16_f32(a.out)).any(), what


# ---- exact: launch_mm_wide ----------------------------------------------------------------------------------------
WIDE_M = [17, 32, 33, 64]


@pytest.mark.parametrize("ntiles", [6, 4, 2, 2048, 4096])
def test_exact_wide_f32(mx, ntiles):
    for M in WIDE_M + ([1, 16] if ntiles == 6 else []):
        run_exact(mx, 2, F32, 16 * ntiles, 128, M)
    run_exact(mx, 3, F32, 16 * ntiles, 128, 33)


@pytest.mark.parametrize("ntiles", [3, 5, 770, 1030, 1540, 1541, 2048])
def test_exact_wide_swiglu(mx, ntiles):
    for M in WIDE_M + ([1, 16] if ntiles == 5 else []):
        run_exact(mx, 2, SWIGLU, 16 * ntiles, 128, M)
    run_exact(mx, 3, SWIGLU, 16 * ntiles, 128, 33)


# (epi, N, K): wide_split cfg and split (tests/test_mm_layout.py pins canon_kgroups for these)
WIDE_SPLIT = [
    (QKV, 192, 128),     # cfg 3 <3,1>, split 1
    (QKV, 192, 1024),    # cfg 3, split 2
    (QKV, 192, 4096),    # cfg 3, split 4
    (QKV, 256, 2048),    # cfg 0 <4,2>, split 4
    (QKV, 320, 2048),    # cfg 1 <2,1>, split 4
    (QKV, 320, 8320),    # cfg 2 <4,1> (K > 8192), split 4, RG (65-tile ranges)
    (QKV, 320, 2176),    # cfg 1, split 4, RG (17-tile ranges)
    (RESID, 64, 128),    # cfg 1, split 1
    (RESID, 64, 1024),   # split 2
    (RESID, 64, 2048),   # split 4
    (RESID, 64, 4096),   # split 4
    (RESID, 64, 2176),   # split 4, RG
    (RESID, 64, 8320),   # cfg 2, split 4, RG
    (RESID, 128, 8320),  # cfg 4 <4,2>, split 8, RG (32.5-tile ranges)
    (RESID, 128, 8704),  # cfg 4, split 8, 34-tile ranges (RG: a last chunk of 2 tiles)
    (RESID, 128, 16384), # cfg 4, split 8, 64-tile ranges (non-RG)
    (RESID, 4096, 11008),  # Llama-2-7B ffn_down: cfg 4, split 8, 43-tile ranges (RG)
]


@pytest.mark.parametrize("epi,N,K", WIDE_SPLIT, ids=[f"{EPI_NAME[e]}-{n}x{k}" for e, n, k in WIDE_SPLIT])
def test_exact_wide_split(mx, epi, N, K):
    big = N * K > (1 << 24)
    for path in (2, 3):
        for M in ([33] if big else WIDE_M + ([1, 16] if K == 2048 else [])):
            for rope in (("id", "quarter") if epi == QKV else ("id",)):
                run_exact(mx, path, epi, N, K, M, rope=rope)


# ---- exact: launch_gemm_split ---------------------------------------------------------------------------------------
GEMM_M = [65, 255, 256, 257, 300, 513]


def gemm_case(mx, epi, N, K, M, target, slab_floats=None, mrows=513):
    sf = 16 * M * N if slab_floats is None else slab_floats
    r = run_exact(mx, 4, epi, N, K, M, mrows=mrows, target=target, slab_floats=sf)
    written = int((r.slabs.view(np.uint32) != 0xFFFFFFFF).sum()) if r.slabs is not None else 0
    assert written % (M * N) == 0, "a partial slab was written in part"
    S = written // (M * N)
    if epi == RESID:
        assert r.split == (S if S else 0)
    if S:
        c = case(N, K, mrows, 1 if epi == SWIGLU else 0)
        slabs = r.slabs[:S * M * N].reshape(S, M, N).astype(np.float64)
        tot = slabs.sum(axis=0)
        ref = c[2][:M] * 2.0 ** -c[3]
        if epi == SWIGLU:  # slab rows are in packed (interleaved) order
            F = N // 2
            ref = L.interleave_gate_up(ref[:, :F].T, ref[:, F:].T).T
        assert np.array_equal(tot, ref), "slabs do not sum to the product"
    return S


@pytest.mark.parametrize("K", [64, 512, 2048])
@pytest.mark.parametrize("N", [256, 512, 768])
@pytest.mark.parametrize("epi", [F32, RESID, QKV, SWIGLU])
def test_exact_gemm(mx, epi, N, K):
    assert mx.matmul_plan(epi, 65, N, K)["gemm_ok"]
    for M in GEMM_M:
        assert gemm_case(mx, epi, N, K, M, 0) == 0  # target 0: never split
        S = gemm_case(mx, epi, N, K, M, 256)
        # gemm_split: largest power of two with 2 S base <= 256 + base / 2, 8 S <= K / 64 (F32 never splits)
        base = (N // 256) * ((M + 255) // 256)
        want = 1
        while want < 16 and 2 * want * base <= 256 + base // 2 and 2 * want * 4 <= K // 64:
            want *= 2
        assert S == (0 if epi == F32 or want == 1 else want), (M, S, want)


@pytest.mark.parametrize("epi", [RESID, QKV, SWIGLU])
def test_gemm_split_capped_by_slab_space(mx, epi):
    M, N, K = 65, 256, 2048
    assert gemm_case(mx, epi, N, K, M, 256) == 8  # 32 K steps of 64: 8 ranges of 4
    assert gemm_case(mx, epi, N, K, M, 256, slab_floats=5 * M * N) == 4
    assert gemm_case(mx, epi, N, K, M, 256, slab_floats=3 * M * N) == 2
    assert gemm_case(mx, epi, N, K, M, 256, slab_floats=2 * M * N - 1) == 0


def gemm_rw_heuristic(N, nm):
    """gemm_rw as kernels.hip states it: fewest (rounds of 256 blocks) x (height + 1), ties to the taller."""
    best, cost = 4, None
    for rw in (4, 3, 2, 1):
        if N % (64 * rw):
            continue
        c = -(-(N // (64 * rw) * nm) // 256) * (rw + 1)
        if cost is None or c < cost:
            best, cost = rw, c
    return best


@pytest.mark.parametrize("N,M,rw", [(1280, 3073, 2), (3072, 2561, 3), (11008, 513, 4)])
def test_exact_gemm_row_block_heights(mx, N, M, rw):
    """The heuristic's own picks of heights 2, 3 and 4: the shapes with the fewest N x (token blocks) among
    N <= 16384 (a multiple of 256), M <= 4096 that reach each height (enumerated with gemm_rw_heuristic); every
    shape of test_exact_gemm takes height 1."""
    assert gemm_rw_heuristic(N, (M + 255) // 256) == rw
    assert all(gemm_rw_heuristic(n, nm) == 1 for n in (256, 512, 768) for nm in range(1, 4))
    for epi in (F32, RESID):
        run_exact(mx, 4, epi, N, 64, M, mrows=M)


def child_gemm_rw():  # the child of test_exact_gemm_forced_heights: MX_GEMM_RW is read once per process
    from llama_p2p_amd import engine

    engine.lib()
    for epi in (F32, RESID, QKV, SWIGLU):
        run_exact(engine, 4, epi, 768, 512, 300, mrows=300)
    print("child ok")


@pytest.mark.parametrize("rw", [2, 3, 4])
def test_exact_gemm_forced_heights(rw):
    """Heights 2, 3 and 4 at a small shape (N 768 = 12 x 64 = 6 x 128 = 4 x 192 = 3 x 256), reachable there only
    through MX_GEMM_RW -- read once per process, so each runs in a fresh child."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import test_matmul_kernel_gpu as T\nT.child_gemm_rw()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MX_GEMM_RW=str(rw)),
                       capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or "mx error -2" in r.stderr:
        pytest.exit(f"the child met a GPU error, nothing more is launched: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- onehot: a mismatch names the (n, k) that was read ----------------------------------------------------------------
@pytest.mark.parametrize("path,M,N,K", [(0, 16, 96, 2080), (0, 64, 96, 2080), (1, 16, 2048, 2048), (2, 64, 96, 2176),
                                        (3, 64, 96, 2176), (4, 300, 256, 2048)])
def test_onehot(mx, path, M, N, K):
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    code = ((n * 131 + k) % 251 - 125).astype(np.float32)
    wb = L.bf16_bits(code, exact=True)
    hot = (np.arange(M) * 67 + 31) % K  # row c reads column hot[c]
    x = np.zeros((M, K), dtype=np.float32)
    x[np.arange(M), hot] = 1
    epi = RESID if path in (1, 4) else F32  # path 4: RESID splits (target 256) and is folded
    kw = dict(resid=np.zeros((M, N), dtype=np.float32)) if epi == RESID else {}
    if path == 4:
        kw.update(target=256, slab_floats=16 * M * N)
    r = mx.matmul_probe(path, epi, wb, L.bf16_bits(x, exact=True), **kw)
    want = code[:, hot].T
    bad = np.argwhere(r.out != want)
    if len(bad):
        c, nn = bad[0]
        v = r.out[c, nn]
        src = np.argwhere(code == v)[:4].tolist()
        pytest.fail(f"{len(bad)} wrong: row {c} output {nn} should be W[{nn}][{hot[c]}] = {want[c, nn]}, got {v} "
                    f"(the code of (n, k) in {src} ...)")


# ---- swiglu, f32 output ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,N,K,M", [(0, 96, 4096, 16), (0, 64, 512, 64), (0, 48, 2080, 33), (1, 16 * 704, 2048, 16),
                                        (1, 16 * 1792, 4096, 5), (2, 16 * 770, 128, 64), (2, 16 * 5, 128, 17),
                                        (3, 16 * 2048, 128, 33), (4, 512, 512, 300)])
def test_swiglu_f32(mx, path, N, K, M):
    """The f32 (actf) output against float64 silu(g) * u of the exact sums.  Its error is expf's and a
    division's: measured worst over all cases here ACTF_WORST (relative), asserted at 4x that -- far below
    2^-12, which a bf16-rounded value written to actf could not meet."""
    mrows = 300 if path == 4 else 64 if path != 1 else 16
    wb, xb, ref, e, _ = case(N, K, mrows, 1)
    s = ref[:M] * 2.0 ** -e
    F = N // 2
    want = L.swiglu_ref(s[:, :F], s[:, F:])
    assert np.abs(s[:, :F]).max() <= 32
    r = mx.matmul_probe(path, SWIGLU, wb, xb[:M], act_f32=True)
    got = r.out.astype(np.float64)
    nz = want != 0
    assert (got[~nz] == 0).all()
    rel = float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max())
    MEASURED["actf"] = max(MEASURED["actf"], rel)
    print(f"actf worst relative error: this case {rel:.3e} = 2^{np.log2(max(rel, 1e-300)):.2f}; so far "
          f"{MEASURED['actf']:.3e}")
    assert all_ones(r.guard)
    assert ACTF_BAR < 2.0 ** -12
    assert rel <= ACTF_BAR


# ---- norm on load -------------------------------------------------------------------------------------------------
def nol_operands(M, K, exact):
    rng = np.random.default_rng(900 + M + K)
    if exact:
        # x = +-1: mean square exactly 1, 1.0f / sqrtf(1.0f) exactly 1; w = 2^(j - sh), j in -2..2:
        # bf16((x * 1) * w) = +-w exactly.  Returns the operand as integers in units of 2^-(2 + sh).
        sh = xexp(K) + 1  # the operand's rms is 8.3 units against int_x's 2.6: sums of order 4, |g| <= 32
        xf = rng.integers(0, 2, size=(M, K)).astype(np.float32) * 2 - 1
        j = rng.integers(-2, 3, size=K)
        return xf, (2.0 ** (j - sh)).astype(np.float32), 0.0, xf.astype(np.int64) * (2 ** (j + 2))[None, :], 2.0 ** -(2 + sh)
    xf = rng.standard_normal((M, K)).astype(np.float32) * np.float32(3.0)
    return xf, (1 + 0.25 * rng.standard_normal(K)).astype(np.float32), 1e-5, None, None


def nol_exact(mx, path, epi, N, K, mrows):
    c = case(N, K, mrows, 1 if epi == SWIGLU else 0)
    wb, wi = c[0], c[4]
    for M in (1, 2, 3, 4):
        xf, nw, eps, bi, unit = nol_operands(M, K, True)
        s = L.int_matmul(wi, bi) * unit
        what = f"norm on load path {path} {EPI_NAME[epi]} M={M} N={N} K={K}"
        if epi == F32:
            r = mx.matmul_probe(path, F32, wb, xf=xf, norm_w=nw, eps=eps)
            assert np.array_equal(r.out, s.astype(np.float32)), what
        elif epi == QKV:
            qa = qkv_args(M, GEOM[N], "quarter")
            r = mx.matmul_probe(path, QKV, wb, xf=xf, norm_w=nw, eps=eps, qkv=qa)
            check_qkv(r, qa, s, what)
        else:
            F = N // 2
            assert np.abs(s[:, :F]).max() <= 32
            want = L.swiglu_ref(s[:, :F], s[:, F:])
            r = mx.matmul_probe(path, SWIGLU, wb, xf=xf, norm_w=nw, eps=eps)
            got = L.bf16_f32(r.out).astype(np.float64)
            assert (np.abs(got - want) <= 2.0 ** -8 * np.abs(want)).all(), what
        assert all_ones(r.guard), what


@pytest.mark.parametrize("epi,N,K", [(F32, 48, 512), (F32, 48, 2048), (F32, 48, 8192), (SWIGLU, 96, 2048), (QKV, 192, 2048),
                                     (QKV, 320, 512)])
def test_norm_on_load_exact(mx, epi, N, K):
    """launch_mm with RMS_NORM on load, M 1..4 (launch_mm_pers: inside test_pers): xf = +-1, eps 0, norm_w powers
    of two -- the normalised operand is exact, so the product is again checked bitwise."""
    assert mx.matmul_plan(epi, 4, N, K)["norm_on_load_ok"]
    nol_exact(mx, 0, epi, N, K, 64)


@pytest.mark.parametrize("path,N,K", [(0, 48, 512), (0, 48, 2048), (0, 48, 8192), (1, 6144, 4096), (1, 2560, 2048),
                                      (1, 10240, 8192)])
def test_norm_on_load_random(mx, path, N, K):
    """Random xf, eps 1e-5, against float64 with the operand rounded to bf16 in the reference: per output
    |err| <= 2^-8 sum_k |w_nk b_k| (each operand at most one bf16 ulp off when the f32 scale differs in its last
    bit).  Measured worst |err| / bar over these cases: NOL_WORST_FRACTION."""
    epi = F32 if path == 0 else QKV
    wb = case(N, K, 16 if path == 1 else 64)[0]
    w64 = L.bf16_f32(wb).astype(np.float64)
    for M in (1, 2, 3, 4):
        xf, nw, eps, _, _ = nol_operands(M, K, False)
        b = L.bf16_round(L.rmsnorm_ref(xf, nw, eps)).astype(np.float64)
        want, bar = b @ w64.T, 2.0 ** -8 * (np.abs(b) @ np.abs(w64).T)
        if epi == F32:
            got = mx.matmul_probe(path, F32, wb, xf=xf, norm_w=nw, eps=eps).out.astype(np.float64)
        else:  # v rows take no RoPE and q rows none under the identity table: compare q, which is f32
            qa = qkv_args(M, GEOM[N], "id")
            r = mx.matmul_probe(path, QKV, wb, xf=xf, norm_w=nw, eps=eps, qkv=qa)
            nq = qa["n_head"] * qa["head_dim"]
            keep = qa["pos"] < N_CTX
            got, want, bar = r.out.astype(np.float64)[keep], want[keep, :nq], bar[keep, :nq]
        frac = float((np.abs(got - want) / bar).max())
        MEASURED["nol"] = max(MEASURED["nol"], frac)
        print(f"norm on load worst |err| / bar: this case {frac:.2e}; so far {MEASURED['nol']:.2e}")
        assert frac <= 1.0, (M, frac)


# ---- RESID sum-of-squares partials ----------------------------------------------------------------------------------
def check_ssq(r, what):
    """ssq[c][t] within 2^-22 relative of the float64 sum of squares of the exact updated residual: squares
    rounded once to f32 (2^-24 each), a double sum, one rounding to f32 (2^-24)."""
    want = L.ssq16_ref(r.final)
    got = r.ssq.astype(np.float64)
    assert not np.isnan(got).any(), f"{what}: ssq partial never written"
    assert (np.abs(got - want) <= 2.0 ** -22 * want).all(), f"{what}: ssq partials"


@pytest.mark.parametrize("N,K", [(16, 32), (48, 512), (96, 2080), (64, 4096)])
def test_resid_ssq_mm(mx, N, K):
    for M in MM_M:
        check_ssq(run_exact(mx, 0, RESID, N, K, M, want_ssq=True), f"mm RESID ssq M={M} N={N} K={K}")


# ---- norm -----------------------------------------------------------------------------------------------------------
NORM_NSLAB = [0, 1, 2, 3, 4, 5, 8, 16]


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("n", [64, 2048, 4096, 5632, 8192, 16384])
def test_norm(mx, n, M):
    """launch_resid_norm over every slab count: integer slabs fold into x exactly; y within one bf16 ulp of
    float64 and bitwise equal across nslab for the same final x (the batch-invariance statement above
    norm_kernel: norm_kernel<NS, 1>, <NS, 2> and the generic kernel agree).  Worst distance: NORM_WORST_ULP."""
    rng = np.random.default_rng(n + M)
    e = 3
    fin_i = rng.integers(-64, 65, size=(M, n)).astype(np.int64)
    fin = (fin_i * 2.0 ** -e)
    w = (1 + 0.25 * rng.standard_normal(n)).astype(np.float32)
    want = L.rmsnorm_ref(fin, w, 1e-5)
    ulp = L.bf16_ulp(want)
    sl_i = rng.integers(-16, 17, size=(16, M, n)).astype(np.int64)
    y0 = None
    for ns in NORM_NSLAB:
        x0 = ((fin_i - sl_i[:ns].sum(axis=0)) * 2.0 ** -e).astype(np.float32)
        slabs = (sl_i[:ns] * 2.0 ** -e).astype(np.float32) if ns else None
        xo, xg, y, yg = mx.norm_probe(x0, slabs, w, eps=1e-5)
        what = f"norm n={n} M={M} nslab={ns}"
        assert np.array_equal(xo, fin.astype(np.float32)), f"{what}: folded x"
        assert all_ones(xg) and all_ones(yg), f"{what}: guard rows"
        d = float((np.abs(L.bf16_f32(y).astype(np.float64) - want) / ulp).max())
        MEASURED["norm_ulp"] = max(MEASURED["norm_ulp"], d)
        assert d <= 1.0, f"{what}: y {d:.3f} bf16 ulp from float64"
        if y0 is None:
            y0 = y.copy()
        assert np.array_equal(y, y0), f"{what}: y differs from nslab 0's for the same x"
        # fold only (no y), as the engine's last fold of a stage
        xo2, xg2, _, _ = mx.norm_probe(x0, slabs, None)
        assert np.array_equal(xo2, fin.astype(np.float32)) and all_ones(xg2), f"{what}: fold without y"
    print(f"norm worst bf16-ulp distance so far {MEASURED['norm_ulp']:.4f}")


@pytest.mark.parametrize("n", [64, 4096, 5632, 8192])
def test_norm_row_map(mx, n):
    rows = 20
    rng = np.random.default_rng(n)
    x = (rng.integers(-64, 65, size=(rows, n)) * 0.125).astype(np.float32)
    w = (1 + 0.25 * rng.standard_normal(n)).astype(np.float32)
    row_map = [19, 3, 3, 0, 7, 11, 5]  # out of order, with a repeat
    xo, xg, y, yg = mx.norm_probe(x, None, w, row_map=row_map, eps=1e-5)
    assert np.array_equal(xo, x) and all_ones(xg) and all_ones(yg)
    _, _, yall, _ = mx.norm_probe(x, None, w, eps=1e-5)
    assert np.array_equal(y, yall[row_map])
    want = L.rmsnorm_ref(x[row_map], w, 1e-5)
    assert (np.abs(L.bf16_f32(y).astype(np.float64) - want) <= L.bf16_ulp(want)).all()


# ---- cross-path equality (batch invariance, at the kernel) ---------------------------------------------
CROSS = [(F32, 96, 4096), (F32, 64, 128), (SWIGLU, 96, 4096), (SWIGLU, 160, 1024), (RESID, 64, 1024), (RESID, 64, 4096),
         (RESID, 64, 2176), (RESID, 128, 8320), (RESID, 64, 8320), (QKV, 192, 4096), (QKV, 256, 2048), (QKV, 320, 2176),
         (QKV, 320, 1024)]


@pytest.mark.parametrize("epi,N,K", CROSS, ids=[f"{EPI_NAME[e]}-{n}x{k}" for e, n, k in CROSS])
def test_rows_do_not_depend_on_row_count_or_path(mx, epi, N, K):
    """Random bf16 operands (the order of the sums matters): a row's result from launch_mm at M = 1 equals the
    same row's from launch_mm at M = 16 and from launch_mm_wide at M = 17, 33, 64."""
    wb = rand_bf16((N, K), 11 + N + K)
    xb = rand_bf16((64, K), 12 + N + K)
    resid = np.random.default_rng(13).standard_normal((64, N)).astype(np.float32)

    pos64, slot64 = qkv_rows(64)  # row i keeps its (slot, position) at every M; row 2 sits at n_ctx

    def rows(path, M):
        kw, qa = {}, None
        if epi == RESID:
            kw["resid"] = resid[:M]
        if epi == QKV:
            qa = qkv_args(M, GEOM[N], "mixed")
            qa["pos"], qa["slot"] = pos64[:M].copy(), slot64[:M].copy()
            kw["qkv"] = qa
        r = mx.matmul_probe(path, epi, wb, xb[:M], **kw)
        res = [r.out.view(np.uint32 if r.out.dtype == np.float32 else np.uint16)]
        if epi == QKV:  # each row's own K / V entries (a row at n_ctx: an entry nobody writes)
            S = L.kv_layout.ctx_stride(N_CTX)
            K1, V1 = L.untile_caches(r.kcache, r.vcache, qa["n_slots"], qa["n_head_kv"], S, qa["head_dim"])
            p = np.minimum(qa["pos"], N_CTX - 1)
            res += [K1[qa["slot"], :, p], V1[qa["slot"], :, p]]
        else:
            assert not (res[0] == (0xFFFFFFFF if res[0].dtype == np.uint32 else 0xFFFF)).any()
        return res

    one, full = rows(0, 1), rows(0, 16)
    for path, M in [(0, 16), (2, 17), (2, 33), (2, 64)]:
        got = rows(path, M)
        for a, b in zip(one, got):
            assert np.array_equal(a[0], b[0]), f"row 0 differs between launch_mm M=1 and path {path} M={M}"
        if path == 2:
            for a, b in zip(full, got):
                assert np.array_equal(a[:16], b[:16]), f"rows 0..15 differ between launch_mm M=16 and path 2 M={M}"


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(mx):
    """Every argument the probes must refuse gives MX_ERR_ARG before anything is launched: the output buffer
    passed in comes back untouched."""
    wb, xb = case(64, 128)[:2]
    w192 = case(192, 128)[0]
    sentinel = np.full(4200 * 256, 0x5A5A5A5A, dtype=np.uint32)
    res = np.zeros((64, 64), dtype=np.float32)
    xf, nw = np.ones((4, 128), dtype=np.float32), np.ones(128, dtype=np.float32)
    xf512, nw512 = np.ones((5, 512), dtype=np.float32), np.ones(512, dtype=np.float32)
    w512 = case(48, 512)[0]
    qa = lambda M, **over: {**qkv_args(M, (1, 1, 64), "id"), **over}

    def refused(*a, **kw):
        out = sentinel.copy()
        with pytest.raises(mx.MxError) as ei:
            mx.matmul_probe(*a, out=out, **kw)
        assert ei.value.code == mx.MX_ERR_ARG, (a, ei.value)
        assert np.array_equal(out, sentinel), "a refused call wrote its output"
        return str(ei.value)

    refused(5, F32, wb, xb[:4])                                  # path
    refused(-1, F32, wb, xb[:4])
    refused(0, 4, wb, xb[:4])                                    # epilogue
    refused(0, F32, wb[:24], xb[:4])                             # N % 16
    refused(0, F32, wb[:, :48], xb[:4, :48])                     # K % 32
    refused(0, F32, wb, xb[:0])                                  # M = 0
    refused(0, F32, wb, np.zeros((65, 128), np.uint16))          # M > 64
    refused(1, RESID, wb, xb[:17], resid=res[:17])               # path 1: M > 16
    refused(2, F32, wb, np.zeros((65, 128), np.uint16))
    refused(4, F32, wb, xb[:64], target=0)                       # path 4: M <= 64 is not the GEMM's
    refused(4, F32, np.zeros((256, 64), np.uint16), np.zeros((4097, 64), np.uint16))
    refused(4, RESID, np.zeros((256, 64), np.uint16), np.zeros((65, 64), np.uint16), resid=np.zeros((65, 256), np.float32),
            target=257, slab_floats=1 << 20)                     # target
    refused(0, RESID, wb, xb[:4])                                # RESID without resid
    refused(0, QKV, w192, xb[:4])                                # QKV without its operands
    refused(0, QKV, w192, xb[:4], qkv=qa(4, rope_cs=None))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, kcache=None))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, pos=None))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, n_head=2))           # geometry does not give N
    refused(0, QKV, wb, xb[:4], qkv={**qkv_args(4, (2, 1, 16), "id")})  # head_dim
    refused(0, QKV, w192, xb[:4], qkv=qa(4, pos=np.array([0, 1, N_CTX + 1, 2])))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, pos=np.array([0, -1, 1, 2])))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, slot=np.array([0, 1, 3, 2])))
    refused(0, QKV, w192, xb[:4], qkv=qa(4, slot=np.array([0, -1, 1, 2])))
    refused(0, F32, wb, xf=np.ones((5, 128), np.float32), norm_w=nw)      # norm on load: M > 4
    refused(0, F32, wb, xf=xf, norm_w=nw)                        # K 128 has no norm-on-load form
    refused(0, F32, w512, xf=xf512[:4], norm_w=None)             # norm_w missing
    refused(2, F32, w512, xf=xf512[:4], norm_w=nw512)            # only paths 0 and 1
    refused(0, RESID, w512, xf=xf512[:4], norm_w=nw512, resid=np.zeros((4, 48), np.float32))
    refused(0, F32, wb, xb[:4], act_f32=True)                    # act_f32 is SWIGLU's
    refused(0, F32, wb, xb[:4], want_ssq=True)                   # want_ssq is RESID's ...
    refused(2, RESID, wb, xb[:33], resid=res[:33], want_ssq=True)  # ... on paths 0 and 1
    refused(2, RESID, case(96, 128)[0], xb[:33], resid=np.zeros((33, 96), np.float32))  # fold width N % 64
    refused(2, RESID, case(48, 128)[0], xb[:33], resid=np.zeros((33, 48), np.float32))  # an odd tile count
    refused(4, SWIGLU, np.zeros((256, 64), np.uint16), np.zeros((65, 64), np.uint16), act_f32=True, target=256,
            slab_floats=1 << 20)                                 # the split finish writes bf16 only
    # shapes the launchers themselves refuse: reported with the launcher's name, nothing launched
    assert "launch_mm_pers" in refused(1, RESID, wb, xb[:4], resid=res[:4])
    assert "launch_mm_wide" in refused(2, F32, case(64, 96)[0], case(64, 96)[1][:33])     # K % 128
    assert "launch_mm_wide" in refused(2, RESID, case(192, 96)[0], case(192, 96)[1][:33], resid=np.zeros((33, 192), np.float32))
    assert "launch_mm_wide" in refused(2, F32, case(48, 128)[0], xb[:33])                 # 3 tiles: no <2,1> grouping
    assert "launch_gemm_split" in refused(4, F32, wb, np.zeros((65, 128), np.uint16))     # N % 256

    def norm_refused(*a, **kw):
        with pytest.raises(mx.MxError) as ei:
            mx.norm_probe(*a, **kw)
        assert ei.value.code == mx.MX_ERR_ARG

    x = np.zeros((4, 128), dtype=np.float32)
    norm_refused(np.zeros((4, 96), np.float32), None, np.ones(96, np.float32))           # n % 64
    norm_refused(np.zeros((1, 16448), np.float32), None, np.ones(16448, np.float32))     # n > 16384
    norm_refused(x, np.zeros((17, 4, 128), np.float32), np.ones(128, np.float32))        # nslab > 16
    norm_refused(x, None, np.ones(128, np.float32), row_map=[0, 4])                      # row_map out of range
    norm_refused(x, None, np.ones(128, np.float32), row_map=[-1])
    norm_refused(x, np.zeros((1, 4, 128), np.float32), np.ones(128, np.float32), row_map=[0])  # row_map with slabs
    norm_refused(x, None, None, row_map=[0])                                             # row_map without w


def test_packer_matches_layout(mx):
    """launch_pack's tiles (PACK_ROWS, PACK_GATE / PACK_UP) against the numpy restatement of the layout."""
    N, K = 96, 160
    wb = np.random.default_rng(3).integers(0, 0x7F00, size=(N, K)).astype(np.uint16)
    xb = case(N, K)[1][:4]
    r = mx.matmul_probe(0, F32, wb, xb, want_packed=True)
    assert np.array_equal(r.packed, L.pack_tiles(wb))
    r = mx.matmul_probe(0, SWIGLU, wb, xb, want_packed=True)
    assert np.array_equal(r.packed, L.pack_swiglu(wb))
