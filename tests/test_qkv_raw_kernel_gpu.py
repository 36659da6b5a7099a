"""launch_mm's raw q|k|v epilogue (EPI_QKV_RAW) alone, through mx_matmul_probe's epi 6 -- no model.

A layer with Qwen3's q/k norm weights takes its q|k|v sums raw (one f32 slab [M][N]) from launch_mm and finishes them
in the attention's FIN path or in qkn_finish_kernel.  It arrived with five geometries:

    nb = 1 (M <= 16, or RMS_NORM on load)   <16,1,RAW,4>
    nb = 2 (M 17..32)   tiles even <8,2,RAW,8>   odd <8,1,RAW,8>
    nb = 3, 4 (M 33..64) tiles even <4,2,RAW,4>  odd <4,1,RAW,4>

of which the last four ran in a model only at 17..64 rows of a bf16 Qwen3 model whose width is no multiple of 128 (every
other shape takes launch_mm_wide there) -- and test_canonical_grouping[448] failed on them when it was written: row 0
alone != row 0 of the 17-row launch (8 and 4 waves chain two and four canonical K slices in one MFMA accumulator; the
16-wave form adds them after).  EPI_QKV's 17..64-row geometries had the same fault.  Both now take <16,1,.,4> at every
row count (NB 1, 2, 4).  N = 576 (36 tiles, Qwen2's qwen-g7 q|k|v) and N = 560 (35 tiles; the raw epilogue needs no head
geometry) x M on both sides of 16, 32 and 48 reach every form; test_every_geometry_is_reached asserts that from the row
counts.

exact: the integer operands of tests/test_matmul_kernel_gpu.py (every product and partial sum exact in f32 in any
  order): out == the integer product, bitwise; the probe's 64 guard rows past row M still 0xFF.  An off-by-one tile,
  a wrong ldo or a wrong K range changes an integer sum.
norm on load: x == nullptr, M 1 and 4, K 1024 -- that file's exact operands (xf = +-1, norm_w powers of two).
grouping: random bf16 operands, where the K grouping decides the rounding.  A row launched alone equals the same row
  of the 16-, 17-, 33- and 64-row launches, bitwise (batch invariance); and an EPI_QKV launch of the same operands
  (identity RoPE table, no bias) gives the raw output's q columns bitwise and f16 of its k / v columns in the caches:
  "EPI_QKV's canonical K grouping" read off the code, not off a comment.
refusals: epi 6 on every path but 0, and epi 4 / 5 / 7 anywhere, give MX_ERR_ARG and launch nothing.
Nothing is left out: the probe refuses no geometry of launch_mm's raw epilogue."""
import numpy as np
import pytest

import mm_layout as L
from test_matmul_kernel_gpu import (F32, QKV, N_CTX, all_ones, case, mx, nol_operands, qkv_args,  # noqa: F401
                                    rand_bf16)

pytestmark = pytest.mark.gpu

RAW = 6
RAW_M = [1, 4, 5, 16, 17, 32, 33, 64]
RAW_N = [576, 560]  # 36 tiles (even), 35 tiles (odd)
K_EXACT = 448       # 14 K tiles: uneven over 16, 8 and 4 waves


def test_every_geometry_is_reached():
    """launch_mm's dispatch restated: column tiles nb = ceil(M / 16) in {1, 2, 3..4} x the parity of N / 16 (nb = 1
    has one geometry for both).  No GPU."""
    reached = {(min((M + 15) // 16, 3), (N // 16) % 2) for M in RAW_M for N in RAW_N}
    assert reached == {(nb, par) for nb in (1, 2, 3) for par in (0, 1)}
    assert {(M + 15) // 16 for M in RAW_M} == {1, 2, 3, 4}
    assert [N // 16 for N in RAW_N] == [36, 35]


@pytest.mark.parametrize("N", RAW_N)
def test_exact(mx, N):
    wb, xb, ref, e, _ = case(N, K_EXACT)
    for M in RAW_M:
        r = mx.matmul_probe(0, RAW, wb, xb[:M])
        assert r.out.shape == (M, N)
        assert np.array_equal(r.out, (ref[:M] * 2.0 ** -e).astype(np.float32)), f"raw M={M} N={N}"
        assert all_ones(r.guard), f"raw M={M} N={N}: rows past M written"


@pytest.mark.parametrize("N", RAW_N)
def test_norm_on_load_exact(mx, N):
    K = 1024
    wb, wi = case(N, K)[0], case(N, K)[4]
    for M in (1, 4):
        assert mx.matmul_plan(QKV, M, N, K)["norm_on_load_ok"]
        xf, nw, eps, bi, unit = nol_operands(M, K, True)
        r = mx.matmul_probe(0, RAW, wb, xf=xf, norm_w=nw, eps=eps)
        assert np.array_equal(r.out, (L.int_matmul(wi, bi) * unit).astype(np.float32)), f"raw norm on load M={M} N={N}"
        assert all_ones(r.guard)


@pytest.mark.parametrize("K", [448, 2048])
def test_canonical_grouping(mx, K):
    N, geom = 576, (7, 1, 64)
    nq = geom[0] * geom[2]
    kg = mx.matmul_plan(QKV, 1, N, K)["kgroups"]
    assert all(mx.matmul_plan(QKV, M, N, K)["kgroups"] == kg for M in (16, 17, 33, 64)), "canon_kgroups reads the row count"
    wb, xb = rand_bf16((N, K), 21 + K), rand_bf16((64, K), 22 + K)
    alone = {i: mx.matmul_probe(0, RAW, wb, xb[i:i + 1]).out.view(np.uint32)[0] for i in (0, 5, 15)}
    assert len({a.tobytes() for a in alone.values()}) == 3
    for M in (1, 16, 17, 33, 64):
        raw = mx.matmul_probe(0, RAW, wb, xb[:M])
        bits = raw.out.view(np.uint32)
        assert not (bits == 0xFFFFFFFF).any() and all_ones(raw.guard)
        for i, a in alone.items():
            if i < M:
                assert np.array_equal(a, bits[i]), f"K={K}: row {i} alone != row {i} of the {M}-row launch"
        qa = qkv_args(M, geom, "id")
        r = mx.matmul_probe(0, QKV, wb, xb[:M], qkv=qa)
        st = qa["pos"] < N_CTX
        assert np.array_equal(r.out.view(np.uint32)[st], bits[st, :nq]), f"K={K} M={M}: EPI_QKV's q != the raw q columns"
        K1, V1 = L.untile_caches(r.kcache, r.vcache, qa["n_slots"], 1, L.kv_layout.ctx_stride(N_CTX), 64)
        kv16 = raw.out[:, nq:].astype(np.float16).view(np.uint16)
        for i in np.flatnonzero(st):
            assert np.array_equal(K1[qa["slot"][i], 0, qa["pos"][i]], kv16[i, :64]), f"K={K} M={M} row {i}: K"
            assert np.array_equal(V1[qa["slot"][i], 0, qa["pos"][i]], kv16[i, 64:]), f"K={K} M={M} row {i}: V"


def test_refusals(mx):
    wb, xb = case(576, K_EXACT)[:2]
    sentinel = np.full(200 * 576, 0x5A5A5A5A, dtype=np.uint32)
    for path, epi, M in [(1, RAW, 4), (2, RAW, 33), (3, RAW, 33), (0, 4, 4), (0, 5, 4), (0, 7, 4), (0, RAW, 65)]:
        out = sentinel.copy()
        with pytest.raises(mx.MxError) as ei:
            mx.matmul_probe(path, epi, wb, np.zeros((M, K_EXACT), np.uint16), out=out)
        assert ei.value.code == mx.MX_ERR_ARG, (path, epi, ei.value)
        assert np.array_equal(out, sentinel), "a refused call wrote its output"
    out = np.full(400 * 576, 0x5A5A5A5A, dtype=np.uint32)
    with pytest.raises(mx.MxError) as ei:  # path 4 (the GEMM) has no raw epilogue either
        mx.matmul_probe(4, RAW, case(768, 64)[0], np.zeros((65, 64), np.uint16), out=out)
    assert ei.value.code == mx.MX_ERR_ARG and (out == 0x5A5A5A5A).all()
    xf, nw = np.ones((5, 1024), np.float32), np.ones(1024, np.float32)
    with pytest.raises(mx.MxError) as ei:  # norm on load keeps its conditions: M <= 4
        mx.matmul_probe(0, RAW, case(576, 1024)[0], xf=xf, norm_w=nw)
    assert ei.value.code == mx.MX_ERR_ARG
