"""The IQ4_XS (ggml type 23) instances of the K-quant kernels alone, through mx_kq_matmul_probe / mx_kq_side_probe, against
exact integers -- the scheme of tests/test_kq_kernel_gpu.py, whose operand checks, epilogue checks and q|k|v geometry
are imported: d = 2^j and activations that are small integers x 2^-e with one +-127 per super-block, so (d d_x) S is
exact and every partial sum is a multiple of one unit below 2^24 units (asserted on the actual operands): f32 gives the
float64 product in any summation order and the comparison is by value.  Scales ls - 32 are drawn from [-8, 8) with one
sub-block per row at 0, 31, 32 or 63 to keep that bound; the extremes case covers the full range and says what it
assumes instead.  The reference is tests/iq4_ref.py (pinned to the format by tests/test_iq4_xs_host.py)."""
import functools
import types

import numpy as np
import pytest

import iq4_ref as Q
import kq_ref as R
import mm_layout as L
import test_kq_kernel_gpu as T
from test_kq_kernel_gpu import F32, QKV, RESID, SWIGLU, all_ones, mx, plan_is  # noqa: F401 (mx: the module's fixture)

pytestmark = pytest.mark.gpu
IQ = 23


@functools.lru_cache(maxsize=4)
def wcase(N, K, seed=0):
    rng = np.random.default_rng(4000 + N + K + seed)
    SB = K // 256
    ls = rng.integers(24, 40, size=(N, SB, 8))
    n_i, s_i = np.indices((N, SB))
    ls[n_i, s_i, n_i % 8] = np.array([0, 31, 32, 63])[(n_i // 8 + s_i) % 4]
    b = Q.blocks(R.f16_bits(2.0 ** rng.integers(-8, -6, size=(N, SB))), ls, rng.integers(0, 16, size=(N, K), dtype=np.uint8))
    return b, Q.fields(b)


@functools.lru_cache(maxsize=4)
def case(segs, K, rows, swiglu=False):
    """(blocks flat, xf, xi, e, s float64 [rows][N], unit) over row segments of type 23 / 13 / 14 (T.case's contract)."""
    t0, parts, cols, jmin = 0, [], [], 0
    xi, er = T.xcase(K, rows, 14)  # the narrowest activation range
    for i, (t, te) in enumerate(segs):
        n = 16 * (te - t0)
        if t == IQ:
            b, f = wcase(n, K, i)
            s, mag = Q.product(f, xi, 2.0 ** -er.astype(np.float64))
            d = [f["d"]]
        else:
            b, f = T.wcase(n, K, t, seed=i)
            s, mag = R.product(t, f, xi, 2.0 ** -er.astype(np.float64))
            d = [f["d"]] + ([] if t == 14 else [f["dmin"]])
        jmin = min([jmin] + [int(np.log2(R.f16_f32(x).min())) for x in d])
        parts.append(b.reshape(-1)), cols.append((s, mag))
        t0 = te
    unit = 2.0 ** (jmin - int(er.max()))
    assert max(m.max() for _, m in cols) / unit < 2 ** 24, "partial sums could leave f32's exact range"
    s_rel = np.concatenate([s for s, _ in cols], axis=1)
    peak = np.abs(s_rel[:, :s_rel.shape[1] // 2] if swiglu else s_rel).max()
    e0 = max(0, int(np.ceil(np.log2(max(peak, 1) / 64))))
    e = er + e0
    xf = (xi * np.repeat(2.0 ** -e, 256, axis=1)).astype(np.float32)
    return np.concatenate(parts), xf, xi, e, s_rel * 2.0 ** -e0, unit * 2.0 ** -e0


def run(mx, path, epi, segs, K, M, act=0, norm=False, rope="mixed", rows=32):
    N = 16 * segs[-1][1]
    blocks, xf, xi, e, s, unit = case(tuple(segs), K, rows, epi == SWIGLU)
    what = f"path {path} {segs} {T.EPI_NAME[epi]} M={M} K={K} act {act} norm {norm}"
    kw, qa, ri, x = dict(want_slabs=path >= 1), None, None, xf[:M]
    if epi == RESID:
        ri = T.resid_ints(M, N)
        kw["resid"] = (ri * unit).astype(np.float32)
        if path == 1:
            kw["fold_w"] = np.ones(N, np.float32)
    if epi == QKV:
        qa = kw["qkv"] = T.qkv_args(M, T.GEOM[N], rope)
    if norm:
        x1, w = T.normed(xi[0], e[0])
        x, kw["norm_w"] = x1[None], w
    r = mx.kq_matmul_probe(path, epi, blocks, x, list(segs), N=N, K=K, act=act, **kw)
    if act != 2:
        T.check_operand(r, xi, e, M, what)
    T.check_out(r, epi, s[:M], M, N, what, qa, ri, unit)
    if path >= 1:
        assert r.split >= 1 and np.array_equal(r.slabs.astype(np.float64).sum(axis=0), s[:M]), f"{what}: slabs"


# (plan kind, epilogue, N, K, row counts, on load, further plan fields).  K: bd_tile and qkv_pers have fixed K (2048 /
# 4096); pers at 8 super-blocks gives each of its 8 waves one; mkq_kernel's 8 waves split 9 super-blocks 1|1|..|2 at
# K 2304 and leave 7 waves empty at K 256; the wide form's one wave per tile walks the whole K and needs SB % 4 == 0:
# K 1024 and 2048 (one and two turns of its 4-deep ring).
FORMS = [("bd_tile", F32, 16, 2048, (1,), True, dict(w=8)), ("bd_tile", F32, 144, 2048, (1,), True, dict(w=8)),
         ("bd_tile", SWIGLU, 160, 2048, (1,), True, dict(w=3)), ("bd_tile", F32, 80, 4096, (1,), True, dict(w=8, tpw=4)),
         ("pers", F32, 16 * 1025, 2048, (1, 2, 16), False, dict(nkw=1, tpw=8)),
         ("pers", SWIGLU, 16 * 704, 2048, (1, 16), False, dict(nkw=1, tpw=3)),
         ("wide", F32, 64, 1024, (17, 32), False, dict(w=4)), ("wide", SWIGLU, 192, 2048, (17, 32), False, dict(w=4)),
         ("mkq", F32, 16, 256, (1, 2, 16, 17, 32, 64), False, {}), ("mkq", F32, 48, 2304, (1, 2, 16, 17, 32, 64), False, {}),
         ("mkq", RESID, 48, 2304, (1, 2, 16, 17, 32, 64), False, {}), ("mkq", RESID, 48, 2304, (1,), True, dict(ql=1)),
         ("mkq", SWIGLU, 96, 4352, (1, 16), False, {})]


@pytest.mark.parametrize("kind,epi,N,K,Ms,on_load,want", FORMS,
                         ids=[f"{k}-{T.EPI_NAME[e]}-{n}x{kk}{'-ql' if o else ''}" for k, e, n, kk, _, o, _ in FORMS])
def test_every_form(mx, kind, epi, N, K, Ms, on_load, want):
    segs = ((IQ, N // 16),)
    for M in Ms:
        for norm in ((False, True) if on_load else (False,)):
            plan_is(mx, epi, M, N, K, segs, on_load=on_load, norm=norm, kind=kind, **want)
            run(mx, 0, epi, segs, K, M, act=2 if on_load else 0, norm=norm, rows=max(Ms) if max(Ms) > 32 else 32)


MIXED = [((IQ, 12), (13, 16)), ((IQ, 8), (IQ, 12), (14, 16)), ((IQ, 8), (13, 12), (14, 16))]


@pytest.mark.parametrize("segs", MIXED, ids=["iq4|q5k", "iq4|iq4|q6k", "iq4|q5k|q6k"])
def test_mixed_segments(mx, segs):
    """q|k|v with IQ4_XS segments (one, or two adjacent ones each with its own base and tile end) beside Q5_K / Q6_K, N
    256: mkq_pers_seg_kernel (one normed token, K 4096), mkq_kernel (2 rows) and launch_mkq_qkv_slab's
    mkq_wide_seg_kernel (17 and 32 rows, K 4096 split 4 ways and K 1024 unsplit)."""
    plan_is(mx, QKV, 1, 256, 4096, segs, on_load=True, norm=True, kind="qkv_pers", grid_x=8)
    run(mx, 0, QKV, segs, 4096, 1, act=2, norm=True)
    plan_is(mx, QKV, 2, 256, 4096, segs, kind="mkq")
    run(mx, 0, QKV, segs, 4096, 2)
    for K, ks in ((4096, 4), (1024, 1)):
        for M in (17, 32):
            assert plan_is(mx, QKV, M, 256, K, segs)["qkv_slab_ks"] == ks
            run(mx, 2, QKV, segs, K, M)


def test_slab_resid(mx):
    """launch_mkq_slab (mkq_wide_kernel<23, 4, EPI_SLAB>): N 64, K 2304 split 4 + 5, folded by the norm that follows."""
    assert plan_is(mx, RESID, 31, 64, 2304, ((IQ, 4),))["slab_ks"] == 2
    run(mx, 1, RESID, ((IQ, 4),), 2304, 31)


def one_sb(mx, b, x, N, M, act=0, kind="mkq", s0=0):
    """T.run_one_sb for type 23: activations zero outside super-block s0, the result fl(fl(S) (d d_x)) -- S is rounded to
    f32 as the kernel's (float)S does, d d_x is a power of two: exactness of S itself is NOT assumed."""
    K = x.shape[1]
    f = Q.fields(b)
    q, d, bs = R.quantize_q8k(x[:M])
    S = Q.superblock_ints(f, q)[..., s0]
    ref = (S.astype(np.float32).astype(np.float64) * (R.f16_f32(f["d"][:, s0]).astype(np.float64)[None] * d[:, s0, None])).astype(np.float32)
    plan_is(mx, F32, M, N, K, ((IQ, N // 16),), on_load=act == 2, kind=kind)
    r = mx.kq_matmul_probe(0, F32, b, x[:M], IQ, N=N, K=K, act=act)
    assert np.array_equal(r.out, ref) and all_ones(r.guard), f"N={N} K={K} M={M} act {act}"
    return np.abs(S).max()


def test_extremes(mx):
    """Every index 0 (-127) or 15 (113), every ls 0 (-32) or 63 (+31), every q_x +-127: |S| reaches 8 x 32 x 32 x 127 x
    127 = 1.3e8 > 2^24 and each sub-block product 32 x 127 x 127 < 2^19 stays inside __mul24."""
    top = 0
    for idx, ls in ((0, 0), (0, 63), (15, 0), (15, 63)):
        b1 = Q.blocks(R.f16_bits(np.full((64, 1), 2.0 ** -8)), np.full((64, 1, 8), ls), np.full((64, 256), idx))
        for sign in (1.0, -1.0):
            x = np.full((33, 256), sign * 127.0 * 2.0 ** -6, np.float32)
            for M, act in ((1, 0), (1, 2), (2, 0), (17, 0), (33, 0)):
                top = max(top, one_sb(mx, b1, x, 64, M, act))
            for K, M, act, kind in ((2048, 1, 2, "bd_tile"), (1024, 17, 0, "wide")):
                xx = np.zeros((33, K), np.float32)
                xx[:, K - 256:] = x
                one_sb(mx, np.tile(b1, (1, K // 256)), xx, 64, M, act, kind, s0=K // 256 - 1)
    assert top == 8 * 32 * 32 * 127 * 127 > 2 ** 24


def test_onehot(mx):
    """One non-zero activation at each k of a super-block against weights whose index at k is k mod 16 (row n: (k + n)
    mod 16) and whose scale differs per sub-block: a nibble-order, codebook-order or scale-column mistake shows."""
    N, K = 16, 256
    idx = (np.arange(K)[None] + np.arange(N)[:, None]) % 16
    ls = 33 + (np.arange(8)[None] * 3 + np.arange(N)[:, None]) % 30
    b = Q.blocks(R.f16_bits(np.full((N, 1), 2.0 ** -8)), ls[:, None, :], idx)
    for k in range(K):
        x = np.zeros((17, K), np.float32)
        x[:, k] = 127 * 2.0 ** -6
        for M, act in ((1, 0), (1, 2), (2, 0), (17, 0)):
            if (M, act) == (1, 0) or k % 4 == 0:
                one_sb(mx, b, x, N, M, act)


def edge_blocks(N, SB, seed):
    """Random blocks with finite d, among them a subnormal, a zero and a negative one."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(N, SB, 136), dtype=np.uint8)
    v = rng.uniform(-2, 2, size=(N, SB)).astype(np.float16)
    v[0, 0], v[1, 0], v[2, 0] = np.float16(3e-7), np.float16(0.0), np.float16(-1.25)
    b[..., 0], b[..., 1] = v.view(np.uint16) & 0xFF, v.view(np.uint16) >> 8
    return b.reshape(N, -1)


@pytest.mark.parametrize("N,K", [(16, 256), (48, 768)])
def test_packer_dequant_embed(mx, N, K):
    """pack_kq_kernel<23>, dequant_kq_kernel<23> (alone and between a Q5_K and a Q6_K segment), embed_kq_kernel and
    dequant_bf16_kernel on type 23, each bitwise against tests/iq4_ref.py, guards untouched."""
    b = edge_blocks(N, K // 256, N + K)
    f = Q.fields(b)
    for mode, off in ((0, 0), (0, 16), (1, 0), (2, 0)):
        got, guard = mx.kq_pack_probe(b, IQ, N, K, pack=mode, offset=off)
        assert np.array_equal(got, Q.pack_tiles(b, mode, off)) and all_ones(guard), f"pack mode {mode} offset {off}"
    want = Q.dequant_f32(f)
    got, guard = mx.kq_dequant_probe(b, [(IQ, N // 16)], N, K)
    assert np.array_equal(got, L.pack_tiles(L.bf16_bits(want))) and all_ones(guard)
    b5, b6 = T.edge_blocks(13, 16, K // 256, 1), T.edge_blocks(14, 16, K // 256, 2)
    segs = [(13, 1), (IQ, 1 + N // 16), (14, 2 + N // 16)]
    got, guard = mx.kq_dequant_probe(np.concatenate([b5.reshape(-1), b.reshape(-1), b6.reshape(-1)]), segs, N + 32, K)
    ref = np.concatenate([R.dequant_f32(13, R.kq_fields(13, b5)), want, R.dequant_f32(14, R.kq_fields(14, b6))])
    assert np.array_equal(got, L.pack_tiles(L.bf16_bits(ref))) and all_ones(guard)
    ids = [N - 1, 0, 2, 1, 7, N - 1]
    x, xg, ssq, sg = mx.kq_embed_probe(b, IQ, N, K, ids)
    assert np.array_equal(x.view(np.uint32), want[ids].view(np.uint32)) and all_ones(xg) and all_ones(sg)
    T.check_ssq(types.SimpleNamespace(final=want[ids].astype(np.float64), ssq=ssq), "embed iq4_xs")
    out, guard = mx.glue_flat_probe(0, b, N * K, type=IQ)
    assert np.array_equal(out, L.bf16_bits(want).reshape(-1)) and all_ones(guard)


REAL = [(F32, 48, 2304, 1, False, dict(kind="mkq", bd=1)), (F32, 48, 2304, 16, False, dict(kind="mkq", u=2)),
        (F32, 48, 4096, 33, False, dict(kind="mkq", nb=2, grid_y=2)), (F32, 64, 2048, 32, False, dict(kind="wide", w=4)),
        (RESID, 64, 4352, 31, False, dict(slab_ks=4)), (F32, 144, 2048, 1, True, dict(kind="bd_tile", w=8)),
        (F32, 16 * 1025, 2048, 2, False, dict(kind="pers")), (QKV, 256, 4096, 1, True, dict(kind="qkv_pers"))]


@pytest.mark.parametrize("epi,N,K,M,on_load,want", REAL, ids=[f"{T.EPI_NAME[e]}-{n}x{k}-M{m}" for e, n, k, m, *_ in REAL])
def test_real_scales(mx, epi, N, K, M, on_load, want):
    """synth.kq_blocks (random f16 d, every scale and index) and Gaussian rows against float64 on the device's own xq /
    xd.  tests/test_kq_kernel_gpu.py::test_real_scales derives (3 + 2 SB + 8) 2^-24 sum |terms| for the two terms per
    super-block of Q4_K; with no mins term there is one term and one addition per super-block, so the same count of
    roundings gives (3 + SB + 8) 2^-24 sum_s |d d_x S|, which is what is asserted here.  The QKV case (mkq_pers_seg_kernel,
    q|k IQ4_XS + v Q5_K, identity RoPE) compares the q rows the launch returns: 8 of the 12 IQ4_XS tiles."""
    from llama_p2p_amd import synth

    segs = ((IQ, 12), (13, 16)) if epi == QKV else ((IQ, N // 16),)
    nq = 16 * segs[0][1]
    blocks = synth.kq_blocks(IQ, nq * K // 256, seed=11, tid=923).reshape(nq, -1)
    w = np.concatenate([blocks.reshape(-1), synth.kq_blocks(13, (N - nq) * K // 256, seed=11, tid=924).reshape(-1)])
    x = (np.random.default_rng(K + M).standard_normal((M, K)) * 1.5).astype(np.float32)
    plan_is(mx, epi, M, N, K, segs, on_load=on_load, **want)
    kw = dict(resid=np.zeros((M, N), np.float32), fold_w=np.ones(N, np.float32)) if epi == RESID else {}
    if epi == QKV:
        kw["qkv"] = T.qkv_args(M, T.GEOM[N], "id")
    r = mx.kq_matmul_probe(1 if epi == RESID else 0, epi, w, x, list(segs), N=N, K=K, act=2 if on_load else 0, **kw)
    q, d, _ = R.quantize_q8k(x)
    if not on_load:
        assert np.array_equal(R.unperm_rows(r.xq), q) and np.array_equal(r.xd, d)
    ref, mag = (a[:, :r.out.shape[1]] for a in Q.product(Q.fields(blocks), q, d))
    assert r.out.shape[1] == (128 if epi == QKV else N)
    frac = float((np.abs(r.out.astype(np.float64) - ref) / ((3 + K // 256 + 8) * 2.0 ** -24 * mag)).max())
    print(f"iq4_xs real scales worst |err| / bound: {T.EPI_NAME[epi]} N={N} K={K} M={M} {frac:.3f}")
    assert frac <= 1.0 and all_ones(r.guard)
