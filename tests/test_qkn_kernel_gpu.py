"""Qwen3's per-head q/k norm kernels alone, through mx_qkn_probe -- no model: qkn_finish_kernel
against float64, and the decode attention's FIN path with the norm weights bitwise against qkn_finish_kernel followed
by the plain attention.

Slabs are small integers and the norm weights powers of two, so the slab sum and the MUL are exact in f32 and the rms
scale (and RoPE's roundings) are the only inexact steps.  The bound on q / K is measured, not chosen: the worst error
of the same formula evaluated in plain float32 NumPy against float64 on these inputs; the kernel, whose sums are double,
is allowed twice that (both figures: profiles/qwen3.txt)."""
import functools

import numpy as np
import pytest

import kv_layout

pytestmark = pytest.mark.gpu

N_CTX, NKV, EPS = 64, 2, 1e-6
POS = np.array([0, 15, 16, 31, 32, N_CTX - 1, N_CTX], np.int32)  # the last row stores nothing
SLOT = np.arange(len(POS), dtype=np.int32)
CASES = [(D, G, ns) for D in (64, 128) for G in (1, 2, 5, 8) for ns in (1, 3, 8)]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def formula(s, wq, wk, cs, D, G, dt):
    """RMS_NORM, MUL, adjacent-pair RoPE of the q and k heads of s [M][N] in dtype dt -> (q [M][G NKV D], k [M][NKV D])."""
    M, nq = s.shape[0], G * NKV * D
    out = []
    for x, w in ((s[:, :nq].reshape(M, -1, D), wq), (s[:, nq:nq + NKV * D].reshape(M, -1, D), wk)):
        x, w = x.astype(dt), w.astype(dt)
        n = x / np.sqrt((x * x).mean(-1, keepdims=True, dtype=dt) + dt(EPS)) * w
        c, sn = cs[:, None, :, 0].astype(dt), cs[:, None, :, 1].astype(dt)
        o = np.empty_like(n)
        o[..., 0::2] = n[..., 0::2] * c - n[..., 1::2] * sn
        o[..., 1::2] = n[..., 0::2] * sn + n[..., 1::2] * c
        out.append(o.reshape(M, -1))
    return out


@functools.lru_cache(maxsize=None)
def case(D, G, ns):
    rng = np.random.default_rng(1000 * D + 10 * G + ns)
    M, N = len(POS), (G + 2) * NKV * D
    slabs = rng.integers(-8, 9, (ns, M, N)).astype(np.float32)
    wq, wk = (2.0 ** rng.integers(-2, 3, D) for _ in range(2))
    th = np.arange(N_CTX, dtype=np.float64)[:, None] * 1e6 ** (-2.0 * np.arange(D // 2) / D)[None, :]
    cs = np.stack([np.cos(th), np.sin(th)], -1).astype(np.float32)
    elems = len(POS) * NKV * kv_layout.ctx_stride(N_CTX) * D
    init = (((np.arange(elems, dtype=np.int64) * 37) % 201 - 100) / 64.0).astype(np.float16).view(np.uint16)
    return slabs, wq.astype(np.float32), wk.astype(np.float32), cs, init, init[::-1].copy()


def probe(mx, mode, D, G, ns):
    slabs, wq, wk, cs, k0, v0 = case(D, G, ns)
    try:
        return mx.qkn_probe(mode, G * NKV, NKV, D, N_CTX, len(POS), POS, SLOT, k0, v0, slabs, cs, wq, wk, EPS)
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:
            pytest.exit(f"HIP error, nothing more is launched: {e}", returncode=3)
        raise


def untiled(kc, vc, D):
    S = kv_layout.ctx_stride(N_CTX)
    return (kv_layout.untile_k(kc.reshape(len(POS), NKV, S * D), D), kv_layout.untile_v(vc.reshape(len(POS), NKV, S * D), D))


@pytest.mark.parametrize("D,G,ns", CASES, ids=[f"D{D}-G{G}-s{ns}" for D, G, ns in CASES])
def test_finish_kernel_against_float64(mx, D, G, ns):
    slabs, wq, wk, cs, k0, v0 = case(D, G, ns)
    s = slabs.astype(np.float64).sum(0)  # exact, and exact in f32
    st = POS < N_CTX
    csr = cs[np.minimum(POS, N_CTX - 1)]
    q64, k64 = formula(s, wq, wk, csr, D, G, np.float64)
    q32, k32 = formula(s, wq, wk, csr, D, G, np.float32)
    e32 = max(np.abs(q32 - q64)[st].max(), np.abs(k32 - k64)[st].max())
    q, _, kc, vc = probe(mx, 0, D, G, ns)
    K1, V1 = untiled(kc, vc, D)
    K0, V0 = (a.copy() for a in untiled(k0, v0, D))
    eq = np.abs(q[st] - q64[st]).max()
    kgot = K1[SLOT[st], :, POS[st], :].view(np.float16).astype(np.float64).reshape(st.sum(), -1)
    ek = (np.abs(kgot - k64[st]) - np.spacing(np.abs(k64[st]).astype(np.float16)).astype(np.float64) / 2).max()
    print(f"D={D} G={G} nslab={ns}: float32 NumPy vs float64 {e32:.3g}; kernel q {eq:.3g}, K beyond half an f16 ulp {ek:.3g}")
    assert e32 > 0
    assert eq <= 2 * e32, "q"
    assert ek <= 2 * e32, "K"
    assert (q[~st].view(np.uint8) == 0xFF).all(), "q of the row at n_ctx written"
    nq = G * NKV * D
    for i in np.flatnonzero(st):  # V: f16 of the exact sum; every other cache element as it was
        K0[SLOT[i], :, POS[i], :] = K1[SLOT[i], :, POS[i], :]
        V0[SLOT[i], :, POS[i], :] = s[i, nq + NKV * D:].reshape(NKV, D).astype(np.float16).view(np.uint16)
    assert np.array_equal(K1, K0), "K cache outside the rows' positions"
    assert np.array_equal(V1, V0), "V cache"


@pytest.mark.parametrize("D,G,ns", CASES, ids=[f"D{D}-G{G}-s{ns}" for D, G, ns in CASES])
def test_fin_path_is_bitwise_the_finish_kernel(mx, D, G, ns):
    _, o0, k0, v0 = probe(mx, 0, D, G, ns)
    _, o1, k1, v1 = probe(mx, 1, D, G, ns)
    st = POS < N_CTX
    assert not np.isnan(o1[st]).any()
    assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes(), "stored K / V"
    assert o0[st].tobytes() == o1[st].tobytes(), "attention output"
