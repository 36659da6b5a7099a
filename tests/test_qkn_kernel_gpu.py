"""Qwen3's per-head q/k norm kernels alone, through mx_qkn_probe -- no model: qkn_finish_kernel
against float64, and the decode attention's FIN path with the norm weights bitwise against qkn_finish_kernel followed
by the plain attention.

Slabs are small integers and the norm weights powers of two, so the slab sum and the MUL are exact in f32 and the rms
scale (and RoPE's roundings) are the only inexact steps.  The bound on q / K is measured, not chosen: the worst error
of the same formula evaluated in plain float32 NumPy against float64 on these inputs; the kernel, whose sums are double,
is allowed twice that (both figures: profiles/qwen3.txt).

Those two tests (M = 7, n_ctx 64, every row its own slot) stay as they were.  The rest of the file takes the kernels
to their edges, with the same two checks and the same measured bound, NKV = 2, D in {64, 128} x G in {1, 2, 4, 5, 6,
7, 8}:

 plans: tests/test_attention_kernel_gpu.py's mode 1 plans -- M in {17, 33, 64} x nslab in {1, 4, 5, 8} at n_ctx 512
   (positions walking EDGE: chunk seams, wave rounds, one row at pos == n_ctx; nslab 1 is the MS = 1 instance), n_ctx
   100 (ctx_stride 128, positions 99 and 100) and n_ctx 2048 (position 2047).  Every cache position from a slot's
   first new one on holds f16 NaN (0x7E00) before the launch: an over-read shows as NaN in the output.
 families: "int" -- integer slabs, power-of-two weights (sum and MUL exact); "real" -- N(0, 1) slabs summed in f32 in
   slab order (the reference takes that f32 sum: the one thing both kernels are specified to do), log-normal weights
   as tests/qwen3_ref.py's qk_norm (the MUL rounds too), caches 0.25 N(0, 1) / N(0, 1).  A normalised head has norm
   sqrt(D) |w|, so the k-norm weights are a quarter of the q-norm's and K a quarter of N(0, 1): the scores then stay
   within family (c)'s precondition (spread <= 9, asserted on the reference; checked on the CPU for every case).
 attention output (mode 0, "real"): against kv_layout.ref_attention on the q and the caches the probe returned, at
   family (c)'s bound 2^-10 A, unchanged.
 prompt chunks (mode 0, rows sharing a slot; CHUNK_PLANS): M in {8, 9, 16, 40, 64} as blocks of consecutive positions
   of 1 to 3 slots at n_ctx 100 -- a block from position 5, blocks across 31|32 and 63|64, a block ending at n_ctx - 1;
   blockIdx.y up to 7.  The probe admits no two storing rows on one (slot, position), so the block that ends at
   n_ctx - 1 carries no copies of its last row (the one geometry left out; test_bad_arguments pins the refusal).
 a zero head: all-zero slab sums in one q head and one K head of a row -> exactly 0, nothing NaN.
 batch invariance of FIN with the norm: rows at M = 17 == among 64; a row at M = 1 (nslab 1) == among 16, bitwise.

Found by test_fin_plans[D64-G1-real] (plan M=33 nslab=4 n_ctx=512): with the scale, x * scale and * w formed in f32 the
kernel's q was 1.79e-06 from float64 against a measured float32-NumPy error of 6.02e-07 (an element near 8.6, 1.9 f32
ulp off; a NumPy restatement of the device's f32 steps gives the same 1.79e-06).  qk_norm_rope_head now forms them in
double and rounds once, which leaves it fewer roundings than the float32 NumPy formula."""
import functools

import numpy as np
import pytest

import kv_layout
from test_attention_kernel_gpu import EDGE, NAN16, PLANS, Plan, bank, block, slab_sum

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


# ---- the kernels at their edges ---------------------------------------------------------------------------------------
GEOMS = [(D, G) for D in (64, 128) for G in (1, 2, 4, 5, 6, 7, 8)]
GEOM_IDS = [f"D{D}-G{G}" for D, G in GEOMS]
FIN_PLANS = [p for p in PLANS if p.mode == 1]
CHUNK_CTX = 100
CHUNK_PLANS = [  # mode 0 only: rows share slots (nslab cycles 1, 3, 4, 5, 8)
    Plan(0, block(0, 5, 8), n_ctx=CHUNK_CTX, nslab=1),
    Plan(0, block(0, 5, 9), n_ctx=CHUNK_CTX, nslab=3),
    Plan(0, block(1, 24, 16), n_ctx=CHUNK_CTX, nslab=4, n_slots=2),
    Plan(0, block(0, 5, 8) + block(1, 26, 16) + block(2, 56, 16), n_ctx=CHUNK_CTX, nslab=5),
    Plan(0, block(0, 20, 50) + block(1, CHUNK_CTX - 14, 14), n_ctx=CHUNK_CTX, nslab=8),
]
MEASURED = {}


def test_the_plans_are_the_ones_described():
    assert sorted({(len(p.rows), p.nslab) for p in FIN_PLANS if p.n_ctx == 512}) == \
        [(M, ns) for M in (17, 33, 64) for ns in (1, 4, 5, 8)]
    assert {p.n_ctx for p in FIN_PLANS} == {100, 512, 2048}
    assert any(pos == p.n_ctx for p in FIN_PLANS for _, pos in p.rows)
    assert all(len({s for s, _ in p.rows}) == len(p.rows) for p in FIN_PLANS), "FIN: every row its own slot"
    assert [len(p.rows) for p in CHUNK_PLANS] == [8, 9, 16, 40, 64]
    pos = [{(s, q) for s, q in p.rows} for p in CHUNK_PLANS]
    assert all(len(a) == len(p.rows) for a, p in zip(pos, CHUNK_PLANS)), "distinct (slot, position) pairs"
    assert (0, 5) in pos[0] and {(1, 31), (1, 32)} <= pos[2] and {(0, 31), (0, 32), (0, 63), (0, 64)} <= pos[4]
    assert max(q for s, q in CHUNK_PLANS[4].rows if s == 1) == CHUNK_CTX - 1


class Inputs:
    """One plan at one geometry: slabs, weights, RoPE table, the logical caches (uint16 bits, poisoned) and their tiled
    form, and the f32 slab-order sum the kernels are specified to form."""

    def __init__(self, plan, D, G, family, seed, zero=None):
        rng = np.random.default_rng([seed, D, G, family == "real"])
        self.plan, self.D, self.G, self.n_ctx, self.n_slots = plan, D, G, plan.n_ctx, plan.n_slots
        self.slot = np.array([s for s, _ in plan.rows], np.int32)
        self.pos = np.array([p for _, p in plan.rows], np.int32)
        M, N, S = len(plan.rows), (G + 2) * NKV * D, kv_layout.ctx_stride(plan.n_ctx)
        shape = (plan.n_slots, NKV, S, D)
        n = int(np.prod(shape))
        if family == "int":
            self.slabs = rng.integers(-8, 9, (plan.nslab, M, N)).astype(np.float32)
            self.wq, self.wk = ((2.0 ** rng.integers(-2, 3, D)).astype(np.float32) for _ in range(2))
            init = (((np.arange(n, dtype=np.int64) * 37) % 201 - 100) / 64.0).astype(np.float16)
            K, V = init.reshape(shape), init[::-1].reshape(shape)
        else:
            self.slabs = (rng.standard_normal((plan.nslab, M, N)) / np.sqrt(plan.nslab)).astype(np.float32)
            self.wq = np.exp(0.5 * rng.standard_normal(D)).astype(np.float32)
            self.wk = (0.25 * np.exp(0.5 * rng.standard_normal(D))).astype(np.float32)
            a, b = bank()
            K, V = (a[:n] * np.float32(0.25)).astype(np.float16).reshape(shape), b[:n].astype(np.float16).reshape(shape)
        if zero is not None:  # (row, q head, kv head): all-zero sums
            r, h, kvh = zero
            self.slabs[:, r, h * D:(h + 1) * D] = 0
            self.slabs[:, r, G * NKV * D + kvh * D:G * NKV * D + (kvh + 1) * D] = 0
        self.K, self.V = K.view(np.uint16).copy(), V.view(np.uint16).copy()
        for s in set(self.slot.tolist()):  # poison from the slot's first new position on
            first = min(int(self.pos[self.slot == s].min()), plan.n_ctx)
            self.K[s, :, first:] = NAN16
            self.V[s, :, first:] = NAN16
        th = np.arange(plan.n_ctx, dtype=np.float64)[:, None] * 1e6 ** (-2.0 * np.arange(D // 2) / D)[None, :]
        self.cs = np.stack([np.cos(th), np.sin(th)], -1).astype(np.float32)
        self.k0, self.v0 = kv_layout.tile_k(self.K).reshape(-1), kv_layout.tile_v(self.V).reshape(-1)
        self.sum = slab_sum(self.slabs)
        assert self.sum.dtype == np.float32

    def probe(self, mx, mode, idx=None):
        """-> q, attention out, K after, V after (logical uint16 [n_slots][NKV][S][D])."""
        idx = slice(None) if idx is None else idx
        try:
            q, o, kc, vc = mx.qkn_probe(mode, self.G * NKV, NKV, self.D, self.n_ctx, self.n_slots, self.pos[idx],
                                        self.slot[idx], self.k0, self.v0, self.slabs[:, idx], self.cs, self.wq, self.wk, EPS)
        except mx.MxError as e:
            if e.code == mx.MX_ERR_HIP:
                pytest.exit(f"{self.plan} D={self.D} G={self.G}: HIP error, nothing more is launched: {e}", returncode=3)
            raise
        return (q, o, kv_layout.untile_k(kc.reshape(self.n_slots, NKV, -1), self.D),
                kv_layout.untile_v(vc.reshape(self.n_slots, NKV, -1), self.D))


def check_finish(c, q, K1, V1, what):
    """test_finish_kernel_against_float64's checks on any plan.  -> (e32, q error, K error beyond half an f16 ulp)."""
    D, G, pos, slot = c.D, c.G, c.pos, c.slot
    s = c.sum.astype(np.float64)
    st = pos < c.n_ctx
    csr = c.cs[np.minimum(pos, c.n_ctx - 1)]
    q64, k64 = formula(s, c.wq, c.wk, csr, D, G, np.float64)
    q32, k32 = formula(s, c.wq, c.wk, csr, D, G, np.float32)
    e32 = max(np.abs(q32 - q64)[st].max(), np.abs(k32 - k64)[st].max())
    assert not np.isnan(q[st]).any(), f"{what}: q never written"
    eq = np.abs(q[st] - q64[st]).max()
    kgot = K1[slot[st], :, pos[st], :].view(np.float16).astype(np.float64).reshape(st.sum(), -1)
    ek = (np.abs(kgot - k64[st]) - np.spacing(np.abs(k64[st]).astype(np.float16)).astype(np.float64) / 2).max()
    assert e32 > 0
    assert eq <= 2 * e32, f"{what}: q {eq:.3g} > 2 x {e32:.3g}"
    assert ek <= 2 * e32, f"{what}: K {ek:.3g} > 2 x {e32:.3g}"
    assert (q[~st].view(np.uint8) == 0xFF).all(), f"{what}: q of a row at n_ctx written"
    K0, V0 = c.K.copy(), c.V.copy()
    nq = G * NKV * D
    for i in np.flatnonzero(st):  # V: f16 of the sum; every other cache element as it was
        K0[slot[i], :, pos[i], :] = K1[slot[i], :, pos[i], :]
        V0[slot[i], :, pos[i], :] = c.sum[i, nq + NKV * D:].reshape(NKV, D).astype(np.float16).view(np.uint16)
    assert np.array_equal(K1, K0), f"{what}: K cache outside the rows' positions"
    assert np.array_equal(V1, V0), f"{what}: V cache"
    return float(e32), float(eq), float(ek)


def check_attention(c, q, out, K1, V1, what):
    """The attention output against float64 on the q and the caches the probe returned: family (c) of
    tests/test_attention_kernel_gpu.py, its precondition and its bound.  -> worst |out - ref| / tolerance."""
    D, G, worst = c.D, c.G, 0.0
    Kf, Vf = K1.view(np.float16), V1.view(np.float16)
    for i in np.flatnonzero(c.pos < c.n_ctx):
        for kvh in range(NKV):
            hs = slice(kvh * G * D, (kvh + 1) * G * D)
            ref, A, spread = kv_layout.ref_attention(q[i, hs].reshape(G, D), Kf[c.slot[i], kvh], Vf[c.slot[i], kvh],
                                                     c.pos[i], 1.0 / np.sqrt(D), c.n_ctx)
            assert spread.max() <= 9.0, f"{what}: input condition: score spread {spread.max():.2f} > 9"
            ratio = float((np.abs(out[i, hs].reshape(G, D) - ref) / (2.0 ** -10 * A)).max())
            assert ratio <= 1.0, f"{what} row {i} (slot {c.slot[i]}, pos {c.pos[i]}) kv head {kvh}: {ratio:.3g} x tolerance"
            worst = max(worst, ratio)
    return worst


def run_plans(mx, plans, D, G, family, seed, fin):
    worst = [0.0, 0.0, 0.0, 0.0]  # e32, q, K, attention ratio
    for pi, plan in enumerate(plans):
        c = Inputs(plan, D, G, family, seed + pi)
        what = f"{plan} D={D} G={G} {family}"
        q, o0, K1, V1 = c.probe(mx, 0)
        st = c.pos < c.n_ctx
        assert not np.isnan(o0[st]).any(), f"{what}: NaN in the attention output (a read past pos)"
        res = check_finish(c, q, K1, V1, what) + ((check_attention(c, q, o0, K1, V1, what),) if family == "real" else (0.0,))
        worst = [max(a, b) for a, b in zip(worst, res)]
        if fin:
            _, o1, K2, V2 = c.probe(mx, 1)
            assert np.array_equal(K1, K2) and np.array_equal(V1, V2), f"{what}: FIN's stored K / V != the finish kernel's"
            assert o0[st].tobytes() == o1[st].tobytes(), f"{what}: FIN's attention output != finish + plain attention"
    print(f"D={D} G={G} {family} ({'FIN plans' if fin else 'prompt chunks'}): float32 NumPy vs float64 {worst[0]:.3g}; kernel q "
          f"{worst[1]:.3g}, K beyond half an f16 ulp {worst[2]:.3g}; attention worst |out - ref| / (2^-10 A) {worst[3]:.3f}")


@pytest.mark.parametrize("family", ["int", "real"])
@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_fin_plans(mx, geom, family):
    """Both kernels on every mode 1 plan of the attention test: the finish kernel against float64 (q, K, V, untouched
    cache), the attention output against float64 ("real"), and FIN bitwise the finish kernel + the plain attention."""
    D, G = GEOMS[geom]
    run_plans(mx, FIN_PLANS, D, G, family, 100 * geom, True)


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_prompt_chunks(mx, geom):
    """qkn_finish_kernel with rows of one slot at consecutive positions (blockIdx.y 0..7), both families."""
    D, G = GEOMS[geom]
    for family in ("int", "real"):
        run_plans(mx, CHUNK_PLANS, D, G, family, 200 * geom, False)


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_a_zero_head(mx, geom):
    D, G = GEOMS[geom]
    plan = next(p for p in FIN_PLANS if len(p.rows) == 17 and p.nslab == 4 and p.n_ctx == 512)
    r, h, kvh = 6, NKV * G - 1, 1
    assert plan.rows[r][1] < plan.n_ctx
    c = Inputs(plan, D, G, "int", 300 + geom, zero=(r, h, kvh))
    assert not c.sum[r, h * D:(h + 1) * D].any() and c.sum[r].any()
    st = c.pos < c.n_ctx
    for mode in (0, 1):
        q, o, K1, V1 = c.probe(mx, mode)
        if mode == 0:
            check_finish(c, q, K1, V1, f"zero head D={D} G={G}")
            assert not q[r, h * D:(h + 1) * D].any(), "q of the zero head"
        assert not K1[c.slot[r], kvh, c.pos[r]].view(np.float16).any(), f"mode {mode}: stored K of the zero head"
        assert np.isfinite(o[st]).all(), f"mode {mode}: attention output"
        assert np.isfinite(K1[c.slot[st], :, c.pos[st]].view(np.float16).astype(np.float32)).all()


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_batch_invariance_of_fin_with_the_norm(mx, geom):
    """Family (e) of the attention test on the FIN instances with the norm weights."""
    D, G = GEOMS[geom]
    for ns in (4, 8):
        plan = next(p for p in FIN_PLANS if len(p.rows) == 64 and p.nslab == ns)
        c = Inputs(plan, D, G, "real", 400 + geom)
        _, full, K64, V64 = c.probe(mx, 1)
        _, part, K17, V17 = c.probe(mx, 1, idx=slice(0, 17))
        st = c.pos[:17] < c.n_ctx
        assert not np.isnan(part[st]).any()
        assert part[st].tobytes() == full[:17][st].tobytes(), f"D={D} G={G} nslab {ns}: rows at M=17 != at M=64"
        for K, V in ((K17, K64), (V17, V64)):
            assert np.array_equal(K[c.slot[:17][st], :, c.pos[:17][st]], V[c.slot[:17][st], :, c.pos[:17][st]]), "stored K / V"
    c = Inputs(Plan(1, [(i, EDGE[i + 3]) for i in range(16)], nslab=1), D, G, "real", 500 + geom)
    _, full, K16, V16 = c.probe(mx, 1)
    for i in (0, 7, 15):
        _, one, K1, V1 = c.probe(mx, 1, idx=slice(i, i + 1))
        assert not np.isnan(one).any()
        assert one[0].tobytes() == full[i].tobytes(), f"D={D} G={G}: row {i} at M=1 != among 16"
        assert np.array_equal(K1[c.slot[i], :, c.pos[i]], K16[c.slot[i], :, c.pos[i]])
        assert np.array_equal(V1[c.slot[i], :, c.pos[i]], V16[c.slot[i], :, c.pos[i]])


def test_bad_arguments(mx):
    """mode 1 takes every row in its own slot; mode 0 distinct (slot, position) pairs among the rows below n_ctx;
    everything else as before.  A refusal is MX_ERR_ARG."""
    D, n_ctx = 64, 128

    def call(mode=0, n_head=4, n_head_kv=2, head_dim=D, pos=(5, 6), slot=(0, 1), nslab=2, n_slots=4):
        M = len(pos)
        cache = np.zeros(max(n_slots, 0) * max(n_head_kv, 0) * kv_layout.ctx_stride(n_ctx) * max(head_dim, 0), np.uint16)
        slabs = np.ones((nslab, M, (n_head + 2 * n_head_kv) * head_dim), np.float32)
        cs = np.ones((n_ctx, head_dim // 2, 2), np.float32)
        w = np.ones(head_dim, np.float32)
        return mx.qkn_probe(mode, n_head, n_head_kv, head_dim, n_ctx, n_slots, list(pos), list(slot), cache, cache, slabs, cs,
                            w, w, EPS)

    try:
        for kw in (dict(mode=0), dict(mode=1), dict(mode=0, slot=(2, 2)), dict(mode=0, pos=(n_ctx, n_ctx), slot=(1, 1)),
                   dict(mode=0, pos=(7, 7), slot=(0, 1)), dict(mode=1, pos=(7, 7))):
            assert call(**kw)[1].shape == (2, 4 * D), kw
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:
            pytest.exit(f"HIP error, nothing more is launched: {e}", returncode=3)
        raise
    bad = [(dict(mode=1, slot=(2, 2)), "mode 1"), (dict(mode=1, pos=(n_ctx, n_ctx), slot=(1, 1)), "mode 1"),
           (dict(mode=0, pos=(9, 9), slot=(3, 3)), "mode 0"), (dict(mode=0, pos=(9, 4, 9), slot=(3, 3, 3)), "mode 0"),
           (dict(mode=2), ""), (dict(mode=-1), ""), (dict(head_dim=96), ""), (dict(n_head=6), ""), (dict(n_head=3), ""),
           (dict(pos=(), slot=()), ""), (dict(pos=[1] * 65, slot=list(range(65)), n_slots=70), ""), (dict(nslab=0), ""),
           (dict(nslab=9), ""), (dict(slot=(0, 4)), ""), (dict(slot=(0, -1)), ""), (dict(pos=(0, -1)), ""),
           (dict(pos=(0, n_ctx + 1)), "")]
    for kw, msg in bad:
        with pytest.raises(mx.MxError) as ei:
            call(**kw)
        assert ei.value.code == mx.MX_ERR_ARG and msg in str(ei.value), f"{kw}: {ei.value}"
