"""attn_decode_kernel / attn_prefill_kernel on crafted q / K / V through mx_attention_probe -- no model.

Every launch goes through the production launchers (launch_attention, launch_attention_prefill); the caches
are tiled here in numpy (tests/kv_layout.py, from the layout sentence of DESIGN.md §3) and every cache
position after a slot's last used one holds f16 NaN (0x7E00) in K and V, so a read past `pos` that reaches
the result shows as NaN; the probe pre-fills the output with 0xFF bytes, so an element never written shows
as NaN too.  n_kv = 2 everywhere; geometries D in {64, 128} x G in {1, 2, 4, 8}.

Launch plans (PLANS): n_ctx 512 --
  mode 0 (decode, final q): M = 16, 5, 1 (8 waves; 4 for G = 1) and M = 128 (the 4-wave form), one row with
    pos == n_ctx;
  mode 1 (decode finishing q/k/v from split-K slabs, FIN): M in {17, 33, 64} x nslab in {1, 4, 5, 8}
    (MS = 4 and MS = 8), one row per slot, one row with pos == n_ctx where M >= 33;
  mode 2 (prefill): M = 16; 100 (partial last block); 48 as three blocks of different slots starting at 16,
    240, 256; 32 = a block starting at 5 + a block 500..511 ending in four copies of its last row;
plus n_ctx = 100 (ctx_stride 128, not a chunk multiple: positions 99 and 100) and n_ctx = 2048 (2 slots,
position 2047) in every mode.  Decode rows walk the edge set EDGE (chunk seams at 32, wave rounds at 128 /
256, partial last chunks).

Families, each over every geometry x plan x both output types:
 (a) coverage, exact: q = 0 (every P is exactly 1), V[p][d] = [p % D == d] -> out[d] = count / ctx.  f32:
     relative 1e-6 (at most three f32 roundings); bf16: one bf16 ulp.  One key dropped, doubled or over-read
     moves a count by >= 1 (>= 1/32 relative at ctx 2048 = 8 bf16 ulp).
 (b) peak: per (row, head) one target key (0, pos, chunk / wave seams <= pos, different per head): q = +-16 e_j,
     K[target] = +-32 e_j (one code = dim and sign per target position of a (slot, kv head), so rows sharing a
     slot agree), other K entries 0.25 N(0,1); V[p][0:4] = (p // 64, p % 64, slot, kv head).  The reference's
     score gap is asserted >= 30, so the other keys weigh < 2048 e^-30; out[0:4] must equal the target's code to
     1e-6 (relative to max(1, |value|)).  Pins slot, kv head, head -> row mapping and per-position tile
     addressing; in mode 1 target == pos pins the FIN path's LDS patch.
 (c) random vs float64 (kv_layout.ref_attention): q ~ N(0,1), K ~ 0.5 N(0,1), V ~ N(0,1).  Per element
     |out - ref| <= 2^-10 A, A = sum_j p_j |v_j|; bf16 output adds 2^-8 |ref|.  Derivation: P is rounded to f16
     before P.V while l sums the unrounded e, so the worst case is 2^-11 A (every rounding aligned with the sign
     of v); 2^-10 doubles that for the f32 accumulation and the v_exp_f32 ulps.  Asserted on the reference:
     score spread <= 9, so no P falls below f16's smallest normal.  The worst ratio per mode is printed.
 (d) FIN stores (mode 1): V at (slot, kv head, pos) == f16 of the f32 slab sum in slab order, bitwise; K within
     one f16 ulp of f16(RoPE of that sum) (rope4's fma recomputed through float64 can double-round); every
     other element of both caches bitwise unchanged; rows with pos == n_ctx write nothing.  With G = 1 (MHA
     dispatch) and nslab = 8, slabs 4..7 carry values that change every result.
 (e) batch invariance: mode 0, a row alone == the same row among 16; mode 1, the same rows at M = 17 and at
     M = 64 -- bitwise.  M >= 128 runs 4 waves per work-group instead of 8 (another chunk-to-wave assignment
     and merge order) and is not expected to equal the 8-wave form bitwise: out of scope.
 (f) every argument the probe must refuse raises MxError and launches nothing.
"""
import functools

import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

NKV = 2
GEOMS = [(D, G) for D in (64, 128) for G in (1, 2, 4, 8)]
GEOM_IDS = [f"D{D}-G{G}" for D, G in GEOMS]
EDGE = [0, 1, 7, 8, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 255, 256, 257, 287, 511]
SEAMS = [31, 32, 63, 64, 127, 128, 255, 256, 257, 1023, 1024]
NAN16 = 0x7E00
NSLABS = [1, 4, 5, 8]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


class Plan:
    def __init__(self, mode, rows, n_ctx=512, nslab=0, n_slots=None):
        self.mode, self.rows, self.n_ctx, self.nslab = mode, rows, n_ctx, nslab
        self.n_slots = n_slots if n_slots is not None else max(s for s, _ in rows) + 1

    def __repr__(self):
        return f"mode {self.mode} M={len(self.rows)} n_ctx={self.n_ctx} nslab={self.nslab}"


def block(slot, start, n=16, last=None):
    """n rows of consecutive positions from `start`; past `last`, copies of the row at `last`."""
    return [(slot, min(start + i, last if last is not None else start + i)) for i in range(n)]


def make_plans():
    P = []
    # mode 0
    P.append(Plan(0, [(i, EDGE[i]) for i in range(16)]))
    P.append(Plan(0, [(0, 257), (1, 287), (2, 511), (3, 300), (4, 512)]))
    P.append(Plan(0, [(0, 200)]))
    P.append(Plan(0, [(i % 64, EDGE[i % 19] if i < 64 else (37 * i + 11) % 512) for i in range(128)]))
    # mode 1: one row per slot, the edge set rotated so that every M meets every position
    for M in (17, 33, 64):
        for k, ns in enumerate(NSLABS):
            rows = [((7 * i + 3) % M, EDGE[(i + 5 * k) % 19]) for i in range(M)]
            if M >= 33:
                rows[20] = (rows[20][0], 512)
            P.append(Plan(1, rows, nslab=ns))
    # mode 2
    P.append(Plan(2, block(0, 0)))
    P.append(Plan(2, [(0, p) for p in range(100)]))
    P.append(Plan(2, block(2, 16) + block(0, 240) + block(1, 256)))
    P.append(Plan(2, block(0, 5) + block(1, 500, last=511)))
    # n_ctx = 100: ctx_stride 128, the last chunk 96..99 is partial
    P.append(Plan(0, [(0, 99), (1, 100), (2, 0), (3, 64), (4, 95)], n_ctx=100))
    P.append(Plan(1, [((5 * i + 1) % 17, [99, 100, 96, 95, 64, 63, 32, 31, 0, 1, 97, 98, 33, 16, 15, 8, 7][i])
                      for i in range(17)], n_ctx=100, nslab=4))
    P.append(Plan(2, [(0, p) for p in range(100)], n_ctx=100))
    # n_ctx = 2048, two slots
    P.append(Plan(0, [(1, 2047), (0, 2048)], n_ctx=2048))
    P.append(Plan(1, [(1, 2047), (0, 2048)], n_ctx=2048, nslab=8))
    P.append(Plan(2, block(1, 2032), n_ctx=2048, n_slots=2))
    return P


PLANS = make_plans()


@functools.lru_cache(maxsize=None)
def bank():
    """Two fixed N(0,1) f32 streams, long enough for the largest caches (64 slots x 2 x 512 x 128)."""
    rng = np.random.default_rng(20260)
    n = 64 * NKV * 512 * 128
    a, b = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def dyadic(x):
    """Multiples of 2^-10: sums of a few of them with small integers are exact in f32."""
    return np.round(np.asarray(x, np.float64) * 1024.0) / 1024.0


def rope_table(n_ctx, D, identity=False):
    cs = np.zeros((n_ctx, D // 2, 2), np.float32)
    if identity:
        cs[..., 0] = 1.0
        return cs
    th = np.arange(n_ctx, dtype=np.float64)[:, None] * 10000.0 ** (-2.0 * np.arange(D // 2) / D)[None, :]
    cs[..., 0], cs[..., 1] = np.cos(th), np.sin(th)
    return cs


def rope_f32(x, cs):
    """rope4 (device_common.h) on x [..., D] f32 with cs [D/2][2]: o0 = fma(s0, c0, -(s1*c1)), o1 = fma(s0, c1,
    s1*c0); the inner product is rounded to f32, the fma formed in float64 and rounded once more."""
    s0, s1 = x[..., 0::2], x[..., 1::2]
    c0, c1 = cs[:, 0], cs[:, 1]
    t0, t1 = (s1 * c1).astype(np.float32), (s1 * c0).astype(np.float32)
    o = np.empty_like(x)
    o[..., 0::2] = (s0.astype(np.float64) * c0 - t0).astype(np.float32)
    o[..., 1::2] = (s0.astype(np.float64) * c1 + t1).astype(np.float32)
    return o


def slab_sum(slabs):
    v = slabs[0].copy()
    for k in range(1, len(slabs)):
        v = v + slabs[k]  # f32, slab order
    return v


class Case:
    """One plan at one geometry: logical caches K, V [n_slots][NKV][S][D] f16, q [M][H][D] f32, and in mode 1
    the slabs, the RoPE table and each row's new key / value (knew, vnew [M][NKV][D] f32)."""

    def __init__(self, plan, D, G, seed):
        self.plan, self.D, self.G, self.H = plan, D, G, NKV * G
        self.mode, self.rows, self.n_ctx, self.n_slots = plan.mode, plan.rows, plan.n_ctx, plan.n_slots
        self.M = len(self.rows)
        self.S = L.ctx_stride(self.n_ctx)
        self.scale = 1.0 / np.sqrt(D)
        self.rng = np.random.default_rng(seed)
        self.shape = (self.n_slots, NKV, self.S, D)
        self.slot_len = [self.n_ctx] * self.n_slots  # valid positions before the launch
        used = {}
        for s, p in self.rows:
            used[s] = max(used.get(s, -1), p)
        for s, p in used.items():
            self.slot_len[s] = min(self.n_ctx, p if self.mode == 1 else p + 1)
        self.q = np.zeros((self.M, self.H, D), np.float32)
        self.knew = self.vnew = self.slabs = self.cs = None
        self._tiled = None

    def ctx(self, i):
        return min(self.rows[i][1] + 1, self.n_ctx)

    def stores(self, i):  # mode 1: does row i write its position?
        return self.mode == 1 and self.rows[i][1] < self.n_ctx

    def bank_caches(self, kscale):
        a, b = bank()
        n = int(np.prod(self.shape))
        self.K = (a[:n] * np.float32(kscale)).astype(np.float16).reshape(self.shape)
        self.V = b[:n].astype(np.float16).reshape(self.shape)

    def slabs_from_totals(self):
        """Exact split of q | knew | vnew (dyadic) into nslab slabs; identity RoPE table."""
        M, ns = self.M, self.plan.nslab
        tot = np.concatenate([self.q.reshape(M, -1), self.knew.reshape(M, -1), self.vnew.reshape(M, -1)], axis=1)
        tot = tot.astype(np.float64)
        assert np.array_equal(tot, dyadic(tot))
        parts = self.rng.integers(-32, 33, (ns - 1,) + tot.shape) / 8.0
        sl = np.concatenate([(tot - parts.sum(axis=0))[None], parts]).astype(np.float32)
        assert np.array_equal(slab_sum(sl), tot.astype(np.float32))
        self.slabs, self.cs = sl, rope_table(self.n_ctx, self.D, identity=True)

    def effective(self, i, kvh):
        """K, V [S][D] f16 that row i's heads of kv head kvh attend (mode 1: with its own new position)."""
        s, p = self.rows[i]
        K, V = self.K[s, kvh], self.V[s, kvh]
        if self.stores(i):
            K, V = K.copy(), V.copy()
            K[p], V[p] = self.knew[i, kvh].astype(np.float16), self.vnew[i, kvh].astype(np.float16)
        return K, V

    def tiled(self):
        if self._tiled is None:
            K, V = self.K.view(np.uint16).copy(), self.V.view(np.uint16).copy()
            for s in range(self.n_slots):
                K[s, :, self.slot_len[s]:] = NAN16
                V[s, :, self.slot_len[s]:] = NAN16
            self.K_in, self.V_in = K, V
            self._tiled = L.tile_k(K).reshape(-1), L.tile_v(V).reshape(-1)
        return self._tiled

    def launch(self, mx, out_f32, idx=None):
        """-> out [len(idx)][H][D] f32, K after, V after (logical, uint16 bits)."""
        idx = list(range(self.M)) if idx is None else idx
        kc, vc = self.tiled()
        slot, pos = [self.rows[i][0] for i in idx], [self.rows[i][1] for i in idx]
        kw = dict(slabs=self.slabs[:, idx], rope_cs=self.cs) if self.mode == 1 else \
            dict(q=self.q[idx].reshape(len(idx), -1))
        try:
            out, ka, va = mx.attention_probe(self.mode, self.H, NKV, self.D, self.n_ctx, self.n_slots, pos, slot, kc,
                                             vc, out_f32=out_f32, **kw)
        except mx.MxError as e:
            if e.code == mx.MX_ERR_HIP:  # nothing more is started on a device that reported an error
                pytest.exit(f"{self.plan} D={self.D} G={self.G}: {e}", returncode=3)
            raise
        assert not np.isnan(out).any(), f"{self.plan}: NaN in the output (a read past pos, or an element not written)"
        return (out.reshape(len(idx), self.H, self.D), L.untile_k(ka.reshape(self.n_slots, NKV, -1), self.D),
                L.untile_v(va.reshape(self.n_slots, NKV, -1), self.D))


# ---------------------------------------------------------------------------------------------- families
def cover_case(plan, D, G, seed):
    c = Case(plan, D, G, seed)
    c.bank_caches(0.5)
    c.V = np.zeros(c.shape, np.float16)
    p = np.arange(c.S)
    c.V[:, :, p, p % D] = 1.0
    if c.mode == 1:
        c.knew = dyadic(0.5 * c.rng.standard_normal((c.M, NKV, D))).astype(np.float32)
        c.vnew = np.zeros((c.M, NKV, D), np.float32)
        for i, (_, pos) in enumerate(c.rows):
            c.vnew[i, :, pos % D] = 1.0
        c.slabs_from_totals()
    return c


def bf16_ulp(x):
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-30))) - 7), 0.0)


def check_cover(c, out, out_f32):
    for i in range(c.M):
        ctx = c.ctx(i)
        count = np.maximum(0, (ctx - np.arange(c.D) + c.D - 1) // c.D).astype(np.float32)  # keys p < ctx, p % D == d
        want = (count / np.float32(ctx)).astype(np.float64)
        tol = 1e-6 * want if out_f32 else bf16_ulp(want)
        err = np.abs(out[i].astype(np.float64) - want[None, :])
        assert (err <= tol[None, :]).all(), (f"{c.plan} D={c.D} G={c.G} row {i} pos {c.rows[i][1]} "
                                             f"{'f32' if out_f32 else 'bf16'}: count/ctx off by up to "
                                             f"{(err * ctx).max():.3g} keys")


def peak_case(plan, D, G, seed):
    c = Case(plan, D, G, seed)
    c.bank_caches(0.25)
    enc = np.zeros(c.shape[:3] + (4,), np.float16)
    p = np.arange(c.S)
    enc[..., 0], enc[..., 1] = (p // 64)[None, None, :], (p % 64)[None, None, :]
    enc[..., 2], enc[..., 3] = np.arange(c.n_slots)[:, None, None], np.arange(NKV)[None, :, None]
    c.V[..., :4] = enc
    if c.mode == 1:
        c.knew = dyadic(0.25 * c.rng.standard_normal((c.M, NKV, D))).astype(np.float32)
        c.vnew = dyadic(c.rng.standard_normal((c.M, NKV, D))).astype(np.float32)
    codes, order = {}, {}
    c.target = np.zeros((c.M, c.H), np.int64)
    for i, (s, pos) in enumerate(c.rows):
        ctx = c.ctx(i)
        cand = sorted({0, ctx - 1, (ctx - 1) // 32 * 32} | {x for x in SEAMS if x < ctx})
        for h in range(c.H):
            kvh = h // G
            t = cand[(i + h) % len(cand)]
            key = (s, kvh)
            if key not in order:
                order[key], codes[key] = c.rng.permutation(2 * D), {}
            if t not in codes[key]:
                assert len(codes[key]) < 2 * D, "more target positions than codes in one (slot, kv head)"
                codes[key][t] = int(order[key][len(codes[key])])
            code = codes[key][t]
            dim, sign = code % D, 1.0 if code < D else -1.0
            c.q[i, h, dim] = 16.0 * sign
            c.target[i, h] = t
    for (s, kvh), tab in codes.items():
        for t, code in tab.items():
            row = np.zeros(D, np.float32)
            row[code % D] = 32.0 if code < D else -32.0
            if t < c.slot_len[s]:
                c.K[s, kvh, t] = row
            else:  # mode 1: the row's own new position
                (i,) = [j for j, (s2, p2) in enumerate(c.rows) if s2 == s and p2 == t]
                c.knew[i, kvh] = row
    if c.mode == 1:
        for i, (s, pos) in enumerate(c.rows):
            for kvh in range(NKV):
                c.vnew[i, kvh, :4] = (pos // 64, pos % 64, s, kvh)
        c.slabs_from_totals()
    return c


def check_peak(c, outs):
    for i, (s, pos) in enumerate(c.rows):
        for kvh in range(NKV):
            K, V = c.effective(i, kvh)
            hs = slice(kvh * c.G, (kvh + 1) * c.G)
            sc = c.q[i, hs].astype(np.float16).astype(np.float64) @ K[:c.ctx(i)].astype(np.float64).T * c.scale
            ref, _, _ = L.ref_attention(c.q[i, hs], K, V, pos, c.scale, c.n_ctx)
            for g, h in enumerate(range(kvh * c.G, (kvh + 1) * c.G)):
                t = int(c.target[i, h])
                others = np.delete(sc[g], t)
                assert sc[g].argmax() == t and (others.size == 0 or sc[g, t] - others.max() >= 30.0), "reference gap < 30"
                want = np.array([t // 64, t % 64, s, kvh], np.float64)
                assert np.abs(ref[g, :4] - want).max() <= 1e-6
                for out in outs:
                    err = np.abs(out[i, h, :4] - want)
                    assert (err <= 1e-6 * np.maximum(1.0, want)).all(), (
                        f"{c.plan} D={c.D} G={c.G} row {i} (slot {s}, pos {pos}) head {h}: found "
                        f"(p//64, p%64, slot, kvh) = {out[i, h, :4].tolist()}, target key {t} = {want.tolist()}")


def random_case(plan, D, G, seed):
    c = Case(plan, D, G, seed)
    c.bank_caches(0.5)
    if c.mode != 1:
        c.q = c.rng.standard_normal(c.q.shape).astype(np.float32)
        return c
    ns, nq, nkv = plan.nslab, c.H * D, NKV * D
    sl = (c.rng.standard_normal((ns, c.M, nq + 2 * nkv)) / np.sqrt(ns)).astype(np.float32)
    sl[:, :, nq:nq + nkv] *= np.float32(0.5)
    c.slabs, c.cs = sl, rope_table(c.n_ctx, D)
    tot = slab_sum(sl)
    qs, ks = tot[:, :nq].reshape(c.M, c.H, D), tot[:, nq:nq + nkv].reshape(c.M, NKV, D)
    c.vnew = tot[:, nq + nkv:].reshape(c.M, NKV, D).copy()
    c.knew = np.zeros_like(ks)
    for i, (_, pos) in enumerate(c.rows):
        if pos < c.n_ctx:
            c.q[i], c.knew[i] = rope_f32(qs[i], c.cs[pos]), rope_f32(ks[i], c.cs[pos])
        else:  # nothing is stored and q takes no RoPE: the row attends [0, n_ctx) as it is
            c.q[i] = qs[i]
    return c


def check_random(c, outs):
    """outs: {out_f32: out}.  -> {out_f32: worst |out - ref| / tolerance}."""
    worst = {k: 0.0 for k in outs}
    for i, (s, pos) in enumerate(c.rows):
        for kvh in range(NKV):
            K, V = c.effective(i, kvh)
            hs = slice(kvh * c.G, (kvh + 1) * c.G)
            ref, A, spread = L.ref_attention(c.q[i, hs], K, V, pos, c.scale, c.n_ctx)
            assert spread.max() <= 9.0, f"input condition: score spread {spread.max():.2f} > 9"
            for out_f32, out in outs.items():
                tol = 2.0 ** -10 * A + (0.0 if out_f32 else 2.0 ** -8 * np.abs(ref))
                ratio = float((np.abs(out[i, hs] - ref) / tol).max())
                assert ratio <= 1.0, (f"{c.plan} D={c.D} G={c.G} row {i} (slot {s}, pos {pos}) kv head {kvh} "
                                      f"{'f32' if out_f32 else 'bf16'}: |out - ref| = {ratio:.3g} x tolerance")
                worst[out_f32] = max(worst[out_f32], ratio)
    return worst


def f16_ordinal(bits):
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def check_fin_stores(c, ka, va):
    want_k, want_v = c.K_in.copy(), c.V_in.copy()
    for i, (s, pos) in enumerate(c.rows):
        if not c.stores(i):
            continue  # pos == n_ctx: nothing written
        v16 = c.vnew[i].astype(np.float16).view(np.uint16)
        assert np.array_equal(va[s, :, pos], v16), f"{c.plan} D={c.D} G={c.G} row {i}: stored V != f16(slab sum)"
        k16 = c.knew[i].astype(np.float16).view(np.uint16)
        d = np.abs(f16_ordinal(ka[s, :, pos]) - f16_ordinal(k16))
        assert d.max() <= 1, f"{c.plan} D={c.D} G={c.G} row {i}: stored K is {d.max()} f16 ulp from RoPE(slab sum)"
        want_k[s, :, pos], want_v[s, :, pos] = ka[s, :, pos], va[s, :, pos]
    assert np.array_equal(ka, want_k), f"{c.plan} D={c.D} G={c.G}: K cache changed outside the rows' positions"
    assert np.array_equal(va, want_v), f"{c.plan} D={c.D} G={c.G}: V cache changed outside the rows' positions"


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_coverage_exact(mx, geom):
    D, G = GEOMS[geom]
    for pi, plan in enumerate(PLANS):
        c = cover_case(plan, D, G, 1000 * geom + pi)
        for out_f32 in (True, False):
            out, _, _ = c.launch(mx, out_f32)
            check_cover(c, out, out_f32)


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_peak_finds_the_target_key(mx, geom):
    D, G = GEOMS[geom]
    for pi, plan in enumerate(PLANS):
        c = peak_case(plan, D, G, 2000 * geom + pi)
        check_peak(c, [c.launch(mx, out_f32)[0] for out_f32 in (True, False)])


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_random_vs_float64(mx, geom):
    D, G = GEOMS[geom]
    worst = {}
    for pi, plan in enumerate(PLANS):
        c = random_case(plan, D, G, 3000 * geom + pi)
        for out_f32, r in check_random(c, {f: c.launch(mx, f)[0] for f in (True, False)}).items():
            key = (plan.mode, "f32" if out_f32 else "bf16")
            worst[key] = max(worst.get(key, 0.0), r)
    for (mode, ty), r in sorted(worst.items()):
        print(f"attention vs float64, D={D} G={G} mode {mode} {ty}: worst |out - ref| / tolerance = {r:.3f}")


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_fin_stores(mx, geom):
    D, G = GEOMS[geom]
    for pi, plan in enumerate(PLANS):
        if plan.mode != 1:
            continue
        c = random_case(plan, D, G, 3000 * geom + pi)
        _, ka, va = c.launch(mx, True)
        check_fin_stores(c, ka, va)


@pytest.mark.parametrize("geom", range(len(GEOMS)), ids=GEOM_IDS)
def test_batch_invariance_of_the_kernel(mx, geom):
    """8-wave (G = 1: 4-wave) forms only; M >= 128 changes the wave count and is out of scope (see above)."""
    D, G = GEOMS[geom]
    for out_f32 in (True, False):
        c = random_case(PLANS[0], D, G, 4000 + geom)  # mode 0, 16 rows
        full, _, _ = c.launch(mx, out_f32)
        for i in (0, 5, 9, 12, 15):
            alone, _, _ = c.launch(mx, out_f32, idx=[i])
            assert alone[0].tobytes() == full[i].tobytes(), f"mode 0 D={D} G={G}: row {i} alone != among 16"
        for ns in (4, 8):
            plan = next(p for p in PLANS if p.mode == 1 and len(p.rows) == 64 and p.nslab == ns)
            c = random_case(plan, D, G, 5000 + geom)
            full, _, _ = c.launch(mx, out_f32)
            part, _, _ = c.launch(mx, out_f32, idx=list(range(17)))
            assert part.tobytes() == full[:17].tobytes(), f"mode 1 D={D} G={G} nslab {ns}: rows at M=17 != at M=64"


def test_bad_arguments_are_refused(mx):
    D, n_ctx, n_slots = 64, 128, 70

    def call(mode=0, n_head=4, n_head_kv=2, head_dim=D, pos=(5, 6), slot=(0, 1), nslab=2, n_slots=n_slots):
        M = len(pos)
        S = L.ctx_stride(n_ctx)
        cache = np.zeros(max(n_slots, 0) * max(n_head_kv, 0) * S * max(head_dim, 0), np.uint16)
        nq, N = n_head * head_dim, (n_head + 2 * n_head_kv) * head_dim
        kw = dict(q=np.zeros((M, nq), np.float32))
        if mode == 1:
            kw = dict(slabs=np.zeros((nslab, M, N), np.float32), rope_cs=rope_table(n_ctx, head_dim, identity=True))
        return mx.attention_probe(mode, n_head, n_head_kv, head_dim, n_ctx, n_slots, list(pos), list(slot), cache,
                                  cache, **kw)

    blk = list(range(16))
    for mode in (0, 1, 2):  # the base call of every mode is accepted
        out, _, _ = call(mode=mode, pos=blk if mode == 2 else (5, 6), slot=[3] * 16 if mode == 2 else (0, 1))
        assert np.array_equal(out, np.zeros_like(out))
    assert call(pos=(n_ctx, 0))[0].shape == (2, 4 * D)  # pos == n_ctx is accepted
    bad = [
        dict(head_dim=96), dict(n_head=6), dict(n_head=32), dict(n_head=3), dict(n_head_kv=0, n_head=0),
        dict(mode=3), dict(mode=-1),
        dict(pos=(), slot=()), dict(pos=[0] * 4097, slot=[0] * 4097),
        dict(slot=(0, -1)), dict(slot=(0, n_slots)), dict(pos=(0, -1)), dict(pos=(0, n_ctx + 1)),
        dict(mode=1, nslab=0), dict(mode=1, nslab=9), dict(mode=1, slot=(4, 4)),
        dict(mode=1, pos=[1] * 65, slot=list(range(65))),
        dict(mode=2, pos=blk, slot=[0] * 8 + [1] * 8), dict(mode=2, pos=blk[:8] + [9] + blk[9:], slot=[0] * 16),
        dict(mode=2, pos=[0, 2], slot=[0, 0]),
    ]
    for kw in bad:
        with pytest.raises(mx.MxError) as ei:
            call(**kw)
        assert ei.value.code == mx.MX_ERR_ARG, f"{kw}: {ei.value}"
