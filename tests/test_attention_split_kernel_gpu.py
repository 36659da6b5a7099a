"""attn_split_kernel + attn_merge_kernel on crafted q / K / V through mx_attention_long_probe -- no model.

One kv head, two slots, n_ctx just large enough per case.  Every cache position past a slot's used length holds f16
NaN and the probe pre-fills the output and the workspace with 0xFF bytes, so a key read past ctx, an element never
written or a segment record read before it was stored shows as NaN.  The reference is kv_layout.ref_attention
(float64 over the f16 K / V, q rounded to f16) and the bound the one of test_attention_kernel_gpu.check_random:
|out - ref| <= 2^-10 A, A = sum_j p_j |v_j|, plus 2^-8 |ref| for bf16 output.  The threshold T, the cap and seg_len
come from the build (mx_attention_split_plan); the contexts are derived from them.
"""
import functools

import numpy as np
import pytest

import kv_layout as L

pytestmark = pytest.mark.gpu

GEOMS = [(64, 1), (128, 4), (128, 8), (64, 7)]
PARAMS = [(D, G, f) for D, G in GEOMS for f in (True, False)]
IDS = [f"D{D}-G{G}-{'f32' if f else 'bf16'}" for D, G, f in PARAMS]
NAN16 = 0x7E00


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


@functools.lru_cache(maxsize=None)
def plan_facts():
    """(T, smallest ctx of nseg_max segments, a ctx above it whose seg_len is longer and does not divide it)."""
    from llama_p2p_amd.engine import attention_split_plan as plan

    T, cap_n = plan(1)["threshold"], plan(1)["nseg_max"]
    cap = next(c for c in range(T + 1, 1 << 18) if plan(c)["nseg"] == cap_n)
    above = cap_n * plan(cap)["seg_len"] + 563
    assert plan(T)["nseg"] == 1 < plan(T + 1)["nseg"] and plan(above)["seg_len"] > plan(cap)["seg_len"]
    assert above % plan(above)["seg_len"] and plan(above)["nseg"] > 1
    return T, cap, above


def contexts():
    """name -> (ctx, n_ctx, pos): every context at which the split kernels take another path."""
    from llama_p2p_amd.engine import attention_split_plan as plan

    T, cap, above = plan_facts()
    seam = 12 * plan(T + 1)["seg_len"]  # k * seg_len inside the shortest-segment range
    assert T < seam - 1 and plan(seam + 1)["seg_len"] == plan(T + 1)["seg_len"]
    C = {"first-split": T + 1, "seam-1": seam - 1, "seam": seam, "seam+1": seam + 1, "cap": cap, "above-cap": above}
    out = {k: (c, c, c - 1) for k, c in C.items()}
    out["clamp"] = (T + 100, T + 100, T + 100)  # pos == n_ctx, n_ctx no multiple of 32: the last chunk is partial
    return out


@functools.lru_cache(maxsize=None)
def bank(D):
    """K (0.5 N(0,1)) and V (N(0,1)) [2][S][D] f16 for the longest case, and q [4][8][D] f32."""
    rng = np.random.default_rng(31000 + D)
    S = L.ctx_stride(plan_facts()[2])
    K = (0.5 * rng.standard_normal((2, S, D), dtype=np.float32)).astype(np.float16)
    V = rng.standard_normal((2, S, D), dtype=np.float32).astype(np.float16)
    q = rng.standard_normal((4, 8, D), dtype=np.float32)
    for a in (K, V, q):
        a.setflags(write=False)
    return K, V, q


def launch(mx, D, G, n_ctx, rows, K, V, q, out_f32, split=True):
    """rows [(slot, pos)], K / V [2][>= S][D] f16 (NaN written past each slot's largest context), q [M][G][D]
    -> out [M][G][D] f32."""
    S = L.ctx_stride(n_ctx)
    Kb, Vb = K[:, None, :S].view(np.uint16).copy(), V[:, None, :S].view(np.uint16).copy()
    for s in (0, 1):
        used = max([min(p + 1, n_ctx) for sl, p in rows if sl == s], default=0)
        Kb[s, :, used:] = NAN16
        Vb[s, :, used:] = NAN16
    kc, vc = L.tile_k(Kb).reshape(-1), L.tile_v(Vb).reshape(-1)
    slot, pos = [r[0] for r in rows], [r[1] for r in rows]
    qf = np.ascontiguousarray(q, np.float32).reshape(len(rows), -1)
    try:
        if split:
            out, guard = mx.attention_long_probe(G, 1, D, n_ctx, 2, pos, slot, kc, vc, qf, out_f32=out_f32)
            assert guard.size == (64 - len(rows)) * G * D * (4 if out_f32 else 2) and (guard == 0xFF).all(), \
                "bytes of out past the M rows were written"
        else:
            out = mx.attention_probe(0, G, 1, D, n_ctx, 2, pos, slot, kc, vc, q=qf, out_f32=out_f32)[0]
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:  # nothing more is started on a device that reported an error
            pytest.exit(f"D={D} G={G} rows {rows}: {e}", returncode=3)
        raise
    assert not np.isnan(out).any(), f"D={D} G={G} rows {rows}: NaN (a read past ctx, or an element not written)"
    return out.reshape(len(rows), G, D)


def worst_ratio(out, q, K, V, rows, n_ctx, D, out_f32, max_spread=9.0):
    worst = 0.0
    for i, (s, p) in enumerate(rows):
        ref, A, spread = L.ref_attention(q[i], K[s], V[s], p, 1.0 / np.sqrt(D), n_ctx)
        assert max_spread is None or spread.max() <= max_spread, f"input condition: score spread {spread.max():.2f}"
        tol = 2.0 ** -10 * A + (0.0 if out_f32 else 2.0 ** -8 * np.abs(ref))
        worst = max(worst, float((np.abs(out[i] - ref) / tol).max()))
    return worst


@pytest.mark.parametrize("D,G,out_f32", PARAMS, ids=IDS)
def test_split_rows_vs_float64(mx, D, G, out_f32):
    K, V, q = bank(D)
    for name, (ctx, n_ctx, pos) in contexts().items():
        rows = [(1, pos)]  # slot 0 is NaN throughout: a wrong slot shows
        out = launch(mx, D, G, n_ctx, rows, K, V, q[:1, :G], out_f32)
        r = worst_ratio(out, q[:1, :G], K, V, rows, n_ctx, D, out_f32)
        print(f"split attention vs float64, D={D} G={G} {name} (ctx {ctx}): worst |out - ref| / tolerance = {r:.3f}")
        assert r <= 1.0, f"{name} (ctx {ctx}): |out - ref| = {r:.3g} x tolerance"


@pytest.mark.parametrize("D,G,out_f32", PARAMS, ids=IDS)
def test_one_segment_rows_equal_launch_attention(mx, D, G, out_f32):
    K, V, q = bank(D)
    T = plan_facts()[0]
    for ctx in (T, 100):
        rows = [(1, ctx - 1)]
        got = launch(mx, D, G, ctx, rows, K, V, q[:1, :G], out_f32)
        want = launch(mx, D, G, ctx, rows, K, V, q[:1, :G], out_f32, split=False)
        assert got.tobytes() == want.tobytes(), f"ctx {ctx}: a one-segment row differs from launch_attention's bits"


@pytest.mark.parametrize("D,G,out_f32", PARAMS, ids=IDS)
def test_peaked_key_in_the_last_segment(mx, D, G, out_f32):
    """Segment 0 holds the largest negative scores (-40 below the rest) and one key of the last segment stands 40
    above: a merge that takes the wrong max overflows, one that does not rescale weighs every segment alike.  The
    other keys weigh < ctx e^-30 (asserted on the reference) and V[target] = +-1, so A >= 1 - 1e-9 and the bound
    is check_random's; the spread condition of the random cases does not apply."""
    Kb, Vb, qb = bank(D)
    T = plan_facts()[0]
    from llama_p2p_amd import engine as E

    ctx = T + 1000
    pl = E.attention_split_plan(ctx)
    assert pl["nseg"] >= 3
    t = (pl["nseg"] - 1) * pl["seg_len"] + 37
    assert t < ctx
    K, V, q = Kb.copy(), Vb.copy(), qb[:1, :G].copy()
    c = np.float16(40.0 / (8.0 / np.sqrt(D)))
    q[..., 0] = 8.0
    K[1, :, 0] = 0
    K[1, :pl["seg_len"], 0] = -c
    K[1, t, 0] = c
    V[1, t] = np.where(np.arange(D) % 2, -1.0, 1.0)
    rows = [(1, ctx - 1)]
    sc = q[0].astype(np.float16).astype(np.float64) @ K[1, :ctx].astype(np.float64).T / np.sqrt(D)
    assert (sc.argmax(axis=1) == t).all() and (sc[:, t] - np.delete(sc, t, axis=1).max(axis=1) >= 30.0).all()
    assert (sc[:, :pl["seg_len"]].max(axis=1) < np.delete(sc, t, axis=1)[:, pl["seg_len"]:].min(axis=1)).all()
    out = launch(mx, D, G, ctx, rows, K, V, q, out_f32)
    r = worst_ratio(out, q, K, V, rows, ctx, D, out_f32, max_spread=None)
    print(f"split attention, peaked, D={D} G={G}: worst |out - ref| / tolerance = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("D,G,out_f32", PARAMS, ids=IDS)
def test_mixed_launch_is_row_invariant(mx, D, G, out_f32):
    K, V, q = bank(D)
    T, _, n_ctx = plan_facts()
    rows = [(0, 4), (1, T - 1), (0, T), (1, n_ctx - 1)]  # ctx 5, T, T + 1, above the cap
    full = launch(mx, D, G, n_ctx, rows, K, V, q[:, :G], out_f32)
    assert worst_ratio(full, q[:, :G], K, V, rows, n_ctx, D, out_f32) <= 1.0
    for i in range(4):
        alone = launch(mx, D, G, n_ctx, [rows[i]], K, V, q[i:i + 1, :G], out_f32)
        assert alone[0].tobytes() == full[i].tobytes(), f"row {i} (ctx {rows[i][1] + 1}) alone != among 4"
    plain = launch(mx, D, G, n_ctx, rows[:2], K, V, q[:2, :G], out_f32, split=False)
    assert plain.tobytes() == full[:2].tobytes(), "the short rows of a mixed launch differ from launch_attention's bits"


def test_bad_arguments_are_refused(mx):
    def call(n_head=4, head_dim=64, M=2):
        cache = np.zeros(2 * L.ctx_stride(128) * max(head_dim, 0), np.uint16)
        return mx.attention_long_probe(n_head, 1, head_dim, 128, 2, [5] * M, [i % 2 for i in range(M)], cache, cache,
                                       np.zeros((M, n_head * head_dim), np.float32))

    out, _ = call()
    assert np.array_equal(out, np.zeros_like(out))
    for kw in (dict(M=65), dict(head_dim=96), dict(n_head=3)):
        with pytest.raises(mx.MxError) as ei:
            call(**kw)
        assert ei.value.code == mx.MX_ERR_ARG, f"{kw}: {ei.value}"
