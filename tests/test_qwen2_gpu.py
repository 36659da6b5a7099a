"""Qwen2 / Qwen2.5 on the GPU: q/k/v bias in the QKV epilogues, NeoX RoPE by the row permutation at
load, GQA groups 5, 6 and 7.

The C oracle knows no bias, so the references are tests/qwen2_ref.py (NumPy float64 at the oracle's rounding points,
itself checked against transformers in tests/test_qwen2_host.py), the engine's own llama path where a Qwen2 file
must reproduce it bit for bit, and exact integer operands for the kernels alone.

Row regimes of the whole-model tests (n_ctx 64): "one": the 40 tokens teacher-forced as one-row steps; "chunk5" /
"chunk16": chunks of 5 / 16 rows; "slots24": one 24-row step over 24 slots that hold ids[:p], p = 8..31 (the
17..64-row walk, FIN attention); "prefill144": three copies of the sequence in three slots as one 144-row blocked
prefill (the MFMA GEMM where gemm_supported, else the GEMVs), read back by a 3-row step at positions 39, 25 and 12.
"""
import functools

import numpy as np
import pytest
from conftest import assert_logits_close, assert_tokens_match

import kv_layout
import mm_layout as L
import qwen2_ref as Q
import walk_ref
from llama_p2p_amd import gguf, synth

pytestmark = pytest.mark.gpu

N_CTX = 64
N_SEQ = 30
REGIMES = ("one", "chunk5", "chunk16", "slots24", "prefill144")
P24 = list(range(8, 32))
P144 = (39, 25, 12)


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("qwen2_gpu")


def open_engine(mx, path, **kw):
    try:
        return StopOnHipError(mx.Engine(path, n_ctx=N_CTX, n_seq_max=N_SEQ, device=0, **kw), mx)
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:  # nothing more is started on a device that reported an error
            pytest.exit(f"{path}: {e}", returncode=3)
        raise


class StopOnHipError:
    """An Engine whose forward_rows ends the session on a HIP runtime error: after a GPU fault nothing more is launched."""

    def __init__(self, eng, mx):
        self._e, self._mx = eng, mx

    def __getattr__(self, name):
        return getattr(self._e, name)

    def forward_rows(self, *a, **kw):
        try:
            return self._e.forward_rows(*a, **kw)
        except self._mx.MxError as err:
            if err.code == self._mx.MX_ERR_HIP:
                pytest.exit(f"HIP error, nothing more is launched: {err}", returncode=3)
            raise


def run_regime(eng, ids, regime):
    """-> (positions of `ids` whose logits the regime returns, logits [len][n_vocab])."""
    ids = [int(t) for t in ids]
    T = len(ids)
    if regime == "one":
        return list(range(T)), np.concatenate([eng.forward_rows([0], [p], [ids[p]]) for p in range(T)])
    if regime in ("chunk5", "chunk16"):
        c, slot = (5, 1) if regime == "chunk5" else (16, 2)
        return list(range(T)), np.concatenate([eng.forward_rows([slot] * len(ids[i:i + c]), list(range(i, min(i + c, T))),
                                                                ids[i:i + c]) for i in range(0, T, c)])
    if regime == "slots24":
        slots, pos, tok = [], [], []
        for k, p in enumerate(P24):
            slots += [3 + k] * p
            pos += list(range(p))
            tok += ids[:p]
        for i in range(0, len(slots), 64):
            assert eng.forward_rows(slots[i:i + 64], pos[i:i + 64], tok[i:i + 64], want_logits=False) is None
        return P24, eng.forward_rows([3 + k for k in range(len(P24))], P24, [ids[p] for p in P24])
    assert regime == "prefill144"
    slots, pos, tok, _ = walk_ref.blocked_layout([ids] * 3, 27, N_CTX)
    assert len(slots) == 144 and walk_ref.is_blocked(slots, pos, tok)
    assert eng.forward_rows(slots, pos, tok, want_logits=False) is None
    return list(P144), eng.forward_rows([27, 28, 29], list(P144), [ids[p] for p in P144])


@functools.lru_cache(maxsize=None)
def reference(name):
    ids, _ = Q.golden(name)
    ref = Q.forward(name, ids, "ggml").astype(np.float32)
    ref.setflags(write=False)
    return ids, ref


# ---- 1. bf16 against the ggml-mode reference, every row regime --------------------------------------------------------
@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_bf16_logits_every_regime(mx, tmp, name):
    ids, ref = reference(name)
    shape, _ = Q.SHAPES[name]
    eng = open_engine(mx, Q.write_gguf(str(tmp / f"{name}.gguf"), name))
    try:
        assert (eng.info.n_head, eng.info.n_head_kv, eng.info.head_dim) == (shape.n_head, shape.n_head_kv, shape.head_dim)
        for regime in REGIMES:
            if name == "qwen-h3584" and regime.startswith("chunk"):
                continue
            rows, got = run_regime(eng, ids, regime)
            r = ref[rows]
            print(f"{name} {regime}: max |d| {np.abs(got - r).max():.4g} of max|ref| {np.abs(r).max():.4g}")
            assert_logits_close(got, r, f"{name} {regime}")
            assert_tokens_match(got, r, f"{name} {regime}")
    finally:
        eng.close()


# ---- 2. the NeoX twin is exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wtype", ["bf16", "q8_0", "q4_0_synth", "q4_k_m", "q5_k_m"])
def test_neox_twin_is_bitwise_the_llama_file(mx, tmp, wtype):
    """qwen-tiny's weights written qwen2 / NeoX row order / zero biases, and as a plain llama file: after the load-time
    permutation the packed weights are the same bytes, so the logits are the same bits in every regime."""
    shape, tied = Q.SHAPES["qwen-tiny"]
    ids, _ = Q.golden("qwen-tiny")
    a = Q.write_gguf(str(tmp / f"twin_qwen_{wtype}.gguf"), "qwen-tiny", wtype=wtype, qk_rows="neox", qkv_bias=0.0)
    b = Q.write_gguf(str(tmp / f"twin_llama_{wtype}.gguf"), "qwen-tiny", wtype=wtype, arch="llama", qkv_bias=None)
    out = []
    for path in (a, b):
        eng = open_engine(mx, path)
        try:
            out.append({r: run_regime(eng, ids[:8] if r == "one" else ids, r)[1] for r in ("one", "slots24", "prefill144")})
        finally:
            eng.close()
    for r in out[0]:
        assert not np.isnan(out[0][r]).any()
        assert np.array_equal(out[0][r], out[1][r]), f"{wtype} {r}: {(out[0][r] != out[1][r]).sum()} logits differ"


# ---- 3. the bias in each kernel family, exact ---------------------------------------------------------------------------
GEOM7 = (7, 1, 64)  # N = 576: 36 tiles
N7 = 576
PROBE_M = [1, 4, 5, 16, 17, 32, 64]
PROBE_CTX = 40


def probe_rows(M):
    i = np.arange(M)
    slot, pos = i % 3, (7 * (i // 3) + 3) % PROBE_CTX  # every row its own (slot, position); 3 slots x 40 positions
    if M >= 5:
        pos[2] = PROBE_CTX  # a row at n_ctx stores nothing
    return pos.astype(np.int32), slot.astype(np.int32)


def probe_cs(D, kind, n_ctx=PROBE_CTX):
    cs = np.zeros((n_ctx, D // 2, 2), np.float32)
    if kind == "id":
        cs[..., 0] = 1
    else:
        th = np.arange(n_ctx, dtype=np.float64)[:, None] * 1e6 ** (-2.0 * np.arange(D // 2) / D)[None, :]
        cs[..., 0], cs[..., 1] = np.cos(th), np.sin(th)
    return cs


def probe_qkv(M, geom, kind, bias):
    nh, nkv, D = geom
    pos, slot = probe_rows(M)
    elems = 3 * nkv * kv_layout.ctx_stride(PROBE_CTX) * D
    init = ((np.arange(elems, dtype=np.int64) * 37) % 2001 - 1000).astype(np.float16).view(np.uint16)
    return dict(n_head=nh, n_head_kv=nkv, head_dim=D, n_ctx=PROBE_CTX, n_slots=3, pos=pos, slot=slot,
                rope_cs=probe_cs(D, kind), kcache=init, vcache=init[::-1].copy(), bias=bias)


def bias_vec(N, seed=7):
    """Not dyadic on purpose: s + b rounds, so an add in another place (or after the f16 cast) shows."""
    return (np.random.default_rng(seed).standard_normal(N) * 0.3).astype(np.float32)


def rope_f32(x, cs):
    """rope4 (device_common.h) on x [M][heads][D] f32 with cs [M][D/2][2]: the inner product rounded to f32, the fma
    formed in float64 and rounded once more."""
    s0, s1 = x[..., 0::2], x[..., 1::2]
    c0, c1 = cs[:, None, :, 0], cs[:, None, :, 1]
    t0, t1 = (s1 * c1).astype(np.float32), (s1 * c0).astype(np.float32)
    o = np.empty_like(x)
    o[..., 0::2] = (s0.astype(np.float64) * c0 - t0).astype(np.float32)
    o[..., 1::2] = (s0.astype(np.float64) * c1 + t1).astype(np.float32)
    return o


def f16_ordinal(bits):
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def check_biased(r, qa, s, what, real_rope=False):
    """The probe's outputs against f32(s + b), s [M][N] the exact product (float64, exact in f32): q rows bitwise (real
    RoPE: through rope_f32, within one f32 ulp of double rounding -> compared at 2^-22 relative), K / V entries the f16
    of it (real RoPE: K within one f16 ulp), every other cache element unchanged, rows at n_ctx write nothing."""
    nh, nkv, D = qa["n_head"], qa["n_head_kv"], qa["head_dim"]
    pos, slot, b = qa["pos"], qa["slot"], qa["bias"]
    M, nq, nk = len(pos), nh * D, nkv * D
    stored = pos < PROBE_CTX
    sb = s.astype(np.float32) + (b[None, :] if b is not None else np.float32(0))  # one f32 add, as the device's
    assert sb.dtype == np.float32
    q, k, v = sb[:, :nq], sb[:, nq:nq + nk], sb[:, nq + nk:]
    if real_rope:
        cs = qa["rope_cs"][np.minimum(pos, PROBE_CTX - 1)]
        q = rope_f32(q.reshape(M, nh, D), cs).reshape(M, nq)
        k = rope_f32(k.reshape(M, nkv, D), cs).reshape(M, nk)
        assert np.allclose(r.out[stored], q[stored], rtol=2.0 ** -22, atol=2.0 ** -30), f"{what}: q"
    else:
        assert np.array_equal(r.out[stored], q[stored]), f"{what}: q != f32(sum + bias)"
    assert (np.ascontiguousarray(r.out[~stored]).view(np.uint8) == 0xFF).all(), f"{what}: q of a row at n_ctx written"
    S = kv_layout.ctx_stride(PROBE_CTX)
    K0, V0 = L.untile_caches(qa["kcache"], qa["vcache"], 3, nkv, S, D)
    K1, V1 = L.untile_caches(r.kcache, r.vcache, 3, nkv, S, D)
    K0, V0 = K0.copy(), V0.copy()
    for i in range(M):
        if not stored[i]:
            continue
        k16 = k[i].reshape(nkv, D).astype(np.float16).view(np.uint16)
        got = K1[slot[i], :, pos[i], :]
        if real_rope:
            d = np.abs(f16_ordinal(got) - f16_ordinal(k16)).max()
            assert d <= 1, f"{what}: stored K is {d} f16 ulp from f16(RoPE(sum + bias))"
            K0[slot[i], :, pos[i], :] = got
        else:
            K0[slot[i], :, pos[i], :] = k16
        V0[slot[i], :, pos[i], :] = v[i].reshape(nkv, D).astype(np.float16).view(np.uint16)
    assert np.array_equal(K1, K0), f"{what}: K cache (f16(sum + bias) at the rows' positions, nothing else)"
    assert np.array_equal(V1, V0), f"{what}: V cache"


def call_probe(mx, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except mx.MxError as e:
        if e.code == mx.MX_ERR_HIP:
            pytest.exit(f"HIP error, nothing more is launched: {e}", returncode=3)
        raise


def test_bias_bf16_kernels(mx):
    """launch_mm (path 0, K 448 as qwen-g7) and launch_mm_wide's slabs finished by qkv_finish_kernel (path 2, 17..64
    rows; K 2048: four slabs, and launch_mm_wide takes multiples of 128 only) on (7, 1, 64), and launch_mm_pers on
    Qwen2.5-3B's q|k|v shape (2560 x 2048: the prefetched bias) -- integer operands, so the sum is exact and the only
    rounding is the bias add."""
    import test_matmul_kernel_gpu as B

    b = bias_vec(N7)
    for path, K, Ms in ((0, 448, PROBE_M), (2, 2048, [M for M in PROBE_M if M > 16])):
        wb, xb, ref, e, _ = B.case(N7, K, 64)
        if path == 2:
            assert mx.matmul_plan(B.QKV, 17, N7, K)["kgroups"] == 4
        for M in Ms:
            s = ref[:M] * 2.0 ** -e
            for bias in (b, None):
                qa = probe_qkv(M, GEOM7, "id", bias)
                r = call_probe(mx, mx.matmul_probe, path, B.QKV, wb, xb[:M], qkv=qa)
                check_biased(r, qa, s, f"bf16 path {path} K={K} M={M} bias {'on' if bias is not None else 'off'}")
    qa = probe_qkv(5, GEOM7, "real", b)
    check_biased(call_probe(mx, mx.matmul_probe, 0, B.QKV, wb, xb[:5], qkv=qa), qa, ref[:5] * 2.0 ** -e,
                 "bf16 path 0 M=5 real RoPE", real_rope=True)
    N, K = 2560, 2048
    assert mx.matmul_plan(B.QKV, 1, N, K)["pers_ok"]
    wb, xb, ref, e, _ = B.case(N, K, 16)
    b = bias_vec(N, 8)
    for M in (1, 4):
        for bias in (b, None):
            qa = probe_qkv(M, (32, 4, 64), "id", bias)
            r = call_probe(mx, mx.matmul_probe, 1, B.QKV, wb, xb[:M], qkv=qa)
            check_biased(r, qa, ref[:M] * 2.0 ** -e, f"bf16 pers M={M} bias {'on' if bias is not None else 'off'}")


@pytest.mark.parametrize("q4", [False, True], ids=["q8_0", "q4_0"])
def test_bias_q8_kernels(mx, q4):
    """launch_mq8 (path 0) and launch_mq8_slab finished by launch_qkv_finish (path 1, where it takes the shape)."""
    import test_q8_kernel_gpu as T8

    K = 448
    blocks, xf, xi, e, s, unit = T8.case(N7, K, q4, 64)
    b = bias_vec(N7)
    for M in PROBE_M:
        paths = [0]
        if 16 < M <= 32 and mx.q8_matmul_plan(T8.QKV, M, N7, K, wq4=q4)["slab_ks"] > 0:
            paths.append(1)
        for path in paths:
            qa = probe_qkv(M, GEOM7, "id", b)
            r = call_probe(mx, mx.q8_matmul_probe, path, T8.QKV, blocks, xf[:M], wq4=q4, qkv=qa)
            check_biased(r, qa, s[:M], f"{'q4_0' if q4 else 'q8_0'} path {path} M={M}")
    qa = probe_qkv(5, GEOM7, "real", b)
    check_biased(call_probe(mx, mx.q8_matmul_probe, 0, T8.QKV, blocks, xf[:5], wq4=q4, qkv=qa), qa, s[:5],
                 "q8 path 0 M=5 real RoPE", real_rope=True)


def test_bias_kquant_kernels(mx):
    """launch_mkq (path 0), launch_mkq_qkv_slab finished by launch_qkv_finish (path 2, 17..32 rows) on Q4_K q|k + Q6_K v
    segments of (7, 1, 64), and mkq_pers_seg_kernel (K 4096, one token quantised on load: the prefetched bias)."""
    import test_kq_kernel_gpu as TK

    segs, K = ((12, 32), (14, 36)), 256
    blocks, fields, xf, xi, e, s, unit = TK.case(segs, K, 64)
    b = bias_vec(N7)
    for M in PROBE_M:
        paths = [0]
        if 16 < M <= 32 and mx.kq_matmul_plan(TK.QKV, M, N7, K, list(segs))["qkv_slab_ks"] > 0:
            paths.append(2)
        for path in paths:
            qa = probe_qkv(M, GEOM7, "id", b)
            r = call_probe(mx, mx.kq_matmul_probe, path, TK.QKV, blocks, xf[:M], list(segs), N=N7, K=K, qkv=qa)
            check_biased(r, qa, s[:M], f"kq path {path} M={M}")
    qa = probe_qkv(5, GEOM7, "real", b)
    check_biased(call_probe(mx, mx.kq_matmul_probe, 0, TK.QKV, blocks, xf[:5], list(segs), N=N7, K=K, qkv=qa), qa, s[:5],
                 "kq path 0 M=5 real RoPE", real_rope=True)
    segs = ((12, 12), (14, 16))
    assert mx.kq_matmul_plan(TK.QKV, 1, 256, 4096, list(segs), on_load=True, norm=True)["kind"] == "qkv_pers"
    blocks, fields, xf, xi, e, s, unit = TK.case(segs, 4096, 2)
    x1, w = TK.normed(xi[0], e[0])
    b = bias_vec(256, 9)
    for bias in (b, None):
        qa = probe_qkv(1, (2, 1, 64), "id", bias)
        r = call_probe(mx, mx.kq_matmul_probe, 0, TK.QKV, blocks, x1[None], list(segs), N=256, K=4096, act=2, norm_w=w,
                       qkv=qa)
        check_biased(r, qa, s[:1], f"kq qkv_pers bias {'on' if bias is not None else 'off'}")


@pytest.mark.parametrize("nslab", [4, 5])
@pytest.mark.parametrize("M", [17, 64])
def test_bias_attention_fin(mx, M, nslab):
    """attn_decode_kernel's FIN block: the bias joins the slab sum before RoPE, and the biased q / K / V are what the
    step attends with -- the launch with (slabs, bias) equals the launch with the bias folded into slab 0 where that
    fold is exact (dyadic values), in its output and in both caches, bit for bit; and the stores are f16(sum + b)."""
    import test_attention_kernel_gpu as T

    D, G = 64, 7
    plan = next(p for p in T.PLANS if p.mode == 1 and len(p.rows) == M and p.nslab == nslab)
    c = T.peak_case(plan, D, G, 99)  # dyadic q / knew / vnew, identity RoPE, slabs that sum exactly
    N = (c.H + 2 * T.NKV) * D
    b = (np.random.default_rng(3).integers(-64, 65, N) / 16.0).astype(np.float32)  # dyadic: sum + b is exact
    kc, vc = c.tiled()
    slot, pos = [r[0] for r in c.rows], [r[1] for r in c.rows]
    folded = c.slabs.copy()
    folded[0] = c.slabs[0] + b[None, :]
    tot = T.slab_sum(c.slabs)
    assert np.array_equal(T.slab_sum(folded), tot + b[None, :]) and \
        np.array_equal((tot.astype(np.float64) + b[None, :]).astype(np.float32), tot + b[None, :]), "the fold is exact"
    args = (1, c.H, T.NKV, D, c.n_ctx, c.n_slots, pos, slot, kc, vc)
    got = call_probe(mx, mx.attention_probe, *args, slabs=c.slabs, rope_cs=c.cs, bias=b)
    want = call_probe(mx, mx.attention_probe, *args, slabs=folded, rope_cs=c.cs)
    plain = call_probe(mx, mx.attention_probe, *args, slabs=c.slabs, rope_cs=c.cs)
    assert not np.isnan(got[0]).any()
    for g, w, what in zip(got, want, ("out", "K cache", "V cache")):
        assert np.array_equal(g, w), f"M={M} nslab={nslab}: {what} with a bias != the bias folded into the slabs"
    assert not np.array_equal(got[0], plain[0]) and not np.array_equal(got[1], plain[1])
    ka = kv_layout.untile_k(got[1].reshape(c.n_slots, T.NKV, -1), D)
    va = kv_layout.untile_v(got[2].reshape(c.n_slots, T.NKV, -1), D)
    nq, nkv = c.H * D, T.NKV * D
    sb = tot + b[None, :]
    for i, (s_, p_) in enumerate(c.rows):
        if p_ >= c.n_ctx:
            continue
        assert np.array_equal(ka[s_, :, p_], sb[i, nq:nq + nkv].reshape(T.NKV, D).astype(np.float16).view(np.uint16))
        assert np.array_equal(va[s_, :, p_], sb[i, nq + nkv:].reshape(T.NKV, D).astype(np.float16).view(np.uint16))


def test_bias_attention_fin_real_rope(mx):
    """Family (d)'s bound with a bias and the real RoPE table: V == f16(slab sum + b) bitwise, K within one f16 ulp of
    f16(RoPE(slab sum + b)), every other cache element unchanged."""
    import test_attention_kernel_gpu as T

    D, G = 128, 7
    plan = next(p for p in T.PLANS if p.mode == 1 and len(p.rows) == 33 and p.nslab == 5)
    c = T.random_case(plan, D, G, 77)
    N = (c.H + 2 * T.NKV) * D
    nq, nkv = c.H * D, T.NKV * D
    b = bias_vec(N, 11)
    tot = T.slab_sum(c.slabs) + b[None, :]
    c.vnew = tot[:, nq + nkv:].reshape(c.M, T.NKV, D).copy()
    for i, (_, pos) in enumerate(c.rows):
        if pos < c.n_ctx:
            c.knew[i] = T.rope_f32(tot[i, nq:nq + nkv].reshape(T.NKV, D), c.cs[pos])
    kc, vc = c.tiled()
    out, ka, va = call_probe(mx, mx.attention_probe, 1, c.H, T.NKV, D, c.n_ctx, c.n_slots, [r[1] for r in c.rows],
                             [r[0] for r in c.rows], kc, vc, slabs=c.slabs, rope_cs=c.cs, bias=b)
    assert not np.isnan(out).any()
    T.check_fin_stores(c, kv_layout.untile_k(ka.reshape(c.n_slots, T.NKV, -1), D),
                       kv_layout.untile_v(va.reshape(c.n_slots, T.NKV, -1), D))


# ---- 4. the attention kernels at the new groups ---------------------------------------------------------------------------
NEW_GEOMS = [(D, G) for D in (64, 128) for G in (5, 6, 7)]


@pytest.mark.parametrize("D,G", NEW_GEOMS, ids=[f"D{D}-G{G}" for D, G in NEW_GEOMS])
def test_attention_kernels_new_groups(mx, D, G):
    """Families (a) coverage-exact, (c) random vs float64, (d) FIN stores and (e) batch invariance of
    tests/test_attention_kernel_gpu.py, its plans and bounds unchanged, at G = 5, 6, 7."""
    import test_attention_kernel_gpu as T

    seed = 100 * D + G
    for pi, plan in enumerate(T.PLANS):
        c = T.cover_case(plan, D, G, 1000 * seed + pi)
        for out_f32 in (True, False):
            T.check_cover(c, c.launch(mx, out_f32)[0], out_f32)
        c = T.random_case(plan, D, G, 3000 * seed + pi)
        outs = {}
        for out_f32 in (True, False):
            outs[out_f32], ka, va = c.launch(mx, out_f32)
        T.check_random(c, outs)
        if plan.mode == 1:
            T.check_fin_stores(c, ka, va)
    for out_f32 in (True, False):
        c = T.random_case(T.PLANS[0], D, G, 4000 + seed)
        full, _, _ = c.launch(mx, out_f32)
        for i in (0, 5, 9, 12, 15):
            assert c.launch(mx, out_f32, idx=[i])[0][0].tobytes() == full[i].tobytes(), f"D={D} G={G}: row {i} alone"
        for ns in (4, 8):
            plan = next(p for p in T.PLANS if p.mode == 1 and len(p.rows) == 64 and p.nslab == ns)
            c = T.random_case(plan, D, G, 5000 + seed)
            full, _, _ = c.launch(mx, out_f32)
            part, _, _ = c.launch(mx, out_f32, idx=list(range(17)))
            assert part.tobytes() == full[:17].tobytes(), f"mode 1 D={D} G={G} nslab {ns}: rows at M=17 != at M=64"


# ---- 5. quantised models with a bias, whole model -------------------------------------------------------------------------
QUANT_REGIMES = ("one", "slots24", "prefill144")


def quant_vs_own_bf16(mx, tmp, tag, wtype, **kw):
    """Worst |logit - logit of the same file dequantised to BF16| / max|that| over the three regimes."""
    ids, _ = Q.golden("qwen-g7-d128")
    pq = Q.write_gguf(str(tmp / f"{tag}_{wtype}.gguf"), "qwen-g7-d128", wtype=wtype, **kw)
    pb = Q.write_gguf(str(tmp / f"{tag}_{wtype}_bf16.gguf"), "qwen-g7-d128", dequant_from=pq, **kw)
    res = []
    for path in (pq, pb):
        eng = open_engine(mx, path)
        try:
            res.append([run_regime(eng, ids[:12] if r == "one" else ids, r)[1] for r in QUANT_REGIMES])
        finally:
            eng.close()
    worst = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(*res))
    assert all(not np.isnan(a).any() for a in res[0])
    return worst


@pytest.mark.parametrize("wtype", ["q8_0", "q4_k_m"])
def test_quantised_model_with_bias(mx, tmp, wtype):
    """qwen-g7-d128 quantised, against this engine on the same file rewritten as BF16.  The bar is twice what the llama
    twin of the shape (zero bias, arch llama: existing code on both sides) shows in the same comparison: the bias adds
    one f32 add per element but shifts the ranges that Q8_0 / Q8_K quantise.  A dropped bias is off by the whole logit
    scale.  The measured values are in DESIGN.md §18."""
    twin = quant_vs_own_bf16(mx, tmp, "twin", wtype, arch="llama", qkv_bias=None)
    qwen = quant_vs_own_bf16(mx, tmp, "qwen", wtype)
    print(f"qwen-g7-d128 {wtype}: quantised vs its own BF16, worst |d| / max|ref|: llama twin {twin:.4g}, qwen2 {qwen:.4g}")
    assert twin > 0
    assert qwen <= 2 * twin, f"{wtype}: qwen2 {qwen:.4g} > 2 x llama twin {twin:.4g}"


# ---- 6. the front ----------------------------------------------------------------------------------------------------------
def test_llama_front_on_a_qwen2_file(mx, tmp):
    from llama_p2p_amd.llama import Llama

    path = Q.write_gguf(str(tmp / "front.gguf"), "qwen-tiny")
    ids = [int(t) for t in Q.golden("qwen-tiny")[0][:12]]
    llm = Llama(path, n_ctx=N_CTX, n_seq_max=4, device=0, verbose=False)
    try:
        assert llm.metadata["general.architecture"] == "qwen2"
        out = llm.create_completion(ids, max_tokens=8, temperature=0.0)
        text = out["choices"][0]["text"]
    finally:
        llm.close()
    eng = open_engine(mx, path)
    try:
        toks, _ = eng.generate(ids, 8, temperature=0.0)
    finally:
        eng.close()
    assert out["usage"]["completion_tokens"] == len(toks)
    assert text == llm.tokenizer_.detokenize(toks, prev_tokens=ids).decode("utf-8", errors="ignore")
    shape, _ = Q.SHAPES["qwen-tiny"]
    rng = np.random.default_rng(5)
    pair = {"blk.0.attn_q.weight": (rng.integers(-4, 5, (2, shape.n_embd)) / 64.0, rng.integers(-4, 5, (shape.n_embd, 2)) / 64.0)}
    good = gguf.write_lora_gguf(str(tmp / "lora_qwen2.gguf"), pair, 0.0, arch="qwen2")
    bad = gguf.write_lora_gguf(str(tmp / "lora_llama.gguf"), pair, 0.0, arch="llama")
    llm = Llama(path, n_ctx=N_CTX, n_seq_max=4, device=0, verbose=False, lora_path=good)
    try:
        assert llm._engine.lora_info()["n_tensors"] == 1
        assert llm.create_completion(ids, max_tokens=4, temperature=0.0)["usage"]["completion_tokens"] >= 1
    finally:
        llm.close()
    with pytest.raises(RuntimeError):
        Llama(path, n_ctx=N_CTX, n_seq_max=4, device=0, verbose=False, lora_path=bad)
    with pytest.raises(mx.MxError) as ei:
        mx.Engine(path, n_ctx=N_CTX, n_seq_max=4, device=0, lora_path=bad)
    assert ei.value.code == mx.MX_ERR_MODEL and "general.architecture" in str(ei.value)


def test_lora_on_qwen2_is_merged_before_the_permutation(mx, tmp):
    """dequantise -> merge -> permute -> pack: the adapter's B rows are in file order, so Engine(lora_path=) on the
    qwen2 file gives the bits of the file written already merged."""
    shape, _ = Q.SHAPES["qwen-tiny"]
    ids = Q.golden("qwen-tiny")[0]
    rng = np.random.default_rng(6)
    pairs = {f"blk.{l}.attn_{k}.weight": (rng.integers(-4, 5, (3, shape.n_embd)) / 64.0,
                                          rng.integers(-4, 5, (n, 3)) / 64.0)
             for l in range(2) for k, n in (("q", shape.n_embd), ("k", shape.n_embd_kv))}
    ad = gguf.write_lora_gguf(str(tmp / "lora_qk.gguf"), pairs, 0.0, arch="qwen2")
    base = Q.write_gguf(str(tmp / "lora_base.gguf"), "qwen-tiny")
    merged = Q.write_gguf(str(tmp / "lora_merged.gguf"), "qwen-tiny", merge_lora=(ad, 1.0))
    out = []
    for path, kw in ((base, dict(lora_path=ad)), (merged, {}), (base, {})):
        eng = open_engine(mx, path, **kw)
        try:
            out.append(run_regime(eng, ids, "chunk16")[1])
        finally:
            eng.close()
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[0], out[2])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def edited_gguf(monkeypatch, path, edit, **kw):
    """Q.write_gguf of qwen-tiny with the tensor list passed through edit(name, ne, type, array) -> the same, or None."""

    class Edited(gguf.GGUFWriter):
        def write(self, data_iter):
            infos, arrays = [], []
            for (name, ne, t, _), arr in zip(self.tensors, data_iter):
                res = edit(name, ne, t, np.asarray(arr))
                if res is not None:
                    name, ne, t, arr = res
                    infos.append((name, tuple(ne), t, gguf.type_nbytes(t, int(np.prod(ne)))))
                    arrays.append(arr)
            self.tensors = infos
            super().write(arrays)

    monkeypatch.setattr(gguf, "GGUFWriter", Edited)
    try:
        return Q.write_gguf(path, "qwen-tiny", **kw)
    finally:
        monkeypatch.undo()


def test_refusals(mx, tmp, monkeypatch):
    def only_q(name, ne, t, a):
        return None if name.endswith(("attn_k.bias", "attn_v.bias")) else (name, ne, t, a)

    def short_q(name, ne, t, a):
        return (name, (ne[0] - 1,), t, a[:-1]) if name == "blk.1.attn_q.bias" else (name, ne, t, a)

    def f16_k(name, ne, t, a):
        return (name, ne, gguf.GGML_F16, a.astype(np.float16)) if name == "blk.0.attn_k.bias" else (name, ne, t, a)

    cases = {"only attn_q.bias": (only_q, {}, "come together"), "a bias of length h - 1": (short_q, {}, "elements"),
             "an F16 bias": (f16_k, {}, "F32"),
             "architecture gemma": (lambda *a: a, dict(arch="gemma"), "'llama' or 'qwen2'"),
             "a subset under llama": (only_q, dict(arch="llama"), "come together")}
    for what, (edit, kw, msg) in cases.items():
        path = edited_gguf(monkeypatch, str(tmp / f"bad_{len(what)}_{kw.get('arch', 'q')}.gguf"), edit, **kw)
        with pytest.raises(mx.MxError) as ei:
            mx.Engine(path, n_ctx=N_CTX, n_seq_max=2, device=0)
        assert ei.value.code == mx.MX_ERR_MODEL and msg in str(ei.value), f"{what}: {ei.value}"
    # the same checks hold for a stage engine's layer range: the bad bias is in layer 1 only
    path = edited_gguf(monkeypatch, str(tmp / "bad_stage.gguf"), short_q)
    eng = mx.Engine(path, n_ctx=N_CTX, n_seq_max=2, device=0, layer_begin=0, layer_end=1)
    eng.close()
    with pytest.raises(mx.MxError) as ei:
        mx.Engine(path, n_ctx=N_CTX, n_seq_max=2, device=0, layer_begin=1, layer_end=2)
    assert ei.value.code == mx.MX_ERR_MODEL
    g3 = synth.LlamaShape("g3", 384, 1, 6, 2, 512, 512, 1e6, 1e-6)
    p3 = gguf.write_synthetic_gguf(str(tmp / "g3.gguf"), g3, arch="qwen2", qkv_bias=0.3)
    with pytest.raises(mx.MxError) as ei:
        mx.Engine(p3, n_ctx=N_CTX, n_seq_max=2, device=0)
    assert ei.value.code == mx.MX_ERR_ARG, "G = 3 stays refused"


# ---- 8. llama + biases -----------------------------------------------------------------------------------------------------
def test_llama_architecture_with_biases(mx, tmp):
    """llama.cpp reads optional attn_*.bias for architecture llama too.  qwen-tiny's weights written arch="llama" with
    the rows as they are ("norm": no permutation at load) and the biases in the same order: the model of the reference
    with unpermuted rows."""
    ids, _ = Q.golden("qwen-tiny")
    ref = Q.forward("qwen-tiny", ids, "ggml", t=Q.weights("qwen-tiny", permute=False)).astype(np.float32)
    eng = open_engine(mx, Q.write_gguf(str(tmp / "llama_bias.gguf"), "qwen-tiny", arch="llama"))
    try:
        for regime in REGIMES:
            rows, got = run_regime(eng, ids, regime)
            assert_logits_close(got, ref[rows], f"llama + biases {regime}")
            assert_tokens_match(got, ref[rows], f"llama + biases {regime}")
    finally:
        eng.close()
