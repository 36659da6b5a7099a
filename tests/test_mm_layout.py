"""tests/mm_layout.py against hand-computed cases, and the matmul dispatch facts (mx_matmul_plan) -- no GPU.

The expected plan values are written down from wide_split / mm_pers_supported / mm_can_norm_on_load /
gemm_supported as they stand: a retune of any of them has to touch this file, and the GPU tests of
tests/test_matmul_kernel_gpu.py choose their shapes from the same facts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kv_layout
import mm_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, RESID, QKV, SWIGLU = 0, 1, 2, 3


# ---- layout -------------------------------------------------------------------------------------------------
def test_pack_places_elements_by_the_layout_sentence():
    N, K = 48, 96
    W = (np.arange(N)[:, None] * 1000 + np.arange(K)[None, :]).astype(np.int64)  # entry encodes (row, col)
    flat = L.pack_tiles(W)
    KT = K // 32
    for nt, kt, lane, j in [(0, 0, 0, 0), (0, 0, 15, 7), (0, 0, 16, 0), (0, 0, 63, 7), (1, 2, 37, 5), (2, 1, 48, 3)]:
        want = W[16 * nt + (lane & 15), 32 * kt + 8 * (lane >> 4) + j]
        assert flat[(nt * KT + kt) * 512 + lane * 8 + j] == want
    # tile (0, 1) follows tile (0, 0): nt-major, 512 elements (1 KiB of bf16) apart
    assert flat[512] == W[0, 32] and flat[3 * 512] == W[16, 0]


@pytest.mark.parametrize("N,K", [(16, 32), (48, 96), (160, 2080)])
def test_pack_round_trip(N, K):
    W = np.random.default_rng(N + K).integers(0, 1 << 16, size=(N, K)).astype(np.uint16)
    flat = L.pack_tiles(W)
    assert flat.shape == (N * K,) and sorted(flat.tolist()) == sorted(W.reshape(-1).tolist())
    assert np.array_equal(L.unpack_tiles(flat, N, K), W)


def test_gate_up_interleave():
    F, K = 24, 32
    gate = (np.arange(F)[:, None] * 100 + np.arange(K)[None, :]).astype(np.int64)  # (row, col)
    up = -gate - 1
    m = L.interleave_gate_up(gate, up)
    assert m.shape == (2 * F, K)
    for t in range(F // 8):
        assert np.array_equal(m[16 * t:16 * t + 8], gate[8 * t:8 * t + 8])
        assert np.array_equal(m[16 * t + 8:16 * t + 16], up[8 * t:8 * t + 8])
    # logical [gate; up] -> tiles: lane l < 8 of tile t, k group 0 = gate row 8t + l; lanes 8..15 = up row 8t + l - 8
    flat = L.pack_swiglu(np.concatenate([gate, up]))
    assert flat[1 * 512 + 3 * 8 + 2] == gate[8 + 3, 2]
    assert flat[1 * 512 + 11 * 8 + 2] == up[8 + 3, 2]
    assert flat[2 * 512 + (8 + 16) * 8 + 5] == up[16, 8 + 5]


# ---- bf16 helpers -------------------------------------------------------------------------------------------
def test_bf16_rounding():
    assert L.bf16_bits(np.float32(1.0)) == 0x3F80 and L.bf16_bits(np.float32(-2.5)) == 0xC020
    # 1 + 2^-8 is a tie: to even (1.0); 1 + 3 * 2^-8 is a tie: to even (1 + 2^-6)
    assert L.bf16_bits(np.float32(1 + 2.0 ** -8)) == 0x3F80
    assert L.bf16_bits(np.float32(1 + 3 * 2.0 ** -8)) == 0x3F82
    assert L.bf16_bits(np.float32(1 + 2.0 ** -8 + 2.0 ** -20)) == 0x3F81
    assert L.bf16_f32(np.uint16(0x3F81)) == np.float32(1 + 2.0 ** -7)
    with pytest.raises(AssertionError):
        L.bf16_bits(np.float32(1 + 2.0 ** -8), exact=True)
    assert L.bf16_ulp(1.0) == 2.0 ** -7 and L.bf16_ulp(3.9) == 2.0 ** -6 and L.bf16_ulp(-0.5) == 2.0 ** -8


# ---- references ---------------------------------------------------------------------------------------------
def test_int_matmul_by_hand():
    W = np.array([[1, 2, 3], [0, -1, 4]])
    X = np.array([[1, 1, 1], [2, 0, -1]])
    assert np.array_equal(L.int_matmul(W, X), [[6, 3], [-1, -4]])
    with pytest.raises(AssertionError):  # the exactness bound is checked, not assumed
        L.int_matmul(np.full((1, 1 << 16), 16), np.full((1, 1 << 16), 16))
    rng = np.random.default_rng(0)
    W, X = rng.integers(-4, 5, size=(40, 4096)), rng.integers(-4, 5, size=(3, 4096))
    assert np.array_equal(L.int_matmul(W, X), X.astype(np.int64) @ W.astype(np.int64).T)


def test_swiglu_by_hand():
    assert L.swiglu_ref(0.0, 5.0) == 0.0
    assert abs(L.swiglu_ref(1.0, 2.0) - 2.0 / (1.0 + np.exp(-1.0))) < 1e-15
    assert abs(L.swiglu_ref(-1.0, 3.0) + 3.0 / (1.0 + np.e)) < 1e-15


def test_rope_and_qkv_split_by_hand():
    D = 4
    cs = np.zeros((3, D // 2, 2))
    cs[0] = [[1, 0], [1, 0]]          # identity
    cs[1] = [[0, 1], [0, 1]]          # quarter turn: (s0, s1) -> (-s1, s0)
    cs[2] = [[0.6, 0.8], [1, 0]]      # pair 0 turned, pair 1 not
    s = np.array([[1., 2., 3., 4.]] * 3)
    o = L.rope_ref(s, D, [0, 1, 2], cs)
    assert np.array_equal(o[0], [1, 2, 3, 4])
    assert np.array_equal(o[1], [-2, 1, -4, 3])
    assert np.allclose(o[2], [1 * 0.6 - 2 * 0.8, 1 * 0.8 + 2 * 0.6, 3, 4], atol=1e-15)
    # 2 q heads, 1 kv head: rows [0, 8) q, [8, 12) k, [12, 16) v (no RoPE)
    row = np.arange(1.0, 17.0)[None, :]
    q, k, v = L.qkv_ref(row, 2, 1, D, [1], cs)
    assert np.array_equal(q[0], [-2, 1, -4, 3, -6, 5, -8, 7])
    assert np.array_equal(k[0], [-10, 9, -12, 11])
    assert np.array_equal(v[0], [13, 14, 15, 16])


def test_untile_caches_uses_kv_layout():
    D, S = 64, 64
    K = np.arange(2 * 1 * S * D, dtype=np.uint16).reshape(2, 1, S, D)
    V = K[::-1].copy()
    k2, v2 = L.untile_caches(kv_layout.tile_k(K).reshape(-1), kv_layout.tile_v(V).reshape(-1), 2, 1, S, D)
    assert np.array_equal(k2, K) and np.array_equal(v2, V)


def test_rmsnorm_and_ssq_by_hand():
    x = np.array([[3.0, 4.0] + [0.0] * 14])
    assert np.array_equal(L.ssq16_ref(x), [[25.0]])
    w = np.full(16, 2.0)
    y = L.rmsnorm_ref(x, w, 0.0)  # mean square 25/16 -> scale 4/5
    assert np.allclose(y[0, :2], [3 * 0.8 * 2, 4 * 0.8 * 2], atol=1e-15) and not y[0, 2:].any()
    x32 = np.arange(32.0)[None, :]
    assert np.array_equal(L.ssq16_ref(x32), [[sum(i * i for i in range(16)), sum(i * i for i in range(16, 32))]])


# ---- the binding and the dispatch facts -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def E():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def test_probes_are_exported(E):
    for name in ("mx_matmul_probe", "mx_matmul_plan", "mx_norm_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)


@pytest.mark.parametrize("epi,N,K,want", [
    (QKV, 6144, 4096, 4),      # Llama-3-8B q|k|v: cfg 3 (tiles % 3), target 4
    (QKV, 12288, 4096, 4),     # Llama-2-7B q|k|v: cfg 3
    (QKV, 2560, 2048, 4),      # TinyLlama: cfg 0
    (QKV, 10240, 8192, 4),     # Llama-3-70B: cfg 0
    (RESID, 4096, 4096, 4),    # attn_output: cfg 1
    (RESID, 4096, 14336, 8),   # ffn_down: cfg 4, the only 8-way split
    (RESID, 4096, 11008, 8),   # Llama-2-7B ffn_down: cfg 4, 43-tile K ranges (RG form)
    (RESID, 2048, 5632, 4),
    (RESID, 8192, 28672, 8),
    (RESID, 64, 128, 1),       # KT = 4: one range
    (RESID, 64, 1024, 2),      # KT = 32: 2 ranges of 16 tiles
    (RESID, 64, 2048, 4),
    (RESID, 64, 2176, 4),      # 17-tile ranges (RG)
    (RESID, 128, 8320, 8),     # cfg 4, 32.5-tile ranges (RG)
    (RESID, 64, 8320, 4),      # cfg 2 (K > 8192, tiles % 8 != 0)
    (RESID, 64, 96, 1),        # K % 128 != 0: no wide form, one group
    (QKV, 192, 1024, 2),
    (F32, 128256, 4096, 1),    # lm_head and gate/up never split K
    (SWIGLU, 28672, 4096, 1),
])
def test_canon_kgroups(E, epi, N, K, want):
    assert E.matmul_plan(epi, 1, N, K)["kgroups"] == want


def test_pers_supported_for_the_four_model_families(E):
    ok = lambda epi, M, N, K: E.matmul_plan(epi, M, N, K)["pers_ok"]
    yes = [
        (SWIGLU, 28672, 4096), (RESID, 4096, 4096), (RESID, 4096, 14336), (QKV, 6144, 4096),   # Llama-3-8B
        (SWIGLU, 11264, 2048), (RESID, 2048, 2048), (RESID, 2048, 5632), (QKV, 2560, 2048),   # TinyLlama
        (SWIGLU, 57344, 8192), (QKV, 10240, 8192),                                             # Llama-3-70B
        (SWIGLU, 22016, 4096), (QKV, 12288, 4096),                                             # Llama-2-7B
        (SWIGLU, 16 * 1025, 4096), (SWIGLU, 16 * 1537, 4096),                                  # the 1025..1792 range
    ]
    no = [
        (RESID, 8192, 8192), (RESID, 8192, 28672), (RESID, 4096, 11008), (F32, 128256, 4096),
        (SWIGLU, 16 * 1024, 4096), (SWIGLU, 16 * 1793, 4096), (QKV, 6144, 2048), (SWIGLU, 11264, 4096),
    ]
    for epi, N, K in yes:
        assert ok(epi, 1, N, K) and ok(epi, 16, N, K) and not ok(epi, 17, N, K), (epi, N, K)
    for epi, N, K in no:
        assert not ok(epi, 1, N, K), (epi, N, K)


def test_norm_on_load_and_gemm_facts(E):
    nol = lambda M, K: E.matmul_plan(F32, M, 64, K)["norm_on_load_ok"]
    assert nol(1, 512) and nol(4, 4096) and nol(4, 8192) and nol(1, 2048)
    assert not nol(5, 4096) and not nol(1, 16384) and not nol(1, 96) and not nol(1, 2080)
    gemm = lambda N, K: E.matmul_plan(F32, 100, N, K)["gemm_ok"]
    assert gemm(256, 64) and gemm(768, 2048)
    assert not gemm(128, 64) and not gemm(256, 32) and not gemm(384, 64)


def test_plan_refuses_bad_shapes(E):
    for args in [(4, 1, 64, 64), (-1, 1, 64, 64), (0, 0, 64, 64), (0, 1, 24, 64), (0, 1, 64, 48), (0, 1, 0, 64)]:
        with pytest.raises(E.MxError) as ei:
            E.matmul_plan(*args)
        assert ei.value.code == E.MX_ERR_ARG


def test_split_override_is_capped_at_the_slab_count():
    """MX_WIDE_QKV_SPLIT / MX_WIDE_RESID_SPLIT = 16 (read once per process, so a child): the engine's slab buffer
    and the attention's FIN path hold 8 partials, and the split applied must not exceed that."""
    code = ("from llama_p2p_amd import engine as E\n"
            "print(E.matmul_plan(1, 1, 4096, 14336)['kgroups'], E.matmul_plan(2, 1, 6144, 8192)['kgroups'],\n"
            "      E.matmul_plan(1, 1, 8192, 8192)['kgroups'], E.matmul_plan(2, 1, 6144, 1024)['kgroups'])\n")
    env = dict(os.environ, MX_WIDE_QKV_SPLIT="16", MX_WIDE_RESID_SPLIT="16")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # K tiles 448 / 256 / 256 would all allow 16 ranges of >= 16 tiles; K 1024 (32 tiles) allows 2
    assert r.stdout.split() == ["8", "8", "8", "2"]
