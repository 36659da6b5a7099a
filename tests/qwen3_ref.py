"""Qwen3 test models (no GPU needed to import): the shapes, their GGUF files, and a NumPy float64 forward in the
engine's form, built from tests/qwen2_ref.py's pieces -- no q/k/v bias, and an RMS_NORM over each head of q and of k
with a learned [head_dim] weight between the projection and RoPE.  attn_q / attn_k rows and the two
norm weights are permuted inside each head as the loader permutes them, so RoPE rotates adjacent pairs.

Modes as qwen2_ref: "exact" (float64 throughout; must reproduce transformers' Qwen3ForCausalLM, tests/golden/
hf_qwen3-*.npz) and "ggml" (the oracle's rounding points; the head norm itself is f32 arithmetic on f32 sums in
ggml, so it adds no rounding point of its own at this precision).
"""
import os

import numpy as np

from llama_p2p_amd import synth
from llama_p2p_amd.synth import LlamaShape
from qwen2_ref import GOLDEN, permute_rows, rbf16, rf16, rope_adjacent

SEED = 0

# name: (shape, tied embeddings); two layers each, rope_base 1e6 and eps 1e-6 as Qwen3
SHAPES = {
    "q3-tiny": (LlamaShape("q3-tiny", 256, 2, 4, 2, 512, 512, 1e6, 1e-6), True),           # d 64, G 2
    "q3-g4-d128": (LlamaShape("q3-g4-d128", 1024, 2, 8, 2, 1024, 512, 1e6, 1e-6), False),  # multiples of 256: quantised
    "q3-g5": (LlamaShape("q3-g5", 640, 2, 5, 1, 512, 512, 1e6, 1e-6), False),              # d 128, G 5 (14B)
    "q3-mha": (LlamaShape("q3-mha", 256, 2, 4, 4, 512, 512, 1e6, 1e-6), False),            # d 64, G 1: 4-wave attention
}
# Shapes without a transformers golden: the reference for them is forward(..., "ggml") (checked against transformers
# on the four shapes above), the ids come from seeded_ids.  q3-g7: Qwen2's qwen-g7 geometry, a width that is no multiple
# of 128 (no launch_mm_wide, no prefill GEMM: 17..64-row forwards take launch_mm's raw q|k|v epilogue).
EXTRA_SHAPES = {
    "q3-g7": (LlamaShape("q3-g7", 448, 2, 7, 1, 512, 512, 1e6, 1e-6), False),              # d 64, G 7
}


def shape_of(name):
    return SHAPES[name] if name in SHAPES else EXTRA_SHAPES[name]


def seeded_ids(name, T=40):
    shape, _ = shape_of(name)
    rng = np.random.default_rng([SEED, len(name), T])
    return np.concatenate([[1], rng.integers(3, shape.n_vocab, T - 1)]).astype(np.int32)


def golden(name):
    g = np.load(os.path.join(GOLDEN, f"hf_qwen3-{name}.npz"))
    return g["ids"].astype(np.int32), g["logits"].astype(np.float32)


def qk_norm(name, seed=SEED, ones=False):
    """{(layer, "q" | "k"): f32 [head_dim]} in file order: log-normal around 1 (0.3 .. 3), or all ones."""
    shape, _ = shape_of(name)
    out = {}
    for l in range(shape.n_layer):
        for j, k in enumerate("qk"):
            w = np.exp(0.5 * np.random.default_rng([seed, l, j]).standard_normal(shape.head_dim))
            out[(l, k)] = np.ones(shape.head_dim, np.float32) if ones else w.astype(np.float32)
    return out


def write_gguf(path, name, wtype="bf16", ones=False, **kw):
    from llama_p2p_amd import gguf

    shape, tied = shape_of(name)
    kw.setdefault("arch", "qwen3")
    kw.setdefault("tie_embeddings", tied)
    kw.setdefault("qk_norm", qk_norm(name, ones=ones))
    return gguf.write_synthetic_gguf(path, shape, seed=SEED, wtype=wtype, **kw)


def weights(name, seed=SEED, permute=True, ones=False):
    """{gguf name: float64 array}: the synthetic bf16 weights and the head-norm weights; attn_q / attn_k rows and the
    norm weights in the engine's order when `permute`."""
    shape, tied = shape_of(name)
    t = {}
    for nm, kind, arr in synth.synth_tensors(shape, seed):
        t[nm] = (synth.bf16_bits_to_f32(arr) if kind == "bf16" else arr).astype(np.float64)
    for (l, k), w in qk_norm(name, seed, ones).items():
        t[f"blk.{l}.attn_{k}_norm.weight"] = w.astype(np.float64)
    if tied:
        t["output.weight"] = t["token_embd.weight"]
    if permute:
        for l in range(shape.n_layer):
            for k, nh in (("q", shape.n_head), ("k", shape.n_head_kv)):
                t[f"blk.{l}.attn_{k}.weight"] = permute_rows(t[f"blk.{l}.attn_{k}.weight"], nh)
                t[f"blk.{l}.attn_{k}_norm.weight"] = permute_rows(t[f"blk.{l}.attn_{k}_norm.weight"], 1)
    return t


def head_norm(x, w, eps):
    """x [T][heads][d], w [d]: RMS_NORM over d, then MUL."""
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def forward(name, ids, mode="exact", t=None):
    """Logits [T][n_vocab] (float64) of `ids` at positions 0..T-1, every position attending to its prefix."""
    assert mode in ("exact", "ggml")
    shape, _ = shape_of(name)
    t = t or weights(name)
    act = rbf16 if mode == "ggml" else (lambda v: v)
    half = rf16 if mode == "ggml" else (lambda v: v)
    H, KV, d, G = shape.n_head, shape.n_head_kv, shape.head_dim, shape.n_head // shape.n_head_kv
    ids = np.asarray(ids)
    T = len(ids)
    pos = np.arange(T)

    def norm(x, w):
        return x / np.sqrt((x * x).mean(-1, keepdims=True) + shape.eps) * w

    x = t["token_embd.weight"][ids]
    mask = np.tril(np.ones((T, T), bool))
    for l in range(shape.n_layer):
        p = f"blk.{l}."
        xn = act(norm(x, t[p + "attn_norm.weight"]))
        q, k, v = (xn @ t[p + f"attn_{c}.weight"].T for c in "qkv")
        q = head_norm(q.reshape(T, H, d), t[p + "attn_q_norm.weight"], shape.eps)
        k = head_norm(k.reshape(T, KV, d), t[p + "attn_k_norm.weight"], shape.eps)
        q, k = half(rope_adjacent(q, pos, shape.rope_base)), half(rope_adjacent(k, pos, shape.rope_base))
        v = half(v.reshape(T, KV, d))
        k, v = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
        s = np.einsum("thd,shd->hts", q, k) / np.sqrt(d)
        s = np.where(mask[None], s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        o = np.einsum("hts,shd->thd", half(e), v) / e.sum(-1).T[:, :, None]  # P as f16, the sum from the f32 values
        x = x + act(o.reshape(T, H * d)) @ t[p + "attn_output.weight"].T
        xn = act(norm(x, t[p + "ffn_norm.weight"]))
        g, u = xn @ t[p + "ffn_gate.weight"].T, xn @ t[p + "ffn_up.weight"].T
        x = x + act(g / (1.0 + np.exp(-g)) * u) @ t[p + "ffn_down.weight"].T
    return act(norm(x, t["output_norm.weight"])) @ t["output.weight"].T
