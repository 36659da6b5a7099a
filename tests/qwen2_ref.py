"""Qwen2 test models (no GPU needed to import): the shapes, their GGUF files, and a NumPy float64 forward in the
engine's form -- attn_q / attn_k rows and biases permuted inside each head (new row 2i + j = file row j*d/2 + i),
adjacent-pair RoPE on the permuted rows, the q/k/v bias added before RoPE.

Two modes.  "exact": float64 throughout; it must reproduce transformers' Qwen2ForCausalLM (tests/golden/
hf_qwen2-*.npz, NeoX RoPE on the file-order rows), which is what shows the permutation argument on the CPU.
"ggml": the oracle's rounding points -- activations rounded to bf16 before every weight product;
q, K, V and P rounded to f16 -- the reference of the GPU tests under conftest.logit_tol.
"""
import os

import numpy as np

from llama_p2p_amd import synth
from llama_p2p_amd.synth import LlamaShape

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIAS_STD = 0.3
SEED = 0

# name: (shape, tied embeddings).  rope_base 1e6 and eps 1e-6 as Qwen2.5.
SHAPES = {
    # G = 2: bias + NeoX alone, every format
    "qwen-tiny": (LlamaShape("qwen-tiny", 256, 2, 4, 2, 512, 512, 1e6, 1e-6), True),
    # G = 7; n_embd not a multiple of 256 (as 0.5B's 896); QKV width 576 not a multiple of 256
    "qwen-g7": (LlamaShape("qwen-g7", 448, 2, 7, 1, 512, 512, 1e6, 1e-6), True),
    "qwen-g6": (LlamaShape("qwen-g6", 768, 2, 12, 2, 1024, 512, 1e6, 1e-6), False),
    "qwen-g5": (LlamaShape("qwen-g5", 640, 2, 5, 1, 512, 512, 1e6, 1e-6), False),  # d 128
    # G = 7, d 128, multiples of 256: K-quant capable (half of Qwen2.5-7B's width)
    "qwen-g7-d128": (LlamaShape("qwen-g7-d128", 1792, 2, 14, 2, 1024, 1024, 1e6, 1e-6), False),
    # Qwen2.5-7B's hidden geometry
    "qwen-h3584": (LlamaShape("qwen-h3584", 3584, 1, 28, 4, 2048, 1024, 1e6, 1e-6), False),
}


def golden(name):
    g = np.load(os.path.join(GOLDEN, f"hf_qwen2-{name}.npz"))
    return g["ids"].astype(np.int32), g["logits"].astype(np.float32)


def write_gguf(path, name, wtype="bf16", **kw):
    """The qwen2 file of a shape: NeoX (file-order) rows, synthetic biases, tied embeddings where the shape has them."""
    from llama_p2p_amd import gguf

    shape, tied = SHAPES[name]
    kw.setdefault("arch", "qwen2")
    kw.setdefault("qkv_bias", BIAS_STD)
    kw.setdefault("tie_embeddings", tied)
    return gguf.write_synthetic_gguf(path, shape, seed=SEED, wtype=wtype, **kw)


def permute_rows(w, n_head):
    """The loader's permutation: new row 2i + j of a head = old row j*d/2 + i (llama.cpp's permute)."""
    d = w.shape[0] // n_head
    return w.reshape(n_head, 2, d // 2, *w.shape[1:]).swapaxes(1, 2).reshape(w.shape)


def rbf16(x):
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(np.asarray(x, np.float32))).astype(np.float64)


def rf16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def weights(name, seed=SEED, bias_std=BIAS_STD, permute=True):
    """{gguf name: float64 array}: the synthetic bf16 weights, the biases of synth_bias_f32 (zeros for bias_std 0,
    absent for None), attn_q / attn_k and their biases in the engine's row order when `permute`."""
    shape, tied = SHAPES[name]
    t = {}
    for nm, kind, arr in synth.synth_tensors(shape, seed):
        t[nm] = (synth.bf16_bits_to_f32(arr) if kind == "bf16" else arr).astype(np.float64)
    if tied:
        t["output.weight"] = t["token_embd.weight"]
    for l in range(shape.n_layer):
        p = f"blk.{l}."
        if bias_std is not None:
            for k, tid, n in (("q", synth.L_QB, shape.n_embd), ("k", synth.L_KB, shape.n_embd_kv),
                              ("v", synth.L_VB, shape.n_embd_kv)):
                t[p + f"attn_{k}.bias"] = synth.synth_bias_f32(seed, synth.layer_tid(l, tid), n, bias_std).astype(np.float64)
        if permute:
            for k, nh in (("q", shape.n_head), ("k", shape.n_head_kv)):
                t[p + f"attn_{k}.weight"] = permute_rows(t[p + f"attn_{k}.weight"], nh)
                if bias_std is not None:
                    t[p + f"attn_{k}.bias"] = permute_rows(t[p + f"attn_{k}.bias"], nh)
    return t


def rope_adjacent(x, pos, base):
    """x [T][heads][d]: pairs (2i, 2i+1) rotated by pos * base^(-2i/d)."""
    d = x.shape[-1]
    th = pos[:, None].astype(np.float64) * base ** (-2.0 * np.arange(d // 2) / d)[None, :]
    c, s = np.cos(th)[:, None, :], np.sin(th)[:, None, :]
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


def forward(name, ids, mode="exact", seed=SEED, bias_std=BIAS_STD, t=None):
    """Logits [T][n_vocab] (float64) of the sequence `ids` at positions 0..T-1, every position attending to its
    prefix.  t: weights() to reuse."""
    assert mode in ("exact", "ggml")
    shape, _ = SHAPES[name]
    t = t or weights(name, seed, bias_std)
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
        q, k, v = (xn @ t[p + f"attn_{c}.weight"].T + t.get(p + f"attn_{c}.bias", 0.0) for c in "qkv")
        q = half(rope_adjacent(q.reshape(T, H, d), pos, shape.rope_base))
        k = half(rope_adjacent(k.reshape(T, KV, d), pos, shape.rope_base))
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
