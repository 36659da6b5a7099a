"""Generate the Qwen2 golden vectors tests/golden/hf_qwen2-<name>.npz (committed; re-run to refresh).

    python tests/golden/make_golden_qwen2.py

The C oracle knows no q/k/v bias, so the reference for Qwen2 is an independent implementation, transformers'
``Qwen2ForCausalLM`` (5.15, local code, built from a config -- no download), as make_golden.py uses
``LlamaForCausalLM``.  A qwen2 GGUF keeps attn_q / attn_k in HF's row order (NeoX RoPE: convert_hf_to_gguf does not
permute them), so HF is loaded with the synthetic weights *in file order* and the synthetic biases; the engine and
tests/qwen2_ref.py permute the rows at load and rotate adjacent pairs instead.  HF runs in float32, eager attention.

Each fixture holds ``ids`` (40 tokens, the generator of make_golden.py) and the fp32 ``logits`` at every position.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import qwen2_ref as Q  # noqa: E402

SEQ_LEN = 40


def hf_model(name):
    import torch
    from transformers import Qwen2Config, Qwen2ForCausalLM

    shape, tied = Q.SHAPES[name]
    cfg = Qwen2Config(vocab_size=shape.n_vocab, hidden_size=shape.n_embd, intermediate_size=shape.n_ff,
                      num_hidden_layers=shape.n_layer, num_attention_heads=shape.n_head,
                      num_key_value_heads=shape.n_head_kv, rms_norm_eps=shape.eps, rope_theta=shape.rope_base,
                      max_position_embeddings=4096, tie_word_embeddings=tied, use_sliding_window=False,
                      attn_implementation="eager")
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).float().eval()
    t = Q.weights(name, permute=False)  # file order

    def W(n):
        return torch.from_numpy(np.ascontiguousarray(t[n], dtype=np.float32))

    sd = {"model.embed_tokens.weight": W("token_embd.weight"), "model.norm.weight": W("output_norm.weight")}
    if not tied:
        sd["lm_head.weight"] = W("output.weight")
    for l in range(shape.n_layer):
        p, q = f"blk.{l}.", f"model.layers.{l}."
        for c in "qkv":
            sd[q + f"self_attn.{c}_proj.weight"] = W(p + f"attn_{c}.weight")
            sd[q + f"self_attn.{c}_proj.bias"] = W(p + f"attn_{c}.bias")
        sd[q + "self_attn.o_proj.weight"] = W(p + "attn_output.weight")
        sd[q + "mlp.gate_proj.weight"] = W(p + "ffn_gate.weight")
        sd[q + "mlp.up_proj.weight"] = W(p + "ffn_up.weight")
        sd[q + "mlp.down_proj.weight"] = W(p + "ffn_down.weight")
        sd[q + "input_layernorm.weight"] = W(p + "attn_norm.weight")
        sd[q + "post_attention_layernorm.weight"] = W(p + "ffn_norm.weight")
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [m for m in missing if "rotary" not in m and not (tied and m == "lm_head.weight")]
    assert not missing and not unexpected, (missing, unexpected)
    if tied:
        assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    return model


def make(name):
    import torch

    shape, _ = Q.SHAPES[name]
    rng = np.random.default_rng(1234)
    ids = np.concatenate([[1], rng.integers(3, shape.n_vocab, SEQ_LEN - 1)]).astype(np.int32)
    model = hf_model(name)
    with torch.no_grad():
        out = model(torch.from_numpy(ids.astype(np.int64))[None], use_cache=False)
    logits = out.logits[0].float().numpy().astype(np.float32)
    path = os.path.join(HERE, f"hf_qwen2-{name}.npz")
    np.savez_compressed(path, ids=ids, logits=logits, shape=name, seed=Q.SEED, bias_std=Q.BIAS_STD)
    print(f"wrote {path}: ids {ids.shape}, logits {logits.shape}, max|logit| {np.abs(logits).max():.3f}")


if __name__ == "__main__":
    for s in Q.SHAPES:
        make(s)
