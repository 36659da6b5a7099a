"""Qwen2 on the CPU: the NumPy reference in the engine's form (permuted rows, adjacent-pair RoPE, bias
before RoPE) against transformers' Qwen2ForCausalLM goldens, the GGUF writer's qwen2 options, and the qwen2
pre-tokeniser."""
import functools
import hashlib

import numpy as np
import pytest
from conftest import logit_tol

import qwen2_ref as Q
from llama_p2p_amd import gguf, synth
from llama_p2p_amd.tokenizer import Tokenizer


@functools.lru_cache(maxsize=None)
def _both(name):
    ids, lg = Q.golden(name)
    w = Q.weights(name)
    return lg, Q.forward(name, ids, "exact", t=w), Q.forward(name, ids, "ggml", t=w)


@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_exact_reference_reproduces_hf(name):
    """Permuted rows + adjacent-pair RoPE + bias before RoPE is Qwen2: within 1e-5 of the logit scale of HF's NeoX
    forward on the file-order rows (measured 5e-7 .. 1.2e-6)."""
    lg, ex, _ = _both(name)
    d = np.abs(ex - lg).max() / np.abs(lg).max()
    print(f"{name}: exact vs HF {d:.3g} of max|logit| {np.abs(lg).max():.3f}")
    assert d <= 1e-5


@pytest.mark.parametrize("name", list(Q.SHAPES))
def test_ggml_reference_within_bf16_tolerance(name):
    """The oracle's rounding points leave the reference inside conftest.logit_tol of HF (measured 0.11 .. 0.20 of it)."""
    lg, _, gg = _both(name)
    r = (np.abs(gg - lg) / logit_tol(lg)).max()
    print(f"{name}: ggml vs HF {r:.3f} of the tolerance")
    assert r <= 1.0


def test_bias_moves_the_logits():
    """std 0.3 is no decoration: without the bias most logits leave the tolerance and most argmaxes change."""
    ids, lg = Q.golden("qwen-g7")
    nb = Q.forward("qwen-g7", ids, "exact", t=Q.weights("qwen-g7", bias_std=None))
    out = np.abs(nb - lg) > logit_tol(lg)
    assert out.mean() > 0.8 and (nb.argmax(-1) != lg.argmax(-1)).mean() > 0.8


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_writer_qwen2_keys_bias_and_tied(tmp_path):
    shape, tied = Q.SHAPES["qwen-tiny"]
    r = gguf.GGUFReader(Q.write_gguf(str(tmp_path / "q.gguf"), "qwen-tiny"))
    md = r.metadata
    assert md["general.architecture"] == "qwen2" and tied
    assert md["qwen2.embedding_length"] == shape.n_embd and md["qwen2.block_count"] == shape.n_layer
    assert md["qwen2.attention.head_count"] == shape.n_head and md["qwen2.attention.head_count_kv"] == shape.n_head_kv
    assert md["qwen2.feed_forward_length"] == shape.n_ff and md["qwen2.rope.dimension_count"] == shape.head_dim
    assert md["qwen2.rope.freq_base"] == np.float32(1e6) and md["qwen2.attention.layer_norm_rms_epsilon"] == np.float32(1e-6)
    assert not any(k.startswith("llama.") for k in md)
    assert "output.weight" not in r.tensors and "token_embd.weight" in r.tensors
    for l in range(shape.n_layer):
        for k, tid, n in (("q", synth.L_QB, shape.n_embd), ("k", synth.L_KB, shape.n_embd_kv), ("v", synth.L_VB, shape.n_embd_kv)):
            info = r.tensors[f"blk.{l}.attn_{k}.bias"]
            assert info["type"] == gguf.GGML_F32 and tuple(info["ne"]) == (n,)
            assert np.array_equal(r.tensor(f"blk.{l}.attn_{k}.bias"), synth.synth_bias_f32(Q.SEED, synth.layer_tid(l, tid), n))
    # the matrices are the synthetic ones in file order
    assert np.array_equal(r.tensor("blk.1.attn_q.weight"), synth.synth_weight_bf16(Q.SEED, synth.layer_tid(1, synth.L_Q), 256, 256))


@pytest.mark.parametrize("wtype", ["bf16", "q8_0"])
def test_writer_neox_rows_are_the_inverse_of_the_loader_permutation(tmp_path, wtype):
    """qk_rows="neox" is a row gather on values or blocks: the loader's permutation (qwen2_ref.permute_rows) of the
    file's rows gives the "norm" file's rows back, and nothing but attn_q / attn_k moves."""
    shape, _ = Q.SHAPES["qwen-tiny"]
    a = gguf.GGUFReader(Q.write_gguf(str(tmp_path / "a.gguf"), "qwen-tiny", wtype=wtype, qk_rows="norm"))
    b = gguf.GGUFReader(Q.write_gguf(str(tmp_path / "b.gguf"), "qwen-tiny", wtype=wtype, qk_rows="neox"))
    assert list(a.tensors) == list(b.tensors)
    for name in a.tensors:
        x, y = np.asarray(a.tensor(name)), np.asarray(b.tensor(name))
        nh = shape.n_head if ".attn_q." in name else shape.n_head_kv if ".attn_k." in name else 0
        if nh:
            assert not np.array_equal(x, y), name
            assert np.array_equal(Q.permute_rows(y, nh), x), name
        else:
            assert np.array_equal(x, y), name
    if wtype == "q8_0":  # 34-byte blocks moved whole
        assert a.tensors["blk.0.attn_q.weight"]["type"] == gguf.GGML_Q8_0
        assert a.tensor("blk.0.attn_q.weight").shape == (256, 256 // 32 * 34)


def test_writer_defaults_are_byte_identical(tmp_path):
    shape = synth.SHAPES["test-tiny"]
    p0 = gguf.write_synthetic_gguf(str(tmp_path / "0.gguf"), shape, seed=3)
    p1 = gguf.write_synthetic_gguf(str(tmp_path / "1.gguf"), shape, seed=3, arch="llama", qkv_bias=None,
                                   tie_embeddings=False, qk_rows="norm")
    assert _sha(p0) == _sha(p1)
    l0 = gguf.write_lora_gguf(str(tmp_path / "l0.gguf"), {"blk.0.attn_q.weight": (np.ones((2, 256)), np.ones((256, 2)))}, 4.0)
    l1 = gguf.write_lora_gguf(str(tmp_path / "l1.gguf"), {"blk.0.attn_q.weight": (np.ones((2, 256)), np.ones((256, 2)))}, 4.0,
                              arch="llama")
    assert _sha(l0) == _sha(l1)
    with pytest.raises(ValueError):
        gguf.write_synthetic_gguf(str(tmp_path / "x.gguf"), shape, qk_rows="other")


def _bpe_tokenizer(pre, add_bos=True):
    b2u = Tokenizer(["x"])._b2u
    toks = ["<bos>"] + [b2u[b] for b in range(256)]
    md = {"tokenizer.ggml.model": "gpt2", "tokenizer.ggml.tokens": toks, "tokenizer.ggml.merges": [],
          "tokenizer.ggml.token_type": [3] + [1] * 256, "tokenizer.ggml.bos_token_id": 0,
          "tokenizer.ggml.add_bos_token": add_bos}
    if pre is not None:
        md["tokenizer.ggml.pre"] = pre
    return Tokenizer.from_gguf_metadata(md)


def test_qwen2_pretokeniser_splits_digits():
    """The words the pre-tokeniser makes of "12345": five for qwen2, 123 | 45 for the Llama-3 default."""
    words = lambda tk: (tk.tokenize(b"12345", add_bos=False), list(tk._seg_cache))
    assert words(_bpe_tokenizer("qwen2"))[1] == ["1", "2", "3", "4", "5"]
    for pre in (None, "llama-bpe", "something-else"):
        assert words(_bpe_tokenizer(pre))[1] == ["123", "45"]
    # the ids are the same bytes either way (no merges in this vocabulary)
    assert words(_bpe_tokenizer("qwen2"))[0] == words(_bpe_tokenizer(None))[0] == [1 + b for b in b"12345"]


def test_add_bos_token_false_is_honoured():
    assert _bpe_tokenizer("qwen2", add_bos=False).tokenize(b"1", add_bos=True) == [1 + ord("1")]
    assert _bpe_tokenizer("qwen2", add_bos=True).tokenize(b"1", add_bos=True) == [0, 1 + ord("1")]
