"""GGUF IQ4_XS on the host: gguf.dequantize_iq4_xs against the format's formula in float64 on a hand-built block, the
synthetic blocks of synth.kq_blocks, and the per-tensor types of a write_synthetic_gguf(wtype="iq4_xs") file."""
import numpy as np

import iq4_ref as Q
from llama_p2p_amd import gguf, synth


def hand_block():
    """One block with every index present in both nibbles, ls 0, 31, 32, 63 among the scales, d = 0x2E66 (0.0999...)."""
    ls = np.array([0, 31, 32, 63, 1, 62, 33, 17])
    idx = (np.arange(256) * 7 + np.arange(256) // 16) % 16
    b = np.zeros(136, np.uint8)
    b[0], b[1] = 0x66, 0x2E
    sh = sum(int(l >> 4) << (2 * j) for j, l in enumerate(ls))
    b[2], b[3] = sh & 0xFF, sh >> 8
    for j, l in enumerate(ls):
        b[4 + j // 2] |= (l & 15) << (4 * (j & 1))
    for k in range(256):
        b[8 + 16 * (k // 32) + k % 16] |= idx[k] << (4 * ((k % 32) // 16))
    return b, ls, idx


def test_dequantize_one_block_against_the_formula():
    b, ls, idx = hand_block()
    assert set(idx[:16]) | set(idx[16:32]) == set(range(16))
    d = float(np.array([0x2E66], np.uint16).view(np.float16)[0])
    want = d * np.repeat(ls - 32, 32).astype(np.float64) * Q.KV[idx]  # |.| < 2^24 d: every product exact in f32
    got = gguf.dequantize(gguf.GGML_IQ4_XS, b[None], (1, 256))
    assert got.dtype == np.float32 and np.array_equal(got[0].astype(np.float64), want)


def test_synthetic_blocks_and_file_types(tmp_path):
    blk = synth.kq_blocks(synth.GGML_IQ4_XS, 40, seed=5, tid=77)
    assert blk.shape == (40, 136) and (blk[:, 1] == 0x01).all()  # d = 0x0100 + a random byte; the rest is the hash
    shape = synth.LlamaShape("iq4-host", 256, 8, 4, 2, 512, 512)
    path = gguf.write_synthetic_gguf(str(tmp_path / "iq4.gguf"), shape, seed=2, wtype="iq4_xs")
    r = gguf.GGUFReader(path)
    assert r.metadata["general.file_type"] == 30
    want = {"token_embd.weight": 23, "output.weight": 14}
    for l in range(8):
        for k in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up"):
            want[f"blk.{l}.{k}.weight"] = 23
        want[f"blk.{l}.attn_v.weight"] = 13
        want[f"blk.{l}.ffn_down.weight"] = 13 if l < 1 else 23
    assert {n: i["type"] for n, i in r.tensors.items() if n in want} == want
    t, b = synth.kq_tensor("iq4_xs", "attn_q", 3, shape, 2)
    assert t == 23 and np.array_equal(r.tensor("blk.3.attn_q.weight"), b)
