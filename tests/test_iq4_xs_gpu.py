"""An IQ4_XS GGUF (llama-quantize's recipe: IQ4_XS with Q5_K attn_v, Q6_K output) on the native K-quant path, against the
CPU oracle built from the same file's dequantised weights (write_synthetic_gguf(dequant_from=)).

The oracle has no Q8_K activation rounding, so the tolerance is measured, not invented: the same comparison for a
Q4_K_M file of the same shape (native engine against the oracle on ITS dequantised weights) gives the yardstick, and
IQ4_XS may be 2x it -- the codebook's values are up to 8x Q4_K's 0..15 but the scales shrink to match, so the relative
rounding is of the same order.  Figure: worst |logit - oracle| / max |oracle| over a 70-row prompt (prefill GEMM on the
dequantised tiles), a 20-row step (the 17..32-row forms) and four one-row steps (the one-token forms).

Measured on MI355X (profiles/iq4_xs.txt):  test-tiny  q4_k_m 1.694e-2, iq4_xs 2.155e-2 (1.27x);  test-d128  q4_k_m
1.748e-2, iq4_xs 3.196e-2 (1.83x)."""
import functools

import numpy as np
import pytest

from test_kquants_gpu import _oracle_from_gguf

pytestmark = pytest.mark.gpu
ROWS = (70, 20, 1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def run(oracle_mod, tmp, name, wtype):
    """(worst normalised logit error, engine greedy tokens, oracle greedy tokens, weight_type, path)."""
    from llama_p2p_amd import engine, gguf, synth

    shape = synth.SHAPES[name]
    p, q = f"{tmp}/{name}_{wtype}.gguf", f"{tmp}/{name}_{wtype}_deq.gguf"
    gguf.write_synthetic_gguf(p, shape, seed=4, wtype=wtype)
    gguf.write_synthetic_gguf(q, shape, seed=4, dequant_from=p)
    ids = np.concatenate([[1], np.random.default_rng(5).integers(3, shape.n_vocab, sum(ROWS) - 1)]).astype(np.int32)
    octx = _oracle_from_gguf(oracle_mod, q, shape).context(128)
    ref = octx.eval(ids, 0, all_logits=True)
    eng = engine.Engine(p, n_ctx=128, n_seq_max=2)
    got, pos = [], 0
    for n in ROWS:
        got.append(eng.forward_logits(ids[pos:pos + n], pos, slot=0))
        pos += n
    got = np.concatenate(got)
    toks, _ = eng.generate(ids[:70], 4, temperature=0.0, ignore_eos=True)
    wt = eng.info.weight_type
    eng.close()
    want, seq = [], list(ids[:70])
    o2 = _oracle_from_gguf(oracle_mod, q, shape).context(128)
    lg = o2.eval(np.array(seq, np.int32), 0)[0]
    for i in range(4):
        want.append(int(lg.argmax()))
        lg = o2.eval(np.array([want[-1]], np.int32), 70 + i)[0]
    return float(np.abs(got - ref).max() / np.abs(ref).max()), list(toks), want, wt, p


@pytest.mark.parametrize("name", ["test-tiny", "test-d128"])
def test_iq4_xs_file_against_oracle(oracle_mod, tmp_path_factory, name):
    tmp = str(tmp_path_factory.getbasetemp())
    yard, *_ = run(oracle_mod, tmp, name, "q4_k_m")
    err, toks, want, wt, _ = run(oracle_mod, tmp, name, "iq4_xs")
    print(f"{name}: worst |d logit| / max |logit|: q4_k_m {yard:.3e}, iq4_xs {err:.3e}")
    assert wt == 23
    assert toks == want, "greedy tokens"
    assert err <= 2 * yard


def test_llama_completion(oracle_mod, tmp_path_factory):
    from llama_p2p_amd.llama import Llama

    path = run(oracle_mod, str(tmp_path_factory.getbasetemp()), "test-tiny", "iq4_xs")[4]
    out = Llama(model_path=path, n_ctx=64, verbose=False, n_seq_max=2).create_completion("hello model", max_tokens=4, temperature=0.0)
    assert isinstance(out["choices"][0]["text"], str) and out["usage"]["completion_tokens"] >= 1
