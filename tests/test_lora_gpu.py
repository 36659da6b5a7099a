"""LoRA adapters end to end on the GPU: Engine(lora_path=) / Llama(lora_path=) merge the adapter
into the weights at load, so the engine must equal -- bit for bit where the adapter is dyadic -- the engine on a
BF16 file of the merged model (gguf.write_synthetic_gguf(merge_lora=)), and follow the CPU oracle built from the
float64 merge of tests/lora_ref.py.

test-tiny, n_ctx 64, a 24-token prompt and 8 greedy steps.  Dyadic adapters: integer A and B in [-8, 8] with
alpha = 2^-8 at r = 16 (alpha / r = 2^-12), or integers times 2^-6 at r = 3 with alpha 0 (scale = lora_scale): every
f32 evaluation of the merge then gives the same bits (tests/test_lora_host.py)."""
import ctypes

import numpy as np
import pytest

import lora_ref as R
from conftest import assert_logits_close, assert_tokens_match

pytestmark = pytest.mark.gpu

SEED, N_CTX, N_PROMPT, N_STEPS = 3, 64, 24, 8
MATS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
KINDS = {"attn_norm": 0, "attn_q": 1, "attn_k": 2, "attn_v": 3, "attn_output": 4, "ffn_norm": 5, "ffn_gate": 6,
         "ffn_up": 7, "ffn_down": 8}


def _shape():
    from llama_p2p_amd import synth

    return synth.SHAPES["test-tiny"]


def _dims(kind):
    sh = _shape()
    h, kv, ff = sh.n_embd, sh.n_embd_kv, sh.n_ff
    return {"attn_q": (h, h), "attn_k": (kv, h), "attn_v": (kv, h), "attn_output": (h, h), "ffn_gate": (ff, h),
            "ffn_up": (ff, h), "ffn_down": (h, ff)}[kind]


def _adapter(rng, r, names, unit=1.0, real=False):
    t = {}
    for name in names:
        n_out, n_in = _dims(name.split(".")[2])
        if real:
            t[name] = ((0.02 * rng.standard_normal((r, n_in))).astype(np.float32),
                       (0.02 * rng.standard_normal((n_out, r))).astype(np.float32))
        else:
            t[name] = ((rng.integers(-8, 9, (r, n_in)) * unit).astype(np.float32),
                       (rng.integers(-8, 9, (n_out, r)) * unit).astype(np.float32))
    return t


ALL = [f"blk.{l}.{k}.weight" for l in range(2) for k in MATS]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from llama_p2p_amd import gguf

    d = tmp_path_factory.mktemp("lora_gpu")
    rng = np.random.default_rng(17)
    f = {"dir": d, "base": gguf.write_synthetic_gguf(str(d / "base.gguf"), _shape(), seed=SEED)}
    # name -> (tensors, alpha, dtype)
    f["adapters"] = {
        "r16": (_adapter(rng, 16, ALL), 2.0 ** -8, gguf.GGML_F32),
        "r3": (_adapter(rng, 3, ALL, unit=2.0 ** -6), 0.0, gguf.GGML_BF16),
        "qv1": (_adapter(rng, 16, ["blk.1.attn_q.weight", "blk.1.attn_v.weight"]), 2.0 ** -8, gguf.GGML_F32),
        "real": (_adapter(rng, 8, ALL, real=True), 16.0, gguf.GGML_F16),
    }
    for name, (tensors, alpha, dtype) in f["adapters"].items():
        f[name] = gguf.write_lora_gguf(str(d / f"{name}.gguf"), tensors, alpha, dtype=dtype)
    return f


def _prompt():
    rng = np.random.default_rng(23)
    return np.concatenate([[1], rng.integers(3, _shape().n_vocab, N_PROMPT - 1)]).astype(np.int32)


def _run(eng):
    """(logits [N_PROMPT + N_STEPS][V], the N_STEPS greedy tokens)."""
    rows = [eng.forward_logits(_prompt())]
    toks = []
    for k in range(N_STEPS):
        toks.append(int(rows[-1][-1].argmax()))
        rows.append(eng.forward_logits([toks[-1]], pos0=N_PROMPT + k))
    return np.concatenate(rows), toks


def _engine(path, **kw):
    from llama_p2p_amd import engine

    return engine.Engine(path, n_ctx=N_CTX, n_seq_max=2, **kw)


def _result(path, **kw):
    e = _engine(path, **kw)
    try:
        return _run(e), e.lora_info(), e.info.weight_type
    finally:
        e.close()


@pytest.fixture(scope="module")
def base_result(files):
    return _result(files["base"])[0]


def _merged_file(files, name, scale, dequant_from=None):
    from llama_p2p_amd import gguf

    p = str(files["dir"] / f"merged_{name}_{scale}_{'deq' if dequant_from else 'bf16'}.gguf")
    return gguf.write_synthetic_gguf(p, _shape(), seed=SEED, dequant_from=dequant_from, merge_lora=(files[name], scale))


@pytest.mark.parametrize("name,scale", [("r16", 1.0), ("r16", 0.5), ("r3", 1.0), ("r3", 0.5)])
def test_adapter_equals_its_merged_file_and_differs_from_the_base(files, base_result, name, scale):
    (lg, toks), info, wt = _result(files["base"], lora_path=files[name], lora_scale=scale)
    (lm, tm), info_m, _ = _result(_merged_file(files, name, scale))
    assert np.array_equal(lg, lm) and toks == tm
    assert not np.array_equal(lg, base_result[0])  # the adapter matters
    tensors, alpha, _ = files["adapters"][name]
    r = next(iter(tensors.values()))[0].shape[0]
    assert info == {"n_tensors": 14, "rank_max": r, "alpha": alpha, "lora_scale": scale} and wt == 30
    assert info_m == {"n_tensors": 0, "rank_max": 0, "alpha": 0.0, "lora_scale": 0.0}


def _oracle(oracle_mod, files, name, scale):
    """The oracle on the base file's tensors with the merged matrices of the float64 reference put in."""
    from llama_p2p_amd import gguf

    tensors, alpha, dtype = files["adapters"][name]
    stored, _ = gguf.read_lora_gguf(files[name])  # the values as the file's type holds them
    r = gguf.GGUFReader(files["base"])
    om = oracle_mod.OracleModel(_shape(), seed=None)
    for tname in r.tensors:
        arr = np.ascontiguousarray(r.tensor(tname))
        if tname in stored:
            A, B = stored[tname]
            _, arr = R.merge_f64(arr, A, B, gguf.lora_effective_scale(scale, alpha, A.shape[0]))
        if tname == "token_embd.weight":
            om.set_tensor(-1, 1, arr)
        elif tname == "output_norm.weight":
            om.set_tensor(-1, 2, arr)
        elif tname == "output.weight":
            om.set_tensor(-1, 3, arr)
        else:
            _, l, kind, _ = tname.split(".")
            om.set_tensor(int(l), KINDS[kind], arr)
    return om


@pytest.mark.parametrize("name", ["r16", "real"])
def test_adapter_against_the_oracle(oracle_mod, files, base_result, name):
    (lg, toks), info, _ = _result(files["base"], lora_path=files[name], lora_scale=1.0)
    assert info["n_tensors"] == 14
    seq = np.concatenate([_prompt(), np.asarray(toks[:-1], np.int32)])
    ref = _oracle(oracle_mod, files, name, 1.0).context(N_CTX).eval(seq, 0, all_logits=True)
    got = lg[:len(seq)]
    assert_logits_close(got, ref, name)
    assert_tokens_match(got, ref, name)
    assert not np.array_equal(lg, base_result[0])


def test_scale_zero_is_the_base_bit_for_bit(files, base_result):
    (lg, toks), info, wt = _result(files["base"], lora_path=files["r16"], lora_scale=0.0)
    assert np.array_equal(lg, base_result[0]) and toks == base_result[1]
    assert info == {"n_tensors": 0, "rank_max": 0, "alpha": 2.0 ** -8, "lora_scale": 0.0} and wt == 30


def test_adapter_of_two_tensors_of_layer_1(files, base_result):
    (lg, toks), info, _ = _result(files["base"], lora_path=files["qv1"])
    assert info["n_tensors"] == 2 and info["rank_max"] == 16
    (lm, tm), _, _ = _result(_merged_file(files, "qv1", 1.0))
    assert np.array_equal(lg, lm) and toks == tm
    assert not np.array_equal(lg, base_result[0])


def test_q8_0_base_is_dequantised_and_merged(files):
    from llama_p2p_amd import gguf

    p8 = gguf.write_synthetic_gguf(str(files["dir"] / "q8.gguf"), _shape(), seed=SEED, wtype="q8_0")
    (lg, toks), info, wt = _result(p8, lora_path=files["r16"])
    assert wt == 30 and info["n_tensors"] == 14
    (lm, tm), _, wtm = _result(_merged_file(files, "r16", 1.0, dequant_from=p8))
    assert wtm == 30 and np.array_equal(lg, lm) and toks == tm
    (l8, _), info8, wt8 = _result(p8)
    assert wt8 == 8 and info8["n_tensors"] == 0 and not np.array_equal(l8, lg)


def test_two_stage_engines_equal_one_engine(files):
    import torch

    sh = _shape()
    full = _engine(files["base"], lora_path=files["r16"])
    stages = [_engine(files["base"], layer_begin=lb, layer_end=le, lora_path=files["r16"]) for lb, le in ((0, 1), (1, 2))]
    assert [s.lora_info()["n_tensors"] for s in stages] == [7, 7] and full.lora_info()["n_tensors"] == 14
    buf = torch.empty((64, sh.n_embd), dtype=torch.float32, device=torch.device("cuda", 0))

    def one(ids, pos0):
        n = len(ids)
        return full.stage_rows([0] * n, list(range(pos0, pos0 + n)), ids, want_logits=True)

    def two(ids, pos0):
        n = len(ids)
        slots, pos = [0] * n, list(range(pos0, pos0 + n))
        stages[0].stage_rows(slots, pos, ids, x_out=buf.data_ptr())
        stages[0].sync()
        return stages[1].stage_rows(slots, pos, None, x_in=buf.data_ptr(), want_logits=True)

    results = []
    for fwd in (one, two):
        rows = [fwd(_prompt(), 0)]
        toks = []
        for k in range(N_STEPS):
            toks.append(int(rows[-1][-1].argmax()))
            rows.append(fwd(np.asarray([toks[-1]], np.int32), N_PROMPT + k))
        results.append((np.concatenate(rows), toks))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]
    for e in stages + [full]:
        e.close()


def test_bad_adapter_leaves_no_engine(files):
    from llama_p2p_amd import engine as E
    from llama_p2p_amd import gguf

    # an adapter for another model: its attn_k does not fit test-tiny's 128 kv rows
    rng = np.random.default_rng(1)
    bad = gguf.write_lora_gguf(str(files["dir"] / "bad.gguf"),
                               {"blk.0.attn_k.weight": (rng.standard_normal((4, 256)), rng.standard_normal((256, 4)))}, 8.0)
    h = ctypes.c_void_p()
    rc = E.lib().mx_engine_create_lora(files["base"].encode(), None, bad.encode(), 1.0, ctypes.byref(h))
    assert rc == E.MX_ERR_MODEL and not h.value
    assert "blk.0.attn_k.weight.lora_b" in E.lib().mx_last_error().decode()
    with pytest.raises(E.MxError):
        _engine(files["base"], lora_path=bad)


def test_llama_keywords(files, capsys):
    from llama_p2p_amd import gguf
    from llama_p2p_amd.llama import Llama

    prompt = "hello model peer node"

    def text(path, **kw):
        llm = Llama(path, n_ctx=N_CTX, n_seq_max=2, **kw)
        try:
            return llm(prompt, max_tokens=N_STEPS, temperature=0.0)["choices"][0]["text"], llm
        finally:
            llm.close()

    capsys.readouterr()
    got, llm = text(files["base"], lora_path=files["r16"], lora_scale=0.5, lora_base="ignored.gguf", verbose=True)
    assert (llm.lora_path, llm.lora_scale, llm.lora_base) == (files["r16"], 0.5, "ignored.gguf")
    line = capsys.readouterr().err
    assert "merged 14 tensors" in line and "dequantised" not in line
    want, _ = text(_merged_file(files, "r16", 0.5), verbose=False)
    base, llm0 = text(files["base"], verbose=False)
    assert llm0.lora_path is None and llm0.lora_scale == 1.0
    assert got == want and got != base

    p8 = gguf.write_synthetic_gguf(str(files["dir"] / "q8_llama.gguf"), _shape(), seed=SEED, wtype="q8_0")
    text(p8, lora_path=files["qv1"], verbose=True)
    line = capsys.readouterr().err
    assert "merged 2 tensors" in line and "runs as bf16" in line and "bytes" in line

    bad = gguf.write_lora_gguf(str(files["dir"] / "bad_llama.gguf"),
                               {"token_embd.weight": (np.zeros((2, 256)), np.zeros((512, 2)))}, 1.0)
    with pytest.raises(RuntimeError, match="Failed to initialize LoRA adapter from lora path: ") as err:
        Llama(files["base"], n_ctx=N_CTX, lora_path=bad, verbose=False)
    assert "token_embd.weight" in str(err.value.__cause__)
