"""LoRA adapters, host side (no GPU): the adapter file format, the checks of an adapter against its
base (mx_lora_check), the numpy merge against the float64 reference, and the Llama keywords."""
import ctypes
import hashlib
import inspect

import numpy as np
import pytest

import lora_ref as R

SEED = 3


@pytest.fixture(scope="module")
def E():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    from llama_p2p_amd import gguf, synth

    p = str(tmp_path_factory.mktemp("lora_host") / "base.gguf")
    gguf.write_synthetic_gguf(p, synth.SHAPES["test-tiny"], seed=SEED)
    return p


def _pair(rng, n_out, n_in, r):
    return (rng.integers(-8, 9, (r, n_in)).astype(np.float32), rng.integers(-8, 9, (n_out, r)).astype(np.float32))


def _good_tensors(rng, r_down=3):
    # test-tiny: n_embd 256, n_embd_kv 128, n_ff 512
    return {"blk.0.attn_q.weight": _pair(rng, 256, 256, 4), "blk.1.attn_v.weight": _pair(rng, 128, 256, 2),
            "blk.1.ffn_down.weight": _pair(rng, 256, 512, r_down)}


def _write_raw(path, tensors, meta=None):
    """An adapter file with any metadata and any tensors: [(name, array in numpy order, ggml type)]."""
    from llama_p2p_amd import gguf

    md = {"general.type": "adapter", "general.architecture": "llama", "adapter.type": "lora"}
    md.update(meta or {})
    w = gguf.GGUFWriter(path)
    for k, v in md.items():
        if v is not None:
            w.add_string(k, v)
    w.add_float32("adapter.lora.alpha", 8.0)
    arrays = []
    for name, arr, t in tensors:
        w.add_tensor_info(name, arr.shape, t)
        arrays.append(gguf.quantize_q8_0(arr) if t == gguf.GGML_Q8_0 else arr)
    w.write(arrays)
    return path


def test_adapter_file_round_trip(E, tmp_path):
    from llama_p2p_amd import gguf

    rng = np.random.default_rng(1)
    tensors = _good_tensors(rng)
    for dtype in (gguf.GGML_F32, gguf.GGML_F16, gguf.GGML_BF16):
        p = str(tmp_path / f"a{dtype}.gguf")
        gguf.write_lora_gguf(p, tensors, alpha=0.5, dtype=dtype)
        r = gguf.GGUFReader(p)
        assert r.metadata["general.type"] == "adapter" and r.metadata["adapter.type"] == "lora"
        assert r.metadata["general.architecture"] == "llama" and r.metadata["adapter.lora.alpha"] == 0.5
        assert sorted(r.tensors) == sorted(n + s for n in tensors for s in (".lora_a", ".lora_b"))
        for name, (A, B) in tensors.items():
            ia, ib = r.tensors[name + ".lora_a"], r.tensors[name + ".lora_b"]
            assert ia["type"] == dtype and ib["type"] == dtype
            assert tuple(ia["ne"]) == (A.shape[1], A.shape[0]) and tuple(ib["ne"]) == (B.shape[1], B.shape[0])
            # small integers are exact in all three types
            assert np.array_equal(gguf.dequantize(dtype, r.tensor(name + ".lora_a"), A.shape), A)
            assert np.array_equal(gguf.dequantize(dtype, r.tensor(name + ".lora_b"), B.shape), B)
        got, alpha = gguf.read_lora_gguf(p)
        assert alpha == 0.5 and all(np.array_equal(got[n][0], tensors[n][0]) for n in tensors)
        E.gguf_check(p)


def test_llama_names_the_keywords():
    from llama_p2p_amd.llama import Llama

    params = inspect.signature(Llama.__init__).parameters
    assert params["lora_path"].default is None and params["lora_base"].default is None
    assert params["lora_scale"].default == 1.0
    for name in ("lora_path", "lora_scale", "lora_base"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY


def test_engine_binding_declares_the_surface(E):
    for name in ("mx_engine_create_lora", "mx_lora_check", "mx_engine_lora_info", "mx_lora_merge_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
    params = inspect.signature(E.Engine.__init__).parameters
    assert params["lora_path"].default is None and params["lora_scale"].default == 1.0
    assert [n for n, _ in E.MxLoraInfo._fields_] == ["n_tensors", "rank_max", "alpha", "lora_scale"]


def test_lora_check_accepts_a_good_pair(E, base, tmp_path):
    from llama_p2p_amd import gguf

    p = str(tmp_path / "good.gguf")
    gguf.write_lora_gguf(p, _good_tensors(np.random.default_rng(2)), alpha=16.0, dtype=gguf.GGML_F16)
    E.lora_check(base, p)
    assert E.lib().mx_lora_check(base.encode(), p.encode()) == E.MX_OK


F32, Q8 = 0, 8
_Z = np.zeros


def _refusals():
    a, b = _Z((4, 256), np.float32), _Z((256, 4), np.float32)
    q = "blk.0.attn_q.weight"
    good = [(q + ".lora_a", a, F32), (q + ".lora_b", b, F32)]

    def on(target, n_out, n_in, r=4):
        return [(target + ".lora_a", _Z((r, n_in), np.float32), F32), (target + ".lora_b", _Z((n_out, r), np.float32), F32)]

    return [
        # (case, tensors, metadata overrides, what the message must name)
        ("general_type", good, {"general.type": "model"}, "general.type"),
        ("no_general_type", good, {"general.type": None}, "general.type"),
        ("adapter_type", good, {"adapter.type": "ia3"}, "adapter.type"),
        ("architecture", good, {"general.architecture": "gemma"}, "general.architecture"),
        ("a_without_b", good[:1], None, q + ".lora_a"),
        ("b_without_a", good[1:], None, q + ".lora_b"),
        ("a_ne0", [(q + ".lora_a", _Z((4, 128), np.float32), F32), good[1]], None, q + ".lora_a"),
        ("b_ne1", [good[0], (q + ".lora_b", _Z((128, 4), np.float32), F32)], None, q + ".lora_b"),
        ("rank_mismatch", [good[0], (q + ".lora_b", _Z((256, 8), np.float32), F32)], None, q + ".lora_a"),
        ("rank_0", on(q, 256, 256, r=0), None, q),
        ("not_in_base", on("blk.7.attn_q.weight", 256, 256), None, "blk.7.attn_q.weight"),
        ("token_embd", on("token_embd.weight", 512, 256), None, "token_embd.weight"),
        ("output", on("output.weight", 512, 256), None, "output.weight"),
        ("norm", on("blk.0.attn_norm.weight", 256, 1), None, "blk.0.attn_norm.weight"),
        ("quantised", [(q + ".lora_a", a, Q8), (q + ".lora_b", b, F32)], None, q + ".lora_a"),
        ("stray_tensor", good + [("blk.0.attn_q.weight.scale", _Z((4,), np.float32), F32)], None,
         "blk.0.attn_q.weight.scale"),
    ]


@pytest.mark.parametrize("case,tensors,meta,names", _refusals(), ids=[c[0] for c in _refusals()])
def test_lora_check_refuses(E, base, tmp_path, case, tensors, meta, names):
    p = _write_raw(str(tmp_path / f"{case}.gguf"), tensors, meta)
    E.gguf_check(p)  # a sound container: the refusal is the adapter's
    assert E.lib().mx_lora_check(base.encode(), p.encode()) == E.MX_ERR_MODEL
    msg = E.lib().mx_last_error().decode()
    assert names in msg, msg
    # the engine refuses the same file with the same words before it looks for a GPU
    h = ctypes.c_void_p()
    rc = E.lib().mx_engine_create_lora(base.encode(), None, p.encode(), 1.0, ctypes.byref(h))
    assert rc == E.MX_ERR_MODEL and not h.value and names in E.lib().mx_last_error().decode()


def test_lora_check_arguments(E, base, tmp_path):
    from llama_p2p_amd import gguf

    p = str(tmp_path / "good.gguf")
    gguf.write_lora_gguf(p, _good_tensors(np.random.default_rng(2)), alpha=1.0)
    L = E.lib()
    assert L.mx_lora_check(None, p.encode()) == E.MX_ERR_ARG
    assert L.mx_lora_check(base.encode(), None) == E.MX_ERR_ARG
    assert L.mx_lora_check(b"synthetic:test-tiny", p.encode()) == E.MX_ERR_ARG
    assert L.mx_lora_check(base.encode(), str(tmp_path / "missing.gguf").encode()) == E.MX_ERR_MODEL
    h = ctypes.c_void_p()
    assert L.mx_engine_create_lora(b"synthetic:test-tiny", None, p.encode(), 1.0, ctypes.byref(h)) == E.MX_ERR_ARG
    assert L.mx_engine_create_lora(base.encode(), None, p.encode(), float("nan"), ctypes.byref(h)) == E.MX_ERR_ARG
    assert L.mx_engine_create_lora(base.encode(), None, None, 1.0, ctypes.byref(h)) == E.MX_ERR_ARG
    assert L.mx_engine_lora_info(None, None) == E.MX_ERR_ARG


def test_reference_rounding():
    # exact RNE to bf16: ties to even, carries into the exponent, signed zeros, the subnormal spacing
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 2.0 - 2.0 ** -9, -0.0, 0.0,
                  2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, -(1.0 + 2.0 ** -8)])
    want = np.array([0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x4000, 0x8000, 0x0000, 0x0001, 0x0000, 0x0002, 0xBF80], np.uint16)
    assert np.array_equal(R.f64_to_bf16_rne(x), want)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 0x7F80, 4096).astype(np.uint16)  # every finite positive bf16 is a fixed point
    assert np.array_equal(R.f64_to_bf16_rne(R.bf16_to_f64(bits)), bits)


@pytest.mark.parametrize("rows,cols,r", R.KERNEL_SHAPES)
def test_numpy_merge_equals_reference_on_dyadic_inputs(rows, cols, r):
    """gguf.lora_merge_bf16 (numpy f32) against the float64 reference, bit for bit, on the inputs of the kernel's
    bitwise test: there the f32 evaluation has one rounding, the last, and the tests on the GPU rely on that."""
    from llama_p2p_amd import gguf

    w, A, B, scale = R.dyadic_case(rows, cols, r, seed=100 + r)
    x, want = R.merge_f64(w, A, B, scale)
    acc = B.astype(np.float64) @ A.astype(np.float64)
    assert np.array_equal(acc, np.rint(acc)) and np.abs(acc).max() <= 64 * r
    assert np.array_equal(gguf.lora_merge_bf16(w, A, B, scale), want)
    # the sum in ascending and in descending r, one f32 operation at a time
    for order in (range(r), range(r - 1, -1, -1)):
        s = np.zeros((rows, cols), np.float32)
        for j in order:
            s = (s + B[:, j:j + 1] * A[j:j + 1, :]).astype(np.float32)
        f32 = (R.bf16_to_f64(w).astype(np.float32) + np.float32(scale) * s).astype(np.float32)
        assert np.array_equal(R.f64_to_bf16_rne(f32.astype(np.float64)), want)
    assert (want != w).mean() > 0.5


@pytest.mark.parametrize("rows,cols,r", R.KERNEL_SHAPES)
def test_interval_rule_holds_an_f32_evaluation_and_is_tight(rows, cols, r):
    """The rule of the real-valued kernel test, checked on the CPU: an f32 evaluation in ascending and in descending
    r stays inside [RNE(x - d), RNE(x + d)] everywhere, and at most 1 % of the intervals hold more than one value."""
    w, A, B, scale = R.real_case(rows, cols, r, seed=200 + r)
    lo, hi, _ = R.merge_interval(w, A, B, scale, r)
    lo_v, hi_v = R.bf16_to_f64(lo), R.bf16_to_f64(hi)
    assert (lo != hi).mean() <= 0.01
    for order in (range(r), range(r - 1, -1, -1)):
        s = np.zeros((rows, cols), np.float32)
        for j in order:
            s = (s + B[:, j:j + 1] * A[j:j + 1, :]).astype(np.float32)
        f32 = (R.bf16_to_f64(w).astype(np.float32) + np.float32(scale) * s).astype(np.float32)
        got = R.bf16_to_f64(R.f64_to_bf16_rne(f32.astype(np.float64)))
        assert ((got >= lo_v) & (got <= hi_v)).all()


def test_effective_scale_is_llama_cpps():
    from llama_p2p_amd import gguf

    assert gguf.lora_effective_scale(0.5, 2.0 ** -8, 16) == np.float32(2.0 ** -13)
    assert gguf.lora_effective_scale(0.5, 0.0, 16) == np.float32(0.5)
    assert gguf.lora_effective_scale(1.0, 16.0, 3) == np.float32(np.float32(16.0) / np.float32(3.0))


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_synthetic_file_without_merge_is_unchanged_and_merge_writes_the_merged_matrices(base, tmp_path):
    from llama_p2p_amd import gguf, synth

    sh = synth.SHAPES["test-tiny"]
    p0, p1 = str(tmp_path / "again.gguf"), str(tmp_path / "none.gguf")
    gguf.write_synthetic_gguf(p0, sh, seed=SEED)
    gguf.write_synthetic_gguf(p1, sh, seed=SEED, merge_lora=None)
    assert _sha(p0) == _sha(base) == _sha(p1)

    rng = np.random.default_rng(5)
    tensors = _good_tensors(rng, r_down=8)  # ranks that are powers of two: alpha / r is dyadic, the merge exact
    ad = gguf.write_lora_gguf(str(tmp_path / "ad.gguf"), tensors, alpha=2.0 ** -8)
    pm = gguf.write_synthetic_gguf(str(tmp_path / "merged.gguf"), sh, seed=SEED, merge_lora=(ad, 0.5))
    pz = gguf.write_synthetic_gguf(str(tmp_path / "zero.gguf"), sh, seed=SEED, merge_lora=(ad, 0.0))
    assert _sha(pz) == _sha(base)
    rb, rm = gguf.GGUFReader(base), gguf.GGUFReader(pm)
    assert rb.tensors.keys() == rm.tensors.keys()
    for name in rb.tensors:
        wb, wm = np.asarray(rb.tensor(name)), np.asarray(rm.tensor(name))
        if name in tensors:
            A, B = tensors[name]
            _, want = R.merge_f64(wb, A, B, 0.5 * 2.0 ** -8 / A.shape[0])
            assert np.array_equal(wm, want) and not np.array_equal(wm, wb), name
        else:
            assert np.array_equal(wm, wb), name
    # composes with dequant_from: dequantise first, then merge
    p8 = gguf.write_synthetic_gguf(str(tmp_path / "q8.gguf"), sh, seed=SEED, wtype="q8_0")
    pd = gguf.write_synthetic_gguf(str(tmp_path / "deq.gguf"), sh, seed=SEED, dequant_from=p8)
    pdm = gguf.write_synthetic_gguf(str(tmp_path / "deqm.gguf"), sh, seed=SEED, dequant_from=p8, merge_lora=(ad, 0.5))
    rd, rdm = gguf.GGUFReader(pd), gguf.GGUFReader(pdm)
    for name in tensors:
        A, B = tensors[name]
        _, want = R.merge_f64(np.asarray(rd.tensor(name)), A, B, 0.5 * 2.0 ** -8 / A.shape[0])
        assert np.array_equal(np.asarray(rdm.tensor(name)), want), name
    with pytest.raises(ValueError):
        gguf.write_synthetic_gguf(str(tmp_path / "bad.gguf"), sh, seed=SEED, wtype="q8_0", merge_lora=(ad, 0.5))


def test_llama_with_a_missing_adapter_raises_llama_cpp_pythons_error(base, tmp_path):
    from llama_p2p_amd import engine
    from llama_p2p_amd.llama import Llama

    missing = str(tmp_path / "no_such_adapter.gguf")
    with pytest.raises(RuntimeError, match="Failed to initialize LoRA adapter from lora path: ") as err:
        Llama(base, lora_path=missing, lora_scale=0.5, verbose=False)
    assert str(err.value).endswith(missing)
    assert isinstance(err.value.__cause__, engine.MxError) and err.value.__cause__.code == engine.MX_ERR_MODEL
