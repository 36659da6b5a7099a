"""The load-time LoRA merge kernel alone (csrc/lora.hip through mx_lora_merge_probe) against the
float64 reference of tests/lora_ref.py: bit for bit on dyadic inputs, where every f32 evaluation order gives the
same bits (checked on the CPU in tests/test_lora_host.py), and inside the derived f32 error interval on real-valued
ones."""
import numpy as np
import pytest

import lora_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def _guard_intact(guard):
    return guard.size == 4096 and (guard == 0xFFFF).all()


@pytest.mark.parametrize("rows,cols,r", R.KERNEL_SHAPES)
def test_dyadic_inputs_bit_for_bit(E, rows, cols, r):
    w, A, B, scale = R.dyadic_case(rows, cols, r, seed=100 + r)
    _, want = R.merge_f64(w, A, B, scale)
    out, guard, us = E.lora_merge_probe(w, A, B, scale)
    assert us is None and _guard_intact(guard)
    bad = np.argwhere(out != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first at {bad[0].tolist()}"
    assert (out != w).mean() > 0.5


@pytest.mark.parametrize("rows,cols,r", R.KERNEL_SHAPES)
def test_real_inputs_inside_the_f32_interval(E, rows, cols, r):
    w, A, B, scale = R.real_case(rows, cols, r, seed=200 + r)
    lo, hi, _ = R.merge_interval(w, A, B, scale, r)
    ambiguous = float((lo != hi).mean())
    assert ambiguous <= 0.01, f"the rule leaves {ambiguous:.2%} of the elements a choice: a slack test"
    out, guard, _ = E.lora_merge_probe(w, A, B, scale)
    assert _guard_intact(guard)
    got, lo_v, hi_v = R.bf16_to_f64(out), R.bf16_to_f64(lo), R.bf16_to_f64(hi)
    bad = np.argwhere((got < lo_v) | (got > hi_v))
    print(f"({rows}, {cols}, {r}): {ambiguous:.3%} ambiguous, {len(bad)} outside")
    assert bad.size == 0, f"{len(bad)} elements outside their interval, first at {bad[0].tolist()}"
    assert (out != w).mean() > 0.5


@pytest.mark.parametrize("rows,cols,r", [(5, 13, 2), (70, 257, 17)])
def test_rows_not_on_16_byte_boundaries(E, rows, cols, r):
    """cols % 8 != 0: the element-wise form of the kernel (no model matrix has such a width; the probe reaches it)."""
    w, A, B, scale = R.dyadic_case(rows, cols, r, seed=300 + r)
    _, want = R.merge_f64(w, A, B, scale)
    out, guard, _ = E.lora_merge_probe(w, A, B, scale)
    assert _guard_intact(guard) and np.array_equal(out, want)


def test_timing_leaves_the_first_result(E):
    w, A, B, scale = R.dyadic_case(128, 256, 16, seed=7)
    _, want = R.merge_f64(w, A, B, scale)
    out, guard, us = E.lora_merge_probe(w, A, B, scale, iters=3)
    assert np.array_equal(out, want) and _guard_intact(guard) and us is not None and us > 0


@pytest.mark.parametrize("kw", [dict(rows=0), dict(cols=0), dict(r=0), dict(rows=-1), dict(rows=65537), dict(r=4097), dict(scale=float("nan")),
                                dict(scale=float("inf")), dict(iters=-1)])
def test_invalid_arguments_launch_nothing(E, kw):
    w, A, B, scale = R.dyadic_case(16, 32, 2, seed=1)
    out = np.full(16 * 32 + E.LORA_GUARD, 0xFFFF, np.uint16)
    args = dict(scale=scale, iters=0, out=out)
    args.update(kw)
    with pytest.raises(E.MxError) as err:
        E.lora_merge_probe(w, A, B, **args)
    assert err.value.code == E.MX_ERR_ARG and "mx_lora_merge_probe" in str(err.value)
    assert (out == 0xFFFF).all()


def test_null_pointers_launch_nothing(E):
    import ctypes

    w, A, B, scale = R.dyadic_case(16, 32, 2, seed=1)
    out = np.full(16 * 32 + E.LORA_GUARD, 0xFFFF, np.uint16)
    us = ctypes.c_double()
    ptrs = [w.ctypes.data, A.ctypes.data, B.ctypes.data, out.ctypes.data]
    for i in range(4):
        p = list(ptrs)
        p[i] = None
        rc = E.lib().mx_lora_merge_probe(0, 16, 32, 2, p[0], p[1], p[2], scale, p[3], 0, ctypes.byref(us))
        assert rc == E.MX_ERR_ARG
    assert E.lib().mx_lora_merge_probe(0, 16, 32, 2, *ptrs[:3], scale, ptrs[3], 2, None) == E.MX_ERR_ARG
    # more elements than a probe may allocate
    assert E.lib().mx_lora_merge_probe(0, 65536, 65536, 2, *ptrs[:3], scale, ptrs[3], 0, None) == E.MX_ERR_ARG
    assert (out == 0xFFFF).all()
