"""The candidate chain over more than 64 candidates on the CPU: the reference table of
sampler_wide_ref.py and its margin rule, the host sampler through sample_probe(device=-1) as the yardstick the
wide kernel is measured against, and sample_plan's routing rules.  No GPU is touched.
"""
import math

import numpy as np
import pytest

import sampler_ext_ref as R
import sampler_wide_ref as W
from llama_p2p_amd import engine as E

MAX_LEFT_OUT = 0.02  # share of the cases the margin rule may leave out


def candidate_rows():
    """(V, call, row index, rewritten row, reference result) of every non-Mirostat row of the table."""
    for V in W.VOCABS:
        for call, ref in W.table(V):
            for i, (x, res) in enumerate(ref):
                if not call["miro"][i]:
                    yield V, call, i, x, res


def test_margin_rule_leaves_out_at_most_two_percent():
    """Counted from the reference alone."""
    total = left = 0
    for V, call, i, x, res in candidate_rows():
        total += 1
        left += not W.decided(res)
    print(f"left out by the 1e-9 margins: {left}/{total}")
    assert total > 500 and left <= MAX_LEFT_OUT * total


def test_restatement_agrees_with_the_sorted_reference():
    """sampler_ext_ref.chain walks the same semantics over the sorted candidates; its tokens are the
    restatement's in every row (its own 1e-6 margins are not used here)."""
    n = wide = 0
    for V, call, i, x, res in candidate_rows():
        s = call["settings"][i]
        other = R.chain(x, s, R.samp_u01(call["seeds"][i], call["n_drawn"][i]), 0.0)
        assert other["tok"] == res["tok"], f"V={V} row {i} {s}"
        n, wide = n + 1, wide + W.is_wide(s, V)
    assert wide >= 300, f"{wide} of {n} rows have more than 64 candidates"


@pytest.mark.parametrize("V", W.VOCABS)
def test_host_sampler_is_the_reference(V):
    """The yardstick: the host sampler's tokens in every decided case, its rows bit-equal to the f32 rewrite."""
    for call, ref in W.table(V):
        tok, mu_out, rows = E.sample_probe(call["logits"], call["settings"], call["seeds"], call["n_drawn"],
                                           call["windows"], call["mu_in"], V=V, device=-1, want_logits=True)
        assert rows[:, V:].tobytes() == call["logits"][:, V:].tobytes(), "padding columns changed"
        for i, (x, res) in enumerate(ref):
            what = f"V={V} n={len(ref)} row {i} {call['settings'][i]}"
            assert rows[i, :V].tobytes() == x.tobytes(), f"{what}: rewritten row differs from the f32 restatement"
            assert 0 <= tok[i] < V
            dec = R.decided(res) if call["miro"][i] else W.decided(res)
            if dec and res["tok"] is not None:
                assert tok[i] == res["tok"], f"{what}: token {tok[i]}, reference {res['tok']} ({res['margins']})"


PEN = dict(repeat_penalty=1.1)
PLAN = [
    # the rules of mx_sample_plan, in its order
    (dict(temperature=0.0), 1000, E.MX_PICK_ARGMAX),
    (dict(temperature=0.0, top_k=0), 1000, E.MX_PICK_ARGMAX),
    (dict(temperature=-1.0, top_k=100, top_p=0.5), 1000, E.MX_PICK_ARGMAX),
    (dict(temperature=0.8, repeat_last_n=65, **PEN), 1000, E.MX_PICK_HOST),
    (dict(temperature=0.8, repeat_last_n=-1, presence_penalty=0.5), 1000, E.MX_PICK_HOST),
    (dict(temperature=0.0, repeat_last_n=65, frequency_penalty=0.5), 1000, E.MX_PICK_HOST),
    (dict(temperature=0.8, repeat_last_n=65), 1000, E.MX_PICK_CHAIN),  # no penalty: the window is never read
    (dict(temperature=0.0, top_k=0, **PEN), 1000, E.MX_PICK_CHAIN),   # greedy never reads top_k
    (dict(temperature=0.0, top_k=500, logit_bias={3: 1.0}), 1000, E.MX_PICK_CHAIN),
    (dict(temperature=0.0, top_k=0, tfs_z=0.9, **PEN), 1000, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=0, mirostat_mode=2), 1000, E.MX_PICK_MIROSTAT),
    (dict(temperature=0.8, top_k=0, mirostat_mode=2, tfs_z=0.5), 300000, E.MX_PICK_MIROSTAT),
    (dict(temperature=0.0, mirostat_mode=2), 1000, E.MX_PICK_ARGMAX),
    (dict(temperature=0.8, top_k=1), 1000, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=64), 1000, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=0), 50, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=-1), 64, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=100), 64, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=40, tfs_z=0.9, typical_p=0.5), 1000, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=0, tfs_z=0.9), 1000, E.MX_PICK_HOST),
    (dict(temperature=0.8, top_k=65, typical_p=0.5), 1000, E.MX_PICK_HOST),
    (dict(temperature=0.8, top_k=0, tfs_z=0.9), 64, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=0), 262145, E.MX_PICK_HOST),
    (dict(temperature=0.8, top_k=65), 262145, E.MX_PICK_HOST),
    (dict(temperature=0.8, top_k=64), 262145, E.MX_PICK_CHAIN),
    (dict(temperature=0.8, top_k=65), 65, E.MX_PICK_WIDE),
    (dict(temperature=0.8, top_k=65), 1000, E.MX_PICK_WIDE),
    (dict(temperature=0.8, top_k=0), 65, E.MX_PICK_WIDE),
    (dict(temperature=0.8, top_k=-1, top_p=1.0, min_p=0.0), 128256, E.MX_PICK_WIDE),
    (dict(temperature=0.8, top_k=100, repeat_last_n=64, logit_bias={3: -math.inf}, **PEN), 262144, E.MX_PICK_WIDE),
    (dict(temperature=0.8, top_k=2000), 1000, E.MX_PICK_WIDE),
]


@pytest.mark.parametrize("s,V,path", PLAN)
def test_sample_plan_rules(s, V, path):
    assert E.sample_plan(s, V) == path


@pytest.mark.parametrize("what,s,V", [
    ("mode 1", dict(mirostat_mode=1), 100),
    ("mode 3", dict(mirostat_mode=3), 100),
    ("NaN typical_p", dict(typical_p=math.nan), 100),
    ("NaN tfs_z", dict(tfs_z=math.nan), 100),
    ("NaN tau", dict(mirostat_tau=math.nan), 100),
    ("NaN eta", dict(mirostat_eta=math.nan), 100),
    ("257 entries", dict(logit_bias=(list(range(257)), [0.5] * 257)), 300),
    ("duplicate id", dict(logit_bias=([3, 5, 3], [0.5, 1.0, 2.0])), 100),
    ("id >= V", dict(logit_bias={100: 0.5}), 100),
    ("id < 0", dict(logit_bias={-1: 0.5}), 100),
    ("NaN bias", dict(logit_bias={2: math.nan}), 100),
    ("+inf bias", dict(logit_bias={2: math.inf}), 100),
    ("V = 0", dict(), 0),
])
def test_sample_plan_refuses_what_submit_refuses(what, s, V):
    with pytest.raises(E.MxError) as ei:
        E.sample_plan(dict(temperature=0.8, top_k=0, **s), V)
    assert ei.value.code == E.MX_ERR_ARG, what


def test_sample_plan_null_arguments_and_exports():
    import ctypes

    L = E.lib()
    x, _ = E.sampling_ext(E.sampling(temperature=0.8))
    path = ctypes.c_int32(-7)
    assert L.mx_sample_plan(None, 100, ctypes.byref(path)) == E.MX_ERR_ARG
    assert L.mx_sample_plan(ctypes.byref(x), 100, None) == E.MX_ERR_ARG
    assert path.value == -7
    assert L.mx_sampler_stats(None, None) == E.MX_ERR_ARG
    for name in ("mx_sample_plan", "mx_sampler_stats"):
        assert name in E.EXPORTS and hasattr(L, name)
    assert (E.MX_PICK_ARGMAX, E.MX_PICK_CHAIN, E.MX_PICK_MIROSTAT, E.MX_PICK_WIDE, E.MX_PICK_HOST) == (0, 1, 2, 3, 4)


def test_plan_agrees_with_the_table_helper():
    for V in (64, 65, 2049):
        for call, _ in W.table(V):
            for s, m in zip(call["settings"], call["miro"]):
                want = E.MX_PICK_MIROSTAT if m else E.MX_PICK_WIDE if W.is_wide(s, V) else E.MX_PICK_CHAIN
                assert E.sample_plan(s, V) == want, f"V={V} {s}"
