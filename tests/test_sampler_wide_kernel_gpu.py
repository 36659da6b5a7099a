"""The wide sampler kernel alone (the candidate chain over more than 64 candidates, up to the whole
vocabulary) through sample_probe(device=0): the mixed table of sampler_wide_ref.py, crafted rows at the smallest
shapes at which the kernel can go wrong, and the independence of a row from its launch.

Wide rows are compared with the float64 numpy restatement under its 1e-9 margins; rows of at most 64 candidates
run the per-row chain and must equal the host sampler bit for bit; Mirostat rows are checked as
test_sampler_ext_kernel_gpu.py checks them.
"""
import numpy as np
import pytest

import sampler_ext_ref as R
import sampler_wide_ref as W
from llama_p2p_amd import engine as E

pytestmark = pytest.mark.gpu


def probe(call, device, rows=None):
    sel = list(range(len(call["settings"]))) if rows is None else rows
    return E.sample_probe(call["logits"][sel], [call["settings"][i] for i in sel], [call["seeds"][i] for i in sel],
                          [call["n_drawn"][i] for i in sel], [call["windows"][i] for i in sel],
                          call["mu_in"][sel], V=call["V"], device=device, want_logits=True)


@pytest.mark.parametrize("V", W.VOCABS)
def test_mixed_table_vs_reference_and_host_sampler(V):
    wide = left = 0
    for call, ref in W.table(V):
        n = len(ref)
        tok_d, mu_d, rows_d = probe(call, 0)
        tok_h, mu_h, rows_h = probe(call, -1)
        assert rows_d.tobytes() == rows_h.tobytes(), "rewritten rows (or their padding) differ from the host sampler's"
        assert rows_d[:, V:].tobytes() == call["logits"][:, V:].tobytes(), "padding columns changed"
        for i, (x, res) in enumerate(ref):
            s = call["settings"][i]
            what = f"V={V} n={n} row {i} {dict(s, logit_bias=len(s.get('logit_bias') or {}))}"
            assert 0 <= tok_d[i] < V, f"{what}: token {tok_d[i]} outside the vocabulary"
            if call["miro"][i]:
                if R.decided(res):
                    if res["tok"] is not None:
                        assert tok_d[i] == res["tok"], f"{what}: token {tok_d[i]}, reference {res['tok']}"
                    tol = R.mu_tol(s, float(call["mu_in"][i]))
                    assert abs(float(mu_d[i]) - res["mu_out"]) <= tol, f"{what}: mu_out {mu_d[i]} vs {res['mu_out']}"
                continue
            assert mu_d[i:i + 1].tobytes() == call["mu_in"][i:i + 1].tobytes(), f"{what}: mu written"
            if not W.is_wide(s, V):
                assert tok_d[i] == tok_h[i], f"{what}: narrow row, device {tok_d[i]} host sampler {tok_h[i]}"
                continue
            wide += 1
            if not W.decided(res):
                left += 1
            elif res["tok"] is not None:
                assert tok_d[i] == res["tok"], f"{what}: token {tok_d[i]}, reference {res['tok']} ({res['margins']})"
    print(f"V={V}: {wide} wide cases, {left} left out by the margin rule")
    assert wide > 0 or V <= 64


def crafted(row, n_seeds=64, **s):
    """One row under 64 seeds in one call -> (tokens, [reference result per seed])."""
    row = np.asarray(row, dtype=np.float32)
    s = dict(dict(temperature=1.0, top_p=1.0, min_p=0.0), **s)
    seeds = [1000003 * (j + 1) for j in range(n_seeds)]
    drawn = [j % 7 for j in range(n_seeds)]
    tok, _ = E.sample_probe(np.tile(row, (n_seeds, 1)), [s] * n_seeds, seeds, drawn, device=0)
    refs = [W.chain(row, s, R.samp_u01(seeds[j], drawn[j])) for j in range(n_seeds)]
    assert all(0 <= t < len(row) for t in tok)
    for j, res in enumerate(refs):
        if W.decided(res) and res["tok"] is not None:
            assert tok[j] == res["tok"], f"seed {j}: token {tok[j]}, reference {res['tok']} ({res['margins']})"
    return tok.tolist(), refs


def test_all_equal_values_cut_by_id():
    tok, _ = crafted(np.full(130, 0.25), top_k=65)
    assert max(tok) < 65 and len(set(tok)) > 20


def test_signed_zeros_are_one_value():
    row = np.zeros(140, dtype=np.float32)
    row[1::2] = -0.0
    tok, _ = crafted(row, top_k=70)
    assert max(tok) < 70 and {t % 2 for t in tok} == {0, 1}


def _five_ones():
    row = np.zeros(8192, dtype=np.float32)
    row[[5, 2047, 2048, 4096, 8191]] = 1.0
    return row


@pytest.mark.parametrize("top_p", [1.0, 0.5])
def test_boundary_group_spans_slices(top_p):
    """top_k = 66 of five ones over zeros: the ones and ids 0..61 minus none of them (61 zeros: 0..61 without 5)."""
    tok, refs = crafted(_five_ones(), top_k=66, top_p=top_p)
    allowed = {5, 2047, 2048, 4096, 8191} | (set(range(62)) - {5})
    assert set(tok) <= allowed


def test_one_hot_row_under_top_p():
    row = np.full(500, -50.0, dtype=np.float32)
    row[321] = 50.0
    tok, _ = crafted(row, top_k=0, top_p=0.9)
    assert set(tok) == {321}


def test_only_the_finite_tokens_of_a_banned_row():
    row = np.full(300, -np.inf, dtype=np.float32)
    row[[7, 150, 299]] = [0.5, 1.0, 0.0]
    tok, _ = crafted(row, top_k=100)
    assert set(tok) == {7, 150, 299}


def test_row_of_minus_inf_returns_a_token():
    tok, _ = crafted(np.full(300, -np.inf), n_seeds=3, top_k=0)
    assert all(0 <= t < 300 for t in tok)


@pytest.mark.parametrize("temp", [0.05, 5.0])
def test_temperatures(temp):
    row = np.random.default_rng(4097).normal(size=4097).astype(np.float32)
    tok, refs = crafted(row, top_k=0, top_p=0.95, min_p=0.02, temperature=temp)
    assert sum(W.decided(r) for r in refs) >= 60  # from the reference alone


def test_largest_vocabulary():
    V = 262144
    row = np.random.default_rng(262144).normal(size=V).astype(np.float32)
    s = dict(temperature=1.0, top_k=0, top_p=0.95, min_p=0.0)
    tok, _ = E.sample_probe(row[None], [s], [77], [3], device=0)
    res = W.chain(row, s, R.samp_u01(77, 3))
    assert W.decided(res) and tok[0] == res["tok"]


def test_vocabulary_past_the_slice_limit_is_refused():
    V = 262145
    with pytest.raises(E.MxError) as ei:
        E.sample_probe(np.zeros((1, V), dtype=np.float32), [dict(temperature=1.0, top_k=0)], [1], [0], device=0)
    assert ei.value.code == E.MX_ERR_ARG
    tok, mu = ei.value.outputs
    assert set(tok.tobytes()) == {0xFF} and set(mu.tobytes()) == {0xFF}


@pytest.mark.parametrize("V", [65, 2049, 128256])
def test_row_does_not_depend_on_its_launch(V):
    call = W.table(V)[0][0]  # the 64-row call
    tok, mu, rows = probe(call, 0)
    for i in (0, 31, 63):
        t1, m1, r1 = probe(call, 0, rows=[i])
        assert t1[0] == tok[i], f"row {i} alone vs in the 64-row call"
    i = next(i for i in range(64) if W.is_wide(call["settings"][i], V))
    t2, _, _ = probe(call, 0, rows=[i, 5, i])
    assert t2[0] == t2[2] == tok[i], "two copies of one row in a call"
    again, _, _ = probe(call, 0)
    assert again.tolist() == tok.tolist(), "two identical calls"
