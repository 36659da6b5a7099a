"""The extended sampler chain's kernels alone (bias_kernel -> penalty_kernel -> top-k -> sample_ext_kernel, and
the Mirostat v2 kernels) through sample_probe(device=0), on the case table of sampler_ext_ref.py.

Candidate-chain rows (tail-free, typical, bias, penalties) run samp_pick, the host sampler's own code: their
tokens and rewritten rows must equal the host sampler's (device=-1) in every case, bit for bit.  Mirostat rows
are compared with the float64 numpy reference under its margin rule.  A row's result does not depend on the
rows it shares a launch with.
"""
import numpy as np
import pytest

import sampler_ext_ref as R
from llama_p2p_amd import engine as E

pytestmark = pytest.mark.gpu


def probe(call, device, rows=None):
    sel = list(range(len(call["settings"]))) if rows is None else rows
    return E.sample_probe(call["logits"][sel], [call["settings"][i] for i in sel], [call["seeds"][i] for i in sel],
                          [call["n_drawn"][i] for i in sel], [call["windows"][i] for i in sel],
                          call["mu_in"][sel], V=call["V"], device=device, want_logits=True)


@pytest.mark.parametrize("V", R.VOCABS)
def test_device_chain_vs_host_sampler_and_reference(V):
    total = left = 0
    for n in R.ROW_COUNTS:
        call = R.make_call(V, n)
        tok_d, mu_d, rows_d = probe(call, 0)
        tok_h, mu_h, rows_h = probe(call, -1)
        assert rows_d.tobytes() == rows_h.tobytes(), "rewritten rows (or their padding) differ from the host sampler's"
        assert rows_d[:, V:].tobytes() == call["logits"][:, V:].tobytes(), "padding columns changed"
        miro = call["miro"]
        cand = np.flatnonzero(~miro)
        assert tok_d[cand].tolist() == tok_h[cand].tolist(), "candidate chain: device and host sampler disagree"
        assert mu_d[cand].tobytes() == call["mu_in"][cand].tobytes()
        ref = R.reference(call)
        for i in np.flatnonzero(miro):
            res = ref[i][1]
            total += 1
            assert 0 <= tok_d[i] < V
            if not R.decided(res):
                left += 1
                continue
            what = f"V={V} n={n} row {i} {call['settings'][i]} mu_in {call['mu_in'][i]}"
            if res["tok"] is not None:
                assert tok_d[i] == res["tok"], f"{what}: token {tok_d[i]}, reference {res['tok']}"
            tol = R.mu_tol(call["settings"][i], float(call["mu_in"][i]))
            assert abs(float(mu_d[i]) - res["mu_out"]) <= tol, f"{what}: mu_out {mu_d[i]} vs {res['mu_out']}"
    # which cases are left out depends on the reference alone: the 2 % cap over this very table is asserted by
    # test_sampler_ext_host.py::test_margin_rule_leaves_out_at_most_two_percent
    print(f"V={V}: {total} Mirostat cases, {left} left out by the margin rule")


@pytest.mark.parametrize("V", [65, 2049, 128256])
def test_row_does_not_depend_on_its_batch_mates(V):
    call = R.make_call(V, 64)
    tok, mu, rows = probe(call, 0)
    for i in (0, 31, 63, 2, 32, 62):  # candidate-chain and Mirostat rows (every third row is a Mirostat one)
        t1, m1, r1 = probe(call, 0, rows=[i])
        assert t1[0] == tok[i] and m1.tobytes() == mu[i:i + 1].tobytes(), f"row {i} alone vs in the 64-row call"
        assert r1.tobytes() == rows[i:i + 1].tobytes()
