"""The extended sampler chain (typical_p, tfs_z, logit_bias, Mirostat v2) on the CPU: the host
sampler through sample_probe(device=-1) against the float64 numpy restatement of sampler_ext_ref.py, the refusals
of the C ABI, and Llama.create_completion's new keywords over a canned engine.  No GPU is touched.
"""
import ctypes
import math

import numpy as np
import pytest

import sampler_ext_ref as R
from llama_p2p_amd import engine as E
from llama_p2p_amd.llama import Llama

MAX_LEFT_OUT = 0.02  # share of the cases the margin rule may leave out


def check_call(call, device):
    """One probe call against the reference: tokens equal wherever the reference is decided, rows bit-equal to
    the f32 rewrite, padding untouched, mu_out within its tolerance.  Returns (cases, left out)."""
    ref = R.reference(call)
    tok, mu_out, rows = E.sample_probe(call["logits"], call["settings"], call["seeds"], call["n_drawn"],
                                       call["windows"], call["mu_in"], V=call["V"], device=device, want_logits=True)
    V, left = call["V"], 0
    assert rows[:, V:].tobytes() == call["logits"][:, V:].tobytes(), "padding columns changed"
    for i, (x, res) in enumerate(ref):
        what = f"V={V} n={len(ref)} row {i} {call['settings'][i]}"
        assert rows[i, :V].tobytes() == x.tobytes(), f"{what}: rewritten row differs from the f32 restatement"
        assert 0 <= tok[i] < V, f"{what}: token {tok[i]} outside the vocabulary"
        if not R.decided(res):
            left += 1
            continue
        if res["tok"] is not None:
            assert tok[i] == res["tok"], f"{what}: token {tok[i]}, reference {res['tok']} (margins {res['margins']})"
        tol = R.mu_tol(call["settings"][i], float(call["mu_in"][i]))
        assert abs(float(mu_out[i]) - res["mu_out"]) <= tol, f"{what}: mu_out {mu_out[i]} vs {res['mu_out']}"
    return len(ref), left


@pytest.mark.parametrize("V", R.VOCABS)
def test_host_sampler_vs_numpy_reference(V):
    total = left = 0
    for n in R.ROW_COUNTS:
        t, l = check_call(R.make_call(V, n), device=-1)
        total, left = total + t, left + l
    print(f"V={V}: {total} cases, {left} left out by the margin rule")


def test_margin_rule_leaves_out_at_most_two_percent():
    """Counted from the reference alone, over the whole table (both the candidate chain and Mirostat)."""
    total = {False: 0, True: 0}
    left = {False: 0, True: 0}
    for V in R.VOCABS:
        for n in R.ROW_COUNTS:
            call = R.make_call(V, n)
            for (x, res), m in zip(R.reference(call), call["miro"]):
                total[bool(m)] += 1
                left[bool(m)] += not R.decided(res)
    print(f"left out: candidate chain {left[False]}/{total[False]}, Mirostat {left[True]}/{total[True]}")
    for m in (False, True):
        assert left[m] <= MAX_LEFT_OUT * total[m]


def test_table_covers_the_grid():
    seen_c, seen_m, kinds = set(), set(), set()
    for V in R.VOCABS:
        for n in R.ROW_COUNTS:
            call = R.make_call(V, n)
            for s, mu in zip(call["settings"], call["mu_in"]):
                if s.get("mirostat_mode") == 2:
                    seen_m.add((s["mirostat_tau"], s["mirostat_eta"], float(mu)))
                else:
                    seen_c.add((s["typical_p"], s["tfs_z"], s["top_k"], s["top_p"]))
                kinds.add(len(s.get("logit_bias") or {}) if "logit_bias" in s else 0)
    assert len(seen_c) == len(R.CAND) and len(seen_m) == len(R.MIRO)
    assert {0, 1, 256} <= kinds


def test_whole_vocabulary_candidates_on_the_host():
    """top_k = 0 (every token a candidate) is the host sampler's alone: the cuts run over thousands of candidates
    and the typical order comes from a stable sort of the library."""
    call = R.make_call(2049, 64, salt=1)
    for s, m in zip(call["settings"], call["miro"]):
        if not m:
            s["top_k"] = 0
    total, left = check_call(call, device=-1)
    assert left <= MAX_LEFT_OUT * total  # one of the 64, counted from the reference alone


def test_every_candidate_banned_still_returns_a_token():
    V = 300
    lg = np.random.default_rng(5).normal(size=(2, V)).astype(np.float32)
    ban = {t: -math.inf for t in range(256)}
    lg[:, 256:] = -np.inf
    sets = [dict(temperature=0.9, typical_p=0.5, tfs_z=0.9, logit_bias=ban),
            dict(temperature=1.0, mirostat_mode=2, logit_bias=ban)]
    tok, mu = E.sample_probe(lg, sets, [1, 2], [0, 0], device=-1)
    assert all(0 <= t < V for t in tok) and np.isfinite(mu).all()


def _probe_raw(n=1, V=8, ldl=8, **ext):
    """mx_sample_probe with one hand-built mx_sampling_ext per row; returns (rc, tok bytes, mu bytes)."""
    L = E.lib()
    arr = (E.MxSamplingExt * n)()
    keep = []
    for i in range(n):
        e = dict(ext)
        bias = e.pop("bias", None)
        keep.append(E.sampling_ext(E.sampling(temperature=1.0), into=arr[i], logit_bias=bias, **e)[1])
    lg = np.zeros((n, ldl), dtype=np.float32)
    seeds = np.ones(n, dtype=np.uint64)
    z = np.zeros(n, dtype=np.int32)
    win = np.zeros((n, 64), dtype=np.int32)
    mu = np.zeros(n, dtype=np.float32)
    tok = np.zeros(n, dtype=np.int32)
    mu_out = np.zeros(n, dtype=np.float32)
    rc = L.mx_sample_probe(-1, lg.ctypes.data, n, V, ldl, arr, seeds.ctypes.data, z.ctypes.data, win.ctypes.data,
                           z.ctypes.data, mu.ctypes.data, tok.ctypes.data, mu_out.ctypes.data, None)
    return rc, tok.tobytes(), mu_out.tobytes()


@pytest.mark.parametrize("what,kw", [
    ("mode 1", dict(mirostat_mode=1)),
    ("mode 3", dict(mirostat_mode=3)),
    ("257 entries", dict(V=300, ldl=300, bias=(list(range(257)), [0.5] * 257))),
    ("duplicate id", dict(bias=([3, 5, 3], [0.5, 1.0, 2.0]))),
    ("id >= V", dict(bias=([8], [0.5]))),
    ("NaN bias", dict(bias=([2], [math.nan]))),
    ("+inf bias", dict(bias=([2], [math.inf]))),
    ("n = 65", dict(n=65)),
    ("V > ldl", dict(V=9, ldl=8)),
])
def test_probe_refusals_leave_the_outputs_untouched(what, kw):
    rc, tok, mu = _probe_raw(**kw)
    assert rc == E.MX_ERR_ARG, what
    assert set(tok) == {0xFF} and set(mu) == {0xFF}, f"{what}: outputs written"


def test_minus_inf_bias_is_accepted():
    rc, tok, mu = _probe_raw(bias=([2], [-math.inf]))
    assert rc == E.MX_OK and set(tok) != {0xFF}


def test_exports_and_defaults():
    for name in ("mx_sampling_ext_default", "mx_submit_ext", "mx_sample_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
    s = E.MxSamplingExt()
    ctypes.memset(ctypes.byref(s), 0xFF, ctypes.sizeof(s))
    E.lib().mx_sampling_ext_default(ctypes.byref(s))
    assert (s.typical_p, s.tfs_z, s.mirostat_mode, s.mirostat_tau, s.n_logit_bias) == (1.0, 1.0, 0, 5.0, 0)
    assert s.mirostat_eta == np.float32(0.1) and not s.bias_tok and not s.bias_val
    base = E.MxSampling()
    E.lib().mx_sampling_default(ctypes.byref(base))
    assert all(getattr(s.base, f) == getattr(base, f) for f, _ in E.MxSampling._fields_)
    assert E.Engine.supports_sampler_ext is True


# ---- Llama over a canned engine ---------------------------------------------------------------------------------
class Canned:
    supports_sampler_ext = True

    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd, self.submits = n_vocab, 64, []

    def submit(self, ids, max_tokens, **kw):
        self.submits.append(kw)
        return 1

    def poll(self, r, n_have=0):
        return [5, 6], True

    def wait(self, r, cap=None):
        return [5, 6], E.FINISH_LENGTH

    def cancel(self, r):
        pass


class CannedOld(Canned):
    """A front from before the extended chain: no keyword of it, no supports_sampler_ext."""
    supports_sampler_ext = False

    def submit(self, ids, max_tokens, temperature=0.0, top_k=40, top_p=0.95, min_p=0.05, repeat_penalty=1.0,
               frequency_penalty=0.0, presence_penalty=0.0, seed=None):
        self.submits.append({})
        return 1


NEW = ("typical_p", "tfs_z", "mirostat_mode", "mirostat_tau", "mirostat_eta", "logit_bias")


def llama(cls=Canned):
    eng = cls()
    return Llama.from_engine("synthetic:test-tiny:seed=0", eng, n_ctx=128), eng


def test_defaults_send_none_of_the_new_keywords():
    for cls in (Canned, CannedOld):
        llm, eng = llama(cls)
        out = llm.create_completion([1, 2, 3], max_tokens=2)
        assert out["usage"]["completion_tokens"] == 2
        assert not set(eng.submits[0]) & set(NEW)
    llm, eng = llama()
    llm.create_completion([1, 2, 3], max_tokens=2, typical_p=1.0, tfs_z=1.0, mirostat_mode=0, mirostat_tau=5.0,
                          mirostat_eta=0.1, logit_bias=None)
    assert not set(eng.submits[0]) & set(NEW)


@pytest.mark.parametrize("kw,sent", [
    (dict(typical_p=0.5), dict(typical_p=0.5)),
    (dict(tfs_z=0.9), dict(tfs_z=0.9)),
    (dict(mirostat_mode=2), dict(mirostat_mode=2)),
    (dict(mirostat_mode=2, mirostat_tau=3.0, mirostat_eta=0.2), dict(mirostat_mode=2, mirostat_tau=3.0, mirostat_eta=0.2)),
    (dict(logit_bias={7: -math.inf, 9: 2.0}), dict(logit_bias={7: -math.inf, 9: 2.0})),
])
def test_non_default_keywords_reach_submit(kw, sent):
    llm, eng = llama()
    llm.create_completion([1, 2, 3], max_tokens=2, **kw)  # typical_p=0.5 among them: it raised before
    got = {k: v for k, v in eng.submits[0].items() if k in NEW}
    assert got == sent


def test_create_completion_signature_follows_llama_cpp_python():
    import inspect

    p = inspect.signature(Llama.create_completion).parameters
    names = list(p)
    i = names.index("seed")
    assert names[i + 1:i + 6] == ["tfs_z", "mirostat_mode", "mirostat_tau", "mirostat_eta", "logit_bias"]
    assert [p[n].default for n in names[i + 1:i + 6]] == [1.0, 0, 5.0, 0.1, None]


def test_refused_settings():
    llm, eng = llama()
    with pytest.raises(NotImplementedError):
        llm.create_completion([1, 2], max_tokens=2, mirostat_mode=1)
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, mirostat_mode=3)
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, logit_bias={t: 1.0 for t in range(257)})
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, logit_bias={512: 1.0})
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, logit_bias={-1: 1.0})
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, logit_bias={3: math.nan})
    with pytest.raises(ValueError):
        llm.create_completion([1, 2], max_tokens=2, logit_bias={3: math.inf})
    for name in ("typical_p", "tfs_z", "mirostat_tau", "mirostat_eta"):
        with pytest.raises(ValueError):
            llm.create_completion([1, 2], max_tokens=2, **{name: math.nan})
    assert eng.submits == []


@pytest.mark.parametrize("kw", [dict(typical_p=0.5), dict(tfs_z=0.9), dict(mirostat_mode=2), dict(logit_bias={3: 1.0})])
def test_front_without_the_extended_chain_refuses(kw):
    llm, eng = llama(CannedOld)
    with pytest.raises(NotImplementedError):
        llm.create_completion([1, 2], max_tokens=2, **kw)
    assert eng.submits == []
