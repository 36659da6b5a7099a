"""How requests end (DESIGN.md §1 "How requests end"): the model emits an end-of-generation token.

Every other GPU file submits with ignore_eos, so the token compares of sched_step, sched_step_spec, the admission
path (engine.cpp) and pipeserve.Scheduler._finished ran only through a cancel.  Here the test chooses the EOS: a
small GGUF per EOS id E (gguf.write_synthetic_gguf(eos_token_id=E)), its weights those of synthetic:<shape>:seed=0.

Reference: every pool prompt (termination_ref.pool) generated alone, greedy, ignore_eos, on the synthetic engine and
teacher-forced through the CPU oracle (conftest.check_chain_batched).  A stopping request must return
ref[:ref.index(E) + 1] with FINISH_STOP when E occurs in its reference output and ref[:T] with FINISH_LENGTH
otherwise (termination_ref.expectation) -- token-exact, no tolerances: bf16 is batch-invariant (DESIGN.md §1 item
10), the sampler's draws are counter-based, and a round that ran past EOS on the device changes nothing the host
keeps.  E is a token whose first occurrence in a reference output is at the index j under test.

Models test-tiny and test-d128, bf16 unless stated, n_ctx 128, max_tokens 24.

Value-only mutations of the bookkeeping, each tried on a scratch copy (none committed), and the first test of this
file that fails (parametrised ids in brackets):
  * `&& !r->done` removed from the plain round's k loop: test_greedy_alone_stops_at_every_index[test-tiny-True-1];
  * the same removed from the speculating round's j loop:
    test_speculating_request_stops_inside_an_accepted_run[test-tiny-4-2-False];
  * the log-prob entry appended after the finish test, only while the request is live:
    test_logprob_entries_end_with_the_tokens[test-tiny-0] (moved without a condition it changes nothing: finish()
    does not read the entries);
  * the admission test pushing an EOS first token to `active`: test_greedy_alone_stops_at_every_index[test-tiny-True-0];
  * the `break` of pipeserve.Scheduler.apply_round removed: test_termination_host.py::
    test_scheduler_stops_at_the_end_of_turn_id on the CPU;
  * finish() recording `out` whole, and note_kv() without the `pos` bound: not observable one at a time --
    pos == len(prompt) + len(out) - 1 at every call (sched_step_spec checks that invariant before it speculates), so
    either bound makes the other redundant; with both bounds of finish() removed,
    test_slot_record_after_a_stop[test-tiny-bf16-False-4] fails on the reused-token count.
"""
import threading

import numpy as np
import pytest

import termination_ref as R
from conftest import check_chain_batched
from termination_ref import N_CTX, T

pytestmark = pytest.mark.gpu

GREEDY = dict(temperature=0.0)
SAMPLED = [dict(temperature=0.8),
           dict(temperature=0.8, repeat_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.2, repeat_last_n=32)]
BIG = 1 << 26


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """GGUF files by (model, wtype, eos, eot): written once, shared by every test of the module."""
    from llama_p2p_amd import gguf, synth

    root = tmp_path_factory.mktemp("termination")
    made = {}

    def path(name, eos, eot=None, wtype="bf16"):
        key = (name, wtype, eos, eot)
        if key not in made:
            p = str(root / f"{name}_{wtype}_{eos}_{eot}.gguf")
            gguf.write_synthetic_gguf(p, synth.SHAPES[name], seed=0, wtype=wtype, eos_token_id=eos, eot_token_id=eot)
            made[key] = p
        return made[key]

    path.made = made
    return path


def synthetic(name, wtype="bf16"):
    return f"synthetic:{name}:seed=0" + ("" if wtype == "bf16" else f":{wtype}")


_ref = {}


def reference(mx, oracle_mod, name):
    """(prompts, greedy ignore_eos outputs) of the pool on the synthetic engine, each run alone and teacher-forced
    through the oracle: computed once per model, shared, never modified."""
    if name not in _ref:
        from llama_p2p_amd import synth

        prompts = R.pool(name)
        eng = mx.Engine(synthetic(name), n_ctx=N_CTX, n_seq_max=2)
        outs = []
        for p in prompts:
            toks, fin = eng.generate(p, T, ignore_eos=True, **GREEDY)
            assert len(toks) == T and fin == mx.FINISH_LENGTH
            outs.append(tuple(toks))
        eng.close()
        om = oracle_mod.OracleModel(synth.SHAPES[name], seed=0)
        exact = 0
        for i, (p, o) in enumerate(zip(prompts, outs)):
            exact += check_chain_batched(om.context(N_CTX), np.array(p, np.int32), list(o), f"{name} pool {i}")[0]
        assert exact >= 0.85 * T * len(prompts)
        _ref[name] = (prompts, outs)
    return _ref[name]


_sampled = {}


def sampled_reference(mx, name, variant, wtype="bf16", n=8):
    """The first n pool prompts sampled with SAMPLED[variant], seeds 1000 + i, ignore_eos, each alone."""
    key = (name, variant, wtype)
    if key not in _sampled:
        prompts = R.pool(name)[:n]
        eng = mx.Engine(synthetic(name, wtype), n_ctx=N_CTX, n_seq_max=2)
        _sampled[key] = (prompts, [tuple(eng.generate(p, T, seed=1000 + i, ignore_eos=True, **SAMPLED[variant])[0])
                                   for i, p in enumerate(prompts)])
        eng.close()
    return _sampled[key]


def stops_of(files, name, outs, prompts, indices=R.STOP_INDICES, wtype="bf16"):
    """{j: (prompt index, E)}, preferring the E whose file exists already."""
    have = [k[2] for k in files.made if k[0] == name and k[1] == wtype and k[3] is None]
    return R.choose_stops(outs, prompts, indices, prefer=have)


def expect(mx, ref, E):
    return R.expectation(ref, E, mx.FINISH_STOP, mx.FINISH_LENGTH)


# ------------------------------------------------------------------------------- (a) plain greedy, alone
@pytest.mark.parametrize("j", R.STOP_INDICES)
@pytest.mark.parametrize("use_graphs", [True, False])
@pytest.mark.parametrize("name", R.MODELS)
def test_greedy_alone_stops_at_every_index(mx, oracle_mod, files, name, use_graphs, j):
    prompts, outs = reference(mx, oracle_mod, name)
    stops = stops_of(files, name, outs, prompts)
    assert j in stops, f"{name}: no pool prompt has a token first at index {j}"  # every j is reached: no skip
    p, E = stops[j]
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2, use_graphs=use_graphs)
    assert eng.info.eos_id == E and eng.info.eot_id == -1
    g0 = eng.stats()["generated_tokens"]
    toks, fin = eng.generate(prompts[p], T, **GREEDY)  # on a fresh slot
    print(f"{name} graphs {use_graphs} j {j}: prompt {p} ({len(prompts[p])} tokens) E {E} -> {len(toks)} tokens, "
          f"finish {fin}")
    assert (toks, fin) == (list(outs[p][:j + 1]), mx.FINISH_STOP)
    assert eng.stats()["generated_tokens"] - g0 == j + 1  # kept tokens only
    # invariance: the file's weights are the synthetic model's, and ignore_eos runs on past E
    assert eng.generate(prompts[p], T, ignore_eos=True, **GREEDY) == (list(outs[p]), mx.FINISH_LENGTH)
    # again, now over the K/V the full run left in the slot, and a prompt whose output never holds E
    assert eng.generate(prompts[p], T, **GREEDY) == (list(outs[p][:j + 1]), mx.FINISH_STOP)
    q = next(i for i, o in enumerate(outs) if E not in o)
    assert eng.generate(prompts[q], T, **GREEDY) == (list(outs[q]), mx.FINISH_LENGTH)
    eng.close()


# ----------------------------------------------------------------------------- (b) plain greedy, batched
@pytest.mark.parametrize("name", R.MODELS)
def test_greedy_batch_rows_stop_at_different_steps(mx, oracle_mod, files, name):
    """16 rows on one E (the most frequent token): rows leave the batch at many different steps and some never stop
    -- test_batch_invariance_gpu's shrinking batch, driven by EOS -- while 8 more requests wait for the slots they
    free, so rounds of one step (an admission is due) are mixed in.  Every row keeps exactly its tokens."""
    prompts, outs = reference(mx, oracle_mod, name)
    E = R.most_frequent(outs[:16])
    where = [o.index(E) if E in o else None for o in outs]
    # at least two different stop steps and a row that never stops (test-d128's 2048-token vocabulary repeats little
    # across rows; test-tiny's rows stop at four steps)
    assert None in where[:16] and len(set(where[:16])) >= 3, where
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=16)
    first = eng.submit_many(prompts[:16], T, **GREEDY)
    more = eng.submit_many(prompts[16:], T, **GREEDY)  # all 16 slots are taken: admitted as rows stop
    got = [eng.wait(r) for r in first + more]
    st = eng.stats()
    print(f"{name}: E {E} stops the rows at {where}")
    for i, (o, g) in enumerate(zip(outs, got)):
        assert g == expect(mx, o, E), f"{name} row {i} (E at {where[i]})"
    assert st["generated_tokens"] == sum(len(g[0]) for g in got)
    # the same rows with ignore_eos: nobody stops
    reqs = eng.submit_many(prompts[:16], T, ignore_eos=True, **GREEDY)
    assert [eng.wait(r) for r in reqs] == [(list(o), mx.FINISH_LENGTH) for o in outs[:16]]
    eng.close()


# ------------------------------------------------------------ (c), (d) sampling on the device / on the host
@pytest.mark.parametrize("host_sampler", [False, True])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", R.MODELS)
def test_sampled_requests_stop(mx, files, monkeypatch, name, variant, host_sampler):
    """temperature 0.8 (and, variant 1, penalties over the last 32 tokens), fixed seeds: the device chain runs K
    steps per round, the host sampler (MX_NO_DEV_TOPK, a fresh engine) one.  The reference is the same seed with
    ignore_eos: the draw of token k depends on (seed, k) only, so a stopped request is a prefix of it."""
    prompts, outs = sampled_reference(mx, name, variant)
    stops = stops_of(files, name, outs, prompts, indices=[0, 4, 8, 9])
    assert sorted(stops) == [0, 4, 8, 9], f"{name}: sampled outputs leave no candidate for some index: {stops}"
    if host_sampler:
        monkeypatch.setenv("MX_NO_DEV_TOPK", "1")
    for j, (p, E) in stops.items():
        eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2)
        kw = dict(seed=1000 + p, **SAMPLED[variant])
        g0 = eng.stats()["generated_tokens"]
        got = eng.generate(prompts[p], T, **kw)
        print(f"{name} variant {variant} host {host_sampler} j {j}: E {E} -> {len(got[0])} tokens, finish {got[1]}")
        assert got == (list(outs[p][:j + 1]), mx.FINISH_STOP), f"j {j}"
        assert eng.stats()["generated_tokens"] - g0 == j + 1
        assert eng.generate(prompts[p], T, ignore_eos=True, **kw) == (list(outs[p]), mx.FINISH_LENGTH)
        q = next(i for i, o in enumerate(outs) if E not in o)
        assert eng.generate(prompts[q], T, seed=1000 + q, **SAMPLED[variant]) == (list(outs[q]), mx.FINISH_LENGTH)
        eng.close()


# --------------------------------------------------------------------------------- (e) log-probabilities
def _with_logprobs(eng, prompt, **kw):
    req = eng.submit(prompt, T, logprobs=3, **GREEDY, **kw)
    n, done = 0, False
    while not done:
        toks, done = eng.poll(req, n)
        n = len(toks)
    lp = eng.logprobs(req)  # the entries live with the request: read before wait() releases it
    return eng.wait(req), lp


@pytest.mark.parametrize("j", [0, 4, 8])
@pytest.mark.parametrize("name", R.MODELS)
def test_logprob_entries_end_with_the_tokens(mx, oracle_mod, files, name, j):
    prompts, outs = reference(mx, oracle_mod, name)
    p, E = stops_of(files, name, outs, prompts)[j]
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2)
    (full, fin_full), lp_full = _with_logprobs(eng, prompts[p], ignore_eos=True)
    assert full == list(outs[p]) and fin_full == mx.FINISH_LENGTH and len(lp_full[0]) == T
    eng.close()
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2)  # a fresh slot, as the full run had
    (toks, fin), lp = _with_logprobs(eng, prompts[p])
    assert (toks, fin) == (list(outs[p][:j + 1]), mx.FINISH_STOP)
    n = len(toks)
    assert len(lp[0]) == n and lp[1].shape == (n, 3) and lp[2].shape == (n, 3)
    for a, b in zip(lp, lp_full):  # the same kernels on the same rows: the same bits
        assert np.array_equal(a, b[:n])
    assert lp[2][n - 1][0] == E and np.isfinite(lp[0]).all()  # greedy: EOS is the top entry of its own step
    eng.close()


# ----------------------------------------------------------------------------------- (f) speculating rounds
def repeat_prompt(seed, n_vocab):
    """test_spec_decode_gpu's prompts: BOS + a 12-token random block twice, so the lookup has something to find."""
    block = [int(t) for t in np.random.default_rng(seed).integers(3, n_vocab, 12)]
    return [1] + block + block


_plain = {}


def plain_of(mx, name, prompt):
    """The plain greedy ignore_eos output of a prompt, alone on a fresh synthetic engine: computed once, shared."""
    key = (name, tuple(prompt))
    if key not in _plain:
        eng = mx.Engine(synthetic(name), n_ctx=N_CTX, n_seq_max=2)
        _plain[key] = tuple(eng.generate(list(prompt), T, ignore_eos=True, **GREEDY)[0])
        eng.close()
    return _plain[key]


def plain_repeat(mx, name, seed):
    return plain_of(mx, name, repeat_prompt(seed, R.vocab(name)))


def inside_a_draft_run(prompt, ref, D, NG):
    """(tokens dropped, index) for the indices of `ref` that fall inside an accepted draft run -- the token there
    is an accepted draft, and the step emitted more after it: a request stopping there drops the rest of the run
    and the step's last token.  Only first occurrences can be an EOS.  Most dropped first."""
    found = []
    for m, _, a in R.replay_spec(prompt, ref, D, NG):
        found += [(m + a - i, i) for i in range(m + 1, m + a) if ref[i] not in ref[:i]]
    return sorted(found, key=lambda f: (-f[0], f[1]))


_spec_case = {}


def spec_case(mx, name, D, NG):
    """(prompt, plain output, index).  An accepted draft token is a copy from the context, so it is the first of its
    kind in the output only when the copy comes from the prompt: the prompts are a repeat prompt plus the first s
    tokens of its own plain output, which the output then goes on repeating."""
    if (name, D, NG) in _spec_case:
        return _spec_case[(name, D, NG)]
    V = R.vocab(name)
    for seed in range(100, 124):
        base = repeat_prompt(seed, V)
        ref = list(plain_of(mx, name, base))
        for s in range(0, 21):
            prompt = base + ref[:s]
            if not inside_a_draft_run(prompt, ref[s:], D, NG):  # what its output would be if no near tie flips
                continue
            out = list(plain_of(mx, name, prompt))
            idx = inside_a_draft_run(prompt, out, D, NG)
            if idx:
                _spec_case[(name, D, NG)] = (prompt, out, idx[0][1])
                return _spec_case[(name, D, NG)]
    return None


def run_spec(eng, prompt, draft, **kw):
    req = eng.submit(prompt, T, draft=draft, **GREEDY, **kw)
    n, done = 0, False
    while not done:
        toks, done = eng.poll(req, n)
        n = len(toks)
    st = eng.spec_stats(req)
    return eng.wait(req), st


@pytest.mark.parametrize("as_eot", [False, True])
@pytest.mark.parametrize("D,NG", [(4, 2), (10, 2)])
@pytest.mark.parametrize("name", R.MODELS)
def test_speculating_request_stops_inside_an_accepted_run(mx, files, name, D, NG, as_eot):
    case = spec_case(mx, name, D, NG)
    assert case is not None, f"{name} D {D}: no prompt whose output holds a first occurrence inside an accepted run"
    prompt, ref, i = case
    E = ref[i]
    # as the end-of-turn token: EOS is an id the output never holds
    path = files(name, R.absent_token([ref], R.vocab(name), avoid=prompt), E) if as_eot else files(name, E)
    eng = mx.Engine(path, n_ctx=N_CTX, n_seq_max=2)
    (toks, fin), st = run_spec(eng, prompt, (D, NG))
    hand = R.replay_spec(prompt, toks, D, NG)
    print(f"{name} D {D} eot {as_eot}: prompt of {len(prompt)} E {E} at {i}; stats {st}; by hand {hand}")
    assert (toks, fin) == (ref[:i + 1], mx.FINISH_STOP)
    # by hand from the step log: in the last step only the tokens up to EOS count
    assert st == {"steps": len(hand), "drafted": sum(d for _, d, _ in hand), "accepted": sum(a for _, _, a in hand)}
    assert hand[-1][2] >= 1, "the stopping step accepted no draft token"
    assert st["steps"] + st["accepted"] == len(toks) - 1
    # the full run accepts more: what was dropped is the rest of that run
    (full, fin_full), st_full = run_spec(eng, prompt, (D, NG), ignore_eos=True)
    assert (full, fin_full) == (ref, mx.FINISH_LENGTH) and st_full["accepted"] > st["accepted"]
    eng.close()


@pytest.mark.parametrize("name", R.MODELS)
def test_speculating_beside_a_plain_request_only_one_stops(mx, files, name):
    """A speculating and a non-speculating request in one engine (rounds run plain while both are active): the plain
    one stops at E, the speculating one -- whose output never holds E -- keeps every token and speculates once
    alone; then the other way round."""
    V = R.vocab(name)
    seeds = list(range(100, 108))
    refs = {s: list(plain_repeat(mx, name, s)) for s in seeds}
    pick = None
    for a in seeds:  # a: runs on; b: stops early
        for b in seeds:
            early = [t for k, t in enumerate(refs[b][:9]) if t not in refs[b][:k] and t not in refs[a]]
            if a != b and early and pick is None:
                pick = (a, b, early[0])
    assert pick is not None
    a, b, E = pick
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2)
    ra = eng.submit(repeat_prompt(a, V), T, draft=(4, 2), **GREEDY)
    rb = eng.submit(repeat_prompt(b, V), T, **GREEDY)
    n, done = 0, False
    while not done:
        toks, done = eng.poll(ra, n)
        n = len(toks)
    st = eng.spec_stats(ra)
    assert eng.wait(rb) == expect(mx, refs[b], E) and eng.wait(ra) == (refs[a], mx.FINISH_LENGTH)
    assert st["steps"] > 0, st  # it speculated after the plain request had gone
    # the other way round: the speculating request stops, the plain one runs on
    rb = eng.submit(repeat_prompt(b, V), T, draft=(4, 2), **GREEDY)
    ra = eng.submit(repeat_prompt(a, V), T, **GREEDY)
    assert eng.wait(rb) == expect(mx, refs[b], E) and eng.wait(ra) == (refs[a], mx.FINISH_LENGTH)
    eng.close()


# ------------------------------------------------------------------------- (g) what the slot holds afterwards
_fresh = {}


def fresh(mx, name, wtype, prompt, n):
    key = (name, wtype, tuple(prompt), n)
    if key not in _fresh:
        eng = mx.Engine(synthetic(name, wtype), n_ctx=N_CTX, n_seq_max=1)
        _fresh[key] = eng.generate(prompt, n, ignore_eos=True, **GREEDY)[0]
        eng.close()
    return _fresh[key]


def oracle_of(oracle_mod, name, wtype):
    from llama_p2p_amd import synth

    om = oracle_mod.OracleModel(synth.SHAPES[name], seed=0)
    if wtype == "q8_0":
        om.quantize_q8()
    elif wtype != "bf16":
        om.kq_synthetic(wtype, 0)
    return om


def decided_prefix(om, prompt, tokens):
    """How many leading picks of `tokens` the oracle decides: teacher-forced along them, its top-1 / top-2 gap
    exceeds the near-tie bound of conftest.check_chain_batched (twice the logit tolerance).  A decided pick must be
    the oracle's argmax whichever kernels computed the K/V it reads; past the first near tie two correct runs may
    part (a slot's K/V written by decode steps and the same K/V written by a prefill differ in their last bits)."""
    seq = np.concatenate([np.asarray(prompt, np.int32), np.asarray(tokens[:-1], np.int32)])
    lg = om.context(N_CTX).eval(seq, 0, all_logits=True)[len(prompt) - 1:]
    n = 0
    for k, t in enumerate(tokens):
        row = np.sort(lg[k])
        tol = 2 * (1e-2 * abs(float(row[-1])) + 2e-2 * float(np.abs(row).max()))
        if float(row[-1] - row[-2]) <= tol:
            break
        assert int(lg[k].argmax()) == int(t), f"step {k}: {t} is not the oracle's decided pick {int(lg[k].argmax())}"
        n += 1
    return n


def decided_tail(mx, om, name, wtype, head, avoid, n=12, need=2):
    """A 3-token tail after `head` whose fresh continuation starts with `need` decided picks: (tail, fresh tokens,
    decided).  The tail never starts with `avoid` (the token the stopped request would have fed next)."""
    for c in range(48):
        tail = [7 + 5 * c, 8 + 5 * c, 9 + 5 * c]
        tail = [t % (R.vocab(name) - 3) + 3 for t in tail]
        if tail[0] == avoid:
            continue
        want = fresh(mx, name, wtype, head + tail, n)
        d = decided_prefix(om, head + tail, want)
        if d >= need:
            return tail, want, d
    raise AssertionError(f"{name} {wtype}: no tail with {need} decided picks")


_greedy = {}


def greedy_reference(mx, name, wtype, n=8):
    """The first n pool prompts, greedy, ignore_eos, each alone on the synthetic engine of that weight type."""
    if (name, wtype) not in _greedy:
        prompts = R.pool(name)[:n]
        eng = mx.Engine(synthetic(name, wtype), n_ctx=N_CTX, n_seq_max=1)
        _greedy[(name, wtype)] = (prompts, [tuple(eng.generate(p, T, ignore_eos=True, **GREEDY)[0]) for p in prompts])
        eng.close()
    return _greedy[(name, wtype)]


def tail_of(name, *avoid):
    """Three ids that do not continue the recorded sequence by chance."""
    t = [x for x in range(7, 7 + 3 + len(avoid)) if x not in avoid]
    return t[:3]


@pytest.mark.parametrize("name,wtype,sampled,j", [
    ("test-tiny", "bf16", False, 4), ("test-tiny", "bf16", False, 8), ("test-tiny", "bf16", True, 4),
    ("test-d128", "bf16", False, 4), ("test-d128", "bf16", True, 4), ("test-d128", "bf16", False, 9),
    ("test-tiny", "q8_0", False, 4), ("test-tiny", "q4_k_m", False, 4)])
def test_slot_record_after_a_stop(mx, oracle_mod, files, name, wtype, sampled, j):
    """One slot.  A request stops at step j of a round whose later steps were already computed and written into the
    slot; the record must cover the prompt and every kept token but the last -- no more, or the next request would
    reuse K/V of tokens that were dropped (j = 8: the last step of a round, whose token was never fed back at all).
    The request that continues it reuses exactly the record and returns (1) bitwise the tokens it returns after a
    predecessor that ended at max_tokens = j + 1 instead -- the slot is in the same state -- and (2) a fresh
    engine's tokens for the same prompt up to the oracle's first near tie (decided_prefix; at least two picks)."""
    if sampled:
        prompts, outs = sampled_reference(mx, name, 0, wtype)
        kw = lambda p: dict(seed=1000 + p, **SAMPLED[0])
    else:
        prompts, outs = greedy_reference(mx, name, wtype)
        kw = lambda p: dict(GREEDY)
    stops = stops_of(files, name, outs, prompts, indices=[j], wtype=wtype)
    assert j in stops
    p, E = stops[j]
    kept = list(outs[p][:j + 1])
    tail, want, decided = decided_tail(mx, oracle_of(oracle_mod, name, wtype), name, wtype, prompts[p] + kept,
                                       outs[p][j + 1] if j + 1 < T else -1)
    longer = prompts[p] + kept + tail
    got = {}
    for how in ("eos", "max_tokens"):
        eng = mx.Engine(files(name, E, wtype=wtype), n_ctx=N_CTX, n_seq_max=1)
        st0 = eng.stats()
        if how == "eos":
            toks, fin = eng.generate(prompts[p], T, **kw(p))
            assert (toks, fin) == (kept, mx.FINISH_STOP), f"{name} {wtype}"
        else:
            toks, fin = eng.generate(prompts[p], j + 1, ignore_eos=True, **kw(p))
            assert (toks, fin) == (kept, mx.FINISH_LENGTH), f"{name} {wtype}"
        st1 = eng.stats()
        assert st1["generated_tokens"] - st0["generated_tokens"] == j + 1  # kept tokens only
        got[how], _ = eng.generate(longer, 12, ignore_eos=True, **GREEDY)
        st2 = eng.stats()
        assert st2["reused_prompt_tokens"] - st1["reused_prompt_tokens"] == len(prompts[p]) + len(kept) - 1, how
        assert st2["generated_tokens"] - st1["generated_tokens"] == 12
        eng.close()
    print(f"{name} {wtype} sampled {sampled} j {j}: E {E} tail {tail}: {decided} decided picks; "
          f"after eos {got['eos']} fresh {want}")
    assert got["eos"] == got["max_tokens"], "the slot after an EOS stop is not the slot after a max_tokens stop"
    assert got["eos"][:decided] == want[:decided], "the request over the stopped one's K/V differs from a fresh engine"


def _long_prompt_stop(mx, oracle_mod, files, name, need):
    """A pool prompt stopping mid-round (j = 4) whose record -- prompt + 4 tokens -- holds at least `need` tokens."""
    prompts, outs = reference(mx, oracle_mod, name)
    c = [(p, E) for p, E in R.candidates(outs, 4, prompts) if len(prompts[p]) + 4 >= need]
    assert c, f"{name}: no prompt of {need - 4} tokens stops at index 4"
    have = [k[2] for k in files.made if k[0] == name and k[1] == "bf16" and k[3] is None]
    p, E = next((pe for pe in c if pe[1] in have), c[0])
    return prompts[p], list(outs[p]), E


@pytest.mark.parametrize("name", R.MODELS)
def test_slot_record_after_a_stop_feeds_prefix_sharing(mx, oracle_mod, files, name):
    """Prefix sharing on, two slots: B continues the stopped request in its slot, C -- a follower in the other
    slot -- receives the record by a copy.  Both records must end at the kept position."""
    prompt, ref, E = _long_prompt_stop(mx, oracle_mod, files, name, 16)  # SHARE_MIN
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=2, prefix_sharing=True)
    toks, fin = eng.generate(prompt, T, **GREEDY)
    assert (toks, fin) == (ref[:5], mx.FINISH_STOP)
    rec = len(prompt) + len(toks) - 1
    t1 = tail_of(name, ref[5])
    B, C = prompt + toks + t1, prompt + toks + [t1[0] + 20, 5, 6, 7]
    st0, sh0 = eng.stats(), eng.sharing_stats()
    got = [eng.wait(r)[0] for r in eng.submit_many([B, C], 12, ignore_eos=True, **GREEDY)]
    st1, sh1 = eng.stats(), eng.sharing_stats()
    assert st1["reused_prompt_tokens"] - st0["reused_prompt_tokens"] == rec, (st0, st1)
    # one of them takes the slot in place, the other receives the record by one copy from the slot as it stands
    assert sh1["shared_prompt_tokens"] - sh0["shared_prompt_tokens"] == rec, (sh0, sh1)
    assert sh1["copies"] - sh0["copies"] == 1
    assert got[0] == fresh(mx, name, "bf16", B, 12) and got[1] == fresh(mx, name, "bf16", C, 12)
    eng.close()


@pytest.mark.parametrize("name", R.MODELS)
def test_slot_record_after_a_stop_spills_and_restores(mx, oracle_mod, files, name):
    """Host tier on, one slot: the stopped request's record is spilled by an unrelated request and restored for a
    request that continues it."""
    prompt, ref, E = _long_prompt_stop(mx, oracle_mod, files, name, 32)  # HOST_MIN
    eng = mx.Engine(files(name, E), n_ctx=N_CTX, n_seq_max=1, host_cache_bytes=BIG)
    toks, fin = eng.generate(prompt, T, **GREEDY)
    assert (toks, fin) == (ref[:5], mx.FINISH_STOP)
    rec = len(prompt) + len(toks) - 1
    other = [int(x) for x in np.random.default_rng(12).integers(3, R.vocab(name), 40)]
    other[0] = 7
    eng.generate(other, 4, ignore_eos=True, **GREEDY)
    h0 = eng.host_cache_stats()
    assert h0["spills"] == 1 and h0["entries"] == 1 and h0["restores"] == 0, h0
    longer = prompt + toks + tail_of(name, ref[5])
    got, _ = eng.generate(longer, 12, ignore_eos=True, **GREEDY)
    h1 = eng.host_cache_stats()
    assert h1["restores"] == 1 and h1["restored_prompt_tokens"] == rec, h1
    assert eng.stats()["reused_prompt_tokens"] == 0
    assert got == fresh(mx, name, "bf16", longer, 12), "the request fed by the restored record differs from a fresh engine"
    eng.close()


# ------------------------------------------------------------------------------------- (h) context edge
@pytest.mark.parametrize("name", R.MODELS)
def test_context_edge_lengths(mx, oracle_mod, name):
    """n_ctx 64: max_tokens = 0 means "as many as the context holds", n_ctx - n tokens, FINISH_LENGTH -- alone and
    beside two short requests whose tokens do not change; a prompt of 63 tokens gets its one token at admission."""
    from llama_p2p_amd import synth

    rng = np.random.default_rng(64)
    V = R.vocab(name)
    longs = {n: [1] + [int(t) for t in rng.integers(3, V, n - 1)] for n in (62, 61, 40, 63)}
    shorts = R.pool(name)[:2]
    assert all(len(s) + T <= 64 for s in shorts)
    eng = mx.Engine(synthetic(name), n_ctx=64, n_seq_max=4)
    om = oracle_mod.OracleModel(synth.SHAPES[name], seed=0)
    alone = [eng.generate(s, T, ignore_eos=True, **GREEDY) for s in shorts]
    assert all(len(t) == T and f == mx.FINISH_LENGTH for t, f in alone)
    for n, prompt in longs.items():
        toks, fin = eng.generate(prompt, 0, ignore_eos=True, **GREEDY)
        assert len(toks) == 64 - n and fin == mx.FINISH_LENGTH, f"{name}: prompt of {n}"
        check_chain_batched(om.context(64), np.array(prompt, np.int32), toks, f"{name} n_ctx edge {n}")
        reqs = eng.submit_many([shorts[0], prompt, shorts[1]], [T, 0, T], ignore_eos=True, **GREEDY)
        got = [eng.wait(r) for r in reqs]
        assert got[1] == (toks, mx.FINISH_LENGTH), f"{name}: prompt of {n} beside two short requests"
        assert [got[0], got[2]] == alone
    eng.close()


# ------------------------------------------------------------------------ (i) pipeline server on one GPU
def _wave(front, prompts, **kw):
    outs = [None] * len(prompts)

    def run(i):
        outs[i] = front.generate(prompts[i], T, temperature=0.0, **kw)

    th = [threading.Thread(target=run, args=(i,)) for i in range(len(prompts))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return [(list(o[0]), o[1]) for o in outs]


@pytest.mark.parametrize("as_eot", [False, True])
def test_pipeline_server_rows_stop(mx, oracle_mod, files, as_eot):
    from llama_p2p_amd import pipeserve

    name = "test-d128"
    prompts, outs = reference(mx, oracle_mod, name)
    prompts, outs = prompts[:10], outs[:10]
    E = R.most_frequent(outs)
    path = files(name, R.absent_token(outs, R.vocab(name)), E) if as_eot else files(name, E)
    llm = pipeserve.local_pipeline_llama(path, [(0, 1), (1, 2)], lanes=2, rows=4, n_ctx=N_CTX)
    front = llm._engine
    assert (llm.scheduler.eos, llm.scheduler.eot) == ((R.absent_token(outs, R.vocab(name)), E) if as_eot else (E, -1))
    ref = _wave(front, prompts, ignore_eos=True)  # the same front's own outputs (bf16 hand-off between the stages)
    assert all(len(t) == T and f == mx.FINISH_LENGTH for t, f in ref)
    where = [t.index(E) if E in t else None for t, _ in ref]
    print(f"pipeline eot {as_eot}: E {E} at {where}")
    assert None in where and sum(w is not None and w < T - 1 for w in where) >= 2, where
    for wave in range(2):  # the second wave runs to completion only if the first released its rows
        got = _wave(front, prompts)
        for i, ((r, _), g) in enumerate(zip(ref, got)):
            assert g == expect(mx, r, E), f"wave {wave} request {i} (E at {where[i]})"
        assert all(x is None for lane in llm.scheduler.table for x in lane)
    llm.close()
    assert not llm._stage_errors, llm._stage_errors


# ----------------------------------------------------------------------------------- (j) the Llama front
@pytest.mark.parametrize("j", [0, 4, 9])
def test_llama_front_reports_stop(mx, oracle_mod, files, j):
    from llama_p2p_amd.llama import Llama

    name = "test-tiny"
    prompts, outs = reference(mx, oracle_mod, name)
    p, E = stops_of(files, name, outs, prompts)[j]
    llm = Llama(model_path=files(name, E), n_ctx=N_CTX, verbose=False)
    assert llm.token_eos() == E
    out = llm.create_completion(prompts[p], max_tokens=T, temperature=0.0)
    want = llm.detokenize(list(outs[p][:j]), prev_tokens=prompts[p]).decode("utf-8", errors="ignore")
    assert out["choices"][0]["finish_reason"] == "stop" and out["choices"][0]["text"] == want
    assert out["usage"]["completion_tokens"] == j and out["usage"]["prompt_tokens"] == len(prompts[p])
    chunks = list(llm.create_completion(prompts[p], max_tokens=T, temperature=0.0, stream=True))
    assert "".join(c["choices"][0]["text"] for c in chunks) == want
    assert chunks[-1]["choices"][0]["finish_reason"] == "stop"
    assert all(c["choices"][0]["finish_reason"] is None for c in chunks[:-1])
    llm.close()


# ------------------------------------------------------------------------------------- end-of-turn token
@pytest.mark.parametrize("j", [0, 4, 8])
@pytest.mark.parametrize("name", R.MODELS)
def test_end_of_turn_token_ends_a_request(mx, oracle_mod, files, name, j):
    """tokenizer.ggml.eot_token_id = E and an EOS id no output holds (a Llama-3-Instruct-style file): a request stops
    at E at admission (j = 0) and in a round; ignore_eos runs on; a file without the key behaves as ever."""
    prompts, outs = reference(mx, oracle_mod, name)
    p, E = stops_of(files, name, outs, prompts)[j]
    A = R.absent_token(outs, R.vocab(name))
    eng = mx.Engine(files(name, A, E), n_ctx=N_CTX, n_seq_max=4)
    assert eng.info.eos_id == A and eng.info.eot_id == E
    assert eng.generate(prompts[p], T, **GREEDY) == (list(outs[p][:j + 1]), mx.FINISH_STOP)
    assert eng.generate(prompts[p], T, ignore_eos=True, **GREEDY) == (list(outs[p]), mx.FINISH_LENGTH)
    got = [eng.wait(r) for r in eng.submit_many(prompts[:4], T, **GREEDY)]
    assert got == [expect(mx, o, E) for o in outs[:4]]
    eng.close()
    eng = mx.Engine(files(name, A), n_ctx=N_CTX, n_seq_max=2)  # no eot key: nothing ends this request early
    assert eng.info.eos_id == A and eng.info.eot_id == -1
    assert eng.generate(prompts[p], T, **GREEDY) == (list(outs[p]), mx.FINISH_LENGTH)
    eng.close()
