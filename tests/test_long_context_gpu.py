"""Long-context decode in the engine: forwards that hold a row past the split threshold T take
launch_attention_split + attn_merge_kernel, short forwards what they always took.  Tiny synthetic models, n_ctx a
little above T, against the CPU oracle with the tolerance of tests/test_engine_gpu.py's n_ctx = 2048 case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_logits_close, assert_tokens_match, check_chain_batched, logit_tol

pytestmark = pytest.mark.gpu
NAME = "test-d128"
QUANTS = pytest.mark.parametrize("quant", ["", ":q8_0"], ids=["bf16", "q8_0"])


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


@pytest.fixture(scope="module")
def T(mx):
    return mx.attention_split_plan(1)["threshold"]


def seq(n, seed=123):
    from llama_p2p_amd import synth

    rng = np.random.default_rng(seed)
    return np.concatenate([[1], rng.integers(3, synth.SHAPES[NAME].n_vocab, n - 1)]).astype(np.int32)


def oracle(oracle_mod, quant):
    from llama_p2p_amd import synth

    om = oracle_mod.OracleModel(synth.SHAPES[NAME], seed=0)
    if quant:
        om.quantize_q8()
    return om


@QUANTS
def test_decode_across_the_threshold(mx, oracle_mod, T, quant):
    """A prompt of T - 6 tokens, then 16 decode steps: teacher-forced one-token forwards (each long from the step
    whose context passes T) against the oracle's logits, and 16 greedy steps of one captured decode batch against
    the oracle's greedy chain."""
    P = T - 6
    ids = seq(P + 16)
    eng = mx.Engine(f"synthetic:{NAME}:seed=0{quant}", n_ctx=T + 64, n_seq_max=4)
    octx = oracle(oracle_mod, quant).context(T + 64)
    ref = octx.eval(ids, 0, all_logits=True)[P - 1:]
    for slot in (0, 1):
        assert eng.forward_rows([slot] * (P - 1), list(range(P - 1)), ids[:P - 1], want_logits=False) is None
    got = np.stack([eng.forward_logits(ids[p:p + 1], p, slot=0)[0] for p in range(P - 1, P + 16)])
    print(f"long decode{quant}: max |d| {np.abs(got - ref).max():.4g} of max|ref| {np.abs(ref).max():.4g}")
    assert_logits_close(got, ref, f"decode across T{quant}")
    assert_tokens_match(got, ref, f"decode across T{quant}")
    b = eng.batch(slots=[1], pos=[P - 1], ids=[int(ids[P - 1])], max_steps=16)
    for _ in range(16):
        b.step()
    check_chain_batched(octx, ids[:P], b.tokens()[0], f"greedy batch across T{quant}")
    b.close()
    eng.close()


def finish(eng, req):
    """-> (tokens, per-token log-probabilities, top-4 log-probabilities) of a logprobs= request, once it is done."""
    n, done = 0, False
    while not done:
        got, done = eng.poll(req, n)
        n = len(got)
    tok_lp, top_lp, _ = eng.logprobs(req)
    return eng.wait(req)[0], tok_lp.copy(), top_lp.copy()


def test_scheduler_rounds_across_the_threshold(mx, oracle_mod, T):
    """submit / wait from context T - 6, 16 greedy tokens: the scheduler replays one captured step up to 8 times a
    round, so the row passes T inside a round and the round must be long from its first step (max pos + K).  Every
    step's log-probabilities (the values the scheduler exposes per step) against the oracle's log-softmax, within twice
    the logit tolerance (log-softmax moves by at most twice the largest logit error); and bitwise equal to the same
    request decoded beside three short ones, whose rounds mix long and short rows."""
    P = T - 6
    ids = seq(P, seed=7)
    eng = mx.Engine(f"synthetic:{NAME}:seed=0", n_ctx=T + 64, n_seq_max=4)
    toks, tok_lp, top_lp = finish(eng, eng.submit(ids, 16, temperature=0.0, ignore_eos=True, logprobs=4))
    reqs = [eng.submit(p, 16, temperature=0.0, ignore_eos=True, logprobs=4)
            for p in [ids] + [seq(9, seed=60 + s) for s in range(3)]]
    mixed = [finish(eng, r) for r in reqs][0]
    eng.close()
    assert len(toks) == 16
    octx = oracle(oracle_mod, "").context(T + 64)
    check_chain_batched(octx, ids, toks, "scheduler across T")
    ref = octx.eval(np.concatenate([ids, toks[:-1]]).astype(np.int32), 0, all_logits=True)[P - 1:].astype(np.float64)
    lsm = ref - ref.max(-1, keepdims=True)
    lsm -= np.log(np.exp(lsm).sum(-1, keepdims=True))
    d = np.abs(tok_lp - lsm[np.arange(16), toks])
    print(f"scheduler across T: worst |log-prob - oracle| {d.max():.4g}, bound {2 * logit_tol(ref).max():.4g}")
    assert (d <= 2 * logit_tol(ref).max(-1)).all()
    assert mixed[0] == toks and mixed[1].tobytes() == tok_lp.tobytes() and mixed[2].tobytes() == top_lp.tobytes(), \
        "the long request's log-probabilities depend on its batch-mates"


def test_speculative_rounds_across_the_threshold(mx, oracle_mod, T):
    """The same request with prompt-lookup drafts (sched_step_spec: 1 + D rows a request, several steps a round)."""
    ids = seq(T - 6, seed=7)
    eng = mx.Engine(f"synthetic:{NAME}:seed=0", n_ctx=T + 64, n_seq_max=4)
    toks, _ = eng.generate(ids, 16, temperature=0.0, ignore_eos=True, draft=(3, 2))
    steps = eng.spec_stats()["steps"]
    eng.close()
    assert steps > 0 and len(toks) == 16
    check_chain_batched(oracle(oracle_mod, "").context(T + 64), ids, toks, "speculative rounds across T")


CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from llama_p2p_amd import engine as E
ids = np.load({ids!r})
eng = E.Engine("synthetic:{name}:seed=0", n_ctx={n_ctx}, n_seq_max=4)
for s in (1, 2, 3):
    eng.forward_rows([s] * 8, list(range(8)), ids[s][:8], want_logits=False)
np.save({out!r}, np.stack([eng.forward_rows([1, 2, 3], [8 + k] * 3, [int(ids[s][8 + k]) for s in (1, 2, 3)])
                           for k in range(8)]))
eng.close()
"""


def test_batch_invariance_across_the_threshold(mx, T, tmp_path):
    """bf16: the long request's logits alone == beside three short requests, bitwise, at every step before and
    after its context passes T; the short requests' logits == those of an engine without the split path."""
    P = T - 4
    long_ids = seq(P + 8, seed=5)
    short = {s: seq(16, seed=50 + s) for s in (1, 2, 3)}
    eng = mx.Engine(f"synthetic:{NAME}:seed=0", n_ctx=T + 64, n_seq_max=4)
    eng.forward_rows([0] * P, list(range(P)), long_ids[:P], want_logits=False)
    for s in (1, 2, 3):
        eng.forward_rows([s] * 8, list(range(8)), short[s][:8], want_logits=False)
    alone, mixed = [], []
    for k in range(8):  # contexts T - 3 .. T + 4
        mixed.append(eng.forward_rows([0, 1, 2, 3], [P + k] + [8 + k] * 3,
                                      [int(long_ids[P + k])] + [int(short[s][8 + k]) for s in (1, 2, 3)]))
        alone.append(eng.forward_rows([0], [P + k], [int(long_ids[P + k])])[0])
    eng.close()
    mixed = np.stack(mixed)
    assert np.stack(alone).tobytes() == mixed[:, 0].tobytes(), "the long row's logits depend on its batch-mates"
    ids_file, out_file = str(tmp_path / "ids.npy"), str(tmp_path / "short.npy")
    np.save(ids_file, np.stack([short[1]] + [short[s] for s in (1, 2, 3)]))
    env = dict(os.environ, MX_NO_ATTN_SPLIT="1")
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, ids=ids_file, out=out_file, name=NAME, n_ctx=T + 64)],
                   check=True, env=env, timeout=120)
    assert np.load(out_file).tobytes() == mixed[:, 1:].tobytes(), "short rows of a long forward != the unsplit engine's"


@QUANTS
def test_17_rows_with_one_long_row(mx, oracle_mod, T, quant):
    """17 rows, each its own slot (the forms that finish q|k|v inside the attention at short contexts): one row past
    T sends the forward through launch_qkv_finish + the split attention; every row against the oracle."""
    P = T + 3
    long_ids = seq(P + 1, seed=9)
    shorts = [seq(9, seed=80 + i) for i in range(16)]
    eng = mx.Engine(f"synthetic:{NAME}:seed=0{quant}", n_ctx=T + 64, n_seq_max=17)
    om = oracle(oracle_mod, quant)
    eng.forward_rows([16] * P, list(range(P)), long_ids[:P], want_logits=False)
    for i, sq in enumerate(shorts):
        eng.forward_rows([i] * 8, list(range(8)), sq[:8], want_logits=False)
    got = eng.forward_rows(list(range(17)), [8] * 16 + [P], [int(sq[8]) for sq in shorts] + [int(long_ids[P])])
    assert_logits_close(got[16:], om.context(T + 64).eval(long_ids, 0), f"17 rows{quant}: the long row")
    for i, sq in enumerate(shorts):
        assert_logits_close(got[i:i + 1], om.context(64).eval(sq, 0), f"17 rows{quant}: short row {i}")
    eng.close()


def test_qwen3_rows_with_one_long_row(mx, T, tmp_path):
    """A Qwen3 model (per-head q/k norm weights), four rows of four slots, one past T: at <= 16 distinct rows the short
    form finishes the raw q|k|v inside the attention; the long forward finishes them with qkn_finish_kernel first and
    attends in the split form.  Every row against tests/qwen3_ref.py."""
    import qwen3_ref as Q

    P = T + 3
    long_ids = Q.seeded_ids("q3-tiny", P + 1)
    shorts = [Q.seeded_ids("q3-tiny", 9 + i) for i in range(3)]
    eng = mx.Engine(Q.write_gguf(str(tmp_path / "q3.gguf"), "q3-tiny"), n_ctx=T + 64, n_seq_max=4)
    eng.forward_rows([3] * P, list(range(P)), long_ids[:P], want_logits=False)
    for i, sq in enumerate(shorts):
        eng.forward_rows([i] * (len(sq) - 1), list(range(len(sq) - 1)), sq[:-1], want_logits=False)
    got = eng.forward_rows([0, 1, 2, 3], [len(sq) - 1 for sq in shorts] + [P], [int(sq[-1]) for sq in shorts] + [int(long_ids[P])])
    eng.close()
    for i, sq in enumerate(shorts + [long_ids]):
        ref = Q.forward("q3-tiny", sq, "ggml")[-1:].astype(np.float32)
        assert_logits_close(got[i:i + 1], ref, f"qwen3 row {i} (ctx {len(sq)})")
        assert_tokens_match(got[i:i + 1], ref, f"qwen3 row {i}")
