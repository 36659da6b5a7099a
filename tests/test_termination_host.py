"""How requests end, the parts that need no GPU (DESIGN.md §1 "How requests end"):

  * gguf.write_synthetic_gguf(eos_token_id=, eot_token_id=): with the defaults the file is byte for byte what the
    writer produced before the two keywords existed (tests/golden/synthetic_gguf_sha256.json, recorded from that
    writer); a chosen EOS changes only the four bytes of its value; both keys travel through GGUFReader, the
    Tokenizer and mx_gguf_check;
  * the prompt pool of test_termination_gpu.py covers every stop index with the oracle's own greedy chains;
  * pipeserve.Scheduler ends a request at the end-of-turn id as it does at EOS.
"""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import termination_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


@pytest.mark.parametrize("key", ["test-tiny:bf16", "test-tiny:q8_0", "test-tiny:q4_k_m", "test-d128:bf16"])
def test_default_file_is_byte_identical_to_the_earlier_writer(tmp_path, key):
    from llama_p2p_amd import gguf, synth

    with open(os.path.join(HERE, "golden", "synthetic_gguf_sha256.json")) as f:
        want = json.load(f)[key]
    name, wtype = key.split(":")
    a, b = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    gguf.write_synthetic_gguf(a, synth.SHAPES[name], seed=0, wtype=wtype)
    assert os.path.getsize(a) == want["bytes"] and _sha(a) == want["sha256"]
    gguf.write_synthetic_gguf(b, synth.SHAPES[name], seed=0, wtype=wtype, eos_token_id=2, eot_token_id=None)
    assert _sha(b) == want["sha256"]


def test_chosen_eos_changes_four_bytes_and_both_keys_round_trip(tmp_path):
    from llama_p2p_amd import engine, gguf, synth
    from llama_p2p_amd.tokenizer import Tokenizer

    shape = synth.SHAPES["test-tiny"]
    base, eos, both = (str(tmp_path / n) for n in ("base.gguf", "eos.gguf", "both.gguf"))
    gguf.write_synthetic_gguf(base, shape, seed=0)
    gguf.write_synthetic_gguf(eos, shape, seed=0, eos_token_id=0x1A7)
    gguf.write_synthetic_gguf(both, shape, seed=0, eos_token_id=300, eot_token_id=77)
    x = np.fromfile(base, dtype=np.uint8)
    y = np.fromfile(eos, dtype=np.uint8)
    assert x.size == y.size
    d = np.flatnonzero(x != y)
    assert 1 <= d.size <= 4 and d[-1] - d[0] < 4, d  # only the value: the weights are the synthetic model's
    assert int.from_bytes(y[d[0]:d[0] + 4].tobytes(), "little") == 0x1A7 and x[d[0]] == 2
    md0, md1, md2 = (gguf.GGUFReader(p).metadata for p in (base, eos, both))
    assert md0["tokenizer.ggml.eos_token_id"] == 2 and "tokenizer.ggml.eot_token_id" not in md0
    assert md1["tokenizer.ggml.eos_token_id"] == 0x1A7 and "tokenizer.ggml.eot_token_id" not in md1
    assert md2["tokenizer.ggml.eos_token_id"] == 300 and md2["tokenizer.ggml.eot_token_id"] == 77
    assert list(md0) == list(md1) and len(md2) == len(md0) + 1
    r0, r2 = gguf.GGUFReader(base), gguf.GGUFReader(both)
    assert list(r0.tensors) == list(r2.tensors)
    for name in ("token_embd.weight", "blk.1.ffn_down.weight", "output_norm.weight"):
        assert np.array_equal(r0.tensor(name), r2.tensor(name))
    tok = Tokenizer.from_gguf_metadata(md2)
    assert tok.eos_id == 300 and tok.eot_id == 77 and tok.is_eog(300) and tok.is_eog(77) and not tok.is_eog(2)
    for p in (base, eos, both):
        engine.gguf_check(p)  # the C++ parser accepts the files (no GPU)


def test_model_info_mirror_ends_with_eot_id():
    from llama_p2p_amd import engine

    names = [n for n, _ in engine.MxModelInfo._fields_]
    assert names[-1] == "eot_id" and names[-2] == "weight_type"
    with open(os.path.join(os.path.dirname(HERE), "include", "mx_engine.h")) as f:
        header = f.read()
    body = header[:header.index("} mx_model_info;")]
    body = body[body.rindex("typedef struct {"):]
    assert body.rstrip().splitlines()[-1].lstrip().startswith("int32_t eot_id;")


@pytest.mark.parametrize("name", R.MODELS)
def test_pool_covers_every_stop_index_with_the_oracle_chains(oracle_mod, name):
    """The oracle's own greedy chain of every pool prompt: each stop index has a prompt whose chain holds a token
    first at that index (and not in the prompt), so the GPU file can place EOS there; the most frequent token
    leaves rows that stop at different steps and rows that never stop."""
    from llama_p2p_amd import synth

    prompts = R.pool(name)
    assert len(prompts) == R.N_POOL and all(4 <= len(p) <= 40 for p in prompts)
    assert all(p[0] == 1 and all(3 <= t < R.vocab(name) for t in p[1:]) for p in prompts)
    om = oracle_mod.OracleModel(synth.SHAPES[name], seed=0)
    chains = [om.context(R.N_CTX).generate_greedy(p, R.T).tolist() for p in prompts]
    stops = R.choose_stops(chains, prompts)
    assert sorted(stops) == R.STOP_INDICES, f"{name}: no candidate for {set(R.STOP_INDICES) - set(stops)}"
    for j, (p, E) in stops.items():
        toks, fin = R.expectation(chains[p], E)
        assert len(toks) == j + 1 and toks[-1] == E and fin == 1
    assert len({E for _, E in stops.values()}) <= len(R.STOP_INDICES)
    E = R.most_frequent(chains[:16])
    where = {c.index(E) if E in c else None for c in chains[:16]}
    assert None in where and len(where) >= 3, f"{name}: token {E} stops the 16 rows at {where}"


def test_expectation_and_replay_helpers():
    assert R.expectation([5, 6, 7, 6], 6) == ([5, 6], 1)
    assert R.expectation([5, 6, 7], 9) == ([5, 6, 7], 0)
    assert R.expectation(list(range(30)), 23) == (list(range(24)), 1)  # EOS on the token that reaches max_tokens
    assert R.expectation(list(range(30)), 24) == (list(range(24)), 0)
    assert R.candidates([[4, 4, 5], [5, 9, 9]], 1) == [(1, 9)]
    assert R.candidates([[4, 8, 5]], 1, prompts=[[1, 8]]) == []
    # prompt 1 2 3 1 2, output 3 1 2 9: out[0] = 3 from the prefill, then one step drafts [1, 2, 3] (the 2-gram
    # (2, 3) is found at 1), keeps 1, 2 and the correction 9
    assert R.replay_spec([1, 2, 3, 1, 2], [3, 1, 2, 9], 3, 2) == [(1, 3, 2)]
    # the same request stopped at EOS = 2: the step keeps 1, 2 only, one of them counted as accepted
    assert R.replay_spec([1, 2, 3, 1, 2], [3, 1, 2], 3, 2) == [(1, 3, 1)]
    assert R.replay_spec([1, 2, 3, 1, 2], [3, 1], 3, 2) == [(1, 3, 0)]


# ------------------------------------------------------------------ pipeline Scheduler: end of turn
def _serve_one_stage(eos, eot, n_ctx=64):
    """test_pipeserve_cpu's single-stage server over its toy executor, with both end-of-generation ids."""
    import torch

    import test_pipeserve_cpu as S
    from llama_p2p_amd import pipeserve as P
    from llama_p2p_amd.placement import PeerScoreboard

    lanes, rows = 2, 3
    ex = S.ToyServeEngine(0, S.L, lanes * rows)
    runner = P.StageRunner(ex, None, 0, 1, lanes, rows, kmax=4, device=torch.device("cpu"), stage_time_every=3)
    sched = P.Scheduler(lanes, rows, n_ctx, eos, kmax=4, policy="score_aware", seed=11, eot=eot)
    front = P.PipelineFront(runner, None, sched, n_ctx, S.V, S.H, PeerScoreboard([0]))
    reqs = S._requests()
    res = [None] * len(reqs)

    def one(i):
        ids, mt = reqs[i]
        res[i] = front.generate(ids, mt, temperature=0.0, ignore_eos=(i % 4 == 3))

    th = [threading.Thread(target=one, args=(i,)) for i in range(len(reqs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    free = all(x is None for ln in sched.table for x in ln)
    front.close()
    return [r[0] for r in res], [r[1] for r in res], free


def test_scheduler_stops_at_the_end_of_turn_id():
    from llama_p2p_amd import pipeserve as P

    ref, fins, _ = _serve_one_stage(-1, -1)
    assert all(f == P.FINISH_LENGTH for f in fins)
    toks = [t for seq in ref for t in seq]
    eot = max(sorted(set(toks)), key=toks.count)
    assert P.Scheduler(1, 1, 8, 2).eot == -1  # the default: no end-of-turn id
    for eos, e in ((-1, eot), (eot, -1)):  # as the end-of-turn id, and as EOS: the same rows stop
        got, fins, free = _serve_one_stage(eos, e)
        stopped = 0
        for i, (a, b, fin) in enumerate(zip(ref, got, fins)):
            stop = eot in a and i % 4 != 3  # every fourth request ignores it
            k = a.index(eot) + 1 if stop else len(a)
            assert b == a[:k], f"request {i}"
            assert fin == (P.FINISH_STOP if stop else P.FINISH_LENGTH)
            stopped += int(stop and k < len(a))
        assert stopped >= 2 and free  # some rows lost a tail; every row was released
    # an id of -1 never matches a token, and the other id still does
    got, fins, _ = _serve_one_stage(-1, -1)
    assert got == ref
