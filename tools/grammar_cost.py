"""What grammar-constrained sampling costs, in the scheduler's rounds.

    python tools/grammar_cost.py --baseline PARENT [--bench] [--model synthetic:llama3-8b:seed=0] [--tokens 64]
                                 [--out profiles/grammar.txt]

PARENT is a checkout of the parent commit with its library built.  Everything in profiles/grammar.txt comes from
this one command:

(a) Without a grammar: greedy and the default chain, 1 and 32 rows, ms per decode step from the scheduler's trace
    (tools/sampler_chain_cost.py's child and figures): the parent's build, this tree, the parent's, this tree,
    the parent's -- three runs of the yardstick around two of this tree.  With --bench, bench.py --gpus 1
    --steps 64 --warmup 8 in both checkouts, alternating three times.
(b) K = 1 against K = 8 without a grammar, in one child process with the trace on: rounds of one step are made by
    requests of max_tokens = 2 (the first token comes from the prefill, the second from a round of K = 1),
    twenty of them per row count after a warm-up, next to the K = 8 rounds of a 64-token completion.
(c) The mask kernel alone: mx_grammar_mask_time -- resident buffers, 200 launches between two HIP events -- over
    the masks of real JSON_GBNF states and over crafted ones, 1 and 32 rows.
(d) With JSON_GBNF: 1 and 32 rows all constrained, and one constrained row among 31 plain ones; wall clock per
    token against the same requests without a grammar; the host mask on a cache miss and on a hit; the bytes
    uploaded per step; cache hit rates over 256 generated tokens.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def vocab_of(E, n):
    from llama_p2p_amd.gguf import synthetic_spm_vocab
    from llama_p2p_amd.tokenizer import Tokenizer

    toks, scores, types = synthetic_spm_vocab(n)
    tk = Tokenizer(toks, scores, types, "llama", bos_id=1, eos_id=2)
    pieces = [tk.token_to_piece(t) for t in range(n)]
    return E.GrammarVocab(pieces, [t for t in range(n) if tk.is_eog(t)]), pieces


def timed(eng, prompts, tokens, per):
    """Plain requests queued together, then one submit per grammar request (there is no batch entry for those)."""
    t0 = time.perf_counter()
    plain = [i for i, kw in enumerate(per) if "grammar" not in kw]
    reqs = {}
    if plain:
        ids = eng.submit_many([prompts[i] for i in plain], tokens, seeds=[i + 1 for i in plain],
                              per_request=[per[i] for i in plain])
        reqs.update(zip(plain, ids))
    for i, kw in enumerate(per):
        if "grammar" in kw:
            reqs[i] = eng.submit(prompts[i], tokens, seed=i + 1, **kw)
    outs = [eng.wait(reqs[i]) for i in range(len(per))]
    dt = time.perf_counter() - t0
    return 1e3 * dt / max(len(t) for t, _ in outs), outs


def part_b(a, lines):
    import numpy as np
    from llama_p2p_amd import engine as E
    from llama_p2p_amd.llama_grammar import JSON_GBNF

    eng = E.Engine(a.model, n_ctx=32 + 2 * a.tokens, n_seq_max=32)
    V = eng.n_vocab
    gv, pieces = vocab_of(E, V)
    rng = np.random.default_rng(0)
    lines.append(f"-- (d) JSON_GBNF, {a.model} (V = {V}), {a.tokens} tokens per request after a warm-up completion; wall "
                 f"clock ms per token of the longest request, prefill included")
    for name, kw in (("greedy", dict(temperature=0.0)), ("default chain", dict(temperature=0.8))):
        for rows, n_gram in ((1, 1), (32, 32), (32, 1)):
            prompts = [np.concatenate([[1], rng.integers(3, V, 7)]).astype(np.int32) for _ in range(rows)]
            res = {}
            for label, ng in (("no grammar", 0), ("grammar", n_gram)):
                g = E.CompiledGrammar(gv, JSON_GBNF)
                per = [dict(kw, grammar=g) if i < ng else dict(kw, ignore_eos=True) for i in range(rows)]
                timed(eng, prompts, a.tokens, per)  # warm-up: captures the graphs, fills the mask cache
                s0 = eng.sampler_stats()
                ms, outs = timed(eng, prompts, a.tokens, per)
                s1 = eng.sampler_stats()
                res[label] = (ms, s1["rounds"] - s0["rounds"], s1["device_steps"] - s0["device_steps"], g.cache_stats(),
                              min(len(t) for t, _ in outs))
            (m0, r0, d0, _, _), (m1, r1, d1, cs, shortest) = res["no grammar"], res["grammar"]
            lines.append(f"{name:>14s}, {rows:2d} rows, {n_gram:2d} constrained: {m1:.3f} ms/token against {m0:.3f} without "
                         f"({m1 / m0:.2f}x); rounds / steps {r1} / {d1} against {r0} / {d0}; shortest request {shortest} "
                         f"tokens; cache {cs}")
    eng.close()
    # the host mask of a state: a miss (one walk of the vocabulary) and a hit
    g = E.CompiledGrammar(gv, JSON_GBNF)
    st, miss, hit, rng = g.state(), [], [], np.random.default_rng(1)
    eog = {2}
    for _ in range(256):
        c0 = g.cache_stats()
        t0 = time.perf_counter()
        w, status = st.mask()
        dt = 1e3 * (time.perf_counter() - t0)
        (miss if g.cache_stats()["misses"] > c0["misses"] else hit).append(dt)
        ids = [t for t in np.nonzero(np.unpackbits(w.view(np.uint8), bitorder="little")[:V])[0] if t not in eog]
        if not ids:
            break
        st.accept(int(rng.choice(ids)))
    cs = g.cache_stats()
    lines.append(f"host mask over V = {V}: miss median {statistics.median(miss):.3f} ms (max {max(miss):.3f}, {len(miss)} "
                 f"states), hit median {statistics.median(hit) if hit else float('nan'):.4f} ms ({len(hit)} lookups; the "
                 f"copy of {4 * ((V + 31) // 32)} bytes into the caller's buffer included)")
    lines.append(f"-- cache over a random walk of {len(miss) + len(hit)} tokens through JSON_GBNF: {cs}, hit rate "
                 f"{cs['hits'] / max(1, cs['hits'] + cs['misses']):.3f}")
    lines.append(f"upload per step: {4 * ((V + 31) // 32)} bytes per constrained row + 4 bytes per row of the round")
    # (c) the kernel alone, on the masks of real states and on crafted ones
    nw = (V + 31) // 32
    real = {}
    st = E.CompiledGrammar(gv, JSON_GBNF).state()
    real["JSON_GBNF at root (one token allowed)"] = st.mask()[0]
    for piece in (b"{", b'"', b"a"):
        st.accept(next(t for t in range(V) if pieces[t] == piece))
    real["JSON_GBNF inside a string"] = st.mask()[0]
    real["half of the tokens banned, at random"] = rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
    real["every token allowed"] = np.full(nw, 0xFFFFFFFF, dtype=np.uint32)
    real["every token banned"] = np.zeros(nw, dtype=np.uint32)
    lines.append(f"-- (c) grammar_mask_kernel alone, V = ldl = {V}: us per launch, mean of 200 launches between two HIP "
                 f"events on resident buffers after 3 warm-up launches (the kernel reads {4 * nw} bytes of mask per row "
                 f"and writes 4 bytes per banned token)")
    for label, w in real.items():
        banned = V - int(np.unpackbits(w.view(np.uint8), bitorder="little")[:V].sum())
        for rows in (1, 32):
            us = E.grammar_mask_time(np.tile(w, (rows, 1)), V)
            lines.append(f"{label:>40s}, {rows:2d} rows ({banned} banned per row, {4 * banned * rows / 1e6:.3f} MB written): "
                         f"{us:.2f} us")


def k1_child(a):
    """Rounds of one step without a grammar, and the K = 8 rounds of the same engine (trace on stderr)."""
    import numpy as np
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=32 + 2 * a.tokens, n_seq_max=32)
    rng = np.random.default_rng(0)
    for name, kw in (("greedy", dict(temperature=0.0)), ("default chain", dict(temperature=0.8))):
        for rows in (1, 32):
            prompts = [np.concatenate([[1], rng.integers(3, eng.n_vocab, 7)]).astype(np.int32) for _ in range(rows)]
            for phase, tokens, n in (("warm-up", a.tokens, 1), ("warm-up", 2, 2), ("K8", a.tokens, 1), ("K1", 2, 20)):
                print(f"cfg: {name} | {rows} | {phase}", file=sys.stderr, flush=True)
                for _ in range(n):
                    for r in eng.submit_many(prompts, tokens, seeds=list(range(1, rows + 1)), ignore_eos=True, **kw):
                        eng.wait(r)
    eng.close()


def part_k1(a, lines):
    import re
    import subprocess

    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--k1-child", "--model", a.model, "--tokens",
                        str(a.tokens)], env=dict(os.environ, MX_SCHED_TRACE="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"K = 1 child failed ({p.returncode}):\n{p.stderr[-3000:]}")
    got, key = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"cfg: (.*) \| (\d+) \| (.*)", line)
        if m:
            key = (m[1], int(m[2]), m[3]) if m[3] in ("K8", "K1") else None
            continue
        m = re.match(r"sched: decode M=(\d+) K=(\d+) (.*?)([0-9.]+) ms", line)
        if m and key and "graph captured" not in m[3] and int(m[1]) == key[1]:
            if (key[2] == "K8" and int(m[2]) == 8) or (key[2] == "K1" and int(m[2]) == 1):
                got.setdefault(key, []).append(float(m[4]) / int(m[2]))
    lines.append("-- (b) K = 1 against K = 8, no grammar, one process: ms per decode step from the trace; a round of one step "
                 "is the round of a max_tokens = 2 request")
    for (name, rows, phase), v in sorted(got.items()):
        if phase != "K1" or (name, rows, "K8") not in got:
            continue
        k8 = got[(name, rows, "K8")]
        m1, m8 = statistics.median(v), statistics.median(k8)
        lines.append(f"{name:>14s}, {rows:2d} rows: K = 1 median {m1:.4f} ms/step (min {min(v):.4f}, max {max(v):.4f}, "
                     f"{len(v)} rounds), K = 8 median {m8:.4f} ms/step ({len(k8)} rounds): {m1 - m8:+.4f} ms/step "
                     f"({100 * (m1 / m8 - 1):+.2f} %)")


def part_bench(a, lines):
    import json
    import subprocess

    lines.append("-- bench.py --gpus 1 --steps 64 --warmup 8, the parent's build and this tree alternating")
    for i in range(1, 4):
        for label, tree in (("parent's build", os.path.abspath(a.baseline[0])), ("this tree", ROOT)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "64", "--warmup", "8"], cwd=tree,
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=a.timeout)
            d = json.loads(p.stdout.strip().splitlines()[-1])
            lines.append(f"{label:>16s}, run {i}: {d['value']:.2f} tokens/s, {d['ms_per_step']:.4f} ms/step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:llama3-8b:seed=0")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--baseline", action="append", default=[])
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--k1-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.k1_child:
        return k1_child(a)
    import sampler_chain_cost as S

    a.rows = [1, 32]
    names = ["greedy", "default chain"]
    order = [("this tree", ROOT)]
    if a.baseline:
        b = os.path.abspath(a.baseline[0])
        order = [("parent's build, run 1", b), ("this tree, run 1", ROOT), ("parent's build, run 2", b),
                 ("this tree, run 2", ROOT), ("parent's build, run 3", b)]
    lines = [f"grammar cost: {a.model}", "-- (a) no grammar: ms per decode step = a round's traced time / its K steps, rounds "
             "of the largest K without a graph capture; one child process per run, in the order listed"]
    med = {}
    for label, tree in order:
        out, wall = S.run_child(a, tree, names)
        for (name, rows), rounds in out.items():
            steps, k, sample = S.summarise(rounds)
            med[(label, name, rows)] = statistics.median(steps)
            lines.append(f"{label:>24s} {name:>14s}, {rows:2d} rows: median {statistics.median(steps):.4f} ms/step, min "
                         f"{min(steps):.4f}, max {max(steps):.4f} ({len(steps)} rounds of K={k}), wall "
                         f"{wall[(name, rows)]:.4f} ms/token")
    if a.baseline:
        for name in names:
            for rows in a.rows:
                base = [x for (lab, n, r), x in med.items() if lab.startswith("parent") and n == name and r == rows]
                here = [x for (lab, n, r), x in med.items() if lab.startswith("this") and n == name and r == rows]
                lo, hi = min(base), max(base)
                where = ["inside" if lo <= v <= hi else ("below" if v < lo else "above") for v in here]
                lines.append(f"{name:>14s}, {rows:2d} rows: this tree {', '.join(f'{v:.4f}' for v in here)} ms/step; the parent's "
                             f"three runs {lo:.4f} .. {hi:.4f}: {', '.join(where)} their spread")
        if a.bench:
            part_bench(a, lines)
    part_k1(a, lines)
    part_b(a, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
