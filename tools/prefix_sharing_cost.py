"""What prefix sharing saves and what its copy costs: 32 requests of 448 shared + 32 own tokens in
one submit_batch, max_tokens 1, with sharing off and on.

    python tools/prefix_sharing_cost.py [--model synthetic:test-8b-v128k:seed=0] [--reps 10] [--out profiles/prefix_sharing.txt]

Time to all first tokens: a host clock from submit_batch to the last wait() (max_tokens = 1: a request ends with
its prefill).  Off and on alternate in one process on the same batch, new tokens every repetition; before each
timed batch every slot takes a short unrelated prompt (untimed), so no slot holds anything of the batch beyond
BOS and the only reuse is what the round itself shares.  The first tokens of the two runs are compared.

The copy launch alone: a child process repeats the sharing round with MX_SCHED_TRACE=1, where the scheduler
synchronises around the launch and prints its copies, bytes and time ("sched: kv copy ..."); those extra
synchronises are why the timed repetitions above run without the trace.  Its rate, (read + written) bytes / time,
stands next to mx_probe_copy's figure from the same run -- a 4 GiB streaming copy, where launch latency and the
last wave's tail vanish, which they do not in a copy of tens of microseconds.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(rng, n_vocab, n_req, shared, own):
    head = np.concatenate([[1], rng.integers(3, n_vocab, shared - 1)])
    return [np.concatenate([head, [3 + i], rng.integers(3, n_vocab, own - 1)]).astype(np.int32) for i in range(n_req)]


def first_tokens(eng, prompts):
    t0 = time.perf_counter()
    reqs = eng.submit_many(prompts, 1, temperature=0.0, ignore_eos=True)
    toks = [eng.wait(r)[0] for r in reqs]
    return time.perf_counter() - t0, toks


def child(a):
    """One warm-up round and `reps` traced rounds with sharing on; the scheduler's trace goes to stderr."""
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=a.shared + a.own + 32, n_seq_max=a.requests, prefix_sharing=True)
    rng = np.random.default_rng(1)
    for _ in range(1 + a.reps):
        first_tokens(eng, batch(rng, eng.n_vocab, a.requests, a.shared, a.own))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:test-8b-v128k:seed=0")
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--shared", type=int, default=448)
    ap.add_argument("--own", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return child(a)
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=a.shared + a.own + 32, n_seq_max=a.requests)
    rng = np.random.default_rng(0)
    t = {False: [], True: []}
    same = True
    for rep in range(2 + a.reps):  # two warm-up pairs
        prompts = batch(rng, eng.n_vocab, a.requests, a.shared, a.own)
        toks = {}
        for on in (False, True):
            # every slot first takes an unrelated prompt (untimed), so neither run finds its batch in a slot
            eng.set_prefix_sharing(False)
            first_tokens(eng, [p[:17] for p in batch(rng, eng.n_vocab, a.requests, 1, 16)])
            eng.set_prefix_sharing(on)
            dt, toks[on] = first_tokens(eng, prompts)
            if rep >= 2:
                t[on].append(dt)
        same &= toks[False] == toks[True]
    sh, st = eng.sharing_stats(), eng.stats()
    info = eng.info
    eng.close()
    gbs, desc = E.probe_copy(0, gib=4, iters=10)

    env = dict(os.environ, MX_SCHED_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--trace-child", "--model", a.model, "--requests", str(a.requests),
           "--shared", str(a.shared), "--own", str(a.own), "--reps", str(a.reps)]
    tr = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if tr.returncode != 0:
        raise SystemExit(f"traced child failed ({tr.returncode}):\n{tr.stderr[-2000:]}")
    cp = [(int(m[1]), int(m[2]), float(m[3])) for m in re.finditer(r"sched: kv copy (\d+) copies (\d+) bytes ([0-9.]+) ms",
                                                                   tr.stderr)][1:]  # drop the warm-up round's
    pf = [float(m[2]) for m in re.finditer(r"sched: prefill (\d+) requests ([0-9.]+) ms", tr.stderr)]

    ms = lambda v: (f"median {statistics.median(v) * 1e3:.3f} ms, min {min(v) * 1e3:.3f} ms, max {max(v) * 1e3:.3f} ms"
                    f" ({len(v)} repetitions)" if len(v) > 1 else f"{v[0] * 1e3:.3f} ms (one run)")
    per_pos = info.n_layer * 2 * info.n_head_kv * info.head_dim * 2
    lines = [
        f"prefix sharing cost: {a.model} ({info.n_layer} layers, K/V {per_pos} B per position), {a.requests} requests of "
        f"{a.shared} shared + {a.own} own tokens in one submit_batch, max_tokens 1, greedy; off / on alternating on the "
        f"same batch after 2 warm-up pairs, new tokens every repetition, slots scrubbed with unrelated prompts before "
        f"each timed batch; host clock from submit_batch to the last wait()",
        f"time to all first tokens, sharing off: {ms(t[False])}",
        f"time to all first tokens, sharing on:  {ms(t[True])}",
        f"ratio of the medians off / on: {statistics.median(t[False]) / statistics.median(t[True]):.2f}",
        f"rows evaluated per batch: off {a.requests * (a.shared + a.own)}, on {a.shared + a.own + (a.requests - 1) * a.own} "
        f"(+ padding to 16-row blocks)",
        f"first tokens with sharing on == first tokens of the same batch with sharing off, every repetition: {same}",
        f"counters of the run: {sh}, reused_prompt_tokens {st['reused_prompt_tokens']}",
    ]
    if cp:
        n, b, _ = cp[0]
        tms = [c[2] * 1e-3 for c in cp]
        med = statistics.median(tms)
        lines += [
            f"copy launch (traced child process, MX_SCHED_TRACE: host clock between two stream synchronises): {n} copies, "
            f"{b} bytes written ({b / 1e6:.1f} MB, as many read): {ms(tms)}",
            f"copy rate (read + written) at the median: {2 * b / med / 1e9:.0f} GB/s; at the minimum: "
            f"{2 * b / min(tms) / 1e9:.0f} GB/s",
            f"all {n} copies read the one leader's slot ({b // n / 1e6:.1f} MB): it comes from HBM once and from the "
            f"caches after that, so HBM sees about the written bytes: {b / med / 1e9:.0f} GB/s of stores at the median",
        ]
    else:
        lines.append("copy launch: no 'sched: kv copy' line in the traced child's output")
    if pf:
        lines.append(f"traced child, prefill_batch calls (leaders, then followers, per round): "
                     f"{', '.join(f'{v:.3f}' for v in pf[-4:])} ms (last two rounds)")
    lines.append(f"mx_probe_copy, same run: {gbs:.0f} GB/s (read + written; 4 GiB, {desc})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
