"""What the sampler chain costs per decode step: greedy, the default chain, typical + tail-free,
a 256-entry logit_bias, Mirostat v2 and more than 64 candidates (top_k = 0, top_k = 100: the wide kernel; the host
sampler in a tree from before it), 1 and 32 rows, in the scheduler's rounds.

    python tools/sampler_chain_cost.py [--model synthetic:llama3-8b:seed=0] [--tokens 64] [--out profiles/sampler_chain.txt]
                                       [--baseline PATH ...]

Every configuration runs in a child process with MX_SCHED_TRACE=1: one engine, per configuration a warm-up
completion (captures the round's graph) and a timed one of --tokens tokens for every row count.  The scheduler's
trace line of a round ("sched: decode M=.. K=.. ... ms": host clock from the round's first copy to its
synchronise, K decode steps) gives ms per step = ms / K; rounds that captured a graph and the short last round
are left out, the median, minimum and maximum of the rest are reported, with the trace lines of one round each.
A host-sampled round's trace ends at its synchronise, before the host sampler runs, so every configuration also
reports the wall clock of the timed completion per token (submit to the last wait, its prefill included): that is
the figure to compare a host-sampled configuration by.

--baseline PATH: a checkout of another commit with its library built (e.g. the parent); its greedy, default chain,
top_k = 0 and top_k = 100 (one host-sampled step per round there) are measured by the same child, importing that
tree's package, before and after this tree's run, so the two baseline runs bracket it on the same machine in the
same session.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIAS = {3 + 7 * j: (-float("inf") if j % 16 == 0 else 0.25 * (j % 9) - 1.0) for j in range(256)}
CONFIGS = {
    "greedy": dict(temperature=0.0),
    "default chain": dict(temperature=0.8),
    "typical + tfs": dict(temperature=0.8, typical_p=0.9, tfs_z=0.95),
    "bias (256 entries)": dict(temperature=0.8, logit_bias=BIAS),
    "mirostat v2": dict(temperature=0.8, mirostat_mode=2),
    "top_k=0": dict(temperature=0.8, top_k=0),
    "top_k=100": dict(temperature=0.8, top_k=100),
}
OLD = ("greedy", "default chain", "top_k=0", "top_k=100")  # what a tree from before the extended chain can run


def child(a):
    sys.path.insert(0, a.tree)
    import numpy as np
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=32 + 2 * a.tokens, n_seq_max=max(a.rows))
    rng = np.random.default_rng(0)
    for name in a.configs:
        for rows in a.rows:
            prompts = [np.concatenate([[1], rng.integers(3, eng.n_vocab, 7)]).astype(np.int32) for _ in range(rows)]
            for phase in ("warm-up", "timed"):
                print(f"cfg: {name} | {rows} | {phase}", file=sys.stderr, flush=True)
                t0 = time.perf_counter()
                reqs = eng.submit_many(prompts, a.tokens, seeds=list(range(1, rows + 1)), ignore_eos=True,
                                       **CONFIGS[name])
                for r in reqs:
                    eng.wait(r)
                print(f"wall: {1e3 * (time.perf_counter() - t0) / a.tokens:.4f}", file=sys.stderr, flush=True)
    eng.close()


def run_child(a, tree, configs):
    env = dict(os.environ, MX_SCHED_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--model", a.model, "--tokens",
           str(a.tokens), "--rows", ",".join(map(str, a.rows)), "--configs", ";".join(configs)]
    print(f"measuring {len(configs)} configurations over {tree} ...", file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit(f"child over {tree} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    out, wall, key = {}, {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"cfg: (.*) \| (\d+) \| (.*)", line)
        if m:
            key = (m[1], int(m[2])) if m[3] == "timed" else None
            continue
        m = re.match(r"wall: ([0-9.]+)", line)
        if m and key:
            wall[key] = float(m[1])
            continue
        m = re.match(r"sched: decode M=(\d+) K=(\d+) (.*?)([0-9.]+) ms", line)
        if m and key:
            out.setdefault(key, []).append((int(m[2]), float(m[4]), "graph captured" in m[3], line))
    return out, wall


def summarise(rounds):
    kmax = max(k for k, *_ in rounds)
    steps = [ms / k for k, ms, cap, _ in rounds if k == kmax and not cap]
    sample = next(line for k, ms, cap, line in rounds if k == kmax and not cap)
    return steps, kmax, sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:llama3-8b:seed=0")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--rows", default="1,32")
    ap.add_argument("--baseline", action="append", default=[])
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=600, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--configs", default=";".join(CONFIGS), help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.rows = [int(r) for r in a.rows.split(",")]
    a.configs = a.configs.split(";")
    if a.child:
        return child(a)
    runs = []
    for b in a.baseline:
        runs.append((f"baseline {os.path.relpath(b, ROOT)}, run 1", run_child(a, os.path.abspath(b), OLD)))
    runs.append(("this tree", run_child(a, ROOT, list(CONFIGS))))
    for b in a.baseline:
        runs.append((f"baseline {os.path.relpath(b, ROOT)}, run 2", run_child(a, os.path.abspath(b), OLD)))
    lines = [f"sampler chain cost: {a.model}, {a.tokens} tokens per request after a warm-up completion, rows {a.rows}; "
             f"ms per decode step = a round's traced time / its K steps, rounds of the largest K without a graph "
             f"capture; every run is one child process with one engine, in the order listed"]
    med, wal = {}, {}
    for label, (out, wall) in runs:
        lines.append(f"-- {label}")
        for (name, rows), rounds in out.items():
            steps, k, sample = summarise(rounds)
            med[(label, name, rows)] = statistics.median(steps)
            wal[(label, name, rows)] = wall[(name, rows)]
            lines.append(f"{name:>20s}, {rows:2d} rows: median {statistics.median(steps):.4f} ms/step, min {min(steps):.4f}, "
                         f"max {max(steps):.4f} ({len(steps)} rounds of K={k}), wall {wall[(name, rows)]:.4f} ms/token"
                         f"   | {sample}")
    here = {(n, r): v for (lab, n, r), v in med.items() if lab == "this tree"}
    lines.append("-- over the default chain, this tree (medians)")
    for (name, rows), v in here.items():
        if name not in OLD:
            lines.append(f"{name:>20s}, {rows:2d} rows: {v - here[('default chain', rows)]:+.4f} ms/step "
                         f"({100 * (v / here[('default chain', rows)] - 1):+.2f} %)")
    if a.baseline:
        lines.append("-- this tree against the baseline runs (medians)")
        for name in OLD:
            for rows in a.rows:
                base = [v for (lab, n, r), v in med.items() if lab != "this tree" and n == name and r == rows]
                lo, hi = min(base), max(base)
                v = here[(name, rows)]
                where = "inside" if lo <= v <= hi else ("below" if v < lo else "above")
                lines.append(f"{name:>20s}, {rows:2d} rows: {v:.4f} ms/step, baseline runs {lo:.4f} .. {hi:.4f}: {where} their spread")
        lines.append("-- wall clock per token (host sampling included), this tree against the baseline runs")
        for name in OLD:
            for rows in a.rows:
                base = [v for (lab, n, r), v in wal.items() if lab != "this tree" and n == name and r == rows]
                v = wal[("this tree", name, rows)]
                lines.append(f"{name:>20s}, {rows:2d} rows: {v:.4f} ms/token, baseline runs {min(base):.4f} .. {max(base):.4f}"
                             f" ({min(base) / v:.2f}x .. {max(base) / v:.2f}x)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
