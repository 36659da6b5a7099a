"""What the sampler chain costs per decode step: greedy, the default chain, typical + tail-free,
a 256-entry logit_bias and Mirostat v2, 1 and 32 rows, in the scheduler's multi-step device rounds.

    python tools/sampler_chain_cost.py [--model synthetic:llama3-8b:seed=0] [--tokens 64] [--out profiles/sampler_chain.txt]
                                       [--baseline PATH ...]

Every configuration runs in a child process with MX_SCHED_TRACE=1: one engine, per configuration a warm-up
completion (captures the round's graph) and a timed one of --tokens tokens for every row count.  The scheduler's
trace line of a round ("sched: decode M=.. K=.. ... ms": host clock from the round's first copy to its
synchronise, K decode steps) gives ms per step = ms / K; rounds that captured a graph and the short last round
are left out, the median, minimum and maximum of the rest are reported, with the trace lines of one round each.

--baseline PATH: a checkout of another commit with its library built (e.g. the parent); its greedy and default
chain are measured by the same child, importing that tree's package, before and after this tree's run, so the
two baseline runs bracket it on the same machine in the same session.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIAS = {3 + 7 * j: (-float("inf") if j % 16 == 0 else 0.25 * (j % 9) - 1.0) for j in range(256)}
CONFIGS = {
    "greedy": dict(temperature=0.0),
    "default chain": dict(temperature=0.8),
    "typical + tfs": dict(temperature=0.8, typical_p=0.9, tfs_z=0.95),
    "bias (256 entries)": dict(temperature=0.8, logit_bias=BIAS),
    "mirostat v2": dict(temperature=0.8, mirostat_mode=2),
}
OLD = ("greedy", "default chain")  # what a tree from before the extended chain can run


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
                reqs = eng.submit_many(prompts, a.tokens, seeds=list(range(1, rows + 1)), ignore_eos=True,
                                       **CONFIGS[name])
                for r in reqs:
                    eng.wait(r)
    eng.close()


def run_child(a, tree, configs):
    env = dict(os.environ, MX_SCHED_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--model", a.model, "--tokens",
           str(a.tokens), "--rows", ",".join(map(str, a.rows)), "--configs", ";".join(configs)]
    print(f"measuring {len(configs)} configurations over {tree} ...", file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child over {tree} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    out, key = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"cfg: (.*) \| (\d+) \| (.*)", line)
        if m:
            key = (m[1], int(m[2])) if m[3] == "timed" else None
            continue
        m = re.match(r"sched: decode M=(\d+) K=(\d+) (.*?)([0-9.]+) ms", line)
        if m and key:
            out.setdefault(key, []).append((int(m[2]), float(m[4]), "graph captured" in m[3], line))
    return out


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
    med = {}
    for label, out in runs:
        lines.append(f"-- {label}")
        for (name, rows), rounds in out.items():
            steps, k, sample = summarise(rounds)
            med[(label, name, rows)] = statistics.median(steps)
            lines.append(f"{name:>20s}, {rows:2d} rows: median {statistics.median(steps):.4f} ms/step, min {min(steps):.4f}, "
                         f"max {max(steps):.4f} ({len(steps)} rounds of K={k})   | {sample}")
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
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
