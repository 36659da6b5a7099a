"""Cost of per-token log-probabilities in the scheduler's decode step.

    python tools/logprobs_overhead.py [--model synthetic:test-8b-v128k:seed=0] [--rows 1 32] [--rounds 60]

For each row count M, M greedy requests run 8-step rounds (one captured graph replayed 8 times per
round) once without and once with logprobs=5, in the same process and build.  Round times come from the
engine's MX_SCHED_TRACE lines ("sched: decode M=.. K=.. ms"); rounds that captured a graph, rounds with
another M or K (admission, tail) and the first 5 of each run are dropped.  Prints microseconds per
decode step (round time / 8): median and mean over the kept rounds, and the difference.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"sched: decode M=(\d+) K=(\d+) (.*?)([0-9.]+) ms")


def child(model, M, rounds, lp):
    sys.path.insert(0, ROOT)
    import numpy as np

    from llama_p2p_amd.engine import Engine

    eng = Engine(model, n_ctx=8 * rounds + 64, n_seq_max=max(M, 1))
    rng = np.random.default_rng(0)
    prompts = [[1] + [int(t) for t in rng.integers(3, eng.n_vocab, 8)] for _ in range(M)]
    for tag, k in (("plain", None), ("logprobs", lp)):
        print(f"run {tag}", file=sys.stderr, flush=True)
        reqs = [eng.submit(p, 8 * rounds + 1, temperature=0.0, ignore_eos=True, logprobs=k) for p in prompts]
        for r in reqs:
            eng.wait(r)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:test-8b-v128k:seed=0")
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--logprobs", type=int, default=5)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.model, a.child, a.rounds, a.logprobs)
    print(f"model {a.model}, logprobs={a.logprobs}, {a.rounds} rounds of 8 steps per run (first 5 dropped)")
    for M in a.rows:
        env = dict(os.environ, MX_SCHED_TRACE="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", a.model, "--rounds", str(a.rounds),
                            "--logprobs", str(a.logprobs), "--child", str(M)], env=env, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        if p.returncode:
            sys.stderr.write(p.stderr[-2000:])
            raise SystemExit(f"child for M={M} exited with {p.returncode}")
        runs, cur = {}, None
        for ln in p.stderr.splitlines():
            if ln.startswith("run "):
                cur = runs.setdefault(ln[4:], [])
                continue
            m = LINE.search(ln)
            if m and cur is not None and int(m.group(1)) == M and int(m.group(2)) == 8 and "captured" not in m.group(3):
                assert ("(logprobs)" in m.group(3)) == (cur is runs.get("logprobs")), ln
                cur.append(float(m.group(4)) * 1000.0 / 8)
        res = {}
        for tag, v in runs.items():
            v = v[5:]
            res[tag] = (statistics.median(v), statistics.fmean(v), len(v))
            print(f"M={M:3d} {tag:9s}: {res[tag][0]:9.1f} us/step median, {res[tag][1]:9.1f} mean over {res[tag][2]} rounds")
        d = res["logprobs"][0] - res["plain"][0]
        print(f"M={M:3d} logprobs={a.logprobs} adds {d:.1f} us/step (median), {100 * d / res['plain'][0]:.1f}% of this model's step")


if __name__ == "__main__":
    main()
