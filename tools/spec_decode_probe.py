"""What prompt-lookup speculative decoding costs and gains at batch 1.

    python tools/spec_decode_probe.py [--model synthetic:llama3-8b:seed=0 ...] [--tokens 256] [--repeats 3]
                                      [--out profiles/spec_decode.txt]

One request (BOS + a 12-token random block twice, as tests/test_spec_decode_gpu.py) generates `tokens` greedy
tokens on one engine: plain, with draft=(10, 2) and with draft=(4, 2), the three alternating `repeats` times
after an untimed pass of each that captures the graphs.  Reported per variant, medians over the repeats:

  * wall tok/s: tokens / host time from submit to wait (prefill included, the same for all three);
  * the step time: from the engine's MX_SCHED_TRACE lines -- a round's host time around K graph replays and the
    sync that ends them, divided by K; only full K = 8 rounds that captured no graph.  M = 1 is the plain step,
    M = 1 + D the speculating one (draft kernel + forward of 1 + D rows + argmax + accept kernel);
  * accepted drafts per speculating step (spec_stats), so tokens per step = 1 + accepted per step;
  * the break-even acceptance per step, t_spec / t_plain - 1: speculation gains when accepted per step exceeds it.

The tokens of the three variants are compared and must be equal.  The acceptance printed here says nothing
about real text: a random-weight model either falls into a loop, which the lookup predicts almost perfectly
(the small test models), or hardly repeats a token within the run, so next to nothing is drafted or accepted
(Llama-3-8B's and TinyLlama's shapes).
The step times and the break-even are the portable numbers.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = re.compile(r"sched: decode M=1 K=8 (.*?)([0-9.]+) ms")
SPEC = re.compile(r"sched: speculating R=1 D=(\d+) K=8 kept (\d+) tokens (.*?)([0-9.]+) ms")
VARIANTS = [("plain", None), ("draft=(10, 2)", (10, 2)), ("draft=(4, 2)", (4, 2))]


def child(model, tokens, repeats):
    sys.path.insert(0, ROOT)
    import numpy as np

    from llama_p2p_amd.engine import Engine

    eng = Engine(model, n_ctx=tokens + 64, n_seq_max=1)
    block = [int(t) for t in np.random.default_rng(100).integers(3, eng.n_vocab, 12)]
    prompt = [1] + block + block
    first = None
    for rep in range(repeats + 1):  # pass 0: untimed (graph capture, first launches)
        for tag, draft in VARIANTS:
            print(f"run {rep} {tag}", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            req = eng.submit(prompt, tokens, temperature=0.0, ignore_eos=True, draft=draft)
            n, done = 0, False
            while not done:
                toks, done = eng.poll(req, n)
                n = len(toks)
            st = eng.spec_stats(req)
            toks, _ = eng.wait(req)
            dt = time.perf_counter() - t0
            first = first or toks
            if toks != first:
                raise SystemExit(f"{tag}: tokens differ from the plain run's")
            print(json.dumps({"rep": rep, "tag": tag, "seconds": dt, "tokens": len(toks), **st}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", nargs="+", default=["synthetic:llama3-8b:seed=0"])
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_decode.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.model[0], a.tokens, a.repeats)
    text = "".join(measure(m, a) for m in a.model)
    text += ("acceptance of random-weight models is not that of real text: the small test models loop (nearly every "
             "draft right), the large shapes hardly repeat a token within the run (next to nothing drafted or "
             "accepted); DESIGN.md §10\n")
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def measure(model, a):
    env = dict(os.environ, MX_SCHED_TRACE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", model, "--tokens", str(a.tokens),
                        "--repeats", str(a.repeats), "--child"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    if p.returncode:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit(f"child exited with {p.returncode}")
    runs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    step_ms = {tag: [] for tag, _ in VARIANTS}  # ms per step of full, uncaptured rounds of the timed passes
    cur, timed = None, False
    for ln in p.stderr.splitlines():
        if ln.startswith("run "):
            _, rep, cur = ln.split(" ", 2)
            timed = int(rep) > 0
            continue
        m = PLAIN.search(ln) if cur == "plain" else SPEC.search(ln)
        if m and timed and "captured" not in m.group(m.lastindex - 1):
            step_ms[cur].append(float(m.group(m.lastindex)) / 8)
    lines = [f"model {model}, one request, {a.tokens} greedy tokens, prompt = BOS + a 12-token block twice; "
             f"medians over {a.repeats} alternating repeats"]
    t_plain = statistics.median(step_ms["plain"]) if step_ms["plain"] else float("nan")
    for tag, draft in VARIANTS:
        rs = [r for r in runs if r["tag"] == tag and r["rep"] > 0]
        tps = statistics.median(r["tokens"] / r["seconds"] for r in rs)
        t = statistics.median(step_ms[tag]) if step_ms[tag] else float("nan")
        M = 1 if draft is None else 1 + draft[0]
        ln = f"{tag:14s}: {tps:8.1f} tok/s wall; step M={M:2d} {1000 * t:8.1f} us ({len(step_ms[tag])} rounds of 8)"
        if draft is not None:
            r0 = rs[0]
            ln += (f"; {r0['steps']} speculating steps, drafted {r0['drafted']}, accepted {r0['accepted']} = "
                   f"{r0['accepted'] / max(1, r0['steps']):.2f} per step; break-even {t / t_plain - 1:.2f} per step")
        lines.append(ln)
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
