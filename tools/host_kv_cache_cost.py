"""What the host-RAM tier saves and what its transfers cost: one KV slot, prompts of 448 shared +
32 own tokens alternated with an unrelated prompt so that every admission evicts the other, max_tokens 1, with
the tier on and with capacity 0 (the engine's behaviour without the tier); then the same for shared prefixes of 32
tokens -- the smallest the tier can restore, one packed tile -- 64, 96 and 128.

    python tools/host_kv_cache_cost.py [--model synthetic:test-8b-v128k:seed=0] [--reps 10] [--out profiles/host_kv_cache.txt]

One repetition, for capacity 0 and then for the tier on, on the same tokens: head + own_a (untimed: the slot holds
the head), an unrelated prompt (untimed: it evicts the head -- to host memory when the tier is on), then head +
own_b, timed by a host clock from submit to wait(): time to its first token.  With capacity 0 that prompt is
evaluated whole; with the tier on its head comes back from the host entry and only own_b is evaluated -- and the
same admission spills the unrelated prompt's record, which is part of the time.  The store is emptied after every
timed request and the slot then takes a short unrelated prompt, so no run finds anything of the one before it.  A third run keeps the tier on but replaces head + own_a by a second unrelated prompt, so head +
own_b finds no host entry: it is evaluated whole and the admission spills as before -- the restore against
recomputing at equal spill cost, which is what HOST_MIN is chosen by.  The first tokens of the three runs must be
equal in every repetition: that is the one requirement (exit status 1 otherwise).  The speed-up is reported, not
required.

The transfers alone: a child process repeats the tier-on sequence with MX_SCHED_TRACE=1, where the scheduler
synchronises around each step and prints "sched: host spill ... pack .. d2h .." and "sched: host restore ... h2d ..
unpack .."; those synchronises are why the timed repetitions run without the trace.  The rates stand against the
63 GB/s of the host link's specification (PCIe Gen5 x16).
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

LINK_GBS = 63.0
CAP = 1 << 30


def prompts(rng, n_vocab, shared, own):
    """head + own_a, an unrelated prompt of the same length, head + own_b (the own parts differ at once), and a
    second unrelated prompt that stands in for head + own_a in the runs without a host match."""
    head = np.concatenate([[1], rng.integers(3, n_vocab, shared - 1)])
    a, b = (np.concatenate([head, [3 + i], rng.integers(3, n_vocab, own - 1)]).astype(np.int32) for i in range(2))
    other, miss = (np.concatenate([[5 + i], rng.integers(3, n_vocab, shared + own - 1)]).astype(np.int32)
                   for i in range(2))
    scrub = np.concatenate([[7], rng.integers(3, n_vocab, 16)]).astype(np.int32)
    return a, other, b, miss, scrub


def first_token(eng, p):
    t0 = time.perf_counter()
    tok = eng.wait(eng.submit(p, 1, temperature=0.0, ignore_eos=True))[0]
    return time.perf_counter() - t0, tok


def sequence(eng, ps, cap, match=True):
    eng.set_host_cache(cap)
    first_token(eng, ps[0 if match else 3])
    first_token(eng, ps[1])
    dt, tok = first_token(eng, ps[2])
    eng.set_host_cache(0)
    first_token(eng, ps[4])  # the slot forgets head + own_b before the next run (17 tokens: never worth a spill)
    return dt, tok


def child(a):
    """One warm-up and `reps` traced tier-on sequences per prefix length; the scheduler's trace goes to stderr."""
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=a.shared + a.own + 32, n_seq_max=1)
    rng = np.random.default_rng(1)
    for shared in [a.shared] + a.small:
        print(f"prefix {shared}", file=sys.stderr, flush=True)
        for _ in range(1 + a.reps):
            sequence(eng, prompts(rng, eng.n_vocab, shared, a.own), CAP)
    eng.close()


def ms(v):
    return (f"median {statistics.median(v) * 1e3:.3f} ms, min {min(v) * 1e3:.3f} ms, max {max(v) * 1e3:.3f} ms "
            f"({len(v)} repetitions)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:test-8b-v128k:seed=0")
    ap.add_argument("--shared", type=int, default=448)
    ap.add_argument("--small", type=int, nargs="+", default=[32, 64, 96, 128],
                    help="further shared prefixes, from HOST_MIN up: where a restore starts to win")
    ap.add_argument("--own", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return child(a)
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=a.shared + a.own + 32, n_seq_max=1)
    info = eng.info
    per_pos = info.n_layer * 2 * info.n_head_kv * info.head_dim * 2
    rng = np.random.default_rng(0)
    same = True
    lines = [
        f"host KV cache cost: {a.model} ({info.n_layer} layers, K/V {per_pos} B per position), one KV slot, max_tokens 1, "
        f"greedy; per repetition, capacity 0, the tier on without a host match and the tier on, on the same tokens: head + "
        f"own_a (without a match: a second unrelated prompt), an unrelated prompt, "
        f"then head + own_b timed (host clock from submit to wait()); {a.own} own tokens; 2 warm-up repetitions, new "
        f"tokens every repetition"]
    modes = (("off", 0, True), ("miss", CAP, False), ("on", CAP, True))
    for shared in [a.shared] + a.small:
        t = {m: [] for m, _, _ in modes}
        for rep in range(2 + a.reps):
            ps = prompts(rng, eng.n_vocab, shared, a.own)
            tok = {}
            for m, cap, match in modes:
                dt, tok[m] = sequence(eng, ps, cap, match)
                if rep >= 2:
                    t[m].append(dt)
            same &= tok["off"] == tok["on"] == tok["miss"]
        md = {m: statistics.median(v) for m, v in t.items()}
        lines += [
            f"shared prefix {shared}: time to first token, capacity 0:                     {ms(t['off'])}",
            f"shared prefix {shared}: time to first token, tier on, no host match (spill): {ms(t['miss'])}",
            f"shared prefix {shared}: time to first token, tier on, restored:              {ms(t['on'])}",
            f"shared prefix {shared}: medians, capacity 0 / restored: {md['off'] / md['on']:.2f}; no match / restored "
            f"(the restore against recomputing, both spilling the unrelated prompt's record): {md['miss'] / md['on']:.2f} "
            f"(rows evaluated: {shared + a.own} against {a.own}; restored {-(-shared // 32) * 32 * per_pos} bytes)"]
    h, st = eng.host_cache_stats(), eng.stats()
    eng.close()
    lines.append(f"first tokens of the three runs equal, every repetition: {same}")
    lines.append(f"counters of the run: {h}, reused_prompt_tokens {st['reused_prompt_tokens']}")

    env = dict(os.environ, MX_SCHED_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--trace-child", "--model", a.model, "--shared", str(a.shared),
           "--small", *map(str, a.small), "--own", str(a.own), "--reps", str(a.reps)]
    tr = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if tr.returncode != 0:
        raise SystemExit(f"traced child failed ({tr.returncode}):\n{tr.stderr[-2000:]}")
    parts = re.split(r"^prefix (\d+)$", tr.stderr, flags=re.M)
    for shared, text in zip(parts[1::2], parts[2::2]):
        sp = [(int(m[1]), float(m[2]), float(m[3])) for m in re.finditer(
            r"sched: host spill \d+ entries (\d+) bytes pack ([0-9.]+) ms d2h ([0-9.]+) ms", text)]
        rs = [(int(m[1]), float(m[2]), float(m[3])) for m in re.finditer(
            r"sched: host restore \d+ entries (\d+) bytes h2d ([0-9.]+) ms unpack ([0-9.]+) ms", text)]
        pf = [float(m[1]) for m in re.finditer(r"sched: prefill \d+ requests ([0-9.]+) ms", text)]
        # the spills of this prefix's records (the first one of a phase is the previous phase's, of another length)
        full = statistics.mode([b for b, _, _ in sp]) if sp else 0
        sp = [x for x in sp if x[0] == full][2:]  # without the warm-up sequence's
        rs = rs[1:]
        if not sp or not rs:
            lines.append(f"shared prefix {shared}: no spill / restore lines in the traced child's output")
            continue
        med = lambda v: statistics.median(v)
        b, pk, d2h = sp[0][0], med([x[1] for x in sp]), med([x[2] for x in sp])
        rb, h2d, un = rs[0][0], med([x[1] for x in rs]), med([x[2] for x in rs])
        lines += [
            f"shared prefix {shared}, traced child (MX_SCHED_TRACE: host clock between stream synchronises, medians of "
            f"{len(sp)} spills / {len(rs)} restores):",
            f"  spill of {b} bytes: pack launch {pk:.3f} ms ({2 * b / pk / 1e6:.0f} GB/s read + written), device-to-host "
            f"{d2h:.3f} ms = {b / d2h / 1e6:.1f} GB/s ({b / d2h / 1e6 / LINK_GBS:.2f} of the link's {LINK_GBS:.0f} GB/s)",
            f"  restore of {rb} bytes: host-to-device {h2d:.3f} ms = {rb / h2d / 1e6:.1f} GB/s "
            f"({rb / h2d / 1e6 / LINK_GBS:.2f} of the link's), unpack launch {un:.3f} ms "
            f"({2 * rb / un / 1e6:.0f} GB/s read + written)"]
        if pf:
            lines.append(f"  prefill_batch calls of the last sequence (head + own_a whole, the unrelated prompt whole, "
                         f"own_b after the restore): {', '.join(f'{v:.3f}' for v in pf[-4:-1])} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
