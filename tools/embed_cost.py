"""What the embedding tail costs: Engine.embed of 32 prompts x 128 tokens with MEAN pooling and
normalize against forward_rows(want_logits=False) over the same 4096 rows -- the same one-chunk GEMM forward
without lm_head, so the difference is the tail (output norm in f32, mean, L2: three launches), the copy of the 32
vectors, and the request path (scheduler hand-off, per-request waits).

    python tools/embed_cost.py [--model synthetic:test-8b-v128k:seed=0] [--reps 20] [--out profiles/embeddings.txt]

Both calls end in a stream synchronise, so a host clock around them times the device work plus the host path.
The two are warmed, then timed alternately in one process.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:test-8b-v128k:seed=0")
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from llama_p2p_amd import engine as E

    eng = E.Engine(a.model, n_ctx=a.tokens, n_seq_max=a.prompts)
    rng = np.random.default_rng(0)
    prompts = [np.concatenate([[1], rng.integers(3, eng.n_vocab, a.tokens - 1)]).astype(np.int32)
               for _ in range(a.prompts)]
    slots = np.repeat(np.arange(a.prompts), a.tokens)
    pos = np.tile(np.arange(a.tokens), a.prompts)
    ids = np.concatenate(prompts)

    def t_embed():
        t0 = time.perf_counter()
        out = eng.embed(prompts, pooling=E.POOL_MEAN, normalize=True)
        dt = time.perf_counter() - t0
        assert len(out) == a.prompts and all(np.isfinite(o).all() for o in out)
        return dt

    def t_forward():
        t0 = time.perf_counter()
        eng.forward_rows(slots, pos, ids, want_logits=False)
        return time.perf_counter() - t0

    for _ in range(3):
        t_embed(), t_forward()
    te, tf = [], []
    for _ in range(a.reps):
        te.append(t_embed())
        tf.append(t_forward())
    eng.close()
    ms = lambda v: f"median {statistics.median(v) * 1e3:.3f} ms, min {min(v) * 1e3:.3f} ms, max {max(v) * 1e3:.3f} ms"
    rows = a.prompts * a.tokens
    lines = [
        f"embedding tail cost: {a.model}, {a.prompts} prompts x {a.tokens} tokens = {rows} rows, {a.reps} alternating "
        f"repetitions after 3 warm-up pairs, host clock around calls that end in a stream synchronise",
        f"Engine.embed(MEAN, normalize=True):        {ms(te)}",
        f"forward_rows(want_logits=False), same rows: {ms(tf)}",
        f"difference of the medians: {(statistics.median(te) - statistics.median(tf)) * 1e6:.1f} us "
        f"(of the minima: {(min(te) - min(tf)) * 1e6:.1f} us)",
        f"the tail reads {rows} x {eng.n_embd} x 4 B = {rows * eng.n_embd * 4 / 1e6:.1f} MB of x once and of y once "
        f"(about 10-20 us at HBM rate) in 3 launches",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
