#!/usr/bin/env python3
"""Bit-level digests of the engine's layer walks, for comparing two builds of the library (a refactor of the
walks must leave every output the same bits; the oracle tolerances of tests/test_layer_walk_gpu.py cannot show that).

    python tools/walk_digest.py > run.txt                          one line per case and output, on the GPU
    python tools/walk_digest.py --table a1.txt a2.txt b.txt        three-column table: the old build twice, the new

The cases are those of tests/walk_ref.py: the models of test_layer_walk_gpu.py (bf16, q8_0, q4_0, q4_k_m, q5_k_m on
test-d128 and test-tiny, the Q4_0 GGUF with a Q6_K output), 1, 4, 5, 16, 17, 32, 33, 64 rows in the distinct and the
one-sequence layout, and the blocked chunk of 80 rows.  Per case, the first 16 hex digits of the SHA-256 of
  logits   forward_rows, every row
  hidden   x_out of stage_rows (the 80-row chunk: stage_rows_pick)
  picks    the tokens of stage_rows_pick on a rowmap subset (every other row and the last; the last row of each
           prompt of the chunk)
  loop     six steps of Engine.batch (distinct rows only)
Every case first stores its own histories, so a line does not depend on the cases before it beyond the K/V they
left in slots it overwrites.  --table drops the cases whose digests differ between the first two files (not
run-to-run stable) and compares the rest with the third.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CTX, N_SLOTS = 128, 64
ROWS = (1, 4, 5, 16, 17, 32, 33, 64)
CHUNK = 80


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def run():
    import torch
    import walk_ref as W
    from llama_p2p_amd import engine, gguf, synth

    engine.lib()
    dev = torch.device("cuda", 0)
    models = [(f, s) for s in ("test-d128", "test-tiny") for f in W.FORMATS] + [(W.GGUF_Q4_0, "test-d128")]
    tmp = tempfile.mkdtemp()
    for fmt, name in models:
        sh = synth.SHAPES[name]
        if fmt == W.GGUF_Q4_0:
            path = os.path.join(tmp, f"{name}_q4_0.gguf")
            gguf.write_synthetic_gguf(path, sh, seed=6, wtype="q4_0")
        else:
            path = W.model_path(fmt, name)
        eng = engine.Engine(path, n_ctx=N_CTX, n_seq_max=N_SLOTS, device=0)

        def prefill(hist):
            for c in range(0, len(hist[0]), 64):
                eng.forward_rows(*[a[c:c + 64] for a in hist], want_logits=False)

        def hidden(new, pick):
            out = torch.full((len(new[0]), sh.n_embd), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            if pick:
                eng.stage_rows_pick(*new, x_out=out.data_ptr())
            else:
                eng.stage_rows(*new, x_out=out.data_ptr())
            return out.cpu().numpy()

        def emit(layout, M, what, a):
            print(f"{fmt}-{name}/{layout}-{M}/{what} {sha(a)}", flush=True)

        for layout in ("distinct", "one"):
            for M in ROWS:
                hist, new, _ = W.layout_rows(sh, layout, M)
                prefill(hist)
                emit(layout, M, "logits", eng.forward_rows(*new))
                prefill(hist)
                emit(layout, M, "hidden", hidden(new, False))
                prefill(hist)
                rowmap = sorted(set(range(0, M, 2)) | {M - 1})
                emit(layout, M, "picks", np.asarray(eng.stage_rows_pick(*new, rowmap=rowmap), dtype=np.int32))
                if layout == "distinct":
                    prefill(hist)
                    b = eng.batch(slots=new[0], pos=new[1], ids=new[2], max_steps=6)
                    for _ in range(6):
                        b.step()
                    emit(layout, M, "loop", np.asarray(b.tokens(), dtype=np.int32))
                    b.close()
        new, spans, _ = W.blocked_case(sh, CHUNK, N_CTX)
        emit("blocked", CHUNK, "hidden", hidden(new, True))
        emit("blocked", CHUNK, "picks",
             np.asarray(eng.stage_rows_pick(*new, rowmap=[b - 1 for _, b in spans]), dtype=np.int32))
        eng.close()


def table(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(dict(line.split() for line in f if line.strip()))
    a1, a2, b = runs
    assert a1.keys() == a2.keys() == b.keys(), "the runs do not hold the same cases"
    unstable = [k for k in a1 if a1[k] != a2[k]]
    differ = [k for k in a1 if k not in unstable and a1[k] != b[k]]
    print(f"# {len(a1)} digests, {len(unstable)} dropped as not run-to-run stable, {len(a1) - len(unstable)} compared, "
          f"{len(differ)} differ")
    print(f"# {'case':44s} {'old build, run 1':16s} {'old build, run 2':16s} {'new build':16s}")
    for k in a1:
        mark = "  UNSTABLE" if k in unstable else "  DIFFERS" if k in differ else ""
        print(f"{k:46s} {a1[k]} {a2[k]} {b[k]}{mark}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--table":
        sys.exit(table(sys.argv[2:]))
    run()
