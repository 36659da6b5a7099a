"""bench.py's plain run, --full and --dump-outputs.

A plain `bench.py --gpus 1 --steps K --warmup W` times the K decode steps and prints the headline
line only; the roofline and every other section need --full.  --dump-outputs DIR writes the token
ids the timed batch returned (float32 .npy); the inputs are seeded, so two runs with the same
arguments write the same arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "batch1", "prefill", "serving", "serving_default_sampling", "cpu_baseline", "tinyllama",
             "hbm_probe", "q8_0", "q4_k_m", "q4_0", "llama3_70b", "llama2_7b_geometry", "section_seconds")


def _bench(*args, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + list(args), capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must be one JSON line, got {len(lines)}: {p.stdout[:2000]}"
    return json.loads(lines[0])


def _dump(d):
    toks, last = np.load(os.path.join(d, "tokens.npy")), np.load(os.path.join(d, "last_step.npy"))
    assert sorted(os.listdir(d)) == ["last_step.npy", "tokens.npy"]
    assert toks.dtype == np.float32 and last.dtype == np.float32
    assert np.array_equal(last, toks[..., -1])
    assert np.array_equal(toks, np.round(toks)) and toks.min() >= 0
    return toks


def test_dump_outputs_pipeline_dry_run(tmp_path):
    """The pipeline path (CPU stand-in engine): [micro-batches, sequences, warm-up + steps], twice the same."""
    common = ["--gpus", "1", "--force-pipeline", "--micro-batches", "2", "--dry-run", "--steps", "5", "--warmup", "2",
              "--seqs", "3"]
    a = _bench(*common, "--dump-outputs", str(tmp_path / "a"))
    _bench(*common, "--dump-outputs", str(tmp_path / "b"))
    ta, tb = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert ta.shape == (2, 3, 7)
    assert np.array_equal(ta, tb)
    assert a["steps"] == 5 and a["ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_its_tokens(tmp_path):
    common = ["--gpus", "1", "--model", "test-d128", "--seqs", "5", "--steps", "6", "--warmup", "2"]
    a = _bench(*common, "--dump-outputs", str(tmp_path / "a"))
    _bench(*common, "--dump-outputs", str(tmp_path / "b"))
    for k in HEADLINE:
        assert k in a, k
    assert not [k for k in FULL_ONLY if k in a]
    assert a["steps"] == 6 and a["warmup"] == 2 and a["unit"] == "tokens/s" and a["higher_is_better"] is True
    # value = sequences x steps / timed seconds, ms_per_step = timed seconds / steps (both rounded in the line)
    assert a["value"] == pytest.approx(5 / (a["ms_per_step"] * 1e-3), rel=1e-2)
    ta, tb = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert ta.shape == (5, 8)
    assert np.array_equal(ta, tb)



@pytest.mark.gpu
def test_steps_beyond_n_ctx_rearm_the_batch(tmp_path):
    """--steps sets the number of timed steps even past n_ctx: the batch is re-armed at the prompts' ends
    whenever the longest sequence reaches n_ctx, so the dumped tokens repeat with that period."""
    import bench
    from llama_p2p_amd import synth

    n_ctx, seqs, steps, warmup = 300, 5, 100, 3
    prompts = bench.make_prompts(synth.SHAPES["test-d128"].n_vocab, seqs)
    cycle = n_ctx - max(len(p) - 1 for p in prompts)
    assert 1 <= cycle < steps  # the run below crosses n_ctx at least once
    common = ["--gpus", "1", "--model", "test-d128", "--seqs", str(seqs), "--n-ctx", str(n_ctx), "--steps", str(steps),
              "--warmup", str(warmup)]
    a = _bench(*common, "--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == steps and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(seqs / (a["ms_per_step"] * 1e-3), rel=1e-2)
    ta = _dump(tmp_path / "a")
    assert ta.shape == (seqs, warmup + steps)
    assert np.array_equal(ta[:, cycle:], ta[:, :-cycle])
    # the first cycle is what a run that stays inside n_ctx computes
    assert cycle > warmup
    short = ["--gpus", "1", "--model", "test-d128", "--seqs", str(seqs), "--n-ctx", str(n_ctx), "--steps",
             str(cycle - warmup), "--warmup", str(warmup)]
    _bench(*short, "--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(_dump(tmp_path / "b"), ta[:, :cycle])
