"""BASELINE configs 4 and 5 on their own models, and per-layer parity at full depth (one GPU).

* Per layer (north_star: "logits agree within a stated fp tolerance"): each of the 32 Llama-3-8B
  layers runs as a one-layer stage engine fed the ORACLE's hidden state (f32 x_in / x_out), so every
  layer is checked against the oracle's own output of that layer (oracle.OracleContext.layers =
  orc_layers) without the 32-layer chaotic amplification the end-to-end tests must allow for.  The
  prompt rows go through the engine's prefill path, then one 32-row decode step (wide path: split-K
  slabs, FIN attention) and one 1-row step (persistent GEMVs, RMS_NORM on load); the last layer's
  stage also runs the 128256-token head.  Bar: the bf16 tolerance of every other test, per row.
* Config 4 (Llama-3-8B pipeline-sharded over 2/4/8 stages): all 32 layers split by
  pipeline.partition_layers, S micro-batches of M=32 sequences driven stage by stage in one process
  (the RCCL send/recv is a device copy here; the schedule is tested over gloo on CPU).  With the
  f32 hand-off every stage split gives BITWISE the one-engine logits and greedy tokens; with the
  bf16 hand-off (what the 8-GPU bench sends) the logits stay within the full-depth bar of
  test_baseline_gpu (twice the oracle's own deviation under 1e-6 activation noise).
* Config 5's model (Llama-3-70B bf16, 80 layers) as 8 stages vs the one-engine 70B run, created one
  after the other (141 GB each): bitwise with the f32 hand-off.
"""
import numpy as np
import pytest
import torch

from walk_ref import bf16_tol_rows as _bf16_tol  # the bf16 bar (conftest.logit_tol) row by row

pytestmark = pytest.mark.gpu


def _prompts(vocab, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[1], rng.integers(3, vocab, int(rng.integers(lo, hi)))]).astype(np.int32)
            for _ in range(n)]


def _stage(fn):
    from llama_p2p_amd.engine import torch_stream_handle

    return fn(torch_stream_handle())


def _one_layer_vs_oracle(name, l, ctxs, prompts, xp, xd, last, dev):
    """Layer l of `name` as a one-layer stage engine fed the same inputs as the oracle contexts: the
    prompt rows (`xp`, or their ids at layer 0) through the prefill path, then a 32-row decode step
    (wide path) and a 1-row step (persistent GEMVs, RMS_NORM on load); with `last` also the head.
    Returns (oracle x_out of the prompt rows, of the decode rows, {rows: (max|d|/tol, max|d|)})."""
    from llama_p2p_amd import synth
    from llama_p2p_amd.engine import Engine

    sh = synth.SHAPES[name]
    M = len(prompts)
    slots, pos = [], []
    for i, p in enumerate(prompts):
        slots += [i] * (len(p) - 1)
        pos += list(range(len(p) - 1))
    ids_all = [int(t) for p in prompts for t in p[:-1]]
    dslots, dpos = list(range(M)), [len(p) - 1 for p in prompts]
    eng = Engine(f"synthetic:{name}:seed=0", n_ctx=32, n_seq_max=M, layer_begin=l, layer_end=l + 1, device=0)
    # oracle: this layer on the prompt rows, then on the decode rows (reading the prompt K/V)
    xp_next = [ctxs[i].layers(xp[i], 0, l, l + 1) for i in range(M)]
    od = [ctxs[i].layers(xd[i], dpos[i], l, l + 1, logits=last) for i in range(M)]
    xd_next = np.concatenate([o[0] if last else o for o in od])
    ref_lg = np.concatenate([o[1] for o in od]) if last else None
    # engine: prompt rows fed the oracle's layer input (its K/V then come from the same values)
    x_in = torch.from_numpy(np.concatenate(xp)).to(dev) if l else None
    for c0 in range(0, len(slots), 64):  # mx_stage_rows takes <= 64 rows per call
        c1 = min(len(slots), c0 + 64)
        _stage(lambda s: eng.stage_rows(slots[c0:c1], pos[c0:c1], ids_all[c0:c1] if l == 0 else None,
                                        0 if l == 0 else x_in[c0:c1].data_ptr(), 0, False, s))
    dx = torch.from_numpy(np.concatenate(xd)).to(dev) if l else None
    res = {}
    for rows in (M, 1):
        out = torch.empty((rows, sh.n_embd), dtype=torch.float32, device=dev)
        ids_d = [int(prompts[i][-1]) for i in range(rows)] if l == 0 else None
        lg = _stage(lambda s: eng.stage_rows(dslots[:rows], dpos[:rows], ids_d, 0 if l == 0 else dx[:rows].data_ptr(),
                                             0 if last else out.data_ptr(), last, s))
        torch.cuda.synchronize()
        if last:
            got, ref = lg, ref_lg[:rows]
        else:
            got, ref = out.cpu().numpy(), xd_next[:rows]
        res[rows] = (float((np.abs(got - ref) / _bf16_tol(ref)).max()), float(np.abs(got - ref).max()))
    eng.close()
    return xp_next, xd_next, res


@pytest.mark.timeout(600)
def test_8b_every_layer_vs_oracle(oracle_mod):
    from llama_p2p_amd import synth

    name = "llama3-8b"
    sh = synth.SHAPES[name]
    M = 32
    prompts = _prompts(sh.n_vocab, M, 3, 9, seed=31)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream())
    om = oracle_mod.OracleModel(sh, seed=0)
    ctxs = [om.context(32) for _ in range(M)]
    # oracle layer inputs: prompt rows (all but the last token) and the decode row (the last token)
    xp = [ctxs[i].layers(None, 0, 0, 0, ids=p[:-1]) for i, p in enumerate(prompts)]
    xd = [ctxs[i].layers(None, len(p) - 1, 0, 0, ids=p[-1:]) for i, p in enumerate(prompts)]
    worst = []
    for l in range(sh.n_layer):
        last = l == sh.n_layer - 1
        xp_next, xd_next, res = _one_layer_vs_oracle(name, l, ctxs, prompts, xp, xd, last, dev)
        for rows in (M, 1):
            assert res[rows][0] <= 1.0, f"layer {l}, {rows} rows: max |d|/tol {res[rows][0]:.3f} (max |d| {res[rows][1]:.4g})"
        worst.append((l, res[M][0], res[1][0]))
        print(f"layer {l:2d}{' + head' if last else ''}: max |d|/bf16-tol 32 rows {res[M][0]:.4f} "
              f"(max |d| {res[M][1]:.3g}), 1 row {res[1][0]:.4f}", flush=True)
        xp, xd = xp_next, [xd_next[i:i + 1] for i in range(M)]
    for c in ctxs:
        c.close()
    om.close()
    print("worst layer ratio", max(worst, key=lambda w: max(w[1], w[2])))


@pytest.mark.timeout(900)
def test_70b_sampled_layers_vs_oracle(oracle_mod):
    """Config 5's model against the oracle layer by layer: Llama-3-70B (h 8192, 64 q / 8 kv heads, ff 28672)
    layers 0 (from the token ids), 41 and 79 (+ the 128256-token head), each as a one-layer stage engine
    at 32 and 1 rows.  The host cannot synthesise all 80 layers for the oracle (141 GB), so the oracle
    synthesises only these (orc_fill_synthetic_layers) and layers 41 / 79 take the same seeded random
    residual stream on both sides instead of the output of the layers before them."""
    from llama_p2p_amd import synth

    name = "llama3-70b"
    sh = synth.SHAPES[name]
    M = 32
    prompts = _prompts(sh.n_vocab, M, 3, 7, seed=37)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream())
    om = oracle_mod.OracleModel(sh, seed=None)
    rng = np.random.default_rng(5)
    for l in (0, 41, 79):
        last = l == sh.n_layer - 1
        om.fill_synthetic_layers(0, l, l + 1, globals_=(l == 0 or last))
        ctxs = [om.context(32) for _ in range(M)]
        if l == 0:
            xp = [ctxs[i].layers(None, 0, 0, 0, ids=p[:-1]) for i, p in enumerate(prompts)]
            xd = [ctxs[i].layers(None, len(p) - 1, 0, 0, ids=p[-1:]) for i, p in enumerate(prompts)]
        else:  # a residual stream of the scale the 70B's layers carry (seeded, the same on both sides)
            xp = [rng.normal(0.0, 0.5, (len(p) - 1, sh.n_embd)).astype(np.float32) for p in prompts]
            xd = [rng.normal(0.0, 0.5, (1, sh.n_embd)).astype(np.float32) for _ in prompts]
        _, _, res = _one_layer_vs_oracle(name, l, ctxs, prompts, xp, xd, last, dev)
        print(f"70B layer {l:2d}{' + head' if last else ''}: max |d|/bf16-tol 32 rows {res[M][0]:.4f} "
              f"(max |d| {res[M][1]:.3g}), 1 row {res[1][0]:.4f}", flush=True)
        for rows in (M, 1):
            assert res[rows][0] <= 1.0, f"70B layer {l}, {rows} rows: max |d|/tol {res[rows][0]:.3f} (max |d| {res[rows][1]:.4g})"
        for c in ctxs:
            c.close()
    om.close()


@pytest.mark.timeout(600)
def test_llama2_7b_geometry_sampled_layers_vs_oracle(oracle_mod):
    """A shape with no hand-tuned dispatch: Llama-2-7B (h 4096, 32 kv heads, ff 11008,
    vocab 32000) layers 0 (from the token ids) and 31 (+ the head) as one-layer stage engines at 32 and 1
    rows against the oracle -- the generic paths: gate/up as 344 four-wave groups, ffn_down's K (344
    tiles) split 8 ways into ranges that are not whole chunks (mm_wide_kernel RG), the lm_head as 500
    groups."""
    from llama_p2p_amd import synth

    name = "llama2-7b"
    sh = synth.SHAPES[name]
    M = 32
    prompts = _prompts(sh.n_vocab, M, 3, 7, seed=41)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream())
    om = oracle_mod.OracleModel(sh, seed=None)
    rng = np.random.default_rng(6)
    for l in (0, sh.n_layer - 1):
        last = l == sh.n_layer - 1
        om.fill_synthetic_layers(0, l, l + 1, globals_=True)
        ctxs = [om.context(32) for _ in range(M)]
        if l == 0:
            xp = [ctxs[i].layers(None, 0, 0, 0, ids=p[:-1]) for i, p in enumerate(prompts)]
            xd = [ctxs[i].layers(None, len(p) - 1, 0, 0, ids=p[-1:]) for i, p in enumerate(prompts)]
        else:
            xp = [rng.normal(0.0, 0.5, (len(p) - 1, sh.n_embd)).astype(np.float32) for p in prompts]
            xd = [rng.normal(0.0, 0.5, (1, sh.n_embd)).astype(np.float32) for _ in prompts]
        _, _, res = _one_layer_vs_oracle(name, l, ctxs, prompts, xp, xd, last, dev)
        print(f"Llama-2-7B layer {l:2d}{' + head' if last else ''}: max |d|/bf16-tol 32 rows {res[M][0]:.4f} "
              f"(max |d| {res[M][1]:.3g}), 1 row {res[1][0]:.4f}", flush=True)
        for rows in (M, 1):
            assert res[rows][0] <= 1.0, f"Llama-2-7B layer {l}, {rows} rows: max |d|/tol {res[rows][0]:.3f}"
        for c in ctxs:
            c.close()
    om.close()


def _pipeline_run(path, sh, splits, prompts, S, M, steps, handoff_bf16, n_ctx=64):
    """Stage engines for `splits` (one split = one engine), S micro-batches x M sequences driven stage
    by stage: the prompt rows in 64-row chunks, a teacher-free first decode step whose last-stage logits
    are returned, then `steps` device greedy steps per micro-batch (each stage's decode graph, the last
    stage's argmax fed back to stage 0).  Returns (first-step logits [S*M][V], tokens [S*M][steps+1])."""
    from llama_p2p_amd.engine import Engine
    from llama_p2p_amd.pipeline import EngineAdapter

    dev = torch.device("cuda", 0)
    engs = [Engine(path, n_ctx=n_ctx, n_seq_max=S * M, layer_begin=lb, layer_end=le, device=0,
                   handoff_bf16=handoff_bf16) for lb, le in splits]
    ads = [EngineAdapter(e) for e in engs]
    n = len(engs)
    dt = torch.bfloat16 if handoff_bf16 else torch.float32
    slots, pos, ids = [], [], []
    for i, p in enumerate(prompts):
        slots += [i] * (len(p) - 1)
        pos += list(range(len(p) - 1))
        ids += [int(t) for t in p[:-1]]
    buf = [torch.empty((64, sh.n_embd), dtype=dt, device=dev) for _ in range(n)]
    for i in range(0, len(slots), 64):
        k = min(64, len(slots) - i)
        for s in range(n):
            ads[s].stage_rows_tensors(slots[i:i + k], pos[i:i + k], ids[i:i + k] if s == 0 else None,
                                      buf[s - 1][:k] if s > 0 else None, buf[s][:k] if s < n - 1 else None)
    logits = []
    first = []
    for mb in range(S):
        rows = list(range(mb * M, (mb + 1) * M))
        dp, di = [len(prompts[r]) - 1 for r in rows], [int(prompts[r][-1]) for r in rows]
        x = None
        for s in range(n):
            if s < n - 1:
                out = torch.empty((M, sh.n_embd), dtype=dt, device=dev)
                _stage(lambda st: engs[s].stage_rows(rows, dp, di if s == 0 else None, x.data_ptr() if x is not None else 0,
                                                     out.data_ptr(), False, st))
                x = out
            else:
                lg = _stage(lambda st: engs[s].stage_rows(rows, dp, di if s == 0 else None,
                                                          x.data_ptr() if x is not None else 0, 0, True, st))
        logits.append(lg)
        first.append([int(np.argmax(r)) for r in lg])
    batches, toks = [], []
    for mb in range(S):
        rows = list(range(mb * M, (mb + 1) * M))
        bp = [len(prompts[r]) for r in rows]
        bs = [ads[s].batch(rows, bp, first[mb] if s == 0 else None, steps if s == n - 1 else 0) for s in range(n)]
        tok = torch.tensor(first[mb], dtype=torch.int32, device=dev)
        bs[0].bind_ids_tensor(tok)
        if n > 1:
            bs[-1].bind_ids_tensor(torch.zeros(M, dtype=torch.int32, device=dev))
        batches.append(bs)
        toks.append(tok)
    xs = [torch.empty((M, sh.n_embd), dtype=dt, device=dev) for _ in range(n)]
    for _ in range(steps):
        for mb in range(S):
            for s in range(n):
                batches[mb][s].step_tensors(xs[s - 1] if s > 0 else None, xs[s] if s < n - 1 else None)
            if n > 1:
                toks[mb].copy_(batches[mb][-1]._ids_tensor)
    torch.cuda.synchronize()
    tokens = np.concatenate([np.concatenate([np.asarray(first[mb])[:, None], batches[mb][-1].tokens()], 1)
                             for mb in range(S)])
    for bs in batches:
        for b in bs:
            b.close()
    for e in engs:
        e.close()
    return np.concatenate(logits), tokens


@pytest.mark.timeout(600)
def test_config4_8b_stage_splits_bitwise():
    from llama_p2p_amd import synth
    from llama_p2p_amd.pipeline import partition_layers

    name = "llama3-8b"
    sh = synth.SHAPES[name]
    path = f"synthetic:{name}:seed=0"
    torch.cuda.set_stream(torch.cuda.Stream())
    M, S, steps = 32, 2, 6
    prompts = _prompts(sh.n_vocab, S * M, 4, 40, seed=41)
    layer = 2 * (2 * sh.n_embd ** 2 + 2 * sh.n_embd * sh.n_embd_kv + 3 * sh.n_embd * sh.n_ff)
    ref_lg, ref_tok = _pipeline_run(path, sh, [(0, sh.n_layer)], prompts, S, M, steps, False)
    for n in (2, 4, 8):
        splits = partition_layers(sh.n_layer, layer, 2 * sh.n_vocab * sh.n_embd, n)
        lg, tok = _pipeline_run(path, sh, splits, prompts, S, M, steps, False)
        assert np.array_equal(lg, ref_lg), f"{n} stages {splits}: logits differ (max |d| {np.abs(lg - ref_lg).max()})"
        assert np.array_equal(tok, ref_tok), f"{n} stages {splits}: tokens differ"
        print(f"{n} stages {splits}: f32 hand-off bitwise == one engine ({S}x{M} sequences, {steps + 1} tokens)")


@pytest.mark.timeout(600)
def test_config4_8b_bf16_handoff_within_full_depth_bar(oracle_mod):
    from llama_p2p_amd import synth
    from llama_p2p_amd.pipeline import partition_layers

    name = "llama3-8b"
    sh = synth.SHAPES[name]
    path = f"synthetic:{name}:seed=0"
    torch.cuda.set_stream(torch.cuda.Stream())
    M, S, steps = 32, 1, 2
    prompts = _prompts(sh.n_vocab, S * M, 6, 14, seed=43)
    layer = 2 * (2 * sh.n_embd ** 2 + 2 * sh.n_embd * sh.n_embd_kv + 3 * sh.n_embd * sh.n_ff)
    ref_lg, _ = _pipeline_run(path, sh, [(0, sh.n_layer)], prompts, S, M, steps, False)
    # the oracle's own deviation under 1e-6 relative activation noise (test_baseline_gpu's bar), 3 rows
    om = oracle_mod.OracleModel(sh, seed=0)
    base = [om.context(64).eval(prompts[i], 0) for i in (0, 11, 22)]
    oracle_mod.q8_jitter(1e-6)
    try:
        self_dev = max(float(np.abs(om.context(64).eval(prompts[i], 0) - b).max()) for i, b in zip((0, 11, 22), base))
    finally:
        oracle_mod.q8_jitter(0.0)
    om.close()
    scale = float(np.abs(ref_lg).max())
    for n in (2, 8):
        splits = partition_layers(sh.n_layer, layer, 2 * sh.n_vocab * sh.n_embd, n)
        lg, _ = _pipeline_run(path, sh, splits, prompts, S, M, steps, True)
        d = float(np.abs(lg - ref_lg).max())
        same = int((lg.argmax(-1) == ref_lg.argmax(-1)).sum())
        print(f"{n} stages, bf16 hand-off: max |d| {d:.4g} vs the f32 one-engine logits; oracle self-deviation "
              f"{self_dev:.4g}; greedy picks equal {same}/{len(lg)}")
        assert d <= 2 * self_dev + 1e-4 * scale, (d, self_dev)
        assert same >= 0.85 * len(lg)


@pytest.mark.timeout(900)
def test_config5_70b_eight_stages_bitwise():
    from llama_p2p_amd import synth
    from llama_p2p_amd.pipeline import partition_layers

    name = "llama3-70b"
    sh = synth.SHAPES[name]
    path = f"synthetic:{name}:seed=0"
    torch.cuda.set_stream(torch.cuda.Stream())
    M, S, steps = 32, 1, 3
    prompts = _prompts(sh.n_vocab, S * M, 4, 20, seed=47)
    ref_lg, ref_tok = _pipeline_run(path, sh, [(0, sh.n_layer)], prompts, S, M, steps, False, n_ctx=32)
    layer = 2 * (2 * sh.n_embd ** 2 + 2 * sh.n_embd * sh.n_embd_kv + 3 * sh.n_embd * sh.n_ff)
    splits = partition_layers(sh.n_layer, layer, 2 * sh.n_vocab * sh.n_embd, 8)
    lg, tok = _pipeline_run(path, sh, splits, prompts, S, M, steps, False, n_ctx=32)
    assert np.array_equal(lg, ref_lg), f"70B 8 stages {splits}: max |d| {np.abs(lg - ref_lg).max()}"
    assert np.array_equal(tok, ref_tok)
    print(f"70B 8 stages {splits}: bitwise == one engine ({M} sequences, {steps + 1} tokens)")
