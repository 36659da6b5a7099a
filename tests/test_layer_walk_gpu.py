"""Every branch of the engine's layer walks (engine.cpp enqueue_forward: the <= 16-row walk, enqueue_forward_wide,
_quant (Q8_0 / Q4_0 and K-quants), _gemm) against the CPU oracle, through whole two-layer models.

The kernels are tested alone elsewhere; this file tests what the walks decide between them: which operand a GEMV
gets (normed / quantised on load from the residual stream's sum-of-squares partials, or by a launch), whether
attn_output / ffn_down leave split-K slabs and who folds them into x (the next layer's norm, the end of the walk,
the head), whether the attention finishes q|k|v from slabs (rows_distinct) or launch_qkv_finish does, whether the
prefill attention runs (rows_blocked), and whether the head sees every row or a rowmap subset.  Those are whole-row
mistakes (a slab never folded, stale partials, the wrong row), which only a whole-model run can see.

Models: bf16, q8_0, q4_0, q4_k_m, q5_k_m as synthetic:<shape>:seed=0[:<format>] on test-d128 and test-tiny (two
layers: layer 0's ffn_down slabs are folded by layer 1's attention norm, layer 1's at the end of the walk), and a
Q4_0 GGUF with a Q6_K output on test-d128 (out_kq_head).  One engine and one oracle per model for the module.

Row counts 1, 2, 4, 5, 16, 17, 24, 32, 33, 64 and chunks of 65, 80, 272 rows, in four layouts (tests/walk_ref.py):
distinct (every row its own slot, histories of 3 + (5 i mod 40) tokens), one (consecutive positions of one slot),
mixed (three slots, several consecutive rows each: neither distinct nor blocked) and blocked (the scheduler's
layout through stage_rows_pick).  Outputs: logits of every row (forward_rows), picks of a rowmap subset
(stage_rows_pick: the oracle's argmax wherever its top-1/top-2 gap exceeds twice the tolerance), the hidden state
alone (x_out), the hidden state in (a second engine with layer_begin = 1 fed the oracle's layer-0 output, f32 and
bf16 hand-off), and the device greedy loop (Engine.batch, 6 steps).

Reached branches, asserted on the CPU from mx_matmul_plan / mx_q8_matmul_plan / mx_kq_matmul_plan before anything
is launched (walk_ref.walk_facts against expect() below; the "walk" key of both restates enqueue_forward's
conditions on the row count and prefill_gemm and only names the branch -- the on-load, gemm_shapes and slab facts
come from the plan functions):
  bf16      RMS_NORM on load at <= 4 rows on test-d128 (h 256 of test-tiny is below mm_can_norm_on_load: the norm
            launch there); wide walk at > 16 rows with 2 / 2 / 4 slabs (q|k|v, attn_output, ffn_down) on test-d128
            and 1 / 1 / 1 on test-tiny; GEMM walk at 65, 80, 272; through stage_rows_pick (prefill_gemm) the
            full-chain wide walk at every count <= 64 (one K range, handed over as one slab each: the picks at 4..64
            rows reach the fold before the rowmap norm with that slab pending), with the prefill attention at
            blocked 32 / 64.
  q8_0/q4_0 quantise on load at <= 4 rows, launches at 5+; slab forms at 17..32 rows: 1 / 1 / 2 slabs on test-d128,
            1 / 1 / 1 on test-tiny; in place at 33+; prefill attention at blocked 80 / 272.
  K-quants  quantise on load at 1 row only (mkq_can_quantize_on_load), launches at 2+; slabs at 17..32 rows: q|k|v 1
            and ffn_down 2 on test-d128, q|k|v 1 on test-tiny; the dequantised-GEMM walk at > 64 rows, without a
            head (hidden state out) and with the K-quant head on a rowmap (the picks of the 65-, 80-, 272-row cases).
Unreachable at these shapes, and why: the row-tile-persistent GEMVs (mm_pers_supported / the K-quant bd_tile and
pers kernels need Llama-sized tile counts: covered by the kernel tests and the 8B-shaped whole-model tests);
K-quant attn_output slabs (K 1024 / 256 holds too few super-blocks to split); K-quant ffn_down slabs on test-tiny
(K 512); the fold-first branch of the K-quant norm (h > 4096); the multi-slab (2 / 2 / 4) bf16 wide walk with a
rowmap head, and forward_rows_chunk's last_row_only head: a rowmap reaches the walks only through stage_rows_pick,
whose prefill_gemm turns bf16 to the full-chain form, and no exported call sets last_row_only; a head together with
x_out: forward_rows_chunk and mx_batch_step run the head only when x_out is null.  Rowmap results are tokens only
(stage_rows_pick returns no logits), so they are judged by the argmax rule, not bitwise.

Bounds, none new: bf16 logits conftest.logit_tol; hidden states the row-wise bf16 bar of
test_fulldepth_stages_gpu.py; quantised formats what their own whole-model tests use -- q8_0 and the K-quants the
bf16 tolerance and twice the oracle's self-deviation under oracle.q8_jitter(1e-6) (walk_ref.jitter_bound), q4_0 the
jitter bound and the decided-argmax rule of test_q4_0_gpu.py.  The self-deviation is taken once per model over the
file's sequence pool (every position of the 64 distinct sequences and the one-sequence chunk): a one-row case has
too few roundings to flip for its own figure to mean anything, and larger cases are no safer -- over the sequences
of single cases of 64 to 272 rows the oracle's hidden-state figure ranges from 0.0002 (q8_0 test-tiny, the blocked
80-row case: four short prompts in which the noise flips next to nothing) to 0.0031 on the same model, against
0.0024 over the pool.  The sensitivity is a property of the model; about 1700 positions estimate it, 80 may not.

Self-consistency (bf16, bitwise): a row's logits at a given row count are the same bits through forward_rows with
distinct rows and as the last row of a one-sequence chunk of as many rows with the same history; the device greedy
loop's first step leaves the same bits in x and in the head's operand xn as forward_rows of the same rows (the head
is the same launch on that operand; a batch returns no logits), and picks, step by step, the argmax of forward_rows
at the same row count.  Printed, not asserted, for the quantised formats (their walks keep per-row-count K splits).

Poison: K/V positions past each slot's used length are still zero bits after everything this module ran; calls
return exactly the rows they were asked for.

Measured on MI355X, worst |d| / bound over all cases (every case prints its own): bf16 0.286; q8_0 0.973 (the
row-wise bf16 bar on the hidden state of the blocked 272-row chunk, test-d128; 0.70 of the jitter bound); q4_0
0.665; q4_k_m 0.673; q5_k_m 0.661; the K-quant GEMM walk against the dequantised-weights oracle 0.723 (the 65-row
chunk, whose 3-token history was stored by the Q8_K walk; 0.12-0.15 for the blocked chunks).  bf16: the
self-consistency comparisons are bit-equal at every row count.  Quantised formats, printed: a distinct row and the
last row of a one-sequence chunk have the same bits at 5, 16, 33 and 64 rows in every model, and at 17 / 32 rows (the
slab forms: the attention finishes q|k|v from slabs for distinct rows, launch_qkv_finish otherwise) they differ in
every logit, max |d| 0.009-0.024, for q8_0 and q4_0 on test-d128 at 17 and 32, q4_k_m and q5_k_m on test-d128 at 32
and q8_0 on test-tiny at 32, and are equal elsewhere; the loop's picks equal forward_rows' argmax in every case, and
x after the loop's first step has forward_rows' bits except, in those same cases (and q5_k_m test-d128 at 17), in
row 0, whose history the one-sequence chunk run in between had just rewritten.

Mutations tried on scratch copies of engine.cpp (values only; none committed), each run against this file, with the
first test that failed:
  enqueue_forward_quant's end-of-walk fold skipped when rowmap is set (a Q8_0 model) -> test_picks_of_a_rowmap_subset[q8_0-test-d128-mixed-17]
  operand() handed nullptr for the q8 head's rmap -> test_picks_of_a_rowmap_subset[q8_0-test-d128-one-17]
  b.ssq / d.ssq left null on the <= 4-row q8 walk -> test_logits_of_every_row[q8_0-test-d128-distinct-1]
  nslab not reset after the folding norm in quant_operand (a K-quant model) -> test_logits_of_every_row[q4_k_m-test-d128-distinct-17]
  the rows_distinct tests inverted in enqueue_forward_wide -> test_logits_of_every_row[bf16-test-d128-distinct-4]
    (its 42 history rows of four slots are one wide forward)
  launch_f32_in given a null ssq -> test_hidden_state_in[bf16-test-d128-f32-1]
"""
import os

import numpy as np
import pytest

import kv_layout as KL
import walk_ref as W
from conftest import assert_tokens_match, check_chain_batched, logit_tol

pytestmark = pytest.mark.gpu

N_CTX, N_SLOTS = 128, 64
SHAPES = ("test-d128", "test-tiny")
MODELS = [(f, s) for s in SHAPES for f in W.FORMATS] + [(W.GGUF_Q4_0, "test-d128")]
MODEL_IDS = [f"{f}-{s}" for f, s in MODELS]
ROWS = (1, 2, 4, 5, 16, 17, 24, 32, 33, 64)


def expect(fmt, shape_name, M, prefill_gemm=False):
    """The branch a forward of M rows must take (module docstring), to be compared with walk_ref.walk_facts.
    prefill_gemm: the call goes through stage_rows_pick."""
    fmt = "q4_0" if fmt == W.GGUF_Q4_0 else fmt
    fam, d128 = W.family(fmt), shape_name == "test-d128"
    if fam == "bf16":
        if prefill_gemm and M <= 64:  # one K range per GEMV, still handed over as one slab each
            return {"walk": "wide_full_chain", "gemm_shapes": True, "on_load": False, "slabs": (1, 1, 1)}
        walk = "gemm" if M > 64 else "wide" if M > 16 else "rows16"
        slabs = ((2, 2, 4) if d128 else (1, 1, 1)) if walk == "wide" else (0, 0, 0)
        return {"walk": walk, "gemm_shapes": True, "on_load": d128 and M <= 4, "slabs": slabs}
    if fam == "q8":
        return {"walk": "q8", "on_load": M <= 4, "slabs": ((1, 1, 2) if d128 else (1, 1, 1)) if 16 < M <= 32 else (0, 0, 0)}
    return {"walk": "kq_gemm" if M > 64 else "kq", "on_load": M == 1,
            "slabs": ((1, 0, 2) if d128 else (1, 0, 0)) if 16 < M <= 32 else (0, 0, 0)}


class Guarded:
    """An Engine (or Batch) whose calls end the session on a HIP runtime error: after a GPU fault nothing more is
    launched (the StopOnHipError pattern of tests/test_matmul_kernel_gpu.py)."""

    def __init__(self, obj, mx):
        self._o, self._mx = obj, mx

    def __getattr__(self, name):
        attr = getattr(self._o, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            try:
                r = attr(*a, **kw)
            except self._mx.MxError as err:
                if err.code == self._mx.MX_ERR_HIP:
                    pytest.exit(f"HIP error, nothing more is launched: {err}", returncode=3)
                raise
            return Guarded(r, self._mx) if isinstance(r, self._mx.Batch) else r

        return call


class Models:
    """Engines, oracles and each slot's used K/V length, per model, for the module."""

    def __init__(self, O, tmp):
        from llama_p2p_amd import engine

        engine.lib()
        self.mx, self.O, self.tmp = engine, O, tmp
        self.engines, self.refs, self.refs_deq, self.used = {}, {}, {}, {}
        assert "MX_NO_WIDE" not in os.environ and "MX_NO_PERS" not in os.environ

    def shape(self, model):
        from llama_p2p_amd import synth

        return synth.SHAPES[model[1]]

    def path(self, model):
        fmt, name = model
        if fmt != W.GGUF_Q4_0:
            return W.model_path(fmt, name)
        from llama_p2p_amd import gguf

        p = str(self.tmp / f"{name}_q4_0.gguf")
        if not os.path.exists(p):
            gguf.write_synthetic_gguf(p, self.shape(model), seed=6, wtype="q4_0")
        return p

    def engine(self, model, layer_begin=0, handoff_bf16=False):
        key = (model, layer_begin, handoff_bf16)
        if key not in self.engines:
            e = self.mx.Engine(self.path(model), n_ctx=N_CTX, n_seq_max=N_SLOTS, layer_begin=layer_begin, device=0,
                               handoff_bf16=handoff_bf16)
            self.engines[key] = Guarded(e, self.mx)
            self.used[key] = {}
        return self.engines[key]

    def ref(self, model):
        if model not in self.refs:
            fmt, name = model
            sh = self.shape(model)
            if fmt == W.GGUF_Q4_0:
                path = self.path(model)
                make = lambda: W.oracle_from_q4_0_gguf(self.O, path, sh)  # noqa: E731
            else:
                make = lambda: W.oracle_model(self.O, fmt, sh)  # noqa: E731
            self.refs[model] = W.Reference(self.O, make, sh, N_CTX)
        return self.refs[model]

    def ref_dequantised(self, model):
        """A K-quant model's oracle for the dequantised-GEMM walk (walk_ref.oracle_kq_dequantised)."""
        if model not in self.refs_deq:
            fmt, sh = model[0], self.shape(model)
            self.refs_deq[model] = W.Reference(self.O, lambda: W.oracle_kq_dequantised(self.O, fmt, sh), sh, N_CTX)
        return self.refs_deq[model]

    def note(self, model, rows, layer_begin=0, handoff_bf16=False):
        u = self.used[(model, layer_begin, handoff_bf16)]
        for s, p in zip(rows[0], rows[1]):
            u[s] = max(u.get(s, 0), p + 1)

    def close(self):
        for e in self.engines.values():
            e.close()
        for r in list(self.refs.values()) + list(self.refs_deq.values()):
            r.close()


@pytest.fixture(scope="module")
def models(oracle_mod, tmp_path_factory):
    m = Models(oracle_mod, tmp_path_factory.mktemp("walk"))
    yield m
    m.close()


def check(models, model, got, ref, what, hidden=False):
    """got vs the oracle under the model's bound (module docstring); prints the worst |d| / bound."""
    fmt = "q4_0" if model[0] == W.GGUF_Q4_0 else model[0]
    assert got.shape == ref.shape, f"{what}: {got.shape} returned, {ref.shape} asked for"
    assert np.isfinite(got).all(), f"{what}: non-finite values in rows {np.nonzero(~np.isfinite(got).all(axis=1))[0].tolist()}"
    d = np.abs(got - ref)
    ratios = {}
    if fmt != "q4_0":
        tol = W.bf16_tol_rows(ref) if hidden else logit_tol(ref)
        ratios["bf16"] = d / tol
    if fmt != "bf16":
        dev = models.ref(model).self_deviation()[1 if hidden else 0]
        ratios["jitter"] = d / W.jitter_bound(dev, ref)
    print(f"{what}: worst |d| / bound " + ", ".join(f"{k} {float(r.max()):.3f}" for k, r in ratios.items()) +
          f" (max |d| {float(d.max()):.4g}, max |ref| {float(np.abs(ref).max()):.4g})")
    for k, r in ratios.items():
        bad = np.nonzero((r > 1.0).any(axis=1))[0]
        assert bad.size == 0, f"{what}: rows {bad.tolist()} outside the {k} bound, worst {float(r.max()):.3f} x"
    if not hidden:
        if fmt == "q4_0":
            srt = np.sort(ref, axis=-1)
            bar = 2 * np.maximum(1e-2 * np.abs(srt[:, -1]) + 2e-2 * np.abs(ref).max(), 2 * dev)
            bad = ((srt[:, -1] - srt[:, -2]) > bar) & (got.argmax(-1) != ref.argmax(-1))
            assert not bad.any(), f"{what}: argmax differs at decided rows {np.nonzero(bad)[0].tolist()}"
        else:
            assert_tokens_match(got, ref, what)


def prefill(models, model, eng, hist):
    """The histories, in calls of <= 64 rows: larger chunks would take the GEMM walk, whose K-quant form computes
    with bf16 activations, not the oracle's Q8_K rows."""
    for c in range(0, len(hist[0]), 64):
        assert eng.forward_rows(*[a[c:c + 64] for a in hist], want_logits=False) is None
    models.note(model, hist)


def ref_rows(models, model, seqs, new, hidden=False, dequantised=False):
    """The oracle's rows for the new rows of a layout, in row order."""
    r = models.ref_dequantised(model) if dequantised else models.ref(model)
    by_slot = {slot: ((r.hidden if hidden else r.logits)(s), p0) for slot, s, p0 in seqs}
    return np.stack([by_slot[s][0][p] for s, p in zip(new[0], new[1])])


def layout_facts(layout, new):
    distinct, blocked = W.is_distinct(new[0]), W.is_blocked(*new)
    if layout == "distinct":
        assert distinct
    elif layout == "blocked":
        assert blocked and not distinct
    else:  # one sequence or mixed: launch_qkv_finish, rows attending to each other's new K/V
        assert not distinct or len(new[0]) == 1
        if layout == "mixed":
            assert not blocked
    return distinct, blocked


CASES = [(lay, M) for lay in ("distinct", "one", "mixed") for M in ROWS if lay != "mixed" or M >= 6]


@pytest.mark.parametrize("layout,M", CASES, ids=[f"{lay}-{M}" for lay, M in CASES])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_logits_of_every_row(models, model, layout, M):
    sh = models.shape(model)
    assert W.walk_facts(model[0], sh, M) == expect(model[0], model[1], M)
    hist, new, seqs = W.layout_rows(sh, layout, M)
    layout_facts(layout, new)
    ref = ref_rows(models, model, seqs, new)
    eng = models.engine(model)
    prefill(models, model, eng, hist)
    got = eng.forward_rows(*new)
    models.note(model, new)
    check(models, model, got, ref, f"{model[0]} {model[1]} {layout} M={M}")


HIDDEN_CASES = [(lay, M) for lay in ("distinct", "one") for M in ROWS] + [("mixed", 24), ("one", 65)] + \
               [("blocked", M) for M in (32, 64, 80, 272)]


@pytest.mark.parametrize("layout,M", HIDDEN_CASES, ids=[f"{lay}-{M}" for lay, M in HIDDEN_CASES])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_hidden_state_out(models, model, layout, M):
    """No head: x after the last layer (every pending slab folded at the end of the walk).  <= 64 unblocked rows
    through stage_rows; the 65-row chunk and the blocked layouts through stage_rows_pick, which sets prefill_gemm:
    bf16 takes the full-chain wide walk (<= 64 rows) or the GEMM walk with the prefill attention, the K-quants the
    dequantised GEMM walk at > 64 rows, Q8_0 / Q4_0 their own walk with the prefill attention at > 64 rows.

    The K-quant GEMM walk computes with bf16 activations over weights dequantised to bf16 (llama.cpp's GPU route
    for large batches; MX_KQ_GGML_PREFILL=1 keeps ggml's arithmetic), so its reference is the oracle holding those
    bf16 weights (walk_ref.oracle_kq_dequantised), under the row-wise bf16 bar.  Against the format's own oracle,
    whose MUL_MATs round every activation row to Q8_K, the same hidden states lie at up to 2.63 x that bar (q5_k_m
    test-d128, the 65-row chunk; 1.18 x for q4_k_m): the distance between the two arithmetics, printed per case."""
    import torch

    sh = models.shape(model)
    fam = W.family("q4_0" if model[0] == W.GGUF_Q4_0 else model[0])
    pg = layout == "blocked" or M > 64  # through stage_rows_pick
    facts = W.walk_facts(model[0], sh, M, pg)
    assert facts == expect(model[0], model[1], M, pg)
    if layout == "blocked":
        new, spans, prompts = W.blocked_case(sh, M, N_CTX)
        hist, seqs = ([], [], []), [(k, p, 0) for k, p in enumerate(prompts)]
        keep = [r for a, b in spans for r in range(a, b)]  # the padding rows are not results
        assert facts.get("gemm_shapes", True)
    else:
        hist, new, seqs = W.layout_rows(sh, layout, M)
        keep = list(range(M))
    layout_facts(layout, new)
    ref = ref_rows(models, model, seqs, [[new[0][r] for r in keep], [new[1][r] for r in keep]], hidden=True)
    eng = models.engine(model)
    prefill(models, model, eng, hist)
    out = torch.full((M, sh.n_embd), float("nan"), dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    if pg:
        assert eng.stage_rows_pick(*new, x_out=out.data_ptr()) == []
    else:
        assert eng.stage_rows(*new, x_out=out.data_ptr()) is None
    models.note(model, new)
    got = out.cpu().numpy()[keep]
    what = f"{model[0]} {model[1]} hidden {layout} M={M}"
    if facts["walk"] == "kq_gemm":
        rows = [[new[0][r] for r in keep], [new[1][r] for r in keep]]
        deq = ref_rows(models, model, seqs, rows, hidden=True, dequantised=True)
        d = np.abs(got - deq) / W.bf16_tol_rows(deq)
        q8k = float((np.abs(got - ref) / W.bf16_tol_rows(ref)).max())
        print(f"{what}: worst |d| / bf16 bar {float(d.max()):.3f} against the dequantised bf16 oracle "
              f"({q8k:.3f} against the Q8_K oracle)")
        assert got.shape == deq.shape and np.isfinite(got).all()
        assert float(d.max()) <= 1.0, f"{what}: {float(d.max()):.3f} x the bf16 bar"
    else:
        check(models, model, got, ref, what, hidden=True)


PICK_CASES = [("one", M) for M in (1, 4, 5, 17, 32, 33, 64, 65)] + [("mixed", M) for M in (17, 24, 32, 33)] + \
             [("blocked", M) for M in (32, 64, 80, 272)]


@pytest.mark.parametrize("layout,M", PICK_CASES, ids=[f"{lay}-{M}" for lay, M in PICK_CASES])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_picks_of_a_rowmap_subset(models, model, layout, M):
    """stage_rows_pick with n_out < M: the head sees the rowmap rows only -- the last row of a one-sequence chunk,
    the last row of each slot / prompt otherwise.  At 17..32 rows of a quantised model the slabs of the last
    ffn_down are still pending when the walk ends and must be folded before the rowmap norm reads x.  Every pick
    is the oracle's argmax wherever the oracle's top-1/top-2 gap exceeds twice the tolerance.  At 1 row (every
    quantised format) and 4 rows (Q8_0 / Q4_0) the walks take their operands on load, but the head's rowmap operand
    falls back to a norm launch (operand(): ql && rmap).  bf16 takes the full-chain wide walk at every count <= 64 here (stage_rows_pick sets
    prefill_gemm), whose single slab of the last ffn_down is pending at the head too.  A K-quant chunk of 65 rows
    takes the dequantised-GEMM walk with the K-quant head: its picks are judged by the oracle of that arithmetic
    (walk_ref.oracle_kq_dequantised), as the hidden states are."""
    sh = models.shape(model)
    facts = W.walk_facts(model[0], sh, M, True)
    assert facts == expect(model[0], model[1], M, True)
    if M <= 4:  # on-load walks whose head operand is a rowmap: Q8_0 / Q4_0 at 1 and 4 rows, the K-quants at 1
        assert facts["on_load"] == (model[0] != "bf16" and (M == 1 or W.family(model[0]) == "q8"))
    if layout == "blocked":
        new, spans, prompts = W.blocked_case(sh, M, N_CTX)
        hist, seqs = ([], [], []), [(k, p, 0) for k, p in enumerate(prompts)]
        rowmap = [b - 1 for a, b in spans]
    else:
        hist, new, seqs = W.layout_rows(sh, layout, M)
        rowmap = [r for r in range(M) if r == M - 1 or new[0][r + 1] != new[0][r]]
    layout_facts(layout, new)
    assert 0 < len(rowmap) < M or M == 1  # one row: the rowmap still replaces the on-load head operand
    if 16 < M <= 32 or model[0] == "bf16" and M <= 64:  # slabs pending at the head with n_out != M
        assert facts["slabs"][2] > 0 or (W.family(model[0]) == "kq" and model[1] == "test-tiny")
    ref = ref_rows(models, model, seqs, [[new[0][r] for r in rowmap], [new[1][r] for r in rowmap]],
                   dequantised=facts["walk"] == "kq_gemm")
    eng = models.engine(model)
    prefill(models, model, eng, hist)
    toks = eng.stage_rows_pick(*new, rowmap=rowmap)
    models.note(model, new)
    assert len(toks) == len(rowmap)
    srt = np.sort(ref, axis=-1)
    gap = srt[:, -1] - srt[:, -2]
    tol = 2 * (1e-2 * np.abs(srt[:, -1]) + 2e-2 * np.abs(ref).max())  # conftest.assert_tokens_match's rule
    decided = gap > tol
    same = np.asarray(toks) == ref.argmax(-1)
    print(f"{model[0]} {model[1]} picks {layout} M={M}: {int(same.sum())}/{len(toks)} the oracle's argmax, "
          f"{int(decided.sum())} decided")
    assert not (decided & ~same).any(), f"picks differ at decided rowmap entries {np.nonzero(decided & ~same)[0].tolist()}"
    for t, row in zip(toks, ref):  # an undecided pick is still a near tie of its own row, not another row's token
        assert float(row.max() - row[int(t)]) <= 2 * (1e-2 * abs(float(row.max())) + 2e-2 * float(np.abs(ref).max()))


@pytest.mark.parametrize("M", (1, 4, 5, 17, 32, 33))
@pytest.mark.parametrize("handoff", ("f32", "bf16"))
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_hidden_state_in(models, model, handoff, M):
    """A stage engine holding layer 1 and the head, fed the oracle's layer-0 output (f32, or rounded to bf16 for the
    bf16 hand-off; the oracle continues from the same values): launch_f32_in / launch_bf16_to_f32 must leave the
    sum-of-squares partials that the on-load norms and on-load quantisation of <= 4 rows read."""
    import torch

    sh = models.shape(model)
    assert W.walk_facts(model[0], sh, M) == expect(model[0], model[1], M)
    bf = handoff == "bf16"
    hist, new, seqs = W.layout_rows(sh, "distinct", M)
    r = models.ref(model)
    dev = torch.device("cuda", 0)

    def hand(x):  # what the engine is fed, and the same values as f32 for the oracle
        t = torch.from_numpy(np.ascontiguousarray(x))
        t = t.to(torch.bfloat16) if bf else t
        return t.to(dev), t.to(torch.float32).numpy()

    x1 = [hand(r.layer0(s)) for _, s, _ in seqs]
    ref = np.stack([r.from_layer1(xo)[1][-1] for _, xo in x1])
    eng = models.engine(model, 1, bf)
    xh = torch.cat([xd[:-1] for xd, _ in x1]).contiguous()
    xn = torch.cat([xd[-1:] for xd, _ in x1]).contiguous()
    torch.cuda.synchronize()
    for c in range(0, len(hist[0]), 64):
        assert eng.stage_rows(hist[0][c:c + 64], hist[1][c:c + 64], None, x_in=xh[c:c + 64].data_ptr()) is None
    got = eng.stage_rows(new[0], new[1], None, x_in=xn.data_ptr(), want_logits=True)
    models.note(model, hist, 1, bf)
    models.note(model, new, 1, bf)
    check(models, model, got, ref, f"{model[0]} {model[1]} layer 1 + head from the {handoff} hand-off M={M}")


LOOP_ROWS = (1, 4, 5, 16, 17, 32, 33, 64)


@pytest.mark.parametrize("M", LOOP_ROWS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_device_greedy_loop(models, model, M):
    """Engine.batch, 6 steps: the argmax / pick tail of each walk, every row's chain teacher-forced through the
    oracle (conftest.check_chain_batched)."""
    sh = models.shape(model)
    assert W.walk_facts(model[0], sh, M) == expect(model[0], model[1], M)
    G = 6
    hist, new, seqs = W.layout_rows(sh, "distinct", M)
    eng = models.engine(model)
    prefill(models, model, eng, hist)
    b = eng.batch(slots=new[0], pos=new[1], ids=new[2], max_steps=G)
    for _ in range(G):
        b.step()
    toks = b.tokens()
    b.close()
    models.note(model, (new[0], [p + G - 1 for p in new[1]]))
    assert toks.shape == (M, G)
    om = models.ref(model).om
    exact = 0
    for i, (_, s, _) in enumerate(seqs):
        ctx = om.context(N_CTX)
        e, _ = check_chain_batched(ctx, s, toks[i].tolist(), f"{model[0]} {model[1]} loop M={M} row {i}")
        ctx.close()
        exact += e
    print(f"{model[0]} {model[1]} greedy loop M={M}: {exact}/{M * G} picks the oracle's argmax, the rest near ties")


@pytest.mark.parametrize("M", (5, 16, 17, 32, 33, 64))
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_same_bits_through_every_plumbing(models, model, M):
    """Row 0 of M distinct rows (slot 0 after a history of 69 tokens) and the last row of an M-row chunk of slot 0
    ending at the same position: the same history and token, FIN attention / one row per slot against
    launch_qkv_finish / rows attending to each other's new K/V.  Then the device greedy loop over the M distinct
    rows: a batch has no logits getter, so after its first step the residual stream x [M][n_embd] (slabs folded) and
    the normed rows xn that the head GEMV reads are dumped (Engine.debug_read) and compared with the same buffers
    after forward_rows of the same rows -- the head is the same launch on the same operand in both, so equal xn bits
    are equal logits bits -- and every step's token is the argmax of forward_rows at the same row count along the
    loop's own tokens.  bf16: the same bits and the same tokens; quantised formats (x only: their
    heads read Q8 rows, not xn): printed."""
    sh = models.shape(model)
    bf16 = model[0] == "bf16"
    long = W.tokens(sh, 70, 5000)
    hist, new, seqs = W.layout_rows(sh, "distinct", M)
    hist = ([0] * 69 + [s for s in hist[0] if s], list(range(69)) + [p for s, p in zip(hist[0], hist[1]) if s],
            long[:69] + [t for s, t in zip(hist[0], hist[2]) if s])
    new = (new[0], [69] + new[1][1:], [long[69]] + new[2][1:])
    eng = models.engine(model)
    prefill(models, model, eng, hist)
    a = eng.forward_rows(*new)
    models.note(model, new)
    h = sh.n_embd
    xa, xna = eng.debug_read("x", M * h * 4).view(np.uint32), eng.debug_read("xn", M * h * 2).view(np.uint16)
    assert xa.any() and (xna.any() or not bf16)
    one = eng.forward_rows([0] * M, list(range(70 - M, 70)), long[70 - M:])
    diff = int((a[0].view(np.uint32) != one[-1].view(np.uint32)).sum())
    print(f"{model[0]} {model[1]} M={M}: distinct row vs last row of a one-sequence chunk: {diff} logits differ in bits, "
          f"max |d| {float(np.abs(a[0] - one[-1]).max()):.3g}")
    if bf16:
        assert diff == 0
    G = 4
    b = eng.batch(slots=new[0], pos=new[1], ids=new[2], max_steps=G)
    for k in range(G):
        b.step()
        if k == 0:
            xb, xnb = eng.debug_read("x", M * h * 4).view(np.uint32), eng.debug_read("xn", M * h * 2).view(np.uint16)
    toks = b.tokens()
    b.close()
    dx, dxn = int((xa != xb).sum()), int((xna != xnb).sum())
    print(f"{model[0]} {model[1]} M={M}: first loop step vs forward_rows: {dx} values of x differ in bits" +
          (f", {dxn} of xn" if bf16 else ""))
    if bf16:
        assert dx == 0 and dxn == 0
    ids, same = list(new[2]), 0
    for k in range(G):
        lg = eng.forward_rows(new[0], [p + k for p in new[1]], ids)
        pick = lg.argmax(-1)
        same += int((pick == toks[:, k]).sum())
        if bf16:
            assert np.array_equal(pick, toks[:, k]), f"step {k}: loop and forward_rows pick differently at rows " \
                                                     f"{np.nonzero(pick != toks[:, k])[0].tolist()}"
        ids = [int(t) for t in toks[:, k]]
    models.note(model, (new[0], [p + G - 1 for p in new[1]]))
    print(f"{model[0]} {model[1]} M={M}: loop picks equal to forward_rows' argmax {same}/{M * G}")


def test_stage_rows_pick_cuts_unpadded_prompts_between_picks():
    """More than 64 unpadded prompts ending in one mx_stage_rows_pick call (bf16 test-tiny): the cut after the 64th
    pick must not skip a later prompt's last row.  70 prompts of 3 tokens (the 64th pick ends a 16-row block: the
    cut lands on it), and the same with a first prompt of 4 tokens: the cut's 16-row rounding would pass the
    65th prompt's last row, and the chunk ends there instead.  Every pick equals the pick of the same prompt alone."""
    from llama_p2p_amd import engine, synth

    engine.lib()
    sh = synth.SHAPES["test-tiny"]
    eng = Guarded(engine.Engine("synthetic:test-tiny:seed=0", n_ctx=32, n_seq_max=72, device=0), engine)
    try:
        for first in (3, 4):
            prompts = [W.tokens(sh, first if k == 0 else 3, 6000 + k) for k in range(70)]
            slots = [k for k, p in enumerate(prompts) for _ in p]
            pos = [i for p in prompts for i in range(len(p))]
            ids = [t for p in prompts for t in p]
            rowmap = list(np.cumsum([len(p) for p in prompts]) - 1)
            rounded = (rowmap[63] + 16) // 16 * 16
            assert (rounded > rowmap[64]) == (first == 4)  # the 4-token case is the one the clamp is for
            toks = eng.stage_rows_pick(slots, pos, ids, rowmap=rowmap)
            alone = [eng.stage_rows_pick([71] * len(p), list(range(len(p))), p, rowmap=[len(p) - 1])[0] for p in prompts]
            assert toks == alone, f"first prompt of {first}: picks differ at prompts " \
                                  f"{[k for k in range(70) if toks[k] != alone[k]]}"
            lg = eng.forward_rows([70] * 3, [0, 1, 2], prompts[69])  # the engine still serves a following call
            assert int(lg[-1].argmax()) == toks[69]
    finally:
        eng.close()


@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_nothing_written_past_the_used_positions(models, model):
    """After everything this module ran on the model's engine (and, run alone, after three calls of its own): the
    K / V of every position past a slot's used length, all layers, is still zero bits (the creation memset)."""
    sh = models.shape(model)
    eng = models.engine(model)
    for layout, M in (("distinct", 17), ("one", 33)):
        hist, new, _ = W.layout_rows(sh, layout, M)
        prefill(models, model, eng, hist)
        eng.forward_rows(*new)
        models.note(model, new)
    new, _, _ = W.blocked_case(sh, 80, N_CTX)
    eng.stage_rows_pick(*new)
    models.note(model, new)
    used = models.used[(model, 0, False)]
    NKV, D, S = sh.n_head_kv, sh.n_embd // sh.n_head, KL.ctx_stride(N_CTX)
    n = sh.n_layer * N_SLOTS * NKV * S * D
    for name, untile in (("kcache", KL.untile_k), ("vcache", KL.untile_v)):
        c = untile(eng.debug_read(name, n * 2).view(np.uint16).reshape(sh.n_layer, N_SLOTS, NKV, S * D), D)
        assert c.shape == (sh.n_layer, N_SLOTS, NKV, S, D)
        for s in range(N_SLOTS):
            tail = c[:, s, :, used.get(s, 0):]
            assert not tail.any(), (f"{name} of slot {s} holds non-zero bits at positions "
                                    f"{sorted(set((used.get(s, 0) + np.nonzero(tail.any(axis=(0, 1, 3)))[0]).tolist()))[:8]}"
                                    f" >= {used.get(s, 0)}")
            assert used.get(s, 0) == 0 or c[:, s, :, :used[s]].any()
