"""Shared pieces of the whole-model tests (no GPU needed to import): the scheduler's prefill row layout, the bound
of the quantised formats, the models of tests/test_layer_walk_gpu.py with their CPU oracles and cached oracle
results, the row layouts of that file, and the dispatch facts of a forward as the mx_*_plan functions give them.
"""
import numpy as np

FORMATS = ("bf16", "q8_0", "q4_0", "q4_k_m", "q5_k_m")
GGUF_Q4_0 = "q4_0_q6k"  # a Q4_0 file as llama-quantize writes it: Q4_0 matrices and token_embd, Q6_K output
EPI_F32, EPI_RESID, EPI_QKV, EPI_SWIGLU = 0, 1, 2, 3


# ---- the scheduler's prefill layout -------------------------------------------------------------------------------
def blocked_layout(prompts, slot0, n_ctx=512):
    """The scheduler's prefill layout (engine.cpp prefill_batch, pipeserve._prefill): each prompt from a
    16-row block boundary, padded to whole blocks; returns rows and each prompt's row range."""
    slots, pos, ids, spans = [], [], [], []
    for k, p in enumerate(prompts):
        n = len(p)
        r0 = len(slots)
        slots += [slot0 + k] * n
        pos += list(range(n))
        ids += p
        spans.append((r0, r0 + n))
        pad = (16 - n % 16) % 16
        slots += [slot0 + k] * pad
        pos += list(range(n, n + pad)) if n + pad <= n_ctx else [n - 1] * pad
        ids += [p[-1]] * pad
    return slots, pos, ids, spans


def is_blocked(slots, pos, ids):
    """engine.cpp blocked_rows: rows in blocks of 16 consecutive positions of one sequence (or copies of the row
    before them)."""
    for k in range(len(slots)):
        if k % 16 == 0:
            continue
        if slots[k] != slots[k - 1]:
            return False
        if pos[k] == pos[k - 1] + 1:
            continue
        if pos[k] != pos[k - 1] or ids[k] != ids[k - 1]:
            return False
    return True


def is_distinct(slots):
    return len(set(slots)) == len(slots)


# ---- the quantised formats' bound ---------------------------------------------------------------------------------
def jitter_bound(self_dev, ref):
    """Q8_0 / Q8_K activation rounding is discontinuous in its inputs, so an engine that does the oracle's arithmetic
    in another order is bounded by twice the oracle's own deviation under 1e-6 relative activation noise
    (oracle.q8_jitter), plus 1e-4 of the largest reference value (tests/test_q8_gpu.py)."""
    return 2 * self_dev + 1e-4 * np.abs(ref).max()


def bf16_tol_rows(ref):
    """The bf16 bar (conftest.logit_tol) row by row: 1e-2*|ref| + 2e-2*max|ref of that row|."""
    return 1e-2 * np.abs(ref) + 2e-2 * np.abs(ref).max(axis=-1, keepdims=True)


# ---- models -------------------------------------------------------------------------------------------------------
def family(fmt):
    return "bf16" if fmt == "bf16" else "kq" if fmt.endswith("_k_m") else "q8"


def model_path(fmt, shape_name, seed=0):
    return f"synthetic:{shape_name}:seed={seed}" + ("" if fmt == "bf16" else f":{fmt}")


def oracle_model(O, fmt, shape, seed=0):
    om = O.OracleModel(shape, seed=seed)
    if fmt == "q8_0":
        om.quantize_q8()
    elif fmt == "q4_0":
        om.quantize_q4_0()
    elif fmt != "bf16":
        om.kq_synthetic(fmt, seed)
    return om


def oracle_kq_dequantised(O, fmt, shape, seed=0):
    """The bf16 model a K-quant engine computes a prompt chunk of > 64 rows with (engine.cpp enqueue_forward_gemm:
    launch_dequant_kq, every weight d * q rounded to bf16, bf16 activations): the synthetic K-quant blocks of
    oracle_model(fmt), the layer matrices dequantised and rounded to bf16, under the synthetic norms.  The embedding
    stays K-quant (f32 rows of the dequantised blocks, as the engine looks them up): on these models one bf16 ulp of
    the embedding moves the last hidden state by up to 1.6 x the bf16 bar."""
    from llama_p2p_amd import synth

    om = O.OracleModel(shape, seed=seed)
    h, kv, ff, V = shape.n_embd, shape.n_embd_kv, shape.n_ff, shape.n_vocab
    mats = [(-1, 1, "token_embd", V * h, synth.TID_TOK_EMBD), (-1, 3, "output", V * h, synth.TID_OUTPUT)]
    for l in range(shape.n_layer):
        for kind, k, n in (("attn_q", synth.L_Q, h * h), ("attn_k", synth.L_K, kv * h), ("attn_v", synth.L_V, kv * h),
                           ("attn_output", synth.L_O, h * h), ("ffn_gate", synth.L_GATE, ff * h),
                           ("ffn_up", synth.L_UP, ff * h), ("ffn_down", synth.L_DOWN, h * ff)):
            mats.append((l, k, kind, n, synth.layer_tid(l, k)))
    for layer, k, kind, n, tid in mats:
        t = synth.kq_tensor_type(fmt, kind, layer, shape.n_layer)
        blocks = O.kq_synth_blocks(t, n // 256, seed, tid)
        if layer < 0:  # the embedding lookup and the head stay K-quant in that walk too
            om.set_tensor_kq(layer, k, t, blocks)
        else:
            om.set_tensor(layer, k, synth.f32_to_bf16_bits(O.kq_dequant(t, blocks, n)))
    return om


def oracle_from_q4_0_gguf(O, path, shape):
    """The oracle with the blocks of a Q4_0 GGUF written by gguf.write_synthetic_gguf(wtype="q4_0"): Q4_0 matrices,
    the dequantised token_embd as a bf16 table (what the engine keeps), the Q6_K output."""
    from llama_p2p_amd import gguf, synth

    r = gguf.GGUFReader(path)
    kinds = {"attn_q": 1, "attn_k": 2, "attn_v": 3, "attn_output": 4, "ffn_gate": 6, "ffn_up": 7, "ffn_down": 8}
    om = O.OracleModel(shape, seed=None)
    for name, info in r.tensors.items():
        raw = np.ascontiguousarray(r.tensor(name))
        if name == "token_embd.weight":
            emb = gguf.dequantize(info["type"], raw, (shape.n_vocab, shape.n_embd))
            om.set_tensor(-1, 1, synth.f32_to_bf16_bits(emb))
        elif name == "output_norm.weight":
            om.set_tensor(-1, 2, raw)
        elif name == "output.weight":
            assert info["type"] == gguf.GGML_Q6_K
            om.set_tensor_kq(-1, 3, gguf.GGML_Q6_K, raw)
        else:
            _, l, kind, _ = name.split(".")
            if kind in ("attn_norm", "ffn_norm"):
                om.set_tensor(int(l), {"attn_norm": 0, "ffn_norm": 5}[kind], raw)
            else:
                assert info["type"] == gguf.GGML_Q4_0
                om.set_tensor_q4_0(int(l), kinds[kind], raw)
    return om


# ---- dispatch facts (no GPU) --------------------------------------------------------------------------------------
def walk_facts(fmt, shape, M, prefill_gemm=False):
    """What a forward of M rows of this model dispatches on.  From the functions the engine itself asks
    (mx_matmul_plan, mx_q8_matmul_plan, mx_kq_matmul_plan): whether the GEMVs take their operand on load (RMS_NORM
    on load, bf16; quantise on load, quantised: the consumers of the residual stream's sums of squares), whether the
    GEMM takes every matrix, and the split-K slab counts of q|k|v, attn_output and ffn_down (0: written in place).
    The "walk" key restates enqueue_forward's own conditions on M, prefill_gemm (set by mx_stage_rows_pick) and
    gemm_shapes in Python (no plan function answers it): it names the branch, it is not independent evidence.
    prefill_gemm: a bf16 call of <= 64 rows takes the wide walk with full_chain at every row count (also <= 16): one K
    range per GEMV, which launch_mm_wide still leaves as ONE slab for q|k|v, attn_output and ffn_down."""
    from llama_p2p_amd import engine as E
    from llama_p2p_amd import synth

    h, kv, ff = shape.n_embd, shape.n_embd_kv, shape.n_ff
    mats = ((EPI_QKV, h + 2 * kv, h), (EPI_RESID, h, h), (EPI_RESID, h, ff))
    fmt = "q4_0" if fmt == GGUF_Q4_0 else fmt
    fam = family(fmt)
    if fam == "bf16":
        wide = M > 16
        gemm = all(E.matmul_plan(e, M, n, k)["gemm_ok"] for e, n, k in mats + ((EPI_SWIGLU, 2 * ff, h),))
        if prefill_gemm and gemm and M <= 64:
            return {"walk": "wide_full_chain", "gemm_shapes": gemm, "on_load": False, "slabs": (1, 1, 1)}
        return {"walk": "gemm" if M > 64 else "wide" if wide else "rows16", "gemm_shapes": gemm,
                "on_load": (not wide) and E.matmul_plan(EPI_QKV, M, h + 2 * kv, h)["norm_on_load_ok"],
                "slabs": tuple(E.matmul_plan(e, M, n, k)["kgroups"] for e, n, k in mats) if 16 < M <= 64 else (0, 0, 0)}
    slab_rows = 16 < M <= 32
    if fam == "q8":
        q4 = fmt != "q8_0"
        ql = (E.q8_matmul_plan(EPI_QKV, M, h + 2 * kv, h, wq4=q4, norm=True)["can_on_load"] and
              E.q8_matmul_plan(EPI_RESID, M, h, ff, wq4=q4)["can_on_load"])
        ks = tuple(max(E.q8_matmul_plan(e, M, n, k, wq4=q4)["slab_ks"], 0) for e, n, k in mats)
        return {"walk": "q8", "on_load": ql, "slabs": ks if slab_rows and not ql else (0, 0, 0)}
    worst = [0, 0, 0]
    ql = True
    for l in range(shape.n_layer):
        def t(kind):
            return synth.kq_tensor_type(fmt, kind, l, shape.n_layer)

        segs, end = [], 0
        for kind, n in (("attn_q", h), ("attn_k", kv), ("attn_v", kv)):
            end += n // 16
            if segs and segs[-1][0] == t(kind):
                segs[-1] = (t(kind), end)
            else:
                segs.append((t(kind), end))
        ks = (E.kq_matmul_plan(EPI_QKV, M, h + 2 * kv, h, segs)["qkv_slab_ks"],
              E.kq_matmul_plan(EPI_RESID, M, h, h, t("attn_output"))["slab_ks"],
              E.kq_matmul_plan(EPI_RESID, M, h, ff, t("ffn_down"))["slab_ks"])
        worst = [max(a, b, 0) for a, b in zip(worst, ks)]
        ql = ql and E.kq_matmul_plan(EPI_QKV, M, h + 2 * kv, h, segs, norm=True)["can_on_load"] and \
            E.kq_matmul_plan(EPI_RESID, M, h, ff, t("ffn_down"))["can_on_load"]
    # > 64 rows (never with logits of more than 64 rows or in the device loop): dequantised bf16 GEMMs
    return {"walk": "kq_gemm" if M > 64 else "kq", "on_load": ql,
            "slabs": tuple(worst) if slab_rows and not ql else (0, 0, 0)}


# ---- token sequences and row layouts --------------------------------------------------------------------------------
def tokens(shape, n, seed):
    rng = np.random.default_rng(seed)
    return [1] + [int(t) for t in rng.integers(3, shape.n_vocab, n - 1)]


def distinct_history(i):
    return 3 + (5 * i) % 40


def distinct_seq(shape, i, extra=1):
    """Sequence i of the distinct layout: its history of 3 + (5 i mod 40) tokens and `extra` more."""
    return tokens(shape, distinct_history(i) + 8, 1000 + i)[:distinct_history(i) + extra]


ONE_SEQ_SEED, ONE_SEQ_HISTORY = 2000, 3


def layout_rows(shape, layout, M):
    """(history rows, new rows, sequences): rows are (slots, pos, ids) lists; sequences [(slot, token list, first new
    position)] name what each slot holds once the new rows ran, the oracle's input.
    distinct: M slots, one row each after its own history.  one: M consecutive positions of slot 0 after 3 tokens.
    mixed: three slots with M//3 (+ remainder) consecutive rows each, after histories of 3, 8 and 13 tokens: neither
    distinct nor 16-blocked."""
    hist, new, seqs = ([], [], []), ([], [], []), []

    def add(rows, slot, p0, toks):
        rows[0].extend([slot] * len(toks))
        rows[1].extend(range(p0, p0 + len(toks)))
        rows[2].extend(toks)

    if layout == "distinct":
        for i in range(M):
            s = distinct_seq(shape, i)
            add(hist, i, 0, s[:-1])
            add(new, i, len(s) - 1, s[-1:])
            seqs.append((i, s, len(s) - 1))
    elif layout == "one":
        s = tokens(shape, 96, ONE_SEQ_SEED)[:ONE_SEQ_HISTORY + M]
        add(hist, 0, 0, s[:ONE_SEQ_HISTORY])
        add(new, 0, ONE_SEQ_HISTORY, s[ONE_SEQ_HISTORY:])
        seqs.append((0, s, ONE_SEQ_HISTORY))
    elif layout == "mixed":
        assert M >= 6
        counts = [M // 3 + (1 if j < M % 3 else 0) for j in range(3)]
        for j, c in enumerate(counts):
            hl = distinct_history(j)
            s = tokens(shape, 96, 3000 + j)[:hl + c]
            add(hist, j, 0, s[:hl])
            add(new, j, hl, s[hl:])
            seqs.append((j, s, hl))
    else:
        raise ValueError(layout)
    return hist, new, seqs


BLOCKED_PROMPTS = {32: (9, 16), 64: (7, 16, 20), 80: (7, 16, 20, 5), 272: (100, 33, 64, 40)}


def blocked_case(shape, M, n_ctx):
    """Prompts of BLOCKED_PROMPTS[M] tokens in the scheduler's layout: exactly M rows.  Returns (rows, spans, prompts)."""
    prompts = [tokens(shape, n, 4000 + 10 * M + k) for k, n in enumerate(BLOCKED_PROMPTS[M])]
    slots, pos, ids, spans = blocked_layout(prompts, 0, n_ctx)
    assert len(slots) == M
    return (slots, pos, ids), spans, prompts


class Reference:
    """The oracle of one model with its results cached per token sequence: a sequence that is a prefix of an
    evaluated one reuses its rows (the model is causal).  hidden / logits: after the last layer, every position;
    with jitter=True under oracle.q8_jitter(1e-6), for the quantised formats' bound."""

    def __init__(self, O, make, shape, n_ctx):
        self.O, self.make, self.shape, self.n_ctx = O, make, shape, n_ctx
        self.om = make()
        O.q8_jitter(1e-6)
        try:
            self.om_jit = make()
        finally:
            O.q8_jitter(0.0)
        self._cache = {False: [], True: []}
        self._layer0 = {}
        self._dev = None

    def _eval(self, seq, jitter):
        seq = tuple(int(t) for t in seq)
        for s, res in self._cache[jitter]:
            if s[:len(seq)] == seq:
                return res[0][:len(seq)], res[1][:len(seq)]
        if jitter:
            self.O.q8_jitter(1e-6)
        try:
            ctx = (self.om_jit if jitter else self.om).context(self.n_ctx)
            res = ctx.layers(None, 0, 0, self.shape.n_layer, ids=list(seq), logits=True)
            ctx.close()
        finally:
            self.O.q8_jitter(0.0)
        self._cache[jitter].append((seq, res))
        return res

    def hidden(self, seq, jitter=False):
        return self._eval(seq, jitter)[0]

    def logits(self, seq, jitter=False):
        return self._eval(seq, jitter)[1]

    def layer0(self, seq):
        """The residual stream after layer 0, every position: what a stage engine with layer_begin = 1 is fed."""
        key = tuple(int(t) for t in seq)
        if key not in self._layer0:
            ctx = self.om.context(self.n_ctx)
            self._layer0[key] = ctx.layers(None, 0, 0, 1, ids=list(key))
            ctx.close()
        return self._layer0[key]

    def from_layer1(self, x1, jitter=False):
        """(hidden, logits) of layers 1.. on the given layer-0 output, every position."""
        if jitter:
            self.O.q8_jitter(1e-6)
        try:
            ctx = (self.om_jit if jitter else self.om).context(self.n_ctx)
            res = ctx.layers(x1, 0, 1, self.shape.n_layer, logits=True)
            ctx.close()
        finally:
            self.O.q8_jitter(0.0)
        return res

    def self_deviation(self):
        """The oracle's own deviation under 1e-6 relative activation noise over this file's sequence pool (the 64
        sequences of the distinct layout and the one-sequence chunk, every position): (logits, hidden)."""
        if self._dev is None:
            pool = [distinct_seq(self.shape, i) for i in range(64)] + [tokens(self.shape, 96, ONE_SEQ_SEED)[:83]]
            dl = dh = 0.0
            for s in pool:
                dl = max(dl, float(np.abs(self.logits(s, True) - self.logits(s)).max()))
                dh = max(dh, float(np.abs(self.hidden(s, True) - self.hidden(s)).max()))
            self._dev = (dl, dh)
        return self._dev

    def close(self):
        self.om.close()
        self.om_jit.close()
