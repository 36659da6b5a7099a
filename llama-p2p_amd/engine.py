"""ctypes binding of the engine's C ABI (include/mx_engine.h).

The shared library is built in-tree (``llama-p2p_amd/libmxllama.so``, see
build.py).  There is deliberately no fallback: if the library is missing or no
GPU is visible, every entry point raises -- the product never computes on the
CPU.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MX_LIB") or os.path.join(HERE, "libmxllama.so")  # MX_LIB: A/B builds only

MX_OK = 0
MX_ERR_ARG, MX_ERR_HIP, MX_ERR_MODEL, MX_ERR_CTX, MX_ERR_NOTFOUND, MX_ERR_STATE = -1, -2, -3, -4, -5, -6
MX_DEBUG_STOPPED = 1  # a forward cut short by debug_stop (include/mx_engine.h): raised, never silent
FINISH_LENGTH, FINISH_STOP, FINISH_ERROR = 0, 1, 2

# the K-quant kernel probes, named in a list of their own (tests/test_kq_kernel_gpu.py) and part of EXPORTS
EXPORTS_KQ = ["mx_kq_matmul_probe", "mx_kq_matmul_plan", "mx_kq_side_probe"]
# every symbol include/mx_engine.h declares (checked by tests/test_abi.py)
EXPORTS = EXPORTS_KQ + [
    "mx_opts_default", "mx_sampling_default", "mx_last_error", "mx_engine_create", "mx_engine_destroy", "mx_gguf_check",
    "mx_engine_info", "mx_forward_logits", "mx_forward_rows", "mx_forward_topk", "mx_submit", "mx_wait", "mx_submit_batch", "mx_poll", "mx_cancel", "mx_batch_create",
    "mx_batch_step", "mx_batch_ids_device", "mx_batch_bind_ids", "mx_batch_tokens", "mx_batch_destroy", "mx_stage_rows",
    "mx_profile_kernel", "mx_sync", "mx_device_count", "mx_engine_stats", "mx_batch_reset", "mx_stage_rows_pick",
    "mx_probe_copy", "mx_probe_read", "mx_debug",
    "mx_submit_lp", "mx_request_logprobs", "mx_forward_logprobs", "mx_logprob_probe",
    "mx_attention_probe", "mx_matmul_probe", "mx_matmul_plan", "mx_norm_probe",
    "mx_submit_spec", "mx_spec_stats", "mx_draft_probe", "mx_accept_probe",
    "mx_submit_embed", "mx_wait_embed", "mx_pool_probe",
    "mx_engine_set_prefix_sharing", "mx_prefix_sharing_stats", "mx_kv_copy_probe",
    "mx_engine_set_host_cache", "mx_host_cache_stats", "mx_kv_pack_probe",
    "mx_sampling_ext_default", "mx_submit_ext", "mx_submit_ext_batch", "mx_sample_probe",
    "mx_sample_plan", "mx_sampler_stats",
    "mx_glue_probe",
    "mx_engine_create_lora", "mx_lora_check", "mx_engine_lora_info", "mx_lora_merge_probe",
    "mx_vocab_create", "mx_vocab_destroy", "mx_grammar_create", "mx_grammar_destroy", "mx_grammar_state_create",
    "mx_grammar_state_mask", "mx_grammar_state_accept", "mx_grammar_state_may_end", "mx_grammar_state_destroy",
    "mx_grammar_cache_stats", "mx_submit_grammar", "mx_grammar_mask_probe",
    "mx_grammar_mask_time",
]
# the Q8_0 / Q4_0 kernel probes: names with a digit, listed apart (tests/test_gguf_abi.py checks both lists)
EXPORTS_Q8 = ["mx_q8_matmul_probe", "mx_q8_matmul_plan", "mx_q8_side_probe"]
LOGIT_BIAS_MAX = 256  # kernels.h SAMP_BIAS_MAX: most logit_bias entries per request
POOL_NONE, POOL_MEAN, POOL_CLS, POOL_LAST = 0, 1, 2, 3  # mx_engine.h MX_POOL_*: how embed() pools a sequence's rows
TOPK_MAX = 64  # kernels.h: most top entries per token (logprobs=, device top_k)
# mx_engine.h MX_PICK_*: which sampler picks a row (sample_plan())
MX_PICK_ARGMAX, MX_PICK_CHAIN, MX_PICK_MIROSTAT, MX_PICK_WIDE, MX_PICK_HOST = 0, 1, 2, 3, 4
SPEC_MAX_DRAFT = 15  # kernels.h: most draft tokens per speculating step (1 + 15 rows of the <= 16-row path)


class MxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mx error {code}: {msg}")
        self.code = code


class MxOpts(ctypes.Structure):
    _fields_ = [("n_ctx", ctypes.c_int32), ("n_seq_max", ctypes.c_int32), ("layer_begin", ctypes.c_int32),
                ("layer_end", ctypes.c_int32), ("device", ctypes.c_int32), ("use_graphs", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("handoff_bf16", ctypes.c_int32)]


class MxModelInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_embd", "n_layer", "n_head", "n_head_kv", "head_dim", "n_ff",
                                              "n_vocab", "n_ctx_train")] + \
               [("eps", ctypes.c_float), ("rope_base", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("bos_id", "eos_id", "n_ctx", "n_seq_max", "layer_begin",
                                              "layer_end", "has_embed", "has_head")] + \
               [("weight_bytes", ctypes.c_uint64), ("weight_type", ctypes.c_int32), ("eot_id", ctypes.c_int32)]


class MxSampling(ctypes.Structure):
    _fields_ = [("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float),
                ("min_p", ctypes.c_float), ("repeat_penalty", ctypes.c_float), ("repeat_last_n", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("ignore_eos", ctypes.c_int32),
                ("frequency_penalty", ctypes.c_float), ("presence_penalty", ctypes.c_float)]


class MxSamplingExt(ctypes.Structure):
    _fields_ = [("base", MxSampling), ("typical_p", ctypes.c_float), ("tfs_z", ctypes.c_float),
                ("mirostat_mode", ctypes.c_int32), ("mirostat_tau", ctypes.c_float), ("mirostat_eta", ctypes.c_float),
                ("n_logit_bias", ctypes.c_int32), ("bias_tok", ctypes.POINTER(ctypes.c_int32)),
                ("bias_val", ctypes.POINTER(ctypes.c_float))]


_EXT_KEYS = ("typical_p", "tfs_z", "mirostat_mode", "mirostat_tau", "mirostat_eta", "logit_bias")


def sampling_ext(base: "MxSampling", typical_p: float = 1.0, tfs_z: float = 1.0, mirostat_mode: int = 0,
                 mirostat_tau: float = 5.0, mirostat_eta: float = 0.1, logit_bias=None, into=None):
    """An mx_sampling_ext over `base`; logit_bias: {token id: bias} or (ids, values).  Returns (struct, keepalive):
    the struct points into the keepalive arrays, which must outlive the call that reads it."""
    s = into if into is not None else MxSamplingExt()
    lib().mx_sampling_ext_default(ctypes.byref(s))
    s.base = base
    s.typical_p, s.tfs_z, s.mirostat_mode = typical_p, tfs_z, int(mirostat_mode)
    s.mirostat_tau, s.mirostat_eta = mirostat_tau, mirostat_eta
    keep = None
    if logit_bias is not None and len(logit_bias):
        if isinstance(logit_bias, dict):
            toks, vals = list(logit_bias.keys()), list(logit_bias.values())
        else:
            toks, vals = logit_bias
        bt = np.ascontiguousarray(toks, dtype=np.int32)
        bv = np.ascontiguousarray(vals, dtype=np.float32)
        s.n_logit_bias = len(bt)
        s.bias_tok = bt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        s.bias_val = bv.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        keep = (bt, bv)
    return s, keep


class MxRowSampler(ctypes.Structure):
    _fields_ = [("s", MxSampling), ("seed", ctypes.c_uint64), ("n_drawn", ctypes.c_int32), ("n_win", ctypes.c_int32),
                ("win", ctypes.c_int32 * 64)]


class MxSpecCounts(ctypes.Structure):
    _fields_ = [("steps", ctypes.c_uint64), ("drafted", ctypes.c_uint64), ("accepted", ctypes.c_uint64)]


class MxSamplerCounts(ctypes.Structure):
    _fields_ = [("device_steps", ctypes.c_uint64), ("host_steps", ctypes.c_uint64), ("wide_rows", ctypes.c_uint64),
                ("rounds", ctypes.c_uint64)]


class MxSharingStats(ctypes.Structure):
    _fields_ = [("shared_prompt_tokens", ctypes.c_uint64), ("copies", ctypes.c_uint64),
                ("copied_bytes", ctypes.c_uint64), ("follower_requests", ctypes.c_uint64)]


class MxLoraInfo(ctypes.Structure):
    _fields_ = [("n_tensors", ctypes.c_int32), ("rank_max", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("lora_scale", ctypes.c_float)]


class MxKvCopy(ctypes.Structure):
    _fields_ = [("src_slot", ctypes.c_int32), ("dst_slot", ctypes.c_int32), ("n_pos", ctypes.c_int32)]


class MxHostCacheCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "entries", "bytes", "capacity_bytes", "spills", "spilled_bytes", "restores", "restored_prompt_tokens",
        "restored_bytes", "evictions", "skipped")]


class MxKvPack(ctypes.Structure):
    _fields_ = [("slot", ctypes.c_int32), ("n_pos", ctypes.c_int32), ("offset16", ctypes.c_uint64)]


class MxMatmulArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "epi", "M", "N", "K")] + \
               [(n, ctypes.c_void_p) for n in ("w", "x", "xf", "norm_w")] + \
               [("eps", ctypes.c_float), ("target", ctypes.c_int32), ("slab_floats", ctypes.c_uint64),
                ("want_ssq", ctypes.c_int32), ("act_f32", ctypes.c_int32)] + \
               [(n, ctypes.c_int32) for n in ("n_head", "n_head_kv", "head_dim", "n_ctx", "n_slots")] + \
               [(n, ctypes.c_void_p) for n in ("pos", "slot", "rope_cs", "kcache", "vcache", "resid", "out", "ssq_out",
                                               "slabs_out")] + \
               [("slabs_cap", ctypes.c_uint64), ("split_out", ctypes.c_void_p), ("packed_out", ctypes.c_void_p),
                ("bias", ctypes.c_void_p)]


class MxQ8MatmulArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "epi", "M", "N", "K", "wq4", "act")] + \
               [("w", ctypes.c_void_p), ("xf", ctypes.c_void_p), ("xrows", ctypes.c_int32), ("ldx", ctypes.c_int32),
                ("norm_w", ctypes.c_void_p), ("eps", ctypes.c_float), ("row_map", ctypes.c_void_p),
                ("fold_slabs", ctypes.c_void_p), ("nslab", ctypes.c_int32), ("want_ssq", ctypes.c_int32),
                ("act_f32", ctypes.c_int32)] + \
               [(n, ctypes.c_int32) for n in ("n_head", "n_head_kv", "head_dim", "n_ctx", "n_slots")] + \
               [(n, ctypes.c_void_p) for n in ("pos", "slot", "rope_cs", "kcache", "vcache", "resid", "fold_w", "out",
                                               "ssq_out", "slabs_out")] + \
               [("slabs_cap", ctypes.c_uint64)] + \
               [(n, ctypes.c_void_p) for n in ("split_out", "packed_out", "xq_out", "xd_out", "x_out", "nxq_out",
                                               "nxd_out")] + [("np", ctypes.c_int32), ("bias", ctypes.c_void_p)]


class MxQ8Plan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "qp", "qm", "tpw", "ks", "rt", "nb", "bd", "grid_y", "w", "grid",
                                              "slab_ks", "can_on_load")]


class MxKqMatmulArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "epi", "M", "N", "K", "act", "kq_n")] + \
               [("kq_type", ctypes.c_int32 * 3), ("kq_tile_end", ctypes.c_int32 * 3),
                ("w", ctypes.c_void_p), ("xf", ctypes.c_void_p), ("xrows", ctypes.c_int32), ("ldx", ctypes.c_int32),
                ("norm_w", ctypes.c_void_p), ("eps", ctypes.c_float), ("row_map", ctypes.c_void_p),
                ("ssq_in", ctypes.c_void_p), ("want_ssq", ctypes.c_int32)] + \
               [(n, ctypes.c_int32) for n in ("n_head", "n_head_kv", "head_dim", "n_ctx", "n_slots")] + \
               [(n, ctypes.c_void_p) for n in ("pos", "slot", "rope_cs", "kcache", "vcache", "resid", "fold_w", "out",
                                               "ssq_out", "slabs_out")] + \
               [("slabs_cap", ctypes.c_uint64)] + \
               [(n, ctypes.c_void_p) for n in ("split_out", "packed_out", "xq_out", "xd_out", "xb_out", "nxq_out",
                                               "nxd_out", "nxb_out", "bias")]


class MxKqPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "t", "ks", "nkw", "tpw", "nb", "u", "bd", "ql", "w", "grid_x",
                                              "grid_y", "slab_ks", "qkv_slab_ks", "can_on_load")]


class MxKqSideArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "type", "N", "K")] + \
               [("blocks", ctypes.c_void_p), ("pack", ctypes.c_int32), ("offset", ctypes.c_int32),
                ("kq_n", ctypes.c_int32), ("kq_type", ctypes.c_int32 * 3), ("kq_tile_end", ctypes.c_int32 * 3),
                ("ids", ctypes.c_void_p), ("M", ctypes.c_int32), ("rows", ctypes.c_int32), ("ld", ctypes.c_int32),
                ("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("row_map", ctypes.c_void_p), ("eps", ctypes.c_float),
                ("slabs", ctypes.c_void_p), ("nslab", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("out", "ssq_out", "xq_out", "xd_out", "xb_out", "x_out")]


class MxGlueArgs(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("type", ctypes.c_int32), ("count", ctypes.c_uint64),
                ("src_bytes", ctypes.c_uint64)] + \
               [(n, ctypes.c_int32) for n in ("M", "N", "n", "want_ssq")] + \
               [(n, ctypes.c_void_p) for n in ("src", "ids", "out", "ssq_out")] + \
               [(n, ctypes.c_int32) for n in ("V", "ldl", "hist_stride", "max_hist", "null_mask")] + \
               [(n, ctypes.c_void_p) for n in ("pos", "hist_count", "tok_out", "ids_next_out", "pos_next_out",
                                               "hist_out", "hist_count_out")]


def sampling(temperature: float = 0.0, top_k: int = 40, top_p: float = 0.95, min_p: float = 0.05,
             repeat_penalty: float = 1.0, repeat_last_n: int = 64, seed: Optional[int] = None,
             ignore_eos: bool = False, frequency_penalty: float = 0.0, presence_penalty: float = 0.0) -> MxSampling:
    """An mx_sampling with llama-cpp-python's defaults for the unspecified fields."""
    s = MxSampling()
    lib().mx_sampling_default(ctypes.byref(s))
    s.temperature, s.top_k, s.top_p, s.min_p = temperature, top_k, top_p, min_p
    s.repeat_penalty, s.repeat_last_n, s.ignore_eos = repeat_penalty, repeat_last_n, int(ignore_eos)
    s.frequency_penalty, s.presence_penalty = frequency_penalty, presence_penalty
    if seed is not None and seed >= 0:
        s.seed = seed
    return s


def row_samplers(rows) -> "ctypes.Array":
    """rows: [(MxSampling, seed, n_drawn, window tokens)] -> mx_row_sampler[len(rows)]."""
    arr = (MxRowSampler * len(rows))()
    for i, (smp, seed, n_drawn, win) in enumerate(rows):
        win = list(win)[-64:]
        arr[i].s = smp
        arr[i].seed = seed
        arr[i].n_drawn = n_drawn
        arr[i].n_win = len(win)
        for j, t in enumerate(win):
            arr[i].win[j] = int(t)
    return arr


_lib = None
_lib_lock = threading.Lock()


def _torch_hip_first():
    """Initialise PyTorch's HIP runtime before loading the engine, so the process has ONE runtime.
    libmxllama.so NEEDs libamdhip64.so.7; PyTorch's libc10_hip.so NEEDs libamdhip64.so and loads its
    bundled copy, whose SONAME is also libamdhip64.so.7 -- loaded after PyTorch, the engine binds to that
    copy (and PyTorch stream handles passed to mx_batch_step are objects of the same runtime).  Loaded
    first, the engine pulled in /opt/rocm's copy and PyTorch's second copy then saw no GPU ("No HIP GPUs
    are available"; tools/hip_runtime_order_probe.py).  Nothing to do without a GPU."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def lib() -> ctypes.CDLL:
    """Load libmxllama.so (raises if it was not built)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `python llama-p2p_amd/build.py` "
                              "(the engine has no CPU fallback)")
        _torch_hip_first()
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
        P = ctypes.POINTER
        L.mx_opts_default.argtypes = [P(MxOpts)]
        L.mx_sampling_default.argtypes = [P(MxSampling)]
        L.mx_last_error.restype = ctypes.c_char_p
        L.mx_engine_create.argtypes = [ctypes.c_char_p, P(MxOpts), P(vp)]
        L.mx_engine_destroy.argtypes = [vp]
        L.mx_gguf_check.argtypes = [ctypes.c_char_p]
        L.mx_engine_info.argtypes = [vp, P(MxModelInfo)]
        L.mx_forward_logits.argtypes = [vp, i32, vp, i32, i32, vp]
        L.mx_forward_rows.argtypes = [vp, i32, vp, vp, vp, vp]
        L.mx_forward_topk.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp]
        L.mx_submit.argtypes = [vp, vp, i32, P(MxSampling), i32, P(u64)]
        L.mx_wait.argtypes = [vp, u64, vp, i32, P(i32), P(i32)]
        L.mx_submit_batch.argtypes = [vp, i32, vp, vp, vp, vp, P(u64)]
        L.mx_poll.argtypes = [vp, u64, i32, vp, i32, P(i32), P(i32)]
        L.mx_cancel.argtypes = [vp, u64]
        L.mx_batch_create.argtypes = [vp, i32, vp, vp, vp, i32, P(vp)]
        L.mx_batch_step.argtypes = [vp, vp, vp, vp, vp]
        L.mx_batch_ids_device.argtypes = [vp]
        L.mx_batch_ids_device.restype = vp
        L.mx_batch_tokens.argtypes = [vp, vp, vp, i32, P(i32)]
        L.mx_batch_bind_ids.argtypes = [vp, vp, vp]
        L.mx_batch_destroy.argtypes = [vp, vp]
        L.mx_stage_rows.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.mx_profile_kernel.argtypes = [vp, i32, i32, i32, P(ctypes.c_double), P(ctypes.c_double)]
        L.mx_sync.argtypes = [vp]
        L.mx_probe_copy.argtypes = [i32, ctypes.c_size_t, i32, P(ctypes.c_double), ctypes.c_char_p, i32]
        L.mx_probe_read.argtypes = [i32, ctypes.c_size_t, i32, P(ctypes.c_double), ctypes.c_char_p, i32]
        L.mx_device_count.argtypes = [P(i32)]
        L.mx_engine_stats.argtypes = [vp, P(MxStats)]
        L.mx_batch_reset.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mx_stage_rows_pick.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.mx_debug.argtypes = [vp, i32, ctypes.c_longlong, vp, ctypes.c_size_t]
        L.mx_submit_lp.argtypes = [vp, vp, i32, P(MxSampling), i32, i32, i32, P(u64)]
        L.mx_request_logprobs.argtypes = [vp, u64, vp, vp, vp, i32, P(i32), P(i32)]
        L.mx_forward_logprobs.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.mx_logprob_probe.argtypes = [i32, vp, i32, i32, i32, vp, i32, vp, vp, vp]
        L.mx_attention_probe.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp,
                                         vp, vp]
        L.mx_matmul_probe.argtypes = [i32, P(MxMatmulArgs)]
        L.mx_matmul_plan.argtypes = [i32, i32, i32, i32, P(i32), P(i32), P(i32), P(i32)]
        L.mx_norm_probe.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, vp, ctypes.c_float, vp, vp]
        L.mx_q8_matmul_probe.argtypes = [i32, P(MxQ8MatmulArgs)]
        L.mx_q8_matmul_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, P(MxQ8Plan)]
        L.mx_q8_side_probe.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, vp]
        L.mx_kq_matmul_probe.argtypes = [i32, P(MxKqMatmulArgs)]
        L.mx_kq_matmul_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, P(MxKqPlan)]
        L.mx_kq_side_probe.argtypes = [i32, P(MxKqSideArgs)]
        L.mx_glue_probe.argtypes = [i32, P(MxGlueArgs)]
        L.mx_submit_spec.argtypes = [vp, vp, i32, P(MxSampling), i32, i32, i32, P(u64)]
        L.mx_spec_stats.argtypes = [vp, u64, P(MxSpecCounts)]
        L.mx_draft_probe.argtypes = [i32, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        L.mx_accept_probe.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mx_submit_embed.argtypes = [vp, i32, vp, vp, i32, i32, P(u64)]
        L.mx_wait_embed.argtypes = [vp, u64, vp, ctypes.c_size_t, P(i32)]
        L.mx_pool_probe.argtypes = [i32, i32, i32, vp, vp, ctypes.c_float, i32, vp, i32, i32, i32, vp]
        L.mx_engine_set_prefix_sharing.argtypes = [vp, i32]
        L.mx_prefix_sharing_stats.argtypes = [vp, P(MxSharingStats)]
        L.mx_kv_copy_probe.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
        L.mx_engine_set_host_cache.argtypes = [vp, ctypes.c_uint64]
        L.mx_host_cache_stats.argtypes = [vp, P(MxHostCacheCounts)]
        L.mx_kv_pack_probe.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, ctypes.c_uint64]
        L.mx_sampling_ext_default.argtypes = [P(MxSamplingExt)]
        L.mx_submit_ext.argtypes = [vp, vp, i32, P(MxSamplingExt), i32, i32, i32, P(u64)]
        L.mx_submit_ext_batch.argtypes = [vp, i32, vp, vp, vp, vp, P(u64)]
        L.mx_sample_plan.argtypes = [P(MxSamplingExt), i32, P(i32)]
        L.mx_sampler_stats.argtypes = [vp, P(MxSamplerCounts)]
        L.mx_sample_probe.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mx_engine_create_lora.argtypes = [ctypes.c_char_p, P(MxOpts), ctypes.c_char_p, ctypes.c_float, P(vp)]
        L.mx_lora_check.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        L.mx_engine_lora_info.argtypes = [vp, P(MxLoraInfo)]
        L.mx_lora_merge_probe.argtypes = [i32, i32, i32, i32, vp, vp, vp, ctypes.c_float, vp, i32, P(ctypes.c_double)]
        L.mx_vocab_create.argtypes = [i32, vp, vp, vp, i32, P(vp)]
        L.mx_vocab_destroy.argtypes = [vp]
        L.mx_grammar_create.argtypes = [vp, ctypes.c_char_p, i32, P(vp)]
        L.mx_grammar_destroy.argtypes = [vp]
        L.mx_grammar_state_create.argtypes = [vp, P(vp)]
        L.mx_grammar_state_mask.argtypes = [vp, vp, i32, P(i32)]
        L.mx_grammar_state_accept.argtypes = [vp, i32]
        L.mx_grammar_state_may_end.argtypes = [vp, P(i32)]
        L.mx_grammar_state_destroy.argtypes = [vp]
        L.mx_grammar_cache_stats.argtypes = [vp, P(u64), P(u64), P(u64)]
        L.mx_submit_grammar.argtypes = [vp, vp, i32, P(MxSamplingExt), i32, i32, i32, vp, P(u64)]
        L.mx_grammar_mask_probe.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp]
        L.mx_grammar_mask_time.argtypes = [i32, i32, i32, i32, vp, i32, P(ctypes.c_double)]
        for name in EXPORTS + EXPORTS_Q8:
            if name not in ("mx_opts_default", "mx_sampling_default", "mx_sampling_ext_default", "mx_last_error",
                            "mx_engine_destroy", "mx_vocab_destroy", "mx_grammar_destroy", "mx_grammar_state_destroy",
                            "mx_batch_destroy", "mx_batch_ids_device"):
                getattr(L, name).restype = i32
        _lib = L
        return L


class MxStats(ctypes.Structure):
    _fields_ = [("prompt_tokens", ctypes.c_uint64), ("reused_prompt_tokens", ctypes.c_uint64),
                ("generated_tokens", ctypes.c_uint64)]


def device_count() -> int:
    n = ctypes.c_int32()
    _check(lib().mx_device_count(ctypes.byref(n)))
    return n.value


def gguf_check(path: str):
    """Validate a GGUF container (no GPU needed); raises MxError(MX_ERR_MODEL) with the reason."""
    _check(lib().mx_gguf_check(path.encode()))


def lora_check(model_path: str, lora_path: str):
    """Validate a GGUF LoRA adapter against its base model (no GPU needed; include/mx_engine.h mx_lora_check);
    raises MxError(MX_ERR_MODEL) with the offending tensor or key named."""
    _check(lib().mx_lora_check(model_path.encode(), lora_path.encode()))


LORA_GUARD = 4096  # elements of 0xFF bytes mx_lora_merge_probe returns behind the merged matrix


def lora_merge_probe(w, A, B, scale: float, iters: int = 0, rows: Optional[int] = None, cols: Optional[int] = None,
                     r: Optional[int] = None, out=None, device: int = 0):
    """The load-time LoRA merge kernel on caller-supplied data (no engine; include/mx_engine.h
    mx_lora_merge_probe): w bf16 bits (uint16) [rows][cols], A f32 [r][cols], B f32 [rows][r].  Returns (merged
    bf16 bits [rows][cols], guard [LORA_GUARD] uint16: must be all-ones bits, microseconds per launch or None
    when iters == 0).  rows / cols / r override what the arrays imply and out (a flat uint16 buffer of rows * cols +
    LORA_GUARD) is worked on directly: what a test of a refusal passes and reads afterwards."""
    wa = np.ascontiguousarray(w, dtype=np.uint16)
    aa = np.ascontiguousarray(A, dtype=np.float32)
    ba = np.ascontiguousarray(B, dtype=np.float32)
    rows = wa.shape[0] if rows is None else rows
    cols = wa.shape[1] if cols is None else cols
    r = aa.shape[0] if r is None else r
    n = max(rows, 0) * max(cols, 0)
    if out is None:
        if wa.shape != (rows, cols) or aa.shape != (r, cols) or ba.shape != (rows, r):
            raise ValueError("w [rows][cols], A [r][cols], B [rows][r] expected")
        ob = np.zeros(n + LORA_GUARD, dtype=np.uint16)
    else:
        ob = out
        if ob.dtype != np.uint16 or ob.ndim != 1 or not ob.flags.c_contiguous or ob.size < wa.size + LORA_GUARD:
            raise ValueError("out: a flat contiguous uint16 buffer of w.size + LORA_GUARD elements")
    us = ctypes.c_double(0.0)
    _check(lib().mx_lora_merge_probe(device, rows, cols, r, wa.ctypes.data, aa.ctypes.data, ba.ctypes.data,
                                     float(scale), ob.ctypes.data, int(iters), ctypes.byref(us)))
    return ob[:n].reshape(rows, cols), ob[n:n + LORA_GUARD], (us.value if iters > 0 else None)


def probe_copy(device: int = 0, gib: int = 4, iters: int = 10, read_only: bool = False):
    """Best streaming rate in GB/s over the probe variants: (read + write) bytes / s of a copy or,
    with read_only, bytes read / s.  Returns (gbs, description of the winning variant)."""
    gbs = ctypes.c_double()
    desc = ctypes.create_string_buffer(160)
    fn = lib().mx_probe_read if read_only else lib().mx_probe_copy
    _check(fn(device, gib << 30, iters, ctypes.byref(gbs), desc, len(desc)))
    return gbs.value, desc.value.decode()


def logprob_probe(logits, targets, k: int, V: Optional[int] = None, device: int = 0):
    """The log-prob kernels on caller-supplied f32 rows (no engine): logits [n][ldl] with V <= ldl valid
    columns (default all), n <= 64.  Returns (tgt_lp [n], top_lp [n][min(k, V)], top_idx [n][min(k, V)])."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    n, ldl = lg.shape
    V = ldl if V is None else V
    tg = _i32(targets)
    if len(tg) != n:
        raise ValueError("one target per row")
    ke = max(0, min(k, V))
    tgt = np.empty(n, dtype=np.float32)
    top = np.empty((n, ke), dtype=np.float32)
    idx = np.empty((n, ke), dtype=np.int32)
    _check(lib().mx_logprob_probe(device, lg.ctypes.data, n, V, ldl, tg.ctypes.data, k, tgt.ctypes.data,
                                  top.ctypes.data if ke else None, idx.ctypes.data if ke else None))
    return tgt, top, idx


def sample_plan(settings: dict, V: int) -> int:
    """Which sampler picks the rows of a request with these settings (the keywords of Engine.submit) over a
    vocabulary of V: one of MX_PICK_ARGMAX / CHAIN / MIROSTAT / WIDE / HOST (include/mx_engine.h mx_sample_plan;
    no GPU).  Settings mx_submit_ext refuses raise MxError(MX_ERR_ARG)."""
    kw = dict(settings)
    ext = {k: kw.pop(k) for k in _EXT_KEYS if k in kw}
    kw.pop("seed", None)
    x, keep = sampling_ext(sampling(**kw), **ext)
    path = ctypes.c_int32(-1)
    _check(lib().mx_sample_plan(ctypes.byref(x), int(V), ctypes.byref(path)))
    del keep
    return path.value


def sample_probe(logits, settings, seeds, n_drawn, windows=None, mu_in=None, V: Optional[int] = None,
                 device: int = 0, want_logits: bool = False):
    """The sampler chain on caller-supplied f32 rows (no engine; include/mx_engine.h mx_sample_probe): logits
    [n][ldl] with V <= ldl valid columns, settings: one keyword dict per row (those of Engine.submit: temperature,
    top_k, ..., typical_p, tfs_z, mirostat_*, logit_bias), seeds / n_drawn [n], windows: the rows' penalty windows
    (<= 64 tokens each), mu_in [n] (default 2 tau).  device >= 0: the production kernels; -1: the host sampler,
    no GPU.  Returns (tokens [n], mu_out [n]) and, with want_logits, the rows as the chain left them."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    n, ldl = lg.shape
    V = ldl if V is None else V
    arr = (MxSamplingExt * max(n, 1))()
    keep = []
    for i in range(min(n, len(arr))):
        kw = dict(settings[i])
        ext = {k: kw.pop(k) for k in _EXT_KEYS if k in kw}
        kw.pop("seed", None)
        keep.append(sampling_ext(sampling(**kw), into=arr[i], **ext)[1])
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    nd = _i32(n_drawn)
    win = np.zeros((max(n, 1), 64), dtype=np.int32)
    nw = np.zeros(max(n, 1), dtype=np.int32)
    for i, w in enumerate(windows or []):
        w = list(w)[-64:]
        win[i, :len(w)] = w
        nw[i] = len(w)
    mu = np.ascontiguousarray(mu_in if mu_in is not None else [2.0 * arr[i].mirostat_tau for i in range(n)],
                              dtype=np.float32)
    if len(sd) != n or len(nd) != n or len(mu) != n:
        raise ValueError("one seed, draw index and mu per row")
    tok = np.zeros(n, dtype=np.int32)
    mu_out = np.zeros(n, dtype=np.float32)
    out = np.empty_like(lg) if want_logits else None
    rc = lib().mx_sample_probe(device, lg.ctypes.data, n, V, ldl, arr, sd.ctypes.data, nd.ctypes.data, win.ctypes.data,
                               nw.ctypes.data, mu.ctypes.data, tok.ctypes.data, mu_out.ctypes.data,
                               out.ctypes.data if out is not None else None)
    if rc != MX_OK:
        err = MxError(rc, lib().mx_last_error().decode(errors="replace"))
        err.outputs = (tok, mu_out)  # still 0xFF bytes after a refusal
        raise err
    return (tok, mu_out, out) if want_logits else (tok, mu_out)


def draft_probe(seqs, num_pred_tokens: int, max_ngram_size: int, pos0=None, slot0=None, device: int = 0):
    """The prompt-lookup draft kernel on caller-supplied token sequences (no engine; include/mx_engine.h
    mx_draft_probe).  Returns (ids, pos, slot) [R][1 + D] -- rows 1..D written by the kernel, ids[:, 0] still
    -1 -- and n_draft [R]."""
    R, D = len(seqs), int(num_pred_tokens)
    lens = _i32([len(q) for q in seqs])
    stride = max(1, int(lens.max()) if R else 1)
    tok = np.zeros((max(R, 1), stride), dtype=np.int32)
    for r, q in enumerate(seqs):
        tok[r, :len(q)] = q
    p0 = _i32([n - 1 for n in lens] if pos0 is None else pos0)
    s0 = _i32(list(range(R)) if slot0 is None else slot0)
    if len(p0) != R or len(s0) != R:
        raise ValueError("one pos0 / slot0 per sequence")
    shape = (max(R, 0), 1 + max(D, 0))
    ids, pos, slot = (np.zeros(shape, dtype=np.int32) for _ in range(3))
    nd = np.zeros(max(R, 0), dtype=np.int32)
    _check(lib().mx_draft_probe(device, R, tok.ctypes.data, stride, lens.ctypes.data, D, int(max_ngram_size),
                                p0.ctypes.data, s0.ctypes.data, ids.ctypes.data, pos.ctypes.data, slot.ctypes.data,
                                nd.ctypes.data))
    return ids, pos, slot, nd


def accept_probe(logits, draft, n_draft, pos0, device: int = 0):
    """argmax + the speculation accept kernel on caller-supplied rows (mx_accept_probe): logits [R][1 + D][V]
    f32, draft [R][D], n_draft [R], pos0 [R].  Returns dict(a [R], emitted [R][1 + D] (-1 past a + 1 tokens),
    next_id [R], new_pos [R], counts [R][3] = steps, drafted, accepted)."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    R, D1, V = lg.shape
    D = D1 - 1
    dr, nd, p0 = _i32(draft).reshape(R, -1), _i32(n_draft), _i32(pos0)
    if dr.shape != (R, D) or len(nd) != R or len(p0) != R:
        raise ValueError("draft [R][D], n_draft [R], pos0 [R] expected")
    a, nxt, npos = (np.zeros(R, dtype=np.int32) for _ in range(3))
    em = np.zeros((R, D1), dtype=np.int32)
    cnt = np.zeros((R, 3), dtype=np.int32)
    _check(lib().mx_accept_probe(device, R, D, V, lg.ctypes.data, dr.ctypes.data, nd.ctypes.data, p0.ctypes.data,
                                 a.ctypes.data, em.ctypes.data, nxt.ctypes.data, npos.ctypes.data, cnt.ctypes.data))
    return {"a": a, "emitted": em, "next_id": nxt, "new_pos": npos, "counts": cnt}


KV_POS_ALIGN = 64  # kernels.h: KV positions per slot are allocated in multiples of this


def _set_qkv_bias(a, g: dict, keep: list):
    """The optional "bias" of a matmul probe's qkv= dict (the q/k/v bias, added to each finished row sum before
    RoPE) into the argument struct `a`; the array is kept alive in `keep`."""
    if g.get("bias") is None:
        return
    qb = np.ascontiguousarray(g["bias"], dtype=np.float32)
    if qb.size != (g["n_head"] + 2 * g["n_head_kv"]) * g["head_dim"]:
        raise ValueError("bias [(n_head + 2 n_head_kv) * head_dim] expected")
    a.bias = qb.ctypes.data
    keep.append(qb)


def attention_probe(mode: int, n_head: int, n_head_kv: int, head_dim: int, n_ctx: int, n_slots: int, pos, slot,
                    kcache, vcache, q=None, slabs=None, rope_cs=None, out_f32: bool = True, device: int = 0, bias=None):
    """The production attention launchers on caller-supplied q / K / V (no engine; include/mx_engine.h
    mx_attention_probe).  kcache / vcache: the raw tiled f16 bits (uint16) of n_slots x n_head_kv x ctx_stride x
    head_dim elements each, left untouched.  mode 0 / 2: q [M][n_head * head_dim] f32 (decode / prefill
    kernel); mode 1: slabs [nslab][M][(n_head + 2 n_head_kv) * head_dim] f32 and rope_cs [n_ctx][head_dim/2][2],
    optionally bias [(n_head + 2 n_head_kv) * head_dim] f32 (the q/k/v bias, added to the summed slabs before RoPE).
    Returns (out [M][n_head * head_dim] as f32 -- a bf16 output widened exactly --, kcache after, vcache after)."""
    pos, slot = _i32(pos), _i32(slot)
    M = len(pos)
    if len(slot) != M:
        raise ValueError("one slot per row")
    ctx_stride = (max(n_ctx, 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
    elems = max(n_slots, 0) * max(n_head_kv, 0) * ctx_stride * max(head_dim, 0)
    kc = np.array(kcache, dtype=np.uint16, copy=True).reshape(-1)
    vc = np.array(vcache, dtype=np.uint16, copy=True).reshape(-1)
    if kc.size != elems or vc.size != elems:
        raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
    nq, N = n_head * head_dim, (n_head + 2 * n_head_kv) * head_dim
    qa = sa = ca = None
    nslab = 0
    if mode == 1:
        sa = np.ascontiguousarray(slabs, dtype=np.float32)
        ca = np.ascontiguousarray(rope_cs, dtype=np.float32)
        nslab = sa.shape[0]
        if sa.shape != (nslab, M, N) or ca.size != max(n_ctx, 0) * head_dim:
            raise ValueError("slabs [nslab][M][n_q + 2 n_kv] and rope_cs [n_ctx][head_dim/2][2] expected")
    else:
        qa = np.ascontiguousarray(q, dtype=np.float32)
        if qa.size != M * nq:
            raise ValueError("q [M][n_head * head_dim] expected")
    ba = None
    if bias is not None:  # mode 1: the q/k/v bias, added to the summed slabs before RoPE
        ba = np.ascontiguousarray(bias, dtype=np.float32)
        if ba.size != N:
            raise ValueError("bias [(n_head + 2 n_head_kv) * head_dim] expected")
    out = np.empty((M, max(nq, 0)), dtype=np.float32 if out_f32 else np.uint16)
    _check(lib().mx_attention_probe(device, mode, n_head, n_head_kv, head_dim, n_ctx, n_slots, M, pos.ctypes.data,
                                    slot.ctypes.data, int(bool(out_f32)), qa.ctypes.data if qa is not None else None,
                                    sa.ctypes.data if sa is not None else None, nslab,
                                    ca.ctypes.data if ca is not None else None, kc.ctypes.data, vc.ctypes.data,
                                    out.ctypes.data, ba.ctypes.data if ba is not None else None))
    if not out_f32:
        out = (out.astype(np.uint32) << 16).view(np.float32)
    return out, kc, vc


def kv_copy_probe(n_layer: int, n_slots: int, n_head_kv: int, head_dim: int, n_ctx: int, copies, kcache, vcache,
                  device: int = 0, inplace: bool = False):
    """The prefix-sharing copy kernel on caller-supplied caches (no engine; include/mx_engine.h mx_kv_copy_probe).
    kcache / vcache: the raw tiled f16 bits (uint16) of n_layer x n_slots x n_head_kv x ctx_stride x head_dim
    elements each, left untouched unless `inplace` (flat contiguous uint16 arrays the call works on directly: what
    a test of a refusal reads afterwards); copies: [(src_slot, dst_slot, n_pos)].  Returns (kcache after, vcache
    after); a refused table raises MxError(MX_ERR_ARG)."""
    ctx_stride = (max(n_ctx, 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
    elems = max(n_layer, 0) * max(n_slots, 0) * max(n_head_kv, 0) * ctx_stride * max(head_dim, 0)
    if inplace:
        kc, vc = kcache, vcache
        if any(a.dtype != np.uint16 or a.ndim != 1 or not a.flags.c_contiguous for a in (kc, vc)):
            raise ValueError("inplace takes flat contiguous uint16 arrays")
    else:
        kc = np.array(kcache, dtype=np.uint16, copy=True).reshape(-1)
        vc = np.array(vcache, dtype=np.uint16, copy=True).reshape(-1)
    if kc.size != elems or vc.size != elems:
        raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
    tab = (MxKvCopy * max(len(copies), 1))()
    for i, (s, d, n) in enumerate(copies):
        tab[i].src_slot, tab[i].dst_slot, tab[i].n_pos = int(s), int(d), int(n)
    _check(lib().mx_kv_copy_probe(device, n_layer, n_slots, n_head_kv, head_dim, n_ctx, len(copies), tab,
                                  kc.ctypes.data, vc.ctypes.data))
    return kc, vc


KV_PACK_GUARD_BYTES = 4096  # mx_engine.h MX_KV_PACK_GUARD_BYTES: 0xFF bytes behind a packed output


def kv_pack_probe(direction: int, n_layer: int, n_slots: int, n_head_kv: int, head_dim: int, n_ctx: int, entries,
                  kcache, vcache, packed=None, packed_bytes: int = 0, device: int = 0, inplace: bool = False):
    """The host tier's pack (direction 0) and unpack (1) kernels on caller-supplied caches (no engine;
    include/mx_engine.h mx_kv_pack_probe).  kcache / vcache as for kv_copy_probe; entries: [(slot, n_pos, offset in
    16-byte words)].  Packing returns (packed bytes [packed_bytes + KV_PACK_GUARD_BYTES] uint8, kcache after, vcache
    after): the buffer starts as 0xFF bytes.  Unpacking takes `packed` (uint8) and returns (kcache after, vcache
    after).  With `inplace` the flat uint16 caches -- and, packing, a flat uint8 `packed` of packed_bytes +
    KV_PACK_GUARD_BYTES -- are worked on directly (what a test of a refusal reads afterwards).  A refused table
    raises MxError(MX_ERR_ARG)."""
    ctx_stride = (max(n_ctx, 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
    elems = max(n_layer, 0) * max(n_slots, 0) * max(n_head_kv, 0) * ctx_stride * max(head_dim, 0)
    if inplace:
        kc, vc = kcache, vcache
        if any(a.dtype != np.uint16 or a.ndim != 1 or not a.flags.c_contiguous for a in (kc, vc)):
            raise ValueError("inplace takes flat contiguous uint16 arrays")
    else:
        kc = np.array(kcache, dtype=np.uint16, copy=True).reshape(-1)
        vc = np.array(vcache, dtype=np.uint16, copy=True).reshape(-1)
    if kc.size != elems or vc.size != elems:
        raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
    if direction == 0:
        if inplace and packed is not None:
            pk = packed
            if pk.dtype != np.uint8 or pk.ndim != 1 or not pk.flags.c_contiguous:
                raise ValueError("inplace takes a flat contiguous uint8 packed buffer")
        else:
            pk = np.zeros(max(int(packed_bytes), 0) + KV_PACK_GUARD_BYTES, dtype=np.uint8)
        if pk.size != packed_bytes + KV_PACK_GUARD_BYTES:
            raise ValueError("the packed output holds packed_bytes + KV_PACK_GUARD_BYTES bytes")
    else:
        pk = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
        packed_bytes = pk.size
    tab = (MxKvPack * max(len(entries), 1))()
    for i, (s, n, o) in enumerate(entries):
        tab[i].slot, tab[i].n_pos, tab[i].offset16 = int(s), int(n), int(o)
    _check(lib().mx_kv_pack_probe(device, int(direction), n_layer, n_slots, n_head_kv, head_dim, n_ctx, len(entries),
                                  tab, kc.ctypes.data, vc.ctypes.data, pk.ctypes.data, int(packed_bytes)))
    return (pk, kc, vc) if direction == 0 else (kc, vc)


EPI_F32, EPI_RESID, EPI_QKV, EPI_SWIGLU = 0, 1, 2, 3  # kernels.h Epilogue
PROBE_GUARD_ROWS = 64  # rows of 0xFF bytes the probes return after every output


def matmul_plan(epi: int, M: int, N: int, K: int) -> dict:
    """Dispatch facts of a bf16 matmul shape (mx_matmul_plan; no GPU): kgroups, pers_ok, norm_on_load_ok,
    gemm_ok."""
    v = [ctypes.c_int32() for _ in range(4)]
    _check(lib().mx_matmul_plan(epi, M, N, K, *[ctypes.byref(c) for c in v]))
    return {"kgroups": v[0].value, "pers_ok": bool(v[1].value), "norm_on_load_ok": bool(v[2].value),
            "gemm_ok": bool(v[3].value)}


class MatmulResult:
    """out [M][ld] (f32, or the raw bf16 bits for a bf16 SWIGLU act), guard [64][ld] (the same dtype: must be
    all-ones bits), split (what the launcher returned), ssq [M][N/16], slabs ([split][M][N] on paths 2 / 3, the
    flat slab space on path 4), packed (uint16 [N*K]), kcache / vcache (after the launch)."""
    out = guard = ssq = slabs = packed = kcache = vcache = None
    split = 0


def matmul_probe(path: int, epi: int, w, x=None, *, xf=None, norm_w=None, eps: float = 0.0, resid=None, qkv=None,
                 want_ssq: bool = False, act_f32: bool = False, target: int = 0, slab_floats: int = 0,
                 want_slabs: bool = False, want_packed: bool = False, out=None, device: int = 0) -> MatmulResult:
    """A production bf16 matmul launcher on caller-supplied operands (no engine; include/mx_engine.h
    mx_matmul_probe).  w: bf16 bits (uint16) [N][K] in GGUF order; x: bf16 bits [M][K], or xf f32 [M][K] with
    norm_w f32 [K] (RMS_NORM on load); resid f32 [M][N] (RESID); qkv: dict(n_head, n_head_kv, head_dim, n_ctx,
    n_slots, pos, slot, rope_cs, kcache, vcache) with the caches as in attention_probe, and optionally bias (f32
    [N], the q/k/v bias added to each finished row sum before RoPE; the same key serves q8_matmul_probe and
    kq_matmul_probe).  out (optional): a caller-owned buffer for the [M + 64][ld] result (tests of refusals)."""
    wa = np.ascontiguousarray(w, dtype=np.uint16)
    N, K = wa.shape
    xa = fa = na = ra = None
    if x is not None:
        xa = np.ascontiguousarray(x, dtype=np.uint16)
        M = xa.shape[0]
        if xa.ndim != 2 or xa.shape[1] != K:
            raise ValueError("x [M][K] expected")
    else:
        if xf is None:
            raise ValueError("x or xf expected")
        fa = np.ascontiguousarray(xf, dtype=np.float32)
        M = fa.shape[0]
        if fa.ndim != 2 or fa.shape[1] != K:
            raise ValueError("xf [M][K] expected")
        if norm_w is not None:
            na = np.ascontiguousarray(norm_w, dtype=np.float32)
            if na.size != K:
                raise ValueError("norm_w [K] expected")
    a = MxMatmulArgs()
    a.path, a.epi, a.M, a.N, a.K = path, epi, M, N, K
    a.w = wa.ctypes.data
    a.x = xa.ctypes.data if xa is not None else None
    a.xf = fa.ctypes.data if fa is not None else None
    a.norm_w = na.ctypes.data if na is not None else None
    a.eps, a.target, a.slab_floats = eps, target, slab_floats
    a.want_ssq, a.act_f32 = int(bool(want_ssq)), int(bool(act_f32))
    ld = N
    keep = [wa, xa, fa, na]
    kc = vc = None
    if resid is not None:
        ra = np.ascontiguousarray(resid, dtype=np.float32)
        if ra.shape != (M, N):
            raise ValueError("resid [M][N] expected")
        a.resid = ra.ctypes.data
        keep.append(ra)
    if epi == EPI_SWIGLU:
        ld = N // 2
    if qkv is not None:
        g = qkv
        a.n_head, a.n_head_kv, a.head_dim = g["n_head"], g["n_head_kv"], g["head_dim"]
        a.n_ctx, a.n_slots = g["n_ctx"], g["n_slots"]
        ld = max(g["n_head"] * g["head_dim"], 1)
        for name in ("pos", "slot"):
            if g.get(name) is not None:
                arr = _i32(g[name])
                if len(arr) != M:
                    raise ValueError(f"one {name} per row")
                setattr(a, name, arr.ctypes.data)
                keep.append(arr)
        if g.get("rope_cs") is not None:
            cs = np.ascontiguousarray(g["rope_cs"], dtype=np.float32)
            if cs.size != max(g["n_ctx"], 0) * g["head_dim"]:
                raise ValueError("rope_cs [n_ctx][head_dim/2][2] expected")
            a.rope_cs = cs.ctypes.data
            keep.append(cs)
        _set_qkv_bias(a, g, keep)
        stride = (max(g["n_ctx"], 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
        elems = max(g["n_slots"], 0) * max(g["n_head_kv"], 0) * stride * max(g["head_dim"], 0)
        if g.get("kcache") is not None and g.get("vcache") is not None:
            kc = np.array(g["kcache"], dtype=np.uint16, copy=True).reshape(-1)
            vc = np.array(g["vcache"], dtype=np.uint16, copy=True).reshape(-1)
            if kc.size != elems or vc.size != elems:
                raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
            a.kcache, a.vcache = kc.ctypes.data, vc.ctypes.data
    dt = np.uint16 if (epi == EPI_SWIGLU and not act_f32) else np.float32
    rows = max(M, 0) + PROBE_GUARD_ROWS
    if out is None:
        ob = np.zeros((rows, ld), dtype=dt)
    else:
        ob = out
        if not ob.flags.c_contiguous or ob.nbytes < rows * ld * np.dtype(dt).itemsize:
            raise ValueError("out too small")
    a.out = ob.ctypes.data
    r = MatmulResult()
    ssq = slabs = packed = None
    split = ctypes.c_int32(0)
    a.split_out = ctypes.addressof(split)
    if want_ssq:
        ssq = np.zeros((max(M, 0), N // 16), dtype=np.float32)
        a.ssq_out = ssq.ctypes.data
    if want_slabs:
        cap = slab_floats if path == 4 else 16 * max(M, 0) * N
        slabs = np.zeros(max(cap, 1), dtype=np.float32)
        a.slabs_out, a.slabs_cap = slabs.ctypes.data, cap
    if want_packed:
        packed = np.zeros(N * K, dtype=np.uint16)
        a.packed_out = packed.ctypes.data
    _check(lib().mx_matmul_probe(device, ctypes.byref(a)))
    del keep
    flat = ob.reshape(-1).view(dt)[:rows * ld].reshape(rows, ld)
    r.out, r.guard, r.split = flat[:M], flat[M:], split.value
    r.ssq, r.packed, r.kcache, r.vcache = ssq, packed, kc, vc
    if want_slabs:
        if path == 4:
            r.slabs = slabs[:slab_floats]
        else:
            r.slabs = slabs[:max(r.split, 0) * M * N].reshape(-1, M, N)
    return r


def norm_probe(x, slabs=None, w=None, row_map=None, eps: float = 0.0, device: int = 0):
    """launch_resid_norm / launch_rmsnorm on caller-supplied rows (mx_norm_probe): x f32 [rows][n], slabs
    [nslab][rows][n], w [n], row_map [M].  Returns (x after [rows][n], x guard [64][n] as uint32, y bf16 bits
    [M][n] or None, y guard [64][n] or None)."""
    xa = np.ascontiguousarray(x, dtype=np.float32)
    rows, n = xa.shape
    sa = wa = ma = None
    nslab = 0
    if slabs is not None:
        sa = np.ascontiguousarray(slabs, dtype=np.float32)
        nslab = sa.shape[0]
        if sa.shape != (nslab, rows, n):
            raise ValueError("slabs [nslab][rows][n] expected")
        if nslab == 0:
            sa = None
    if w is not None:
        wa = np.ascontiguousarray(w, dtype=np.float32)
        if wa.size != n:
            raise ValueError("w [n] expected")
    M = rows
    if row_map is not None:
        ma = _i32(row_map)
        M = len(ma)
    xo = np.zeros((rows + PROBE_GUARD_ROWS, n), dtype=np.float32)
    yo = np.zeros((M + PROBE_GUARD_ROWS, n), dtype=np.uint16) if wa is not None else None
    _check(lib().mx_norm_probe(device, rows, n, M, xa.ctypes.data, sa.ctypes.data if sa is not None else None, nslab,
                               wa.ctypes.data if wa is not None else None, ma.ctypes.data if ma is not None else None,
                               eps, xo.ctypes.data, yo.ctypes.data if yo is not None else None))
    return (xo[:rows], xo[rows:].view(np.uint32), yo[:M] if yo is not None else None,
            yo[M:] if yo is not None else None)


Q8_KIND = {0: "none", 1: "ql", 2: "pers_ql", 3: "mq8", 4: "wide", 5: "wsw", 6: "gemm"}


def q8_matmul_plan(epi: int, M: int, N: int, K: int, wq4: bool = False, on_load: bool = False,
                   norm: bool = False) -> dict:
    """The kernel a Q8_0 / Q4_0 shape reaches (mx_q8_matmul_plan; no GPU): kind (a Q8_KIND name) and the
    fields of mx_q8_plan."""
    pl = MxQ8Plan()
    _check(lib().mx_q8_matmul_plan(epi, M, N, K, int(bool(wq4)), int(bool(on_load)), int(bool(norm)), ctypes.byref(pl)))
    d = {n: getattr(pl, n) for n, _ in MxQ8Plan._fields_}
    d["kind"] = Q8_KIND[d["kind"]]
    d["can_on_load"] = bool(d["can_on_load"])
    return d


class Q8Result:
    """out / guard as MatmulResult (always f32); xq int8 [M][K] (q8_perm order) / xd f32 [M][K/32] with their
    guards xq_guard / xd_guard; x (act 1: the rows after the fold); split, ssq [M][N/16] + ssq_guard [64][N/16], slabs [ks][M][N], packed (uint8);
    nxq / nxd (+ guards): the folding norm's Q8_0 rows on path 1 RESID; kcache / vcache."""
    out = guard = ssq = ssq_guard = slabs = packed = kcache = vcache = xq = xd = xq_guard = xd_guard = x = None
    nxq = nxd = nxq_guard = nxd_guard = None
    split = 0


def q8_matmul_probe(path: int, epi: int, w, xf, *, wq4: bool = False, act: int = 0, N: Optional[int] = None,
                    K: Optional[int] = None, M: Optional[int] = None, ldx: int = 0, norm_w=None, eps: float = 0.0,
                    row_map=None, fold_slabs=None, resid=None, fold_w=None, qkv=None, want_ssq: bool = False,
                    act_f32: bool = True, want_slabs: bool = False, want_packed: bool = False, want_x: bool = True,
                    np_partials: int = 0, out=None, device: int = 0) -> Q8Result:
    """A production Q8_0 / Q4_0 launcher on caller-supplied operands (include/mx_engine.h mx_q8_matmul_probe).
    w: raw GGUF blocks uint8 [N][K/32 * 34] (wq4: [N][K/32 * 18]), None on path -1; xf f32 rows; act 0 quantise
    (xf [M][ldx]), 1 RMS_NORM + quantise (norm_w, row_map, fold_slabs [nslab][rows][K]), 2 quantise on load.  N /
    K / M override what the arrays imply (tests of refusals)."""
    fa = np.ascontiguousarray(xf, dtype=np.float32)
    if fa.ndim != 2:
        raise ValueError("xf [rows][ld] expected")
    wa = None
    if w is not None:
        wa = np.ascontiguousarray(w, dtype=np.uint8)
        bb = 18 if wq4 else 34
        if wa.ndim != 2 or wa.shape[1] % bb:
            raise ValueError("w [N][K/32 * block bytes] expected")
        if N is None:
            N = wa.shape[0]
        if K is None:
            K = wa.shape[1] // bb * 32
    if K is None:
        if ldx:
            raise ValueError("K is required when ldx is given without w")
        K = fa.shape[1]
    if N is None:
        N = 0
    a = MxQ8MatmulArgs()
    ma = None
    if row_map is not None:
        ma = _i32(row_map)
        a.row_map = ma.ctypes.data
    m_given = M is not None
    if M is None:
        M = len(ma) if ma is not None else fa.shape[0]
    a.path, a.epi, a.M, a.N, a.K, a.wq4, a.act = path, epi, M, N, K, int(bool(wq4)), act
    a.w = wa.ctypes.data if wa is not None else None
    a.xf, a.xrows, a.ldx = fa.ctypes.data, (fa.shape[0] if act == 1 else 0), ldx
    if act != 1 and fa.shape[0] < M and not m_given:
        raise ValueError("xf holds fewer than M rows")
    if fa.shape[1] != (ldx or K):
        raise ValueError("xf row length")
    keep = [wa, fa, ma]
    if norm_w is not None:
        na = np.ascontiguousarray(norm_w, dtype=np.float32)
        if na.size != K:
            raise ValueError("norm_w [K] expected")
        a.norm_w = na.ctypes.data
        keep.append(na)
    a.eps = eps
    if fold_slabs is not None:
        sa = np.ascontiguousarray(fold_slabs, dtype=np.float32)
        if sa.ndim != 3 or sa.shape[1:] != fa.shape:
            raise ValueError("fold_slabs [nslab][rows][K] expected")
        a.nslab = sa.shape[0]
        if a.nslab:
            a.fold_slabs = sa.ctypes.data
        keep.append(sa)
    a.want_ssq, a.act_f32, a.np = int(bool(want_ssq)), int(bool(act_f32)), np_partials
    if resid is not None:
        ra = np.ascontiguousarray(resid, dtype=np.float32)
        if ra.shape != (M, N):
            raise ValueError("resid [M][N] expected")
        a.resid = ra.ctypes.data
        keep.append(ra)
    if fold_w is not None:
        fw = np.ascontiguousarray(fold_w, dtype=np.float32)
        if fw.size != N:
            raise ValueError("fold_w [N] expected")
        a.fold_w = fw.ctypes.data
        keep.append(fw)
    ld = N // 2 if epi == EPI_SWIGLU else N
    kc = vc = None
    if qkv is not None:
        g = qkv
        a.n_head, a.n_head_kv, a.head_dim = g["n_head"], g["n_head_kv"], g["head_dim"]
        a.n_ctx, a.n_slots = g["n_ctx"], g["n_slots"]
        ld = max(g["n_head"] * g["head_dim"], 1)
        for name in ("pos", "slot"):
            if g.get(name) is not None:
                arr = _i32(g[name])
                if len(arr) != M:
                    raise ValueError(f"one {name} per row")
                setattr(a, name, arr.ctypes.data)
                keep.append(arr)
        if g.get("rope_cs") is not None:
            cs = np.ascontiguousarray(g["rope_cs"], dtype=np.float32)
            if cs.size != max(g["n_ctx"], 0) * g["head_dim"]:
                raise ValueError("rope_cs [n_ctx][head_dim/2][2] expected")
            a.rope_cs = cs.ctypes.data
            keep.append(cs)
        _set_qkv_bias(a, g, keep)
        stride = (max(g["n_ctx"], 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
        elems = max(g["n_slots"], 0) * max(g["n_head_kv"], 0) * stride * max(g["head_dim"], 0)
        if g.get("kcache") is not None and g.get("vcache") is not None:
            kc = np.array(g["kcache"], dtype=np.uint16, copy=True).reshape(-1)
            vc = np.array(g["vcache"], dtype=np.uint16, copy=True).reshape(-1)
            if kc.size != elems or vc.size != elems:
                raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
            a.kcache, a.vcache = kc.ctypes.data, vc.ctypes.data
    Mr = max(M, 0)
    rows = Mr + PROBE_GUARD_ROWS
    ld = max(ld, 0)
    if out is None:
        ob = np.zeros((rows, max(ld, 1)), dtype=np.float32)
    else:
        ob = out
        if not ob.flags.c_contiguous or ob.nbytes < rows * ld * 4:
            raise ValueError("out too small")
    a.out = ob.ctypes.data
    r = Q8Result()
    split = ctypes.c_int32(0)
    a.split_out = ctypes.addressof(split)
    ssq = slabs = packed = xq = xd = xo = nxq = nxd = None
    if want_ssq:
        ssq = np.zeros((rows, max(N // 16, 1)), dtype=np.float32)
        a.ssq_out = ssq.ctypes.data
    if want_slabs:
        slabs = np.zeros(max(8 * Mr * N, 1), dtype=np.float32)
        a.slabs_out, a.slabs_cap = slabs.ctypes.data, 8 * Mr * N
    if want_packed and wa is not None:
        packed = np.zeros(N // 16 * (K // 64) * (576 if wq4 else 1088), dtype=np.uint8)
        a.packed_out = packed.ctypes.data
    if act != 2 and want_x and K > 0:
        xq = np.zeros((rows, K), dtype=np.int8)
        xd = np.zeros((rows, max(K // 32, 1)), dtype=np.float32)
        a.xq_out, a.xd_out = xq.ctypes.data, xd.ctypes.data
        if act == 1:
            xo = np.zeros(fa.shape, dtype=np.float32)
            a.x_out = xo.ctypes.data
    if path == 1 and epi == EPI_RESID and N > 0:
        nxq = np.zeros((rows, N), dtype=np.int8)
        nxd = np.zeros((rows, max(N // 32, 1)), dtype=np.float32)
        a.nxq_out, a.nxd_out = nxq.ctypes.data, nxd.ctypes.data
    _check(lib().mx_q8_matmul_probe(device, ctypes.byref(a)))
    del keep
    if path >= 0:
        flat = ob.reshape(-1).view(np.float32)[:rows * ld].reshape(rows, ld)
        r.out, r.guard = flat[:M], flat[M:]
    r.split, r.packed, r.kcache, r.vcache, r.x = split.value, packed, kc, vc, xo
    if ssq is not None:
        r.ssq, r.ssq_guard = ssq[:M], ssq[M:]
    if xq is not None:
        r.xq, r.xq_guard, r.xd, r.xd_guard = xq[:M], xq[M:], xd[:M], xd[M:]
    if nxq is not None:
        r.nxq, r.nxq_guard, r.nxd, r.nxd_guard = nxq[:M], nxq[M:], nxd[:M], nxd[M:]
    if want_slabs:
        r.slabs = slabs[:max(r.split, 0) * M * N].reshape(-1, M, N)
    return r


def q8_dequant_tiles_probe(blocks, device: int = 0):
    """launch_dequant_q8_tiles on Q8_0 blocks uint8 [N][K/32 * 34] packed as at load: (packed bf16 tiles uint16
    [N * K], guard uint16 [64 * K])."""
    ba = np.ascontiguousarray(blocks, dtype=np.uint8)
    N, K = ba.shape[0], ba.shape[1] // 34 * 32
    ob = np.zeros((N + PROBE_GUARD_ROWS) * K, dtype=np.uint16)
    _check(lib().mx_q8_side_probe(device, 0, N, K, ba.ctypes.data, None, 0, ob.ctypes.data, None))
    return ob[:N * K], ob[N * K:]


def q8_embed_probe(blocks, ids, want_ssq: bool = True, device: int = 0):
    """launch_embed_q8: rows `ids` of a Q8_0 token_embd (blocks uint8 [n_vocab][n/32 * 34]) -> (x f32 [M][n], x
    guard as uint32, ssq [M][n/16] or None, ssq guard or None)."""
    ba = np.ascontiguousarray(blocks, dtype=np.uint8)
    N, K = ba.shape[0], ba.shape[1] // 34 * 32
    ia = _i32(ids)
    M = len(ia)
    ob = np.zeros((M + PROBE_GUARD_ROWS, K), dtype=np.float32)
    sq = np.zeros((M + PROBE_GUARD_ROWS, K // 16), dtype=np.float32) if want_ssq else None
    _check(lib().mx_q8_side_probe(device, 1, N, K, ba.ctypes.data, ia.ctypes.data, M, ob.ctypes.data,
                                  sq.ctypes.data if sq is not None else None))
    return ob[:M], ob[M:].view(np.uint32), (sq[:M] if sq is not None else None), (sq[M:] if sq is not None else None)


KQ_KIND = {0: "none", 1: "qkv_pers", 2: "bd_tile", 3: "pers", 4: "wide", 5: "mkq"}
KQ_BLOCK_BYTES = {12: 144, 13: 176, 14: 210}   # GGUF Q4_K / Q5_K / Q6_K bytes per 256 weights
KQ_TILE_BYTES = {12: 2368, 13: 2880, 14: 3360}  # packed 16-row x 256-k tile (kquant.hip)
KQ_NO_BD_TILE, KQ_NO_PERS, KQ_NO_WIDE = 1, 2, 4  # kq_matmul_plan flags: the MX_NO_KQ_* switches as if set


def _kq_segments(segs, N=None):
    """[(type, tile_end), ...] -> (kq_n, c_int32[3] types, c_int32[3] ends); a bare type with N: one segment."""
    if isinstance(segs, int):
        segs = [(segs, N // 16)]
    segs = list(segs)
    if not 1 <= len(segs) <= 3:
        raise ValueError("1..3 row segments expected")
    ty, te = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
    for i, (t, e) in enumerate(segs):
        ty[i], te[i] = t, e
    return len(segs), ty, te


def kq_matmul_plan(epi: int, M: int, N: int, K: int, segs, on_load: bool = False, norm: bool = False,
                   flags: int = -1) -> dict:
    """The kernel a K-quant shape reaches (mx_kq_matmul_plan; no GPU): kind (a KQ_KIND name) and the fields of
    mx_kq_plan.  segs: a ggml type (one segment) or [(type, tile_end), ...]; flags: -1 = this process's MX_NO_KQ_*
    switches, else KQ_NO_* bits."""
    n, ty, te = _kq_segments(segs, N)
    pl = MxKqPlan()
    _check(lib().mx_kq_matmul_plan(epi, M, N, K, int(bool(on_load)), int(bool(norm)), n, ctypes.addressof(ty),
                                   ctypes.addressof(te), flags, ctypes.byref(pl)))
    d = {f: getattr(pl, f) for f, _ in MxKqPlan._fields_}
    d["kind"] = KQ_KIND[d["kind"]]
    d["can_on_load"] = bool(d["can_on_load"])
    return d


class KqResult:
    """out / guard as MatmulResult (always f32); xq int8 [M][K] (permuted within super-blocks), xd f32 [M][K/256],
    xb f32 [M][K/32] with their guards; split, ssq [M][N/16] + ssq_guard, slabs [ks][M][N], packed (uint8);
    nxq / nxd / nxb (+ guards): the folding norm's Q8_K rows on path 1 (N % 256 == 0, N <= 4096); kcache / vcache."""
    out = guard = ssq = ssq_guard = slabs = packed = kcache = vcache = None
    xq = xd = xb = xq_guard = xd_guard = xb_guard = None
    nxq = nxd = nxb = nxq_guard = nxd_guard = nxb_guard = None
    split = 0


def kq_matmul_probe(path: int, epi: int, w, xf, segs, *, act: int = 0, N: Optional[int] = None,
                    K: Optional[int] = None, M: Optional[int] = None, ldx: int = 0, norm_w=None, eps: float = 0.0,
                    row_map=None, ssq_in=None, resid=None, fold_w=None, qkv=None, want_ssq: bool = False,
                    want_slabs: bool = False, want_packed: bool = False, out=None, device: int = 0) -> KqResult:
    """A production K-quant launcher on caller-supplied operands (include/mx_engine.h mx_kq_matmul_probe).
    w: raw GGUF blocks, flat uint8 (the row segments laid end to end), None on path -1; segs: a ggml type (one
    segment; N then required) or [(type, tile_end), ...]; xf f32 rows; act 0 quantise (xf [M][ldx]), 1 RMS_NORM +
    quantise (norm_w, row_map), 2 one token quantised on load (norm_w, ssq_in optional).  N / K / M override what
    the arrays imply (tests of refusals)."""
    fa = np.ascontiguousarray(xf, dtype=np.float32)
    if fa.ndim != 2:
        raise ValueError("xf [rows][ld] expected")
    if K is None:
        if ldx:
            raise ValueError("K is required when ldx is given")
        K = fa.shape[1]
    a = MxKqMatmulArgs()
    wa = None
    if w is not None:
        wa = np.ascontiguousarray(w, dtype=np.uint8).reshape(-1)
        if N is None:
            if isinstance(segs, int):
                raise ValueError("N is required with a bare type")
            N = 16 * list(segs)[-1][1]
        a.kq_n, ty, te = _kq_segments(segs, N)
        need, t0 = 0, 0
        for i in range(a.kq_n):
            a.kq_type[i], a.kq_tile_end[i] = ty[i], te[i]
            need += max(te[i] - t0, 0) * 16 * (K // 256) * KQ_BLOCK_BYTES.get(ty[i], 0)
            t0 = te[i]
        if wa.size < need:
            raise ValueError(f"w holds {wa.size} bytes, the segments need {need}")
    if N is None:
        N = 0
    ma = None
    if row_map is not None:
        ma = _i32(row_map)
        a.row_map = ma.ctypes.data
    if M is None:
        M = len(ma) if ma is not None else fa.shape[0]
    a.path, a.epi, a.M, a.N, a.K, a.act = path, epi, M, N, K, act
    a.w = wa.ctypes.data if wa is not None else None
    a.xf, a.xrows, a.ldx = fa.ctypes.data, (fa.shape[0] if act == 1 else 0), ldx
    if fa.shape[1] != (ldx or K):
        raise ValueError("xf row length")
    if act != 1 and fa.shape[0] < (1 if act == 2 else M):  # the rows the probe copies (act 1: xrows, checked in C)
        raise ValueError("xf holds fewer rows than the probe reads")
    keep = [wa, fa, ma]
    if norm_w is not None:
        na = np.ascontiguousarray(norm_w, dtype=np.float32)
        if na.size != K:
            raise ValueError("norm_w [K] expected")
        a.norm_w = na.ctypes.data
        keep.append(na)
    if ssq_in is not None:
        qa_ = np.ascontiguousarray(ssq_in, dtype=np.float32)
        if qa_.size != K // 16:
            raise ValueError("ssq_in [K/16] expected")
        a.ssq_in = qa_.ctypes.data
        keep.append(qa_)
    a.eps, a.want_ssq = eps, int(bool(want_ssq))
    if resid is not None:
        ra = np.ascontiguousarray(resid, dtype=np.float32)
        if ra.shape != (M, N):
            raise ValueError("resid [M][N] expected")
        a.resid = ra.ctypes.data
        keep.append(ra)
    if fold_w is not None:
        fw = np.ascontiguousarray(fold_w, dtype=np.float32)
        if fw.size != N:
            raise ValueError("fold_w [N] expected")
        a.fold_w = fw.ctypes.data
        keep.append(fw)
    ld = N // 2 if epi == EPI_SWIGLU else N
    kc = vc = None
    if qkv is not None:
        g = qkv
        a.n_head, a.n_head_kv, a.head_dim = g["n_head"], g["n_head_kv"], g["head_dim"]
        a.n_ctx, a.n_slots = g["n_ctx"], g["n_slots"]
        ld = max(g["n_head"] * g["head_dim"], 1)
        for name in ("pos", "slot"):
            if g.get(name) is not None:
                arr = _i32(g[name])
                if len(arr) != M:
                    raise ValueError(f"one {name} per row")
                setattr(a, name, arr.ctypes.data)
                keep.append(arr)
        if g.get("rope_cs") is not None:
            cs = np.ascontiguousarray(g["rope_cs"], dtype=np.float32)
            if cs.size != max(g["n_ctx"], 0) * g["head_dim"]:
                raise ValueError("rope_cs [n_ctx][head_dim/2][2] expected")
            a.rope_cs = cs.ctypes.data
            keep.append(cs)
        _set_qkv_bias(a, g, keep)
        stride = (max(g["n_ctx"], 0) + KV_POS_ALIGN - 1) // KV_POS_ALIGN * KV_POS_ALIGN
        elems = max(g["n_slots"], 0) * max(g["n_head_kv"], 0) * stride * max(g["head_dim"], 0)
        if g.get("kcache") is not None and g.get("vcache") is not None:
            kc = np.array(g["kcache"], dtype=np.uint16, copy=True).reshape(-1)
            vc = np.array(g["vcache"], dtype=np.uint16, copy=True).reshape(-1)
            if kc.size != elems or vc.size != elems:
                raise ValueError(f"caches hold {kc.size} / {vc.size} elements, the geometry needs {elems}")
            a.kcache, a.vcache = kc.ctypes.data, vc.ctypes.data
    Mr = max(M, 0)
    rows = Mr + PROBE_GUARD_ROWS
    ld = max(ld, 0)
    if out is None:
        ob = np.zeros((rows, max(ld, 1)), dtype=np.float32)
    else:
        ob = out
        if not ob.flags.c_contiguous or ob.nbytes < rows * ld * 4:
            raise ValueError("out too small")
    a.out = ob.ctypes.data
    r = KqResult()
    split = ctypes.c_int32(0)
    a.split_out = ctypes.addressof(split)
    ssq = slabs = packed = xq = xd = xb = nxq = nxd = nxb = None
    if want_ssq:
        ssq = np.zeros((rows, max(N // 16, 1)), dtype=np.float32)
        a.ssq_out = ssq.ctypes.data
    if want_slabs:
        slabs = np.zeros(max(8 * Mr * N, 1), dtype=np.float32)
        a.slabs_out, a.slabs_cap = slabs.ctypes.data, 8 * Mr * N
    if want_packed and wa is not None:
        t0, nbytes = 0, 0
        for i in range(a.kq_n):
            nbytes += (a.kq_tile_end[i] - t0) * (K // 256) * KQ_TILE_BYTES.get(a.kq_type[i], 0)
            t0 = a.kq_tile_end[i]
        packed = np.zeros(max(nbytes, 1), dtype=np.uint8)
        a.packed_out = packed.ctypes.data
    if act != 2 and K >= 256:
        xq = np.zeros((rows, K), dtype=np.int8)
        xd = np.zeros((rows, K // 256), dtype=np.float32)
        xb = np.zeros((rows, K // 32), dtype=np.float32)
        a.xq_out, a.xd_out, a.xb_out = xq.ctypes.data, xd.ctypes.data, xb.ctypes.data
    if path == 1 and N > 0 and N % 256 == 0 and N <= 4096:
        nxq = np.zeros((rows, N), dtype=np.int8)
        nxd = np.zeros((rows, N // 256), dtype=np.float32)
        nxb = np.zeros((rows, N // 32), dtype=np.float32)
        a.nxq_out, a.nxd_out, a.nxb_out = nxq.ctypes.data, nxd.ctypes.data, nxb.ctypes.data
    _check(lib().mx_kq_matmul_probe(device, ctypes.byref(a)))
    del keep
    if path >= 0:
        flat = ob.reshape(-1).view(np.float32)[:rows * ld].reshape(rows, ld)
        r.out, r.guard = flat[:M], flat[M:]
    r.split, r.packed, r.kcache, r.vcache = split.value, packed, kc, vc
    if ssq is not None:
        r.ssq, r.ssq_guard = ssq[:M], ssq[M:]
    if xq is not None:
        r.xq, r.xq_guard, r.xd, r.xd_guard, r.xb, r.xb_guard = xq[:M], xq[M:], xd[:M], xd[M:], xb[:M], xb[M:]
    if nxq is not None:
        r.nxq, r.nxq_guard, r.nxd, r.nxd_guard, r.nxb, r.nxb_guard = nxq[:M], nxq[M:], nxd[:M], nxd[M:], nxb[:M], nxb[M:]
    if want_slabs:
        r.slabs = slabs[:max(r.split, 0) * M * N].reshape(-1, M, N)
    return r


def kq_pack_probe(blocks, type: int, N: int, K: int, pack: int = 0, offset: int = 0, device: int = 0):
    """launch_pack_kq alone (mx_kq_side_probe mode 0): blocks uint8 [N * K/256 * block bytes] -> (the packed bytes
    of the N + offset (pack 0) or 2 N (pack 1 / 2: PACK_GATE / PACK_UP) row matrix, 0xFF where nothing was written,
    guard: 64 tiles that must be all-ones bits)."""
    ba = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
    if ba.size < N * (K // 256) * KQ_BLOCK_BYTES.get(type, 0):
        raise ValueError("blocks too short")
    rows = N + offset if pack == 0 else 2 * N
    wb = max(rows, 0) // 16 * (K // 256) * KQ_TILE_BYTES.get(type, 0)
    ob = np.zeros(wb + PROBE_GUARD_ROWS * KQ_TILE_BYTES.get(type, 0) + 16, dtype=np.uint8)
    a = MxKqSideArgs()
    a.mode, a.type, a.N, a.K, a.blocks, a.pack, a.offset, a.out = 0, type, N, K, ba.ctypes.data, pack, offset, ob.ctypes.data
    _check(lib().mx_kq_side_probe(device, ctypes.byref(a)))
    return ob[:wb], ob[wb:-16]


def kq_dequant_probe(blocks, segs, N: int, K: int, device: int = 0):
    """launch_dequant_kq on blocks packed as at load (mode 1): (packed bf16 tiles uint16 [N * K], guard [64 * K])."""
    ba = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
    a = MxKqSideArgs()
    a.kq_n, ty, te = _kq_segments(segs, N)
    need, t0 = 0, 0
    for i in range(a.kq_n):
        a.kq_type[i], a.kq_tile_end[i] = ty[i], te[i]
        need += max(te[i] - t0, 0) * 16 * (K // 256) * KQ_BLOCK_BYTES.get(ty[i], 0)
        t0 = te[i]
    if ba.size < need:
        raise ValueError("blocks too short")
    ob = np.zeros((max(N, 0) + PROBE_GUARD_ROWS) * K, dtype=np.uint16)
    a.mode, a.N, a.K, a.blocks, a.out = 1, N, K, ba.ctypes.data, ob.ctypes.data
    _check(lib().mx_kq_side_probe(device, ctypes.byref(a)))
    return ob[:N * K], ob[N * K:]


def kq_embed_probe(blocks, type: int, N: int, K: int, ids, want_ssq: bool = True, device: int = 0):
    """launch_embed_kq (mode 2): rows `ids` of a K-quant token_embd -> (x f32 [M][K], x guard as uint32, ssq
    [M][K/16] or None, ssq guard or None)."""
    ba = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
    if ba.size < N * (K // 256) * KQ_BLOCK_BYTES.get(type, 0):
        raise ValueError("blocks too short")
    ia = _i32(ids)
    M = len(ia)
    ob = np.zeros((M + PROBE_GUARD_ROWS, K), dtype=np.float32)
    sq = np.zeros((M + PROBE_GUARD_ROWS, K // 16), dtype=np.float32) if want_ssq else None
    a = MxKqSideArgs()
    a.mode, a.type, a.N, a.K, a.blocks, a.ids, a.M, a.out = 2, type, N, K, ba.ctypes.data, ia.ctypes.data, M, ob.ctypes.data
    a.ssq_out = sq.ctypes.data if sq is not None else None
    _check(lib().mx_kq_side_probe(device, ctypes.byref(a)))
    return ob[:M], ob[M:].view(np.uint32), (sq[:M] if sq is not None else None), (sq[M:] if sq is not None else None)


GLUE_GUARD_FLAT = 4096  # elements of 0xFF behind every flat mx_glue_probe output


def glue_flat_probe(mode: int, src, count: int, type: int = 0, device: int = 0):
    """The flat modes of mx_glue_probe: 0 launch_dequant_bf16 (src: the raw blocks of ggml `type`, any dtype; count
    elements), 5 launch_f32_to_bf16, 6 launch_copy_f32 (src f32 [count]) -> (out [count], guard [4096]), uint16 for
    modes 0 / 5 and uint32 (the f32 bits) for mode 6."""
    if mode not in (0, 5, 6):
        raise ValueError("flat modes are 0, 5 and 6")
    sa = np.ascontiguousarray(src).reshape(-1).view(np.uint8) if mode == 0 else \
        np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    if mode != 0 and sa.size < count:
        raise ValueError("src too short")
    ob = np.zeros(max(count, 0) + GLUE_GUARD_FLAT, dtype=np.uint32 if mode == 6 else np.uint16)
    a = MxGlueArgs()
    a.mode, a.type, a.count, a.src_bytes, a.src, a.out = mode, type, max(count, 0), sa.nbytes, sa.ctypes.data, ob.ctypes.data
    _check(lib().mx_glue_probe(device, ctypes.byref(a)))
    return ob[:count], ob[count:]


def glue_rows_probe(mode: int, src, ids=None, want_ssq: bool = True, M: Optional[int] = None, n: Optional[int] = None,
                    device: int = 0):
    """The row modes of mx_glue_probe: 1 launch_embed (src bf16 bits [N][n], ids [M]), 2 launch_ssq (src f32 [M][n]),
    3 launch_f32_in (src f32 [M][n]), 4 launch_bf16_to_f32 (src bf16 bits [M][n]) -> (x [M][n] as uint32 or None
    (mode 2), x guard [64][n], ssq [M][n/16] as uint32, ssq guard [64][n/16]).  The ssq buffer always travels: with
    want_ssq False the launcher gets NULL and it must return all-ones bits.  M / n override the shape of src (refusal
    tests)."""
    if mode not in (1, 2, 3, 4):
        raise ValueError("row modes are 1..4")
    sa = np.ascontiguousarray(src, dtype=np.uint16 if mode in (1, 4) else np.float32)
    rows, ncol = sa.shape
    n = ncol if n is None else n
    a = MxGlueArgs()
    ia = None
    if mode == 1:
        ia = _i32(ids)
        a.N, a.ids = rows, ia.ctypes.data
        M = len(ia) if M is None else M
    M = rows if M is None else M
    xo = np.zeros((max(M, 0) + PROBE_GUARD_ROWS, max(n, 0)), dtype=np.uint32) if mode != 2 else None
    sq = np.zeros((max(M, 0) + PROBE_GUARD_ROWS, max(n, 0) // 16), dtype=np.uint32)
    a.mode, a.M, a.n, a.want_ssq, a.src = mode, M, n, int(want_ssq), sa.ctypes.data
    a.out = xo.ctypes.data if xo is not None else None
    a.ssq_out = sq.ctypes.data
    _check(lib().mx_glue_probe(device, ctypes.byref(a)))
    return (xo[:M] if xo is not None else None), (xo[M:] if xo is not None else None), sq[:M], sq[M:]


class ArgmaxResult:
    """tok, ids_next, pos_next, hist_count int32 [M] with their 4096-element guards (*_guard), hist [M][hist_stride]
    and hist_guard [64][hist_stride]; a buffer whose pointer was withheld (null_mask) returns as it was filled."""


def argmax_probe(logits, V: int, pos, hist_count, hist_stride: int, max_hist: int, null_mask: int = 0,
                 M: Optional[int] = None, ldl: Optional[int] = None, device: int = 0) -> ArgmaxResult:
    """launch_argmax (argmax_stage1 + argmax_stage2) on caller-supplied logits f32 [M][ldl] (mx_glue_probe mode 7).
    null_mask: bit 0 tok_out, 1 ids_next, 2 pos_next, 3 hist passed as NULL."""
    la = np.ascontiguousarray(logits, dtype=np.float32)
    rows, ld = la.shape
    M = rows if M is None else M
    ldl = ld if ldl is None else ldl
    pa, ha = _i32(pos), _i32(hist_count)
    if len(pa) < M or len(ha) < M:
        raise ValueError("pos [M] and hist_count [M] expected")
    flat = [np.zeros(max(M, 0) + GLUE_GUARD_FLAT, dtype=np.int32) for _ in range(4)]
    hist = np.zeros((max(M, 0) + PROBE_GUARD_ROWS, max(hist_stride, 1)), dtype=np.int32)
    a = MxGlueArgs()
    a.mode, a.M, a.V, a.ldl, a.hist_stride, a.max_hist, a.null_mask = 7, M, V, ldl, hist_stride, max_hist, null_mask
    a.src, a.pos, a.hist_count = la.ctypes.data, pa.ctypes.data, ha.ctypes.data
    a.tok_out, a.ids_next_out, a.pos_next_out, a.hist_count_out = (f.ctypes.data for f in flat)
    a.hist_out = hist.ctypes.data
    _check(lib().mx_glue_probe(device, ctypes.byref(a)))
    r = ArgmaxResult()
    for name, f in zip(("tok", "ids_next", "pos_next", "hist_count"), flat):
        setattr(r, name, f[:M])
        setattr(r, name + "_guard", f[M:])
    r.hist, r.hist_guard = hist[:M], hist[M:]
    return r


class Q8kResult:
    """xq int8 [M][n], xd [M][n/256], xb [M][n/32] and their 64-row guards; x [rows][ld] (the device's x after the
    launch: folded where slabs were given) and x_guard."""
    xq = xd = xb = xq_guard = xd_guard = xb_guard = x = x_guard = None


def q8k_probe(x, n: Optional[int] = None, w=None, row_map=None, eps: float = 0.0, slabs=None, M: Optional[int] = None,
              device: int = 0) -> Q8kResult:
    """launch_quantize_q8k (w None: x f32 [M][ld], ld >= n) / launch_rmsnorm_q8k (w [n]; row_map [M]; slabs
    [nslab][rows][n] folded into x first) on caller-supplied rows (mx_kq_side_probe modes 3 / 4)."""
    xa = np.ascontiguousarray(x, dtype=np.float32)
    if xa.ndim != 2:
        raise ValueError("x [rows][ld] expected")
    rows, ld = xa.shape
    if n is None:
        n = ld
    a = MxKqSideArgs()
    keep = [xa]
    a.mode, a.K, a.x, a.ld, a.eps = (3 if w is None else 4), n, xa.ctypes.data, ld, eps
    if row_map is not None:
        ma = _i32(row_map)
        a.row_map = ma.ctypes.data
        keep.append(ma)
        if M is None:
            M = len(ma)
    if M is None:
        M = rows
    a.M, a.rows = M, rows
    if w is not None:
        wa = np.ascontiguousarray(w, dtype=np.float32)
        if wa.size != n:
            raise ValueError("w [n] expected")
        a.w = wa.ctypes.data
        keep.append(wa)
    if slabs is not None:
        sa = np.ascontiguousarray(slabs, dtype=np.float32)
        if sa.ndim != 3 or sa.shape[1:] != (rows, n):
            raise ValueError("slabs [nslab][rows][n] expected")
        a.nslab = sa.shape[0]
        if a.nslab:
            a.slabs = sa.ctypes.data
        keep.append(sa)
    Mr, g = max(M, 0), PROBE_GUARD_ROWS
    xq = np.zeros((Mr + g, max(n, 1)), dtype=np.int8)
    xd = np.zeros((Mr + g, max(n // 256, 1)), dtype=np.float32)
    xb = np.zeros((Mr + g, max(n // 32, 1)), dtype=np.float32)
    xo = np.zeros((rows + g, ld), dtype=np.float32)
    a.xq_out, a.xd_out, a.xb_out, a.x_out = xq.ctypes.data, xd.ctypes.data, xb.ctypes.data, xo.ctypes.data
    _check(lib().mx_kq_side_probe(device, ctypes.byref(a)))
    del keep
    r = Q8kResult()
    r.xq, r.xq_guard, r.xd, r.xd_guard, r.xb, r.xb_guard = xq[:M], xq[M:], xd[:M], xd[M:], xb[:M], xb[M:]
    r.x, r.x_guard = xo[:rows], xo[rows:]
    return r


def pool_probe(x, w, seq_begin, pooling: int, normalize: bool = False, chunk_rows: int = 0, eps: float = 1e-5,
               out=None, device: int = 0):
    """The embedding tail on caller-supplied rows (no engine; include/mx_engine.h mx_pool_probe): x f32
    [rows][n], w f32 [n], sequence q = rows [seq_begin[q], seq_begin[q + 1]), x taken in chunks of chunk_rows
    rows (0: one chunk).  Returns (vectors [rows][n] for POOL_NONE else [n_seq][n], guard [64][n] as uint32: must
    be all-ones bits).  out (optional): a caller-owned buffer for the result (tests of refusals)."""
    xa = np.ascontiguousarray(x, dtype=np.float32)
    if xa.ndim != 2:
        raise ValueError("x [rows][n] expected")
    rows, n = xa.shape
    wa = np.ascontiguousarray(w, dtype=np.float32)
    if wa.size != n:
        raise ValueError("w [n] expected")
    sb = _i32(seq_begin)
    n_seq = len(sb) - 1
    n_out = max(rows if pooling == POOL_NONE else n_seq, 0)
    if out is None:
        ob = np.zeros((n_out + PROBE_GUARD_ROWS, n), dtype=np.float32)
    else:
        ob = out
        if not ob.flags.c_contiguous or ob.dtype != np.float32 or ob.size < (n_out + PROBE_GUARD_ROWS) * n:
            raise ValueError("out too small")
    _check(lib().mx_pool_probe(device, rows, n, xa.ctypes.data, wa.ctypes.data, eps, n_seq, sb.ctypes.data,
                               int(chunk_rows), int(pooling), int(bool(normalize)), ob.ctypes.data))
    flat = ob.reshape(-1)[:(n_out + PROBE_GUARD_ROWS) * n].reshape(-1, n)
    return flat[:n_out], flat[n_out:].view(np.uint32)


def _check(rc: int):
    if rc != MX_OK:
        raise MxError(rc, lib().mx_last_error().decode(errors="replace"))


# ---- grammar-constrained sampling (include/mx_engine.h mx_vocab_create ...) -- no GPU touched
GRAMMAR_OK, GRAMMAR_DEAD_END, GRAMMAR_CAP = 0, 1, 2  # mx_engine.h MX_GRAMMAR_*: what GrammarState.mask() reports


class GrammarVocab:
    """What grammars are matched against: the piece bytes of every token (an empty piece is never allowed) and the
    end-of-generation ids (allowed exactly where a grammar may end)."""

    def __init__(self, pieces: Sequence[bytes], eog_ids: Sequence[int]):
        self.n_vocab = len(pieces)
        off = np.zeros(self.n_vocab + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
        blob = np.frombuffer(b"".join(pieces) or b"\0", dtype=np.uint8)
        eog = _i32(list(eog_ids))
        h = ctypes.c_void_p()
        _check(lib().mx_vocab_create(self.n_vocab, blob.ctypes.data, off.ctypes.data, eog.ctypes.data if len(eog) else None,
                                     len(eog), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().mx_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CompiledGrammar:
    """A GBNF grammar compiled over one vocabulary: immutable, shared by any number of requests and states, and
    reference-counted in the library -- closing it, or its vocabulary, while a request still uses it is safe.
    What GBNF refuses (syntax, undefined rules, no root, {m,n} with n < m, left recursion) raises ValueError with
    the rule or position.  cache_entries: masks kept (None: the library's default; 0: no cache)."""

    def __init__(self, vocab: GrammarVocab, gbnf: str, cache_entries: Optional[int] = None):
        h = ctypes.c_void_p()
        rc = lib().mx_grammar_create(vocab._h, gbnf.encode("utf-8"), -1 if cache_entries is None else int(cache_entries),
                                     ctypes.byref(h))
        if rc == MX_ERR_ARG:
            raise ValueError(lib().mx_last_error().decode(errors="replace"))
        _check(rc)
        self._h = h
        self.n_vocab = vocab.n_vocab

    def state(self) -> "GrammarState":
        return GrammarState(self)

    def cache_stats(self) -> dict:
        """hits / misses (mask lookups served from the cache / computed by a walk of the vocabulary), entries."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mx_grammar_cache_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"hits": a.value, "misses": b.value, "entries": c.value}

    def close(self):
        if getattr(self, "_h", None):
            lib().mx_grammar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GrammarState:
    """A place in a grammar, as a request holds one (for probing on the CPU): starts at root."""

    def __init__(self, grammar: CompiledGrammar):
        h = ctypes.c_void_p()
        _check(lib().mx_grammar_state_create(grammar._h, ctypes.byref(h)))
        self._h = h
        self.n_vocab = grammar.n_vocab

    def mask(self):
        """(words uint32 [ceil(V / 32)], status): bit t & 31 of word t >> 5 set = token t is allowed; status
        GRAMMAR_OK, GRAMMAR_DEAD_END or GRAMMAR_CAP (the words all zero for the last two)."""
        w = np.zeros((self.n_vocab + 31) // 32, dtype=np.uint32)
        st = ctypes.c_int32()
        _check(lib().mx_grammar_state_mask(self._h, w.ctypes.data, len(w), ctypes.byref(st)))
        return w, st.value

    def allowed(self) -> np.ndarray:
        """The mask as booleans [V]."""
        w, _ = self.mask()
        return np.unpackbits(w.view(np.uint8), bitorder="little")[: self.n_vocab].astype(bool)

    def accept(self, token: int):
        """Moves on by one token; MxError(MX_ERR_ARG) when it is not allowed (the state is unchanged)."""
        _check(lib().mx_grammar_state_accept(self._h, int(token)))

    def may_end(self) -> bool:
        e = ctypes.c_int32()
        _check(lib().mx_grammar_state_may_end(self._h, ctypes.byref(e)))
        return bool(e.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().mx_grammar_state_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grammar_mask_probe(logits, masks, on, V: Optional[int] = None, device: int = 0) -> np.ndarray:
    """The grammar mask kernel on caller-supplied f32 rows (no engine; include/mx_engine.h mx_grammar_mask_probe):
    logits [n][ldl] with V <= ldl valid columns (default all), n <= 64; masks uint32 [n][ceil(V / 32)]; on [n].
    Returns the rows as the kernel left them, [n][ldl]."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    n, ldl = lg.shape
    V = ldl if V is None else V
    mk = np.ascontiguousarray(masks, dtype=np.uint32)
    ov = np.ascontiguousarray(on, dtype=np.uint32)
    if mk.shape != (n, (V + 31) // 32) or ov.shape != (n,):
        raise ValueError("masks [n][ceil(V / 32)] and on [n] expected")
    out = np.empty_like(lg)
    _check(lib().mx_grammar_mask_probe(device, lg.ctypes.data, n, V, ldl, mk.ctypes.data, ov.ctypes.data,
                                       out.ctypes.data))
    return out


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def grammar_mask_time(masks, V: int, ldl: Optional[int] = None, iters: int = 200, device: int = 0) -> float:
    """Microseconds per launch of the grammar mask kernel over masks uint32 [n][ceil(V / 32)], every row on, on
    resident buffers between two HIP events (include/mx_engine.h mx_grammar_mask_time)."""
    mk = np.ascontiguousarray(masks, dtype=np.uint32)
    if mk.ndim != 2 or mk.shape[1] != (V + 31) // 32:
        raise ValueError("masks [n][ceil(V / 32)] expected")
    us = ctypes.c_double()
    _check(lib().mx_grammar_mask_time(device, mk.shape[0], V, V if ldl is None else ldl, mk.ctypes.data, int(iters),
                                      ctypes.byref(us)))
    return us.value


class Engine:
    """One engine instance = one GPU, one model (or one pipeline stage of it)."""

    supports_logprobs = True  # submit(logprobs=) / logprobs(): what Llama.create_completion(logprobs=) needs
    supports_draft = True  # submit(draft=) / spec_stats(): what Llama(draft_model=LlamaPromptLookupDecoding()) needs
    supports_embeddings = True  # embed(): what Llama(embedding=True).embed / create_embedding need
    supports_prefix_sharing = True  # set_prefix_sharing() / sharing_stats(): what Llama.set_cache needs
    supports_sampler_ext = True  # submit(typical_p=, tfs_z=, mirostat_*=, logit_bias=): the whole sampler chain
    supports_host_cache = True  # set_host_cache() / host_cache_stats(): the host-RAM tier of Llama.set_cache
    supports_grammar = True  # submit(grammar=): what Llama.create_completion(grammar=) needs

    def __init__(self, model_path: str, n_ctx: int = 512, n_seq_max: int = 64, layer_begin: int = 0,
                 layer_end: int = -1, device: int = -1, use_graphs: bool = True, seed: int = 0,
                 handoff_bf16: bool = False, prefix_sharing: bool = False, host_cache_bytes: int = 0,
                 lora_path: Optional[str] = None, lora_scale: float = 1.0):
        """lora_path: a GGUF LoRA adapter merged into the weights while the model loads, scaled by
        lora_scale * alpha / r; a quantised base is then dequantised to bf16 (info.weight_type 30)."""
        L = lib()
        opts = MxOpts()
        L.mx_opts_default(ctypes.byref(opts))
        opts.n_ctx, opts.n_seq_max = n_ctx, n_seq_max
        opts.layer_begin, opts.layer_end, opts.device = layer_begin, layer_end, device
        opts.use_graphs, opts.seed = int(use_graphs), seed
        opts.handoff_bf16 = int(handoff_bf16)
        self.handoff_bf16 = bool(handoff_bf16)
        h = ctypes.c_void_p()
        if lora_path is None:
            _check(L.mx_engine_create(model_path.encode(), ctypes.byref(opts), ctypes.byref(h)))
        else:
            _check(L.mx_engine_create_lora(model_path.encode(), ctypes.byref(opts), os.fsencode(lora_path),
                                           float(lora_scale), ctypes.byref(h)))
        self._h = h
        info = MxModelInfo()
        _check(L.mx_engine_info(self._h, ctypes.byref(info)))
        self.info = info
        self.n_vocab = info.n_vocab
        self.n_embd = info.n_embd
        self.n_ctx = info.n_ctx
        if prefix_sharing:
            self.set_prefix_sharing(True)
        if host_cache_bytes:
            self.set_host_cache(host_cache_bytes)

    def lora_info(self) -> dict:
        """n_tensors (matrices of this engine's layers the adapter was merged into), rank_max, alpha, lora_scale
        (include/mx_engine.h mx_lora_info); all 0 for an engine created without an adapter."""
        st = MxLoraInfo()
        _check(lib().mx_engine_lora_info(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in MxLoraInfo._fields_}

    def set_host_cache(self, capacity_bytes: int):
        """The host-RAM tier behind the KV slots (off by default): slot records about to be
        overwritten are kept in pinned host memory up to `capacity_bytes`, least recently used first out, and a
        prompt that matches one gets its K/V back by a transfer instead of a prefill.  Lowering the capacity
        evicts at once; 0 drops everything and switches the tier off.  A pipeline-stage engine raises
        MxError(MX_ERR_STATE)."""
        if capacity_bytes < 0:
            raise ValueError("capacity_bytes must be >= 0")
        _check(lib().mx_engine_set_host_cache(self._h, int(capacity_bytes)))

    def host_cache_stats(self) -> dict:
        """entries, bytes, capacity_bytes, spills, spilled_bytes, restores, restored_prompt_tokens, restored_bytes,
        evictions, skipped (include/mx_engine.h mx_host_cache_counts)."""
        st = MxHostCacheCounts()
        _check(lib().mx_host_cache_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in MxHostCacheCounts._fields_}

    def set_prefix_sharing(self, on: bool):
        """Share prompt prefixes across KV slots by device copies (off by default): from the next
        admission on.  A pipeline-stage engine raises MxError(MX_ERR_STATE)."""
        _check(lib().mx_engine_set_prefix_sharing(self._h, int(bool(on))))

    def sharing_stats(self) -> dict:
        """shared_prompt_tokens (prompt positions received by a copy), copies, copied_bytes, follower_requests."""
        st = MxSharingStats()
        _check(lib().mx_prefix_sharing_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in MxSharingStats._fields_}

    # -- parity hooks --------------------------------------------------------
    def forward_logits(self, ids: Sequence[int], pos0: int = 0, slot: int = 0) -> np.ndarray:
        ids = _i32(ids)
        out = np.empty((len(ids), self.n_vocab), dtype=np.float32)
        _check(lib().mx_forward_logits(self._h, slot, ids.ctypes.data, len(ids), pos0, out.ctypes.data))
        return out

    def forward_rows(self, slots, pos, ids, want_logits: bool = True) -> Optional[np.ndarray]:
        """Rows forward (chunked by 64); want_logits=False skips lm_head (prefill)."""
        slots, pos, ids = _i32(slots), _i32(pos), _i32(ids)
        out = np.empty((len(ids), self.n_vocab), dtype=np.float32) if want_logits else None
        _check(lib().mx_forward_rows(self._h, len(ids), slots.ctypes.data, pos.ctypes.data, ids.ctypes.data,
                                     out.ctypes.data if out is not None else None))
        return out

    def forward_topk(self, slots, pos, ids, k: int):
        """Rows forward (<= 64) + the device top-k kernel: (values [n][k], ids [n][k])."""
        slots, pos, ids = _i32(slots), _i32(pos), _i32(ids)
        vals = np.empty((len(ids), k), dtype=np.float32)
        idx = np.empty((len(ids), k), dtype=np.int32)
        _check(lib().mx_forward_topk(self._h, len(ids), slots.ctypes.data, pos.ctypes.data, ids.ctypes.data, k,
                                     vals.ctypes.data, idx.ctypes.data))
        return vals, idx

    def forward_logprobs(self, slots, pos, ids, targets, k: int, want_logits: bool = False):
        """Rows forward (<= 64) + the log-prob kernels: (log-prob of targets[i] in row i [n], top log-probs
        [n][k'], their ids [n][k']) with k' = min(k, n_vocab); want_logits adds the f32 rows the statistics
        were computed from."""
        slots, pos, ids, targets = _i32(slots), _i32(pos), _i32(ids), _i32(targets)
        n, ke = len(ids), max(0, min(k, self.n_vocab))
        tgt = np.empty(n, dtype=np.float32)
        top = np.empty((n, ke), dtype=np.float32)
        idx = np.empty((n, ke), dtype=np.int32)
        lg = np.empty((n, self.n_vocab), dtype=np.float32) if want_logits else None
        _check(lib().mx_forward_logprobs(self._h, n, slots.ctypes.data, pos.ctypes.data, ids.ctypes.data,
                                         targets.ctypes.data, k, tgt.ctypes.data, top.ctypes.data if ke else None,
                                         idx.ctypes.data if ke else None, lg.ctypes.data if lg is not None else None))
        return (tgt, top, idx, lg) if want_logits else (tgt, top, idx)

    def stage_rows(self, slots, pos, ids, x_in: int = 0, x_out: int = 0, want_logits: bool = False,
                   stream: int = 0) -> Optional[np.ndarray]:
        slots, pos = _i32(slots), _i32(pos)
        ids_p = _i32(ids).ctypes.data if ids is not None else None
        ids_keep = _i32(ids) if ids is not None else None
        if ids_keep is not None:
            ids_p = ids_keep.ctypes.data
        out = np.empty((len(slots), self.n_vocab), dtype=np.float32) if want_logits else None
        _check(lib().mx_stage_rows(self._h, len(slots), slots.ctypes.data, pos.ctypes.data, ids_p,
                                   x_in or None, x_out or None, out.ctypes.data if out is not None else None,
                                   stream or None))
        return out

    def stage_rows_pick(self, slots, pos, ids, x_in: int = 0, x_out: int = 0, rowmap=(), samplers=None,
                        stream: int = 0):
        """Pipelined prefill of any number of rows; on the last stage the rows in `rowmap` pick a token
        each (samplers: row_samplers() array or None for greedy).  Returns the tokens (list)."""
        slots, pos = _i32(slots), _i32(pos)
        ids_a = _i32(ids) if ids is not None else None
        rm = _i32(rowmap)
        tok = np.zeros(max(1, len(rm)), dtype=np.int32)
        _check(lib().mx_stage_rows_pick(self._h, len(slots), slots.ctypes.data, pos.ctypes.data,
                                        ids_a.ctypes.data if ids_a is not None else None, x_in or None, x_out or None,
                                        len(rm), rm.ctypes.data if len(rm) else None, samplers,
                                        tok.ctypes.data if len(rm) else None, stream or None))
        return tok[:len(rm)].tolist()

    # -- request API ---------------------------------------------------------
    def submit(self, ids: Sequence[int], max_tokens: int, temperature: float = 0.0, top_k: int = 40,
               top_p: float = 0.95, min_p: float = 0.05, repeat_penalty: float = 1.0, repeat_last_n: int = 64,
               seed: Optional[int] = None, ignore_eos: bool = False, frequency_penalty: float = 0.0,
               presence_penalty: float = 0.0, logprobs: Optional[int] = None, prompt_logprobs: bool = False,
               draft: Optional[Sequence[int]] = None, typical_p: float = 1.0, tfs_z: float = 1.0,
               mirostat_mode: int = 0, mirostat_tau: float = 5.0, mirostat_eta: float = 0.1, logit_bias=None,
               grammar: Optional["CompiledGrammar"] = None) -> int:
        """grammar: a CompiledGrammar over a vocabulary of the model's size -- every token is picked
        among those the grammar allows after the tokens generated so far, whatever the sampler settings; such a
        request never speculates (draft is ignored for it) and its rounds run one step.
        typical_p / tfs_z / mirostat_mode=2 (mirostat_tau, mirostat_eta) / logit_bias={id: bias}: the rest of
        llama-cpp-python's sampler chain, on the device (mx_submit_ext); such a request never
        speculates.
        draft=(num_pred_tokens 1..15, max_ngram_size >= 1): prompt-lookup speculative decoding on the device --
        the same tokens, several per weight pass where the context repeats itself; only greedy requests without
        penalties or logprobs on a bf16 model ever speculate (spec_stats() tells), the others decode as always.
        logprobs=k (0..64): the request also records each generated token's log-probability and the k
        most likely tokens (read with logprobs()); prompt_logprobs adds the prompt positions >= 1."""
        ids = _i32(ids)
        s = MxSampling()
        lib().mx_sampling_default(ctypes.byref(s))
        s.temperature, s.top_k, s.top_p, s.min_p = temperature, top_k, top_p, min_p
        s.repeat_penalty, s.repeat_last_n, s.ignore_eos = repeat_penalty, repeat_last_n, int(ignore_eos)
        s.frequency_penalty, s.presence_penalty = frequency_penalty, presence_penalty
        if seed is not None and seed >= 0:
            s.seed = seed
        req = ctypes.c_uint64()
        if grammar is not None:
            if not isinstance(grammar, CompiledGrammar):
                raise TypeError("grammar must be a CompiledGrammar")
            if prompt_logprobs and logprobs is None:
                raise ValueError("prompt_logprobs needs logprobs=k")
            x, keep = sampling_ext(s, typical_p, tfs_z, mirostat_mode, mirostat_tau, mirostat_eta, logit_bias)
            _check(lib().mx_submit_grammar(self._h, ids.ctypes.data, len(ids), ctypes.byref(x), max_tokens,
                                           -1 if logprobs is None else int(logprobs), int(bool(prompt_logprobs)),
                                           grammar._h, ctypes.byref(req)))
        elif typical_p != 1.0 or tfs_z != 1.0 or mirostat_mode != 0 or logit_bias:
            if prompt_logprobs and logprobs is None:
                raise ValueError("prompt_logprobs needs logprobs=k")
            x, keep = sampling_ext(s, typical_p, tfs_z, mirostat_mode, mirostat_tau, mirostat_eta, logit_bias)
            _check(lib().mx_submit_ext(self._h, ids.ctypes.data, len(ids), ctypes.byref(x), max_tokens,
                                       -1 if logprobs is None else int(logprobs), int(bool(prompt_logprobs)),
                                       ctypes.byref(req)))
        elif draft is not None and logprobs is None:
            if prompt_logprobs:
                raise ValueError("prompt_logprobs needs logprobs=k")
            d, ng = draft
            _check(lib().mx_submit_spec(self._h, ids.ctypes.data, len(ids), ctypes.byref(s), max_tokens, int(d), int(ng),
                                        ctypes.byref(req)))
        elif logprobs is None:
            if prompt_logprobs:
                raise ValueError("prompt_logprobs needs logprobs=k")
            _check(lib().mx_submit(self._h, ids.ctypes.data, len(ids), ctypes.byref(s), max_tokens, ctypes.byref(req)))
        else:
            _check(lib().mx_submit_lp(self._h, ids.ctypes.data, len(ids), ctypes.byref(s), max_tokens, int(logprobs),
                                      int(bool(prompt_logprobs)), ctypes.byref(req)))
        return req.value

    def logprobs(self, req: int):
        """Entries a logprobs= request holds so far (prompt positions first when asked for, then one per
        generated token; never blocks, valid until wait()): (tok_lp [n], top_lp [n][k], top_idx [n][k])."""
        n, k = ctypes.c_int32(), ctypes.c_int32()
        L = lib()
        _check(L.mx_request_logprobs(self._h, req, None, None, None, 0, ctypes.byref(n), ctypes.byref(k)))
        cap, kk = n.value, k.value
        tok = np.empty(cap, dtype=np.float32)
        top = np.empty((cap, kk), dtype=np.float32)
        idx = np.empty((cap, kk), dtype=np.int32)
        if cap:
            _check(L.mx_request_logprobs(self._h, req, tok.ctypes.data, top.ctypes.data if kk else None,
                                         idx.ctypes.data if kk else None, cap, ctypes.byref(n), ctypes.byref(k)))
        return tok, top, idx

    @staticmethod
    def grammar_cache_stats(grammar: "CompiledGrammar") -> dict:
        """hits / misses / entries of a compiled grammar's mask cache (mx_grammar_cache_stats)."""
        return grammar.cache_stats()

    grammar_mask_probe = staticmethod(grammar_mask_probe)

    def sampler_stats(self) -> dict:
        """device_steps / host_steps (decode steps picked on the device / by the host sampler), wide_rows (row-steps
        of the wide kernel: more than 64 candidates) and rounds (the scheduler rounds behind the
        steps) -- include/mx_engine.h mx_sampler_counts."""
        c = MxSamplerCounts()
        _check(lib().mx_sampler_stats(self._h, ctypes.byref(c)))
        return {k: getattr(c, k) for k, _ in MxSamplerCounts._fields_}

    def spec_stats(self, req: Optional[int] = None) -> dict:
        """Speculation counters of a request not yet released by wait(), or (None) the engine's totals: steps
        (speculating forwards whose tokens were kept), drafted and accepted draft tokens."""
        c = MxSpecCounts()
        _check(lib().mx_spec_stats(self._h, int(req or 0), ctypes.byref(c)))
        return {"steps": c.steps, "drafted": c.drafted, "accepted": c.accepted}

    def submit_many(self, prompts, max_tokens: int, seeds=None, per_request=None, **kw):
        """Several requests queued atomically (one scheduler round admits them all); same sampling
        keywords as submit() (or ``per_request``: one keyword dict per prompt), one seed per prompt,
        max_tokens one value or one per prompt.  Returns the request ids."""
        n = len(prompts)
        if "grammar" in kw or any("grammar" in d for d in (per_request or [])):
            raise ValueError("submit_many takes no grammar: a grammar request is queued with submit()")
        arrs = [_i32(p) for p in prompts]
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = _i32([len(a) for a in arrs])
        mts = _i32(list(max_tokens) if hasattr(max_tokens, "__len__") else [max_tokens] * n)
        samp = (MxSampling * n)()
        base = kw
        kws = [dict(base, **per_request[i]) if per_request is not None else base for i in range(n)]
        if any(k in kwi for kwi in kws for k in _EXT_KEYS):
            # some request has a setting of the extended chain: one mx_sampling_ext each, queued atomically too
            xs = (MxSamplingExt * n)()
            keep = []
            for i in range(n):
                kwi = dict(kws[i])
                ext = {k: kwi.pop(k) for k in _EXT_KEYS if k in kwi}
                sd = kwi.pop("seed", seeds[i] if seeds is not None else None)
                keep.append(sampling_ext(sampling(seed=sd, **kwi), into=xs[i], **ext)[1])
            reqs = (ctypes.c_uint64 * n)()
            _check(lib().mx_submit_ext_batch(self._h, n, ptrs, lens.ctypes.data, xs, mts.ctypes.data, reqs))
            return list(reqs)
        for i in range(n):
            kw = dict(base, **per_request[i]) if per_request is not None else base
            if per_request is not None and "seed" in kw:
                seeds = list(seeds) if seeds is not None else [None] * n
                seeds[i] = kw["seed"]
            lib().mx_sampling_default(ctypes.byref(samp[i]))
            s = samp[i]
            s.temperature, s.top_k = kw.get("temperature", 0.0), kw.get("top_k", 40)
            s.top_p, s.min_p = kw.get("top_p", 0.95), kw.get("min_p", 0.05)
            s.repeat_penalty, s.repeat_last_n = kw.get("repeat_penalty", 1.0), kw.get("repeat_last_n", 64)
            s.ignore_eos = int(kw.get("ignore_eos", False))
            s.frequency_penalty, s.presence_penalty = kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0)
            if seeds is not None and seeds[i] is not None and seeds[i] >= 0:
                s.seed = seeds[i]
        reqs = (ctypes.c_uint64 * n)()
        _check(lib().mx_submit_batch(self._h, n, ptrs, lens.ctypes.data, samp, mts.ctypes.data, reqs))
        return list(reqs)

    def wait(self, req: int, cap: Optional[int] = None):
        """Block until the request finishes; (generated ids, finish reason).  The buffer holds the
        whole context by default; a request that generated more is kept and re-read larger."""
        cap = cap or self.n_ctx
        n, fin = ctypes.c_int32(), ctypes.c_int32()
        while True:
            out = np.empty(cap, dtype=np.int32)
            rc = lib().mx_wait(self._h, req, out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(fin))
            if rc == MX_ERR_ARG and n.value > cap:
                cap = n.value
                continue
            _check(rc)
            return out[: min(n.value, cap)].tolist(), fin.value

    def poll(self, req: int, n_have: int = 0):
        """Block until the request holds more than n_have ids or finishes: (ids so far, done)."""
        cap = self.n_ctx
        out = np.empty(cap, dtype=np.int32)
        n, done = ctypes.c_int32(), ctypes.c_int32()
        _check(lib().mx_poll(self._h, req, n_have, out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(done)))
        return out[: min(n.value, cap)].tolist(), bool(done.value)

    def cancel(self, req: int):
        """End the request after its current step (finish reason STOP); release it with wait()."""
        _check(lib().mx_cancel(self._h, req))

    def generate(self, ids, max_tokens: int, **kw):
        return self.wait(self.submit(ids, max_tokens, **kw))

    def embed(self, prompts, pooling: int = POOL_NONE, normalize: bool = False):
        """Embeddings of token sequences, computed on the device (final norm, pooling, L2 normalisation): one
        mx_submit_embed call -- a batched prefill without lm_head -- then one np.float32 array per prompt,
        [len(prompt)][n_embd] for POOL_NONE, [1][n_embd] for POOL_MEAN / POOL_CLS / POOL_LAST."""
        n = len(prompts)
        arrs = [_i32(p) for p in prompts]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = _i32([len(a) for a in arrs])
        reqs = (ctypes.c_uint64 * max(n, 1))()
        _check(lib().mx_submit_embed(self._h, n, ptrs, lens.ctypes.data, int(pooling), int(bool(normalize)), reqs))
        outs, err = [], None
        for i in range(n):  # every request is released, also after a failure
            rows = len(arrs[i]) if pooling == POOL_NONE else 1
            out = np.empty((rows, self.n_embd), dtype=np.float32)
            got = ctypes.c_int32()
            rc = lib().mx_wait_embed(self._h, reqs[i], out.ctypes.data, out.size, ctypes.byref(got))
            if rc != MX_OK and err is None:
                err = MxError(rc, lib().mx_last_error().decode(errors="replace"))
            outs.append(out[:got.value])
        if err is not None:
            raise err
        return outs

    # -- device-resident batches (bench, pipeline) ---------------------------
    def batch(self, slots, pos, ids=None, max_steps: int = 0) -> "Batch":
        return Batch(self, slots, pos, ids, max_steps)

    def profile_kernel(self, kind: int, M: int, iters: int = 3):
        us, nb = ctypes.c_double(), ctypes.c_double()
        _check(lib().mx_profile_kernel(self._h, kind, M, iters, ctypes.byref(us), ctypes.byref(nb)))
        return us.value, nb.value

    def stats(self) -> dict:
        st = MxStats()
        _check(lib().mx_engine_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in MxStats._fields_}

    def sync(self):
        _check(lib().mx_sync(self._h))

    # -- diagnosis (include/mx_engine.h mx_debug) -------------------------------
    DEBUG_BUFFERS = {"x": 0, "q": 1, "xn": 2, "attn_out": 3, "act": 4, "slabs": 5, "kcache": 6, "vcache": 7,
                     "ssq": 8, "pos": 9, "slot": 10, "rope_cs": 11}

    def debug_stop(self, n: int):
        """End every 17..64-row forward after n launches (-1: never)."""
        _check(lib().mx_debug(self._h, 0, n, None, 0))

    def debug_sync(self, on: bool):
        """Synchronise the stream after every launch of a 17..64-row forward."""
        _check(lib().mx_debug(self._h, 1, int(on), None, 0))

    def debug_read(self, name: str, nbytes: int) -> np.ndarray:
        """The first nbytes of an internal buffer (after a device synchronize), as uint8."""
        out = np.zeros(nbytes, dtype=np.uint8)  # past the buffer's end: zeros
        _check(lib().mx_debug(self._h, 2, self.DEBUG_BUFFERS[name], out.ctypes.data, nbytes))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().mx_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def torch_stream_handle() -> int:
    """hipStream_t of torch's current stream.  The engine's C ABI reads a NULL stream as
    "the engine's own stream", so the legacy default stream (handle 0) is refused: work
    enqueued there would not be ordered with the engine's kernels."""
    import torch

    h = torch.cuda.current_stream().cuda_stream
    if not h:
        raise RuntimeError("run engine tensor calls inside `with torch.cuda.stream(s):` (a non-default stream)")
    return h


class Batch:
    def __init__(self, eng: Engine, slots, pos, ids, max_steps: int):
        self.eng = eng
        slots, pos = _i32(slots), _i32(pos)
        self.M = len(slots)
        ids_a = _i32(ids) if ids is not None else None
        h = ctypes.c_void_p()
        _check(lib().mx_batch_create(eng._h, self.M, slots.ctypes.data, pos.ctypes.data,
                                     ids_a.ctypes.data if ids_a is not None else None, max_steps, ctypes.byref(h)))
        self._h = h
        self.max_steps = max_steps

    @property
    def ids_device_ptr(self) -> int:
        return lib().mx_batch_ids_device(self._h)

    def step(self, x_in: int = 0, x_out: int = 0, stream: int = 0):
        _check(lib().mx_batch_step(self.eng._h, self._h, x_in or None, x_out or None, stream or None))

    def reset(self, pos, ids=None, samplers=None, stream: int = 0):
        """Re-arm for the next run (graphs kept): positions, optional next ids, per-row samplers
        (row_samplers() array; None = greedy argmax); the token history restarts."""
        pos = _i32(pos)
        ids_a = _i32(ids) if ids is not None else None
        _check(lib().mx_batch_reset(self.eng._h, self._h, pos.ctypes.data,
                                    ids_a.ctypes.data if ids_a is not None else None, samplers, stream or None))

    def bind_ids(self, ids_device_ptr: int):
        _check(lib().mx_batch_bind_ids(self.eng._h, self._h, ids_device_ptr))

    # tensor-level interface used by the pipeline driver (torch device tensors)
    def step_tensors(self, x_in=None, x_out=None):
        stream = torch_stream_handle()
        self.step(x_in.data_ptr() if x_in is not None else 0, x_out.data_ptr() if x_out is not None else 0,
                  stream)

    def bind_ids_tensor(self, t):
        self._ids_tensor = t  # keep alive
        self.bind_ids(t.data_ptr())

    def tokens(self) -> np.ndarray:
        out = np.zeros((self.M, max(1, self.max_steps)), dtype=np.int32)
        n = ctypes.c_int32()
        _check(lib().mx_batch_tokens(self.eng._h, self._h, out.ctypes.data, out.shape[1], ctypes.byref(n)))
        return out[:, : min(n.value, self.max_steps)]

    def close(self):
        if getattr(self, "_h", None) and self.eng._h:
            lib().mx_batch_destroy(self.eng._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
