"""``Llama`` -- drop-in for ``llama_cpp.Llama`` as the reference node uses it.

    self.model = Llama(model_path=model_path)                          p2p:19
    result = self.model(prompt, max_tokens=100)["choices"][0]["text"]  p2p:125

(p2p = /root/reference/llama_p2p_network.py.)  Constructor keywords,
``__call__``/``create_completion`` keywords and defaults, the returned
completion dict, ``tokenize``/``detokenize`` and the ``ValueError`` raised for
a prompt that does not fit ``n_ctx`` follow llama-cpp-python (~0.3.1, the
version current at the reference's date).  The
compute runs in the MI355X engine (engine.py -> libmxllama.so); calls release
the GIL, and concurrent calls from several threads are micro-batched by the
engine's scheduler instead of being serialised.

Embeddings (``Llama(embedding=True)``, ``embed``, ``create_embedding``, ``pooling_type``) follow the same
version.  llama_cpp is not installed here, so the contract is pinned as read from its source (llama.py
``Llama.embed`` / ``create_embedding`` / ``_normalize_embedding``): a str gives one item and a list a list; an
item is a list of floats with pooling and a list of per-token lists with LLAMA_POOLING_TYPE_NONE; inputs are
tokenised with BOS and cut to n_batch tokens (``truncate``) or refused with its ``ValueError``; the
``RuntimeError`` without ``embedding=True``; ``(result, total_tokens)`` with ``return_count``; the OpenAI-style
dict of ``create_embedding``.  The final norm, the pooling and the L2 normalisation run on the device
(DESIGN.md §11); the host does not normalise again.  LLAMA_POOLING_TYPE_RANK is not supported.
"""
from __future__ import annotations

import math
import os
import sys
import threading
import time
import uuid
from typing import Any, Dict, Iterator, List, Optional, Sequence, Union

from . import engine as _engine
from . import synth as _synth
from .llama_cache import BaseLlamaCache, LlamaDiskCache
from .llama_grammar import LlamaGrammar
from .speculative import LlamaDraftModel, LlamaPromptLookupDecoding
from .tokenizer import Tokenizer

LLAMA_DEFAULT_SEED = 0xFFFFFFFF
# llama.h enum llama_pooling_type (RANK = 4 is refused: it needs a classification head)
LLAMA_POOLING_TYPE_UNSPECIFIED = -1
LLAMA_POOLING_TYPE_NONE = 0
LLAMA_POOLING_TYPE_MEAN = 1
LLAMA_POOLING_TYPE_CLS = 2
LLAMA_POOLING_TYPE_LAST = 3
_POOLING_TYPES = (LLAMA_POOLING_TYPE_NONE, LLAMA_POOLING_TYPE_MEAN, LLAMA_POOLING_TYPE_CLS, LLAMA_POOLING_TYPE_LAST)


class Llama:
    def __init__(self, model_path: str, *, n_gpu_layers: int = -1, seed: int = LLAMA_DEFAULT_SEED, n_ctx: int = 512,
                 n_batch: int = 512, n_threads: Optional[int] = None, n_threads_batch: Optional[int] = None,
                 lora_base: Optional[str] = None, lora_scale: float = 1.0, lora_path: Optional[str] = None,
                 verbose: bool = True, n_seq_max: int = 64, device: int = -1, synthetic_seed: int = 0,
                 draft_model: Optional[LlamaDraftModel] = None, embedding: bool = False,
                 pooling_type: int = LLAMA_POOLING_TYPE_UNSPECIFIED, **kwargs: Any):
        """lora_path: a GGUF LoRA adapter (convert_lora_to_gguf.py), scaled by lora_scale * alpha / r.  It is
        merged into the weights on the device while the model loads: the model served is the one
        a BF16 file of the merged weights would give, and a quantised base is dequantised to bf16 for it.
        lora_base is accepted and ignored: it named an f16 base for llama.cpp's old merge of an adapter into a
        quantised model, and here the quantised base itself is dequantised."""
        # n_gpu_layers / n_threads are accepted for signature compatibility: the whole model always runs on
        # the GPU.  n_batch only bounds the tokens of one embed() input, as in llama-cpp-python.
        self._check_pooling_type(pooling_type)
        self.model_path = model_path
        self.verbose = verbose
        self._seed = seed
        self.draft_model = draft_model
        self._draft = self._draft_numbers(draft_model)
        if n_ctx == 0:
            n_ctx = 4096
        syn = _synth.parse_synthetic_path(model_path)
        if syn is None and not os.path.exists(model_path):
            raise ValueError(f"Model path does not exist: {model_path}")
        self.lora_base = lora_base
        self.lora_scale = lora_scale
        self.lora_path = lora_path
        if lora_path:
            try:
                self._engine = _engine.Engine(model_path, n_ctx=n_ctx, n_seq_max=n_seq_max, device=device,
                                              seed=synthetic_seed, lora_path=lora_path, lora_scale=lora_scale)
            except _engine.MxError as err:
                if err.code not in (_engine.MX_ERR_MODEL, _engine.MX_ERR_ARG):
                    raise
                raise RuntimeError(f"Failed to initialize LoRA adapter from lora path: {lora_path}") from err
            if verbose:
                self._print_lora_line(model_path)
        else:
            self._engine = _engine.Engine(model_path, n_ctx=n_ctx, n_seq_max=n_seq_max, device=device,
                                          seed=synthetic_seed)
        self._n_ctx = n_ctx
        self.cache = None
        self.n_batch = min(n_batch, n_ctx)
        self._embedding = bool(embedding)
        self._init_tokenizer(model_path, self._engine.info.n_vocab)
        self._pooling_type = self._resolve_pooling_type(pooling_type)

    def _print_lora_line(self, model_path: str):
        """One line on stderr: how many tensors the adapter was merged into and, for a quantised base, that the
        model now runs as bf16 and what that costs."""
        from .gguf import BLOCKS, GGML_BF16, GGUFReader, type_nbytes

        li = self._engine.lora_info()
        line = (f"llama_lora: merged {li['n_tensors']} tensors from {self.lora_path} (rank <= {li['rank_max']}, "
                f"alpha {li['alpha']:g}, scale {li['lora_scale']:g})")
        file_bytes = bf16_bytes = 0
        quantised = False
        for info in GGUFReader(model_path).tensors.values():
            n = 1
            for d in info["ne"]:
                n *= int(d)
            file_bytes += type_nbytes(info["type"], n)
            matrix = len(info["ne"]) == 2
            bf16_bytes += type_nbytes(GGML_BF16 if matrix else info["type"], n)
            quantised |= matrix and info["type"] in BLOCKS
        if quantised:
            line += (f"; the quantised base is dequantised: the model runs as bf16, {bf16_bytes} bytes of weights "
                     f"instead of {file_bytes}")
        print(line, file=sys.stderr)

    @staticmethod
    def _check_pooling_type(pooling_type: int):
        if pooling_type != LLAMA_POOLING_TYPE_UNSPECIFIED and pooling_type not in _POOLING_TYPES:
            raise ValueError(f"pooling_type must be LLAMA_POOLING_TYPE_UNSPECIFIED, NONE, MEAN, CLS or LAST "
                             f"(got {pooling_type}; LLAMA_POOLING_TYPE_RANK is not supported)")

    def _resolve_pooling_type(self, pooling_type: int) -> int:
        """UNSPECIFIED: the GGUF's llama.pooling_type if it has one, else NONE (llama.cpp's choice for a
        model without the key)."""
        self._check_pooling_type(pooling_type)
        if pooling_type != LLAMA_POOLING_TYPE_UNSPECIFIED:
            return int(pooling_type)
        key = f"{self.metadata.get('general.architecture', 'llama')}.pooling_type"
        md = int(self.metadata.get(key, LLAMA_POOLING_TYPE_NONE))
        if md not in _POOLING_TYPES:
            raise ValueError(f"{key} = {md} in {self.model_path} is not supported")
        return md

    @staticmethod
    def _draft_numbers(draft_model):
        """(num_pred_tokens, max_ngram_size) for Engine.submit(draft=), or None.  The lookup runs inside the
        device's decode step, which cannot call Python: only LlamaPromptLookupDecoding is a draft model here."""
        if draft_model is None:
            return None
        if not isinstance(draft_model, LlamaPromptLookupDecoding):
            raise NotImplementedError("draft_model must be a LlamaPromptLookupDecoding: speculation runs on the "
                                      "device, which cannot call another Python draft model")
        d, ng = int(draft_model.num_pred_tokens), int(draft_model.max_ngram_size)
        if d < 1 or d > _engine.SPEC_MAX_DRAFT:
            raise ValueError(f"num_pred_tokens must be 1..{_engine.SPEC_MAX_DRAFT} (a speculating step is one "
                             f"forward of 1 + num_pred_tokens <= 16 rows)")
        if ng < 1:
            raise ValueError("max_ngram_size must be >= 1")
        return d, ng

    @classmethod
    def from_engine(cls, model_path: str, engine, n_ctx: int = 512, seed: int = LLAMA_DEFAULT_SEED,
                    verbose: bool = True, n_batch: int = 512, embedding: bool = False,
                    pooling_type: int = LLAMA_POOLING_TYPE_UNSPECIFIED) -> "Llama":
        """A Llama over another engine object with Engine's request methods (submit / poll / cancel /
        wait, n_vocab, n_embd) -- the pipeline server's rank-0 front (pipeserve.py).  embed() needs an
        engine with supports_embeddings and embed()."""
        cls._check_pooling_type(pooling_type)
        self = cls.__new__(cls)
        self.model_path, self.verbose, self._seed = model_path, verbose, seed
        self._engine, self._n_ctx = engine, n_ctx
        self.draft_model, self._draft = None, None
        self.cache = None
        self.n_batch, self._embedding = min(n_batch, n_ctx), bool(embedding)
        self._init_tokenizer(model_path, engine.n_vocab)
        self._pooling_type = self._resolve_pooling_type(pooling_type)
        return self

    def _init_tokenizer(self, model_path: str, n_vocab: int):
        if _synth.parse_synthetic_path(model_path) is None:
            from .gguf import GGUFReader

            md = GGUFReader(model_path).metadata
            self.metadata = {k: v for k, v in md.items() if not isinstance(v, list)}
            self.tokenizer_ = Tokenizer.from_gguf_metadata(md)
        else:
            from .gguf import synthetic_spm_vocab

            toks, scores, types = synthetic_spm_vocab(n_vocab)
            self.tokenizer_ = Tokenizer(toks, scores, types, "llama", bos_id=1, eos_id=2)
            self.metadata = {"general.architecture": "llama", "general.name": model_path}
        self._lock = threading.Lock()

    # ---------------------------------------------------------------- prompt cache
    def set_cache(self, cache: Optional[BaseLlamaCache]):
        """llama-cpp-python's ``Llama.set_cache``: with a ``BaseLlamaCache`` (``LlamaRAMCache()``) later prompts
        start from the longest prefix whose K/V the engine already holds -- in any KV slot, free or busy, or being
        evaluated by another request of the same round -- copied between slots on the device (llama_cache.py,
        DESIGN.md §12); ``None`` switches that off.  On an engine with ``supports_host_cache`` the cache's
        ``capacity_bytes`` becomes the budget of the host-RAM tier behind the slots: the K/V of a
        slot that is about to be overwritten are kept in pinned host memory and come back by a transfer when a
        later prompt matches them; ``cache.cache_size`` then reports the bytes held, and ``None`` empties the
        tier.  The object is kept in ``Llama.cache``.  ``LlamaDiskCache``, and an engine front without
        ``supports_prefix_sharing`` (the pipeline server's), raise ``NotImplementedError``."""
        if cache is not None and not isinstance(cache, BaseLlamaCache):
            raise TypeError("set_cache takes a BaseLlamaCache (LlamaRAMCache()) or None")
        if isinstance(cache, LlamaDiskCache):
            raise NotImplementedError("LlamaDiskCache is not supported: the prompt cache is the device's KV slots")
        if not getattr(self._engine, "supports_prefix_sharing", False):
            raise NotImplementedError("this engine front has no prefix sharing (the pipeline server)")
        self._engine.set_prefix_sharing(cache is not None)
        if getattr(self._engine, "supports_host_cache", False):
            self._engine.set_host_cache(cache.capacity_bytes if cache is not None else 0)
            if self.cache is not None:
                self.cache._bind(None)
            if cache is not None:
                cache._bind(self._engine)
        self.cache = cache

    # ---------------------------------------------------------------- info
    def n_ctx(self) -> int:
        return self._n_ctx

    def n_vocab(self) -> int:
        return self._engine.n_vocab

    def n_embd(self) -> int:
        return self._engine.n_embd

    def pooling_type(self) -> int:
        return getattr(self, "_pooling_type", LLAMA_POOLING_TYPE_NONE)

    def token_bos(self) -> int:
        return self.tokenizer_.bos_id

    def token_eos(self) -> int:
        return self.tokenizer_.eos_id

    # ----------------------------------------------------------- tokenizer
    def tokenize(self, text: bytes, add_bos: bool = True, special: bool = False) -> List[int]:
        return self.tokenizer_.tokenize(text, add_bos=add_bos, special=special)

    def detokenize(self, tokens: Sequence[int], prev_tokens: Optional[Sequence[int]] = None,
                   special: bool = False) -> bytes:
        return self.tokenizer_.detokenize(tokens, prev_tokens=prev_tokens, special=special)

    # ---------------------------------------------------------- completion
    def create_completion(self, prompt: Union[str, List[int]], suffix: Optional[str] = None, max_tokens: Optional[int] = 16,
                          temperature: float = 0.8, top_p: float = 0.95, min_p: float = 0.05, typical_p: float = 1.0,
                          logprobs: Optional[int] = None, echo: bool = False,
                          stop: Optional[Union[str, List[str]]] = [], frequency_penalty: float = 0.0,
                          presence_penalty: float = 0.0, repeat_penalty: float = 1.0, top_k: int = 40,
                          stream: bool = False, seed: Optional[int] = None, tfs_z: float = 1.0,
                          mirostat_mode: int = 0, mirostat_tau: float = 5.0, mirostat_eta: float = 0.1,
                          logit_bias: Optional[Dict[int, float]] = None, grammar: Optional[LlamaGrammar] = None,
                          **kwargs: Any) -> Union[Dict[str, Any], Iterator[Dict[str, Any]]]:
        """llama-cpp-python's create_completion.  Every sampler setting is applied on the device, several decode
        steps per host round trip; top_k takes any value (<= 0 or at least the vocabulary size: every token is a
        candidate, as in llama-cpp-python).  Only a penalty window over 64 tokens, and tfs_z / typical_p over
        more than 64 candidates, are sampled on the host (engine.sample_plan tells).
        grammar: a LlamaGrammar (GBNF) -- every generated token is one the grammar allows after
        the ones before it, and once the grammar has ended only an end-of-generation token is.  A request whose
        grammar reaches a point where no token of the vocabulary is allowed raises RuntimeError."""
        ext_kw = self._sampler_ext_kw(typical_p, tfs_z, mirostat_mode, mirostat_tau, mirostat_eta, logit_bias)
        if grammar is not None:
            if not isinstance(grammar, LlamaGrammar):
                raise TypeError("grammar must be a LlamaGrammar (LlamaGrammar.from_string(gbnf))")
            if not getattr(self._engine, "supports_grammar", False):
                raise NotImplementedError("grammar is not supported by this engine front")
        if logprobs is not None:
            if logprobs < 0 or logprobs > _engine.TOPK_MAX:
                raise ValueError(f"logprobs must be 0..{_engine.TOPK_MAX} (llama-cpp-python has no cap; the "
                                 f"engine's device top-k holds at most {_engine.TOPK_MAX} entries per token)")
            if stream:
                raise NotImplementedError("logprobs with stream=True are not supported")
            if not getattr(self._engine, "supports_logprobs", False):
                raise NotImplementedError("logprobs are not supported by this engine front")
        created = int(time.time())
        cid = f"cmpl-{uuid.uuid4()}"
        if isinstance(prompt, str):
            prompt_tokens = self.tokenize(prompt.encode("utf-8"), add_bos=True, special=True)
        else:
            prompt_tokens = list(prompt)
        if len(prompt_tokens) >= self._n_ctx:
            raise ValueError(f"Requested tokens ({len(prompt_tokens)}) exceed context window of {self._n_ctx}")
        if max_tokens is None or max_tokens <= 0:
            max_tokens = self._n_ctx - len(prompt_tokens)
        max_tokens = min(max_tokens, self._n_ctx - len(prompt_tokens))
        sd = seed if seed is not None else self._seed
        lp_kw = {} if logprobs is None else {"logprobs": int(logprobs), "prompt_logprobs": bool(echo)}
        draft = getattr(self, "_draft", None)
        if draft is not None:  # only when set: engine fronts without the keyword keep working
            lp_kw["draft"] = draft
        lp_kw.update(ext_kw)  # only the non-default ones, as draft
        if grammar is not None:  # only when given, as draft
            lp_kw["grammar"] = grammar.compiled_for(self, self._grammar_vocab())
        req = self._engine.submit(prompt_tokens, max_tokens, temperature=temperature, top_k=top_k, top_p=top_p,
                                  min_p=min_p, repeat_penalty=repeat_penalty, frequency_penalty=frequency_penalty,
                                  presence_penalty=presence_penalty, seed=None if sd == LLAMA_DEFAULT_SEED else sd,
                                  **lp_kw)
        stops = [s for s in ([stop] if isinstance(stop, str) else list(stop or [])) if s]
        if stream:
            return self._stream(req, prompt_tokens, stops, cid, created, echo)
        if stops:  # stop strings end generation as soon as one appears (llama-cpp-python's check per token)
            n = 0
            while True:
                toks, done = self._engine.poll(req, n)
                n = len(toks)
                text = self.detokenize(toks, prev_tokens=prompt_tokens).decode("utf-8", errors="ignore")
                if done or any(s in text for s in stops):
                    break
            if not done:
                self._engine.cancel(req)
        lp = None
        if logprobs is not None:  # the entries live with the request: read them before wait() releases it
            n, done = 0, False
            while not done:
                toks, done = self._engine.poll(req, n)
                n = len(toks)
            lp = self._engine.logprobs(req)
        toks, finish = self._engine.wait(req)
        finish_reason = "stop" if finish == _engine.FINISH_STOP else "length"
        if toks and self.tokenizer_.is_eog(toks[-1]) and finish == _engine.FINISH_STOP:
            toks = toks[:-1]
        text = self.detokenize(toks, prev_tokens=prompt_tokens).decode("utf-8", errors="ignore")
        cut = min((text.find(s) for s in stops if s in text), default=-1)
        if cut >= 0:
            text = text[:cut]
            finish_reason = "stop"
            # the cancel lands after the scheduler's current round (up to 8 greedy steps), so tokens past
            # the stop may have been generated: count only those up to the one completing the stop
            # string, as llama-cpp-python does (its check runs after every token)
            for k in range(1, len(toks) + 1):
                t = self.detokenize(toks[:k], prev_tokens=prompt_tokens).decode("utf-8", errors="ignore")
                if any(s in t for s in stops):
                    toks = toks[:k]
                    break
        lp_dict = None
        if lp is not None:
            prompt_len = len(prompt) if isinstance(prompt, str) else len(self.detokenize(prompt_tokens).decode(
                "utf-8", errors="ignore"))
            lp_dict = self._logprobs_dict(prompt_tokens, toks, lp, int(logprobs), echo, prompt_len)
        if echo:
            text = self.detokenize(prompt_tokens).decode("utf-8", errors="ignore") + text
        if suffix is not None:
            text = text + suffix
        return {
            "id": cid, "object": "text_completion", "created": created, "model": self.model_path,
            "choices": [{"text": text, "index": 0, "logprobs": lp_dict, "finish_reason": finish_reason}],
            "usage": {"prompt_tokens": len(prompt_tokens), "completion_tokens": len(toks),
                      "total_tokens": len(prompt_tokens) + len(toks)},
        }

    def _grammar_vocab(self) -> "_engine.GrammarVocab":
        """The vocabulary grammars are matched against, built once: every token's piece as detokenize writes it
        (control, unknown and unused tokens have none and are never allowed) and the end-of-generation ids."""
        with self._lock:
            v = getattr(self, "_gvocab", None)
            if v is None:
                tk, n = self.tokenizer_, self._engine.n_vocab
                v = self._gvocab = _engine.GrammarVocab([tk.token_to_piece(t) for t in range(n)],
                                                         [t for t in range(n) if tk.is_eog(t)])
            return v

    def _sampler_ext_kw(self, typical_p, tfs_z, mirostat_mode, mirostat_tau, mirostat_eta, logit_bias) -> Dict[str, Any]:
        """The keywords of the extended sampler chain (typical_p, tfs_z, Mirostat v2, logit_bias) that are off
        llama-cpp-python's defaults, validated: only those are passed to the engine's submit(), so a front
        without them keeps working with default settings and raises NotImplementedError otherwise."""
        for name, v in (("typical_p", typical_p), ("tfs_z", tfs_z), ("mirostat_tau", mirostat_tau),
                        ("mirostat_eta", mirostat_eta)):
            if math.isnan(float(v)):
                raise ValueError(f"{name} is NaN")
        if mirostat_mode == 1:
            raise NotImplementedError("mirostat_mode=1 (Mirostat v1) is not supported; mirostat_mode=2 is")
        if mirostat_mode not in (0, 2):
            raise ValueError("mirostat_mode must be 0, 1 or 2")
        kw: Dict[str, Any] = {}
        if typical_p != 1.0:
            kw["typical_p"] = float(typical_p)
        if tfs_z != 1.0:
            kw["tfs_z"] = float(tfs_z)
        if mirostat_mode != 0:
            kw["mirostat_mode"] = int(mirostat_mode)
        if mirostat_mode != 0 and mirostat_tau != 5.0:  # tau / eta mean nothing without Mirostat
            kw["mirostat_tau"] = float(mirostat_tau)
        if mirostat_mode != 0 and mirostat_eta != 0.1:
            kw["mirostat_eta"] = float(mirostat_eta)
        if logit_bias:
            if len(logit_bias) > _engine.LOGIT_BIAS_MAX:
                raise ValueError(f"logit_bias holds more than {_engine.LOGIT_BIAS_MAX} entries")
            bias = {}
            for t, b in logit_bias.items():
                t, b = int(t), float(b)
                if t < 0 or t >= self.n_vocab():
                    raise ValueError(f"logit_bias: token id {t} is outside the vocabulary")
                if math.isnan(b) or b == math.inf:
                    raise ValueError("logit_bias: a bias must not be NaN or +inf (-inf bans a token)")
                bias[t] = b
            kw["logit_bias"] = bias
        if kw and not getattr(self._engine, "supports_sampler_ext", False):
            raise NotImplementedError(f"{', '.join(sorted(kw))}: not supported by this engine front")
        return kw

    def _logprobs_dict(self, prompt_tokens: List[int], toks: List[int], lp, k: int, echo: bool,
                       prompt_len: int) -> Dict[str, Any]:
        """choices[0]["logprobs"] as llama-cpp-python builds it: tokens / text_offset / token_logprobs /
        top_logprobs over the completion tokens that survived trimming (`toks`) and, with echo, the prompt
        tokens before them (a leading BOS skipped; the first entry's log-probs are None, the OpenAI quirk).
        lp = Engine.logprobs(): with echo one entry per prompt position >= 1 first, then one per generated
        token.  Each token is detokenised with the tokens before it as context -- as the text it adds to
        the text of those tokens, so the strings joined are the returned text even where a character's
        bytes span two tokens; text_offset is its character offset in the returned text, without echo
        offset by the prompt's length."""
        tok_lp, top_lp, top_idx = lp
        dec = lambda ids, prev: self.detokenize(ids, prev_tokens=prev).decode("utf-8", errors="ignore")
        n_p = len(prompt_tokens)
        if echo:  # listed: the prompt without a leading BOS, then the completion; decoded from the start
            skip = 1 if n_p and prompt_tokens[0] == self.token_bos() else 0
            listed, base, off0 = list(prompt_tokens[skip:]) + list(toks), [], 0
            entry = [p - 1 if p >= 1 else None for p in range(skip, n_p)] + [n_p - 1 + i for i in range(len(toks))]
        else:
            listed, base, off0 = list(toks), list(prompt_tokens), prompt_len
            entry = list(range(len(toks)))
        tokens, offsets, token_logprobs, top_logprobs = [], [], [], []
        upto = [""] + [dec(listed[:j + 1], base) for j in range(len(listed))]  # text of the first j listed tokens
        for j, (t, e) in enumerate(zip(listed, entry)):
            ctx = base + listed[:j]
            offsets.append(off0 + len(upto[j]))
            piece = upto[j + 1][len(upto[j]):]
            tokens.append(piece)
            if e is None:
                token_logprobs.append(None)
                top_logprobs.append(None)
                continue
            top = {dec([int(i)], ctx): float(v) for v, i in zip(top_lp[e][:k], top_idx[e][:k])}
            top[piece] = float(tok_lp[e])
            token_logprobs.append(float(tok_lp[e]))
            top_logprobs.append(top)
        if echo and tokens:
            token_logprobs[0] = None
            top_logprobs[0] = None
        return {"tokens": tokens, "text_offset": offsets, "token_logprobs": token_logprobs,
                "top_logprobs": top_logprobs}

    def _chunk(self, cid: str, created: int, text: str, finish_reason: Optional[str]) -> Dict[str, Any]:
        return {"id": cid, "object": "text_completion", "created": created, "model": self.model_path,
                "choices": [{"text": text, "index": 0, "logprobs": None, "finish_reason": finish_reason}]}

    def _stream(self, req: int, prompt_tokens: List[int], stops: List[str], cid: str, created: int,
                echo: bool) -> Iterator[Dict[str, Any]]:
        """stream=True (llama-cpp-python's chunk stream): text as the engine's scheduler produces tokens
        (up to 8 per round for greedy requests), each chunk the text decoded since the last one; text
        that could still become a stop string is held back, a stop string ends the stream there, and
        the last chunk carries the finish reason.  The chunks' texts joined equal the text of the
        same call without stream (tests/test_llama_stream.py)."""
        if echo:
            yield self._chunk(cid, created, self.detokenize(prompt_tokens).decode("utf-8", errors="ignore"), None)
        sent, n, cut, ended = 0, 0, -1, False
        try:
            while True:
                toks, done = self._engine.poll(req, n)
                n = len(toks)
                body = toks[:-1] if toks and self.tokenizer_.is_eog(toks[-1]) else toks
                text = self.detokenize(body, prev_tokens=prompt_tokens).decode("utf-8", errors="ignore")
                cut = min((text.find(s) for s in stops if s in text), default=-1)
                if cut >= 0:
                    if cut > sent:
                        yield self._chunk(cid, created, text[sent:cut], None)
                    sent = cut
                    ended = done
                    break
                # hold back the longest tail that is a proper prefix of a stop string
                hold = max((k for s in stops for k in range(1, len(s)) if text.endswith(s[:k])), default=0)
                if done:
                    hold = 0
                if len(text) - hold > sent:
                    yield self._chunk(cid, created, text[sent:len(text) - hold], None)
                    sent = len(text) - hold
                if done:
                    ended = True
                    break
        finally:  # a stop string, or a consumer that closed the stream: end the request, then release it
            if not ended:
                self._engine.cancel(req)
            toks, finish = self._engine.wait(req)
        yield self._chunk(cid, created, "", "stop" if cut >= 0 or finish == _engine.FINISH_STOP else "length")

    # ---------------------------------------------------------- embeddings
    def embed(self, input: Union[str, List[str]], normalize: bool = False, truncate: bool = True,
              return_count: bool = False):
        """Embeddings of a str (one item) or a list of str (a list of items), llama-cpp-python's Llama.embed:
        an item is a list of n_embd floats with MEAN / CLS / LAST pooling and a list of such lists, one per
        token, with LLAMA_POOLING_TYPE_NONE.  All inputs go to the engine in one call -- one batched prefill
        without lm_head; output norm, pooling and (normalize) v / ||v|| run on the device."""
        if not getattr(self, "_embedding", False):
            raise RuntimeError("Llama model must be created with embedding=True to call this method")
        if not getattr(self._engine, "supports_embeddings", False):
            raise NotImplementedError("embeddings are not supported by this engine front")
        n_batch = getattr(self, "n_batch", self._n_ctx)
        inputs = [input] if isinstance(input, str) else list(input)
        prompts, total_tokens = [], 0
        for text in inputs:
            tokens = self.tokenize(text.encode("utf-8"))
            if truncate:
                tokens = tokens[:n_batch]
            if len(tokens) > n_batch:
                raise ValueError(f"Requested tokens ({len(tokens)}) exceed batch size of {n_batch}")
            total_tokens += len(tokens)
            prompts.append(tokens)
        pooling = self.pooling_type()
        vecs = self._engine.embed(prompts, pooling=pooling, normalize=bool(normalize)) if prompts else []
        if pooling == LLAMA_POOLING_TYPE_NONE:
            data = [[[float(v) for v in row] for row in a] for a in vecs]
        else:
            data = [[float(v) for v in a[0]] for a in vecs]
        output = data[0] if isinstance(input, str) else data
        return (output, total_tokens) if return_count else output

    def create_embedding(self, input: Union[str, List[str]], model: Optional[str] = None) -> Dict[str, Any]:
        """llama-cpp-python's Llama.create_embedding: the OpenAI-style embedding object."""
        inputs = input if isinstance(input, list) else [input]
        embeddings, total_tokens = self.embed(inputs, return_count=True)
        data = [{"object": "embedding", "embedding": e, "index": i} for i, e in enumerate(embeddings)]
        return {"object": "list", "data": data, "model": model if model is not None else self.model_path,
                "usage": {"prompt_tokens": total_tokens, "total_tokens": total_tokens}}

    def __call__(self, prompt: Union[str, List[int]], *args, **kwargs) -> Dict[str, Any]:
        return self.create_completion(prompt, *args, **kwargs)

    def close(self):
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
            self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
