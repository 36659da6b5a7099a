/*
 * mx_engine.h -- C ABI of the MI355X-native local-inference engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * node builds its model and calls it exactly twice:
 *
 *   self.model = Llama(model_path=model_path)                 llama_p2p_network.py:19
 *   result = self.model(prompt, max_tokens=100)["choices"][0]["text"]
 *                                                             llama_p2p_network.py:125
 *
 * Both calls land in llama-cpp-python (module llama_cpp, ~0.3.1), whose own
 * ctypes binding to llama.cpp is what these entry points replace:
 *   mx_engine_create   <- llama_load_model_from_file + llama_new_context_with_model
 *                         (Llama.__init__, reached from :19)
 *   mx_submit/mx_wait  <- Llama.__call__ -> create_completion -> generate():
 *                         llama_decode + sampling per token (reached from :125)
 *   mx_forward_logits  <- llama_decode + llama_get_logits (Llama.eval), parity hook
 *   mx_submit_lp / mx_request_logprobs
 *                      <- create_completion(logprobs=k): Llama.logits_to_logprobs + the top-k sort
 *   mx_submit_ext      <- create_completion(typical_p=, tfs_z=, mirostat_mode=2, logit_bias=): the samplers
 *                         Llama._init_sampler puts around the default chain (logit bias, tail-free, typical,
 *                         Mirostat v2); mx_sample_probe runs that chain on caller-supplied rows
 *   mx_submit_spec     <- Llama(draft_model=LlamaPromptLookupDecoding(...)): generate()'s draft / verify loop
 *   mx_submit_embed / mx_wait_embed
 *                      <- Llama(embedding=True).embed / create_embedding: llama_decode of the inputs, then
 *                         llama_get_embeddings (pooling NONE) / llama_get_embeddings_seq (MEAN, CLS, LAST)
 *   mx_pool_probe      <- the kernels behind them (result_norm, the pooling graph, _normalize_embedding) alone
 *   mx_engine_destroy  <- llama_free / llama_free_model (Llama.__del__)
 * The Python layer (llama-p2p_amd/llama.py) mirrors the Llama class on top of
 * this ABI, so handle_requests / cached_inference / distributed_inference /
 * compute_model_hash (llama_p2p_network.py:84-182) run unchanged.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative MX_ERR_* code, with a message in mx_last_error()
 * (thread-local).  The engine owns device weights, KV cache and streams; the
 * caller owns every host buffer it passes.  mx_submit/mx_wait may be called
 * from any thread (one internal scheduler thread micro-batches all requests);
 * blocking calls are made with the GIL released when bound via ctypes.CDLL.
 */
#ifndef MX_ENGINE_H
#define MX_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_ARG (-1)      /* bad argument / unsupported shape */
#define MX_ERR_HIP (-2)      /* HIP runtime error */
#define MX_ERR_MODEL (-3)    /* model file missing / malformed / unsupported tensor type */
#define MX_ERR_CTX (-4)      /* prompt does not fit n_ctx (Llama raises ValueError) */
#define MX_ERR_NOTFOUND (-5) /* unknown request id */
#define MX_ERR_STATE (-6)    /* engine shutting down / wrong pipeline stage for this call */
#define MX_DEBUG_STOPPED 1   /* a 17..64-row forward ended at the mx_debug stop (diagnosis only) */

#define MX_FINISH_LENGTH 0 /* max_tokens or n_ctx reached  ("length") */
#define MX_FINISH_STOP 1   /* end-of-generation token: tokenizer.ggml.eos_token_id or, when the file has
                              one, tokenizer.ggml.eot_token_id -- returned as the last token; also a
                              cancelled request              ("stop")   */
#define MX_FINISH_ERROR 2

typedef struct mx_engine mx_engine;
typedef struct mx_batch mx_batch;

typedef struct {
  int32_t n_ctx;       /* positions per sequence; llama-cpp-python default 512 */
  int32_t n_seq_max;   /* concurrent sequences (KV slots) */
  int32_t layer_begin; /* pipeline stage: first layer held here (0) */
  int32_t layer_end;   /* one past the last layer held here (-1 = all) */
  int32_t device;      /* HIP device ordinal, -1 = current device */
  int32_t use_graphs;  /* capture decode steps as hipGraphs (1) */
  uint64_t seed;       /* weights seed for "synthetic:<shape>" model paths */
  int32_t handoff_bf16;/* pipeline stage hand-off: x_in / x_out of mx_batch_step, mx_stage_rows and
                          mx_stage_rows_pick are bf16 [rows][n_embd] (1) instead of f32 (0) */
} mx_opts;

typedef struct {
  int32_t n_embd, n_layer, n_head, n_head_kv, head_dim, n_ff, n_vocab, n_ctx_train;
  float eps, rope_base;
  int32_t bos_id, eos_id;
  int32_t n_ctx, n_seq_max;
  int32_t layer_begin, layer_end, has_embed, has_head;
  uint64_t weight_bytes; /* device bytes of the weights this stage streams per decode step */
  int32_t weight_type;       /* ggml type of the layer matrices: 30 BF16, 8 Q8_0, 2 Q4_0, 12 Q4_K (Q4_K_M), 13 Q5_K (Q5_K_M) */
  int32_t eot_id;            /* tokenizer.ggml.eot_token_id: ends a request like eos_id; -1 when the file has none */
} mx_model_info;

typedef struct {
  float temperature;    /* <= 0 -> greedy argmax on device (ties -> lowest id) */
  int32_t top_k;        /* llama-cpp-python defaults: 40 */
  float top_p;          /* 0.95 */
  float min_p;          /* 0.05 */
  float repeat_penalty; /* 1.0 = off */
  int32_t repeat_last_n;/* 64 */
  uint64_t seed;
  int32_t ignore_eos;
  float frequency_penalty; /* 0.0 = off: logit -= count * frequency_penalty (llama.cpp penalties sampler) */
  float presence_penalty;  /* 0.0 = off: logit -= (count > 0) * presence_penalty */
} mx_sampling;

/* One row's sampler for the device sampling chain (pipeline lanes, mx_batch_reset / mx_stage_rows_pick):
 * the settings, the request's sampler stream (seed; the n-th sampled token of a request uses draw n),
 * how many tokens it sampled so far, and its penalty window -- the last n_win (<= 64) tokens of
 * prompt + output.  temperature <= 0 without penalties = greedy argmax.  Device-sampleable settings:
 * top_k in 1..64 and, with penalties, repeat_last_n in 0..64 (otherwise MX_ERR_ARG). */
typedef struct {
  mx_sampling s;
  uint64_t seed;
  int32_t n_drawn;
  int32_t n_win;
  int32_t win[64];
} mx_row_sampler;

void mx_opts_default(mx_opts* o);
void mx_sampling_default(mx_sampling* s);
const char* mx_last_error(void);

/* model_path: a GGUF file (LLaMA; all-BF16, all-Q8_0, all-Q4_0 and Q4_K_M / Q5_K_M files natively -- the
 * quantised ones on the int8 MFMA with ggml's arithmetic; any other mix of F32 / F16 / BF16 / Q4_0 / Q8_0
 * / K-quant matrices dequantised to bf16 at load) or "synthetic:<shape>[:seed=N][:q8_0|:q4_0|:q4_k_m|:q5_k_m]" */
int mx_engine_create(const char* model_path, const mx_opts* opts, mx_engine** out);
void mx_engine_destroy(mx_engine* e);
/* Parse a GGUF container without touching a GPU (header, metadata, tensor table, bounds of every
 * tensor against the file): 0, or MX_ERR_MODEL with the reason in mx_last_error(). */
int mx_gguf_check(const char* path);
int mx_engine_info(const mx_engine* e, mx_model_info* out);

/* LoRA adapters (llama-cpp-python's Llama(lora_path=, lora_scale=)), DESIGN.md §16.  The adapter is merged into
 * the weights while the model loads: for every base matrix T with a pair, W' = bf16(W + scale B A) with A =
 * T.lora_a (f32 [r][n_in]), B = T.lora_b (f32 [n_out][r]), scale = lora_scale * adapter.lora.alpha / r (lora_scale
 * alone when alpha is 0; llama.cpp's rule), the sum over r and the update in f32, one RNE rounding to bf16.  The
 * engine then is the one a BF16 GGUF of the merged model would give -- not llama.cpp's run-time adapter, which adds
 * scale B (A x) beside every product and never rounds W' -- and every kernel, row count and graph runs as without.
 * A quantised base (Q8_0, Q4_0, K-quants) leaves its native path: every matrix, token_embd included, is dequantised
 * to bf16 at load, mx_model_info.weight_type is 30 and the weights take 2 bytes per element.
 * lora_path: a GGUF written by convert_lora_to_gguf.py: general.type "adapter", adapter.type "lora",
 * general.architecture "llama"; tensors T.lora_a ne {n_in, r} and T.lora_b ne {r, n_out} (F32, F16 or BF16) for
 * any subset of blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight, r per tensor, merged in
 * GGUF order (the converter has permuted q / k already).  Checked against the base before anything is allocated
 * on the device; MX_ERR_MODEL with the tensor or key named for a wrong type key, a half pair, a shape that does
 * not fit the base, r < 1, a target outside the base or the seven matrices, a quantised adapter tensor.  Pairs of
 * layers outside [layer_begin, layer_end) are skipped.  lora_scale == 0 and tensors without a pair skip the merge:
 * those weights are the base's bit for bit.  A "synthetic:" base, a NULL path, a non-finite scale: MX_ERR_ARG. */
int mx_engine_create_lora(const char* model_path, const mx_opts* opts, const char* lora_path, float lora_scale,
                          mx_engine** out);
/* The same validation of an adapter against its base, no GPU touched (as mx_gguf_check). */
int mx_lora_check(const char* model_path, const char* lora_path);
/* n_tensors: matrices of this engine's layers the adapter was merged into (0 without an adapter or with
 * lora_scale 0); rank_max: the largest r among them; alpha, lora_scale: as loaded (0 without an adapter). */
typedef struct {
  int32_t n_tensors, rank_max;
  float alpha, lora_scale;
} mx_lora_info;
int mx_engine_lora_info(const mx_engine* e, mx_lora_info* out);
/* launch_lora_merge, the production launch, on caller-supplied data, no engine: w bf16 [rows][cols], A f32
 * [r][cols], B f32 [rows][r]; rows, cols 1..65536 with rows * cols <= 2^28, r 1..4096, scale finite.  out: uint16
 * [rows * cols + 4096], filled with 0xFF bytes before the launch (the last 4096 elements are a guard that must come
 * back as 0xFF); it receives w merged by one launch.  iters > 0: the kernel alone is then launched iters more
 * times (on the merged matrix, after two warm-up launches) between two HIP events, *us_per_launch the mean;
 * iters == 0 leaves it alone.  Anything else is MX_ERR_ARG and nothing is launched. */
int mx_lora_merge_probe(int device, int rows, int cols, int r, const uint16_t* w, const float* A, const float* B,
                        float scale, uint16_t* out, int iters, double* us_per_launch);

/* Parity hook: evaluate n tokens of sequence `slot` at positions pos0..pos0+n-1
 * (prefill or decode, chunked internally by 64 rows) and copy the f32 logits of
 * every row to logits_out[n][n_vocab]; NULL skips lm_head entirely (prefill). */
int mx_forward_logits(mx_engine* e, int slot, const int32_t* ids, int n, int pos0, float* logits_out);

/* General rows forward: row i is token ids[i] of sequence slots[i] at pos[i]; logits_out as above. */
int mx_forward_rows(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                    float* logits_out);

/* Parity hook for the sampler: rows forward as mx_forward_rows (n <= 64), then the device top-k
 * kernel (the sampler chain's candidate selection): vals/idx [n][k], value descending, ties -> lower
 * id; k <= 64. */
int mx_forward_topk(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids, int k,
                    float* vals, int32_t* idx);

/* Request API (what Llama.__call__ uses).  Tokens are generated by the
 * scheduler thread, micro-batched with every other active request. */
int mx_submit(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, uint64_t* req);
/* n_req requests submitted atomically (all validated first, then queued under one lock): the
 * scheduler admits them in one round -- one batched prefill, one decode batch.  s: n_req sampling
 * settings (NULL: defaults); reqs receives the ids. */
int mx_submit_batch(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens, const mx_sampling* s,
                    const int32_t* max_tokens, uint64_t* reqs);
/* Blocks until the request finishes; copies up to cap generated ids and releases the request.
 * If more than cap ids were generated, nothing is released: *n_out is set and MX_ERR_ARG returned,
 * so the caller can retry with a larger buffer. */
int mx_wait(mx_engine* e, uint64_t req, int32_t* out_ids, int cap, int* n_out, int* finish);
/* Incremental read (streaming / stop strings): blocks until the request holds more than n_have
 * generated ids or has finished; copies the first min(cap, n) ids, *n_out = n, *done = finished.
 * The request stays registered (mx_wait releases it). */
int mx_poll(mx_engine* e, uint64_t req, int n_have, int32_t* out_ids, int cap, int* n_out, int* done);
/* Ask the scheduler to end a request after its current step (finish reason STOP), e.g. when the
 * caller found a stop string.  The request still has to be released with mx_wait. */
int mx_cancel(mx_engine* e, uint64_t req);

/* Per-token log-probabilities (llama-cpp-python's create_completion(logprobs=k)).  For a logits row x
 * with m = max x and s = sum exp(x_i - m): logprob(i) = (x_i - m) - log(s), in f32, over the raw lm_head
 * row (before the penalties of the sampler chain rewrite it), computed on the device inside the decode
 * step, so multi-step rounds keep running without a host round-trip.
 *
 * mx_submit_lp: as mx_submit; the request also records, per generated token, the token's log-prob and the
 * min(n_logprobs, n_vocab) most likely tokens (value descending, ties -> lower id).  n_logprobs 0..64
 * (0: the chosen token only), anything else MX_ERR_ARG.  prompt_logprobs != 0: also one entry per prompt
 * position p >= 1 (log-prob of prompt[p] given prompt[:p]); such a request evaluates its whole prompt
 * (no prefix reuse). */
int mx_submit_lp(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, int n_logprobs,
                 int prompt_logprobs, uint64_t* req);
/* Copies the entries the request holds so far -- the prompt's first (when asked for), then one per
 * generated token; a token returned by mx_poll always has its entry: the first min(cap, n) of
 * tok_lp[n], top_lp[n][k], top_idx[n][k] (any may be NULL), *n_out = n, *k_out = k.  Never blocks; valid
 * until mx_wait releases the request.  MX_ERR_ARG for a request submitted without log-probabilities. */
int mx_request_logprobs(mx_engine* e, uint64_t req, float* tok_lp, float* top_lp, int32_t* top_idx, int cap,
                        int* n_out, int* k_out);
/* Parity hook: rows forward as mx_forward_rows (n <= 64), then the log-prob kernels: tgt_lp[n] = log-prob
 * of targets[i] in row i, top_lp / top_idx [n][min(k, n_vocab)] (k 0..64; NULL allowed when k = 0).
 * logits_out (optional, [n][n_vocab]) receives the very rows the statistics were computed from. */
int mx_forward_logprobs(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                        const int32_t* targets, int k, float* tgt_lp, float* top_lp, int32_t* top_idx,
                        float* logits_out);
/* The same kernels on caller-supplied rows, no engine (tests on inputs no model produces):
 * logits_host [n][ldl] f32 with V <= ldl valid columns, n <= 64, V <= 262144; outputs as above. */
int mx_logprob_probe(int device, const float* logits_host, int n, int V, int ldl, const int32_t* targets, int k,
                     float* tgt_lp, float* top_lp, int32_t* top_idx);
/* The rest of llama-cpp-python 0.3.1's sampler chain (create_completion's typical_p, tfs_z, mirostat_mode / tau /
 * eta and logit_bias), on the device inside the multi-step rounds like the chain of mx_sampling:
 *   logit_bias -> penalties -> then
 *     temperature <= 0:    greedy argmax (nothing else applies)
 *     mirostat_mode == 2:  temperature -> Mirostat v2 over the whole vocabulary (no top_k / tfs / typical / top_p / min_p)
 *     otherwise:           top_k -> tail-free (tfs_z) -> locally typical (typical_p) -> top_p -> min_p -> temperature -> draw
 * logit_bias: n_logit_bias <= 256 entries (bias_tok[i], bias_val[i]), distinct ids inside the vocabulary, one f32
 * add each; -inf bans the token, +inf and NaN are refused.  Mirostat v2 keeps per request mu (2 tau at submission,
 * carried across steps and rounds): tokens with -log2 p <= mu stay (the argmax when none does), the draw walks them
 * by ascending id, mu -= eta (-log2 p'_tok - tau).  mirostat_mode 1 (a sort of the whole vocabulary), any other
 * mode, NaN settings and a bad bias table are MX_ERR_ARG.  Log-probabilities stay those of the raw lm_head row.
 * A request with any of these settings never speculates.  mx_sampling / mx_row_sampler are unchanged.
 * base.top_k: any value samples on the device.  <= 0 or >= the vocabulary: every token is a candidate; more than
 * 64 candidates take the wide kernel, which has no tail-free / typical cut: tfs_z < 1 or
 * typical_p < 1 over more than 64 candidates is sampled on the host (mx_sample_plan tells which). */
typedef struct {
  mx_sampling base;
  float typical_p, tfs_z;   /* 1.0 = off */
  int32_t mirostat_mode;    /* 0 or 2 */
  float mirostat_tau, mirostat_eta; /* 5.0, 0.1 */
  int32_t n_logit_bias;
  const int32_t* bias_tok;
  const float* bias_val;
} mx_sampling_ext;
void mx_sampling_ext_default(mx_sampling_ext* s);
/* As mx_submit (n_logprobs == -1) or mx_submit_lp (n_logprobs 0..64, prompt_logprobs): everything is validated
 * before the request is queued, and the bias table is copied. */
int mx_submit_ext(mx_engine* e, const int32_t* ids, int n, const mx_sampling_ext* s, int max_tokens, int n_logprobs,
                  int prompt_logprobs, uint64_t* req);
/* As mx_submit_batch with one mx_sampling_ext per request: all validated first, then queued under one lock. */
int mx_submit_ext_batch(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens,
                        const mx_sampling_ext* s, const int32_t* max_tokens, uint64_t* reqs);
/* Which sampler picks the rows of a request with these settings over a vocabulary of V -- what the scheduler, the
 * prefill and mx_sample_probe dispatch on; no GPU touched.  Validates as mx_submit_ext (MX_ERR_ARG otherwise; also
 * for V < 1).  k_eff = V when top_k <= 0 or top_k >= V, else top_k; penalties = a repeat / frequency / presence
 * penalty off its default.  The first rule that holds:
 *   temperature <= 0, no penalties, no logit_bias       MX_PICK_ARGMAX    the argmax kernels
 *   penalties with repeat_last_n < 0 or > 64            MX_PICK_HOST      the host sampler; the whole round with it
 *   temperature <= 0 otherwise                          MX_PICK_CHAIN     (greedy never reads top_k)
 *   mirostat_mode == 2                                  MX_PICK_MIROSTAT  the Mirostat kernels
 *   k_eff <= 64                                         MX_PICK_CHAIN     top-k kernels + the per-row pick kernel
 *   k_eff > 64 with tfs_z < 1 or typical_p < 1          MX_PICK_HOST
 *   k_eff > 64 with V > 262144                          MX_PICK_HOST
 *   anything else                                       MX_PICK_WIDE      the wide kernel over k_eff candidates */
#define MX_PICK_ARGMAX 0
#define MX_PICK_CHAIN 1
#define MX_PICK_MIROSTAT 2
#define MX_PICK_WIDE 3
#define MX_PICK_HOST 4
int mx_sample_plan(const mx_sampling_ext* s, int V, int32_t* path);
/* Sampler counters of the request path (mx_stats is fixed): device_steps / host_steps: decode steps whose picks
 * ran on the device (greedy or any chain) / in the host sampler; wide_rows: row-steps the wide kernel picked, the
 * first token from the prefill included; rounds: the scheduler rounds those steps ran in (a device round runs
 * several steps per host round trip, a host round one). */
typedef struct {
  uint64_t device_steps, host_steps, wide_rows, rounds;
} mx_sampler_counts;
int mx_sampler_stats(mx_engine* e, mx_sampler_counts* out);
/* The chain on caller-supplied rows, no engine: logits_host [n][ldl] f32 with V <= ldl valid columns, n <= 64,
 * V <= 262144; row i samples draw n_drawn[i] of stream seeds[i] with penalty window win[i][0..n_win[i]) (<= 64) and
 * Mirostat state mu_in[i].  device >= 0: the production launch sequence (bias -> penalties -> top-k -> sample
 * kernel, Mirostat kernels, wide kernel), each row on the path mx_sample_plan gives it, mixed freely; a row on
 * MX_PICK_HOST is refused; device == -1: the host sampler, no GPU touched.  tok_out / mu_out [n] start as 0xFF bytes; logits_out (optional, [n][ldl]): the
 * rows as the chain left them (bias and penalties applied), columns >= V bit-identical.  Anything invalid:
 * MX_ERR_ARG, nothing launched. */
int mx_sample_probe(int device, const float* logits_host, int n, int V, int ldl, const mx_sampling_ext* samp,
                    const uint64_t* seeds, const int32_t* n_drawn, const int32_t* win, const int32_t* n_win,
                    const float* mu_in, int32_t* tok_out, float* mu_out, float* logits_out);
/* Prompt-lookup speculative decoding (llama-cpp-python's draft_model=LlamaPromptLookupDecoding(max_ngram_size,
 * num_pred_tokens)), on the device: the draft is the tokens that followed the earliest earlier occurrence of the
 * sequence's last n-gram, verified in one forward of 1 + num_pred_tokens rows of the request's slot.  The tokens
 * are bitwise those of the same request submitted with mx_submit.
 *
 * mx_submit_spec: as mx_submit; num_pred_tokens 1..15, max_ngram_size >= 1 (otherwise MX_ERR_ARG).  A request
 * speculates in the rounds where every active request is eligible -- greedy (temperature <= 0), no penalties,
 * a bf16 model -- their rows fit (requests x (1 + largest num_pred_tokens) <= 16) and none is close to n_ctx;
 * every other round, and an ineligible request always, decodes as after mx_submit. */
int mx_submit_spec(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, int num_pred_tokens,
                   int max_ngram_size, uint64_t* req);
/* steps: speculating forwards whose tokens the request kept; drafted / accepted: draft tokens those verified /
 * found right (a step yields accepted + 1 tokens).  req: a registered request (until mx_wait releases it), or
 * 0 for the totals of every request so far. */
typedef struct {
  uint64_t steps, drafted, accepted;
} mx_spec_counts;
int mx_spec_stats(mx_engine* e, uint64_t req, mx_spec_counts* out);
/* The draft kernel on caller-supplied sequences, no engine: R (1..8) sequences tokens[r][0..lens[r]) in rows of
 * `stride` int32 (1 <= lens[r] <= stride <= 2^20), D = num_pred_tokens 1..15 with R (1 + D) <= 16, ngram >= 1,
 * pos0[r] (>= 0, pos0[r] + D < 2^30) / slot0[r] (>= 0) the position and slot of each sequence's row 0.
 * ids / pos / slot [R][1 + D] and n_draft [R] start as 0xFF bytes and return whole (row 0 of ids untouched:
 * the kernel writes rows 1..D).  Anything else: MX_ERR_ARG, nothing launched. */
int mx_draft_probe(int device, int R, const int32_t* tokens, int stride, const int32_t* lens, int D, int ngram,
                   const int32_t* pos0, const int32_t* slot0, int32_t* ids, int32_t* pos, int32_t* slot,
                   int32_t* n_draft);
/* argmax_stage1 + the accept kernel on caller-supplied logits rows [R (1 + D)][V] (R 1..8, D 1..15,
 * R (1 + D) <= 16, 1 <= V <= 2^20), draft [R][D] (ids in [0, V)), n_draft [R] (0..D), pos0 [R] >= 0.
 * a [R]: accepted drafts; emitted [R][1 + D]: the a + 1 tokens, the rest still 0xFF bytes; next_id [R];
 * new_pos [R] = pos0 + a + 1; counts [R][3] = steps, drafted, accepted (from 0).  Anything else: MX_ERR_ARG. */
int mx_accept_probe(int device, int R, int D, int V, const float* logits, const int32_t* draft, const int32_t* n_draft,
                    const int32_t* pos0, int32_t* a, int32_t* emitted, int32_t* next_id, int32_t* new_pos,
                    int32_t* counts);

/* Embeddings (llama-cpp-python's Llama(embedding=True).embed / create_embedding), DESIGN.md §11.  Per row of the
 * last layer's f32 residual stream x: y = (x * 1/sqrtf(mean(x^2) + eps)) * output_norm.weight in f32 (ggml's
 * result_norm, with the engine's canonical sum of squares); then over the rows of one sequence of T tokens:
 * NONE every y, MEAN per column (((y0 + y1) + y2) + ...) / T in f32 in position order, CLS y0, LAST y(T-1);
 * normalize != 0: every output vector v becomes v / ||v|| (a vector of norm 0 stays as it is; never NaN).
 * All of it runs on the device; only the result crosses to the host. */
#define MX_POOL_NONE 0
#define MX_POOL_MEAN 1
#define MX_POOL_CLS 2
#define MX_POOL_LAST 3
/* n_req embedding requests queued atomically (as mx_submit_batch): one batched prefill without lm_head.  Each
 * takes a KV slot while it runs and evaluates its whole prompt (no prefix reuse); the slot keeps the prompt's
 * K/V for a later completion to reuse.  lens[i] 1..n_ctx (0: MX_ERR_ARG, above n_ctx: MX_ERR_CTX); pooling
 * MX_POOL_*, anything else MX_ERR_ARG; a pipeline-stage engine: MX_ERR_STATE.  mx_wait / mx_poll /
 * mx_request_logprobs on such a request give MX_ERR_ARG. */
int mx_submit_embed(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens, int pooling, int normalize,
                    uint64_t* reqs);
/* Blocks until the request is done; copies rows * n_embd floats (rows = its length for MX_POOL_NONE, else 1) and
 * releases it.  Too small a cap: *rows_out set, MX_ERR_ARG, nothing released (as mx_wait).  MX_ERR_ARG for a
 * request that is not an embedding request. */
int mx_wait_embed(mx_engine* e, uint64_t req, float* out, size_t cap_floats, int* rows_out);
/* The same kernels through the same launch sequence on caller-supplied rows, no engine (tests on inputs no model
 * produces): x f32 [rows][n] (1 <= rows <= 32768, n % 64 == 0, 64 <= n <= 16384, rows * n <= 2^26), w f32 [n];
 * sequence q is rows [seq_begin[q], seq_begin[q + 1]) (seq_begin [n_seq + 1] strictly increasing from 0 to rows);
 * x is processed in chunks of chunk_rows rows (a multiple of 16; 0: one chunk), the MEAN running sums carried
 * between chunks as the engine carries them.  out: [(NONE ? rows : n_seq) + 64][n], filled with 0xFF bytes before
 * the first launch (the last 64 rows are a guard that must come back as 0xFF).  Anything else is MX_ERR_ARG and
 * nothing is launched. */
int mx_pool_probe(int device, int rows, int n, const float* x, const float* w, float eps, int n_seq,
                  const int32_t* seq_begin, int chunk_rows, int pooling, int normalize, float* out);

/* The production attention launchers on caller-supplied q / K / V, no engine (tests on inputs no model
 * produces).  Geometry: head_dim 64 or 128, n_head / n_head_kv in {1, 2, 4, 5, 6, 7, 8}; caches of n_slots slots with
 * ctx_stride = n_ctx rounded up to 64 positions; M rows (1..4096) at pos[i] in [0, n_ctx] (n_ctx: the kernels
 * clamp it) of slot[i]; scale = 1/sqrt(head_dim).  kcache / vcache: the raw tiled bytes,
 * n_slots * n_head_kv * ctx_stride * head_dim f16 each, copied to the device verbatim and copied back after
 * the launch.  out [M][n_head * head_dim], f32 (out_f32 != 0) or bf16, filled with 0xFF bytes before the
 * launch.  mode 0: the decode attention on final q [M][n_head * head_dim] f32; mode 1: the same launcher
 * finishing q/k/v from split-K slabs [nslab][M][(n_head + 2 n_head_kv) * head_dim] (1 <= nslab <= 8, M <= 64,
 * every row its own slot) with rope_cs [n_ctx][head_dim/2][cos, sin] -- it stores each row's K/V into the
 * caches; mode 2: the prefill attention on final q (rows in 16-row blocks of consecutive positions of one
 * slot, a block may end in copies of its last row).  bias (mode 1, optional): the q/k/v bias, f32 [(n_head + 2
 * n_head_kv) * head_dim], added to the summed slabs before RoPE; NULL: none.
 * Anything else is MX_ERR_ARG and nothing is launched. */
int mx_attention_probe(int device, int mode, int n_head, int n_head_kv, int head_dim, int n_ctx, int n_slots, int M,
                       const int32_t* pos, const int32_t* slot, int out_f32, const float* q, const float* slabs,
                       int nslab, const float* rope_cs, void* kcache, void* vcache, void* out, const float* bias);

/* Prefix sharing across KV slots (llama-cpp-python's Llama.set_cache(LlamaRAMCache())), DESIGN.md §12.  Off by
 * default.  On: at admission a request whose prompt shares a longer prefix with the tokens another slot holds
 * K/V for -- free or busy, or a request admitted earlier in the same round -- than with its own slot's gets those
 * positions by a device copy between the slots (one launch for all copies of a round) instead of evaluating
 * them, when that saves at least 16 positions.  Requests with prompt log-probabilities and embedding requests
 * evaluate their whole prompt as before (their slots serve as sources).  Takes effect at the next admission; a
 * pipeline-stage engine returns MX_ERR_STATE. */
int mx_engine_set_prefix_sharing(mx_engine* e, int on);
/* shared_prompt_tokens: prompt positions a request received by a copy (mx_stats.reused_prompt_tokens keeps
 * counting only the positions kept in place); copies: slot-to-slot copies; copied_bytes: bytes they wrote;
 * follower_requests: requests that waited for a request of their own round and copied its prefix. */
typedef struct {
  uint64_t shared_prompt_tokens, copies, copied_bytes, follower_requests;
} mx_sharing_stats;
int mx_prefix_sharing_stats(mx_engine* e, mx_sharing_stats* out);
/* The copy kernel on caller-supplied caches, no engine.  kcache / vcache: the raw tiled bytes of
 * n_layer * n_slots * n_head_kv * ctx_stride * head_dim f16 each ([layer][slot][kv head], ctx_stride = n_ctx
 * rounded up to 64), at most 1 GiB each, copied to the device verbatim and copied back after the launch.  Copy i
 * moves positions [0, P), P = n_pos rounded up to 32, of slot src_slot to slot dst_slot in every layer and kv
 * head of both caches; every other byte stays.  n_layer 1..256, n_slots 1..4096, n_head_kv 1..64, head_dim 64 or
 * 128, n_ctx 1..2^20, 1 <= n_copies <= n_slots; slots in range, src_slot != dst_slot, 1 <= n_pos <= n_ctx, no
 * slot a destination twice, none both a source and a destination.  Anything else is MX_ERR_ARG and nothing is
 * launched. */
typedef struct {
  int32_t src_slot, dst_slot, n_pos;
} mx_kv_copy;
int mx_kv_copy_probe(int device, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx, int n_copies,
                     const mx_kv_copy* copies, void* kcache, void* vcache);

/* Host-RAM tier behind the KV slots (llama-cpp-python's LlamaRAMCache(capacity_bytes)), DESIGN.md §14.  Off by
 * default (capacity 0).  On: when a request is admitted into a slot whose recorded tokens (at least 32) are held
 * to within 31 positions by nothing else -- the request's own prompt, another slot, a host entry -- the slot's
 * K/V are first packed on the device and written to pinned host memory in the background; a later prompt that
 * matches a host entry by at least 32 positions more than any device source gets those positions back by one
 * host-to-device transfer and one kernel instead of a prefill.  The entries' bytes never exceed capacity_bytes:
 * least recently used entries are evicted, an entry above the capacity is not stored.  Lowering the capacity
 * evicts at once, 0 drops every entry and switches the tier off.  Requests with prompt log-probabilities and
 * embedding requests are not restored (their slots are spilled like any other).  Takes effect at the next
 * admission; a pipeline-stage engine returns MX_ERR_STATE. */
int mx_engine_set_host_cache(mx_engine* e, uint64_t capacity_bytes);
/* entries / bytes: what the store holds now; spills / spilled_bytes: entries written to host memory;
 * restores / restored_bytes: host-to-device transfers and their bytes; restored_prompt_tokens: prompt positions
 * requests received from host entries beyond what their slot held (mx_stats.reused_prompt_tokens keeps counting
 * only those); evictions: entries dropped for the budget; skipped: records larger than the capacity. */
typedef struct {
  uint64_t entries, bytes, capacity_bytes, spills, spilled_bytes, restores, restored_prompt_tokens, restored_bytes,
      evictions, skipped;
} mx_host_cache_counts;
int mx_host_cache_stats(mx_engine* e, mx_host_cache_counts* out);
/* The pack / unpack kernels on caller-supplied caches, no engine.  kcache / vcache as for mx_kv_copy_probe.  The
 * packed form of entry i is packed[t][layer][K|V][kv head][32 * head_dim] f16, t = 0 .. P/32 - 1, P = n_pos
 * rounded up to 32, starting at 16-byte word offset16 of `packed`; one tile t is n_layer * 2 * n_head_kv * 32 *
 * head_dim * 2 bytes.  dir 0 packs: `packed` (packed_bytes + MX_KV_PACK_GUARD_BYTES bytes, output only) is filled
 * with 0xFF on the device before the launch and copied back with its guard; the caches are copied back too and
 * must come back unchanged.  dir 1 unpacks `packed` (packed_bytes bytes, input) into the caches: positions [0, P)
 * of slot `slot` change, every other byte stays.  Slots in range, 1 <= n_pos <= n_ctx, offsets a whole number of
 * tiles, every entry inside packed_bytes, no two packed ranges overlapping, (dir 1) no slot twice, packed_bytes a
 * multiple of 16 and at most 1 GiB.  Anything else is MX_ERR_ARG and nothing is launched. */
#define MX_KV_PACK_GUARD_BYTES 4096
typedef struct {
  int32_t slot, n_pos;
  uint64_t offset16;
} mx_kv_pack;
int mx_kv_pack_probe(int device, int dir, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                     int n_entries, const mx_kv_pack* entries, void* kcache, void* vcache, void* packed,
                     uint64_t packed_bytes);

/* The production bf16 matmul launchers on caller-supplied W / X, no engine (tests on shapes no model has).
 * path 0 launch_mm (M 1..64), 1 launch_mm_pers (M 1..16, shapes of mx_matmul_plan's pers_ok), 2 launch_mm_wide
 * (M 1..64), 3 launch_mm_wide with full_chain, 4 launch_gemm_split (M 65..4096 as in the engine, `target`
 * 0..256 work-groups, slab space `slab_floats` <= 2^26; act_f32 only with target 0: the split finish writes
 * bf16).  epi: 0 F32, 1 RESID, 2 QKV, 3 SWIGLU.  w: bf16 [N][K] row-major in GGUF order (N % 16,
 * K % 32; SWIGLU: rows [0, N/2) ffn_gate, [N/2, N) ffn_up), packed on the device with launch_pack as at model
 * load (packed_out, optional, receives the N*K packed bf16).  Activations: x bf16 [M][K] -- the device buffer
 * has 16 / 32 / 64 rows for M <= 16 / 32 / 64 (else M rounded up to 16), rows >= M hold bf16 NaN -- or, paths
 * 0 and 1 with M <= 4 and not RESID, RMS_NORM on load: xf f32 [M][K], norm_w f32 [K], eps (the sum-of-squares
 * partials come from launch_ssq, as for an embedded row).
 * out: [M + 64][ld] elements, filled with 0xFF bytes before the launch (rows >= M are a guard that must
 * come back as 0xFF): F32 f32, ld N; RESID f32, ld N, rows < M start as resid [M][N] and return updated (the
 * split paths 2, 3 and a split path 4 fold their partials with launch_resid_norm, as the engine does); SWIGLU
 * bf16 (act_f32: f32), ld N/2; QKV q f32, ld n_head * head_dim, with N = (n_head + 2 n_head_kv) * head_dim,
 * head_dim 64 or 128, pos[M] in [0, n_ctx], slot[M] in [0, n_slots), rope_cs [n_ctx][head_dim/2][cos, sin] and
 * the raw tiled caches as in mx_attention_probe (copied back after the launch).
 * ssq_out (RESID, paths 0 and 1, optional): the [M][N/16] sum-of-squares partials the epilogue writes.
 * slabs_out (optional, slabs_cap floats): paths 2 / 3 with QKV or RESID: the raw split-K partials [split][M][N]
 * as the launcher left them (QKV: before launch_qkv_finish runs), slabs_cap >= kgroups * M * N; path 4: the
 * whole slab space (slabs_cap >= slab_floats), 0xFF where nothing was written.  *split_out: what the launcher
 * returned.  Everything a kernel indexes with is checked before any launch (MX_ERR_ARG, nothing launched); a
 * launcher that refuses the shape gives MX_ERR_ARG with its name in mx_last_error(). */
typedef struct {
  int32_t path, epi, M, N, K;
  const void* w;
  const void* x;
  const float* xf;
  const float* norm_w;
  float eps;
  int32_t target;
  uint64_t slab_floats;
  int32_t want_ssq, act_f32;
  int32_t n_head, n_head_kv, head_dim, n_ctx, n_slots;
  const int32_t* pos;
  const int32_t* slot;
  const float* rope_cs;
  void* kcache;
  void* vcache;
  const float* resid;
  void* out;
  float* ssq_out;
  float* slabs_out;
  uint64_t slabs_cap;
  int32_t* split_out;
  void* packed_out;
  const float* bias; /* QKV, optional: f32 [N] added to each finished row sum before RoPE (q/k/v bias); NULL: none */
} mx_matmul_args;
int mx_matmul_probe(int device, const mx_matmul_args* a);
/* The dispatch facts of a bf16 matmul shape, no GPU needed: *kgroups = canon_kgroups(epi, N, K) (the K split
 * of the 17..64-row launch = the canonical K grouping), *pers_ok = mm_pers_supported(epi, M, N, K),
 * *norm_on_load_ok = mm_can_norm_on_load(M, K), *gemm_ok = gemm_supported(N, K).  Any pointer may be NULL. */
int mx_matmul_plan(int epi, int M, int N, int K, int32_t* kgroups, int32_t* pers_ok, int32_t* norm_on_load_ok,
                   int32_t* gemm_ok);
/* The production Q8_0 / Q4_0 launchers on caller-supplied operands, no engine.
 * path 0 launch_mq8 (whatever it dispatches, M 1..4096); path 1 launch_mq8_slab (17..32 rows, RESID or QKV)
 * finished as the engine finishes it: RESID slabs folded by the next launch_rmsnorm_q8 (weights fold_w [N]; out
 * receives x, nxq_out / nxd_out that norm's Q8_0 rows [M + 64][N] / [M + 64][N/32]), QKV slabs by
 * launch_qkv_finish; path -1: the activation step alone (no weights, no matmul).
 * w: raw GGUF blocks, row-major [N][K/32]: Q8_0 (34 bytes) or, wq4 = 1, Q4_0 (18 bytes); N % 16, K % 64; SWIGLU:
 * rows [0, N/2) ffn_gate, [N/2, N) ffn_up.  Packed on the device with launch_pack_q8 / launch_pack_q4 as at model
 * load (packed_out, optional, receives the packed bytes).
 * Activations (act), from f32 rows xf as the engine's quant_operand makes them: 0 launch_quantize_q8 of xf
 * [M][ldx] (ldx >= K, 0 = K); 1 launch_rmsnorm_q8 of xf [xrows][K] with norm_w [K], eps, optional row_map [M]
 * (entries in [0, xrows); without it xrows = M) or fold_slabs [nslab][xrows][K], nslab 0..8, folded into x first
 * (x_out, optional, receives the folded rows); 2 quantise on load (path 0, mq8_can_quantize_on_load(M, K, norm)):
 * xf [M][K], optional norm_w with the sum-of-squares partials from launch_ssq.  Device rows past the caller's hold
 * 0xFF bytes (f32 NaN).  xq_out [M + 64][K] (int8, in q8_perm order) and xd_out [M + 64][K/32] (optional) receive
 * the device's Q8_0 rows of acts 0 / 1, rows >= M still 0xFF.
 * out: [M + 64][ld] f32, filled with 0xFF bytes before any launch (rows >= M: a guard): F32 ld N; RESID ld N,
 * rows < M start as resid; SWIGLU ld N/2, act_f32 must be set (Q8_0 models use the f32 act; without it the
 * launcher refuses); QKV as mx_matmul_probe.  ssq_out (want_ssq: RESID, path 0): the partials, [M + 64][N/16], rows
 * >= M a guard that starts as 0xFF.
 * slabs_out (path 1, slabs_cap >= 8 * M * N floats): the raw partials [ks][M][N]; *split_out: the launcher's
 * return (ks).  Everything a kernel indexes with is checked before any launch (MX_ERR_ARG, nothing launched); a
 * launcher that refuses the shape gives MX_ERR_ARG with its name in mx_last_error(). */
typedef struct {
  int32_t path, epi, M, N, K, wq4, act;
  const void* w;
  const float* xf;
  int32_t xrows, ldx;
  const float* norm_w;
  float eps;
  const int32_t* row_map;
  const float* fold_slabs;
  int32_t nslab;
  int32_t want_ssq, act_f32;
  int32_t n_head, n_head_kv, head_dim, n_ctx, n_slots;
  const int32_t* pos;
  const int32_t* slot;
  const float* rope_cs;
  void* kcache;
  void* vcache;
  const float* resid;
  const float* fold_w;
  void* out;
  float* ssq_out;
  float* slabs_out;
  uint64_t slabs_cap;
  int32_t* split_out;
  void* packed_out;
  void* xq_out;
  float* xd_out;
  float* x_out;
  void* nxq_out;
  float* nxd_out;
  int32_t np; /* leave 0 (np = K / 16, the only value launch_mq8 accepts).  A test hook, not an operand: with act 2 and
                 norm_w, a multiple of 4 in [4, K / 16) is handed to launch_mq8 as MMArgs.np to show that it refuses
                 np * 16 != K; no kernel ever runs with it */
  const float* bias; /* QKV, optional: f32 [N] added to each finished row sum before RoPE (q/k/v bias); NULL: none */
} mx_q8_matmul_args;
int mx_q8_matmul_probe(int device, const mx_q8_matmul_args* a);
/* The kernel a Q8_0 / Q4_0 shape reaches, no GPU needed (the launchers dispatch on the same host functions).
 * kind: 0 launch_mq8 refuses, 1 mq8_kernel quantising on load (qp, qm, bd), 2 mq8_pers_ql_kernel (tpw), 3
 * mq8_kernel<ks, rt, nb> (bd: the block-diagonal one-token form; grid_y), 4 mq8_wide_kernel<w>, 5
 * mq8_wsw_kernel<w>, 6 q8gemm_kernel (grid).  slab_ks: launch_mq8_slab's split for pre-quantised rows, -1 = it
 * refuses.  can_on_load: mq8_can_quantize_on_load(M, K, norm). */
typedef struct {
  int32_t kind, qp, qm, tpw, ks, rt, nb, bd, grid_y, w, grid, slab_ks, can_on_load;
} mx_q8_plan;
int mx_q8_matmul_plan(int epi, int M, int N, int K, int wq4, int on_load, int norm, mx_q8_plan* out);
/* mode 0 launch_dequant_q8_tiles: Q8_0 blocks [N][K/32] (N % 16) packed as at load -> packed bf16 tiles, out
 * [(N + 64) * K] uint16; mode 1 launch_embed_q8: rows ids [M] (in [0, N)) of the blocks -> out f32 [M + 64][K]
 * and, optionally, ssq_out [M + 64][K/16].  Outputs start as 0xFF bytes. */
int mx_q8_side_probe(int device, int mode, int N, int K, const void* blocks, const int32_t* ids, int M, void* out,
                     float* ssq_out);
/* The production K-quant (Q4_K 12, Q5_K 13, Q6_K 14) launchers on caller-supplied operands, no engine.
 * path 0 launch_mkq (whatever it dispatches, M 1..4096); path 1 launch_mkq_slab (17..32 rows, RESID) finished as
 * the engine finishes it: the slabs folded by the next launch_rmsnorm_q8k (weights fold_w [N]; out receives the
 * folded x, nxq_out / nxd_out / nxb_out that norm's Q8_K rows [M + 64][N], [N/256], [N/32]; N > 4096, where that
 * fold has no form: launch_resid_norm folds and no rows are made); path 2 launch_mkq_qkv_slab (17..32 rows, QKV)
 * finished by launch_qkv_finish; path -1: the activation step alone (no weights, no matmul).
 * w: raw GGUF blocks of kq_n (1..3) row segments laid end to end: segment i holds rows [16 kq_tile_end[i-1],
 * 16 kq_tile_end[i]) as [rows][K/256] blocks of kq_type[i] (144 / 176 / 210 bytes), kq_tile_end strictly
 * increasing, the last 16 * it = N; K % 256.  Each segment is packed on the device with launch_pack_kq at its own
 * byte offset, as at model load (packed_out, optional, receives the packed bytes).  SWIGLU: one segment, rows
 * [0, N/2) ffn_gate (PACK_GATE), [N/2, N) ffn_up (PACK_UP), N % 32.
 * Activations (act), from f32 rows xf as the engine's quant_operand makes them: 0 launch_quantize_q8k of xf
 * [M][ldx] (ldx >= K, 0 = K); 1 launch_rmsnorm_q8k of xf [xrows][K] with norm_w [K], eps and optional row_map [M]
 * (entries in [0, xrows); without it xrows = M); 2 one token quantised on load (path 0, M 1,
 * mkq_can_quantize_on_load(1, K, norm)): xf [K], optional norm_w with the sum-of-squares partials ssq_in [K/16]
 * (NULL: launch_ssq makes them).  Device rows past the caller's hold 0xFF bytes (f32 NaN).  xq_out [M + 64][K]
 * (int8, permuted within each super-block), xd_out [M + 64][K/256], xb_out [M + 64][K/32] (optional) receive the
 * device's Q8_K rows of acts 0 / 1, rows >= M still 0xFF.
 * out: [M + 64][ld] f32, filled with 0xFF bytes before any launch (rows >= M: a guard): F32 ld N; RESID ld N, rows
 * < M start as resid; SWIGLU ld N/2 (the f32 act); QKV as mx_matmul_probe (K need not equal n_head * head_dim).
 * ssq_out (want_ssq: RESID, path 0, not with norm on load: MMArgs has one ssq pointer): the partials
 * [M + 64][N/16], rows >= M a guard.  slabs_out (paths 1 / 2, slabs_cap >= 8 * M * N floats): the raw partials
 * [ks][M][N] as the launcher left them (the device buffer holds exactly the ks slabs of mkq_slab_ks /
 * mkq_qkv_slab_ks, which the launcher dispatches on); *split_out: the launcher's return (ks).
 * Everything a kernel indexes with is checked before any launch (MX_ERR_ARG, nothing launched).  A matmul launcher
 * that refuses the shape gives MX_ERR_ARG with its name in mx_last_error(): it launched nothing itself, but the
 * packer and the activation step before it have run. */
typedef struct {
  int32_t path, epi, M, N, K, act;
  int32_t kq_n;
  int32_t kq_type[3], kq_tile_end[3];
  const void* w;
  const float* xf;
  int32_t xrows, ldx;
  const float* norm_w;
  float eps;
  const int32_t* row_map;
  const float* ssq_in;
  int32_t want_ssq;
  int32_t n_head, n_head_kv, head_dim, n_ctx, n_slots;
  const int32_t* pos;
  const int32_t* slot;
  const float* rope_cs;
  void* kcache;
  void* vcache;
  const float* resid;
  const float* fold_w;
  void* out;
  float* ssq_out;
  float* slabs_out;
  uint64_t slabs_cap;
  int32_t* split_out;
  void* packed_out;
  void* xq_out;
  float* xd_out;
  float* xb_out;
  void* nxq_out;
  float* nxd_out;
  float* nxb_out;
  const float* bias; /* QKV, optional: f32 [N] added to each finished row sum before RoPE (q/k/v bias); NULL: none */
} mx_kq_matmul_args;
int mx_kq_matmul_probe(int device, const mx_kq_matmul_args* a);
/* The kernel a K-quant shape reaches, no GPU needed: mkq_plan, the function launch_mkq and its sub-launchers
 * dispatch on.  on_load / norm: one token quantised on load, with RMS_NORM; the row segments as in
 * mx_kq_matmul_args.  flags: -1 = this process's MX_NO_KQ_* switches, else bit 0 MX_NO_KQ_BD_TILE, bit 1
 * MX_NO_KQ_PERS, bit 2 MX_NO_KQ_WIDE as if set (the split target stays the process's).
 * kind: 0 launch_mkq refuses, 1 qkv_pers (mkq_pers_seg_kernel<ks, nkw, tpw, QKV, u>), 2 bd_tile
 * (mkq_bd_tile_kernel<t, w, nkw = K/256, tpw, epi, u>), 3 pers (mkq_pers_kernel<t, ks, nkw, tpw, nb, epi, u, ql,
 * bd>), 4 wide (mkq_wide_kernel<t, w, nb, epi, u>), 5 mkq (mkq_kernel<ks, 1, nb, epi, u, ql, bd>); t 0: the type is
 * chosen per work-group; grid_x, grid_y: the launch grid.  slab_ks / qkv_slab_ks: what launch_mkq_slab /
 * launch_mkq_qkv_slab return for pre-quantised rows of this shape (-1: refused).  can_on_load:
 * mkq_can_quantize_on_load(M, K, norm). */
typedef struct {
  int32_t kind, t, ks, nkw, tpw, nb, u, bd, ql, w, grid_x, grid_y, slab_ks, qkv_slab_ks, can_on_load;
} mx_kq_plan;
int mx_kq_matmul_plan(int epi, int M, int N, int K, int on_load, int norm, int kq_n, const int32_t* kq_type,
                      const int32_t* kq_tile_end, int flags, mx_kq_plan* out);
/* The K-quant side kernels alone, no engine; K % 256.  Outputs start as 0xFF bytes; a launcher that refuses gives
 * MX_ERR_ARG and nothing is launched.
 * mode 0 launch_pack_kq: blocks [N][K/256] of `type` (N % 16) into a matrix of N + offset rows with PACK_ROWS
 *   (pack 0, offset % 16 == 0) or of 2 N rows with PACK_GATE / PACK_UP (pack 1 / 2) -> out: that matrix's packed
 *   bytes (kq_matrix_bytes) then 64 tiles of guard.
 * mode 1 launch_dequant_kq: blocks in row segments (kq_n, kq_type, kq_tile_end as in mx_kq_matmul_args), each
 *   packed with launch_pack_kq -> out uint16 [(N + 64) * K] packed bf16 tiles (kernels.h layout).
 * mode 2 launch_embed_kq: rows ids [M] (in [0, N)) of blocks [N][K/256] of `type` -> out f32 [M + 64][K], ssq_out
 *   (optional) [M + 64][K/16].
 * mode 3 launch_quantize_q8k of x f32 [M][ld] (ld >= K, 0 = K; rows = M); mode 4 launch_rmsnorm_q8k of x [rows][K]
 *   with w [K], eps, optional row_map [M] (entries in [0, rows); without it M = rows) and slabs [nslab][rows][K],
 *   nslab 0..8, folded into x first -> xq_out [M + 64][K] int8, xd_out [M + 64][K/256], xb_out [M + 64][K/32], and
 *   x_out (optional) [rows + 64][ld]: the device's x after the launch. */
typedef struct {
  int32_t mode, type, N, K;
  const void* blocks;
  int32_t pack, offset;
  int32_t kq_n;
  int32_t kq_type[3], kq_tile_end[3];
  const int32_t* ids;
  int32_t M, rows, ld;
  const float* x;
  const float* w;
  const int32_t* row_map;
  float eps;
  const float* slabs;
  int32_t nslab;
  void* out;
  float* ssq_out;
  void* xq_out;
  float* xd_out;
  float* xb_out;
  float* x_out;
} mx_kq_side_args;
int mx_kq_side_probe(int device, const mx_kq_side_args* a);

/* The dequantise-at-load, residual-stream boundary and greedy-pick launchers alone, no engine.  Every output starts
 * as 0xFF bytes, carries a guard behind it (64 rows for row-shaped outputs, 4096 elements for flat ones) and returns
 * whole.  Arguments a launcher would mishandle give MX_ERR_ARG and nothing is launched.
 * mode 0 launch_dequant_bf16: src = src_bytes bytes of raw GGUF blocks of ggml `type`, count elements -> out uint16
 *   [count + 4096].  An unsupported type, or a count that is no multiple of the type's block, is handed to the
 *   launcher, and its refusal is reported (MX_ERR_ARG, "launch_dequant_bf16 refused" in mx_last_error()).
 * mode 1 launch_embed: src bf16 [N][n], ids [M] in [0, N) -> out f32 [M + 64][n]; ssq_out (optional) [M + 64][n/16],
 *   handed to the launcher only when want_ssq is set (otherwise it returns all 0xFF).
 * mode 2 launch_ssq: src f32 [M][n] -> ssq_out [M + 64][n/16].
 * mode 3 launch_f32_in: src f32 [M][n] -> out and ssq_out as mode 1.   mode 4 launch_bf16_to_f32: src bf16 [M][n].
 *   Modes 1..4: n a multiple of 64 (<= 16384), 1 <= M <= 4096.
 * mode 5 launch_f32_to_bf16: src f32 [count] -> out uint16 [count + 4096]; mode 6 launch_copy_f32: -> out f32
 *   [count + 4096]; count a multiple of 4.
 * mode 7 launch_argmax: src = logits f32 [M][ldl], 1 <= V <= ldl; state in: pos [M], hist_count [M] (>= 0),
 *   hist_stride, max_hist <= hist_stride; null_mask: bit 0 tok_out, 1 ids_next, 2 pos_next, 3 hist are handed to the
 *   launcher as NULL (their buffers then return as they were filled) -> tok_out, ids_next_out, pos_next_out (rows < M
 *   start as pos), hist_count_out (rows < M start as hist_count), each int32 [M + 4096], and hist_out int32
 *   [M + 64][hist_stride]. */
typedef struct {
  int32_t mode, type;
  uint64_t count, src_bytes;
  int32_t M, N, n, want_ssq;
  const void* src;
  const int32_t* ids;
  void* out;
  float* ssq_out;
  int32_t V, ldl, hist_stride, max_hist, null_mask;
  const int32_t* pos;
  const int32_t* hist_count;
  int32_t* tok_out;
  int32_t* ids_next_out;
  int32_t* pos_next_out;
  int32_t* hist_out;
  int32_t* hist_count_out;
} mx_glue_args;
int mx_glue_probe(int device, const mx_glue_args* a);

/* launch_resid_norm (row_map NULL) / launch_rmsnorm (row_map given, nslab 0) on caller-supplied rows, no
 * engine.  x f32 [rows][n] (n % 64, n <= 16384, rows 1..4096); slabs [nslab][rows][n] (0 <= nslab <= 16) are
 * folded into x in slab order; w f32 [n] (optional): y = bf16(rmsnorm(x, eps) * w) [M][n]; row_map [M] (entries
 * in [0, rows)): y row i is made from x row row_map[i]; without it M = rows.  x_out [rows + 64][n] and y_out
 * [M + 64][n] start as 0xFF bytes (x_out rows < rows as x) and return whole.  Anything else: MX_ERR_ARG. */
int mx_norm_probe(int device, int rows, int n, int M, const float* x, const float* slabs, int nslab, const float* w,
                  const int32_t* row_map, float eps, float* x_out, void* y_out);

/* Device-resident decode batch (benchmark, pipeline stages).  Rows are M
 * sequences in KV slots `slots`, next token ids[i] at position pos[i].
 * mx_batch_step runs one decode step on `stream` (NULL = engine stream):
 *   x_in  == NULL -> embed ids (stage 0), else f32 [M][n_embd] device input
 *   x_out == NULL -> final norm + lm_head + greedy argmax (last stage), tokens
 *                    written back to the batch's ids and history;
 *                    else f32 [M][n_embd] device output for the next stage.
 * Each stage advances its own positions. */
int mx_batch_create(mx_engine* e, int M, const int32_t* slots, const int32_t* pos, const int32_t* ids, int max_steps,
                    mx_batch** out);
int mx_batch_step(mx_engine* e, mx_batch* b, const void* x_in, void* x_out, void* stream);
/* Device pointer of the batch's next-token ids (int32[M]) -- the pipeline's
 * last stage sends these to stage 0, which receives into the same buffer. */
int32_t* mx_batch_ids_device(mx_batch* b);
/* Make the batch read/write its next-token ids in a caller-owned device buffer
 * (int32[M], e.g. a torch tensor that RCCL receives into); current ids are copied over. */
int mx_batch_bind_ids(mx_engine* e, mx_batch* b, int32_t* ids_device);
int mx_batch_tokens(mx_engine* e, mx_batch* b, int32_t* out, int cap, int* n_steps);
/* Re-arm a batch for its next run without re-capturing its graphs (pipeline lanes): positions of all
 * M rows, next ids (NULL: keep the device ids), per-row samplers (NULL: greedy argmax over the last
 * stage's logits), token history restarted; the copies are ordered on `stream` (NULL: engine stream). */
int mx_batch_reset(mx_engine* e, mx_batch* b, const int32_t* pos, const int32_t* ids, const mx_row_sampler* rows,
                   void* stream);
void mx_batch_destroy(mx_engine* e, mx_batch* b);

/* Stage forward of arbitrary rows (pipelined prefill): like mx_forward_rows but
 * with device x_in / x_out as in mx_batch_step; logits_out (host) only on the last stage. */
int mx_stage_rows(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                  const void* x_in, void* x_out, float* logits_out, void* stream);
/* Pipelined prefill of n rows (any count: GEMM chunks as mx_forward_rows; x_in / x_out device
 * [n][n_embd] in the hand-off dtype).  On the last stage, rows rowmap[0..n_out) (increasing) each pick
 * a token -- the device sampling chain with samp[i], or greedy argmax when samp is NULL -- copied to
 * tok_out (host int32[n_out]); the first token of each prompt in the pipeline server.
 * Rows need no padding: a call with more than 64 picks whose rows fall in one chunk is cut into
 * forwards of at most 64 picks each, after the 64th pick's 16-row block (where padded prompts end) but
 * never past the next picked row, so every rowmap entry is produced by the forward that holds its row.  A prompt the cut
 * divides keeps its result: its later rows attend to the K/V its earlier rows stored. */
int mx_stage_rows_pick(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                       const void* x_in, void* x_out, int n_out, const int32_t* rowmap, const mx_row_sampler* samp,
                       int32_t* tok_out, void* stream);

/* Time `iters` passes of one layer-kernel kind over this stage's layers with
 * HIP events on the engine stream (benchmark roofline); kind: 0 qkv, 1 attn_output,
 * 2 ffn_gate_up, 3 ffn_down, 4 lm_head, 5 qkv with fused RMSNorm, 6 ffn_gate_up with fused
 * RMSNorm (M <= 8), 7 attention (positions = env MX_PROF_POS).  Returns mean microseconds per launch. */
/* Diagnosis: op 0 sets the number of launches after which an eager 17..64-row forward stops (-1:
 * never; the forward then returns MX_DEBUG_STOPPED, never 0), op 1 synchronises the stream after every
 * such launch (arg != 0); neither acts on a forward being captured into a graph (graph replays run
 * whole).  Op 2 copies internal buffer `arg`
 * (0 x, 1 q, 2 xn, 3 attn_out, 4 act, 5 split-K slabs, 6 K cache, 7 V cache, 8 ssq partials, 9 row
 * positions, 10 row slots, 11 RoPE table) to
 * `host`, at most `bytes`.  MX_POISON=1 at creation fills every allocation with 0xFF bytes. */
int mx_debug(mx_engine* e, int op, long long arg, void* host, size_t bytes);
int mx_profile_kernel(mx_engine* e, int kind, int M, int iters, double* us_per_launch, double* bytes_per_launch);

int mx_sync(mx_engine* e);

/* HBM streaming probes on `device` (no engine): the best of a sweep of 16-byte-per-lane streaming
 * kernels (loads in flight per lane x grid x non-temporal) over `bytes`-sized buffers, `iters`
 * passes each timed with HIP events.  copy: *gbs = (read + write) bytes / s; read: bytes read / s.
 * desc (optional) receives the winning variant.  Benchmark support (SURVEY.md §8d "also report a
 * measured copy-kernel peak"), not a reference API. */
int mx_probe_copy(int device, size_t bytes, int iters, double* gbs, char* desc, int desc_len);
int mx_probe_read(int device, size_t bytes, int iters, double* gbs, char* desc, int desc_len);

/* Request-path counters (mx_submit/mx_wait).  reused_prompt_tokens: prompt positions whose K/V were
 * kept from the slot's previous request (longest common prefix, as llama-cpp-python's generate). */
typedef struct {
  uint64_t prompt_tokens, reused_prompt_tokens, generated_tokens;
} mx_stats;
int mx_engine_stats(mx_engine* e, mx_stats* out);

/* Number of visible HIP devices (serving: one engine replica per GPU). */
int mx_device_count(int32_t* n);

/* Grammar-constrained sampling (llama-cpp-python's create_completion(grammar=LlamaGrammar)).
 * The matcher runs on the host; a request's allowed tokens reach the device as a bit mask, and a kernel sets the
 * logit of every other token to -inf before the request's sampler reads the row.
 *
 * mx_vocab: what a grammar is matched against -- the piece bytes of the n_vocab tokens (token t: blob[offsets[t],
 * offsets[t + 1]), offsets[0] == 0, at most 4096 bytes each; an empty piece is never allowed) and the
 * end-of-generation ids (allowed exactly where the grammar may end).  Copied; MX_ERR_ARG for anything malformed.
 * mx_grammar: a compiled GBNF grammar over one vocabulary, immutable and shared by any number of requests and
 * states.  Syntax errors, undefined rules, a missing root, {m,n} with n < m and left-recursive rules are MX_ERR_ARG
 * with the rule or position in mx_last_error().  cache_entries: masks kept per grammar, least recently used out
 * first (< 0: the default of 256; 0: none).  Both handles are reference-counted: destroying one while a grammar,
 * a state or a request still uses it is safe.  No GPU touched. */
typedef struct mx_vocab mx_vocab;
typedef struct mx_grammar mx_grammar;
typedef struct mx_grammar_state mx_grammar_state;
int mx_vocab_create(int n_vocab, const uint8_t* blob, const uint64_t* offsets, const int32_t* eog_ids, int n_eog,
                    mx_vocab** out);
void mx_vocab_destroy(mx_vocab* v);
int mx_grammar_create(const mx_vocab* v, const char* gbnf, int cache_entries, mx_grammar** out);
void mx_grammar_destroy(mx_grammar* g);
/* A state outside any engine (what a request holds; CPU probing): starts at root.  mask: the allowed tokens as
 * n_words = ceil(n_vocab / 32) words, bit t & 31 of word t >> 5; *status MX_GRAMMAR_OK, MX_GRAMMAR_DEAD_END (no
 * token is allowed) or MX_GRAMMAR_CAP (more than 4096 simultaneous grammar positions), the words all zero for the
 * last two.  accept: MX_ERR_ARG when the token is not allowed (the state is unchanged).  may_end: the grammar can
 * end here (and no UTF-8 sequence is open). */
#define MX_GRAMMAR_OK 0
#define MX_GRAMMAR_DEAD_END 1
#define MX_GRAMMAR_CAP 2
int mx_grammar_state_create(const mx_grammar* g, mx_grammar_state** out);
int mx_grammar_state_mask(mx_grammar_state* s, uint32_t* words, int n_words, int32_t* status);
int mx_grammar_state_accept(mx_grammar_state* s, int32_t token);
int mx_grammar_state_may_end(const mx_grammar_state* s, int32_t* may_end);
void mx_grammar_state_destroy(mx_grammar_state* s);
/* mask lookups of the grammar served from its cache / computed by a walk of the vocabulary, and the masks held */
int mx_grammar_cache_stats(const mx_grammar* g, uint64_t* hits, uint64_t* misses, uint64_t* entries);
/* As mx_submit_ext (s NULL: the defaults) with a grammar.  Generated tokens advance it from root (prompt tokens do
 * not); every pick -- argmax, chain, wide, Mirostat, host sampler -- runs on the masked row; log-probabilities
 * stay those of the raw row.  An end-of-generation token ends the request with MX_FINISH_STOP.  A step at which no
 * token is allowed, or whose state is over the position cap, ends it with MX_FINISH_ERROR (mx_wait: MX_ERR_STATE)
 * and leaves the other requests alone.  A round with a grammar row runs one step; such a request never
 * speculates.  MX_ERR_ARG when the grammar's vocabulary is not of the engine's size, MX_ERR_STATE on a
 * pipeline-stage engine. */
int mx_submit_grammar(mx_engine* e, const int32_t* ids, int n, const mx_sampling_ext* s, int max_tokens,
                      int n_logprobs, int prompt_logprobs, const mx_grammar* grammar, uint64_t* req);
/* The mask kernel on caller-supplied rows, no engine: logits_host [n][ldl] f32 with V <= ldl valid columns,
 * n <= 64; masks [n][ceil(V / 32)]; on [n] (0: the row is left alone).  out [n][ldl]: where(on && bit clear,
 * -inf, x) in columns < V, columns >= V bit-identical.  Anything else: MX_ERR_ARG, nothing launched. */
int mx_grammar_mask_probe(int device, const float* logits_host, int n, int V, int ldl, const uint32_t* masks,
                          const uint32_t* on, float* out);
/* The same launch timed: masks [n][ceil(V / 32)] on resident buffers (rows of zeros, every row on), 3 warm-up
 * launches, then `iters` launches between two HIP events; *us_per_launch their mean.  Benchmark support. */
int mx_grammar_mask_time(int device, int n, int V, int ldl, const uint32_t* masks, int iters, double* us_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* MX_ENGINE_H */
