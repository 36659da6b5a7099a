// engine.cpp -- host side of the MI355X-native engine behind include/mx_engine.h.
//
// Replaces llama-cpp-python/llama.cpp as used by the reference node:
//   Llama(model_path=...)                 /root/reference/llama_p2p_network.py:19  -> mx_engine_create
//   self.model(prompt, max_tokens=100)    /root/reference/llama_p2p_network.py:125 -> mx_submit/mx_wait
// The forward pass is llama.cpp's llm_build_llama expressed as
// five fused gfx950 kernels per layer (kernels.hip).  Decode steps are captured
// once per batch shape as hipGraphs and replayed; a scheduler thread replaces
// the reference's serialising lock (p2p:121) with micro-batched decode of all
// active requests.
// This file holds the engine only: every function of the C API that takes an mx_engine.  The stand-alone
// kernel probes (mx_*_probe, mx_*_plan: an `int device`, no engine) are in probes.cpp; what the two files
// share is declared in engine_shared.h and defined here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "engine_shared.h"
#include "grammar.h"
#include "gguf.h"

using namespace mx;

namespace {
thread_local std::string g_err;  // the one error string of the library: probes.cpp reports through fail() too
}  // namespace

int mx::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// the tail of one embedding chunk (engine_shared.h)
int mx::embd_tail(const float* x, const float* w, float eps, int n, const std::vector<EmbdSeg>& segs, int pooling,
                  bool normalize, float* ybuf, float* acc, float* pooled, int* d_tab, size_t tab_ints,
                  std::vector<int32_t>& tab, hipStream_t s) {
  std::vector<int32_t> src, dst, l2, sg;
  int k = 0;
  for (const EmbdSeg& g : segs) {
    const bool last = g.done + g.rows == g.T;
    if (pooling == MX_POOL_NONE) {
      for (int j = 0; j < g.rows; j++) src.push_back(g.row0 + j), dst.push_back(g.dst0 + j), l2.push_back(g.dst0 + j);
    } else if (pooling == MX_POOL_MEAN) {
      for (int j = 0; j < g.rows; j++) src.push_back(g.row0 + j), dst.push_back(k + j);
      const int32_t e[EMBD_SEG] = {k, g.rows, g.seq, g.dst0, g.done == 0, last ? g.T : 0};
      sg.insert(sg.end(), e, e + EMBD_SEG);
      if (last) l2.push_back(g.dst0);
      k += g.rows;
    } else if (pooling == MX_POOL_CLS ? g.done == 0 : last) {
      src.push_back(pooling == MX_POOL_CLS ? g.row0 : g.row0 + g.rows - 1);
      dst.push_back(g.dst0);
      l2.push_back(g.dst0);
    }
  }
  const size_t ns = src.size(), nl = l2.size(), nseg = sg.size() / EMBD_SEG;
  if (ns == 0) return 0;  // CLS / LAST: no sequence starts / ends in this chunk
  tab.assign(src.begin(), src.end());
  tab.insert(tab.end(), dst.begin(), dst.end());
  tab.insert(tab.end(), l2.begin(), l2.end());
  tab.insert(tab.end(), sg.begin(), sg.end());
  if (tab.size() > tab_ints) return fail(MX_ERR_ARG, "embedding tail: too many rows for the index tables");
  HIPC(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
  const bool rows_to_ybuf = pooling == MX_POOL_NONE || pooling == MX_POOL_MEAN;
  if (launch_embd_norm(rows_to_ybuf ? ybuf : pooled, x, w, d_tab, d_tab + ns, (int)ns, n, eps, s))
    return fail(MX_ERR_ARG, "embedding norm launch shape");
  if (pooling == MX_POOL_MEAN && launch_embd_mean(ybuf, d_tab + 2 * ns + nl, (int)nseg, n, acc, pooled, s))
    return fail(MX_ERR_ARG, "embedding mean launch shape");
  if (normalize && nl &&
      launch_embd_l2(pooling == MX_POOL_NONE ? ybuf : pooled, d_tab + 2 * ns, (int)nl, n, s))
    return fail(MX_ERR_ARG, "embedding L2 launch shape");
  HIPC(hipGetLastError());
  return 0;
}

bool mx::blocked_rows(const int32_t* slots, const int32_t* pos, const int32_t* ids, int m) {
  for (int k = 0; k < m; k++) {
    if (k % 16 == 0) continue;
    if (slots[k] != slots[k - 1]) return false;
    if (pos[k] == pos[k - 1] + 1) continue;
    if (pos[k] != pos[k - 1] || (ids && ids[k] != ids[k - 1])) return false;
  }
  return true;
}

namespace {
struct Shape {
  const char* name;
  int n_embd, n_layer, n_head, n_head_kv, n_ff, n_vocab;
  float rope_base, eps;
  int n_ctx_train;
};
// keep in sync with llama-p2p_amd/synth.py SHAPES
const Shape kShapes[] = {
    {"tinyllama-1.1b", 2048, 22, 32, 4, 5632, 32000, 10000.f, 1e-5f, 2048},
    {"llama3-8b", 4096, 32, 32, 8, 14336, 128256, 500000.f, 1e-5f, 8192},
    {"llama3-70b", 8192, 80, 64, 8, 28672, 128256, 500000.f, 1e-5f, 8192},
    {"test-tiny", 256, 2, 4, 2, 512, 512, 10000.f, 1e-5f, 2048},
    {"test-gqa8", 512, 3, 8, 1, 1024, 1024, 500000.f, 1e-5f, 2048},
    {"test-d128", 1024, 2, 8, 2, 2816, 2048, 500000.f, 1e-5f, 2048},
    {"test-h4096", 4096, 1, 32, 8, 2048, 1024, 500000.f, 1e-5f, 2048},
    {"test-h8192", 8192, 1, 64, 8, 2048, 1024, 500000.f, 1e-5f, 2048},
    {"test-8b-ffn", 4096, 2, 32, 8, 14336, 1024, 500000.f, 1e-5f, 2048},
    {"test-70b-ffn", 8192, 1, 64, 8, 28672, 1024, 500000.f, 1e-5f, 2048},
    {"test-tiny-ffn", 2048, 1, 32, 4, 5632, 32000, 10000.f, 1e-5f, 2048},
    {"test-8b-v128k", 4096, 2, 32, 8, 14336, 128256, 500000.f, 1e-5f, 8192},
    // a non-Llama-3 geometry (Llama-2-7B: MHA, ff 11008, V 32000): the generic GEMV fallbacks' cost
    {"llama2-7b", 4096, 32, 32, 32, 11008, 32000, 10000.f, 1e-5f, 4096},
};

// decode steps the scheduler runs on the device between host syncs when every active row is greedy
constexpr int SCHED_KMAX = 8;

// synth.py tensor ids
constexpr uint64_t TID_TOK_EMBD = 1, TID_OUT_NORM = 2, TID_OUTPUT = 3;
enum { L_ATTN_NORM, L_Q, L_K, L_V, L_O, L_FFN_NORM, L_GATE, L_UP, L_DOWN };
uint64_t layer_tid(int l, int k) { return 16u + 16u * (uint64_t)l + (uint64_t)k; }
float std_scale(double std) { return (float)(std / sqrt(4294967295.0 / 3.0)); }

// Row segments of one packed K-quant matrix (MMArgs kq_*): rows appended in order, consecutive rows
// of one ggml type share a segment (q|k Q4_K + v Q6_K = two segments).
struct KqMat {
  int n = 0;
  int type[3] = {0, 0, 0}, tile_end[3] = {0, 0, 0};
  size_t off[3] = {0, 0, 0};
  size_t bytes = 0;
  int rows = 0;
  bool add(int t, int r, int K) {
    if (n && type[n - 1] == t) {
      tile_end[n - 1] += r / 16;
    } else {
      if (n == 3) return false;
      type[n] = t;
      off[n] = bytes;
      tile_end[n] = (n ? tile_end[n - 1] : 0) + r / 16;
      n++;
    }
    bytes += kq_matrix_bytes(t, r, K);
    rows += r;
    return true;
  }
  // segment holding packed row `row`, and that row's index within the segment
  int seg(int row, int* row_in_seg) const {
    int i = 0;
    while (i < n - 1 && row / 16 >= tile_end[i]) i++;
    *row_in_seg = row - 16 * (i ? tile_end[i - 1] : 0);
    return i;
  }
  void set(MMArgs& a) const {
    a.kq_n = n;
    for (int i = 0; i < 3; i++) {
      a.kq_type[i] = type[i];
      a.kq_tile_end[i] = tile_end[i];
      a.kq_off[i] = off[i];
    }
  }
};

// ggml type of a tensor in llama.cpp's Q4_K_M / Q5_K_M recipes (llama_tensor_get_type, Oct 2024;
// synth.py kq_tensor_type is the same rule): output Q6_K; attn_v and ffn_down Q6_K on the
// use_more_bits layers; attn_v of an 80-layer (70B) Q4_K_M model otherwise Q5_K; the rest `base`.
bool use_more_bits(int i, int n) { return i < n / 8 || i >= 7 * n / 8 || (i - n / 8) % 3 == 2; }
int kq_recipe_type(int base, int kind, int layer, int n_layer) {  // kind: L_* or -1 output, -2 token_embd
  if (kind == -1) return 14;
  if ((kind == 3 || kind == 8) && use_more_bits(layer, n_layer)) return 14;  // L_V, L_DOWN
  if (kind == 3 && n_layer == 80 && base == 12) return 13;
  return base;
}

struct Layer {
  uint16_t *qkv = nullptr, *o = nullptr, *gu = nullptr, *down = nullptr;
  float *attn_norm = nullptr, *ffn_norm = nullptr;
  float* qkv_bias = nullptr;  // f32 [n_embd + 2 n_embd_kv] in the packed QKV row order, or nullptr
  KqMat kq_qkv, kq_o, kq_gu, kq_down;  // K-quant model: segments of the four packed matrices
};

struct Request {
  uint64_t id = 0;
  std::vector<int32_t> prompt;
  mx_sampling samp{};
  int max_tokens = 0;
  std::vector<int32_t> out;
  int finish = -1;
  bool done = false;
  bool cancel = false;  // mx_cancel: finish after the current step
  int slot = -1;
  int pos = 0;     // next position to write
  int reuse = 0;   // leading prompt positions whose K/V the slot already holds (prefix reuse)
  int32_t next_tok = 0;
  uint64_t seed = 0;  // sampler stream: the n-th sampled token draws samp_u01(seed, n) (kernels.h)
  std::string error;
  // per-token log-probabilities (mx_submit_lp): lp_k top entries per token (-1 = off), lp_prompt: also one
  // entry per prompt position >= 1.  Entries are appended under mu together with `out`, the prompt's first.
  int lp_k = -1;
  bool lp_prompt = false;
  int lp_n_prompt = 0;         // prompt entries held (0 or prompt.size() - 1)
  std::vector<float> lp_tok;   // [entries] log-prob of the token itself
  std::vector<float> lp_top;   // [entries][lp_k]
  std::vector<int32_t> lp_idx; // [entries][lp_k]
  // prompt-lookup speculation (mx_submit_spec): num_pred_tokens (0 = not asked for) and max_ngram_size; the
  // counters cover the speculating steps whose tokens the request kept
  int spec_d = 0, spec_ng = 0;
  uint64_t spec_steps = 0, spec_drafted = 0, spec_accepted = 0;
  // embedding request (mx_submit_embed): no tokens -- its prefill pass leaves embd_rows vectors of
  // n_embd floats in embd_out (one per prompt token for MX_POOL_NONE, else one) and finishes it
  bool embd = false, embd_l2 = false;
  int embd_pool = 0, embd_rows = 0;
  std::vector<float> embd_out;
  // the rest of the sampler chain (mx_submit_ext): has_ext when any setting is off its default;
  // ext.miro is 2 only for a sampling request (temperature > 0); mu: the Mirostat state, 2 tau at submission
  bool has_ext = false;
  SampExt ext{};
  float mu = 0.f;
  // grammar (mx_submit_grammar): the request's place in its grammar, the mask of the step about to
  // be picked, and how the grammar ended the request during a prefill (0: it did not; MX_FINISH_STOP + 1 /
  // MX_FINISH_ERROR + 1, applied by the scheduler loop once the slot's record is written)
  std::unique_ptr<gram::State> gram;
  std::shared_ptr<const std::vector<uint32_t>> gram_mask;
  int gram_end = 0;
  // one entry [tok_lp | kr top log-probs | kr top ids as int bits] of a round that ran with kr >= lp_k
  void lp_append(const float* entry, int kr) {
    lp_tok.push_back(entry[0]);
    lp_top.insert(lp_top.end(), entry + 1, entry + 1 + lp_k);
    const int32_t* ip = reinterpret_cast<const int32_t*>(entry) + 1 + kr;
    lp_idx.insert(lp_idx.end(), ip, ip + lp_k);
  }
};

// the sampler path of a request's rows (mx_sample_plan's rules over its settings) and the candidates it asks for
int req_path(const Request* r, int V, int* k_eff);

struct GraphKey {
  int M;
  const void* xin;
  void* xout;
  hipStream_t stream;
  int ktop;  // 0: greedy argmax tail; k: the device sampling chain with top-k k
  bool operator<(const GraphKey& o) const {
    if (M != o.M) return M < o.M;
    if (xin != o.xin) return xin < o.xin;
    if (xout != o.xout) return xout < o.xout;
    if (ktop != o.ktop) return ktop < o.ktop;
    return stream < o.stream;
  }
};

// Where a pick's tokens go besides d_tok: the next step's ids / positions and a per-row history (the device
// loops).  All-zero: tokens to d_tok only.
struct PickOut {
  int *ids_next, *pos_next, *hist;
  int hist_stride;
  int* hist_count;
  int max_hist;
};

// One forward of M rows through this stage's layers (mx_engine::enqueue_forward).  ids or x_in feed it; x_out
// takes the residual stream for the next stage; head: logits of n_out rows (the rowmap's, or all M), and with
// argmax their picks.  Call sites name what they set; the rest is zero.
struct Forward {
  int M;
  const int *ids, *pos, *slot;
  const void* x_in;
  void* x_out;
  bool head;
  const int* rowmap;
  int n_out;
  bool argmax;
  PickOut out;
};
}  // namespace

struct mx_batch {
  int M = 0, max_steps = 0;
  SampRow* d_samp = nullptr;  // per-row device sampler settings (mx_batch_reset); null: greedy argmax
  int ktop = 0;               // top-k of the device sampling chain, 0 = greedy argmax
  bool distinct = false;  // every row its own slot (decode); see mx_engine::rows_distinct
  int max_pos = 0;  // host mirror of the largest position, so steps never run past n_ctx
  int *d_ids = nullptr, *d_pos = nullptr, *d_slot = nullptr, *d_hist = nullptr, *d_hist_count = nullptr;
  bool ids_external = false;
  std::map<GraphKey, hipGraphExec_t> graphs;
};

struct mx_engine {
  // hyper-parameters
  int n_embd = 0, n_layer = 0, n_head = 0, n_head_kv = 0, head_dim = 0, n_embd_kv = 0, n_ff = 0, n_vocab = 0;
  int n_ctx_train = 0;
  float eps = 1e-5f, rope_base = 10000.f;
  // RoPE frequency factors (GGUF rope_freqs.weight, Llama-3.1; empty = none) and linear scaling
  std::vector<float> rope_ff;
  float rope_freq_scale = 1.0f;
  int bos = 1, eos = 2;
  int eot = -1;  // tokenizer.ggml.eot_token_id (end of turn): ends a request as eos does; -1 when the file has none
  bool is_eog(int32_t t) const { return t == eos || (eot >= 0 && t == eot); }  // llama.cpp llama_token_is_eog
  int n_ctx = 512, n_seq_max = 64, lb = 0, le = 0, device = 0;
  bool has_embed = true, has_head = true, use_graphs = true;
  // <= 4 rows: RMS_NORM applied while loading the GEMV's B operand, from per-tile sums of squares
  // written by the residual-stream producer (no norm launches)
  static constexpr bool norm_on_load = true;
  // gate/up as a row-tile-persistent GEMV with RMS_NORM on load (<= 4 rows); MX_NO_PERS=1 for A/B
  bool use_pers = getenv("MX_NO_PERS") == nullptr;
  bool q8_gemm_prefill = getenv("MX_Q8_GEMM_PREFILL") != nullptr;  // see enqueue_forward
  // K-quant prefill chunks with ggml's arithmetic (Q8_K activations, the int8 K-quant GEMVs at every
  // row count) instead of bf16 GEMMs over dequantised weights; see enqueue_forward
  bool kq_ggml_prefill = getenv("MX_KQ_GGML_PREFILL") != nullptr;
  float* ssq = nullptr;  // [MAX_ROWS][n_embd/16] per-tile sums of squares of x
  // rows of the next forward belong to distinct sequences (decode): no row attends to another row's
  // new K/V, so the wide path lets the attention kernel finish q/k/v from the split-K slabs
  bool rows_distinct = false;
  // rows of the next forward come in blocks of 16 consecutive positions of one sequence (prefill):
  // attention runs as attn_prefill_kernel, 16 queries per K/V pass
  bool rows_blocked = false;
  // the next forward is a prompt chunk from the scheduler or a pipeline prefill: every row count takes
  // the GEMM path (one K range per output: the arithmetic of a prompt row does not depend on how many
  // rows share its chunk -- batch invariance)
  bool prefill_gemm = false;
  bool use_wide = getenv("MX_NO_WIDE") == nullptr;  // 17..64-row forward through mm_wide (LDS-shared activations)
  float* slabs = nullptr;                           // split-K partials [8][MAX_ROWS][n_embd + 2 n_embd_kv]
  size_t slab_stride = 0;
  float* gslabs = nullptr;  // split-K partials of small-M prefill GEMMs, [S][M][N] (launch_gemm_split)
  // K-quant model prefill: one layer's four matrices dequantised to packed bf16 for the GEMM path
  uint16_t *kqd_qkv = nullptr, *kqd_o = nullptr, *kqd_gu = nullptr, *kqd_down = nullptr;
  static constexpr size_t GSLAB_FLOATS = (size_t)32 << 20;
  // work-groups a split prefill GEMM aims at (MX_GEMM_SPLIT_TARGET; 0 = one K range per tile).  Default 0:
  // a split chosen from the chunk's row count would make a prompt's values depend on its chunk-mates
  int gemm_split_target = getenv("MX_GEMM_SPLIT_TARGET") ? atoi(getenv("MX_GEMM_SPLIT_TARGET")) : 0;
  int ctx_stride = 0;  // KV positions allocated per slot (n_ctx rounded up to KV_POS_ALIGN)
  uint64_t weight_bytes = 0;

  // device state
  hipStream_t stream = nullptr;
  uint16_t *tok_embd = nullptr, *output = nullptr;
  float* out_norm = nullptr;
  // Q8_0 model: layer matrices as packed Q8 tiles; token_embd / output may each
  // be Q8_0 (tok_embd8: GGUF blocks, row-major) or BF16
  bool wq8 = false, embd_q8 = false, out_q8 = false;
  // Q4_0 model (llama.cpp Q4_0 files): the layer matrices are Q4 tiles on the Q8_0 path (Q8_0 activation
  // rows, ggml_vec_dot_q4_0_q8_0); the head is Q8_0 / Q4_0 tiles (out_q4) or, as llama-quantize writes it,
  // a K-quant output (out_kq_head: kq_out segments, Q8_K activation rows)
  bool wq4 = false, out_q4 = false, out_kq_head = false;
  static constexpr bool q8_ql = true;  // Q8_0 GEMVs of <= 4 rows quantise their operand on load
  uint8_t* tok_embd8 = nullptr;
  // K-quant model (Q4_K / Q5_K / Q6_K matrices: llama.cpp's Q4_K_M / Q5_K_M; kquant.hip): packed
  // K-quant tiles, activations as Q8_K rows (q in xq8, d in xqd, sub-block sums in xkb)
  bool wkq = false;
  int kq_main_type = 0;          // type of ffn_gate (mx_model_info.weight_type)
  int embd_kq_type = 0;          // token_embd kept as K-quant GGUF blocks when non-zero
  uint8_t* tok_embd_kq = nullptr;
  // LoRA adapter merged at load: opened and checked against the base before the engine touches
  // the device, released when load_gguf returns; the counters are what mx_engine_lora_info reports
  std::unique_ptr<LoraAdapter> lora;
  float lora_scale = 0.f, lora_alpha = 0.f;
  int lora_merged = 0, lora_rank_max = 0;
  bool has_lora = false;
  float* xkb = nullptr;
  KqMat kq_out;
  int8_t* xq8 = nullptr;    // Q8_0 activation rows [PREFILL_ROWS][max(h, ff)]
  float* xqd = nullptr;     // their block scales
  float *attn_f = nullptr, *act_f = nullptr;  // f32 attention output / SwiGLU product (quantised next)
  std::vector<Layer> layers;  // local layers [lb, le)
  _Float16 *kcache = nullptr, *vcache = nullptr;
  size_t slot_stride = 0, layer_kv_stride = 0;
  float* rope_cs = nullptr;
  // workspaces (MAX_ROWS rows)
  float *x = nullptr, *q = nullptr, *logits = nullptr;
  uint16_t *xn = nullptr, *act = nullptr, *attn_out = nullptr;
  float* am_val = nullptr;
  bool use_dev_topk = getenv("MX_NO_DEV_TOPK") == nullptr;  // MX_NO_DEV_TOPK: all-host sampler (tests)
  float *tk_ws_val = nullptr, *tk_val = nullptr;  // device top-k for the sampler chain
  int *tk_ws_idx = nullptr, *tk_idx = nullptr;
  int *am_idx = nullptr, *d_tok = nullptr;
  int *d_ids = nullptr, *d_pos = nullptr, *d_slot = nullptr, *d_rowmap = nullptr;
  // pinned host staging of forward_rows_chunk's index arrays [4][R]: its async copies read from here
  // (engine-owned), not through the runtime's staging of pageable memory
  int32_t* h_idx = nullptr;
  std::vector<void*> allocations;

  // graphs for the scheduler's decode steps, by (M, top-k of the device sampling chain or 0 = argmax)
  // ... and the top-k of the round's log-probabilities (-1: none; such rounds enqueue what they always did)
  // ... and whether the round runs the extended chain (0: none; 1: bias / tail-free / typical; 2: Mirostat too;
  // + 4: some row takes the wide kernel)
  std::map<std::tuple<int, int, int, int>, hipGraphExec_t> sched_graphs;
  // pipeline stage hand-off dtype: x_in / x_out are bf16 [M][n_embd] instead of f32 (mx_opts.handoff_bf16)
  bool handoff_bf16 = false;
  // token pick at the end of a forward with `argmax` set: greedy argmax, or (pick_samp) the device
  // sampling chain with top-k pick_k over the rows' SampRow settings
  const SampRow* pick_samp = nullptr;
  int pick_k = 0;
  SampRow* d_samp = nullptr;  // [MAX_ROWS] the scheduler's rows
  // log-probabilities of the pick (request path): pick_lp >= 0 runs the row statistics
  // ((m, log s) and the top pick_lp log-probs) on the raw logits before the penalties rewrite them, and
  // after the pick gathers the chosen token's entry into lp_hist [MAX_ROWS][SCHED_KMAX][1 + 2 pick_lp]
  int pick_lp = -1;
  float *lp_part = nullptr, *lp_ms = nullptr, *lp_top = nullptr, *lp_hist = nullptr, *lp_side_val = nullptr;
  int *lp_idx = nullptr, *lp_side_tok = nullptr, *lp_tgt = nullptr;
  // the rest of the chain: pick_ext = d_sext when some row of the run has a SampExt setting
  // (null: the launches are those of the plain chain), pick_miro when one of them is a Mirostat row.
  // d_mu [MAX_ROWS]: Mirostat state of the rows, d_mu_hist [MAX_ROWS][SCHED_KMAX] its value after each step
  const SampExt* pick_ext = nullptr;
  bool pick_miro = false, pick_wide = false;  // pick_wide: a row with more than TOPK_MAX candidates
  SampExt* d_sext = nullptr;
  float *d_bias_raw = nullptr, *d_mu = nullptr, *d_mu_hist = nullptr, *miro_wf = nullptr;
  double* miro_wd = nullptr;
  int* miro_wi = nullptr;
  // grammar masks: pick_gram set when some row of the run has a grammar -- the mask kernel then
  // runs between the log-prob statistics and the pick.  d_gmask [MAX_ROWS][gmask_words], d_gon [MAX_ROWS] and
  // their pinned mirror h_gmask ([MAX_ROWS][gmask_words] then the on words) come with the first grammar request
  bool pick_gram = false;
  bool gram_refused = false;  // launch_grammar_mask refused a launch of pick(): the step's tokens are not kept
  uint32_t *d_gmask = nullptr, *d_gon = nullptr, *h_gmask = nullptr;
  int gmask_words = 0;
  // the mask of the step a grammar request is about to take (from its state, or its grammar's cache); false with
  // its error text set: no token is allowed, or the state is over the position cap
  static bool gram_step_mask(Request* r) {
    const int st = r->gram->mask(&r->gram_mask);
    if (st == gram::STATE_OK) return true;
    r->error = st == gram::STATE_CAP
                   ? "grammar: more than " + std::to_string(gram::MAX_POSITIONS) + " simultaneous positions, or a mask past "
                         "the work budget"
                   : "grammar: dead end, no token of the vocabulary is allowed after " + std::to_string(r->out.size()) +
                         " generated tokens";
    return false;
  }
  static bool gram_row(const Request* r) { return r->gram && !r->gram_end && r->gram_mask; }
  // on words of rows[0..n) and the masks of its grammar rows (those only) to the device; 1 when there is one
  // (pick_gram set), 0 when none (nothing copied), < 0 on an error
  int upload_gram(Request* const* rows, int n, hipStream_t s) {
    pick_gram = false;
    bool any = false;
    for (int i = 0; i < n; i++) any |= gram_row(rows[i]);
    if (!any) return 0;
    const int nw = (n_vocab + 31) / 32;
    // each buffer once: what a failed attempt did allocate is kept for the next one
    if (!d_gmask && alloc((void**)&d_gmask, (size_t)MAX_ROWS * nw * 4)) return d_gmask = nullptr, -1;
    if (!d_gon && alloc((void**)&d_gon, (size_t)MAX_ROWS * 4)) return d_gon = nullptr, -1;
    if (!h_gmask && hipHostMalloc((void**)&h_gmask, ((size_t)MAX_ROWS * nw + MAX_ROWS) * 4) != hipSuccess)
      return h_gmask = nullptr, -1;
    gmask_words = nw;
    uint32_t* h_on = h_gmask + (size_t)MAX_ROWS * nw;
    for (int i = 0; i < n; i++) {
      h_on[i] = gram_row(rows[i]) ? 1u : 0u;
      if (!h_on[i]) continue;
      memcpy(h_gmask + (size_t)i * nw, rows[i]->gram_mask->data(), (size_t)nw * 4);
      if (hipMemcpyAsync(d_gmask + (size_t)i * nw, h_gmask + (size_t)i * nw, (size_t)nw * 4, hipMemcpyHostToDevice, s) !=
          hipSuccess)
        return -1;
    }
    if (hipMemcpyAsync(d_gon, h_on, (size_t)n * 4, hipMemcpyHostToDevice, s) != hipSuccess) return -1;
    pick_gram = true;
    return 1;
  }
  // the same mask on a host copy of a row (host-sampled rounds)
  void gram_mask_host(const Request* r, float* x) const {
    const std::vector<uint32_t>& w = *r->gram_mask;
    for (int t = 0; t < n_vocab; t++)
      if (!((w[t >> 5] >> (t & 31)) & 1u)) x[t] = -INFINITY;
  }
  std::vector<SampExt> h_sext;  // host staging of upload_ext
  std::vector<float> h_mu;
  // SampExt rows and mu of a run over rows[0..n) to the device and pick_ext / pick_miro / pick_wide set; returns
  // the level the graph key carries (0: no row has a setting, nothing copied; 1: some; 2: a Mirostat row among
  // them; + 4: a wide row among them)
  int upload_ext(Request* const* rows, int n, hipStream_t s) {
    pick_ext = nullptr, pick_miro = false, pick_wide = false;
    bool any = false;
    int kw = 0;
    for (int i = 0; i < n; i++) any |= rows[i]->has_ext || req_path(rows[i], n_vocab, &kw) == MX_PICK_WIDE;
    if (!any) return 0;
    // the buffers of the extended chain come with its first request, so an engine that never sees one has the
    // device memory layout it always had
    if (!d_sext &&
        (alloc((void**)&d_sext, (size_t)MAX_ROWS * sizeof(SampExt)) ||
         alloc((void**)&d_bias_raw, (size_t)MAX_ROWS * SAMP_BIAS_MAX * 4) || alloc((void**)&d_mu, (size_t)MAX_ROWS * 4) ||
         alloc((void**)&d_mu_hist, (size_t)MAX_ROWS * SCHED_KMAX * 4) ||
         alloc((void**)&miro_wf, miro_ws_floats(MAX_ROWS) * 4) || alloc((void**)&miro_wd, miro_ws_doubles(MAX_ROWS) * 8) ||
         alloc((void**)&miro_wi, miro_ws_ints(MAX_ROWS) * 4))) {
      d_sext = nullptr;
      return -1;
    }
    h_sext.assign(n, SampExt{});
    h_mu.assign(n, 0.f);
    for (int i = 0; i < n; i++) {
      if (rows[i]->has_ext) h_sext[i] = rows[i]->ext;
      else h_sext[i].typical_p = h_sext[i].tfs_z = 1.0f;
      h_mu[i] = rows[i]->mu;
      pick_miro |= h_sext[i].miro == 2;
      h_sext[i].wide_k = req_path(rows[i], n_vocab, &kw) == MX_PICK_WIDE ? kw : 0;
      pick_wide |= h_sext[i].wide_k > 0;
    }
    if (hipMemcpyAsync(d_sext, h_sext.data(), n * sizeof(SampExt), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_mu, h_mu.data(), n * 4, hipMemcpyHostToDevice, s) != hipSuccess)
      return -1;
    pick_ext = d_sext;
    return (pick_miro ? 2 : 1) + (pick_wide ? 4 : 0);
  }
  void pick(int n_out, const PickOut& o, hipStream_t s) {
    const bool lp = pick_lp >= 0;
    SampExtArgs xa;
    xa.ext = pick_samp ? pick_ext : nullptr;
    xa.bias_raw = d_bias_raw, xa.mu = d_mu, xa.mu_hist = d_mu_hist, xa.mu_stride = SCHED_KMAX;
    xa.ws_f = miro_wf, xa.ws_d = miro_wd, xa.ws_i = miro_wi, xa.any_miro = pick_miro;
    xa.any_wide = pick_wide;
    if (lp)
      launch_logprob_stats(logits, n_vocab, n_out, n_vocab, pick_lp, tk_ws_val, tk_ws_idx, lp_part, lp_ms, lp_top,
                           lp_idx, s);
    if (pick_gram && launch_grammar_mask(logits, n_vocab, n_out, n_vocab, d_gmask, d_gon, s)) gram_refused = true;
    if (pick_samp)
      launch_sample_chain(logits, n_vocab, n_out, n_vocab, pick_samp, pick_k, tk_ws_val, tk_ws_idx, tk_val, tk_idx,
                          d_tok, o.ids_next, o.pos_next, o.hist, o.hist_stride, o.hist_count, o.max_hist, s,
                          lp ? lp_side_tok : nullptr, lp ? lp_side_val : nullptr, xa.ext ? &xa : nullptr);
    else
      launch_argmax(logits, n_vocab, n_out, n_vocab, am_val, am_idx, d_tok, o.ids_next, o.pos_next, o.hist,
                    o.hist_stride, o.hist_count, o.max_hist, s);
    if (lp)
      launch_logprob_gather(logits, n_vocab, n_out, n_vocab, pick_lp, d_tok, o.hist ? o.hist_count : nullptr, SCHED_KMAX,
                            pick_samp ? lp_side_tok : nullptr, lp_side_val, lp_ms, lp_top, lp_idx, lp_hist,
                            (size_t)SCHED_KMAX * (1 + 2 * pick_lp), s, xa.ext, d_bias_raw);
  }
  int copy_out(void* x_out, int M, hipStream_t s) {  // the residual stream to the next stage
    if (handoff_bf16) launch_f32_to_bf16((uint16_t*)x_out, x, (size_t)M * n_embd, s);
    else launch_copy_f32((float*)x_out, x, (size_t)M * n_embd, s);
    return 0;
  }
  // SampRow of a request for a run that starts now (draw index and penalty window at this point)
  void samp_row(const Request* r, SampRow* o) const;

  // scheduler
  std::mutex gpu_mu;  // serialises all GPU work issued through the API
  std::mutex mu;
  std::condition_variable cv, cv_done;
  std::deque<Request*> pending;
  std::vector<Request*> active;
  std::map<uint64_t, std::unique_ptr<Request>> requests;
  std::vector<int> free_slots;
  // prefix-KV reuse (llama-cpp-python's Llama.generate keeps the longest common prefix of the previous
  // evaluation): tokens whose K/V each slot holds at positions 0..n-1.  Of a busy slot too: cut to the
  // request's reuse at admission, its whole prompt after the prefill, prompt + out[:-1] cut at its pos after
  // every round (note_kv) -- what prefix sharing copies from
  std::vector<std::vector<int32_t>> slot_tokens;
  void note_kv(const Request* r);
  // prefix sharing across slots (mx_engine_set_prefix_sharing): a copy has to save at least SHARE_MIN positions
  // -- one prefill row block; below it the block's recomputation is cheaper than a launch
  static constexpr int SHARE_MIN = 16;
  bool prefix_sharing = false;
  KvCopy* d_kvcopy = nullptr;  // [n_seq_max] the copy tables of a round
  uint64_t stat_shared_tokens = 0, stat_copies = 0, stat_copied_bytes = 0, stat_followers = 0;
  // the copies of `tab` in one launch.  The admission rule never makes a table the launcher refuses: a
  // destination is a free slot, taken once; a source that beats the destination's own match is not free (the
  // destination rule would have taken it), and a slot a copy fills never matches better than the slot it is
  // filled from, which wins the tie -- so no slot is both
  int run_kv_copies(const std::vector<KvCopy>& tab);
  // host-RAM tier behind the slots (mx_engine_set_host_cache).  A slot record about to be
  // destroyed is packed into pack_stage on the engine stream and leaves for pinned host memory on stream2; a
  // prompt that matches a host entry HOST_MIN positions better than any device source gets them back through
  // unpack_stage.  HOST_MIN is one packed tile.  The store is the scheduler thread's alone (under mu where the
  // admission loop reads it); host_cap_req is the API's side of the capacity, applied at the top of the loop.
  static constexpr int HOST_MIN = 32;
  struct HostEntry {
    std::vector<int32_t> tokens;  // the record it was spilled from
    void* pinned = nullptr;       // packed K/V of ceil32(tokens.size()) positions
    size_t bytes = 0;
    hipEvent_t done = nullptr;  // its device-to-host transfer
    uint64_t used = 0, born = 0;  // LRU clock; the admission round that made it (visible from the next one on)
  };
  struct HostSpill { std::shared_ptr<HostEntry> e; int slot; };
  struct HostRestore { std::shared_ptr<HostEntry> e; int slot, n_pos; };
  std::vector<std::shared_ptr<HostEntry>> host_entries, host_trash;  // trash: evicted, freed after the round
  uint64_t host_cap = 0, host_cap_req = 0, host_bytes = 0, host_clock = 0, host_round = 0;
  bool host_failed = false;  // the staging could not be allocated
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_packed = nullptr, ev_stage_free = nullptr;
  char *pack_stage = nullptr, *unpack_stage = nullptr;
  size_t stage_bytes = 0, host_tile_bytes = 0;
  KvPack *d_pack_tab = nullptr, *d_unpack_tab = nullptr, *h_pack_tab = nullptr;  // [n_seq_max] each; h: pinned, both
  uint64_t stat_host_spills = 0, stat_host_spilled_bytes = 0, stat_host_restores = 0, stat_host_restored_tokens = 0,
           stat_host_restored_bytes = 0, stat_host_evictions = 0, stat_host_skipped = 0;
  void host_apply_capacity();                                  // under mu, scheduler thread
  void host_drop(size_t i) {                                   // under mu: entry i leaves the store
    host_bytes -= host_entries[i]->bytes;
    host_trash.push_back(std::move(host_entries[i]));
    host_entries.erase(host_entries.begin() + i);
  }
  void host_insert(const std::vector<int32_t>& st, int slot, std::vector<HostSpill>& spills);  // under mu
  void host_free_trash();
  int run_host_spills(std::vector<HostSpill>& spills);
  int run_host_restores(const std::vector<HostRestore>& restores);
  uint64_t stat_prompt_tokens = 0, stat_reused_tokens = 0, stat_generated_tokens = 0;
  uint64_t next_id = 1;
  bool stop = false;
  std::thread worker;
  bool worker_started = false;

  ~mx_engine();
  int alloc(void** p, size_t bytes) {
    HIPC(hipMalloc(p, bytes));
    allocations.push_back(*p);
    if (poison) HIPC(hipMemset(*p, 0xFF, bytes));  // NaN in every f32 / f16 / bf16 lane
    return 0;
  }
  // diagnosis (mx_debug): MX_POISON=1 fills every allocation with 0xFF bytes and skips the zero
  // fills of init_common, so a read of a never-written element shows up as a NaN; dbg_stop ends the
  // 17..64-row forward after that many launches, dbg_sync synchronises the stream after each one
  const bool poison = getenv("MX_POISON") != nullptr;
  int dbg_stop = -1, dbg_count = 0;
  bool dbg_sync = false;
  // never while a graph is being captured: a captured forward would keep the truncation (or the capture
  // would be invalidated by the sync) for every later replay
  bool dbg_hit(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
    if (dbg_sync) hipStreamSynchronize(s);
    return dbg_stop >= 0 && ++dbg_count >= dbg_stop;
  }
  int init_common();
  int load_synthetic(const Shape& s, uint64_t seed, bool q8 = false, int kq_base = 0, bool q4 = false);
  int load_gguf(const std::string& path);
  int enqueue_forward(const Forward& f, hipStream_t s);
  bool q8_on_load(int M) const {
    return wq8 && q8_ql && mq8_can_quantize_on_load(M, n_embd, true) && mq8_can_quantize_on_load(M, n_ff, false);
  }
  // one-token K-quant GEMVs quantise their Q8_K operand on load (no norm / quantise launches)
  bool kq_on_load(int M) const {
    return wkq && mkq_can_quantize_on_load(M, n_embd, true) && mkq_can_quantize_on_load(M, n_ff, false);
  }
  int enqueue_forward_quant(const Forward& f, hipStream_t s);
  int quant_operand(MMArgs& m, const KqMat* km, bool ql, int& nslab, const float* src, int K, const float* norm_w,
                    int rows, const int* rmap, hipStream_t s);
  int quant_head(const Forward& f, int& nslab, hipStream_t s);
  // what every walk's q|k|v GEMV and attention launch of layer li share; the walk adds its operand and outputs
  MMArgs qkv_args(const Layer& L, int li, const Forward& f) const;
  AttnArgs attn_args(int li, const Forward& f) const;
  int enqueue_forward_gemm(const Forward& f, hipStream_t s);
  bool gemm_shapes() const {  // the bf16 prefill GEMM takes every matrix of a layer
    return gemm_supported(n_embd + 2 * n_embd_kv, n_embd) && gemm_supported(n_embd, n_embd) &&
           gemm_supported(2 * n_ff, n_embd) && gemm_supported(n_embd, n_ff);
  }
  // launch_mm_wide walks K in chunks of 4 K tiles: a model whose n_embd or n_ff is no multiple of 128 (n_embd 448)
  // runs its 17..64-row forwards through launch_mm, as it runs its <= 16-row ones
  bool wide_shapes() const { return n_embd % (4 * TILE_K) == 0 && n_ff % (4 * TILE_K) == 0; }
  bool gemm_ok() const {  // chunks of PREFILL_ROWS rows can run (the Q8_0 / K-quant paths take any row count)
    return wq8 || wkq || gemm_shapes();
  }
  int enqueue_forward_wide(const Forward& f, hipStream_t s, bool full_chain = false);
  int forward_rows_chunk(int n, const int32_t* slots, const int32_t* pos, const int32_t* ids, const void* x_in,
                         void* x_out, float* logits_host, hipStream_t s, bool last_row_only = false);
  void scheduler_loop();
  int sched_step(std::vector<Request*>& rows);
  int prefill_batch(std::vector<Request*>& reqs);
  int prefill_prompt_logprobs(Request* r);
  // embeddings: per KV slot the running MEAN sum of a sequence that spans chunks and its pooled
  // vector, [n_seq_max][n_embd] each; the row / segment tables of a chunk's tail launches.  The normed rows of a
  // chunk go to q, which nothing reads once a forward without lm_head has ended.
  float *embd_acc = nullptr, *embd_pooled = nullptr;
  int* d_embd_tab = nullptr;
  static constexpr size_t EMBD_TAB_CAP = embd_tab_ints(PREFILL_ROWS, PREFILL_ROWS / 16);  // a sequence starts a 16-row block
  int prefill_embed(std::vector<Request*>& reqs);
  int* sched_hist = nullptr;        // [MAX_ROWS][SCHED_KMAX] tokens of a multi-step greedy run
  int* sched_hist_count = nullptr;  // [MAX_ROWS]
  // speculating rounds: graphs by (requests, draft rows per request), and the device state
  // of the round's requests -- their token sequences [SPEC_MAX_REQ][n_ctx] and lengths, {num_pred_tokens,
  // max_ngram_size}, draft lengths, the variable-length token history [SPEC_MAX_REQ][SCHED_KMAX * SPEC_ROWS]
  // with its counts, the counters [.][3] and the per-step log [.][SCHED_KMAX][2] = {n_draft, accepted}
  std::map<std::pair<int, int>, hipGraphExec_t> spec_graphs;
  int *spec_ctx = nullptr, *spec_len = nullptr, *spec_par = nullptr, *spec_ndraft = nullptr, *spec_hist = nullptr;
  int *spec_hist_count = nullptr, *spec_cnt = nullptr, *spec_log = nullptr;
  uint64_t stat_spec_steps = 0, stat_spec_drafted = 0, stat_spec_accepted = 0;
  // mx_sampler_stats: decode steps picked on the device / in sample_host, the rounds they ran in, and the
  // row-steps of the wide kernel
  uint64_t stat_dev_steps = 0, stat_host_steps = 0, stat_rounds = 0, stat_wide_rows = 0;
  bool spec_eligible(const Request* r) const;
  // 1 when the round ran speculating (rows updated), 0 when it has to run plain, < 0 on an error
  int sched_step_spec(std::vector<Request*>& rows);
  int32_t sample_host(Request* r, const float* logits);
  int32_t sample_chain(Request* r, std::vector<std::pair<float, int>>& c);  // c: top-k, sorted
  void finish(Request* r, int why);
};

mx_engine::~mx_engine() {
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  if (worker.joinable()) worker.join();
  for (auto& kv : sched_graphs) hipGraphExecDestroy(kv.second);
  for (auto& kv : spec_graphs) hipGraphExecDestroy(kv.second);
  if (stream) hipStreamSynchronize(stream);
  // the host tier: its transfers end before the pinned memory and the staging they use are freed
  if (stream2) hipStreamSynchronize(stream2);
  while (!host_entries.empty()) host_drop(host_entries.size() - 1);
  host_free_trash();
  if (h_pack_tab) hipHostFree(h_pack_tab);
  if (h_gmask) hipHostFree(h_gmask);
  if (ev_packed) hipEventDestroy(ev_packed);
  if (ev_stage_free) hipEventDestroy(ev_stage_free);
  if (stream2) hipStreamDestroy(stream2);

  for (void* p : allocations) hipFree(p);
  if (h_idx) hipHostFree(h_idx);
  if (stream) hipStreamDestroy(stream);
}

int mx_engine::init_common() {
  head_dim = n_embd / n_head;
  n_embd_kv = head_dim * n_head_kv;
  if (n_embd % n_head || n_head % n_head_kv) return fail(MX_ERR_MODEL, "head counts do not divide n_embd/n_head");
  if (head_dim != 64 && head_dim != 128) return fail(MX_ERR_ARG, "head_dim must be 64 or 128");
  if (n_embd > 8192) return fail(MX_ERR_ARG, "n_embd > 8192 is not supported");
  if (n_embd % 64) return fail(MX_ERR_ARG, "n_embd must be a multiple of 64 (RMS_NORM tile partials)");
  const int G = n_head / n_head_kv;
  // 5, 6, 7: the Qwen2.5 groups; 3 has no kernel instance and no model that needs one
  if (G != 1 && G != 2 && (G < 4 || G > 8)) return fail(MX_ERR_ARG, "n_head/n_head_kv must be 1, 2 or 4..8");
  if (n_embd % 32 || n_ff % 32 || n_vocab % 16 || n_embd_kv % 16)
    return fail(MX_ERR_ARG, "n_embd, n_ff must be multiples of 32 and n_vocab, n_embd_kv of 16");
  if (wq8 && (n_embd % Q8_TILE_K || n_ff % Q8_TILE_K))
    return fail(MX_ERR_ARG, "Q8_0 models need n_embd and n_ff multiples of 64");
  if (wkq && (n_embd % 256 || n_ff % 256)) return fail(MX_ERR_ARG, "K-quant models need n_embd and n_ff multiples of 256");
  if (le < 0 || le > n_layer) le = n_layer;
  if (lb < 0 || lb >= le) return fail(MX_ERR_ARG, "bad layer range");
  has_embed = lb == 0;
  has_head = le == n_layer;
  ctx_stride = (n_ctx + KV_POS_ALIGN - 1) / KV_POS_ALIGN * KV_POS_ALIGN;
  const int nl = le - lb;
  layers.resize(nl);

  // KV cache per layer and slot: K and V [kv head][ctx_stride * head_dim] f16 in 1 KiB MFMA B-operand
  // tiles (kernels.hip kv_k_off / kv_v_off)
  slot_stride = (size_t)n_head_kv * ctx_stride * head_dim;
  layer_kv_stride = slot_stride * n_seq_max;
  if (int rc = alloc((void**)&kcache, layer_kv_stride * nl * sizeof(_Float16))) return rc;
  if (int rc = alloc((void**)&vcache, layer_kv_stride * nl * sizeof(_Float16))) return rc;
  if (!poison) {
    HIPC(hipMemsetAsync(kcache, 0, layer_kv_stride * nl * sizeof(_Float16), stream));
    HIPC(hipMemsetAsync(vcache, 0, layer_kv_stride * nl * sizeof(_Float16), stream));
  }

  // RoPE table, ggml_rope_cache_init + rope_yarn (ext_factor 0, mscale 1): theta *= powf(base, -2/d)
  // as an f32 running product, divided by the frequency factor, times the linear freq_scale
  if (!rope_ff.empty() && (int)rope_ff.size() != head_dim / 2) return fail(MX_ERR_MODEL, "rope_freqs.weight size");
  std::vector<float> cs((size_t)n_ctx * head_dim);
  const float theta_scale = powf(rope_base, -2.0f / (float)head_dim);
  for (int p = 0; p < n_ctx; p++) {
    float theta = (float)p;
    for (int i = 0; i < head_dim / 2; i++) {
      const float ff = rope_ff.empty() ? 1.0f : rope_ff[i];
      const float th = rope_freq_scale * (theta / ff);
      cs[((size_t)p * (head_dim / 2) + i) * 2] = cosf(th);
      cs[((size_t)p * (head_dim / 2) + i) * 2 + 1] = sinf(th);
      theta *= theta_scale;
    }
  }
  if (int rc = alloc((void**)&rope_cs, cs.size() * 4)) return rc;
  HIPC(hipMemcpy(rope_cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));

  const int R = PREFILL_ROWS;  // activation rows: prefill chunks (GEMM path); logits only for MAX_ROWS
  if (int rc = alloc((void**)&x, (size_t)R * n_embd * 4)) return rc;
  if (int rc = alloc((void**)&q, (size_t)R * n_embd * 4)) return rc;
  if (int rc = alloc((void**)&xn, (size_t)R * n_embd * 2)) return rc;
  if (int rc = alloc((void**)&attn_out, (size_t)R * n_embd * 2)) return rc;
  if (int rc = alloc((void**)&act, (size_t)R * n_ff * 2)) return rc;
  if (has_head) {
    if (int rc = alloc((void**)&logits, (size_t)MAX_ROWS * n_vocab * 4)) return rc;
  }
  slab_stride = (size_t)MAX_ROWS * (n_embd + 2 * n_embd_kv);
  if (int rc = alloc((void**)&slabs, slab_stride * 8 * 4)) return rc;
  if (gemm_shapes())
    if (int rc = alloc((void**)&gslabs, GSLAB_FLOATS * 4)) return rc;
  if ((wkq || (wq8 && !wq4 && q8_gemm_prefill)) && gemm_shapes()) {  // per-layer bf16 copies for the prefill GEMM
    const size_t h = n_embd, kv = n_embd_kv, ff = n_ff;
    if (int rc = alloc((void**)&kqd_qkv, (h + 2 * kv) * h * 2)) return rc;
    if (int rc = alloc((void**)&kqd_o, h * h * 2)) return rc;
    if (int rc = alloc((void**)&kqd_gu, 2 * ff * h * 2)) return rc;
    if (int rc = alloc((void**)&kqd_down, h * ff * 2)) return rc;
  }
  if (int rc = alloc((void**)&ssq, (size_t)R * (n_embd / 16) * 4)) return rc;
  if (int rc = alloc((void**)&am_val, (size_t)R * 64 * 4)) return rc;
  if (has_head) {
    if (int rc = alloc((void**)&tk_ws_val, (size_t)MAX_ROWS * 64 * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&tk_ws_idx, (size_t)MAX_ROWS * 64 * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&tk_val, (size_t)MAX_ROWS * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&tk_idx, (size_t)MAX_ROWS * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&lp_part, (size_t)MAX_ROWS * 64 * 2 * 4)) return rc;
    if (int rc = alloc((void**)&lp_ms, (size_t)MAX_ROWS * 2 * 4)) return rc;
    if (int rc = alloc((void**)&lp_top, (size_t)MAX_ROWS * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&lp_idx, (size_t)MAX_ROWS * TOPK_MAX * 4)) return rc;
    if (int rc = alloc((void**)&lp_hist, (size_t)MAX_ROWS * SCHED_KMAX * (1 + 2 * TOPK_MAX) * 4)) return rc;
    if (int rc = alloc((void**)&lp_side_tok, (size_t)MAX_ROWS * SAMP_WIN * 4)) return rc;
    if (int rc = alloc((void**)&lp_side_val, (size_t)MAX_ROWS * SAMP_WIN * 4)) return rc;
    if (int rc = alloc((void**)&lp_tgt, (size_t)MAX_ROWS * 4)) return rc;
  }
  if (int rc = alloc((void**)&am_idx, (size_t)R * 64 * 4)) return rc;
  if (int rc = alloc((void**)&d_tok, (size_t)R * 4)) return rc;
  if (int rc = alloc((void**)&d_ids, (size_t)R * 4)) return rc;
  if (int rc = alloc((void**)&d_pos, (size_t)R * 4)) return rc;
  if (int rc = alloc((void**)&d_slot, (size_t)R * 4)) return rc;
  if (int rc = alloc((void**)&d_rowmap, (size_t)R * 4)) return rc;
  HIPC(hipHostMalloc((void**)&h_idx, (size_t)4 * R * 4, hipHostMallocDefault));
  if (int rc = alloc((void**)&sched_hist, (size_t)MAX_ROWS * SCHED_KMAX * 4)) return rc;
  if (int rc = alloc((void**)&sched_hist_count, (size_t)MAX_ROWS * 4)) return rc;
  if (int rc = alloc((void**)&d_samp, (size_t)MAX_ROWS * sizeof(SampRow))) return rc;
  if (int rc = alloc((void**)&d_kvcopy, (size_t)n_seq_max * sizeof(KvCopy))) return rc;
  if (has_embed && has_head && !wq8 && !wkq) {
    if (int rc = alloc((void**)&spec_ctx, (size_t)SPEC_MAX_REQ * n_ctx * 4)) return rc;
    if (int rc = alloc((void**)&spec_len, SPEC_MAX_REQ * 4)) return rc;
    if (int rc = alloc((void**)&spec_par, SPEC_MAX_REQ * 2 * 4)) return rc;
    if (int rc = alloc((void**)&spec_ndraft, SPEC_MAX_REQ * 4)) return rc;
    if (int rc = alloc((void**)&spec_hist, (size_t)SPEC_MAX_REQ * SCHED_KMAX * SPEC_ROWS * 4)) return rc;
    if (int rc = alloc((void**)&spec_hist_count, SPEC_MAX_REQ * 4)) return rc;
    if (int rc = alloc((void**)&spec_cnt, SPEC_MAX_REQ * 3 * 4)) return rc;
    if (int rc = alloc((void**)&spec_log, SPEC_MAX_REQ * SCHED_KMAX * 2 * 4)) return rc;
  }
  if (has_embed && has_head) {
    if (int rc = alloc((void**)&embd_acc, (size_t)n_seq_max * n_embd * 4)) return rc;
    if (int rc = alloc((void**)&embd_pooled, (size_t)n_seq_max * n_embd * 4)) return rc;
    if (int rc = alloc((void**)&d_embd_tab, EMBD_TAB_CAP * 4)) return rc;
  }
  if (wq8 || wkq) {
    const size_t kmax = std::max(n_embd, n_ff);
    if (int rc = alloc((void**)&xq8, (size_t)R * kmax)) return rc;
    if (int rc = alloc((void**)&xqd, (size_t)R * (kmax / 32) * 4)) return rc;
    if (int rc = alloc((void**)&attn_f, (size_t)R * n_embd * 4)) return rc;
    if (int rc = alloc((void**)&act_f, (size_t)R * n_ff * 4)) return rc;
    if (wkq || out_kq_head)
      if (int rc = alloc((void**)&xkb, (size_t)R * (kmax / 32) * 4)) return rc;
  }
  // poison-free start: zero activations so padded MFMA columns never read uninitialised memory
  if (!poison) {
    HIPC(hipMemsetAsync(xn, 0, (size_t)R * n_embd * 2, stream));
    HIPC(hipMemsetAsync(attn_out, 0, (size_t)R * n_embd * 2, stream));
    HIPC(hipMemsetAsync(act, 0, (size_t)R * n_ff * 2, stream));
  }
  for (int i = 0; i < n_seq_max; i++) free_slots.push_back(n_seq_max - 1 - i);
  slot_tokens.assign(n_seq_max, {});
  return 0;
}

static int alloc_layer(mx_engine* e, Layer& L) {
  const size_t h = e->n_embd, kv = e->n_embd_kv, ff = e->n_ff;
  if (e->wq8) {
    auto qb = e->wq4 ? q4_matrix_bytes : q8_matrix_bytes;
    const size_t bq = qb(h + 2 * kv, h), bo = qb(h, h), bg = qb(2 * ff, h), bd = qb(h, ff);
    if (int rc = e->alloc((void**)&L.qkv, bq)) return rc;
    if (int rc = e->alloc((void**)&L.o, bo)) return rc;
    if (int rc = e->alloc((void**)&L.gu, bg)) return rc;
    if (int rc = e->alloc((void**)&L.down, bd)) return rc;
    if (int rc = e->alloc((void**)&L.attn_norm, h * 4)) return rc;
    if (int rc = e->alloc((void**)&L.ffn_norm, h * 4)) return rc;
    e->weight_bytes += bq + bo + bg + bd + 2 * h * 4;
    return 0;
  }
  if (int rc = e->alloc((void**)&L.qkv, (h + 2 * kv) * h * 2)) return rc;
  if (int rc = e->alloc((void**)&L.o, h * h * 2)) return rc;
  if (int rc = e->alloc((void**)&L.gu, 2 * ff * h * 2)) return rc;
  if (int rc = e->alloc((void**)&L.down, h * ff * 2)) return rc;
  if (int rc = e->alloc((void**)&L.attn_norm, h * 4)) return rc;
  if (int rc = e->alloc((void**)&L.ffn_norm, h * 4)) return rc;
  e->weight_bytes += ((h + 2 * kv) * h + h * h + 3 * ff * h) * 2 + 2 * h * 4;
  return 0;
}

// K-quant layer: segments from the seven matrix types (L_Q, L_K, L_V, L_O, L_GATE == L_UP, L_DOWN)
static int alloc_layer_kq(mx_engine* e, Layer& L, const int t[9]) {
  const int h = e->n_embd, kv = e->n_embd_kv, ff = e->n_ff;
  L.kq_qkv = L.kq_o = L.kq_gu = L.kq_down = KqMat();
  L.kq_qkv.add(t[L_Q], h, h);
  L.kq_qkv.add(t[L_K], kv, h);
  L.kq_qkv.add(t[L_V], kv, h);
  L.kq_o.add(t[L_O], h, h);
  if (t[L_GATE] != t[L_UP]) return fail(MX_ERR_MODEL, "ffn_gate and ffn_up of different K-quant types");
  L.kq_gu.add(t[L_GATE], 2 * ff, h);
  L.kq_down.add(t[L_DOWN], h, ff);
  if (int rc = e->alloc((void**)&L.qkv, L.kq_qkv.bytes)) return rc;
  if (int rc = e->alloc((void**)&L.o, L.kq_o.bytes)) return rc;
  if (int rc = e->alloc((void**)&L.gu, L.kq_gu.bytes)) return rc;
  if (int rc = e->alloc((void**)&L.down, L.kq_down.bytes)) return rc;
  if (int rc = e->alloc((void**)&L.attn_norm, (size_t)h * 4)) return rc;
  if (int rc = e->alloc((void**)&L.ffn_norm, (size_t)h * 4)) return rc;
  e->weight_bytes += L.kq_qkv.bytes + L.kq_o.bytes + L.kq_gu.bytes + L.kq_down.bytes + 2 * (size_t)h * 4;
  return 0;
}

// pack GGUF blocks of `rows` logical rows into a K-quant matrix at packed row `row0` (mode as launch_pack)
static int pack_kq_rows(const KqMat& km, uint16_t* base, const uint8_t* blocks, int type, int rows, int K, int mode,
                        int row0, hipStream_t s) {
  int in_seg = 0;
  const int sg = km.seg(row0, &in_seg);
  if (km.type[sg] != type) return -1;
  return launch_pack_kq((uint8_t*)base + km.off[sg], blocks, type, rows, K, mode, in_seg, s);
}

int mx_engine::load_synthetic(const Shape& s, uint64_t seed, bool q8, int kq_base, bool q4) {
  n_embd = s.n_embd; n_layer = s.n_layer; n_head = s.n_head; n_head_kv = s.n_head_kv; n_ff = s.n_ff;
  n_vocab = s.n_vocab; rope_base = s.rope_base; eps = s.eps; n_ctx_train = s.n_ctx_train;
  if (le < 0 || le > n_layer) le = n_layer;
  wq8 = embd_q8 = out_q8 = q8 || q4;
  wq4 = q4;  // layer matrices Q4_0 (quantize_row_q4_0_ref of the bf16 synthetic values); embd / output Q8_0
  wkq = kq_base != 0;
  if (int rc = init_common()) return rc;
  const float ws = std_scale(0.02), ns = std_scale(0.1);
  const int h = n_embd, kv = n_embd_kv, ff = n_ff, V = n_vocab;
  if (wkq) {  // synth.py kq_tensor: the recipe's types, synthetic GGUF blocks packed like a file's
    kq_main_type = kq_base;
    const int bb_max = kq_block_bytes(14) > kq_block_bytes(kq_base) ? kq_block_bytes(14) : kq_block_bytes(kq_base);
    const size_t stage_bytes = std::max({(size_t)V * h, (size_t)ff * h, (size_t)h * h}) / 256 * bb_max;
    uint8_t* stage = nullptr;
    HIPC(hipMalloc((void**)&stage, stage_bytes));
    int rc = 0;
    auto mat = [&](const KqMat& km, uint16_t* base, int type, uint64_t tid, int rows, int K, int mode, int row0) -> int {
      if (launch_synth_kq_blocks(stage, type, (size_t)rows * K / 256, seed, tid, stream)) return fail(MX_ERR_ARG, "synth kq");
      if (pack_kq_rows(km, base, stage, type, rows, K, mode, row0, stream)) return fail(MX_ERR_ARG, "pack kq");
      return 0;
    };
    if (has_embed) {
      embd_kq_type = kq_base;
      if ((rc = alloc((void**)&tok_embd_kq, (size_t)V * (h / 256) * kq_block_bytes(kq_base)))) goto kq_out_label;
      launch_synth_kq_blocks(tok_embd_kq, kq_base, (size_t)V * h / 256, seed, TID_TOK_EMBD, stream);
      weight_bytes += (size_t)(h / 256) * kq_block_bytes(kq_base);
    }
    if (has_head) {
      kq_out = KqMat();
      kq_out.add(kq_recipe_type(kq_base, -1, 0, n_layer), V, h);
      if ((rc = alloc((void**)&output, kq_out.bytes)) || (rc = alloc((void**)&out_norm, (size_t)h * 4))) goto kq_out_label;
      if ((rc = mat(kq_out, output, kq_out.type[0], TID_OUTPUT, V, h, PACK_ROWS, 0))) goto kq_out_label;
      launch_synth_norm(out_norm, h, seed, TID_OUT_NORM, ns, stream);
      weight_bytes += kq_out.bytes + h * 4;
    }
    for (int l = lb; l < le && !rc; l++) {
      Layer& L = layers[l - lb];
      int t[9] = {0};
      for (int k : {L_Q, L_K, L_V, L_O, L_GATE, L_UP, L_DOWN}) t[k] = kq_recipe_type(kq_base, k, l, n_layer);
      if ((rc = alloc_layer_kq(this, L, t))) break;
      launch_synth_norm(L.attn_norm, h, seed, layer_tid(l, L_ATTN_NORM), ns, stream);
      launch_synth_norm(L.ffn_norm, h, seed, layer_tid(l, L_FFN_NORM), ns, stream);
      if ((rc = mat(L.kq_qkv, L.qkv, t[L_Q], layer_tid(l, L_Q), h, h, PACK_ROWS, 0)) ||
          (rc = mat(L.kq_qkv, L.qkv, t[L_K], layer_tid(l, L_K), kv, h, PACK_ROWS, h)) ||
          (rc = mat(L.kq_qkv, L.qkv, t[L_V], layer_tid(l, L_V), kv, h, PACK_ROWS, h + kv)) ||
          (rc = mat(L.kq_o, L.o, t[L_O], layer_tid(l, L_O), h, h, PACK_ROWS, 0)) ||
          (rc = mat(L.kq_gu, L.gu, t[L_GATE], layer_tid(l, L_GATE), ff, h, PACK_GATE, 0)) ||
          (rc = mat(L.kq_gu, L.gu, t[L_UP], layer_tid(l, L_UP), ff, h, PACK_UP, 0)) ||
          (rc = mat(L.kq_down, L.down, t[L_DOWN], layer_tid(l, L_DOWN), h, ff, PACK_ROWS, 0)))
        break;
    }
  kq_out_label:
    hipStreamSynchronize(stream);
    hipFree(stage);
    if (rc) return rc;
    HIPC(hipGetLastError());
    return 0;
  }
  if (wq8) {  // the Q8_0 (Q4_0) quantisation of the bf16 synthetic model (what llama-quantize makes of it)
    if (has_embed) {
      if (int rc = alloc((void**)&tok_embd8, (size_t)V * (h / 32) * 34)) return rc;
      launch_synth_q8_rowmajor(tok_embd8, V, h, seed, TID_TOK_EMBD, ws, stream);
      weight_bytes += (size_t)h / 32 * 34;
    }
    if (has_head) {
      if (int rc = alloc((void**)&output, q8_matrix_bytes(V, h))) return rc;
      if (int rc = alloc((void**)&out_norm, (size_t)h * 4)) return rc;
      launch_synth_q8_packed((uint8_t*)output, V, h, seed, TID_OUTPUT, ws, PACK_ROWS, 0, stream);
      launch_synth_norm(out_norm, h, seed, TID_OUT_NORM, ns, stream);
      weight_bytes += q8_matrix_bytes(V, h) + h * 4;
    }
    for (int l = lb; l < le; l++) {
      Layer& L = layers[l - lb];
      if (int rc = alloc_layer(this, L)) return rc;
      uint8_t *qkv = (uint8_t*)L.qkv, *o = (uint8_t*)L.o, *gu = (uint8_t*)L.gu, *dn = (uint8_t*)L.down;
      launch_synth_norm(L.attn_norm, h, seed, layer_tid(l, L_ATTN_NORM), ns, stream);
      launch_synth_norm(L.ffn_norm, h, seed, layer_tid(l, L_FFN_NORM), ns, stream);
      auto syn = q4 ? launch_synth_q4_packed : launch_synth_q8_packed;
      syn(qkv, h, h, seed, layer_tid(l, L_Q), ws, PACK_ROWS, 0, stream);
      syn(qkv, kv, h, seed, layer_tid(l, L_K), ws, PACK_ROWS, h, stream);
      syn(qkv, kv, h, seed, layer_tid(l, L_V), ws, PACK_ROWS, h + kv, stream);
      syn(o, h, h, seed, layer_tid(l, L_O), ws, PACK_ROWS, 0, stream);
      syn(gu, ff, h, seed, layer_tid(l, L_GATE), ws, PACK_GATE, 0, stream);
      syn(gu, ff, h, seed, layer_tid(l, L_UP), ws, PACK_UP, 0, stream);
      syn(dn, h, ff, seed, layer_tid(l, L_DOWN), ws, PACK_ROWS, 0, stream);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(stream));
    return 0;
  }
  if (has_embed) {
    if (int rc = alloc((void**)&tok_embd, (size_t)V * h * 2)) return rc;
    launch_synth_rowmajor(tok_embd, (size_t)V * h, seed, TID_TOK_EMBD, ws, stream);
    weight_bytes += (size_t)h * 2;  // one embedding row per token
  }
  if (has_head) {
    if (int rc = alloc((void**)&output, (size_t)V * h * 2)) return rc;
    if (int rc = alloc((void**)&out_norm, (size_t)h * 4)) return rc;
    launch_synth_packed(output, V, h, seed, TID_OUTPUT, ws, PACK_ROWS, 0, stream);
    launch_synth_norm(out_norm, h, seed, TID_OUT_NORM, ns, stream);
    weight_bytes += (size_t)V * h * 2 + h * 4;
  }
  for (int l = lb; l < le; l++) {
    Layer& L = layers[l - lb];
    if (int rc = alloc_layer(this, L)) return rc;
    launch_synth_norm(L.attn_norm, h, seed, layer_tid(l, L_ATTN_NORM), ns, stream);
    launch_synth_norm(L.ffn_norm, h, seed, layer_tid(l, L_FFN_NORM), ns, stream);
    launch_synth_packed(L.qkv, h, h, seed, layer_tid(l, L_Q), ws, PACK_ROWS, 0, stream);
    launch_synth_packed(L.qkv, kv, h, seed, layer_tid(l, L_K), ws, PACK_ROWS, h, stream);
    launch_synth_packed(L.qkv, kv, h, seed, layer_tid(l, L_V), ws, PACK_ROWS, h + kv, stream);
    launch_synth_packed(L.o, h, h, seed, layer_tid(l, L_O), ws, PACK_ROWS, 0, stream);
    launch_synth_packed(L.gu, ff, h, seed, layer_tid(l, L_GATE), ws, PACK_GATE, 0, stream);
    launch_synth_packed(L.gu, ff, h, seed, layer_tid(l, L_UP), ws, PACK_UP, 0, stream);
    launch_synth_packed(L.down, h, ff, seed, layer_tid(l, L_DOWN), ws, PACK_ROWS, 0, stream);
  }
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(stream));
  return 0;
}

int mx_engine::load_gguf(const std::string& path) {
  GGUFFile f;
  std::string err = f.open(path);
  if (!err.empty()) return fail(MX_ERR_MODEL, err);
  const GGUFValue* arch = f.get("general.architecture");
  if (!arch || (arch->str != "llama" && arch->str != "qwen2"))
    return fail(MX_ERR_MODEL, "general.architecture must be 'llama' or 'qwen2', got '" + (arch ? arch->str : "") + "'");
  const std::string A = arch->str + ".";  // every hyper-parameter is keyed by the architecture
  // qwen2: NeoX RoPE, run as the kernels' adjacent-pair RoPE on attn_q / attn_k rows permuted at load
  const bool neox = arch->str == "qwen2";
  n_embd = (int)f.get_num(A + "embedding_length", 0);
  n_layer = (int)f.get_num(A + "block_count", 0);
  n_head = (int)f.get_num(A + "attention.head_count", 0);
  n_head_kv = (int)f.get_num(A + "attention.head_count_kv", n_head);
  n_ff = (int)f.get_num(A + "feed_forward_length", 0);
  eps = (float)f.get_num(A + "attention.layer_norm_rms_epsilon", 1e-5);
  rope_base = (float)f.get_num(A + "rope.freq_base", 10000.0);
  n_ctx_train = (int)f.get_num(A + "context_length", 2048);
  bos = (int)f.get_num("tokenizer.ggml.bos_token_id", 1);
  eos = (int)f.get_num("tokenizer.ggml.eos_token_id", 2);
  eot = (int)f.get_num("tokenizer.ggml.eot_token_id", -1);
  const GGUFTensor* te = f.tensor("token_embd.weight");
  if (!te || te->ne.size() != 2) return fail(MX_ERR_MODEL, "missing token_embd.weight");
  n_vocab = (int)te->ne[1];
  if (!n_embd || !n_layer || !n_head || !n_ff) return fail(MX_ERR_MODEL, "missing " + A + "* hyper-parameters");
  if ((int)f.get_num(A + "rope.dimension_count", n_embd / n_head) != n_embd / n_head)
    return fail(MX_ERR_MODEL, "partial RoPE (rope.dimension_count != head_dim) is not supported");
  {  // RoPE scaling: llama.cpp's "linear" (freq_scale = 1/factor) and Llama-3.1 frequency factors
    const GGUFValue* st = f.get(A + "rope.scaling.type");
    const std::string stype = st ? st->str : "none";
    const double factor = f.get_num(A + "rope.scaling.factor", 0.0);
    if (stype == "linear") {
      if (!(factor > 0)) return fail(MX_ERR_MODEL, "linear RoPE scaling without a positive factor");
      rope_freq_scale = (float)(1.0 / factor);
    } else if (stype != "none" && !stype.empty()) {
      return fail(MX_ERR_MODEL, "RoPE scaling type '" + stype + "' is not supported (none, linear and rope_freqs are)");
    }
    if (const GGUFTensor* rf = f.tensor("rope_freqs.weight")) {
      const int half = n_embd / n_head / 2;
      if (rf->type != 0 || rf->ne.size() != 1 || (int)rf->ne[0] != half)
        return fail(MX_ERR_MODEL, "rope_freqs.weight must be f32 [head_dim/2]");
      rope_ff.resize(half);
      memcpy(rope_ff.data(), f.data(*rf), half * 4);
      for (float v : rope_ff)
        if (!(v > 0)) return fail(MX_ERR_MODEL, "rope_freqs.weight has a non-positive factor");
    }
  }
  if (le < 0 || le > n_layer) le = n_layer;
  // Matrix types.  All BF16 -> the bf16 path; all Q8_0 -> the Q8_0 path (int8 MFMA on the blocks);
  // all Q4_K / Q5_K / Q6_K with ffn_gate and ffn_up of one type (llama.cpp's Q4_K_M, Q5_K_M files) ->
  // the K-quant path (kquant.hip: int8 MFMA on the blocks with Q8_K activations); any other mix of
  // F32 / F16 / BF16 / Q4_0 / Q8_0 / K-quants -> every matrix is dequantised to bf16 at load
  // (ggml's dequantize_row_*) and runs on the bf16 path.
  bool deq = false;
  size_t raw_max = 0;
  {
    const int b0 = lb < 0 ? 0 : lb, e0 = (le < 0 || le > n_layer) ? n_layer : le;
    std::vector<std::string> mats;
    static const char* kinds[] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"};
    for (int l = b0; l < e0; l++)
      for (const char* k : kinds) mats.push_back("blk." + std::to_string(l) + "." + k + ".weight");
    if (e0 == n_layer) mats.push_back(f.tensor("output.weight") ? "output.weight" : "token_embd.weight");
    int n8 = 0, n30 = 0, nkq = 0, n4 = 0;
    for (const std::string& nm : mats) {
      const GGUFTensor* t = f.tensor(nm);
      if (!t) return fail(MX_ERR_MODEL, "missing tensor " + nm);
      if (t->type != 30 && !ggml_block_elems(t->type))
        return fail(MX_ERR_MODEL, "tensor " + nm + ": ggml type " + std::to_string(t->type) +
                                      " is not supported (F32, F16, BF16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K are)");
      n8 += t->type == 8;
      n4 += t->type == 2 && nm != mats.back();  // layer matrices only (the head is checked below)
      n30 += t->type == 30;
      nkq += t->type == 12 || t->type == 13 || t->type == 14;
      raw_max = std::max(raw_max, (size_t)t->nbytes);
    }
    wq8 = out_q8 = n8 == (int)mats.size();
    if (!wq8 && n4 == (int)mats.size() - (e0 == n_layer ? 1 : 0) && n4 > 0) {
      // Q4_0 layers; the head: Q8_0 / Q4_0 tiles, or a K-quant output (llama-quantize's Q6_K) on the
      // K-quant kernels -- anything else dequantises the whole model as before
      const int ot = e0 == n_layer ? f.tensor(mats.back())->type : 8;
      if (ot == 8 || ot == 2 || ((ot == 12 || ot == 13 || ot == 14) && n_embd % 256 == 0)) {
        wq8 = wq4 = true;
        out_q8 = ot == 8 || ot == 2;
        out_q4 = ot == 2;
        out_kq_head = !out_q8;
      }
    }
    wkq = nkq == (int)mats.size() && n_embd % 256 == 0 && n_ff % 256 == 0;
    for (int l = b0; l < e0 && wkq; l++) {
      const std::string p = "blk." + std::to_string(l) + ".";
      if (f.tensor(p + "ffn_gate.weight")->type != f.tensor(p + "ffn_up.weight")->type) wkq = false;
    }
    if (wkq) kq_main_type = f.tensor("blk." + std::to_string(b0) + ".ffn_gate.weight")->type;
    deq = !wq8 && !wkq && n30 != (int)mats.size();
    if (wq8 && !out_q8) deq = false;
    embd_q8 = te->type == 8;
    if (wkq && (te->type == 12 || te->type == 13 || te->type == 14)) embd_kq_type = te->type;
    if (lora) {
      // an adapter is merged into bf16 matrices: the native Q8_0 / Q4_0 / K-quant paths are off and every
      // matrix, token_embd included, is dequantised to bf16 at load -- the model a BF16 file of the merged
      // weights would give
      wq8 = out_q8 = wq4 = out_q4 = out_kq_head = wkq = embd_q8 = false;
      kq_main_type = embd_kq_type = 0;
      deq = n30 != (int)mats.size();
    }
    if (te->type != 30 && !embd_q8) {
      if (!ggml_block_elems(te->type))
        return fail(MX_ERR_MODEL, "token_embd.weight: ggml type " + std::to_string(te->type) + " is not supported");
      raw_max = std::max(raw_max, (size_t)te->nbytes);
    }
  }
  // q/k/v biases (qwen2; llama.cpp reads them for llama too): all three of a layer, F32 [h], [kv], [kv], or none
  std::vector<char> has_bias;
  {
    const int b0 = lb < 0 ? 0 : lb, e0 = (le < 0 || le > n_layer) ? n_layer : le;
    const int hd = n_head ? n_embd / n_head : 0;
    for (int l = b0; l < e0; l++) {
      static const char* nm[3] = {"attn_q.bias", "attn_k.bias", "attn_v.bias"};
      int n = 0;
      for (int k = 0; k < 3; k++) {
        const std::string name = "blk." + std::to_string(l) + "." + nm[k];
        const GGUFTensor* t = f.tensor(name);
        if (!t) continue;
        n++;
        const uint64_t want = k == 0 ? (uint64_t)n_embd : (uint64_t)hd * n_head_kv;
        if (t->type != 0) return fail(MX_ERR_MODEL, "tensor " + name + " must be F32, got ggml type " + std::to_string(t->type));
        if (t->ne.size() != 1 || t->ne[0] != want)
          return fail(MX_ERR_MODEL, "tensor " + name + " must have " + std::to_string(want) + " elements");
      }
      if (n != 0 && n != 3)
        return fail(MX_ERR_MODEL, "blk." + std::to_string(l) + ": attn_q.bias, attn_k.bias and attn_v.bias come together or not at all");
      has_bias.push_back(n == 3);
    }
  }
  if (int rc = init_common()) return rc;
  const int h = n_embd, kv = n_embd_kv, ff = n_ff, V = n_vocab;
  const int mat_type = wq4 ? 2 : wq8 ? 8 : 30;

  // staging buffer for the largest matrix (bf16), and for the raw blocks of dequantised tensors
  size_t stage_bytes = std::max({(size_t)V * h * 2, (size_t)ff * h * 2, (size_t)(h + 2 * kv) * h * 2});
  uint16_t* stage = nullptr;
  uint8_t* stage_raw = nullptr;
  uint8_t* stage_perm = nullptr;  // neox: attn_q / attn_k with their rows permuted, what the pack kernels then read
  HIPC(hipMalloc((void**)&stage, stage_bytes));
  if (neox && hipMalloc((void**)&stage_perm, std::max((size_t)h * h * 2, raw_max)) != hipSuccess) {
    hipFree(stage);
    return fail(MX_ERR_HIP, "staging buffer");
  }
  if (raw_max && (deq || wkq || out_kq_head || (te->type != 30 && !embd_q8))) {
    if (hipMalloc((void**)&stage_raw, raw_max) != hipSuccess) {
      hipFree(stage);
      if (stage_perm) hipFree(stage_perm);
      return fail(MX_ERR_HIP, "staging buffer");
    }
  }
  // the largest A and B of the adapter's pairs in this stage's layers, as f32
  float *lora_a = nullptr, *lora_b = nullptr;
  std::vector<float> lora_host;
  if (lora && lora_scale != 0.f) {
    size_t amax = 0, bmax = 0;
    for (const auto& kvp : lora->pairs) {
      const LoraPair& p = kvp.second;
      if (p.layer < lb || p.layer >= le) continue;
      amax = std::max(amax, (size_t)p.r * p.n_in);
      bmax = std::max(bmax, (size_t)p.r * p.n_out);
    }
    if (amax && (hipMalloc((void**)&lora_a, amax * 4) != hipSuccess || hipMalloc((void**)&lora_b, bmax * 4) != hipSuccess)) {
      hipFree(stage);
      if (stage_raw) hipFree(stage_raw);
      if (stage_perm) hipFree(stage_perm);
      if (lora_a) hipFree(lora_a);
      return fail(MX_ERR_HIP, "LoRA staging buffers");
    }
    lora_host.resize(std::max(amax, bmax));
  }
  // any supported type -> bf16 row-major in `stage`
  auto to_bf16 = [&](const GGUFTensor* t, size_t n) -> int {
    if (t->type == 30) {
      HIPC(hipMemcpy(stage, f.data(*t), t->nbytes, hipMemcpyHostToDevice));
      return 0;
    }
    HIPC(hipMemcpy(stage_raw, f.data(*t), t->nbytes, hipMemcpyHostToDevice));
    if (launch_dequant_bf16(stage, stage_raw, t->type, n, stream)) return fail(MX_ERR_MODEL, "dequantise " + t->name);
    return 0;
  };
  // neox: the row-major image of attn_q / attn_k at `src` (bf16, or the raw blocks of each row) with its rows
  // permuted into stage_perm; every other tensor, and every tensor of a llama file, is packed from where it is
  auto qk_rows = [&](const std::string& name, const void* src, int rows, size_t nbytes, const void** out) -> int {
    *out = src;
    const size_t n = name.size();
    const bool qk = n > 14 && (name.compare(n - 14, 14, ".attn_q.weight") == 0 || name.compare(n - 14, 14, ".attn_k.weight") == 0);
    if (!neox || !qk) return 0;
    if (nbytes % rows || launch_permute_rows_neox(stage_perm, src, rows, nbytes / rows, head_dim, stream))
      return fail(MX_ERR_MODEL, "tensor " + name + ": rows cannot be permuted");
    *out = stage_perm;
    return 0;
  };
  auto get_mat = [&](const std::string& name, int rows, int cols, const GGUFTensor** out, int type) -> int {
    const GGUFTensor* t = f.tensor(name);
    if (!t) return fail(MX_ERR_MODEL, "missing tensor " + name);
    if (t->ne.size() != 2 || (int)t->ne[0] != cols || (int)t->ne[1] != rows)
      return fail(MX_ERR_MODEL, "tensor " + name + " has unexpected shape");
    if (t->type != type && !(deq && type == 30))
      return fail(MX_ERR_MODEL, "tensor " + name + ": expected ggml type " + std::to_string(type) +
                                    (type == 8 ? " (Q8_0, like the other matrices)"
                                     : type == 2 ? " (Q4_0, like the other matrices)" : " (BF16, like the other matrices)") +
                                    ", got type " + std::to_string(t->type));
    *out = t;
    return 0;
  };
  auto upload_packed = [&](const std::string& name, int rows, int cols, uint16_t* dst, int mode,
                           int offset) -> int {
    const GGUFTensor* t = nullptr;
    if (int rc = get_mat(name, rows, cols, &t, mat_type)) return rc;
    if (wq8) {
      HIPC(hipMemcpy(stage, f.data(*t), t->nbytes, hipMemcpyHostToDevice));
      const void* src = nullptr;
      if (int rc = qk_rows(name, stage, rows, t->nbytes, &src)) return rc;
      if (t->type == 2) launch_pack_q4((uint8_t*)dst, (const uint8_t*)src, rows, cols, mode, offset, stream);
      else launch_pack_q8((uint8_t*)dst, (const uint8_t*)src, rows, cols, mode, offset, stream);
    } else {
      if (int rc = to_bf16(t, (size_t)rows * cols)) return rc;
      if (lora_a) {  // W' = bf16(W + scale B A) on the row-major matrix, before it is packed
        const auto it = lora->pairs.find(name);
        if (it != lora->pairs.end()) {
          const LoraPair& p = it->second;
          if (p.n_in != cols || p.n_out != rows) return fail(MX_ERR_MODEL, "LoRA adapter: shape of " + name);
          lora->to_f32(*p.a, lora_host.data());
          HIPC(hipMemcpy(lora_a, lora_host.data(), (size_t)p.r * cols * 4, hipMemcpyHostToDevice));
          lora->to_f32(*p.b, lora_host.data());
          HIPC(hipMemcpy(lora_b, lora_host.data(), (size_t)p.r * rows * 4, hipMemcpyHostToDevice));
          if (launch_lora_merge(stage, lora_a, lora_b, rows, cols, p.r, lora->scale(p, lora_scale), stream))
            return fail(MX_ERR_MODEL, "LoRA merge of " + name);
          lora_merged++;
          lora_rank_max = std::max(lora_rank_max, p.r);
        }
      }
      const void* src = nullptr;  // dequantise -> merge -> permute -> pack: the adapter's B rows are in file order
      if (int rc = qk_rows(name, stage, rows, (size_t)rows * cols * 2, &src)) return rc;
      launch_pack(dst, (const uint16_t*)src, rows, cols, mode, offset, stream);
    }
    HIPC(hipStreamSynchronize(stream));
    return 0;
  };
  auto upload_norm = [&](const std::string& name, float* dst) -> int {
    const GGUFTensor* t = f.tensor(name);
    if (!t || t->type != 0 || t->ne[0] != (uint64_t)h) return fail(MX_ERR_MODEL, "bad/missing f32 norm " + name);
    HIPC(hipMemcpy(dst, f.data(*t), (size_t)h * 4, hipMemcpyHostToDevice));
    return 0;
  };
  // K-quant matrix: raw blocks to the device, packed into the segment holding packed row row0
  auto upload_kq = [&](const std::string& name, int rows, int cols, const KqMat& km, uint16_t* dst, int mode,
                       int row0) -> int {
    const GGUFTensor* t = f.tensor(name);
    if (!t) return fail(MX_ERR_MODEL, "missing tensor " + name);
    if (t->ne.size() != 2 || (int)t->ne[0] != cols || (int)t->ne[1] != rows)
      return fail(MX_ERR_MODEL, "tensor " + name + " has unexpected shape");
    HIPC(hipMemcpy(stage_raw, f.data(*t), t->nbytes, hipMemcpyHostToDevice));
    const void* src = nullptr;
    if (int rc = qk_rows(name, stage_raw, rows, t->nbytes, &src)) return rc;
    if (pack_kq_rows(km, dst, (const uint8_t*)src, t->type, rows, cols, mode, row0, stream))
      return fail(MX_ERR_MODEL, "tensor " + name + ": K-quant type does not match its matrix segment");
    HIPC(hipStreamSynchronize(stream));
    return 0;
  };
  // the layer's q|k|v bias as one f32 vector in the packed QKV row order (neox: q and k permuted like their rows)
  auto upload_bias = [&](int l, Layer& L) -> int {
    if (!has_bias[l - lb]) return 0;
    const std::string p = "blk." + std::to_string(l) + ".";
    std::vector<float> b((size_t)h + 2 * kv);
    const int off[3] = {0, h, h + kv}, len[3] = {h, kv, kv};
    static const char* nm[3] = {"attn_q.bias", "attn_k.bias", "attn_v.bias"};
    for (int k = 0; k < 3; k++) {
      const float* src = reinterpret_cast<const float*>(f.data(*f.tensor(p + nm[k])));
      const int d = head_dim;
      for (int r = 0; r < len[k]; r++) {
        const int rr = r % d;
        const int sr = (neox && k < 2) ? r - rr + (rr & 1) * (d / 2) + (rr >> 1) : r;
        memcpy(&b[off[k] + r], src + sr, 4);
      }
    }
    if (int rc = alloc((void**)&L.qkv_bias, b.size() * 4)) return rc;
    HIPC(hipMemcpy(L.qkv_bias, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    weight_bytes += b.size() * 4;
    return 0;
  };
  auto kq_layer_types = [&](int l, int t[9]) {
    const std::string p = "blk." + std::to_string(l) + ".";
    static const char* nm[9] = {nullptr, "attn_q", "attn_k", "attn_v", "attn_output", nullptr, "ffn_gate", "ffn_up", "ffn_down"};
    for (int k = 0; k < 9; k++) t[k] = nm[k] ? f.tensor(p + nm[k] + ".weight")->type : 0;
  };
  int rc = 0;
  if (wkq) {
    if (has_embed) {
      const GGUFTensor* t = f.tensor("token_embd.weight");
      if (t->ne.size() != 2 || (int)t->ne[0] != h || (int)t->ne[1] != V) {
        rc = fail(MX_ERR_MODEL, "tensor token_embd.weight has unexpected shape");
        goto out;
      }
      if (embd_kq_type) {  // GET_ROWS dequantises the blocks per lookup (dequantize_row_q*_K)
        if ((rc = alloc((void**)&tok_embd_kq, t->nbytes))) goto out;
        if (hipMemcpy(tok_embd_kq, f.data(*t), t->nbytes, hipMemcpyHostToDevice) != hipSuccess) {
          rc = fail(MX_ERR_HIP, "upload token_embd");
          goto out;
        }
        weight_bytes += t->nbytes / V;
      } else if (t->type == 30 || t->type == 8) {  // BF16 rows as stored; Q8_0 rows dequantised per lookup
        void** dst = embd_q8 ? (void**)&tok_embd8 : (void**)&tok_embd;
        if ((rc = alloc(dst, t->nbytes))) goto out;
        if (hipMemcpy(*dst, f.data(*t), t->nbytes, hipMemcpyHostToDevice) != hipSuccess) {
          rc = fail(MX_ERR_HIP, "upload token_embd");
          goto out;
        }
        weight_bytes += t->nbytes / V;
      } else {  // F32 / F16 / Q4_0 / ... (llama-quantize --token-embedding-type): a bf16 table once
        if ((rc = alloc((void**)&tok_embd, (size_t)V * h * 2))) goto out;
        if ((rc = to_bf16(t, (size_t)V * h))) goto out;
        if (hipMemcpyAsync(tok_embd, stage, (size_t)V * h * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
          rc = fail(MX_ERR_HIP, "upload token_embd");
          goto out;
        }
        weight_bytes += (size_t)h * 2;
      }
    }
    if (has_head) {
      const char* oname = f.tensor("output.weight") ? "output.weight" : "token_embd.weight";  // tied embeddings
      kq_out = KqMat();
      kq_out.add(f.tensor(oname)->type, V, h);
      if ((rc = alloc((void**)&output, kq_out.bytes))) goto out;
      if ((rc = alloc((void**)&out_norm, (size_t)h * 4))) goto out;
      if ((rc = upload_kq(oname, V, h, kq_out, output, PACK_ROWS, 0))) goto out;
      if ((rc = upload_norm("output_norm.weight", out_norm))) goto out;
      weight_bytes += kq_out.bytes + h * 4;
    }
    for (int l = lb; l < le; l++) {
      Layer& L = layers[l - lb];
      const std::string p = "blk." + std::to_string(l) + ".";
      int t[9];
      kq_layer_types(l, t);
      if ((rc = alloc_layer_kq(this, L, t))) goto out;
      if ((rc = upload_norm(p + "attn_norm.weight", L.attn_norm))) goto out;
      if ((rc = upload_norm(p + "ffn_norm.weight", L.ffn_norm))) goto out;
      if ((rc = upload_bias(l, L))) goto out;
      if ((rc = upload_kq(p + "attn_q.weight", h, h, L.kq_qkv, L.qkv, PACK_ROWS, 0))) goto out;
      if ((rc = upload_kq(p + "attn_k.weight", kv, h, L.kq_qkv, L.qkv, PACK_ROWS, h))) goto out;
      if ((rc = upload_kq(p + "attn_v.weight", kv, h, L.kq_qkv, L.qkv, PACK_ROWS, h + kv))) goto out;
      if ((rc = upload_kq(p + "attn_output.weight", h, h, L.kq_o, L.o, PACK_ROWS, 0))) goto out;
      if ((rc = upload_kq(p + "ffn_gate.weight", ff, h, L.kq_gu, L.gu, PACK_GATE, 0))) goto out;
      if ((rc = upload_kq(p + "ffn_up.weight", ff, h, L.kq_gu, L.gu, PACK_UP, 0))) goto out;
      if ((rc = upload_kq(p + "ffn_down.weight", h, ff, L.kq_down, L.down, PACK_ROWS, 0))) goto out;
    }
    goto out;
  }
  if (has_embed) {
    const GGUFTensor* t = f.tensor("token_embd.weight");
    if (t->ne.size() != 2 || (int)t->ne[0] != h || (int)t->ne[1] != V) {
      rc = fail(MX_ERR_MODEL, "tensor token_embd.weight has unexpected shape");
      goto out;
    }
    if (t->type == 30 || embd_q8) {  // rows used as stored (Q8_0 rows dequantised per lookup)
      void** dst = embd_q8 ? (void**)&tok_embd8 : (void**)&tok_embd;
      if ((rc = alloc(dst, t->nbytes))) goto out;
      if (hipMemcpy(*dst, f.data(*t), t->nbytes, hipMemcpyHostToDevice) != hipSuccess) {
        rc = fail(MX_ERR_HIP, "upload token_embd");
        goto out;
      }
      weight_bytes += t->nbytes / V;
    } else {  // other block types: dequantised to a bf16 table once
      if ((rc = alloc((void**)&tok_embd, (size_t)V * h * 2))) goto out;
      if ((rc = to_bf16(t, (size_t)V * h))) goto out;
      if (hipMemcpyAsync(tok_embd, stage, (size_t)V * h * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess) {
        rc = fail(MX_ERR_HIP, "upload token_embd");
        goto out;
      }
      weight_bytes += (size_t)h * 2;
    }
  }
  if (has_head) {
    const char* oname = f.tensor("output.weight") ? "output.weight" : "token_embd.weight";  // tied embeddings
    if ((rc = alloc((void**)&out_norm, (size_t)h * 4))) goto out;
    if ((rc = upload_norm("output_norm.weight", out_norm))) goto out;
    if (out_kq_head) {  // Q4_0 model with a K-quant output: packed K-quant tiles for mkq
      kq_out = KqMat();
      kq_out.add(f.tensor(oname)->type, V, h);
      if ((rc = alloc((void**)&output, kq_out.bytes))) goto out;
      if ((rc = upload_kq(oname, V, h, kq_out, output, PACK_ROWS, 0))) goto out;
      weight_bytes += kq_out.bytes + h * 4;
    } else {
      const size_t ob = out_q4 ? q4_matrix_bytes(V, h) : wq8 ? q8_matrix_bytes(V, h) : (size_t)V * h * 2;
      if ((rc = alloc((void**)&output, ob))) goto out;
      const GGUFTensor* ot = nullptr;
      if (wq8) {  // the head keeps its own block type (Q8_0 or Q4_0 tiles)
        ot = f.tensor(oname);
        if (!ot || ot->ne.size() != 2 || (int)ot->ne[0] != h || (int)ot->ne[1] != V) {
          rc = fail(MX_ERR_MODEL, "tensor output.weight has unexpected shape");
          goto out;
        }
        if (hipMemcpy(stage, f.data(*ot), ot->nbytes, hipMemcpyHostToDevice) != hipSuccess) {
          rc = fail(MX_ERR_HIP, "upload output");
          goto out;
        }
        if (out_q4) launch_pack_q4((uint8_t*)output, (const uint8_t*)stage, V, h, PACK_ROWS, 0, stream);
        else launch_pack_q8((uint8_t*)output, (const uint8_t*)stage, V, h, PACK_ROWS, 0, stream);
        hipStreamSynchronize(stream);
      } else if ((rc = upload_packed(oname, V, h, output, PACK_ROWS, 0))) {
        goto out;
      }
      weight_bytes += ob + h * 4;
    }
  }
  for (int l = lb; l < le; l++) {
    Layer& L = layers[l - lb];
    const std::string p = "blk." + std::to_string(l) + ".";
    if ((rc = alloc_layer(this, L))) goto out;
    if ((rc = upload_norm(p + "attn_norm.weight", L.attn_norm))) goto out;
    if ((rc = upload_norm(p + "ffn_norm.weight", L.ffn_norm))) goto out;
    if ((rc = upload_bias(l, L))) goto out;
    if ((rc = upload_packed(p + "attn_q.weight", h, h, L.qkv, PACK_ROWS, 0))) goto out;
    if ((rc = upload_packed(p + "attn_k.weight", kv, h, L.qkv, PACK_ROWS, h))) goto out;
    if ((rc = upload_packed(p + "attn_v.weight", kv, h, L.qkv, PACK_ROWS, h + kv))) goto out;
    if ((rc = upload_packed(p + "attn_output.weight", h, h, L.o, PACK_ROWS, 0))) goto out;
    if ((rc = upload_packed(p + "ffn_gate.weight", ff, h, L.gu, PACK_GATE, 0))) goto out;
    if ((rc = upload_packed(p + "ffn_up.weight", ff, h, L.gu, PACK_UP, 0))) goto out;
    if ((rc = upload_packed(p + "ffn_down.weight", h, ff, L.down, PACK_ROWS, 0))) goto out;
  }
out:
  hipStreamSynchronize(stream);
  hipFree(stage);
  if (stage_raw) hipFree(stage_raw);
  if (stage_perm) hipFree(stage_perm);
  if (lora_a) hipFree(lora_a);
  if (lora_b) hipFree(lora_b);
  return rc;
}

MMArgs mx_engine::qkv_args(const Layer& L, int li, const Forward& f) const {
  MMArgs a{};
  a.W = L.qkv; a.N = n_embd + 2 * n_embd_kv; a.K = n_embd; a.M = f.M;
  a.out = q; a.ldo = n_embd; a.n_q = n_embd; a.n_kv = n_embd_kv; a.head_dim = head_dim; a.pos = f.pos; a.slot = f.slot;
  a.rope_cs = rope_cs; a.kc = kcache + layer_kv_stride * li; a.vc = vcache + layer_kv_stride * li; a.n_ctx = n_ctx;
  a.ctx_stride = ctx_stride; a.n_head_kv = n_head_kv; a.slot_stride = slot_stride;
  a.qkv_bias = L.qkv_bias;
  return a;
}

AttnArgs mx_engine::attn_args(int li, const Forward& f) const {
  AttnArgs at{};
  at.q = q; at.kc = kcache + layer_kv_stride * li; at.vc = vcache + layer_kv_stride * li; at.pos = f.pos; at.slot = f.slot;
  at.ldo = n_embd; at.M = f.M; at.n_head = n_head; at.n_head_kv = n_head_kv; at.head_dim = head_dim;
  at.n_ctx = n_ctx; at.ctx_stride = ctx_stride; at.slot_stride = slot_stride;
  at.scale = 1.0f / sqrtf((float)head_dim);
  at.qkv_bias = layers[li].qkv_bias;  // read by the FIN path alone (at.slabs)
  return at;
}

// One forward of M <= MAX_ROWS rows through this stage's layers.
int mx_engine::enqueue_forward(const Forward& f, hipStream_t s) {
  const int M = f.M, n_out = f.n_out, h = n_embd, ff = n_ff;
  const int *ids = f.ids, *rowmap = f.rowmap;
  const void* x_in = f.x_in;
  void* x_out = f.x_out;
  const bool head = f.head, argmax = f.argmax;
  const bool wide = use_wide && M > 16 && wide_shapes();
  // RMS_NORM applied on load by the consuming GEMV (M <= 16); the residual-stream writers
  // (embedding, attn_output, ffn_down, or ssq_kernel for a stage's x_in) leave per-tile partials
  const bool nol = !wide && !wq8 && !wkq && norm_on_load && mm_can_norm_on_load(M, h);
  const bool qql = q8_on_load(M) || kq_on_load(M);  // residual-stream Σx² partials wanted
  if (x_in) {
    if (handoff_bf16) {  // bf16 hand-off from the previous stage: widen, with the Σx² partials on the way
      launch_bf16_to_f32(x, (const uint16_t*)x_in, M, h, (nol || qql) ? ssq : nullptr, s);
    } else {
      launch_f32_in(x, (const float*)x_in, M, h, (nol || qql) ? ssq : nullptr, s);
    }
  } else {
    if (!has_embed) return fail(MX_ERR_STATE, "this stage has no token embedding: x_in required");
    if (embd_kq_type) {
      if (launch_embed_kq(x, tok_embd_kq, embd_kq_type, ids, M, h, qql ? ssq : nullptr, s))
        return fail(MX_ERR_ARG, "K-quant embedding");
    } else if (embd_q8) {
      launch_embed_q8(x, tok_embd8, ids, M, h, (nol || qql) ? ssq : nullptr, s);
    } else {
      launch_embed(x, tok_embd, ids, M, h, (nol || qql) ? ssq : nullptr, s);
    }
  }
  if (wkq && !kq_ggml_prefill && M > MAX_ROWS && kqd_qkv && !argmax && !(head && n_out > MAX_ROWS))
    return enqueue_forward_gemm(f, s);  // dequantised bf16 GEMMs
  // Q8_0 prefill chunks as dequantised bf16 GEMMs (llama.cpp's GPU-backend route for large batches):
  // ~5x the default's rate, but bf16 activations instead of ggml's Q8_0 rows, so opt-in
  // (MX_Q8_GEMM_PREFILL=1; tests/test_q8_gpu.py bounds its deviation)
  if (wq8 && !wq4 && q8_gemm_prefill && M > MAX_ROWS && kqd_qkv && !argmax && !(head && n_out > MAX_ROWS))
    return enqueue_forward_gemm(f, s);
  if (wkq || wq8) return enqueue_forward_quant(f, s);
  if (prefill_gemm && M <= MAX_ROWS && use_wide && gemm_shapes() && !argmax)  // small prompt chunk, GEMM order
    return enqueue_forward_wide(f, s, true);
  if (M > MAX_ROWS || (prefill_gemm && gemm_shapes() && !argmax)) {
    if (!gemm_ok() || argmax || (head && n_out > MAX_ROWS))
      return fail(MX_ERR_ARG, "forward of > 64 rows: GEMM shapes only, logits for <= 64 rows");
    return enqueue_forward_gemm(f, s);
  }
  if (wide) return enqueue_forward_wide(f, s);
  // on-load only for attn_norm -> qkv: qkv's 384 work-groups run 1.5 rounds, so its per-work-group
  // prologue costs less than a norm launch; gate/up (7 rounds) and lm_head (31) keep the norm kernel
  // (tools/kernel_probe.py, profiles/round1_norm_on_load.txt)
  auto norm_operand = [&](MMArgs& m, const float* w, bool on_load) {
    if (nol && on_load) {
      m.X = nullptr; m.xf = x; m.norm_w = w; m.eps = eps; m.ssq = ssq; m.np = h / 16;
    } else {
      launch_rmsnorm(xn, h, x, w, nullptr, M, h, eps, s);
      m.X = xn; m.ldx = h;
    }
  };
  for (int li = 0; li < (int)layers.size(); li++) {
    const Layer& L = layers[li];
    MMArgs a = qkv_args(L, li, f);
    norm_operand(a, L.attn_norm, true);
    AttnArgs at = attn_args(li, f);
    at.out = attn_out;
    const bool pers_qkv = use_pers && a.X == nullptr && mm_pers_supported(EPI_QKV, M, a.N, h);
    if ((pers_qkv ? launch_mm_pers(EPI_QKV, a, s) : -1) != 0 && launch_mm(EPI_QKV, a, s))
      return fail(MX_ERR_ARG, "qkv launch shape");
    MMArgs b{};
    b.W = L.o; b.N = h; b.K = h; b.X = attn_out; b.ldx = h; b.M = M; b.out = x; b.ldo = h;
    if (use_pers && nol && mm_pers_supported(EPI_SWIGLU, M, 2 * ff, h)) {  // partials for gate/up's norm on load
      b.ssq = ssq; b.np = h / 16;
    }
    launch_attention(at, s);
    if ((mm_pers_supported(EPI_RESID, M, h, h) ? launch_mm_pers(EPI_RESID, b, s) : -1) != 0 &&
        launch_mm(EPI_RESID, b, s))
      return fail(MX_ERR_ARG, "attn_output launch shape");
    MMArgs c{};
    c.W = L.gu; c.N = 2 * ff; c.K = h; c.M = M;
    const bool pers_gu = use_pers && nol && mm_pers_supported(EPI_SWIGLU, M, 2 * ff, h);
    norm_operand(c, L.ffn_norm, pers_gu);
    c.act = act; c.lda = ff;
    if ((pers_gu ? launch_mm_pers(EPI_SWIGLU, c, s) : -1) != 0 && launch_mm(EPI_SWIGLU, c, s))
      return fail(MX_ERR_ARG, "ffn gate/up launch shape");
    MMArgs d{};
    d.W = L.down; d.N = h; d.K = ff; d.X = act; d.ldx = ff; d.M = M; d.out = x; d.ldo = h;
    d.ssq = nol ? ssq : nullptr; d.np = h / 16;
    if ((mm_pers_supported(EPI_RESID, M, h, ff) ? launch_mm_pers(EPI_RESID, d, s) : -1) != 0 &&
        launch_mm(EPI_RESID, d, s))
      return fail(MX_ERR_ARG, "ffn_down launch shape");
  }
  if (x_out)
    if (int rc = copy_out(x_out, M, s)) return rc;
  if (head) {
    if (!has_head) return fail(MX_ERR_STATE, "this stage has no output head");
    MMArgs g{};
    g.W = output; g.N = n_vocab; g.K = h; g.M = n_out; g.out = logits; g.ldo = n_vocab;
    // lm_head as a row-tile-persistent GEMV with the output RMS_NORM on load (no norm launch)
    const bool pers_head = use_pers && nol && !rowmap && n_out == M && mm_pers_supported(EPI_F32, M, n_vocab, h);
    if (!rowmap && n_out == M) {
      norm_operand(g, out_norm, pers_head);
    } else {
      launch_rmsnorm(xn, h, x, out_norm, rowmap, n_out, h, eps, s);
      g.X = xn; g.ldx = h;
    }
    if ((pers_head ? launch_mm_pers(EPI_F32, g, s) : -1) != 0 && launch_mm(EPI_F32, g, s))
      return fail(MX_ERR_ARG, "lm_head launch shape");
    if (argmax) pick(n_out, f.out, s);
  }
  HIPC(hipGetLastError());
  return 0;
}

// 17..64 rows: wide GEMVs (activations shared through LDS); attn_output and ffn_down run split-K
// into slabs that the next resid_norm folds into the residual stream in a fixed order.
// full_chain: a prompt chunk of <= 64 rows (prefill_gemm) -- every GEMV one MFMA chain over K, the
// prefill GEMM's order, so a prompt row's values do not depend on whether its chunk had 40 rows or 4000;
// the prompt's 16-row blocks take the prefill attention as in the GEMM path
int mx_engine::enqueue_forward_wide(const Forward& f, hipStream_t s, bool full_chain) {
  const int M = f.M, n_out = f.n_out, h = n_embd, ff = n_ff;
  const int* rowmap = f.rowmap;
  void* x_out = f.x_out;
  const bool head = f.head;
  int nslab = 0;  // partial slabs not yet folded into x
  dbg_count = 0;
  for (int li = 0; li < (int)layers.size(); li++) {
    const Layer& L = layers[li];
    launch_resid_norm(xn, h, x, slabs, nslab, slab_stride, L.attn_norm, M, h, eps, s);
    nslab = 0;
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    MMArgs a = qkv_args(L, li, f);
    a.X = xn; a.ldx = h;
    const int qsplit = launch_mm_wide(EPI_QKV, a, slabs, slab_stride, s, false, full_chain);
    if (qsplit < 0) return fail(MX_ERR_ARG, "wide qkv launch shape");
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    if (!rows_distinct) {  // rows of one sequence attend to each other's new K/V: finish them first
      launch_qkv_finish(a, slabs, qsplit, slab_stride, s);
      if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    }
    AttnArgs at = attn_args(li, f);
    at.out = attn_out;
    if (rows_distinct) {  // the attention kernel finishes q/k/v from the split-K slabs
      at.slabs = slabs; at.nslab = qsplit; at.slab_stride = slab_stride; at.rope_cs = rope_cs; at.kc_w = a.kc;
      at.vc_w = a.vc;
    }
    if (full_chain && rows_blocked) launch_attention_prefill(at, s);
    else launch_attention(at, s);
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    MMArgs b{};
    b.W = L.o; b.N = h; b.K = h; b.X = attn_out; b.ldx = h; b.M = M;
    if ((nslab = launch_mm_wide(EPI_RESID, b, slabs, slab_stride, s, true, full_chain)) < 0)
      return fail(MX_ERR_ARG, "wide attn_output launch shape");
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    launch_resid_norm(xn, h, x, slabs, nslab, slab_stride, L.ffn_norm, M, h, eps, s);
    nslab = 0;
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    MMArgs c{};
    c.W = L.gu; c.N = 2 * ff; c.K = h; c.M = M; c.X = xn; c.ldx = h; c.act = act; c.lda = ff;
    if (launch_mm_wide(EPI_SWIGLU, c, slabs, slab_stride, s, true, full_chain) < 0)
      return fail(MX_ERR_ARG, "wide gate/up launch shape");
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
    MMArgs d{};
    d.W = L.down; d.N = h; d.K = ff; d.X = act; d.ldx = ff; d.M = M;
    if ((nslab = launch_mm_wide(EPI_RESID, d, slabs, slab_stride, s, true, full_chain)) < 0)
      return fail(MX_ERR_ARG, "wide ffn_down launch shape");
    if (dbg_hit(s)) return fail(MX_DEBUG_STOPPED, "forward ended at the mx_debug stop");
  }
  if (x_out || (head && rowmap)) {
    launch_resid_norm(nullptr, 0, x, slabs, nslab, slab_stride, nullptr, M, h, eps, s);
    nslab = 0;
  }
  if (x_out)
    if (int rc = copy_out(x_out, M, s)) return rc;
  if (head) {
    if (!has_head) return fail(MX_ERR_STATE, "this stage has no output head");
    if (rowmap || n_out != M) {
      launch_rmsnorm(xn, h, x, out_norm, rowmap, n_out, h, eps, s);
    } else {
      launch_resid_norm(xn, h, x, slabs, nslab, slab_stride, out_norm, M, h, eps, s);
      nslab = 0;
    }
    MMArgs g{};
    g.W = output; g.N = n_vocab; g.K = h; g.M = n_out; g.X = xn; g.ldx = h; g.out = logits; g.ldo = n_vocab;
    const int rc = n_out > 16 ? launch_mm_wide(EPI_F32, g, slabs, slab_stride, s) : launch_mm(EPI_F32, g, s);
    if (rc < 0) return fail(MX_ERR_ARG, "lm_head launch shape");
    if (f.argmax) pick(n_out, f.out, s);
  } else if (nslab) {
    launch_resid_norm(nullptr, 0, x, slabs, nslab, slab_stride, nullptr, M, h, eps, s);
  }
  HIPC(hipGetLastError());
  return 0;
}

// The operand of one quantised MUL_MAT, ggml's conversion of src1 to the weight's vec_dot_type:
// Q8_K rows for a K-quant matrix (km), Q8_0 rows for a Q8_0 / Q4_0 one (km null).  ql: taken on load by the
// GEMV itself (RMS_NORM from the Σx² partials the residual writers leave) -- never under a row map; otherwise made
// by one launch, RMS_NORM + MUL + quantise (norm_w) or quantise alone.  A norm of the residual stream folds the
// nslab pending split-K slabs into x on its way.
int mx_engine::quant_operand(MMArgs& m, const KqMat* km, bool ql, int& nslab, const float* src, int K,
                             const float* norm_w, int rows, const int* rmap, hipStream_t s) {
  if (km) km->set(m);
  if (ql && !rmap) {
    m.xq = nullptr; m.xf = src; m.norm_w = norm_w; m.eps = eps; m.ssq = norm_w ? ssq : nullptr; m.np = K / 16;
    return 0;
  }
  const bool fold = norm_w && src == x && nslab;
  int rc = 0;
  if (km) {
    if (fold && K > 16 * 256) {  // launch_rmsnorm_q8k folds in one work-group per row, n <= 4096 (h 8192: Llama-3-70B): fold first
      launch_resid_norm(nullptr, 0, x, slabs, nslab, slab_stride, nullptr, rows, K, eps, s);
      rc = launch_rmsnorm_q8k(xq8, xqd, xkb, src, norm_w, rmap, rows, K, eps, s);
    } else if (fold) {
      rc = launch_rmsnorm_q8k(xq8, xqd, xkb, src, norm_w, rmap, rows, K, eps, s, slabs, nslab, slab_stride);
    } else {
      rc = norm_w ? launch_rmsnorm_q8k(xq8, xqd, xkb, src, norm_w, rmap, rows, K, eps, s)
                  : launch_quantize_q8k(xq8, xqd, xkb, src, K, rows, K, s);
    }
    m.xb = xkb;
  } else if (fold) {
    launch_rmsnorm_q8(xq8, xqd, src, norm_w, rmap, rows, K, eps, s, slabs, nslab, slab_stride);
  } else if (norm_w) {
    launch_rmsnorm_q8(xq8, xqd, src, norm_w, rmap, rows, K, eps, s);
  } else {
    launch_quantize_q8(xq8, xqd, src, K, rows, K, s);
  }
  if (fold) nslab = 0;
  m.xq = xq8; m.xd = xqd;
  return rc;
}

// The head of a quantised model: the output norm as the operand of the output matrix, Q8_K rows when that is a
// K-quant (a K-quant model, or a Q4_0 file with its Q6_K output: out_kq_head, ggml's q6_K.q8_K), Q8_0 rows
// otherwise.  nslab: slabs of the last ffn_down still pending (all M rows are read, no row map).
int mx_engine::quant_head(const Forward& f, int& nslab, hipStream_t s) {
  const int h = n_embd;
  const KqMat* km = (wkq || out_kq_head) ? &kq_out : nullptr;
  MMArgs g{};
  g.W = output; g.N = n_vocab; g.K = h; g.M = f.n_out; g.out = logits; g.ldo = n_vocab;
  if (!km) g.wq4 = out_q4;
  bool ql = wkq ? kq_on_load(f.M) : q8_on_load(f.M);
  if (!wkq && km) {  // the Q8_0 walk's K-quant head: always a norm launch, on x with the slabs folded
    if (nslab) launch_resid_norm(nullptr, 0, x, slabs, nslab, slab_stride, nullptr, f.M, h, eps, s);
    nslab = 0;
    ql = false;
  }
  if (quant_operand(g, km, ql, nslab, x, h, out_norm, f.n_out, (f.rowmap || f.n_out != f.M) ? f.rowmap : nullptr, s))
    return fail(MX_ERR_ARG, "kq head norm");
  if (km ? launch_mkq(EPI_F32, g, s) : launch_mq8(EPI_F32, g, s))
    return fail(MX_ERR_ARG, std::string(km ? "kq" : "q8") + " lm_head launch shape");
  return 0;
}

// Q8_0 / Q4_0 or K-quant model, any M <= PREFILL_ROWS: every MUL_MAT takes quantised activation rows
// (quant_operand; Q8_0 rows or Q8_K rows, by the weights' format).  The format shows only in the four helpers.
int mx_engine::enqueue_forward_quant(const Forward& f, hipStream_t s) {
  const int M = f.M, h = n_embd, ff = n_ff;
  const std::string fmt = wkq ? "kq" : "q8";
  if (f.head && f.n_out > MAX_ROWS) return fail(MX_ERR_ARG, "logits for at most 64 rows per forward");
  // Q8_0 at <= 4 rows, K-quants at one: every GEMV quantises its operand on load; more rows: one norm / quantise
  // launch per GEMV.  (A separate launch for gate/up measured slower at Q8_0: profiles/round5_quant_batch1_onload.txt;
  // a v_dot4 K-quant kernel quantising on load measured slower: 3.09 vs 2.80 ms per 8B token.)
  const bool ql = wkq ? kq_on_load(M) : q8_on_load(M);
  // 17..32 rows: q|k|v, attn_output and ffn_down as split-K slabs; the attention (distinct sequences) or
  // launch_qkv_finish finishes q|k|v, the next norm + quantise launch folds the other two into x
  const bool slab_rows = !ql && M > 16 && M <= 32;
  int nslab = 0;  // partials not yet folded into x
  auto operand = [&](MMArgs& m, const KqMat& km, const float* src, int K, const float* norm_w) -> int {
    if (!wkq) m.wq4 = wq4;
    return quant_operand(m, wkq ? &km : nullptr, ql, nslab, src, K, norm_w, M, nullptr, s);
  };
  auto mm = [&](int epi, const MMArgs& m) -> int { return wkq ? launch_mkq(epi, m, s) : launch_mq8(epi, m, s); };
  auto qkv_slab = [&](const MMArgs& m) -> int {  // not resid's launcher for the K-quants
    if (!slab_rows) return -1;
    return wkq ? launch_mkq_qkv_slab(m, slabs, slab_stride, s) : launch_mq8_slab(m, slabs, slab_stride, s);
  };
  auto resid = [&](const MMArgs& m) -> int {  // x += W . operand, in place or as slabs for the next norm
    if (slab_rows) {
      const int ks = wkq ? launch_mkq_slab(m, slabs, slab_stride, s) : launch_mq8_slab(m, slabs, slab_stride, s);
      if (ks > 0) return nslab = ks, 0;
    }
    return mm(EPI_RESID, m);
  };
  for (int li = 0; li < (int)layers.size(); li++) {
    const Layer& L = layers[li];
    MMArgs a = qkv_args(L, li, f);
    if (operand(a, L.kq_qkv, x, h, L.attn_norm)) return fail(MX_ERR_ARG, fmt + " norm shape");
    AttnArgs at = attn_args(li, f);
    at.outf = attn_f;
    const int qs = qkv_slab(a);
    if (qs > 0 && rows_distinct) {  // the attention kernel finishes q/k/v from the split-K slabs
      at.slabs = slabs; at.nslab = qs; at.slab_stride = slab_stride; at.rope_cs = rope_cs; at.kc_w = a.kc;
      at.vc_w = a.vc;
    } else if (qs > 0) {
      launch_qkv_finish(a, slabs, qs, slab_stride, s);
    } else if (mm(EPI_QKV, a)) {
      return fail(MX_ERR_ARG, fmt + " qkv launch shape");
    }
    if (M > MAX_ROWS && rows_blocked) launch_attention_prefill(at, s);
    else launch_attention(at, s);
    MMArgs b{};
    b.W = L.o; b.N = h; b.K = h; b.M = M; b.out = x; b.ldo = h;
    if (operand(b, L.kq_o, attn_f, h, nullptr)) return fail(MX_ERR_ARG, fmt + " quantise shape");
    b.ssq = ql ? ssq : nullptr; b.np = h / 16;  // Σx² partials of the new residual for gate/up's norm
    if (resid(b)) return fail(MX_ERR_ARG, fmt + " attn_output launch shape");
    MMArgs c{};
    c.W = L.gu; c.N = 2 * ff; c.K = h; c.M = M; c.actf = act_f; c.lda = ff;
    if (operand(c, L.kq_gu, x, h, L.ffn_norm) || mm(EPI_SWIGLU, c))
      return fail(MX_ERR_ARG, fmt + " gate/up launch shape");
    MMArgs d{};
    d.W = L.down; d.N = h; d.K = ff; d.M = M; d.out = x; d.ldo = h;
    if (operand(d, L.kq_down, act_f, ff, nullptr)) return fail(MX_ERR_ARG, fmt + " quantise shape");
    d.ssq = ql ? ssq : nullptr; d.np = h / 16;  // ... for the next layer's qkv (or lm_head) norm
    if (resid(d)) return fail(MX_ERR_ARG, fmt + " ffn_down launch shape");
  }
  if (nslab && (f.x_out || !(f.head && !f.rowmap && f.n_out == M))) {  // x itself is read next: fold the partials
    launch_resid_norm(nullptr, 0, x, slabs, nslab, slab_stride, nullptr, M, h, eps, s);
    nslab = 0;
  }
  if (f.x_out)
    if (int rc = copy_out(f.x_out, M, s)) return rc;
  if (f.head) {
    if (!has_head) return fail(MX_ERR_STATE, "this stage has no output head");
    if (int rc = quant_head(f, nslab, s)) return rc;
    if (f.argmax) pick(f.n_out, f.out, s);
  }
  HIPC(hipGetLastError());
  return 0;
}

// Prefill chunk of MAX_ROWS < M <= PREFILL_ROWS rows: MFMA GEMMs read each weight once per 256
// rows (not once per 64 as the wide decode kernels would); RMS_NORM as its own launch.  A K-quant
// model's layer is first dequantised to bf16 tiles (launch_dequant_kq: ~0.6 GB of HBM traffic per
// Llama-3-8B layer, a few % of a 4096-row chunk's GEMM time) -- the route llama.cpp's GPU backends
// take for large batches; decode keeps the int8-MFMA K-quant GEMVs with Q8_K activations.
int mx_engine::enqueue_forward_gemm(const Forward& f, hipStream_t s) {
  const int M = f.M, n_out = f.n_out, h = n_embd, kv = n_embd_kv, ff = n_ff;
  const int* rowmap = f.rowmap;
  void* x_out = f.x_out;
  const bool head = f.head;
  const size_t gstride = (size_t)M * h;  // RESID partial slabs [S][M][h]
  int nslab = 0;                         // ... not yet folded into x
  auto dequant = [&](uint16_t* dst, const KqMat& km, const uint16_t* w, int K) -> int {
    return launch_dequant_kq(dst, w, K, km.n, km.type, km.tile_end, km.off, s);
  };
  for (int li = 0; li < (int)layers.size(); li++) {
    const Layer& L = layers[li];
    const uint16_t *Wqkv = L.qkv, *Wo = L.o, *Wgu = L.gu, *Wdown = L.down;
    if (wkq) {
      if (dequant(kqd_qkv, L.kq_qkv, L.qkv, h) || dequant(kqd_o, L.kq_o, L.o, h) || dequant(kqd_gu, L.kq_gu, L.gu, h) ||
          dequant(kqd_down, L.kq_down, L.down, ff))
        return fail(MX_ERR_ARG, "K-quant dequantisation shape");
      Wqkv = kqd_qkv, Wo = kqd_o, Wgu = kqd_gu, Wdown = kqd_down;
    } else if (wq8) {  // Q8_0: d * q per weight, rounded to bf16
      auto dq = [&](uint16_t* dst, const uint16_t* w, int N, int K) {
        return launch_dequant_q8_tiles(dst, reinterpret_cast<const uint8_t*>(w), N, K, s);
      };
      if (dq(kqd_qkv, L.qkv, h + 2 * kv, h) || dq(kqd_o, L.o, h, h) || dq(kqd_gu, L.gu, 2 * ff, h) ||
          dq(kqd_down, L.down, h, ff))
        return fail(MX_ERR_ARG, "Q8_0 dequantisation shape");
      Wqkv = kqd_qkv, Wo = kqd_o, Wgu = kqd_gu, Wdown = kqd_down;
    }
    launch_resid_norm(xn, h, x, gslabs, nslab, gstride, L.attn_norm, M, h, eps, s);
    MMArgs a = qkv_args(L, li, f);
    a.W = Wqkv; a.X = xn; a.ldx = h;
    if (launch_gemm_split(EPI_QKV, a, gslabs, GSLAB_FLOATS, gemm_split_target, s) < 0) return fail(MX_ERR_ARG, "prefill qkv GEMM shape");
    AttnArgs at = attn_args(li, f);
    at.out = attn_out;
    if (rows_blocked) launch_attention_prefill(at, s);
    else launch_attention(at, s);
    MMArgs b{};
    b.W = Wo; b.N = h; b.K = h; b.X = attn_out; b.ldx = h; b.M = M; b.out = x; b.ldo = h;
    if ((nslab = launch_gemm_split(EPI_RESID, b, gslabs, GSLAB_FLOATS, gemm_split_target, s)) < 0)
      return fail(MX_ERR_ARG, "prefill attn_output GEMM shape");
    launch_resid_norm(xn, h, x, gslabs, nslab, gstride, L.ffn_norm, M, h, eps, s);
    MMArgs c{};
    c.W = Wgu; c.N = 2 * ff; c.K = h; c.M = M; c.X = xn; c.ldx = h; c.act = act; c.lda = ff;
    if (launch_gemm_split(EPI_SWIGLU, c, gslabs, GSLAB_FLOATS, gemm_split_target, s) < 0)
      return fail(MX_ERR_ARG, "prefill gate/up GEMM shape");
    MMArgs d{};
    d.W = Wdown; d.N = h; d.K = ff; d.X = act; d.ldx = ff; d.M = M; d.out = x; d.ldo = h;
    if ((nslab = launch_gemm_split(EPI_RESID, d, gslabs, GSLAB_FLOATS, gemm_split_target, s)) < 0)
      return fail(MX_ERR_ARG, "prefill ffn_down GEMM shape");
  }
  if (nslab) launch_resid_norm(nullptr, 0, x, gslabs, nslab, gstride, nullptr, M, h, eps, s);
  if (x_out)
    if (int rc = copy_out(x_out, M, s)) return rc;
  if (head) {
    if (!has_head) return fail(MX_ERR_STATE, "this stage has no output head");
    if (!rowmap) return fail(MX_ERR_ARG, "prefill head needs a row map");
    if (wkq || out_kq_head || wq8) {  // the quantised head as at decode, on the normed last rows
      int folded = 0;  // the slabs went into x above
      if (int rc = quant_head(f, folded, s)) return rc;
    } else {
      MMArgs g{};
      g.W = output; g.N = n_vocab; g.K = h; g.M = n_out; g.out = logits; g.ldo = n_vocab;
      launch_rmsnorm(xn, h, x, out_norm, rowmap, n_out, h, eps, s);
      g.X = xn; g.ldx = h;
      // the decode GEMVs (canonical K order at every row count), so a prompt's first token does not
      // depend on how many prompts ended in its chunk
      const int rc = (n_out > 16 && use_wide) ? (launch_mm_wide(EPI_F32, g, slabs, slab_stride, s) < 0 ? 1 : 0)
                                              : launch_mm(EPI_F32, g, s);
      if (rc) return fail(MX_ERR_ARG, "lm_head launch shape");
    }
  }
  HIPC(hipGetLastError());
  return 0;
}

__global__ void advance_pos_kernel(int* pos, int M) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) pos[i] += 1;
}

// rows forward, n <= MAX_ROWS, logits for all rows copied to host if requested
// lm_head runs only when logits are wanted: for every row, or (last_row_only, prompt chunks) for the
// last row alone -- a prefill never streams the 1 GB output matrix per 64-row chunk.
int mx_engine::forward_rows_chunk(int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                                  const void* x_in, void* x_out, float* logits_host, hipStream_t s,
                                  bool last_row_only) {
  if (n < 1 || n > PREFILL_ROWS) return fail(MX_ERR_ARG, "forward chunk of 1..PREFILL_ROWS rows");
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= n_seq_max) return fail(MX_ERR_ARG, "slot out of range");
    if (pos[i] < 0 || pos[i] >= n_ctx) return fail(MX_ERR_CTX, "position outside n_ctx");
    if (ids && has_embed && !x_in && (ids[i] < 0 || ids[i] >= n_vocab)) return fail(MX_ERR_ARG, "token id out of range");
  }
  // every call ends with a stream sync below, so the staging rows are free again at entry
  const size_t R = PREFILL_ROWS;
  auto h2d = [&](int* dst, const int32_t* src, int k, int row) -> int {
    memcpy(h_idx + row * R, src, (size_t)k * 4);
    if (hipMemcpyAsync(dst, h_idx + row * R, (size_t)k * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
      hipStreamSynchronize(s);  // earlier copies of this call may still read h_idx
      return fail(MX_ERR_HIP, "index upload");
    }
    return 0;
  };
  if (ids)
    if (int rc = h2d(d_ids, ids, n, 0)) return rc;
  if (int rc = h2d(d_pos, pos, n, 1)) return rc;
  if (int rc = h2d(d_slot, slots, n, 2)) return rc;
  const bool head = has_head && !x_out && logits_host;
  const int n_out = last_row_only ? 1 : n;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < n; i++) slot_tokens[slots[i]].clear();  // direct row writes: contents unknown
  }
  std::vector<int32_t> sorted(slots, slots + n);
  std::sort(sorted.begin(), sorted.end());
  rows_distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
  rows_blocked = blocked_rows(slots, pos, x_in ? nullptr : ids, n);
  if (head && last_row_only) {
    const int32_t last = n - 1;
    if (int rc = h2d(d_rowmap, &last, 1, 3)) return rc;
  }
  const int frc = enqueue_forward({.M = n, .ids = d_ids, .pos = d_pos, .slot = d_slot, .x_in = x_in, .x_out = x_out,
                                   .head = head, .rowmap = head && last_row_only ? d_rowmap : nullptr, .n_out = n_out},
                                  s);
  rows_distinct = false;
  rows_blocked = false;
  if (frc) {  // the index copies enqueued above still read h_idx: drain them before it is reused
    hipStreamSynchronize(s);
    return frc;
  }
  if (head) HIPC(hipMemcpyAsync(logits_host, logits, (size_t)n_out * n_vocab * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return 0;
}

// ---------------------------------------------------------------- scheduler
// The slot's record after a round of a live request (under mu): K/V are valid for the prompt and every generated
// token but the last (never fed back), and only below r->pos -- a speculating round leaves the K/V of rejected
// drafts past it, which must not count.  The record is a prefix of that sequence already, so it only grows.
void mx_engine::note_kv(const Request* r) {
  if (r->slot < 0) return;
  std::vector<int32_t>& st = slot_tokens[r->slot];
  const size_t np = r->prompt.size(), total = np + (r->out.empty() ? 0 : r->out.size() - 1);
  const size_t n = std::min(total, (size_t)std::max(0, r->pos));
  if (st.size() > n) st.resize(n);
  for (size_t k = st.size(); k < n; k++) st.push_back(k < np ? r->prompt[k] : r->out[k - np]);
}

int mx_engine::run_kv_copies(const std::vector<KvCopy>& tab) {
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  const int n = (int)tab.size();
  if (n < 1) return 0;
  if (n > n_seq_max) return fail(MX_ERR_STATE, "more KV copies than slots in one round");
  hipStream_t s = stream;
  HIPC(hipMemcpyAsync(d_kvcopy, tab.data(), (size_t)n * sizeof(KvCopy), hipMemcpyHostToDevice, s));
  std::chrono::steady_clock::time_point t0;
  if (trace) {  // the launch timed alone (the extra synchronise only when tracing)
    hipStreamSynchronize(s);
    t0 = std::chrono::steady_clock::now();
  }
  if (launch_kv_copy(kcache, vcache, tab.data(), d_kvcopy, n, le - lb, n_seq_max, n_head_kv, head_dim, n_ctx,
                     ctx_stride, slot_stride, layer_kv_stride, s)) {
    hipStreamSynchronize(s);
    return fail(MX_ERR_STATE, "KV copy table refused");
  }
  HIPC(hipStreamSynchronize(s));  // tab is the caller's: the table upload has read it
  const size_t bytes = kv_copy_bytes(tab.data(), n, le - lb, n_head_kv, head_dim, ctx_stride);
  if (trace)
    fprintf(stderr, "sched: kv copy %d copies %zu bytes %.3f ms\n", n, bytes,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  std::lock_guard<std::mutex> lk(mu);
  stat_copies += n;
  stat_copied_bytes += bytes;
  return 0;
}

// ---- host-RAM tier
// The capacity the API asked for becomes the store's (scheduler thread, under mu): evict down to it, 0 drops
// everything; the first capacity above 0 allocates the second stream, the events, the two staging areas (one
// slot's whole K/V each) and the tables.
void mx_engine::host_apply_capacity() {
  if (host_cap_req > 0 && !pack_stage && !host_failed) {
    host_tile_bytes = kv_pack_tile_bytes(le - lb, n_head_kv, head_dim);
    stage_bytes = (size_t)(ctx_stride / 32) * host_tile_bytes;
    const bool ok = hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&ev_packed, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&ev_stage_free, hipEventDisableTiming) == hipSuccess &&
                    hipHostMalloc((void**)&h_pack_tab, (size_t)2 * n_seq_max * sizeof(KvPack), hipHostMallocDefault) ==
                        hipSuccess &&
                    !alloc((void**)&d_pack_tab, (size_t)n_seq_max * sizeof(KvPack)) &&
                    !alloc((void**)&d_unpack_tab, (size_t)n_seq_max * sizeof(KvPack)) &&
                    !alloc((void**)&unpack_stage, stage_bytes) && !alloc((void**)&pack_stage, stage_bytes);
    if (!ok) {
      pack_stage = nullptr;
      host_failed = true;
    }
  }
  if (host_failed) host_cap_req = 0;
  host_cap = host_cap_req;
  while (!host_entries.empty() && (host_cap == 0 || host_bytes > host_cap)) {
    size_t lru = 0;
    for (size_t i = 1; i < host_entries.size(); i++)
      if (host_entries[i]->used < host_entries[lru]->used) lru = i;
    if (host_cap) stat_host_evictions++;
    host_drop(lru);
  }
}

// A record that nothing else covers enters the store (under mu): entries whose tokens are a prefix of it leave,
// least recently used ones until it fits; its memory and its transfer follow in run_host_spills.
void mx_engine::host_insert(const std::vector<int32_t>& st, int slot, std::vector<HostSpill>& spills) {
  const size_t bytes = (size_t)(((int)st.size() + 31) / 32) * host_tile_bytes;
  if (bytes > host_cap) {
    stat_host_skipped++;
    return;
  }
  for (size_t i = host_entries.size(); i-- > 0;) {
    const std::vector<int32_t>& t = host_entries[i]->tokens;
    if (t.size() <= st.size() && std::equal(t.begin(), t.end(), st.begin())) host_drop(i);
  }
  while (host_bytes + bytes > host_cap) {
    size_t lru = 0;
    for (size_t i = 1; i < host_entries.size(); i++)
      if (host_entries[i]->used < host_entries[lru]->used) lru = i;
    stat_host_evictions++;
    host_drop(lru);
  }
  auto e = std::make_shared<HostEntry>();
  e->tokens = st;
  e->bytes = bytes;
  e->used = ++host_clock;
  e->born = host_round;
  host_bytes += bytes;
  host_entries.push_back(e);
  spills.push_back({e, slot});
}

// Evicted entries: their pinned memory goes once their transfer has ended (never under mu: the wait may be long)
void mx_engine::host_free_trash() {
  for (auto& e : host_trash) {
    if (e->done) {
      hipEventSynchronize(e->done);
      hipEventDestroy(e->done);
    }
    if (e->pinned) hipHostFree(e->pinned);
    e->pinned = nullptr;
    e->done = nullptr;
  }
  host_trash.clear();
}

// The round's spills: pack launches on the engine stream -- the first thing of the round on it, so they read the
// slots as they stand -- each followed by its entries' device-to-host transfers on stream2.  A launch takes as
// many entries as pack_stage holds; the next one waits on the stream for the transfers that still read it.
int mx_engine::run_host_spills(std::vector<HostSpill>& spills) {
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  if (spills.empty()) return 0;
  if ((int)spills.size() > n_seq_max) return fail(MX_ERR_STATE, "more KV spills than slots in one round");
  // an entry evicted again in the same admission round is not written; one whose memory cannot be had is dropped
  std::vector<HostSpill> live;
  for (HostSpill& sp : spills) {
    const bool kept = std::find(host_entries.begin(), host_entries.end(), sp.e) != host_entries.end();
    if (kept && (hipHostMalloc(&sp.e->pinned, sp.e->bytes, hipHostMallocDefault) != hipSuccess ||
                 hipEventCreateWithFlags(&sp.e->done, hipEventDisableTiming) != hipSuccess)) {
      (void)hipGetLastError();
      std::lock_guard<std::mutex> lk(mu);
      stat_host_skipped++;
      host_drop(std::find(host_entries.begin(), host_entries.end(), sp.e) - host_entries.begin());
    } else if (kept) {
      live.push_back(sp);
    }
  }
  size_t done = 0, total = 0;
  while (done < live.size()) {
    size_t n = 0, off = 0;
    while (done + n < live.size() && off + live[done + n].e->bytes <= stage_bytes) {
      h_pack_tab[done + n] = {live[done + n].slot, (int32_t)live[done + n].e->tokens.size(), (int64_t)(off / 16)};
      off += live[done + n].e->bytes;
      n++;
    }
    if (!n) return fail(MX_ERR_STATE, "a KV spill larger than the staging area");
    HIPC(hipStreamWaitEvent(stream, ev_stage_free, 0));  // (a no-op before the first record)
    HIPC(hipMemcpyAsync(d_pack_tab + done, h_pack_tab + done, n * sizeof(KvPack), hipMemcpyHostToDevice, stream));
    std::chrono::steady_clock::time_point t0;
    if (trace) {
      hipStreamSynchronize(stream);
      t0 = std::chrono::steady_clock::now();
    }
    if (launch_kv_pack(kcache, vcache, pack_stage, stage_bytes, h_pack_tab + done, d_pack_tab + done, (int)n, le - lb,
                       n_seq_max, n_head_kv, head_dim, n_ctx, ctx_stride, slot_stride, layer_kv_stride, stream)) {
      hipStreamSynchronize(stream);
      return fail(MX_ERR_STATE, "KV pack table refused");
    }
    HIPC(hipEventRecord(ev_packed, stream));
    std::chrono::steady_clock::time_point t1;
    if (trace) {
      hipStreamSynchronize(stream);
      t1 = std::chrono::steady_clock::now();
    }
    HIPC(hipStreamWaitEvent(stream2, ev_packed, 0));
    for (size_t i = 0; i < n; i++) {
      HostEntry& e = *live[done + i].e;
      HIPC(hipMemcpyAsync(e.pinned, pack_stage + (size_t)h_pack_tab[done + i].off16 * 16, e.bytes,
                          hipMemcpyDeviceToHost, stream2));
      HIPC(hipEventRecord(e.done, stream2));
    }
    HIPC(hipEventRecord(ev_stage_free, stream2));
    if (trace) {
      hipStreamSynchronize(stream2);
      const auto t2 = std::chrono::steady_clock::now();
      fprintf(stderr, "sched: host spill %zu entries %zu bytes pack %.3f ms d2h %.3f ms\n", n, off,
              std::chrono::duration<double, std::milli>(t1 - t0).count(),
              std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    total += off;
    done += n;
  }
  std::lock_guard<std::mutex> lk(mu);
  stat_host_spills += live.size();
  stat_host_spilled_bytes += total;
  return 0;
}

// The round's restores, all on the engine stream ahead of the round's copies and prefill: each entry's first
// ceil32(n_pos)/32 tiles -- one contiguous prefix of its pinned memory -- to unpack_stage once its own transfer
// out has ended (its event), then one unpack launch for as many as the staging holds.
int mx_engine::run_host_restores(const std::vector<HostRestore>& restores) {
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  if (restores.empty()) return 0;
  if ((int)restores.size() > n_seq_max) return fail(MX_ERR_STATE, "more KV restores than slots in one round");
  KvPack* h_tab = h_pack_tab + n_seq_max;
  size_t done = 0, total = 0;
  while (done < restores.size()) {
    std::chrono::steady_clock::time_point t0;
    if (trace) {
      hipStreamSynchronize(stream);
      for (size_t i = done; i < restores.size(); i++) hipEventSynchronize(restores[i].e->done);
      t0 = std::chrono::steady_clock::now();
    }
    size_t n = 0, off = 0;
    while (done + n < restores.size()) {
      const HostRestore& rs = restores[done + n];
      const size_t bytes = (size_t)((rs.n_pos + 31) / 32) * host_tile_bytes;
      if (!rs.e->pinned || !rs.e->done || bytes > rs.e->bytes)
        return fail(MX_ERR_STATE, "a KV restore from an entry that does not hold it");
      if (off + bytes > stage_bytes) break;
      h_tab[done + n] = {rs.slot, rs.n_pos, (int64_t)(off / 16)};
      HIPC(hipStreamWaitEvent(stream, rs.e->done, 0));
      HIPC(hipMemcpyAsync(unpack_stage + off, rs.e->pinned, bytes, hipMemcpyHostToDevice, stream));
      off += bytes;
      n++;
    }
    if (!n) return fail(MX_ERR_STATE, "a KV restore larger than the staging area");
    HIPC(hipMemcpyAsync(d_unpack_tab + done, h_tab + done, n * sizeof(KvPack), hipMemcpyHostToDevice, stream));
    std::chrono::steady_clock::time_point t1;
    if (trace) {
      hipStreamSynchronize(stream);
      t1 = std::chrono::steady_clock::now();
    }
    if (launch_kv_unpack(kcache, vcache, unpack_stage, stage_bytes, h_tab + done, d_unpack_tab + done, (int)n, le - lb,
                         n_seq_max, n_head_kv, head_dim, n_ctx, ctx_stride, slot_stride, layer_kv_stride, stream)) {
      hipStreamSynchronize(stream);
      return fail(MX_ERR_STATE, "KV unpack table refused");
    }
    if (trace) {
      hipStreamSynchronize(stream);
      const auto t2 = std::chrono::steady_clock::now();
      fprintf(stderr, "sched: host restore %zu entries %zu bytes h2d %.3f ms unpack %.3f ms\n", n, off,
              std::chrono::duration<double, std::milli>(t1 - t0).count(),
              std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    total += off;
    done += n;
  }
  std::lock_guard<std::mutex> lk(mu);
  stat_host_restores += restores.size();
  stat_host_restored_bytes += total;
  return 0;
}

void mx_engine::finish(Request* r, int why) {
  r->finish = why;
  r->done = true;
  if (r->slot >= 0) {
    // K/V written for: the prompt and every generated token but the last (never fed back)
    std::vector<int32_t>& st = slot_tokens[r->slot];
    st = r->prompt;
    if (!r->out.empty()) st.insert(st.end(), r->out.begin(), r->out.end() - 1);
    if ((int)st.size() > r->pos) st.resize(std::max(0, r->pos));
    free_slots.push_back(r->slot);
  }
  stat_generated_tokens += r->out.size();
  r->slot = -1;
}

// llama.cpp default sampling chain (restricted to the parameters exposed in mx_sampling):
// repetition penalty -> top_k -> top_p -> min_p -> temperature -> draw
// llama.cpp's sampler chain as llama-cpp-python 0.3 builds it for create_completion: penalties ->
// top_k -> top_p -> min_p -> temperature -> draw (greedy when temperature <= 0).  The candidates are
// ordered by logit (ties: lower id first); only the top k are ever needed, so they are selected with
// a partial sort here, or on the device (launch_topk) in the decode loop.
bool mx::has_penalties(const mx_sampling& sp) {
  return sp.repeat_penalty != 1.0f || sp.frequency_penalty != 0.0f || sp.presence_penalty != 0.0f;
}

// the request's pick is more than an argmax of the raw row: it samples, or something rewrites its logits first
static bool needs_chain(const Request* r) {
  return r->samp.temperature > 0.f || has_penalties(r->samp) || (r->has_ext && r->ext.n_bias > 0);
}
namespace {
int req_path(const Request* r, int V, int* k_eff) {
  SampExt none{};
  none.typical_p = none.tfs_z = 1.0f;
  return sample_path(r->samp, r->has_ext ? r->ext : none, V, k_eff);
}
}  // namespace
// a device kernel can pick the request's rows: any path but the host sampler's
static bool dev_sampleable(const Request* r, int n_vocab) {
  int k;
  return req_path(r, n_vocab, &k) != MX_PICK_HOST;
}
// top-k the request asks of the device chain (what the round's K is the maximum of): its candidates on the chain
// path, the first one alone for a Mirostat or a wide row
static int chain_topk(const Request* r, int n_vocab) {
  int k = 1;
  return req_path(r, n_vocab, &k) == MX_PICK_CHAIN ? k : 1;
}

// bias and penalties of the host sampler on a copy of the row (the order and f32 arithmetic of the kernels)
static void rewrite_host(const mx_sampling& sp, const SampExt* ext, const int32_t* win, int n_win, int V, float* x) {
  if (ext)
    for (int j = 0; j < ext->n_bias; j++) x[ext->bias_tok[j]] += ext->bias_val[j];
  if (has_penalties(sp) && sp.repeat_last_n != 0) {
    const int n = sp.repeat_last_n < 0 ? n_win : std::min<int>(sp.repeat_last_n, n_win);
    std::vector<int> count(V, 0);
    for (int i = n_win - n; i < n_win; i++) count[win[i]]++;
    for (int i = 0; i < V; i++) {
      const int k = count[i];
      if (!k) continue;
      if (sp.repeat_penalty != 1.0f) x[i] = x[i] <= 0 ? x[i] * sp.repeat_penalty : x[i] / sp.repeat_penalty;
      x[i] -= fmaf((float)k, sp.frequency_penalty, sp.presence_penalty);  // fused, as penalty_kernel
    }
  }
}

// the whole chain on the host for one row x (rewritten in place): what sample_host and mx_sample_probe run
int32_t mx::chain_host(const mx_sampling& sp, const SampExt* ext, const int32_t* win, int n_win, int V, float* x,
                       double u01, float* mu) {
  rewrite_host(sp, ext, win, n_win, V, x);
  auto before = [](const std::pair<float, int>& a, const std::pair<float, int>& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  };
  if (sp.temperature > 0.f && ext && ext->miro == 2)
    return miro_pick_host(x, V, sp.temperature, ext->tau, ext->eta, u01, mu);
  std::vector<std::pair<float, int>> c;
  c.reserve(V);
  for (int i = 0; i < V; i++) c.push_back({x[i], i});
  if (sp.temperature <= 0.f) return std::min_element(c.begin(), c.end(), before)->second;
  const int k = sp.top_k > 0 ? std::min<int>(sp.top_k, V) : V;
  std::partial_sort(c.begin(), c.begin() + k, c.end(), before);
  std::vector<float> v(k), cv(k);
  std::vector<int> id(k), ci(k), ord(k);
  for (int i = 0; i < k; i++) v[i] = c[i].first, id[i] = c[i].second;
  std::vector<double> p(k), w(k);
  return samp_pick(v.data(), id.data(), k, sp.temperature, sp.top_p, sp.min_p, u01, p.data(), w.data(),
                   ext ? ext->tfs_z : 1.0f, ext ? ext->typical_p : 1.0f, cv.data(), ci.data(), ord.data());
}

int32_t mx_engine::sample_host(Request* r, const float* lg) {
  const mx_sampling& sp = r->samp;
  if (r->has_ext) {
    std::vector<float> x(lg, lg + n_vocab);
    std::vector<int32_t> hist(r->prompt);
    hist.insert(hist.end(), r->out.begin(), r->out.end());
    return chain_host(sp, &r->ext, hist.data(), (int)hist.size(), n_vocab, x.data(), samp_u01(r->seed, r->out.size()),
                      &r->mu);
  }
  std::vector<std::pair<float, int>> c;
  c.reserve(n_vocab);
  for (int i = 0; i < n_vocab; i++) c.push_back({lg[i], i});
  if (has_penalties(sp) && sp.repeat_last_n != 0) {
    // llama.cpp penalties sampler over the last repeat_last_n tokens: repeat (divide positive,
    // multiply negative logits), then frequency (per occurrence) and presence (once) subtracted
    std::vector<int> hist(r->prompt);
    hist.insert(hist.end(), r->out.begin(), r->out.end());
    int n = sp.repeat_last_n < 0 ? (int)hist.size() : std::min<int>(sp.repeat_last_n, (int)hist.size());
    std::vector<int> count(n_vocab, 0);
    for (int i = (int)hist.size() - n; i < (int)hist.size(); i++) count[hist[i]]++;
    for (auto& p : c) {
      const int k = count[p.second];
      if (!k) continue;
      if (sp.repeat_penalty != 1.0f) p.first = p.first <= 0 ? p.first * sp.repeat_penalty : p.first / sp.repeat_penalty;
      p.first -= (float)k * sp.frequency_penalty + sp.presence_penalty;
    }
  }
  auto before = [](const std::pair<float, int>& a, const std::pair<float, int>& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  };
  if (sp.temperature <= 0.f) return std::min_element(c.begin(), c.end(), before)->second;
  const int k = sp.top_k > 0 ? std::min<int>(sp.top_k, n_vocab) : n_vocab;
  std::partial_sort(c.begin(), c.begin() + k, c.end(), before);
  c.resize(k);
  return sample_chain(r, c);
}

int32_t mx_engine::sample_chain(Request* r, std::vector<std::pair<float, int>>& c) {
  // the device sampling chain's code (kernels.h samp_pick), over candidates of any count
  const mx_sampling& sp = r->samp;
  const int k = (int)c.size();
  std::vector<float> v(k);
  std::vector<int> id(k);
  for (int i = 0; i < k; i++) v[i] = c[i].first, id[i] = c[i].second;
  std::vector<double> p(k), w(k);
  return samp_pick(v.data(), id.data(), k, sp.temperature, sp.top_p, sp.min_p, samp_u01(r->seed, r->out.size()),
                   p.data(), w.data());
}

bool mx::device_sampleable(const mx_sampling& sp) {
  if (sp.top_k < 1 || sp.top_k > TOPK_MAX) return false;
  if (has_penalties(sp) && (sp.repeat_last_n < 0 || sp.repeat_last_n > SAMP_WIN)) return false;
  return true;
}

// mx_sample_plan's rules, in its order (include/mx_engine.h)
int mx::sample_path(const mx_sampling& sp, const SampExt& x, int V, int* k_eff) {
  const bool pen = has_penalties(sp);
  *k_eff = 1;
  if (sp.temperature <= 0.f && !pen && x.n_bias == 0) return MX_PICK_ARGMAX;
  if (pen && (sp.repeat_last_n < 0 || sp.repeat_last_n > SAMP_WIN)) return MX_PICK_HOST;
  if (!(sp.temperature > 0.f)) {  // greedy never reads top_k; inside 1..64 it still sizes the round's top-k as before
    if (sp.top_k >= 1 && sp.top_k <= TOPK_MAX) *k_eff = std::min(sp.top_k, V);
    return MX_PICK_CHAIN;
  }
  if (x.miro == 2) return MX_PICK_MIROSTAT;
  const int k = sp.top_k <= 0 || sp.top_k >= V ? V : sp.top_k;
  *k_eff = k;
  if (k <= TOPK_MAX) return MX_PICK_CHAIN;
  if (x.tfs_z < 1.0f || x.typical_p < 1.0f) return MX_PICK_HOST;
  if (V > SAMP_WIDE_VMAX) return MX_PICK_HOST;
  return MX_PICK_WIDE;
}

void mx_engine::samp_row(const Request* r, SampRow* o) const {
  const mx_sampling& sp = r->samp;
  memset(o, 0, sizeof(*o));
  o->temp = sp.temperature;
  o->top_p = sp.top_p;
  o->min_p = sp.min_p;
  o->repeat = sp.repeat_penalty;
  o->freq = sp.frequency_penalty;
  o->presence = sp.presence_penalty;
  int k = 1;
  req_path(r, n_vocab, &k);
  o->top_k = std::max(1, std::min(k, TOPK_MAX));  // the chain path's candidates; the wide kernel reads SampExt.wide_k
  o->last_n = has_penalties(sp) ? std::min(sp.repeat_last_n, SAMP_WIN) : 0;
  o->seed = r->seed;
  o->draw0 = (int)r->out.size();
  const int np = (int)r->prompt.size(), no = (int)r->out.size();
  o->n_win = std::min(o->last_n, np + no);
  for (int j = 0; j < o->n_win; j++) {
    const int t = np + no - o->n_win + j;
    o->win[j] = t < np ? r->prompt[t] : r->out[t - np];
  }
}

// Prefill of every newly admitted request together (llama.cpp's eval of the prompt, SURVEY §3.2,
// for all of them in as few forwards as the GEMM chunk allows): their remaining prompt rows back
// to back, each segment padded to a multiple of 16 rows with throw-away positions past the prompt
// when that stays inside n_ctx (so the rows form 16-position blocks of one sequence and the flash
// prefill attention runs; the pad K/V is overwritten by the first decode steps before anything
// reads it), lm_head only on each request's last prompt row, and the first token by the device
// argmax (ties -> lowest id) or, for sampling requests, the device sampling chain (the host sampler
// when a request's settings are outside the device chain's range).
int mx_engine::prefill_batch(std::vector<Request*>& admitted) {
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  struct Log {
    const std::chrono::steady_clock::time_point t0;
    size_t n;
    ~Log() {
      if (trace)
        fprintf(stderr, "sched: prefill %zu requests %.3f ms\n", n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
  } log{t0, admitted.size()};
  // embedding requests are evaluated in a pass of their own (no lm_head, every row pooled); a round without
  // them runs on the admitted list as it is
  std::vector<Request*> embd_reqs, gen_reqs;
  for (Request* r : admitted) (r->embd ? embd_reqs : gen_reqs).push_back(r);
  if (!embd_reqs.empty()) {
    if (int rc = prefill_embed(embd_reqs)) return rc;
    if (gen_reqs.empty()) return 0;
  }
  std::vector<Request*>& reqs = embd_reqs.empty() ? admitted : gen_reqs;
  // requests with prompt log-probabilities first evaluate prompt[0..n-1) in a pass of their own (all rows
  // through lm_head); what is left of them is the last prompt row, which joins the batch below
  for (Request* r : reqs)
    if (r->lp_prompt && r->prompt.size() > 1)
      if (int rc = prefill_prompt_logprobs(r)) return rc;
  // every prompt's rows start a 16-row block and are padded to whole blocks (positions past the prompt,
  // overwritten by its decode later; near n_ctx copies of the last row), so each chunk is blocked
  // (attn_prefill_kernel) and a prompt's blocks are the same whatever shares its chunk
  std::vector<int32_t> slots, pos, ids;
  std::vector<int> end_row(reqs.size()), blk_end(reqs.size());
  for (size_t q = 0; q < reqs.size(); q++) {
    Request* r = reqs[q];
    const int n = (int)r->prompt.size();
    for (int p = r->reuse; p < n; p++) {
      slots.push_back(r->slot);
      pos.push_back(p);
      ids.push_back(r->prompt[p]);
    }
    end_row[q] = (int)slots.size() - 1;
    const int pad = (16 - (n - r->reuse) % 16) % 16;
    for (int k = 0; k < pad; k++) {
      slots.push_back(r->slot);
      pos.push_back(n + pad <= n_ctx ? n + k : n - 1);
      ids.push_back(r->prompt[n - 1]);
    }
    blk_end[q] = (int)slots.size();
    r->pos = n;
  }
  const int chunk = gemm_ok() ? PREFILL_ROWS : MAX_ROWS;
  const int total = (int)slots.size();
  std::vector<int32_t> tok(reqs.size());
  bool any_sampling = false, dev_pick = use_dev_topk;
  for (Request* r : reqs)
    if (needs_chain(r)) {
      any_sampling = true;
      dev_pick &= dev_sampleable(r, n_vocab);
    }
  // every sampling request fits the device chain: first tokens are drawn on the device (the same
  // samp_pick and counter-based draw 0 as the host sampler), no logits rows cross PCIe
  dev_pick &= any_sampling;
  // grammar requests: the first token goes through the mask of the initial state; one that has
  // no first token is evaluated like the others, gets none and ends with its error after the prefill
  for (Request* r : reqs)
    if (r->gram && !gram_step_mask(r)) r->gram_end = MX_FINISH_ERROR + 1;
  std::vector<float> lg;
  std::vector<SampRow> sr;
  size_t q0 = 0;  // first request whose last row is not yet evaluated
  for (int i = 0; i < total;) {
    // chunk [i, e): at most `chunk` rows and at most MAX_ROWS request ends (logits rows)
    int e = std::min(total, i + chunk);
    size_t q1 = q0;
    while (q1 < reqs.size() && end_row[q1] < e && (int)(q1 - q0) < MAX_ROWS) q1++;
    if ((int)(q1 - q0) == MAX_ROWS && q1 < reqs.size() && end_row[q1] < e) e = blk_end[q1 - 1];
    const int m = e - i, n_out = (int)(q1 - q0);
    std::vector<int32_t> rowmap(n_out);
    for (int k = 0; k < n_out; k++) rowmap[k] = end_row[q0 + k] - i;
    hipStream_t st = stream;
    HIPC(hipMemcpyAsync(d_ids, ids.data() + i, m * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_pos, pos.data() + i, m * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_slot, slots.data() + i, m * 4, hipMemcpyHostToDevice, st));
    if (n_out) HIPC(hipMemcpyAsync(d_rowmap, rowmap.data(), n_out * 4, hipMemcpyHostToDevice, st));
    rows_distinct = false;
    rows_blocked = blocked_rows(slots.data() + i, pos.data() + i, ids.data() + i, m);
    prefill_gemm = true;
    const int frc = enqueue_forward({.M = m, .ids = d_ids, .pos = d_pos, .slot = d_slot, .head = n_out > 0,
                                     .rowmap = n_out ? d_rowmap : nullptr, .n_out = n_out},
                                    st);
    rows_blocked = false;
    prefill_gemm = false;
    if (frc) return frc;
    int ktop = 0, lpk = -1;  // lpk: log-probabilities of the first tokens, from these raw last-row logits
    for (int k = 0; k < n_out; k++) lpk = std::max(lpk, reqs[q0 + k]->lp_k);
    pick_lp = lpk;
    struct ResetLp {
      mx_engine* e;
      ~ResetLp() { e->pick_lp = -1, e->pick_gram = false; }
    } reset_lp{this};
    if (n_out && upload_gram(reqs.data() + q0, n_out, st) < 0) return fail(MX_ERR_HIP, "grammar mask copy");
    if (n_out && dev_pick) {
      sr.resize(n_out);
      for (int k = 0; k < n_out; k++) {
        samp_row(reqs[q0 + k], &sr[k]);
        if (needs_chain(reqs[q0 + k])) ktop = std::max(ktop, chain_topk(reqs[q0 + k], n_vocab));
      }
    }
    std::vector<float> mu_new;
    if (n_out && ktop > 0) {
      HIPC(hipMemcpyAsync(d_samp, sr.data(), n_out * sizeof(SampRow), hipMemcpyHostToDevice, st));
      const int xl = upload_ext(reqs.data() + q0, n_out, st);
      if (xl < 0) return fail(MX_ERR_HIP, "sampler settings copy");
      pick_samp = d_samp;
      pick_k = ktop;
      pick(n_out, PickOut{}, st);
      pick_samp = nullptr;
      pick_k = 0;
      pick_ext = nullptr, pick_miro = false, pick_wide = false;
      if (xl & 2) {
        mu_new.resize(n_out);
        HIPC(hipMemcpyAsync(mu_new.data(), d_mu, n_out * 4, hipMemcpyDeviceToHost, st));
      }
      HIPC(hipMemcpyAsync(tok.data() + q0, d_tok, n_out * 4, hipMemcpyDeviceToHost, st));
    } else if (n_out) {
      if (lpk >= 0 || pick_gram)
        pick(n_out, PickOut{}, st);  // pick_samp is null: argmax
      else
        launch_argmax(logits, n_vocab, n_out, n_vocab, am_val, am_idx, d_tok, nullptr, nullptr, nullptr, 0, nullptr,
                      0, st);
      HIPC(hipMemcpyAsync(tok.data() + q0, d_tok, n_out * 4, hipMemcpyDeviceToHost, st));
      if (any_sampling && !dev_pick) {
        lg.resize((size_t)n_out * n_vocab);
        HIPC(hipMemcpyAsync(lg.data(), logits, lg.size() * 4, hipMemcpyDeviceToHost, st));
      }
    }
    if (gram_refused) {
      gram_refused = false;
      hipStreamSynchronize(st);
      return fail(MX_ERR_ARG, "grammar mask launch shape");
    }
    const size_t lps = (size_t)SCHED_KMAX * (1 + 2 * std::max(lpk, 0));  // floats per row of lp_hist
    std::vector<float> lph, lpms;
    if (n_out && lpk >= 0) {
      lph.resize(n_out * lps);
      lpms.resize((size_t)n_out * 2);
      HIPC(hipMemcpyAsync(lph.data(), lp_hist, lph.size() * 4, hipMemcpyDeviceToHost, st));
      HIPC(hipMemcpyAsync(lpms.data(), lp_ms, lpms.size() * 4, hipMemcpyDeviceToHost, st));
    }
    HIPC(hipStreamSynchronize(st));
    std::lock_guard<std::mutex> lk(mu);
    for (int k = 0; k < n_out; k++) {
      Request* r = reqs[q0 + k];
      if (r->gram_end) continue;  // no first token: a grammar at a dead end from the start
      int32_t t = tok[q0 + k];
      const bool host_pick = !dev_pick && needs_chain(r);
      if (host_pick && r->gram) gram_mask_host(r, lg.data() + (size_t)k * n_vocab);
      if (host_pick) t = sample_host(r, lg.data() + (size_t)k * n_vocab);
      else if (int kw = 0; dev_pick && needs_chain(r) && req_path(r, n_vocab, &kw) == MX_PICK_WIDE) stat_wide_rows++;
      if (!mu_new.empty() && r->has_ext && r->ext.miro == 2) r->mu = mu_new[k];
      r->out.push_back(t);
      r->next_tok = t;
      if (r->lp_k >= 0) {
        float* ent = lph.data() + k * lps;
        // host-sampled: the same formula over the raw logit of the copied row
        if (host_pick) ent[0] = (lg[(size_t)k * n_vocab + t] - lpms[2 * k]) - lpms[2 * k + 1];
        r->lp_append(ent, lpk);
      }
      if (r->gram) {
        if (!r->gram->accept(t)) {
          r->error = "grammar: the picked token " + std::to_string(t) + " is not allowed";
          r->gram_end = MX_FINISH_ERROR + 1;
        } else if (r->gram->ended()) {
          r->gram_end = MX_FINISH_STOP + 1;
        }
      }
    }
    q0 = q1;
    i = e;
  }
  return 0;
}

// Prompt log-probabilities of one request (mx_submit_lp with prompt_logprobs): rows 0..n-2 of its prompt
// in chunks of at most MAX_ROWS rows (whole 16-row blocks, padded as in prefill_batch), every real row
// through lm_head, then launch_logprobs with the next prompt token as each row's target.  The last prompt
// row is left to prefill_batch (r->reuse = n - 1), whose logits start generation as for any request.
int mx_engine::prefill_prompt_logprobs(Request* r) {
  const int n = (int)r->prompt.size() - 1, k = r->lp_k, stride = 1 + 2 * k;
  std::vector<float> ent((size_t)MAX_ROWS * stride), all;
  all.reserve((size_t)n * stride);
  hipStream_t st = stream;
  for (int i = 0; i < n; i += MAX_ROWS) {
    const int m = std::min(MAX_ROWS, n - i), pad = (16 - m % 16) % 16, mp = m + pad;
    std::vector<int32_t> slots(mp, r->slot), pos(mp), ids(mp), rowmap(m), tgt(m);
    for (int j = 0; j < m; j++) pos[j] = i + j, ids[j] = r->prompt[i + j], rowmap[j] = j, tgt[j] = r->prompt[i + j + 1];
    for (int j = 0; j < pad; j++) {
      pos[m + j] = i + mp <= n_ctx ? i + m + j : i + m - 1;
      ids[m + j] = r->prompt[i + m - 1];
    }
    HIPC(hipMemcpyAsync(d_ids, ids.data(), mp * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_pos, pos.data(), mp * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_slot, slots.data(), mp * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_rowmap, rowmap.data(), m * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(lp_tgt, tgt.data(), m * 4, hipMemcpyHostToDevice, st));
    rows_distinct = false;
    rows_blocked = blocked_rows(slots.data(), pos.data(), ids.data(), mp);
    prefill_gemm = true;
    const int frc = enqueue_forward(
        {.M = mp, .ids = d_ids, .pos = d_pos, .slot = d_slot, .head = true, .rowmap = d_rowmap, .n_out = m}, st);
    rows_blocked = false;
    prefill_gemm = false;
    if (frc) {
      hipStreamSynchronize(st);
      return frc;
    }
    if (launch_logprobs(logits, n_vocab, m, n_vocab, k, lp_tgt, tk_ws_val, tk_ws_idx, lp_part, lp_ms, lp_top, lp_idx,
                        lp_hist, st)) {
      hipStreamSynchronize(st);
      return fail(MX_ERR_ARG, "log-prob launch shape");
    }
    HIPC(hipMemcpyAsync(ent.data(), lp_hist, (size_t)m * stride * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    all.insert(all.end(), ent.begin(), ent.begin() + (size_t)m * stride);
  }
  std::lock_guard<std::mutex> lk(mu);
  for (int j = 0; j < n; j++) r->lp_append(all.data() + (size_t)j * stride, k);
  r->lp_n_prompt = n;
  r->reuse = n;
  return 0;
}

// The embedding requests of a round (mx_submit_embed): their whole prompts (reuse = 0) laid
// out and padded to 16-row blocks as in prefill_batch, in chunks of the same size, each chunk one forward
// without lm_head followed by the tail over its real rows (embd_tail; the padding rows are in no segment).
// The vectors are copied to the requests; the scheduler then finishes them without a decode step.
int mx_engine::prefill_embed(std::vector<Request*>& reqs) {
  std::vector<int32_t> slots, pos, ids;
  std::vector<int> beg(reqs.size());
  for (size_t ri = 0; ri < reqs.size(); ri++) {
    Request* r = reqs[ri];
    const int n = (int)r->prompt.size();
    beg[ri] = (int)slots.size();
    for (int p = 0; p < n; p++) {
      slots.push_back(r->slot);
      pos.push_back(p);
      ids.push_back(r->prompt[p]);
    }
    const int pad = (16 - n % 16) % 16;
    for (int k = 0; k < pad; k++) {
      slots.push_back(r->slot);
      pos.push_back(n + pad <= n_ctx ? n + k : n - 1);
      ids.push_back(r->prompt[n - 1]);
    }
    r->pos = n;
    r->embd_rows = r->embd_pool == MX_POOL_NONE ? n : 1;
    r->embd_out.assign((size_t)r->embd_rows * n_embd, 0.f);
  }
  const int chunk = gemm_ok() ? PREFILL_ROWS : MAX_ROWS;
  const int total = (int)slots.size();
  hipStream_t st = stream;
  const size_t h = n_embd;
  std::vector<std::vector<int32_t>> tabs;  // host index tables, read by async copies until the chunk's sync
  struct Stage {  // pooled vectors of one tail, copied in one piece: v [owner.size()][n_embd] for reqs[owner[j]]
    std::vector<size_t> owner;
    std::vector<float> v;
  };
  std::vector<Stage> stages;
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  for (int i = 0; i < total; i += chunk) {
    const int e = std::min(total, i + chunk), m = e - i;
    const auto t_chunk = std::chrono::steady_clock::now();
    HIPC(hipMemcpyAsync(d_ids, ids.data() + i, m * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_pos, pos.data() + i, m * 4, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_slot, slots.data() + i, m * 4, hipMemcpyHostToDevice, st));
    rows_distinct = false;
    rows_blocked = blocked_rows(slots.data() + i, pos.data() + i, ids.data() + i, m);
    prefill_gemm = true;
    const int frc = enqueue_forward({.M = m, .ids = d_ids, .pos = d_pos, .slot = d_slot}, st);
    rows_blocked = false;
    prefill_gemm = false;
    if (frc) {
      hipStreamSynchronize(st);
      return frc;
    }
    std::chrono::steady_clock::time_point t_fwd;
    if (trace) {  // forward and tail timed apart (the extra synchronise only when tracing)
      hipStreamSynchronize(st);
      t_fwd = std::chrono::steady_clock::now();
    }
    // the requests of one mx_submit_embed call share pooling and normalize, but two calls may share a round:
    // one tail per (pooling, normalize) present, each followed by its copies (the next tail reuses q and the
    // pooled vectors).  The pooled vectors a tail completes are consecutive rows of embd_pooled: one copy.
    tabs.clear();
    stages.clear();
    for (int mode = 0; mode < 8; mode++) {
      const int pooling = mode >> 1;
      const bool l2 = mode & 1;
      std::vector<EmbdSeg> segs;
      std::vector<size_t> owner;
      Stage sg_out;
      int k = 0;
      for (size_t ri = 0; ri < reqs.size(); ri++) {
        Request* r = reqs[ri];
        if (r->embd_pool != pooling || r->embd_l2 != l2) continue;
        const int n = (int)r->prompt.size();
        const int a = std::max(beg[ri], i), b = std::min(beg[ri] + n, e);
        if (a >= b) continue;
        const bool completes = pooling == MX_POOL_CLS ? a == beg[ri] : b == beg[ri] + n;
        int dst0 = k;  // NONE: the rows compacted in q
        if (pooling != MX_POOL_NONE) {
          dst0 = (int)sg_out.owner.size();
          if (completes) sg_out.owner.push_back(ri);
        }
        segs.push_back({a - i, b - a, r->slot, a - beg[ri], n, dst0});
        owner.push_back(ri);
        k += b - a;
      }
      if (segs.empty()) continue;
      tabs.emplace_back();
      int rc = embd_tail(x, out_norm, eps, n_embd, segs, pooling, l2, q, embd_acc, embd_pooled, d_embd_tab,
                         EMBD_TAB_CAP, tabs.back(), st);
      if (!rc && pooling == MX_POOL_NONE) {
        for (size_t g = 0; g < segs.size() && !rc; g++)
          if (hipMemcpyAsync(reqs[owner[g]]->embd_out.data() + segs[g].done * h, q + segs[g].dst0 * h,
                             segs[g].rows * h * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = fail(MX_ERR_HIP, "embedding copy");
      } else if (!rc && !sg_out.owner.empty()) {
        sg_out.v.resize(sg_out.owner.size() * h);
        if (hipMemcpyAsync(sg_out.v.data(), embd_pooled, sg_out.v.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
          rc = fail(MX_ERR_HIP, "embedding copy");
        stages.push_back(std::move(sg_out));
      }
      if (rc) {
        hipStreamSynchronize(st);
        return rc;
      }
    }
    HIPC(hipStreamSynchronize(st));
    for (const Stage& sg : stages)
      for (size_t j = 0; j < sg.owner.size(); j++)
        memcpy(reqs[sg.owner[j]]->embd_out.data(), sg.v.data() + j * h, h * 4);
    if (trace)
      fprintf(stderr, "sched: embed chunk %d rows: forward %.3f ms, tail + copies %.3f ms\n", m,
              std::chrono::duration<double, std::milli>(t_fwd - t_chunk).count(),
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fwd).count());
  }
  return 0;
}

// Prompt-lookup speculation.  Eligible: asked for, greedy without penalties or
// log-probabilities, on a whole bf16 model -- the path whose rows are bitwise independent of the row count.
bool mx_engine::spec_eligible(const Request* r) const {
  return r->spec_d > 0 && spec_ctx && r->samp.temperature <= 0.f && !has_penalties(r->samp) && r->lp_k < 0 &&
         !r->has_ext && !r->gram &&
         !embd_q8 && !out_q8 && !embd_kq_type && !out_kq_head;
}

// A speculating round: every active request eligible, their R (1 + D) rows within the <= 16-row decode path
// (D = the largest num_pred_tokens asked for), and no row able to reach n_ctx in the round's K steps.  A step
// = draft kernel -> forward over R (1 + D) rows (row r(1+D): the request's last token, then its draft, all
// in its slot; lm_head on every row) -> argmax partials -> accept kernel; everything it indexes with lives
// on the device, so one captured graph replays K times.  Then the variable-length history of each request
// is applied with the plain round's EOS / max_tokens / cancel rules: tokens past the end are dropped, and
// pos / the slot's recorded tokens cover only what was kept.  Returns 1, 0 (run this round plain), or < 0.
int mx_engine::sched_step_spec(std::vector<Request*>& rows) {
  const int R = (int)rows.size();
  if (R > SPEC_MAX_REQ) return 0;
  int D = 0, need = 1;
  for (const Request* r : rows) {
    if (!spec_eligible(r) || r->pos + 1 != (int)(r->prompt.size() + r->out.size())) return 0;
    D = std::max(D, r->spec_d);
    // steps the request still needs at the tokens per step it has had so far (1 + accepted / steps; at least
    // one token per step): a round that falls short is followed by another, one that overshoots wasted steps
    const uint64_t left = (uint64_t)std::max(1, r->max_tokens - (int)r->out.size());
    const uint64_t st = std::max<uint64_t>(1, r->spec_steps), per = st + r->spec_accepted;
    need = std::max(need, (int)((left * st + per - 1) / per));
  }
  if (R * (1 + D) > SPEC_ROWS) return 0;
  int K = std::min(SCHED_KMAX, need);
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!pending.empty() && !free_slots.empty()) K = 1;  // admit waiting requests at the next round
  }
  for (const Request* r : rows)
    while (K >= 1 && r->pos + K * (1 + D) + D > n_ctx - 1) K--;
  if (K < 1) return 0;  // close to n_ctx: the plain round reaches the last positions
  const int M = R * (1 + D), HS = SCHED_KMAX * SPEC_ROWS;
  std::vector<int32_t> ids(M), pos(M), slots(M), par(2 * R), len(R);
  std::vector<std::vector<int32_t>> ctx(R);
  hipStream_t s = stream;
  for (int i = 0; i < R; i++) {
    const Request* r = rows[i];
    for (int j = 0; j <= D; j++) {  // rows 1..D are rewritten by the draft kernel
      ids[i * (1 + D) + j] = r->next_tok;
      pos[i * (1 + D) + j] = r->pos;
      slots[i * (1 + D) + j] = r->slot;
    }
    par[2 * i] = r->spec_d;
    par[2 * i + 1] = r->spec_ng;
    ctx[i] = r->prompt;
    ctx[i].insert(ctx[i].end(), r->out.begin(), r->out.end());
    len[i] = (int)ctx[i].size();
    HIPC(hipMemcpyAsync(spec_ctx + (size_t)i * n_ctx, ctx[i].data(), (size_t)len[i] * 4, hipMemcpyHostToDevice, s));
  }
  HIPC(hipMemcpyAsync(d_ids, ids.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_pos, pos.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_slot, slots.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(spec_par, par.data(), R * 2 * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(spec_len, len.data(), R * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(spec_hist_count, 0, R * 4, s));
  HIPC(hipMemsetAsync(spec_cnt, 0, R * 3 * 4, s));
  auto step = [&]() -> int {
    launch_spec_draft(spec_ctx, n_ctx, spec_len, spec_par, R, D, d_ids, d_pos, d_slot, spec_ndraft, s);
    // rows of one slot: the plain <= 16-row path, whose q|k|v epilogue stores every row's K/V before the
    // attention launch reads them (rows_distinct stays false)
    if (int rc = enqueue_forward({.M = M, .ids = d_ids, .pos = d_pos, .slot = d_slot, .head = true, .n_out = M}, s))
      return rc;
    launch_argmax_stage1(logits, n_vocab, M, n_vocab, am_val, am_idx, s);
    launch_spec_accept(am_val, am_idx, R, D, d_ids, d_pos, spec_ndraft, spec_ctx, n_ctx, spec_len, spec_hist, HS,
                       spec_hist_count, spec_cnt, spec_log, SCHED_KMAX, s);
    return 0;
  };
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  bool captured = false;
  auto it = spec_graphs.find({R, D});
  if (use_graphs && it == spec_graphs.end()) {
    captured = true;
    hipGraph_t g;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = step();
    hipError_t ce = hipStreamEndCapture(s, &g);
    if (rc) return rc;
    if (ce != hipSuccess) return fail(MX_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce));
    hipGraphExec_t ex;
    HIPC(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    it = spec_graphs.emplace(std::make_pair(R, D), ex).first;
  }
  for (int k = 0; k < K; k++) {
    if (use_graphs) HIPC(hipGraphLaunch(it->second, s));
    else if (int rc = step()) return rc;
  }
  std::vector<int32_t> hist((size_t)R * HS), log((size_t)R * SCHED_KMAX * 2);
  HIPC(hipMemcpyAsync(hist.data(), spec_hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(log.data(), spec_log, log.size() * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  std::lock_guard<std::mutex> lk(mu);
  stat_rounds++, stat_dev_steps += K;
  int emitted = 0;
  for (int i = 0; i < R; i++) {
    Request* r = rows[i];
    int off = 0;
    for (int k = 0; k < K && !r->done; k++) {
      const int nd = log[((size_t)i * SCHED_KMAX + k) * 2], a = log[((size_t)i * SCHED_KMAX + k) * 2 + 1];
      if (nd < 0 || nd > D || a < 0 || a > nd || off + a + 1 > HS) return fail(MX_ERR_STATE, "speculation step log");
      int kept = 0;
      for (int j = 0; j <= a && !r->done; j++, kept++) {
        const int32_t t = hist[(size_t)i * HS + off + j];
        r->pos++;
        r->out.push_back(t);
        r->next_tok = t;
        if ((is_eog(t) && !r->samp.ignore_eos) || r->cancel) finish(r, MX_FINISH_STOP);
        else if ((int)r->out.size() >= r->max_tokens || r->pos >= n_ctx) finish(r, MX_FINISH_LENGTH);
      }
      off += a + 1;
      emitted += kept;
      r->spec_steps++, r->spec_drafted += nd, r->spec_accepted += kept - 1;
      stat_spec_steps++, stat_spec_drafted += nd, stat_spec_accepted += kept - 1;
    }
    note_kv(r);  // up to the kept position only
  }
  if (trace) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "sched: speculating R=%d D=%d K=%d kept %d tokens %s%.3f ms\n", R, D, K, emitted,
            captured ? "(graph captured) " : "", ms);
  }
  return 1;
}

// One scheduler round over the active rows.  All greedy (no penalties): K decode steps replayed
// back to back on the device (the captured step feeds its argmax into the next step's ids and
// positions and appends it to a history), one sync, then the K tokens of every row are applied in
// order (a row that finishes early ignores the rest).  Otherwise one step, with the sampler chain
// on the host (top-k candidates from the device when possible).
int mx_engine::sched_step(std::vector<Request*>& rows) {
  // grammar rows: the mask of this step, on the host, before anything is enqueued; a row at a dead
  // end leaves the round with an error and the others run as if it had never been there
  bool any_gram = false;
  for (size_t i = 0; i < rows.size();) {
    Request* r = rows[i];
    if (r->gram && !gram_step_mask(r)) {
      std::lock_guard<std::mutex> lk(mu);
      finish(r, MX_FINISH_ERROR);
      rows.erase(rows.begin() + i);
      continue;
    }
    any_gram |= r->gram != nullptr;
    i++;
  }
  if (rows.empty()) return 0;
  if (const int sp = sched_step_spec(rows)) return sp < 0 ? sp : 0;
  const int M = (int)rows.size();
  std::vector<int32_t> ids(M), pos(M), slots(M);
  bool all_greedy = true, all_dev = true;
  int room = SCHED_KMAX, need = 1, ktop = 0, lpk = -1;  // lpk: max lp_k of the rows, -1 = no log-probabilities
  for (int i = 0; i < M; i++) {
    lpk = std::max(lpk, rows[i]->lp_k);
    ids[i] = rows[i]->next_tok;
    pos[i] = rows[i]->pos;
    slots[i] = rows[i]->slot;
    if (needs_chain(rows[i])) {
      all_greedy = false;
      if (use_dev_topk && dev_sampleable(rows[i], n_vocab)) ktop = std::max(ktop, chain_topk(rows[i], n_vocab));
      else all_dev = false;
    }
    room = std::min(room, n_ctx - rows[i]->pos);
    need = std::max(need, rows[i]->max_tokens - (int)rows[i]->out.size());
  }
  // greedy rows: argmax on the device; every row sampleable on the device: the device sampling chain
  // (penalties, top-k, top-p, min-p, temperature, draw); either way K steps run back to back on the
  // device.  Otherwise one step, sampled on the host.
  const bool dev_chain = !all_greedy && all_dev && ktop > 0;
  int K = 1;
  if (all_greedy || dev_chain) {
    K = std::max(1, std::min(room, need));
    std::lock_guard<std::mutex> lk(mu);
    if (!pending.empty() && !free_slots.empty()) K = 1;  // admit waiting requests at the next round
  }
  if (any_gram) K = 1;  // the next mask depends on the token this step picks
  hipStream_t s = stream;
  HIPC(hipMemcpyAsync(d_ids, ids.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_pos, pos.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_slot, slots.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(sched_hist_count, 0, M * 4, s));
  std::vector<SampRow> sr;
  if (dev_chain) {
    sr.resize(M);
    for (int i = 0; i < M; i++) samp_row(rows[i], &sr[i]);
    HIPC(hipMemcpyAsync(d_samp, sr.data(), M * sizeof(SampRow), hipMemcpyHostToDevice, s));
  }
  struct Reset {
    mx_engine* e;
    ~Reset() {
      e->rows_distinct = false; e->pick_samp = nullptr; e->pick_k = 0; e->pick_lp = -1;
      e->pick_ext = nullptr; e->pick_miro = false; e->pick_wide = false; e->pick_gram = false;
    }
  } reset_flags{this};
  // rows with the extended settings: their SampExt and mu beside the SampRows; the level joins the graph key
  const int xl = dev_chain ? upload_ext(rows.data(), M, s) : 0;
  if (xl < 0) return fail(MX_ERR_HIP, "sampler settings copy");
  // grammar rows: their masks beside them; one more level bit of the graph key
  const int gl = any_gram ? upload_gram(rows.data(), M, s) : 0;
  if (gl < 0) return fail(MX_ERR_HIP, "grammar mask copy");
  rows_distinct = true;  // one row per active request, each its own slot
  pick_samp = dev_chain ? d_samp : nullptr;
  pick_k = dev_chain ? ktop : 0;
  pick_lp = lpk;
  auto step = [&]() -> int {
    return enqueue_forward({.M = M, .ids = d_ids, .pos = d_pos, .slot = d_slot, .head = true, .n_out = M,
                            .argmax = true,
                            .out = {.ids_next = d_ids, .pos_next = d_pos, .hist = sched_hist, .hist_stride = SCHED_KMAX,
                                    .hist_count = sched_hist_count, .max_hist = SCHED_KMAX}},
                           s);
  };
  static const bool trace = getenv("MX_SCHED_TRACE") != nullptr;  // per-round timing on stderr
  const auto t0 = std::chrono::steady_clock::now();
  bool captured = false;
  const std::tuple<int, int, int, int> gkey(M, pick_k, pick_lp, xl | (gl ? 8 : 0));
  auto it = sched_graphs.find(gkey);
  if (use_graphs && it == sched_graphs.end()) {
    captured = true;
    hipGraph_t g;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = step();
    hipError_t ce = hipStreamEndCapture(s, &g);
    if (rc) return rc;
    if (ce != hipSuccess) return fail(MX_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce));
    hipGraphExec_t ex;
    HIPC(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    it = sched_graphs.emplace(gkey, ex).first;
  }
  for (int k = 0; k < K; k++) {
    if (use_graphs) HIPC(hipGraphLaunch(it->second, s));
    else if (int rc = step()) return rc;
  }
  if (gram_refused) {
    gram_refused = false;
    hipStreamSynchronize(s);
    return fail(MX_ERR_ARG, "grammar mask launch shape");
  }
  std::vector<int32_t> hist((size_t)M * SCHED_KMAX);
  std::vector<float> lg, tkv;
  std::vector<int32_t> tki;
  HIPC(hipMemcpyAsync(hist.data(), sched_hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
  // sampling rows: the top-k candidates come from the device (k <= TOPK_MAX, no penalties, which
  // would reorder logits first); otherwise the whole logits rows go to the host
  int TK = 0;
  bool dev_topk = !all_greedy && !dev_chain && use_dev_topk;
  for (int i = 0; i < M && dev_topk; i++) {
    const mx_sampling& sp = rows[i]->samp;
    if (rows[i]->has_ext) dev_topk = false;  // bias reorders the row, Mirostat reads all of it: whole rows
    if (sp.temperature <= 0.f && !has_penalties(sp)) continue;
    if (has_penalties(sp) || sp.top_k < 1 || sp.top_k > TOPK_MAX) dev_topk = false;
    else TK = std::max(TK, std::min(sp.top_k, n_vocab));
  }
  if (dev_topk && TK > 0) {
    if (launch_topk(logits, n_vocab, M, n_vocab, TK, tk_ws_val, tk_ws_idx, tk_val, tk_idx, s))
      return fail(MX_ERR_HIP, "top-k launch");
    tkv.resize((size_t)M * TK);
    tki.resize((size_t)M * TK);
    HIPC(hipMemcpyAsync(tkv.data(), tk_val, (size_t)M * TK * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(tki.data(), tk_idx, (size_t)M * TK * 4, hipMemcpyDeviceToHost, s));
  } else if (!all_greedy && !dev_chain) {
    lg.resize((size_t)M * n_vocab);
    HIPC(hipMemcpyAsync(lg.data(), logits, (size_t)M * n_vocab * 4, hipMemcpyDeviceToHost, s));
  }
  // the round's log-prob history travels with `hist`; (m, log s) too when the host picks (K = 1)
  const size_t lpe = 1 + 2 * (size_t)std::max(lpk, 0), lps = SCHED_KMAX * lpe;
  std::vector<float> lph, lpms;
  if (lpk >= 0) {
    lph.resize(M * lps);
    HIPC(hipMemcpyAsync(lph.data(), lp_hist, lph.size() * 4, hipMemcpyDeviceToHost, s));
    if (!all_greedy && !dev_chain) {
      lpms.resize((size_t)M * 2);
      HIPC(hipMemcpyAsync(lpms.data(), lp_ms, lpms.size() * 4, hipMemcpyDeviceToHost, s));
    }
  }
  // Mirostat rows: mu after each step, so a row keeps the mu of the last step whose token it keeps
  std::vector<float> muh;
  if (xl & 2) {
    muh.resize((size_t)M * SCHED_KMAX);
    HIPC(hipMemcpyAsync(muh.data(), d_mu_hist, muh.size() * 4, hipMemcpyDeviceToHost, s));
  }
  HIPC(hipStreamSynchronize(s));
  if (trace) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "sched: decode M=%d K=%d %s%s%s%s%.3f ms\n", M, K, dev_chain ? "(device sampling) " : "",
            xl & 4 ? "(wide) " : xl & 2 ? "(mirostat) " : xl == 1 ? "(extended chain) " : "", lpk >= 0 ? "(logprobs) " : "",
            captured ? "(graph captured) " : "", ms);
  }
  std::lock_guard<std::mutex> lk(mu);
  stat_rounds++;
  (all_greedy || dev_chain ? stat_dev_steps : stat_host_steps) += K;
  for (int i = 0; i < M; i++) {
    Request* r = rows[i];
    int kw = 0;
    const bool wide = dev_chain && (xl & 4) && req_path(r, n_vocab, &kw) == MX_PICK_WIDE;
    for (int k = 0; k < K && !r->done; k++) {
      r->pos++;
      stat_wide_rows += wide ? 1 : 0;
      int32_t t = hist[(size_t)i * SCHED_KMAX + k];
      float raw = 0.f;  // host pick: the chosen token's raw logit (candidate list or copied row)
      const bool host_pick = !dev_chain && needs_chain(r);
      if (!muh.empty() && r->has_ext && r->ext.miro == 2) r->mu = muh[(size_t)i * SCHED_KMAX + k];
      if (host_pick) {
        if (!tkv.empty()) {
          std::vector<std::pair<float, int>> c(std::min(r->samp.top_k, n_vocab));
          for (size_t j = 0; j < c.size(); j++) c[j] = {tkv[(size_t)i * TK + j], tki[(size_t)i * TK + j]};
          t = sample_chain(r, c);
          for (size_t j = 0; j < c.size(); j++)
            if (tki[(size_t)i * TK + j] == t) raw = tkv[(size_t)i * TK + j];
        } else {
          if (r->gram) gram_mask_host(r, lg.data() + (size_t)i * n_vocab);
          t = sample_host(r, lg.data() + (size_t)i * n_vocab);
          raw = lg[(size_t)i * n_vocab + t];
        }
      }
      r->out.push_back(t);
      r->next_tok = t;
      if (r->lp_k >= 0) {
        float* ent = lph.data() + i * lps + k * lpe;
        if (host_pick) ent[0] = (raw - lpms[2 * i]) - lpms[2 * i + 1];
        r->lp_append(ent, lpk);
      }
      if (r->gram) {  // the token moves the grammar on; an end-of-generation token ends it and the request
        if (!r->gram->accept(t)) {
          r->error = "grammar: the picked token " + std::to_string(t) + " is not allowed";
          finish(r, MX_FINISH_ERROR);
        } else if (r->gram->ended()) {
          finish(r, MX_FINISH_STOP);
        }
      }
      if (r->done) continue;
      if ((is_eog(t) && !r->samp.ignore_eos) || r->cancel) finish(r, MX_FINISH_STOP);
      else if ((int)r->out.size() >= r->max_tokens || r->pos >= n_ctx) finish(r, MX_FINISH_LENGTH);
    }
    note_kv(r);
  }
  return 0;
}

void mx_engine::scheduler_loop() {
  hipSetDevice(device);
  for (;;) {
    std::vector<Request*> admit;
    // prefix sharing: the round's copies from slots as they stand (pre) and from requests of this
    // round to their followers (post); all empty while the switch is off
    std::vector<Request*> followers;
    std::vector<KvCopy> pre, post;
    // host tier: records leaving for host memory and prefixes coming back; empty while it is off
    std::vector<HostSpill> spills;
    std::vector<HostRestore> restores;
    auto lcp =[](const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
      int l = 0;
      const int lim = (int)std::min(a.size(), b.size());
      while (l < lim && a[l] == b[l]) l++;
      return l;
    };
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || !pending.empty() || !active.empty() || host_cap_req != host_cap; });
      if (!stop && host_cap_req != host_cap) {  // mx_engine_set_host_cache waits on cv_done for this
        host_apply_capacity();
        cv_done.notify_all();
      }
      if (host_cap && !pending.empty() && !free_slots.empty()) host_round++;
      if (stop) {
        for (Request* r : pending) { r->error = "engine shutting down"; finish(r, MX_FINISH_ERROR); }
        for (Request* r : active) { r->error = "engine shutting down"; finish(r, MX_FINISH_ERROR); }
        pending.clear();
        active.clear();
        cv_done.notify_all();
        return;
      }
      while (!pending.empty() && !free_slots.empty()) {
        Request* r = pending.front();
        pending.pop_front();
        if (r->cancel) {  // cancelled before admission: no tokens
          finish(r, MX_FINISH_STOP);
          continue;
        }
        // the free slot sharing the longest prefix with this prompt (ties: most recently freed)
        size_t best = free_slots.size() - 1;
        int best_lcp = -1;
        for (size_t k = free_slots.size(); k-- > 0;) {
          const std::vector<int32_t>& st = slot_tokens[free_slots[k]];
          int l = 0;
          const int lim = (int)std::min(st.size(), r->prompt.size());
          while (l < lim && st[l] == r->prompt[l]) l++;
          if (l > best_lcp) best_lcp = l, best = k;
        }
        r->slot = free_slots[best];
        free_slots.erase(free_slots.begin() + best);
        // at least the last prompt token is evaluated (its logits start generation)
        const int n = (int)r->prompt.size();
        r->reuse = (r->lp_prompt || r->embd) ? 0 : std::min(best_lcp, n - 1);
        stat_prompt_tokens += r->prompt.size();
        stat_reused_tokens += r->reuse;
        // the longest match over the host entries of earlier rounds: worth a restore when it beats every device
        // source -- the slot's own record, a copy, a leader of this round -- by HOST_MIN (a device source of
        // equal length is cheaper and wins)
        std::shared_ptr<HostEntry> hsrc;
        int h = -1;
        if (host_cap && !r->lp_prompt && !r->embd)
          for (auto& e : host_entries) {
            const int l = e->born < host_round ? lcp(e->tokens, r->prompt) : -1;
            if (l > h) h = l, hsrc = e;
          }
        bool restore = hsrc && h - best_lcp >= HOST_MIN;
        if (restore) hsrc->used = ++host_clock;  // before the spill below looks for the least recently used
        if (host_cap && (int)slot_tokens[r->slot].size() >= HOST_MIN) {
          // the slot's record is about to be cut to what this request keeps of it: it goes to host memory unless
          // the prompt, another slot's record or a host entry holds it to within HOST_MIN positions
          const std::vector<int32_t>& st = slot_tokens[r->slot];
          const int L = (int)st.size();
          int cover = lcp(st, r->prompt);
          for (int s = 0; s < n_seq_max; s++)
            if (s != r->slot) cover = std::max(cover, lcp(st, slot_tokens[s]));
          for (auto& e : host_entries) {
            const int l = lcp(st, e->tokens);
            cover = std::max(cover, l);
            if (l == L) e->used = ++host_clock;  // it holds the record whole: as good as spilled again
          }
          if (L - cover >= HOST_MIN) host_insert(st, r->slot, spills);
        }
        if (prefix_sharing && !r->lp_prompt && !r->embd) {
          // the longest match over every other slot's record, free or busy (ties: a slot no copy of this round
          // writes, so no slot is both a source and a destination); worth a copy when it beats the slot's own by
          // SHARE_MIN
          int cur = best_lcp, src_slot = -1, src = -1;
          bool src_written = false;
          for (int s = 0; s < n_seq_max; s++) {
            if (s == r->slot) continue;
            const int l = lcp(slot_tokens[s], r->prompt);
            const bool written =
                std::any_of(pre.begin(), pre.end(), [&](const KvCopy& c) { return c.dst == s; }) ||
                std::any_of(restores.begin(), restores.end(), [&](const HostRestore& c) { return c.slot == s; });
            if (l > src || (l == src && src_written && !written)) src = l, src_slot = s, src_written = written;
          }
          const bool copy = src_slot >= 0 && src - cur >= SHARE_MIN;
          if (copy) cur = src;
          // ... or a request admitted earlier in this round that evaluates the prefix itself (not a follower)
          Request* lead = nullptr;
          int fl = -1;
          for (Request* a : admit) {
            if (std::find(followers.begin(), followers.end(), a) != followers.end()) continue;
            const int l = lcp(a->prompt, r->prompt);
            if (l > fl) fl = l, lead = a;
          }
          const bool follow = lead && fl - cur >= SHARE_MIN;
          restore = hsrc && h - (follow ? fl : cur) >= HOST_MIN;
          if (restore) {
            // no copy and no leader for this request: the host entry serves it (below)
          } else if (follow) {
            cur = fl;
            r->reuse = std::min(cur, n - 1);
            post.push_back({lead->slot, r->slot, r->reuse});
            followers.push_back(r);
            stat_followers++;
          } else if (copy) {
            r->reuse = std::min(cur, n - 1);
            pre.push_back({src_slot, r->slot, r->reuse});
          }
          stat_shared_tokens += r->reuse - std::min(best_lcp, n - 1);
        }
        if (restore) {
          r->reuse = std::min(h, n - 1);
          restores.push_back({hsrc, r->slot, r->reuse});
          hsrc->used = ++host_clock;
          stat_host_restored_tokens += r->reuse - std::min(best_lcp, n - 1);
        }
        // the record of the now busy slot: what it holds once the copies from slots as they stand have run (a
        // follower's copy runs after the others' prefill: until then its slot holds its own match only)
        const bool follows = !followers.empty() && followers.back() == r;
        const int held = follows ? std::min(best_lcp, n - 1) : r->reuse;
        slot_tokens[r->slot].assign(r->prompt.begin(), r->prompt.begin() + held);
        admit.push_back(r);
      }
    }
    std::lock_guard<std::mutex> glk(gpu_mu);
    if (!admit.empty()) {
      // copies from slots as they stand, then the prefill -- with followers: the others' prefill, one copy launch
      // from their slots, the followers' prefill.  Without sharing this is prefill_batch(admit), as ever.
      // With the host tier on, ahead of all that and in this order on the engine stream: the packs of the records
      // this round destroys (they read the slots before anything of the round writes them), the restores, then
      // the copies -- a slot a restore filled may be a copy's source.
      int rc = run_host_spills(spills);
      if (rc) {  // none of the round's entries may serve a later restore
        std::lock_guard<std::mutex> lk(mu);
        for (HostSpill& sp : spills) {
          const auto it = std::find(host_entries.begin(), host_entries.end(), sp.e);
          if (it != host_entries.end()) host_drop(it - host_entries.begin());
        }
      }
      if (!rc) rc = run_host_restores(restores);
      if (!rc) rc = run_kv_copies(pre);
      if (!rc && followers.empty()) {
        rc = prefill_batch(admit);
      } else if (!rc) {
        std::vector<Request*> leaders;
        for (Request* r : admit)
          if (std::find(followers.begin(), followers.end(), r) == followers.end()) leaders.push_back(r);
        rc = prefill_batch(leaders);
        if (!rc) rc = run_kv_copies(post);
        if (!rc) rc = prefill_batch(followers);
      }
      std::lock_guard<std::mutex> lk(mu);
      for (Request* r : admit) {
        if (rc) {
          // a copy, a restore or a prefill may not have run: the slot keeps no record
          if (!pre.empty() || !post.empty() || !restores.empty()) r->pos = 0;
          r->error = g_err;
          finish(r, MX_FINISH_ERROR);
          continue;
        }
        slot_tokens[r->slot] = r->prompt;
        if (r->embd) {  // no tokens: its vectors are in embd_out, the slot keeps the prompt's K/V
          finish(r, MX_FINISH_STOP);
          continue;
        }
        if (r->gram_end) {  // the grammar ended it in the prefill: a dead end, or its first token ends the grammar
          finish(r, r->gram_end - 1);
          continue;
        }
        const int32_t t = r->out.back();
        if ((is_eog(t) && !r->samp.ignore_eos) || r->cancel) finish(r, MX_FINISH_STOP);
        else if ((int)r->out.size() >= r->max_tokens || r->pos >= n_ctx) finish(r, MX_FINISH_LENGTH);
        else active.push_back(r);
      }
    }
    if (!host_trash.empty()) {  // evicted entries: a restore of this round may still have read one
      if (!restores.empty()) hipStreamSynchronize(stream);
      restores.clear();
      host_free_trash();
    }
    std::vector<Request*> rows;
    {
      std::lock_guard<std::mutex> lk(mu);
      active.erase(std::remove_if(active.begin(), active.end(), [](Request* r) { return r->done; }), active.end());
      for (Request* r : active)
        if ((int)rows.size() < MAX_ROWS) rows.push_back(r);
      cv_done.notify_all();
    }
    if (rows.empty()) continue;
    int rc = sched_step(rows);
    std::lock_guard<std::mutex> lk(mu);
    if (rc) {
      for (Request* r : rows) {
        r->error = g_err;
        if (!r->done) finish(r, MX_FINISH_ERROR);
      }
    }
    active.erase(std::remove_if(active.begin(), active.end(), [](Request* r) { return r->done; }), active.end());
    cv_done.notify_all();
  }
}

void mx::split_entries(const std::vector<float>& ent, int n, int k, float* tgt_lp, float* top_lp, int32_t* top_idx) {
  const size_t st = 1 + 2 * (size_t)k;
  for (int i = 0; i < n; i++) {
    const float* o = ent.data() + i * st;
    if (tgt_lp) tgt_lp[i] = o[0];
    if (top_lp && k) memcpy(top_lp + (size_t)i * k, o + 1, (size_t)k * 4);
    if (top_idx && k) memcpy(top_idx + (size_t)i * k, o + 1 + k, (size_t)k * 4);
  }
}

int mx::check_sampling_ext(const mx_sampling_ext* s, int V, SampExt* o, bool* has) {
  if (s->mirostat_mode == 1)
    return fail(MX_ERR_ARG, "mirostat_mode 1 is not supported (Mirostat v1 sorts the whole vocabulary); use 2");
  if (s->mirostat_mode != 0 && s->mirostat_mode != 2) return fail(MX_ERR_ARG, "mirostat_mode must be 0 or 2");
  if (std::isnan(s->typical_p) || std::isnan(s->tfs_z) || std::isnan(s->mirostat_tau) || std::isnan(s->mirostat_eta))
    return fail(MX_ERR_ARG, "NaN sampler setting");
  if (s->n_logit_bias < 0 || s->n_logit_bias > SAMP_BIAS_MAX)
    return fail(MX_ERR_ARG, "logit_bias: at most " + std::to_string(SAMP_BIAS_MAX) + " entries");
  if (s->n_logit_bias > 0 && (!s->bias_tok || !s->bias_val)) return fail(MX_ERR_ARG, "logit_bias: null table");
  memset(o, 0, sizeof(*o));
  std::vector<int32_t> seen(s->bias_tok, s->bias_tok + s->n_logit_bias);
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(MX_ERR_ARG, "logit_bias: duplicate token");
  for (int j = 0; j < s->n_logit_bias; j++) {
    const float b = s->bias_val[j];
    if (s->bias_tok[j] < 0 || s->bias_tok[j] >= V) return fail(MX_ERR_ARG, "logit_bias: token id outside the vocabulary");
    if (std::isnan(b) || b == INFINITY) return fail(MX_ERR_ARG, "logit_bias: NaN or +inf bias");
    o->bias_tok[j] = s->bias_tok[j];
    o->bias_val[j] = b;
  }
  o->n_bias = s->n_logit_bias;
  o->typical_p = s->typical_p;
  o->tfs_z = s->tfs_z;
  o->miro = s->mirostat_mode == 2 && s->base.temperature > 0.f ? 2 : 0;
  o->tau = s->mirostat_tau;
  o->eta = s->mirostat_eta;
  *has = o->typical_p < 1.0f || o->tfs_z < 1.0f || o->miro == 2 || o->n_bias > 0;
  return 0;
}

// ---------------------------------------------------------------- C ABI
extern "C" {

void mx_opts_default(mx_opts* o) {
  o->n_ctx = 512;
  o->n_seq_max = 64;
  o->layer_begin = 0;
  o->layer_end = -1;
  o->device = -1;
  o->use_graphs = 1;
  o->seed = 0;
  o->handoff_bf16 = 0;
}

void mx_sampling_default(mx_sampling* s) {
  s->temperature = 0.8f;
  s->top_k = 40;
  s->top_p = 0.95f;
  s->min_p = 0.05f;
  s->repeat_penalty = 1.0f;
  s->repeat_last_n = 64;
  s->seed = 0xFFFFFFFFull;
  s->ignore_eos = 0;
  s->frequency_penalty = 0.0f;
  s->presence_penalty = 0.0f;
}

const char* mx_last_error(void) { return g_err.c_str(); }

// the checks of mx_lora_check and mx_engine_create_lora: both files opened and the adapter validated against the
// base, no GPU touched
static int lora_open(const char* model_path, const char* lora_path, std::unique_ptr<LoraAdapter>& ad) {
  if (!model_path || !lora_path) return fail(MX_ERR_ARG, "null argument");
  if (std::string(model_path).rfind("synthetic:", 0) == 0)
    return fail(MX_ERR_ARG, "a LoRA adapter needs a GGUF base model, not a synthetic: one");
  GGUFFile base;
  std::string err = base.open(model_path);
  if (!err.empty()) return fail(MX_ERR_MODEL, err);
  ad.reset(new LoraAdapter());
  err = ad->open(lora_path, base);
  if (!err.empty()) {
    ad.reset();
    return fail(MX_ERR_MODEL, err);
  }
  return 0;
}

static int engine_create(const char* model_path, const mx_opts* opts, std::unique_ptr<LoraAdapter> lora,
                         float lora_scale, mx_engine** out) {
  mx_opts o;
  mx_opts_default(&o);
  if (opts) o = *opts;
  if (o.n_ctx < 1 || o.n_seq_max < 1) return fail(MX_ERR_ARG, "n_ctx and n_seq_max must be >= 1");
  std::unique_ptr<mx_engine> e(new mx_engine());
  if (lora) {
    e->has_lora = true;
    e->lora_scale = lora_scale;
    e->lora_alpha = lora->alpha;
    e->lora = std::move(lora);
  }
  e->n_ctx = o.n_ctx;
  e->n_seq_max = o.n_seq_max;
  e->lb = o.layer_begin;
  e->le = o.layer_end;
  e->use_graphs = o.use_graphs != 0 && getenv("MX_NO_GRAPHS") == nullptr;  // rocprofv3 runs set MX_NO_GRAPHS
  e->handoff_bf16 = o.handoff_bf16 != 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MX_ERR_HIP, "no HIP device visible");
  if (o.device >= 0) HIPC(hipSetDevice(o.device));
  HIPC(hipGetDevice(&e->device));
  HIPC(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  std::string path(model_path);
  int rc;
  if (path.rfind("synthetic:", 0) == 0) {
    std::string rest = path.substr(10), name = rest;
    uint64_t seed = o.seed;
    bool q8 = false, q4 = false;
    int kq = 0;
    size_t c = rest.find(':');
    if (c != std::string::npos) {
      name = rest.substr(0, c);
      std::string tail = rest.substr(c + 1);
      while (!tail.empty()) {  // ":seed=N" and/or ":q8_0"
        const size_t e2 = tail.find(':');
        const std::string part = tail.substr(0, e2);
        if (part.rfind("seed=", 0) == 0) seed = strtoull(part.c_str() + 5, nullptr, 10);
        else if (part == "q8_0") q8 = true;
        else if (part == "q4_0") q4 = true;
        else if (part == "q4_k_m") kq = 12;
        else if (part == "q5_k_m") kq = 13;
        else if (part != "bf16") return fail(MX_ERR_MODEL, "unknown synthetic option '" + part + "'");
        tail = e2 == std::string::npos ? "" : tail.substr(e2 + 1);
      }
    }
    const Shape* s = nullptr;
    for (const Shape& k : kShapes)
      if (name == k.name) s = &k;
    if (!s) return fail(MX_ERR_MODEL, "unknown synthetic shape '" + name + "'");
    rc = e->load_synthetic(*s, seed, q8, kq, q4);
  } else {
    rc = e->load_gguf(path);
  }
  e->lora.reset();  // the adapter file is needed no longer
  if (rc) return rc;
  *out = e.release();
  return 0;
}

int mx_engine_create(const char* model_path, const mx_opts* opts, mx_engine** out) {
  if (!model_path || !out) return fail(MX_ERR_ARG, "null argument");
  *out = nullptr;
  return engine_create(model_path, opts, nullptr, 0.f, out);
}

int mx_engine_create_lora(const char* model_path, const mx_opts* opts, const char* lora_path, float lora_scale,
                          mx_engine** out) {
  if (!model_path || !lora_path || !out) return fail(MX_ERR_ARG, "null argument");
  *out = nullptr;
  if (!std::isfinite(lora_scale)) return fail(MX_ERR_ARG, "lora_scale must be finite");
  std::unique_ptr<LoraAdapter> ad;
  if (int rc = lora_open(model_path, lora_path, ad)) return rc;  // before any device allocation
  return engine_create(model_path, opts, std::move(ad), lora_scale, out);
}

int mx_lora_check(const char* model_path, const char* lora_path) {
  std::unique_ptr<LoraAdapter> ad;
  return lora_open(model_path, lora_path, ad);
}

int mx_engine_lora_info(const mx_engine* e, mx_lora_info* o) {
  if (!e || !o) return fail(MX_ERR_ARG, "null argument");
  o->n_tensors = e->lora_merged;
  o->rank_max = e->lora_rank_max;
  o->alpha = e->has_lora ? e->lora_alpha : 0.f;
  o->lora_scale = e->has_lora ? e->lora_scale : 0.f;
  return 0;
}

void mx_engine_destroy(mx_engine* e) { delete e; }

int mx_gguf_check(const char* path) {
  if (!path) return fail(MX_ERR_ARG, "null path");
  GGUFFile f;
  const std::string err = f.open(path);
  return err.empty() ? MX_OK : fail(MX_ERR_MODEL, err);
}

int mx_engine_info(const mx_engine* e, mx_model_info* o) {
  if (!e || !o) return fail(MX_ERR_ARG, "null argument");
  o->n_embd = e->n_embd; o->n_layer = e->n_layer; o->n_head = e->n_head; o->n_head_kv = e->n_head_kv;
  o->head_dim = e->head_dim; o->n_ff = e->n_ff; o->n_vocab = e->n_vocab; o->n_ctx_train = e->n_ctx_train;
  o->eps = e->eps; o->rope_base = e->rope_base; o->bos_id = e->bos; o->eos_id = e->eos; o->eot_id = e->eot;
  o->n_ctx = e->n_ctx; o->n_seq_max = e->n_seq_max; o->layer_begin = e->lb; o->layer_end = e->le;
  o->has_embed = e->has_embed; o->has_head = e->has_head; o->weight_bytes = e->weight_bytes;
  o->weight_type = e->wq4 ? 2 : e->wq8 ? 8 : e->wkq ? e->kq_main_type : 30;
  return 0;
}

int mx_forward_rows(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                    float* logits_out) {
  if (!e || n < 0 || (n && (!slots || !pos || !ids))) return fail(MX_ERR_ARG, "bad arguments");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_forward_rows needs a full-model engine");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  const int chunk = (!logits_out && e->gemm_ok()) ? PREFILL_ROWS : MAX_ROWS;  // logits: <= 64 rows per chunk
  for (int i = 0; i < n; i += chunk) {
    int m = std::min(chunk, n - i);
    if (int rc = e->forward_rows_chunk(m, slots + i, pos + i, ids + i, nullptr, nullptr,
                                       logits_out ? logits_out + (size_t)i * e->n_vocab : nullptr, e->stream))
      return rc;
  }
  return 0;
}

int mx_forward_topk(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids, int k,
                    float* vals, int32_t* idx) {
  if (!e || n < 1 || n > MAX_ROWS || !slots || !pos || !ids || !vals || !idx || k < 1 || k > TOPK_MAX)
    return fail(MX_ERR_ARG, "mx_forward_topk: 1 <= n <= 64 rows, 1 <= k <= 64");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_forward_topk needs a full-model engine");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  std::vector<float> lg((size_t)n * e->n_vocab);  // the logits stay on the device too (e->logits)
  if (int rc = e->forward_rows_chunk(n, slots, pos, ids, nullptr, nullptr, lg.data(), e->stream)) return rc;
  if (launch_topk(e->logits, e->n_vocab, n, e->n_vocab, k, e->tk_ws_val, e->tk_ws_idx, e->tk_val, e->tk_idx,
                  e->stream))
    return fail(MX_ERR_ARG, "top-k launch shape");
  HIPC(hipMemcpyAsync(vals, e->tk_val, (size_t)n * k * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(idx, e->tk_idx, (size_t)n * k * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return 0;
}

int mx_forward_logits(mx_engine* e, int slot, const int32_t* ids, int n, int pos0, float* logits_out) {
  if (!e || n < 0) return fail(MX_ERR_ARG, "bad arguments");
  if (pos0 < 0 || pos0 + n > e->n_ctx) return fail(MX_ERR_CTX, "tokens exceed n_ctx");
  std::vector<int32_t> slots(n, slot), pos(n);
  for (int i = 0; i < n; i++) pos[i] = pos0 + i;
  return mx_forward_rows(e, n, slots.data(), pos.data(), ids, logits_out);
}

int mx_stage_rows(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                  const void* x_in, void* x_out, float* logits_out, void* stream) {
  if (!e || n < 1 || n > MAX_ROWS) return fail(MX_ERR_ARG, "mx_stage_rows: 1 <= n <= 64 rows per call");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  return e->forward_rows_chunk(n, slots, pos, ids, x_in, x_out, logits_out, s);
}

int mx_debug(mx_engine* e, int op, long long arg, void* host, size_t bytes) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  switch (op) {
    case 0: e->dbg_stop = (int)arg; return 0;
    case 1: e->dbg_sync = arg != 0; return 0;
    case 2: {
      const size_t R = PREFILL_ROWS, nl = e->layers.size();
      const void* src = nullptr;
      size_t n = 0;
      switch (arg) {
        case 0: src = e->x, n = R * e->n_embd * 4; break;
        case 1: src = e->q, n = R * e->n_embd * 4; break;
        case 2: src = e->xn, n = R * e->n_embd * 2; break;
        case 3: src = e->attn_out, n = R * e->n_embd * 2; break;
        case 4: src = e->act, n = R * e->n_ff * 2; break;
        case 5: src = e->slabs, n = e->slab_stride * 8 * 4; break;
        case 6: src = e->kcache, n = e->layer_kv_stride * nl * 2; break;
        case 7: src = e->vcache, n = e->layer_kv_stride * nl * 2; break;
        case 8: src = e->ssq, n = R * (e->n_embd / 16) * 4; break;
        case 9: src = e->d_pos, n = R * 4; break;
        case 10: src = e->d_slot, n = R * 4; break;
        case 11: src = e->rope_cs, n = (size_t)e->n_ctx * e->head_dim * 4; break;
        default: return fail(MX_ERR_ARG, "mx_debug: unknown buffer");
      }
      if (!host) return fail(MX_ERR_ARG, "mx_debug: null host buffer");
      HIPC(hipDeviceSynchronize());
      HIPC(hipMemcpy(host, src, std::min(n, bytes), hipMemcpyDeviceToHost));
      return 0;
    }
  }
  return fail(MX_ERR_ARG, "mx_debug: unknown op");
}

static int make_request(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens,
                        std::unique_ptr<Request>* out) {
  if (!ids || n < 1) return fail(MX_ERR_ARG, "bad arguments");
  if (n >= e->n_ctx) return fail(MX_ERR_CTX, "Requested tokens (" + std::to_string(n) + ") exceed context window of " +
                                                 std::to_string(e->n_ctx));
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= e->n_vocab) return fail(MX_ERR_ARG, "token id out of range");
  auto r = std::make_unique<Request>();
  r->prompt.assign(ids, ids + n);
  mx_sampling_default(&r->samp);
  if (s) r->samp = *s;
  r->max_tokens = max_tokens <= 0 ? e->n_ctx - n : std::min(max_tokens, e->n_ctx - n);
  r->seed = r->samp.seed == 0xFFFFFFFFull ? ((uint64_t)std::random_device{}() << 32 | std::random_device{}())
                                           : r->samp.seed;
  *out = std::move(r);
  return 0;
}

// Hands n prepared requests to the scheduler under one lock, so that it admits them in the same round (one
// batched prefill, one decode batch); ids[i] is request i's id.  The first call starts the scheduler thread.
static int enqueue_requests(mx_engine* e, std::unique_ptr<Request>* rs, int n, uint64_t* ids) {
  {
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->stop) return fail(MX_ERR_STATE, "engine shutting down");
    for (int i = 0; i < n; i++) {
      Request* r = rs[i].get();
      r->id = e->next_id++;
      ids[i] = r->id;
      e->pending.push_back(r);
      e->requests[r->id] = std::move(rs[i]);
    }
    if (!e->worker_started) {
      e->worker_started = true;
      e->worker = std::thread([e] { e->scheduler_loop(); });
    }
  }
  e->cv.notify_all();
  return 0;
}

// all-or-nothing: every request is validated first, then all are queued under one lock, so the
// scheduler admits them in the same round (one batched prefill, one decode batch)
int mx_submit_batch(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens, const mx_sampling* s,
                    const int32_t* max_tokens, uint64_t* reqs) {
  if (!e || n_req < 1 || !ids || !lens || !max_tokens || !reqs) return fail(MX_ERR_ARG, "bad arguments");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  std::vector<std::unique_ptr<Request>> rs(n_req);
  for (int i = 0; i < n_req; i++)
    if (int rc = make_request(e, ids[i], lens[i], s ? s + i : nullptr, max_tokens[i], &rs[i])) return rc;
  return enqueue_requests(e, rs.data(), n_req, reqs);
}

int mx_submit(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, uint64_t* req) {
  if (!e || !ids || n < 1 || !req) return fail(MX_ERR_ARG, "bad arguments");
  const int32_t len = n;
  return mx_submit_batch(e, 1, &ids, &len, s, &max_tokens, req);
}

int mx_submit_lp(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, int n_logprobs,
                 int prompt_logprobs, uint64_t* req) {
  if (!e || !ids || n < 1 || !req) return fail(MX_ERR_ARG, "bad arguments");
  if (n_logprobs < 0 || n_logprobs > TOPK_MAX) return fail(MX_ERR_ARG, "mx_submit_lp: n_logprobs must be 0..64");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  std::unique_ptr<Request> r;
  if (int rc = make_request(e, ids, n, s, max_tokens, &r)) return rc;
  r->lp_k = std::min(n_logprobs, e->n_vocab);
  r->lp_prompt = prompt_logprobs != 0;
  return enqueue_requests(e, &r, 1, req);
}

int mx_request_logprobs(mx_engine* e, uint64_t req, float* tok_lp, float* top_lp, int32_t* top_idx, int cap, int* n_out,
                        int* k_out) {
  if (!e || cap < 0) return fail(MX_ERR_ARG, "bad arguments");
  std::lock_guard<std::mutex> lk(e->mu);
  auto it = e->requests.find(req);
  if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
  const Request* r = it->second.get();
  if (r->lp_k < 0) return fail(MX_ERR_ARG, "request was submitted without log-probabilities");
  const size_t n = r->lp_tok.size(), c = std::min<size_t>(n, cap), k = r->lp_k;
  if (tok_lp && c) memcpy(tok_lp, r->lp_tok.data(), c * 4);
  if (top_lp && c * k) memcpy(top_lp, r->lp_top.data(), c * k * 4);
  if (top_idx && c * k) memcpy(top_idx, r->lp_idx.data(), c * k * 4);
  if (n_out) *n_out = (int)n;
  if (k_out) *k_out = (int)k;
  return 0;
}

int mx_forward_logprobs(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                        const int32_t* targets, int k, float* tgt_lp, float* top_lp, int32_t* top_idx,
                        float* logits_out) {
  if (!e || n < 1 || n > MAX_ROWS || !slots || !pos || !ids || !targets || !tgt_lp || k < 0 || k > TOPK_MAX ||
      (k && (!top_lp || !top_idx)))
    return fail(MX_ERR_ARG, "mx_forward_logprobs: 1 <= n <= 64 rows, 0 <= k <= 64");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_forward_logprobs needs a full-model engine");
  for (int i = 0; i < n; i++)
    if (targets[i] < 0 || targets[i] >= e->n_vocab) return fail(MX_ERR_ARG, "target id out of range");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  k = std::min(k, e->n_vocab);
  std::vector<float> lg;  // the rows stay on the device too (e->logits): the statistics read those
  if (!logits_out) lg.resize((size_t)n * e->n_vocab), logits_out = lg.data();
  if (int rc = e->forward_rows_chunk(n, slots, pos, ids, nullptr, nullptr, logits_out, e->stream)) return rc;
  std::vector<float> ent((size_t)n * (1 + 2 * k));
  HIPC(hipMemcpyAsync(e->lp_tgt, targets, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  if (launch_logprobs(e->logits, e->n_vocab, n, e->n_vocab, k, e->lp_tgt, e->tk_ws_val, e->tk_ws_idx, e->lp_part,
                      e->lp_ms, e->lp_top, e->lp_idx, e->lp_hist, e->stream)) {
    hipStreamSynchronize(e->stream);
    return fail(MX_ERR_ARG, "log-prob launch shape");
  }
  HIPC(hipMemcpyAsync(ent.data(), e->lp_hist, ent.size() * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  split_entries(ent, n, k, tgt_lp, top_lp, top_idx);
  return 0;
}

void mx_sampling_ext_default(mx_sampling_ext* s) {
  mx_sampling_default(&s->base);
  s->typical_p = 1.0f;
  s->tfs_z = 1.0f;
  s->mirostat_mode = 0;
  s->mirostat_tau = 5.0f;
  s->mirostat_eta = 0.1f;
  s->n_logit_bias = 0;
  s->bias_tok = nullptr;
  s->bias_val = nullptr;
}

int mx_submit_ext(mx_engine* e, const int32_t* ids, int n, const mx_sampling_ext* s, int max_tokens, int n_logprobs,
                  int prompt_logprobs, uint64_t* req) {
  if (!e || !ids || n < 1 || !req || !s) return fail(MX_ERR_ARG, "bad arguments");
  if (n_logprobs < -1 || n_logprobs > TOPK_MAX) return fail(MX_ERR_ARG, "mx_submit_ext: n_logprobs must be -1..64");
  if (n_logprobs < 0 && prompt_logprobs) return fail(MX_ERR_ARG, "mx_submit_ext: prompt_logprobs needs n_logprobs >= 0");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  std::unique_ptr<Request> r;
  if (int rc = make_request(e, ids, n, &s->base, max_tokens, &r)) return rc;
  if (int rc = check_sampling_ext(s, e->n_vocab, &r->ext, &r->has_ext)) return rc;
  r->mu = 2.0f * s->mirostat_tau;
  if (n_logprobs >= 0) {
    r->lp_k = std::min(n_logprobs, e->n_vocab);
    r->lp_prompt = prompt_logprobs != 0;
  }
  return enqueue_requests(e, &r, 1, req);
}

int mx_submit_ext_batch(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens,
                        const mx_sampling_ext* s, const int32_t* max_tokens, uint64_t* reqs) {
  if (!e || n_req < 1 || !ids || !lens || !s || !max_tokens || !reqs) return fail(MX_ERR_ARG, "bad arguments");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  std::vector<std::unique_ptr<Request>> rs(n_req);
  for (int i = 0; i < n_req; i++) {
    if (int rc = make_request(e, ids[i], lens[i], &s[i].base, max_tokens[i], &rs[i])) return rc;
    if (int rc = check_sampling_ext(&s[i], e->n_vocab, &rs[i]->ext, &rs[i]->has_ext)) return rc;
    rs[i]->mu = 2.0f * s[i].mirostat_tau;
  }
  return enqueue_requests(e, rs.data(), n_req, reqs);
}

// ---- grammar.  The handles hold shared pointers: a grammar keeps its vocabulary alive, a state
// and a request their grammar.
struct mx_vocab {
  std::shared_ptr<const gram::Vocab> p;
};
struct mx_grammar {
  std::shared_ptr<gram::Grammar> p;
};
struct mx_grammar_state {
  gram::State s;
};
constexpr int GRAMMAR_CACHE_DEFAULT = 256;

int mx_vocab_create(int n_vocab, const uint8_t* blob, const uint64_t* offsets, const int32_t* eog_ids, int n_eog,
                    mx_vocab** out) {
  if (!out) return fail(MX_ERR_ARG, "mx_vocab_create: null out");
  std::shared_ptr<const gram::Vocab> v;
  const std::string err = gram::Vocab::create(n_vocab, blob, offsets, eog_ids, n_eog, &v);
  if (!err.empty()) return fail(MX_ERR_ARG, "mx_vocab_create: " + err);
  *out = new mx_vocab{std::move(v)};
  return 0;
}

void mx_vocab_destroy(mx_vocab* v) { delete v; }

int mx_grammar_create(const mx_vocab* v, const char* gbnf, int cache_entries, mx_grammar** out) {
  if (!v || !gbnf || !out) return fail(MX_ERR_ARG, "mx_grammar_create: null argument");
  std::shared_ptr<gram::Grammar> g;
  const std::string err =
      gram::Grammar::create(v->p, gbnf, cache_entries < 0 ? GRAMMAR_CACHE_DEFAULT : cache_entries, &g);
  if (!err.empty()) return fail(MX_ERR_ARG, err);
  *out = new mx_grammar{std::move(g)};
  return 0;
}

void mx_grammar_destroy(mx_grammar* g) { delete g; }

int mx_grammar_state_create(const mx_grammar* g, mx_grammar_state** out) {
  if (!g || !out) return fail(MX_ERR_ARG, "mx_grammar_state_create: null argument");
  *out = new mx_grammar_state{gram::State(g->p)};
  return 0;
}

int mx_grammar_state_mask(mx_grammar_state* s, uint32_t* words, int n_words, int32_t* status) {
  if (!s || !words || !status) return fail(MX_ERR_ARG, "mx_grammar_state_mask: null argument");
  const int nw = (s->s.grammar()->vocab->n_vocab + 31) / 32;
  if (n_words != nw) return fail(MX_ERR_ARG, "mx_grammar_state_mask: n_words must be " + std::to_string(nw));
  std::shared_ptr<const std::vector<uint32_t>> m;
  *status = s->s.mask(&m);
  memcpy(words, m->data(), (size_t)nw * 4);
  return 0;
}

int mx_grammar_state_accept(mx_grammar_state* s, int32_t token) {
  if (!s) return fail(MX_ERR_ARG, "mx_grammar_state_accept: null state");
  if (!s->s.accept(token)) return fail(MX_ERR_ARG, "grammar: token " + std::to_string(token) + " is not allowed here");
  return 0;
}

int mx_grammar_state_may_end(const mx_grammar_state* s, int32_t* may_end) {
  if (!s || !may_end) return fail(MX_ERR_ARG, "mx_grammar_state_may_end: null argument");
  *may_end = s->s.may_end() ? 1 : 0;
  return 0;
}

void mx_grammar_state_destroy(mx_grammar_state* s) { delete s; }

int mx_grammar_cache_stats(const mx_grammar* g, uint64_t* hits, uint64_t* misses, uint64_t* entries) {
  if (!g) return fail(MX_ERR_ARG, "mx_grammar_cache_stats: null grammar");
  g->p->stats(hits, misses, entries);
  return 0;
}

int mx_submit_grammar(mx_engine* e, const int32_t* ids, int n, const mx_sampling_ext* s, int max_tokens,
                      int n_logprobs, int prompt_logprobs, const mx_grammar* grammar, uint64_t* req) {
  if (!e || !ids || n < 1 || !req || !grammar) return fail(MX_ERR_ARG, "bad arguments");
  if (n_logprobs < -1 || n_logprobs > TOPK_MAX) return fail(MX_ERR_ARG, "mx_submit_grammar: n_logprobs must be -1..64");
  if (n_logprobs < 0 && prompt_logprobs)
    return fail(MX_ERR_ARG, "mx_submit_grammar: prompt_logprobs needs n_logprobs >= 0");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  if (grammar->p->vocab->n_vocab != e->n_vocab)
    return fail(MX_ERR_ARG, "mx_submit_grammar: the grammar's vocabulary has " +
                                std::to_string(grammar->p->vocab->n_vocab) + " tokens, the model " +
                                std::to_string(e->n_vocab));
  mx_sampling_ext dflt;
  if (!s) mx_sampling_ext_default(&dflt), s = &dflt;
  std::unique_ptr<Request> r;
  if (int rc = make_request(e, ids, n, &s->base, max_tokens, &r)) return rc;
  if (int rc = check_sampling_ext(s, e->n_vocab, &r->ext, &r->has_ext)) return rc;
  r->mu = 2.0f * s->mirostat_tau;
  if (n_logprobs >= 0) {
    r->lp_k = std::min(n_logprobs, e->n_vocab);
    r->lp_prompt = prompt_logprobs != 0;
  }
  r->gram = std::make_unique<gram::State>(grammar->p);
  return enqueue_requests(e, &r, 1, req);
}

int mx_submit_spec(mx_engine* e, const int32_t* ids, int n, const mx_sampling* s, int max_tokens, int num_pred_tokens,
                   int max_ngram_size, uint64_t* req) {
  if (!e || !ids || n < 1 || !req) return fail(MX_ERR_ARG, "bad arguments");
  if (num_pred_tokens < 1 || num_pred_tokens > SPEC_MAX_DRAFT || max_ngram_size < 1)
    return fail(MX_ERR_ARG, "mx_submit_spec: num_pred_tokens must be 1..15 and max_ngram_size >= 1");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit needs a full-model engine");
  std::unique_ptr<Request> r;
  if (int rc = make_request(e, ids, n, s, max_tokens, &r)) return rc;
  r->spec_d = num_pred_tokens;
  r->spec_ng = max_ngram_size;
  return enqueue_requests(e, &r, 1, req);
}

int mx_sample_plan(const mx_sampling_ext* s, int V, int32_t* path) {
  if (!s || !path || V < 1) return fail(MX_ERR_ARG, "mx_sample_plan: settings, V >= 1 and path");
  SampExt x;
  bool has = false;
  if (int rc = check_sampling_ext(s, V, &x, &has)) return rc;
  int k = 1;
  *path = sample_path(s->base, x, V, &k);
  return 0;
}

int mx_sampler_stats(mx_engine* e, mx_sampler_counts* out) {
  if (!e || !out) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *out = {e->stat_dev_steps, e->stat_host_steps, e->stat_wide_rows, e->stat_rounds};
  return 0;
}

int mx_spec_stats(mx_engine* e, uint64_t req, mx_spec_counts* out) {
  if (!e || !out) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (req == 0) {
    *out = {e->stat_spec_steps, e->stat_spec_drafted, e->stat_spec_accepted};
    return 0;
  }
  auto it = e->requests.find(req);
  if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
  *out = {it->second->spec_steps, it->second->spec_drafted, it->second->spec_accepted};
  return 0;
}

int mx_wait(mx_engine* e, uint64_t req, int32_t* out_ids, int cap, int* n_out, int* finish) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  std::unique_ptr<Request> r;
  {
    std::unique_lock<std::mutex> lk(e->mu);
    auto it = e->requests.find(req);
    if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
    Request* rp = it->second.get();
    if (rp->embd) return fail(MX_ERR_ARG, "mx_wait: an embedding request (use mx_wait_embed)");
    e->cv_done.wait(lk, [&] { return rp->done; });
    if (n_out) *n_out = (int)rp->out.size();
    if ((int)rp->out.size() > cap && rp->finish != MX_FINISH_ERROR)
      return fail(MX_ERR_ARG, "mx_wait: " + std::to_string(rp->out.size()) + " tokens do not fit cap " +
                                  std::to_string(cap) + " (request kept; retry with a larger buffer)");
    r = std::move(it->second);
    e->requests.erase(it);
  }
  int n = std::min<int>(cap, (int)r->out.size());
  if (out_ids && n > 0) memcpy(out_ids, r->out.data(), n * 4);
  if (n_out) *n_out = (int)r->out.size();
  if (finish) *finish = r->finish;
  if (r->finish == MX_FINISH_ERROR) return fail(MX_ERR_STATE, "request failed: " + r->error);
  return 0;
}

int mx_poll(mx_engine* e, uint64_t req, int n_have, int32_t* out_ids, int cap, int* n_out, int* done) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  std::unique_lock<std::mutex> lk(e->mu);
  auto it = e->requests.find(req);
  if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
  Request* rp = it->second.get();
  if (rp->embd) return fail(MX_ERR_ARG, "mx_poll: an embedding request (use mx_wait_embed)");
  e->cv_done.wait(lk, [&] { return rp->done || (int)rp->out.size() > n_have; });
  const int n = (int)rp->out.size();
  if (out_ids && cap > 0) memcpy(out_ids, rp->out.data(), (size_t)std::min(cap, n) * 4);
  if (n_out) *n_out = n;
  if (done) *done = rp->done ? 1 : 0;
  return 0;
}

int mx_cancel(mx_engine* e, uint64_t req) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  auto it = e->requests.find(req);
  if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
  it->second->cancel = true;
  return 0;
}

// all-or-nothing as mx_submit_batch: validated first, then queued under one lock, so the scheduler admits
// them in one round and prefill_embed evaluates them in one batched pass
int mx_submit_embed(mx_engine* e, int n_req, const int32_t* const* ids, const int32_t* lens, int pooling, int normalize,
                    uint64_t* reqs) {
  if (!e || n_req < 1 || !ids || !lens || !reqs) return fail(MX_ERR_ARG, "bad arguments");
  if (pooling < MX_POOL_NONE || pooling > MX_POOL_LAST)
    return fail(MX_ERR_ARG, "mx_submit_embed: pooling must be MX_POOL_NONE, MEAN, CLS or LAST");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "mx_submit_embed needs a full-model engine");
  std::vector<std::unique_ptr<Request>> rs(n_req);
  for (int i = 0; i < n_req; i++) {
    const int n = lens[i];
    if (!ids[i] || n < 1) return fail(MX_ERR_ARG, "mx_submit_embed: empty input");
    if (n > e->n_ctx)
      return fail(MX_ERR_CTX, "Requested tokens (" + std::to_string(n) + ") exceed context window of " +
                                  std::to_string(e->n_ctx));
    for (int j = 0; j < n; j++)
      if (ids[i][j] < 0 || ids[i][j] >= e->n_vocab) return fail(MX_ERR_ARG, "token id out of range");
    rs[i] = std::make_unique<Request>();
    rs[i]->prompt.assign(ids[i], ids[i] + n);
    mx_sampling_default(&rs[i]->samp);
    rs[i]->embd = true;
    rs[i]->embd_pool = pooling;
    rs[i]->embd_l2 = normalize != 0;
  }
  return enqueue_requests(e, rs.data(), n_req, reqs);
}

int mx_wait_embed(mx_engine* e, uint64_t req, float* out, size_t cap_floats, int* rows_out) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  std::unique_ptr<Request> r;
  {
    std::unique_lock<std::mutex> lk(e->mu);
    auto it = e->requests.find(req);
    if (it == e->requests.end()) return fail(MX_ERR_NOTFOUND, "unknown request id");
    Request* rp = it->second.get();
    if (!rp->embd) return fail(MX_ERR_ARG, "mx_wait_embed: not an embedding request (use mx_wait)");
    e->cv_done.wait(lk, [&] { return rp->done; });
    const bool ok = rp->finish != MX_FINISH_ERROR && rp->embd_rows > 0;
    if (rows_out) *rows_out = ok ? rp->embd_rows : 0;
    if (ok && (rp->embd_out.size() > cap_floats || !out))
      return fail(MX_ERR_ARG, "mx_wait_embed: " + std::to_string(rp->embd_out.size()) + " floats do not fit cap " +
                                  std::to_string(cap_floats) + " (request kept; retry with a larger buffer)");
    r = std::move(it->second);
    e->requests.erase(it);
  }
  if (r->finish == MX_FINISH_ERROR) return fail(MX_ERR_STATE, "request failed: " + r->error);
  if (r->embd_rows == 0) return fail(MX_ERR_STATE, "request was cancelled before it ran");
  memcpy(out, r->embd_out.data(), r->embd_out.size() * 4);
  return 0;
}

int mx_batch_create(mx_engine* e, int M, const int32_t* slots, const int32_t* pos, const int32_t* ids, int max_steps,
                    mx_batch** out) {
  if (!e || !out || M < 1 || M > MAX_ROWS || !slots || !pos || max_steps < 0) return fail(MX_ERR_ARG, "bad arguments");
  int max_pos = 0;
  for (int i = 0; i < M; i++) {
    if (slots[i] < 0 || slots[i] >= e->n_seq_max) return fail(MX_ERR_ARG, "slot out of range");
    if (pos[i] < 0 || pos[i] >= e->n_ctx) return fail(MX_ERR_CTX, "position outside n_ctx");
    if (ids && (ids[i] < 0 || ids[i] >= e->n_vocab)) return fail(MX_ERR_ARG, "token id out of range");
    max_pos = std::max(max_pos, (int)pos[i]);
  }
  {
    std::lock_guard<std::mutex> lk(e->mu);
    for (int i = 0; i < M; i++) e->slot_tokens[slots[i]].clear();  // decode steps will overwrite them
  }
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  std::unique_ptr<mx_batch> b(new mx_batch());
  b->M = M;
  b->max_steps = max_steps;
  {
    std::vector<int32_t> sorted(slots, slots + M);
    std::sort(sorted.begin(), sorted.end());
    b->distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
  }
  b->max_pos = max_pos;
  HIPC(hipMalloc((void**)&b->d_ids, M * 4));
  HIPC(hipMalloc((void**)&b->d_pos, M * 4));
  HIPC(hipMalloc((void**)&b->d_slot, M * 4));
  HIPC(hipMalloc((void**)&b->d_hist, (size_t)M * std::max(1, max_steps) * 4));
  HIPC(hipMalloc((void**)&b->d_hist_count, M * 4));
  HIPC(hipMemcpy(b->d_pos, pos, M * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(b->d_slot, slots, M * 4, hipMemcpyHostToDevice));
  if (ids) HIPC(hipMemcpy(b->d_ids, ids, M * 4, hipMemcpyHostToDevice));
  else HIPC(hipMemset(b->d_ids, 0, M * 4));
  HIPC(hipMemset(b->d_hist_count, 0, M * 4));
  *out = b.release();
  return 0;
}

int32_t* mx_batch_ids_device(mx_batch* b) { return b ? b->d_ids : nullptr; }

int mx_batch_bind_ids(mx_engine* e, mx_batch* b, int32_t* ids_device) {
  if (!e || !b || !ids_device) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(ids_device, b->d_ids, b->M * 4, hipMemcpyDeviceToDevice));
  if (!b->ids_external) hipFree(b->d_ids);
  b->d_ids = ids_device;
  b->ids_external = true;
  for (auto& kv : b->graphs) hipGraphExecDestroy(kv.second);
  b->graphs.clear();
  return 0;
}

int mx_batch_step(mx_engine* e, mx_batch* b, const void* x_in, void* x_out, void* stream) {
  if (!e || !b) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  const bool head = x_out == nullptr;
  if (b->max_pos >= e->n_ctx) return fail(MX_ERR_CTX, "decode batch reached n_ctx");
  b->max_pos++;
  if (head && !e->has_head) return fail(MX_ERR_STATE, "x_out is required on a non-final pipeline stage");
  if (!x_in && !e->has_embed) return fail(MX_ERR_STATE, "x_in is required on a non-first pipeline stage");
  auto body = [&]() -> int {
    e->rows_distinct = b->distinct;
    e->pick_samp = head && b->ktop > 0 ? b->d_samp : nullptr;
    e->pick_k = head ? b->ktop : 0;
    struct Reset {
      mx_engine* e;
      ~Reset() { e->rows_distinct = false; e->pick_samp = nullptr; e->pick_k = 0; }
    } reset_flags{e};
    if (int rc = e->enqueue_forward(
            {.M = b->M, .ids = b->d_ids, .pos = b->d_pos, .slot = b->d_slot, .x_in = x_in, .x_out = x_out, .head = head,
             .n_out = b->M, .argmax = head,
             .out = {.ids_next = b->d_ids, .pos_next = b->d_pos, .hist = b->d_hist, .hist_stride = b->max_steps,
                     .hist_count = b->d_hist_count, .max_hist = b->max_steps}},
            s))
      return rc;
    if (!head) advance_pos_kernel<<<(b->M + 63) / 64, 64, 0, s>>>(b->d_pos, b->M);
    return 0;
  };
  if (!e->use_graphs) return body();
  GraphKey key{b->M, x_in, x_out, s, head ? b->ktop : 0};
  auto it = b->graphs.find(key);
  if (it == b->graphs.end()) {
    hipGraph_t g;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = body();
    hipError_t ce = hipStreamEndCapture(s, &g);
    if (rc) return rc;
    if (ce != hipSuccess) return fail(MX_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce));
    hipGraphExec_t ex;
    HIPC(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    it = b->graphs.emplace(key, ex).first;
  }
  HIPC(hipGraphLaunch(it->second, s));
  return 0;
}

int mx_batch_tokens(mx_engine* e, mx_batch* b, int32_t* out, int cap, int* n_steps) {
  if (!e || !b) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  HIPC(hipDeviceSynchronize());
  std::vector<int32_t> cnt(b->M);
  HIPC(hipMemcpy(cnt.data(), b->d_hist_count, b->M * 4, hipMemcpyDeviceToHost));
  if (n_steps) *n_steps = cnt[0];
  if (out && cap > 0 && b->max_steps > 0) {
    std::vector<int32_t> h((size_t)b->M * b->max_steps);
    HIPC(hipMemcpy(h.data(), b->d_hist, h.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < b->M; i++)
      for (int j = 0; j < cap && j < b->max_steps; j++) out[(size_t)i * cap + j] = h[(size_t)i * b->max_steps + j];
  }
  return 0;
}

void mx_batch_destroy(mx_engine* e, mx_batch* b) {
  if (!b) return;
  if (e) {
    std::lock_guard<std::mutex> lk(e->gpu_mu);
    hipSetDevice(e->device);
    hipDeviceSynchronize();
  }
  for (auto& kv : b->graphs) hipGraphExecDestroy(kv.second);
  if (!b->ids_external) hipFree(b->d_ids);
  hipFree(b->d_pos);
  hipFree(b->d_slot);
  hipFree(b->d_hist);
  hipFree(b->d_hist_count);
  if (b->d_samp) hipFree(b->d_samp);
  delete b;
}

static int fill_samp_rows(mx_engine* e, int n, const mx_row_sampler* rows, std::vector<SampRow>& out, int* ktop) {
  out.assign(n, SampRow{});
  *ktop = 0;
  for (int i = 0; i < n; i++) {
    const mx_sampling& sp = rows[i].s;
    const bool sampling = sp.temperature > 0.f || has_penalties(sp);
    if (sampling && !device_sampleable(sp))
      return fail(MX_ERR_ARG, "row " + std::to_string(i) + ": sampling settings need the host sampler "
                                  "(top_k outside 1..64 or a penalty window over 64 tokens)");
    if (rows[i].n_win < 0 || rows[i].n_win > SAMP_WIN) return fail(MX_ERR_ARG, "penalty window over 64 tokens");
    SampRow& o = out[i];
    o.temp = sp.temperature; o.top_p = sp.top_p; o.min_p = sp.min_p; o.repeat = sp.repeat_penalty;
    o.freq = sp.frequency_penalty; o.presence = sp.presence_penalty;
    o.top_k = std::max(1, std::min(sp.top_k, TOPK_MAX));
    o.last_n = has_penalties(sp) ? std::min(sp.repeat_last_n, SAMP_WIN) : 0;
    o.seed = rows[i].seed;
    o.draw0 = rows[i].n_drawn;
    o.n_win = std::min(rows[i].n_win, o.last_n);
    for (int j = 0; j < o.n_win; j++) o.win[j] = rows[i].win[rows[i].n_win - o.n_win + j];
    if (sampling) *ktop = std::max(*ktop, std::min(o.top_k, e->n_vocab));
  }
  return 0;
}

int mx_batch_reset(mx_engine* e, mx_batch* b, const int32_t* pos, const int32_t* ids, const mx_row_sampler* rows,
                   void* stream) {
  if (!e || !b || !pos) return fail(MX_ERR_ARG, "null argument");
  int max_pos = 0;
  for (int i = 0; i < b->M; i++) {
    if (pos[i] < 0 || pos[i] >= e->n_ctx) return fail(MX_ERR_CTX, "position outside n_ctx");
    if (ids && (ids[i] < 0 || ids[i] >= e->n_vocab)) return fail(MX_ERR_ARG, "token id out of range");
    max_pos = std::max(max_pos, (int)pos[i]);
  }
  std::vector<SampRow> sr;
  int ktop = 0;
  if (rows)
    if (int rc = fill_samp_rows(e, b->M, rows, sr, &ktop)) return rc;
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  HIPC(hipMemcpyAsync(b->d_pos, pos, b->M * 4, hipMemcpyHostToDevice, s));
  if (ids) HIPC(hipMemcpyAsync(b->d_ids, ids, b->M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(b->d_hist_count, 0, b->M * 4, s));
  if (ktop > 0) {
    if (!b->d_samp) HIPC(hipMalloc((void**)&b->d_samp, (size_t)MAX_ROWS * sizeof(SampRow)));
    HIPC(hipMemcpyAsync(b->d_samp, sr.data(), b->M * sizeof(SampRow), hipMemcpyHostToDevice, s));
  }
  HIPC(hipStreamSynchronize(s));  // the host arrays may go away when this returns
  b->ktop = ktop;
  b->max_pos = max_pos;
  return 0;
}

int mx_stage_rows_pick(mx_engine* e, int n, const int32_t* slots, const int32_t* pos, const int32_t* ids,
                       const void* x_in, void* x_out, int n_out, const int32_t* rowmap, const mx_row_sampler* samp,
                       int32_t* tok_out, void* stream) {
  if (!e || n < 1 || !slots || !pos || n_out < 0 || (n_out && (!rowmap || !tok_out)))
    return fail(MX_ERR_ARG, "mx_stage_rows_pick: bad arguments");
  if (!x_in && (!e->has_embed || !ids)) return fail(MX_ERR_STATE, "x_in is required on a non-first pipeline stage");
  if (n_out && (x_out || !e->has_head)) return fail(MX_ERR_STATE, "tokens are picked on the last stage only");
  for (int k = 0; k < n_out; k++)
    if (rowmap[k] < 0 || rowmap[k] >= n || (k && rowmap[k] <= rowmap[k - 1]))
      return fail(MX_ERR_ARG, "rowmap must be increasing row indices");
  std::vector<SampRow> sr;
  int ktop = 0;
  if (samp && n_out)
    if (int rc = fill_samp_rows(e, n_out, samp, sr, &ktop)) return rc;
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  const size_t xb = (size_t)e->n_embd * (e->handoff_bf16 ? 2 : 4);  // hand-off bytes per row
  const int chunk = e->gemm_ok() ? PREFILL_ROWS : MAX_ROWS;
  int k0 = 0;  // first rowmap entry not yet produced
  for (int i = 0; i < n;) {
    int end = std::min(n, i + chunk), k1 = k0;
    while (k1 < n_out && rowmap[k1] < end && k1 - k0 < MAX_ROWS) k1++;
    // cut after the 64th prompt's last row, rounded up to its 16-row block (the prompts' padding) but
    // never past the next picked row: unpadded prompts may end inside that block, and a row the cut
    // skipped would reach the next chunk's row map as a negative index
    if (k1 - k0 == MAX_ROWS && k1 < n_out && rowmap[k1] < end)
      end = std::min({n, (rowmap[k1 - 1] + 16) / 16 * 16, rowmap[k1]});
    const int m = end - i, no = k1 - k0;
    for (int r = i; r < end; r++) {
      if (slots[r] < 0 || slots[r] >= e->n_seq_max) return fail(MX_ERR_ARG, "slot out of range");
      if (pos[r] < 0 || pos[r] >= e->n_ctx) return fail(MX_ERR_CTX, "position outside n_ctx");
      if (!x_in && (ids[r] < 0 || ids[r] >= e->n_vocab)) return fail(MX_ERR_ARG, "token id out of range");
    }
    if (!x_in) HIPC(hipMemcpyAsync(e->d_ids, ids + i, m * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(e->d_pos, pos + i, m * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(e->d_slot, slots + i, m * 4, hipMemcpyHostToDevice, s));
    std::vector<int32_t> rm(no);
    for (int k = 0; k < no; k++) rm[k] = rowmap[k0 + k] - i;
    if (no) HIPC(hipMemcpyAsync(e->d_rowmap, rm.data(), no * 4, hipMemcpyHostToDevice, s));
    if (no && ktop > 0) HIPC(hipMemcpyAsync(e->d_samp, sr.data() + k0, no * sizeof(SampRow), hipMemcpyHostToDevice, s));
    {
      std::lock_guard<std::mutex> lk2(e->mu);
      for (int r = i; r < end; r++) e->slot_tokens[slots[r]].clear();
    }
    e->rows_distinct = false;
    e->rows_blocked = blocked_rows(slots + i, pos + i, x_in ? nullptr : ids + i, m);
    e->prefill_gemm = true;
    e->pick_samp = ktop > 0 ? e->d_samp : nullptr;
    e->pick_k = ktop;
    const char* xi = (const char*)x_in;
    char* xo = (char*)x_out;
    const int frc = e->enqueue_forward({.M = m, .ids = e->d_ids, .pos = e->d_pos, .slot = e->d_slot,
                                        .x_in = xi ? xi + i * xb : nullptr, .x_out = xo ? xo + i * xb : nullptr,
                                        .head = no > 0, .rowmap = no ? e->d_rowmap : nullptr, .n_out = no},
                                       s);
    e->rows_blocked = false;
    e->prefill_gemm = false;
    if (!frc && no) e->pick(no, PickOut{}, s);  // logits rows [no][V]
    e->pick_samp = nullptr;
    e->pick_k = 0;
    if (frc) return frc;
    if (no) HIPC(hipMemcpyAsync(tok_out + k0, e->d_tok, no * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    k0 = k1;
    i = end;
  }
  return 0;
}

int mx_engine_stats(mx_engine* e, mx_stats* out) {
  if (!e || !out) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  out->prompt_tokens = e->stat_prompt_tokens;
  out->reused_prompt_tokens = e->stat_reused_tokens;
  out->generated_tokens = e->stat_generated_tokens;
  return 0;
}

int mx_engine_set_prefix_sharing(mx_engine* e, int on) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "prefix sharing needs a whole-model engine");
  std::lock_guard<std::mutex> lk(e->mu);
  e->prefix_sharing = on != 0;
  return 0;
}

int mx_prefix_sharing_stats(mx_engine* e, mx_sharing_stats* out) {
  if (!e || !out) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  out->shared_prompt_tokens = e->stat_shared_tokens;
  out->copies = e->stat_copies;
  out->copied_bytes = e->stat_copied_bytes;
  out->follower_requests = e->stat_followers;
  return 0;
}

int mx_engine_set_host_cache(mx_engine* e, uint64_t capacity_bytes) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  if (!e->has_embed || !e->has_head) return fail(MX_ERR_STATE, "the host cache needs a whole-model engine");
  std::unique_lock<std::mutex> lk(e->mu);
  e->host_cap_req = capacity_bytes;
  if (!e->worker_started) return 0;  // nothing is stored yet: the scheduler takes it up before its first admission
  // the scheduler thread owns the store: it evicts down to the new capacity now, and this call returns after that
  e->cv.notify_all();
  e->cv_done.wait(lk, [&] { return e->stop || e->host_cap == e->host_cap_req; });
  if (capacity_bytes && e->host_failed) return fail(MX_ERR_HIP, "the host cache's device staging could not be allocated");
  return 0;
}

int mx_host_cache_stats(mx_engine* e, mx_host_cache_counts* out) {
  if (!e || !out) return fail(MX_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  out->entries = e->host_entries.size();
  out->bytes = e->host_bytes;
  out->capacity_bytes = e->host_cap_req;
  out->spills = e->stat_host_spills;
  out->spilled_bytes = e->stat_host_spilled_bytes;
  out->restores = e->stat_host_restores;
  out->restored_prompt_tokens = e->stat_host_restored_tokens;
  out->restored_bytes = e->stat_host_restored_bytes;
  out->evictions = e->stat_host_evictions;
  out->skipped = e->stat_host_skipped;
  return 0;
}

int mx_device_count(int32_t* n) {
  if (!n) return fail(MX_ERR_ARG, "null argument");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return 0;
}

int mx_sync(mx_engine* e) {
  if (!e) return fail(MX_ERR_ARG, "null engine");
  hipSetDevice(e->device);
  HIPC(hipDeviceSynchronize());
  return 0;
}

int mx_profile_kernel(mx_engine* e, int kind, int M, int iters, double* us, double* bytes) {
  if (!e || M < 1 || M > MAX_ROWS || iters < 1) return fail(MX_ERR_ARG, "bad arguments");
  std::lock_guard<std::mutex> lk(e->gpu_mu);
  hipSetDevice(e->device);
  hipStream_t s = e->stream;
  const int h = e->n_embd, kv = e->n_embd_kv, ff = e->n_ff;
  const int prof_pos = std::min(e->n_ctx - 1, std::max(0, getenv("MX_PROF_POS") ? atoi(getenv("MX_PROF_POS")) : 0));
  const bool prof_fin = getenv("MX_PROF_FIN") != nullptr;  // kind 7: the FIN form (slabs finished in the kernel)
  const bool prof_warm = getenv("MX_PROF_WARM") != nullptr;  // diagnosis: every launch on layer 0 (Infinity-Cache warm)
  std::vector<int32_t> zero(M, prof_pos), slots(M);
  for (int i = 0; i < M; i++) slots[i] = i % e->n_seq_max;
  HIPC(hipMemcpyAsync(e->d_pos, zero.data(), M * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(e->d_slot, slots.data(), M * 4, hipMemcpyHostToDevice, s));
  hipEvent_t t0, t1;
  HIPC(hipEventCreate(&t0));
  HIPC(hipEventCreate(&t1));
  const int nl = (int)e->layers.size();
  size_t per = 0;
  int launches = 0;
  const bool wide = M > 16 && e->use_wide && e->wide_shapes();  // the bf16 forward's own choice (enqueue_forward)
  auto one = [&](int li) -> int {
    const Layer& L = e->layers[li];
    MMArgs a{};
    a.M = M;
    a.qkv_bias = L.qkv_bias;  // read by the EPI_QKV epilogues alone
    if (e->wq8 && kind <= 4) {  // Q8_0 weights: the activations are Q8_0 rows in xq8/xqd
      a.xq = e->xq8; a.xd = e->xqd; a.wq4 = e->wq4;
      // <= 4 rows: the form the decode runs -- the GEMV quantises its operand on load (gate/up and q|k|v
      // with the RMS_NORM from the ssq partials)
      const bool pql = e->q8_on_load(M) && getenv("MX_PROF_PREQUANT") == nullptr;
      auto ql_operand = [&](const float* src, int K, const float* norm_w) {
        if (!pql) return;
        a.xq = nullptr; a.xd = nullptr; a.xf = src; a.norm_w = norm_w; a.eps = e->eps;
        a.ssq = norm_w ? e->ssq : nullptr; a.np = K / 16;
      };
      auto qb = e->wq4 ? q4_matrix_bytes : q8_matrix_bytes;
      switch (kind) {
        case 0:
          a.W = L.qkv; a.N = h + 2 * kv; a.K = h; a.out = e->q; a.ldo = h; a.n_q = h; a.n_kv = kv;
          a.head_dim = e->head_dim; a.pos = e->d_pos; a.slot = e->d_slot; a.rope_cs = e->rope_cs;
          a.kc = e->kcache + e->layer_kv_stride * li; a.vc = e->vcache + e->layer_kv_stride * li;
          a.n_ctx = e->n_ctx; a.ctx_stride = e->ctx_stride; a.n_head_kv = e->n_head_kv; a.slot_stride = e->slot_stride;
          per = qb(h + 2 * kv, h);
          ql_operand(e->x, h, L.attn_norm);
          return launch_mq8(EPI_QKV, a, s);
        case 1: case 3:
          a.W = kind == 1 ? L.o : L.down; a.N = h; a.K = kind == 1 ? h : ff; a.out = e->x; a.ldo = h;
          per = qb(h, a.K);
          ql_operand(kind == 1 ? e->attn_f : e->act_f, a.K, nullptr);
          return launch_mq8(EPI_RESID, a, s);
        case 2:
          a.W = L.gu; a.N = 2 * ff; a.K = h; a.actf = e->act_f; a.lda = ff;
          per = qb(2 * ff, h);
          ql_operand(e->x, h, L.ffn_norm);
          return launch_mq8(EPI_SWIGLU, a, s);
        case 4:
          if (!e->has_head || e->out_kq_head) return -1;
          a.wq4 = e->out_q4;
          a.W = e->output; a.N = e->n_vocab; a.K = h; a.out = e->logits; a.ldo = e->n_vocab;
          per = e->out_q4 ? q4_matrix_bytes(e->n_vocab, h) : q8_matrix_bytes(e->n_vocab, h);
          return launch_mq8(EPI_F32, a, s);
      }
    }
    if (e->wkq && kind <= 4) {  // K-quant weights: the activations are Q8_K rows in xq8/xqd/xkb
      a.xq = e->xq8; a.xd = e->xqd; a.xb = e->xkb;
      const bool pql = e->kq_on_load(M) && getenv("MX_PROF_PREQUANT") == nullptr;  // as the decode runs it
      auto ql_operand = [&](const float* src, int K, const float* norm_w) {
        if (!pql) return;
        a.xq = nullptr; a.xd = nullptr; a.xb = nullptr; a.xf = src; a.norm_w = norm_w; a.eps = e->eps;
        a.ssq = norm_w ? e->ssq : nullptr; a.np = K / 16;
      };
      switch (kind) {
        case 0:
          a.W = L.qkv; a.N = h + 2 * kv; a.K = h; a.out = e->q; a.ldo = h; a.n_q = h; a.n_kv = kv;
          a.head_dim = e->head_dim; a.pos = e->d_pos; a.slot = e->d_slot; a.rope_cs = e->rope_cs;
          a.kc = e->kcache + e->layer_kv_stride * li; a.vc = e->vcache + e->layer_kv_stride * li;
          a.n_ctx = e->n_ctx; a.ctx_stride = e->ctx_stride; a.n_head_kv = e->n_head_kv; a.slot_stride = e->slot_stride;
          L.kq_qkv.set(a);
          per = L.kq_qkv.bytes;
          ql_operand(e->x, h, L.attn_norm);
          return launch_mkq(EPI_QKV, a, s);
        case 1: case 3:
          a.W = kind == 1 ? L.o : L.down; a.N = h; a.K = kind == 1 ? h : ff; a.out = e->x; a.ldo = h;
          (kind == 1 ? L.kq_o : L.kq_down).set(a);
          per = (kind == 1 ? L.kq_o : L.kq_down).bytes;
          ql_operand(kind == 1 ? e->attn_f : e->act_f, a.K, nullptr);
          return launch_mkq(EPI_RESID, a, s);
        case 2:
          a.W = L.gu; a.N = 2 * ff; a.K = h; a.actf = e->act_f; a.lda = ff;
          L.kq_gu.set(a);
          per = L.kq_gu.bytes;
          ql_operand(e->x, h, L.ffn_norm);
          return launch_mkq(EPI_SWIGLU, a, s);
        case 4:
          if (!e->has_head) return -1;
          a.W = e->output; a.N = e->n_vocab; a.K = h; a.out = e->logits; a.ldo = e->n_vocab;
          e->kq_out.set(a);
          per = e->kq_out.bytes;
          return launch_mkq(EPI_F32, a, s);
      }
    }
    if ((e->wq8 || e->wkq) && (kind >= 5 && kind <= 6)) return -1;
    switch (kind) {
      case 0:
        a.W = L.qkv; a.N = h + 2 * kv; a.K = h; a.X = e->xn; a.ldx = h; a.out = e->q; a.ldo = h; a.n_q = h;
        a.n_kv = kv; a.head_dim = e->head_dim; a.pos = e->d_pos; a.slot = e->d_slot; a.rope_cs = e->rope_cs;
        a.kc = e->kcache + e->layer_kv_stride * li; a.vc = e->vcache + e->layer_kv_stride * li; a.n_ctx = e->n_ctx;
        a.ctx_stride = e->ctx_stride;
        a.n_head_kv = e->n_head_kv; a.slot_stride = e->slot_stride;
        per = (size_t)(h + 2 * kv) * h * 2;
        return wide ?(launch_mm_wide(EPI_QKV, a, e->slabs, e->slab_stride, s) < 0) : launch_mm(EPI_QKV, a, s);
      case 1:
        a.W = L.o; a.N = h; a.K = h; a.X = e->attn_out; a.ldx = h; a.out = e->x; a.ldo = h;
        per = (size_t)h * h * 2;
        return wide ?(launch_mm_wide(EPI_RESID, a, e->slabs, e->slab_stride, s) < 0) : launch_mm(EPI_RESID, a, s);
      case 2:
        a.W = L.gu; a.N = 2 * ff; a.K = h; a.X = e->xn; a.ldx = h; a.act = e->act; a.lda = ff;
        per = (size_t)2 * ff * h * 2;
        return wide ?(launch_mm_wide(EPI_SWIGLU, a, e->slabs, e->slab_stride, s) < 0) : launch_mm(EPI_SWIGLU, a, s);
      case 3:
        a.W = L.down; a.N = h; a.K = ff; a.X = e->act; a.ldx = ff; a.out = e->x; a.ldo = h;
        per = (size_t)h * ff * 2;
        return wide ?(launch_mm_wide(EPI_RESID, a, e->slabs, e->slab_stride, s) < 0) : launch_mm(EPI_RESID, a, s);
      case 4:
        if (!e->has_head) return -1;
        a.W = e->output; a.N = e->n_vocab; a.K = h; a.X = e->xn; a.ldx = h; a.out = e->logits; a.ldo = e->n_vocab;
        per = (size_t)e->n_vocab * h * 2;
        return wide ?(launch_mm_wide(EPI_F32, a, e->slabs, e->slab_stride, s) < 0) : launch_mm(EPI_F32, a, s);
      case 5:  // qkv with the attention RMSNorm applied on load (M <= 16)
        a.W = L.qkv; a.N = h + 2 * kv; a.K = h; a.X = nullptr; a.xf = e->x; a.norm_w = L.attn_norm; a.eps = e->eps;
        a.ssq = e->ssq; a.np = h / 16;
        a.out = e->q; a.ldo = h; a.n_q = h; a.n_kv = kv; a.head_dim = e->head_dim; a.pos = e->d_pos;
        a.slot = e->d_slot; a.rope_cs = e->rope_cs; a.kc = e->kcache + e->layer_kv_stride * li;
        a.vc = e->vcache + e->layer_kv_stride * li; a.n_ctx = e->n_ctx; a.ctx_stride = e->ctx_stride;
        a.n_head_kv = e->n_head_kv; a.slot_stride = e->slot_stride;
        per = (size_t)(h + 2 * kv) * h * 2;
        return launch_mm(EPI_QKV, a, s);
      case 6:  // gate/up with the ffn RMSNorm applied on load (M <= 16)
        a.W = L.gu; a.N = 2 * ff; a.K = h; a.X = nullptr; a.xf = e->x; a.norm_w = L.ffn_norm; a.eps = e->eps;
        a.ssq = e->ssq; a.np = h / 16;
        a.act = e->act; a.lda = ff;
        per = (size_t)2 * ff * h * 2;
        return (e->use_pers && mm_pers_supported(EPI_SWIGLU, M, a.N, a.K)) ? launch_mm_pers(EPI_SWIGLU, a, s)
                                                                            : launch_mm(EPI_SWIGLU, a, s);
      case 8: case 9: case 10: {  // RMS_NORM of M rows folding 4 (8) / 8 (9) / 0 (10) split-K slabs
        const int ns = kind == 8 ? 4 : kind == 9 ? 8 : 0;
        per = (size_t)M * h * 4 * (2 + ns) + (size_t)M * h * 2;
        launch_resid_norm(e->xn, h, e->x, e->slabs, ns, e->slab_stride, L.ffn_norm, M, h, e->eps, s);
        return 0;
      }
      case 7: {  // attention at the positions set below (ctx = pos + 1)
        AttnArgs at{};
        at.q = e->q; at.kc = e->kcache + e->layer_kv_stride * li; at.vc = e->vcache + e->layer_kv_stride * li;
        at.pos = e->d_pos; at.slot = e->d_slot; at.out = e->attn_out; at.ldo = h; at.M = M; at.n_head = e->n_head;
        at.n_head_kv = e->n_head_kv; at.head_dim = e->head_dim; at.n_ctx = e->n_ctx; at.ctx_stride = e->ctx_stride;
        at.slot_stride = e->slot_stride; at.scale = 1.0f / sqrtf((float)e->head_dim);
        at.qkv_bias = L.qkv_bias;
        if (prof_fin) {  // the 32-row decode's form: q/k/v still as 4 split-K slabs, finished here
          at.slabs = e->slabs; at.nslab = 4; at.slab_stride = e->slab_stride; at.rope_cs = e->rope_cs;
          at.kc_w = e->kcache + e->layer_kv_stride * li; at.vc_w = e->vcache + e->layer_kv_stride * li;
        }
        per = (size_t)M * (prof_pos + 1) * kv * 2 * 2;
        launch_attention(at, s);
        return 0;
      }
    }
    return -1;
  };
  // warm-up pass, then timed passes; each pass walks every local layer so no
  // launch re-reads weights that the previous one left in the caches
  for (int li = 0; li < nl; li++)
    if (one(li)) return fail(MX_ERR_ARG, "bad kernel kind");
  HIPC(hipEventRecord(t0, s));
  for (int it = 0; it < iters; it++) {
    if (kind == 4) {
      if (one(0)) return fail(MX_ERR_ARG, "bad kernel kind");
      launches++;
    } else {
      for (int li = 0; li < nl; li++) {
        one(prof_warm ? 0 : li);
        launches++;
      }
    }
  }
  HIPC(hipEventRecord(t1, s));
  HIPC(hipEventSynchronize(t1));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, t0, t1));
  hipEventDestroy(t0);
  hipEventDestroy(t1);
  if (kind == 7 && getenv("MX_ATTN_TRACE")) {  // diagnosis: phase stamps of one launch (layer 0)
    const size_t n = (size_t)M * e->n_head_kv * 8 * 8;
    unsigned long long* tr = nullptr;
    HIPC(hipMalloc((void**)&tr, n * 8));
    HIPC(hipMemsetAsync(tr, 0, n * 8, s));
    AttnArgs at{};
    at.q = e->q; at.kc = e->kcache; at.vc = e->vcache; at.pos = e->d_pos; at.slot = e->d_slot; at.out = e->attn_out;
    at.ldo = h; at.M = M; at.n_head = e->n_head; at.n_head_kv = e->n_head_kv; at.head_dim = e->head_dim;
    at.n_ctx = e->n_ctx; at.ctx_stride = e->ctx_stride; at.slot_stride = e->slot_stride;
    at.scale = 1.0f / sqrtf((float)e->head_dim); at.trace = tr;
    at.qkv_bias = e->layers[0].qkv_bias;
    if (prof_fin) {
      at.slabs = e->slabs; at.nslab = 4; at.slab_stride = e->slab_stride; at.rope_cs = e->rope_cs;
      at.kc_w = e->kcache; at.vc_w = e->vcache;
    }
    launch_attention(at, s);
    HIPC(hipStreamSynchronize(s));
    std::vector<unsigned long long> t(n);
    HIPC(hipMemcpy(t.data(), tr, n * 8, hipMemcpyDeviceToHost));
    hipFree(tr);
    unsigned long long t0m = ~0ull, tend = 0;
    double ph[5] = {0, 0, 0, 0, 0};
    int cnt = 0;
    double chunks = 0;
    for (size_t g = 0; g < n / 8; g++) {
      const unsigned long long* p = &t[g * 8];
      if (!p[0]) continue;
      t0m = std::min(t0m, p[0]);
      tend = std::max(tend, p[5]);
      for (int k = 0; k < 5; k++)
        if (p[k + 1] >= p[k] && p[k]) ph[k] += (double)(p[k + 1] - p[k]) / 100.0;
      chunks += (double)p[7];
      cnt++;
    }
    fprintf(stderr, "attn trace M=%d pos=%d: waves %d, span %.2f us (first start -> last end); mean per wave: "
                    "q %.2f | first K/V %.2f | chunks %.2f (%.2f chunks) | merge wait %.2f | store %.2f us\n",
            M, prof_pos, cnt, (tend - t0m) / 100.0, ph[0] / cnt, ph[1] / cnt, ph[2] / cnt, chunks / cnt, ph[3] / cnt,
            ph[4] / cnt);
  }
  if (us) *us = ms * 1000.0 / launches;
  if (bytes) *bytes = (double)per;
  return 0;
}

}  // extern "C"
