// engine_shared.h -- what the engine (engine.cpp) and the stand-alone kernel probes (probes.cpp) both use.
// Everything here is defined once, in engine.cpp; struct mx_engine stays private to that file.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mx_engine.h"
#include "kernels.h"

namespace mx {

// records msg as the calling thread's error (what mx_last_error() returns, for the whole library) and returns code
int fail(int code, const std::string& msg);

#define HIPC(expr)                                                                                  \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return fail(MX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + __FILE__ + \
                                  ":" + std::to_string(__LINE__));                                  \
  } while (0)

// ---- embeddings.  The tail of one forward chunk: its rows of the final residual stream x
// through the f32 output norm, the pooling and the L2 normalisation (kernels.h launch_embd_*).
// One EmbdSeg per sequence with rows in the chunk: rows [row0, row0 + rows) of x are its positions
// [done, done + rows) of T; seq is its accumulator row, dst0 its first output row -- of ybuf for MX_POOL_NONE
// (one output row per row), of pooled otherwise.  MEAN norms every row into ybuf (compacted from row 0), then
// one thread per 4 columns adds a segment's rows in order to the sequence's running sum, carried in acc[seq]
// between chunks; CLS / LAST norm the one row that counts straight into pooled.  L2 runs in place on the
// vectors this chunk completed.  tab: host copy of the index tables, alive until the stream is synchronised.
struct EmbdSeg {
  int row0, rows, seq, done, T, dst0;
};
// ints the tables of a chunk of `rows` rows in `segs` sequences can take: src, dst and L2 rows (<= rows each,
// MEAN: L2 <= segs) plus EMBD_SEG per segment
constexpr size_t embd_tab_ints(size_t rows, size_t segs) { return 3 * rows + (EMBD_SEG + 1) * segs; }
int embd_tail(const float* x, const float* w, float eps, int n, const std::vector<EmbdSeg>& segs, int pooling,
              bool normalize, float* ybuf, float* acc, float* pooled, int* d_tab, size_t tab_ints,
              std::vector<int32_t>& tab, hipStream_t s);

// ---- sampling
bool has_penalties(const mx_sampling& sp);
// the per-row pick kernel can serve these settings: top_k 1..64 and a penalty window of 0..64 tokens (what the
// stage rows of mx_batch_reset / mx_stage_rows_pick still require)
bool device_sampleable(const mx_sampling& sp);
// which sampler picks a row of these settings over a vocabulary of V (MX_PICK_*; the rules of mx_sample_plan, which
// the scheduler, prefill_batch and mx_sample_probe all dispatch on), x the row's validated extended settings;
// *k_eff: the candidates the path takes (CHAIN: 1..64, the round's top-k; WIDE: 65..V; 1 otherwise)
int sample_path(const mx_sampling& sp, const SampExt& x, int V, int* k_eff);
// validates the extended settings against a vocabulary of V and restates them as a SampExt (the bias table
// copied); *has: some setting is off its default, so the request / row takes the extended chain
int check_sampling_ext(const mx_sampling_ext* s, int V, SampExt* o, bool* has);
// the whole chain on the host for one row x (rewritten in place): what sample_host and mx_sample_probe run
int32_t chain_host(const mx_sampling& sp, const SampExt* ext, const int32_t* win, int n_win, int V, float* x,
                   double u01, float* mu);

// [n][1 + 2k] entries (launch_logprobs) -> the three host arrays
void split_entries(const std::vector<float>& ent, int n, int k, float* tgt_lp, float* top_lp, int32_t* top_idx);

// rows form blocks of 16 (from row 0) of one slot each, positions consecutive within a block except
// that a block may end in copies of its last real row (same position and token: the prompt padding
// near n_ctx) -- what attn_prefill_kernel needs (every key position a block reads is written by it)
bool blocked_rows(const int32_t* slots, const int32_t* pos, const int32_t* ids, int m);

}  // namespace mx
