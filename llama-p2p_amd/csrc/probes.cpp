// probes.cpp -- the stand-alone kernel probes of the C API (include/mx_engine.h: mx_*_probe, mx_*_plan).
//
// A probe takes an `int device` and never an mx_engine: it checks every index a kernel would form from its
// arguments, allocates its own buffers, calls the launchers of kernels.h in the engine's order and copies the
// results back, so that the tests can pin one kernel at a time.  No device code lives here.  What the probes
// share with the engine (the error string, the sampler's host chain, the embedding tail) is engine_shared.h.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "engine_shared.h"

using namespace mx;

namespace {
struct DevBufs {  // device allocations of a probe call, freed on every return path
  std::vector<void*> v;
  ~DevBufs() { for (void* p : v) hipFree(p); }
  bool alloc(void* pp, size_t bytes) {  // pp: address of the (typed) device pointer to set
    void* q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return false;
    v.push_back(q);
    *static_cast<void**>(pp) = q;
    return true;
  }
  // alloc, then every byte 0xFF: an element no kernel wrote reads back as NaN in every f32 / f16 / bf16 lane
  bool alloc_ff(void* pp, size_t bytes) {
    return alloc(pp, bytes) && hipMemset(*static_cast<void**>(pp), 0xFF, bytes) == hipSuccess;
  }
};
constexpr int PROBE_GUARD_ROWS = 64;  // rows of 0xFF after every probe output, returned to the caller
constexpr int XQ_ON_LOAD_ROWS = 4;    // f32 source rows of a quantise-on-load GEMV (its QM = 4 image)

// The tiled K / V caches of a probe, [n_layer][n_slots][n_head_kv] regions of ctx_stride positions each, as the
// engine lays them out.  set() refuses, in the probe's name, caches larger than a probe may allocate.
struct KvGeom {
  int ctx_stride = 0;
  size_t slot_stride = 0, layer_kv_stride = 0, cache_elems = 0;
  int set(const char* who, int n_head_kv, int head_dim, int n_ctx, int n_slots, int n_layer = 1) {
    ctx_stride = (n_ctx + KV_POS_ALIGN - 1) / KV_POS_ALIGN * KV_POS_ALIGN;
    slot_stride = (size_t)n_head_kv * ctx_stride * head_dim;
    layer_kv_stride = slot_stride * n_slots;
    cache_elems = layer_kv_stride * n_layer;
    if (cache_elems > ((size_t)1 << 29)) return fail(MX_ERR_ARG, std::string(who) + ": caches above 1 GiB each");
    return 0;
  }
};

// The QKV operand of a matmul probe (P: its argument struct): the caller's caches, pos / slot rows and RoPE table.
// check() goes where the probe validates, upload() where it fills its MMArgs, download() after the last launch.
struct QkvOperand {
  KvGeom g;
  int n_q = 0, n_kv = 0;
  _Float16 *d_k = nullptr, *d_v = nullptr;
  template <class P>
  int check(const std::string& who, const P& p, int M, int N) {
    if (!p.pos || !p.slot || !p.rope_cs || !p.kcache || !p.vcache)
      return fail(MX_ERR_ARG, who + ": QKV takes pos, slot, rope_cs and both caches");
    if ((p.head_dim != 64 && p.head_dim != 128) || p.n_head < 1 || p.n_head_kv < 1 || p.n_head > 1024 ||
        p.n_head_kv > 1024 || (long long)(p.n_head + 2 * p.n_head_kv) * p.head_dim != N)
      return fail(MX_ERR_ARG, who + ": head_dim 64 or 128, N = (n_head + 2 n_head_kv) * head_dim");
    if (p.n_ctx < 1 || p.n_ctx > (1 << 20) || p.n_slots < 1 || p.n_slots > 4096)
      return fail(MX_ERR_ARG, who + ": 1 <= n_ctx <= 2^20, 1 <= n_slots <= 4096");
    n_q = p.n_head * p.head_dim;
    n_kv = p.n_head_kv * p.head_dim;
    if (int rc = g.set(who.c_str(), p.n_head_kv, p.head_dim, p.n_ctx, p.n_slots)) return rc;
    for (int i = 0; i < M; i++) {
      if (p.slot[i] < 0 || p.slot[i] >= p.n_slots) return fail(MX_ERR_ARG, who + ": slot out of range");
      if (p.pos[i] < 0 || p.pos[i] > p.n_ctx) return fail(MX_ERR_ARG, who + ": position outside [0, n_ctx]");
    }
    return 0;
  }
  template <class P>
  int upload(const std::string& who, const P& p, int M, DevBufs& dev, MMArgs& a) {
    int *d_pos = nullptr, *d_slot = nullptr;
    float* d_cs = nullptr;
    const size_t cs_bytes = (size_t)p.n_ctx * p.head_dim * 4;
    if (!dev.alloc(&d_k, g.cache_elems * 2) || !dev.alloc(&d_v, g.cache_elems * 2) || !dev.alloc(&d_pos, (size_t)M * 4) ||
        !dev.alloc(&d_slot, (size_t)M * 4) || !dev.alloc(&d_cs, cs_bytes))
      return fail(MX_ERR_HIP, who + ": device allocation");
    HIPC(hipMemcpy(d_k, p.kcache, g.cache_elems * 2, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_v, p.vcache, g.cache_elems * 2, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_pos, p.pos, (size_t)M * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_slot, p.slot, (size_t)M * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_cs, p.rope_cs, cs_bytes, hipMemcpyHostToDevice));
    a.n_q = n_q; a.n_kv = n_kv; a.head_dim = p.head_dim; a.pos = d_pos; a.slot = d_slot; a.rope_cs = d_cs;
    a.kc = d_k; a.vc = d_v; a.n_ctx = p.n_ctx; a.ctx_stride = g.ctx_stride; a.n_head_kv = p.n_head_kv;
    a.slot_stride = g.slot_stride;
    if (p.bias) {  // the q/k/v bias, [n_q + 2 n_kv] = [N]
      float* d_bias = nullptr;
      const size_t nb = ((size_t)n_q + 2 * (size_t)n_kv) * 4;
      if (!dev.alloc(&d_bias, nb)) return fail(MX_ERR_HIP, who + ": device allocation");
      HIPC(hipMemcpy(d_bias, p.bias, nb, hipMemcpyHostToDevice));
      a.qkv_bias = d_bias;
    }
    return 0;
  }
  template <class P>
  int download(const P& p) const {
    HIPC(hipMemcpy(p.kcache, d_k, g.cache_elems * 2, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(p.vcache, d_v, g.cache_elems * 2, hipMemcpyDeviceToHost));
    return 0;
  }
};

MkqEnv kq_probe_env(int flags) {
  MkqEnv env = mkq_env();
  if (flags >= 0) env.no_bd_tile = flags & 1, env.no_pers = (flags & 2) != 0, env.no_wide = (flags & 4) != 0;
  return env;
}
// the row segments of a K-quant probe matrix: types known, ends strictly increasing up to N / 16
bool kq_segments_ok(int kq_n, const int32_t* type, const int32_t* tile_end, int N) {
  if (kq_n < 1 || kq_n > 3 || N < TILE_N || N % TILE_N) return false;
  for (int i = 0; i < kq_n; i++)
    if (!kq_tile_bytes(type[i]) || tile_end[i] <= (i ? tile_end[i - 1] : 0)) return false;
  return (long long)tile_end[kq_n - 1] * TILE_N == N;
}

constexpr size_t GLUE_GUARD_FLAT = 4096;  // elements of 0xFF after every flat mx_glue_probe output
size_t glue_block_bytes(int type) {       // bytes of ggml_block_elems(type) values in the file
  switch (type) {
    case 0: return 128;
    case 1: return 64;
    case 2: return 18;
    case 8: return 34;
    case 12: return 144;
    case 13: return 176;
    case 14: return 210;
  }
  return 0;
}

// Best of the probe variants (loads in flight x grid x non-temporal): each is warmed twice, then
// `iters` launches are timed with HIP events on a private stream.  Every HIP call is checked and
// every object created is released on all paths.
int probe_hbm(int device, size_t bytes, int iters, bool read_only, double* gbs, char* desc, int desc_len) {
  const size_t n16 = bytes / 16 / 4096 * 4096;  // whole 4096-word chunks (the largest variant's unit)
  if (n16 == 0 || iters < 1 || !gbs) return fail(MX_ERR_ARG, "bad arguments");
  HIPC(hipSetDevice(device));
  uint4 *src = nullptr, *dst = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipError_t err = hipMalloc(&src, n16 * 16);
  if (err == hipSuccess) err = hipMalloc(&dst, read_only ? (size_t)4096 * 256 * 16 : n16 * 16);  // read: sink only
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipEventCreate(&t0);
  if (err == hipSuccess) err = hipEventCreate(&t1);
  if (err == hipSuccess) err = hipMemsetAsync(src, 1, n16 * 16, s);
  double best = 0.0;
  char d[160] = "", bestd[160] = "";
  for (int v = 0; err == hipSuccess && v < mx::probe_variants(); v++) {
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
      mx::launch_probe(v, read_only, src, dst, n16, s, d, sizeof d);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(t0, s);
    for (int i = 0; i < iters && err == hipSuccess; i++) {
      mx::launch_probe(v, read_only, src, dst, n16, s, nullptr, 0);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(t1, s);
    if (err == hipSuccess) err = hipEventSynchronize(t1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
    if (err == hipSuccess && ms > 0.f) {
      const double r = (read_only ? 1.0 : 2.0) * (double)n16 * 16 * iters / (ms * 1e-3) / 1e9;
      if (r > best) {
        best = r;
        memcpy(bestd, d, sizeof d);
      }
    }
  }
  if (t0) hipEventDestroy(t0);
  if (t1) hipEventDestroy(t1);
  if (s) hipStreamDestroy(s);
  if (src) hipFree(src);
  if (dst) hipFree(dst);
  if (err != hipSuccess) return fail(MX_ERR_HIP, std::string("HBM probe: ") + hipGetErrorString(err));
  if (best <= 0.0) return fail(MX_ERR_HIP, "HBM probe: no timing");
  *gbs = best;
  if (desc && desc_len > 0) snprintf(desc, desc_len, "%s", bestd);
  return MX_OK;
}
}  // namespace

extern "C" {

int mx_logprob_probe(int device, const float* logits_host, int n, int V, int ldl, const int32_t* targets, int k,
                     float* tgt_lp, float* top_lp, int32_t* top_idx) {
  if (!logits_host || !targets || !tgt_lp || n < 1 || n > MAX_ROWS || V < 1 || ldl < V || k < 0 || k > TOPK_MAX ||
      (k && (!top_lp || !top_idx)))
    return fail(MX_ERR_ARG, "mx_logprob_probe: 1 <= n <= 64 rows, ldl >= V >= 1, 0 <= k <= 64");
  for (int i = 0; i < n; i++)
    if (targets[i] < 0 || targets[i] >= V) return fail(MX_ERR_ARG, "target id out of range");
  if (device >= 0) HIPC(hipSetDevice(device));
  k = std::min(k, V);
  const int kk = std::max(k, 1);
  const size_t est = 1 + 2 * (size_t)k;
  float *d_lg = nullptr, *d_wsv = nullptr, *d_part = nullptr, *d_ms = nullptr, *d_top = nullptr, *d_out = nullptr;
  int *d_wsi = nullptr, *d_idx = nullptr, *d_tgt = nullptr;
  DevBufs dev;
  if (!dev.alloc(&d_lg, (size_t)n * ldl * 4) || !dev.alloc(&d_wsv, (size_t)n * 64 * kk * 4) ||
      !dev.alloc(&d_wsi, (size_t)n * 64 * kk * 4) || !dev.alloc(&d_part, (size_t)n * 64 * 2 * 4) ||
      !dev.alloc(&d_ms, (size_t)n * 2 * 4) || !dev.alloc(&d_top, (size_t)n * kk * 4) ||
      !dev.alloc(&d_idx, (size_t)n * kk * 4) || !dev.alloc(&d_tgt, (size_t)n * 4) || !dev.alloc(&d_out, (size_t)n * est * 4))
    return fail(MX_ERR_HIP, "mx_logprob_probe: device allocation");
  HIPC(hipMemcpy(d_lg, logits_host, (size_t)n * ldl * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_tgt, targets, (size_t)n * 4, hipMemcpyHostToDevice));
  if (launch_logprobs(d_lg, ldl, n, V, k, d_tgt, d_wsv, d_wsi, d_part, d_ms, d_top, d_idx, d_out, nullptr))
    return fail(MX_ERR_ARG, "log-prob launch shape (V too large for the top-k slices)");
  HIPC(hipDeviceSynchronize());
  std::vector<float> ent((size_t)n * est);
  HIPC(hipMemcpy(ent.data(), d_out, ent.size() * 4, hipMemcpyDeviceToHost));
  split_entries(ent, n, k, tgt_lp, top_lp, top_idx);
  return 0;
}

int mx_sample_probe(int device, const float* logits_host, int n, int V, int ldl, const mx_sampling_ext* samp,
                    const uint64_t* seeds, const int32_t* n_drawn, const int32_t* win, const int32_t* n_win,
                    const float* mu_in, int32_t* tok_out, float* mu_out, float* logits_out) {
  if (tok_out && n >= 1 && n <= 4096) memset(tok_out, 0xFF, (size_t)n * 4);
  if (mu_out && n >= 1 && n <= 4096) memset(mu_out, 0xFF, (size_t)n * 4);
  if (!logits_host || !samp || !seeds || !n_drawn || !win || !n_win || !mu_in || !tok_out || !mu_out || n < 1 ||
      n > MAX_ROWS || V < 1 || V > 262144 || ldl < V || device < -1)
    return fail(MX_ERR_ARG, "mx_sample_probe: 1 <= n <= 64 rows, 1 <= V <= 262144, V <= ldl, device >= -1");
  std::vector<SampExt> sx(n);
  std::vector<SampRow> sr(n, SampRow{});
  int ktop = 1;
  bool any_miro = false, any_wide = false;
  for (int i = 0; i < n; i++) {
    bool has = false;
    if (int rc = check_sampling_ext(&samp[i], V, &sx[i], &has)) return rc;
    const mx_sampling& sp = samp[i].base;
    if (n_drawn[i] < 0 || n_win[i] < 0 || n_win[i] > SAMP_WIN) return fail(MX_ERR_ARG, "mx_sample_probe: n_drawn >= 0, n_win 0..64");
    for (int j = 0; j < n_win[i]; j++)
      if (win[i * SAMP_WIN + j] < 0 || win[i * SAMP_WIN + j] >= V) return fail(MX_ERR_ARG, "mx_sample_probe: window token outside the vocabulary");
    if (std::isnan(sp.temperature) || std::isnan(mu_in[i])) return fail(MX_ERR_ARG, "mx_sample_probe: NaN setting");
    if (device >= 0) {
      int k = 1;
      const int path = sample_path(sp, sx[i], V, &k);
      if (path == MX_PICK_HOST)
        return fail(MX_ERR_ARG, "mx_sample_probe: settings of the host sampler (repeat_last_n outside 0..64, or "
                                "tfs_z / typical_p over more than 64 candidates)");
      sx[i].wide_k = path == MX_PICK_WIDE ? k : 0;
      if (path != MX_PICK_CHAIN || sp.temperature <= 0.f) k = 1;
      any_wide |= sx[i].wide_k > 0;
      SampRow& o = sr[i];
      o.temp = sp.temperature, o.top_p = sp.top_p, o.min_p = sp.min_p;
      o.repeat = sp.repeat_penalty, o.freq = sp.frequency_penalty, o.presence = sp.presence_penalty;
      o.top_k = std::max(1, std::min(k, TOPK_MAX));
      o.last_n = has_penalties(sp) ? std::min(sp.repeat_last_n, SAMP_WIN) : 0;
      o.seed = seeds[i];
      o.draw0 = n_drawn[i];
      o.n_win = std::min(o.last_n, n_win[i]);
      for (int j = 0; j < o.n_win; j++) o.win[j] = win[i * SAMP_WIN + n_win[i] - o.n_win + j];
      ktop = std::max(ktop, std::min(o.top_k, V));
      any_miro |= sx[i].miro == 2;
    }
  }
  if (logits_out) memcpy(logits_out, logits_host, (size_t)n * ldl * 4);
  if (device < 0) {  // the host sampler: no GPU touched
    std::vector<float> x(V);
    for (int i = 0; i < n; i++) {
      memcpy(x.data(), logits_host + (size_t)i * ldl, (size_t)V * 4);
      float mu = mu_in[i];
      tok_out[i] = chain_host(samp[i].base, &sx[i], win + i * SAMP_WIN, n_win[i], V, x.data(),
                              samp_u01(seeds[i], (uint64_t)n_drawn[i]), &mu);
      mu_out[i] = mu;
      if (logits_out) memcpy(logits_out + (size_t)i * ldl, x.data(), (size_t)V * 4);
    }
    return 0;
  }
  HIPC(hipSetDevice(device));
  DevBufs dev;
  float *d_lg, *d_wsv, *d_tkv, *d_mu, *d_wf, *d_braw;
  int *d_wsi, *d_tki, *d_tok, *d_wi;
  double* d_wd;
  SampRow* d_sr;
  SampExt* d_sx;
  if (!dev.alloc(&d_lg, (size_t)n * ldl * 4) || !dev.alloc(&d_wsv, (size_t)n * 64 * TOPK_MAX * 4) ||
      !dev.alloc(&d_wsi, (size_t)n * 64 * TOPK_MAX * 4) || !dev.alloc(&d_tkv, (size_t)n * TOPK_MAX * 4) ||
      !dev.alloc(&d_tki, (size_t)n * TOPK_MAX * 4) || !dev.alloc_ff(&d_tok, (size_t)n * 4) ||
      !dev.alloc(&d_mu, (size_t)n * 4) || !dev.alloc(&d_wf, miro_ws_floats(n) * 4) ||
      !dev.alloc(&d_wd, miro_ws_doubles(n) * 8) || !dev.alloc(&d_wi, miro_ws_ints(n) * 4) ||
      !dev.alloc(&d_braw, (size_t)n * SAMP_BIAS_MAX * 4) || !dev.alloc(&d_sr, (size_t)n * sizeof(SampRow)) ||
      !dev.alloc(&d_sx, (size_t)n * sizeof(SampExt)))
    return fail(MX_ERR_HIP, "mx_sample_probe: device allocation");
  HIPC(hipMemcpy(d_lg, logits_host, (size_t)n * ldl * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_sr, sr.data(), (size_t)n * sizeof(SampRow), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_sx, sx.data(), (size_t)n * sizeof(SampExt), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_mu, mu_in, (size_t)n * 4, hipMemcpyHostToDevice));
  SampExtArgs xa;
  xa.ext = d_sx, xa.bias_raw = d_braw, xa.mu = d_mu, xa.ws_f = d_wf, xa.ws_d = d_wd, xa.ws_i = d_wi;
  xa.any_miro = any_miro, xa.any_wide = any_wide;
  if (launch_sample_chain(d_lg, ldl, n, V, d_sr, ktop, d_wsv, d_wsi, d_tkv, d_tki, d_tok, nullptr, nullptr, nullptr, 0,
                          nullptr, 0, nullptr, nullptr, nullptr, &xa))
    return fail(MX_ERR_ARG, "mx_sample_probe: launch shape (V too large for the top-k slices)");
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(tok_out, d_tok, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(mu_out, d_mu, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (logits_out) HIPC(hipMemcpy(logits_out, d_lg, (size_t)n * ldl * 4, hipMemcpyDeviceToHost));
  return 0;
}

int mx_attention_probe(int device, int mode, int n_head, int n_head_kv, int head_dim, int n_ctx, int n_slots, int M,
                       const int32_t* pos, const int32_t* slot, int out_f32, const float* q, const float* slabs,
                       int nslab, const float* rope_cs, void* kcache, void* vcache, void* out, const float* bias) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  if (mode < 0 || mode > 2 || !pos || !slot || !kcache || !vcache || !out)
    return fail(MX_ERR_ARG, "mx_attention_probe: mode 0..2, non-null pos / slot / caches / out");
  if ((head_dim != 64 && head_dim != 128) || n_head_kv < 1 || n_head < n_head_kv || n_head % n_head_kv != 0 ||
      n_head > 1024)
    return fail(MX_ERR_ARG, "mx_attention_probe: head_dim 64 or 128, n_head a multiple of n_head_kv");
  const int G = n_head / n_head_kv;
  if (G != 1 && G != 2 && (G < 4 || G > 8))
    return fail(MX_ERR_ARG, "mx_attention_probe: n_head / n_head_kv must be 1, 2 or 4..8");
  if (bias && mode != 1) return fail(MX_ERR_ARG, "mx_attention_probe: a bias goes with mode 1 (the slabs)");
  if (n_ctx < 1 || n_ctx > (1 << 20) || n_slots < 1 || n_slots > 4096)
    return fail(MX_ERR_ARG, "mx_attention_probe: 1 <= n_ctx <= 2^20, 1 <= n_slots <= 4096");
  if (M < 1 || M > PREFILL_ROWS) return fail(MX_ERR_ARG, "mx_attention_probe: 1 <= M <= PREFILL_ROWS rows");
  KvGeom g;
  if (int rc = g.set("mx_attention_probe", n_head_kv, head_dim, n_ctx, n_slots)) return rc;
  const size_t cache_elems = g.cache_elems;
  for (int i = 0; i < M; i++) {
    if (slot[i] < 0 || slot[i] >= n_slots) return fail(MX_ERR_ARG, "mx_attention_probe: slot out of range");
    if (pos[i] < 0 || pos[i] > n_ctx) return fail(MX_ERR_ARG, "mx_attention_probe: position outside [0, n_ctx]");
  }
  const size_t nq = (size_t)n_head * head_dim, N = nq + 2 * (size_t)n_head_kv * head_dim;
  if (mode == 1) {
    if (!slabs || !rope_cs || nslab < 1 || nslab > ATTN_FIN_MAXSLAB || M > MAX_ROWS)
      return fail(MX_ERR_ARG, "mx_attention_probe: mode 1 takes slabs, rope_cs, 1 <= nslab <= 8, M <= 64");
    std::vector<int32_t> sorted(slot, slot + M);  // the engine's rows_distinct condition
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      return fail(MX_ERR_ARG, "mx_attention_probe: mode 1 needs every row in its own slot");
  } else {
    if (!q) return fail(MX_ERR_ARG, "mx_attention_probe: modes 0 and 2 take q");
    if (mode == 2 && !blocked_rows(slot, pos, nullptr, M))
      return fail(MX_ERR_ARG, "mx_attention_probe: mode 2 needs rows in 16-position blocks of one slot each");
  }
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs dev;
  _Float16 *d_k = nullptr, *d_v = nullptr;
  float *d_q = nullptr, *d_slabs = nullptr, *d_cs = nullptr;
  int *d_pos = nullptr, *d_slot = nullptr;
  void* d_out = nullptr;
  const size_t out_bytes = (size_t)M * nq * (out_f32 ? 4 : 2);
  const size_t cs_bytes = (size_t)n_ctx * head_dim * 4;
  if (!dev.alloc(&d_k, cache_elems * 2) || !dev.alloc(&d_v, cache_elems * 2) || !dev.alloc(&d_pos, (size_t)M * 4) ||
      !dev.alloc(&d_slot, (size_t)M * 4) || !dev.alloc_ff(&d_out, out_bytes) ||
      (mode == 1 ? !dev.alloc(&d_slabs, (size_t)nslab * M * N * 4) || !dev.alloc(&d_cs, cs_bytes)
                 : !dev.alloc(&d_q, (size_t)M * nq * 4)))
    return fail(MX_ERR_HIP, "mx_attention_probe: device allocation");
  HIPC(hipMemcpy(d_k, kcache, cache_elems * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_v, vcache, cache_elems * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_pos, pos, (size_t)M * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_slot, slot, (size_t)M * 4, hipMemcpyHostToDevice));
  AttnArgs at{};
  if (mode == 1) {
    HIPC(hipMemcpy(d_slabs, slabs, (size_t)nslab * M * N * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_cs, rope_cs, cs_bytes, hipMemcpyHostToDevice));
    at.slabs = d_slabs; at.nslab = nslab; at.slab_stride = (size_t)M * N; at.rope_cs = d_cs; at.kc_w = d_k;
    at.vc_w = d_v;
    if (bias) {
      float* d_bias = nullptr;
      if (!dev.alloc(&d_bias, N * 4)) return fail(MX_ERR_HIP, "mx_attention_probe: device allocation");
      HIPC(hipMemcpy(d_bias, bias, N * 4, hipMemcpyHostToDevice));
      at.qkv_bias = d_bias;
    }
  } else {
    HIPC(hipMemcpy(d_q, q, (size_t)M * nq * 4, hipMemcpyHostToDevice));
  }
  at.q = d_q; at.kc = d_k; at.vc = d_v; at.pos = d_pos; at.slot = d_slot;
  if (out_f32) at.outf = (float*)d_out;
  else at.out = (uint16_t*)d_out;
  at.ldo = (int)nq; at.M = M; at.n_head = n_head; at.n_head_kv = n_head_kv; at.head_dim = head_dim;
  at.n_ctx = n_ctx; at.ctx_stride = g.ctx_stride; at.slot_stride = g.slot_stride;
  at.scale = 1.0f / sqrtf((float)head_dim);
  HIPC(hipDeviceSynchronize());
  if (mode == 2) launch_attention_prefill(at, nullptr);
  else launch_attention(at, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(kcache, d_k, cache_elems * 2, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(vcache, d_v, cache_elems * 2, hipMemcpyDeviceToHost));
  return 0;
}

int mx_matmul_plan(int epi, int M, int N, int K, int32_t* kgroups, int32_t* pers_ok, int32_t* norm_on_load_ok,
                   int32_t* gemm_ok) {
  if (epi < EPI_F32 || epi > EPI_SWIGLU || M < 1 || N < TILE_N || N % TILE_N || K < TILE_K || K % TILE_K)
    return fail(MX_ERR_ARG, "mx_matmul_plan: epi 0..3, M >= 1, N a multiple of 16, K a multiple of 32");
  if (kgroups) *kgroups = canon_kgroups(epi, N, K);
  if (pers_ok) *pers_ok = mm_pers_supported(epi, M, N, K);
  if (norm_on_load_ok) *norm_on_load_ok = mm_can_norm_on_load(M, K);
  if (gemm_ok) *gemm_ok = gemm_supported(N, K);
  return 0;
}

int mx_matmul_probe(int device, const mx_matmul_args* pa) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  if (!pa) return fail(MX_ERR_ARG, "mx_matmul_probe: null arguments");
  const mx_matmul_args& p = *pa;
  const int path = p.path, epi = p.epi, M = p.M, N = p.N, K = p.K;
  if (path < 0 || path > 4 || epi < EPI_F32 || epi > EPI_SWIGLU)
    return fail(MX_ERR_ARG, "mx_matmul_probe: path 0..4, epi 0..3");
  if (N < TILE_N || N % TILE_N || K < TILE_K || K % TILE_K || N > (1 << 18) || K > 32768 ||
      (size_t)N * K > ((size_t)1 << 30))
    return fail(MX_ERR_ARG, "mx_matmul_probe: N a multiple of 16 (<= 2^18), K a multiple of 32 (<= 32768), N*K <= 2^30");
  const int min_m = path == 4 ? MAX_ROWS + 1 : 1;
  const int max_m = path == 1 ? 16 : path == 4 ? PREFILL_ROWS : MAX_ROWS;
  if (M < min_m || M > max_m)
    return fail(MX_ERR_ARG, "mx_matmul_probe: M 1..64 (path 1: 1..16; path 4: 65..4096)");
  if (!p.w || !p.out) return fail(MX_ERR_ARG, "mx_matmul_probe: w and out are required");
  const bool nol = p.x == nullptr;  // RMS_NORM on load
  if (nol) {
    if (path > 1 || M > 4 || epi == EPI_RESID || !p.xf || !p.norm_w)
      return fail(MX_ERR_ARG, "mx_matmul_probe: without x: paths 0 / 1, M <= 4, not RESID, xf and norm_w given");
    if (K % 64 || K / 16 > 512 || (path == 0 && !mm_can_norm_on_load(M, K)))
      return fail(MX_ERR_ARG, "mx_matmul_probe: K has no RMS_NORM-on-load form");
  }
  if (p.act_f32 && (epi != EPI_SWIGLU || (path == 4 && p.target > 0)))
    return fail(MX_ERR_ARG, "mx_matmul_probe: act_f32 is SWIGLU's, and the GEMM's split finish writes bf16 only");
  if (p.want_ssq && (epi != EPI_RESID || path > 1 || !p.ssq_out))
    return fail(MX_ERR_ARG, "mx_matmul_probe: want_ssq: RESID on paths 0 / 1, with ssq_out");
  const bool split_path = path >= 2 && (epi == EPI_QKV || epi == EPI_RESID || (path == 4 && epi == EPI_SWIGLU));
  if (epi == EPI_RESID) {
    if (!p.resid) return fail(MX_ERR_ARG, "mx_matmul_probe: RESID takes resid [M][N]");
    if (path >= 2 && (N % 64 || N > 16384))  // launch_resid_norm's widths
      return fail(MX_ERR_ARG, "mx_matmul_probe: RESID on a split path: N a multiple of 64, <= 16384");
  }
  QkvOperand qkv;
  if (epi == EPI_QKV)
    if (int rc = qkv.check("mx_matmul_probe", p, M, N)) return rc;
  // split-K slab space, sized before any launch: the launchers' own split can never exceed it
  size_t slab_stride = 0, slab_total = 0;
  int kg = 0;
  if (split_path && path != 4) {
    kg = canon_kgroups(epi, N, K);
    if (kg < 1 || kg > 16) return fail(MX_ERR_ARG, "mx_matmul_probe: K split above 16");
    slab_stride = (size_t)MAX_ROWS * N;
    slab_total = slab_stride * kg;
    if (p.slabs_out && p.slabs_cap < (uint64_t)kg * M * N)
      return fail(MX_ERR_ARG, "mx_matmul_probe: slabs_out holds fewer than kgroups * M * N floats");
  } else if (path == 4) {
    if (p.target < 0 || p.target > 256 || p.slab_floats > ((uint64_t)1 << 26))
      return fail(MX_ERR_ARG, "mx_matmul_probe: path 4: target 0..256, slab_floats <= 2^26");
    slab_total = epi == EPI_F32 ? 0 : (size_t)p.slab_floats;
    if (p.slabs_out && p.slabs_cap < slab_total)
      return fail(MX_ERR_ARG, "mx_matmul_probe: slabs_out holds fewer than slab_floats floats");
  }
  if (device >= 0) HIPC(hipSetDevice(device));

  DevBufs dev;
  const size_t wbytes = (size_t)N * K * 2;
  uint16_t *d_src = nullptr, *d_w = nullptr, *d_x = nullptr;
  float *d_xf = nullptr, *d_nw = nullptr, *d_ssq = nullptr, *d_slabs = nullptr;
  uint8_t* d_out = nullptr;
  const int ld = epi == EPI_SWIGLU ? N / 2 : epi == EPI_QKV ? qkv.n_q : N;
  const size_t esz = (epi == EPI_SWIGLU && !p.act_f32) ? 2 : 4;
  const size_t out_bytes = (size_t)(M + PROBE_GUARD_ROWS) * ld * esz;
  const int xrows = M <= 16 ? 16 : M <= 32 ? 32 : M <= 64 ? 64 : (M + 15) / 16 * 16;
  const int np = nol ? K / 16 : N / 16;
  const size_t ssq_bytes = (size_t)(nol ? 4 : M + PROBE_GUARD_ROWS) * np * 4;
  // an element no kernel wrote reads back as 0xFF bytes (NaN); activation rows >= M are bf16 NaN
  if (!dev.alloc(&d_src, wbytes) || !dev.alloc_ff(&d_w, wbytes) || !dev.alloc_ff(&d_out, out_bytes))
    return fail(MX_ERR_HIP, "mx_matmul_probe: device allocation");
  if (nol ? (!dev.alloc_ff(&d_xf, (size_t)4 * K * 4) || !dev.alloc(&d_nw, (size_t)K * 4))
          : !dev.alloc_ff(&d_x, (size_t)xrows * K * 2))
    return fail(MX_ERR_HIP, "mx_matmul_probe: device allocation");
  if ((nol || p.want_ssq) && !dev.alloc_ff(&d_ssq, ssq_bytes)) return fail(MX_ERR_HIP, "mx_matmul_probe: device allocation");
  if (slab_total && !dev.alloc_ff(&d_slabs, slab_total * 4)) return fail(MX_ERR_HIP, "mx_matmul_probe: device allocation");

  // weights: packed on the device exactly as upload_packed does at model load
  HIPC(hipMemcpy(d_src, p.w, wbytes, hipMemcpyHostToDevice));
  if (epi == EPI_SWIGLU) {
    launch_pack(d_w, d_src, N / 2, K, PACK_GATE, 0, nullptr);
    launch_pack(d_w, d_src + (size_t)(N / 2) * K, N / 2, K, PACK_UP, 0, nullptr);
  } else {
    launch_pack(d_w, d_src, N, K, PACK_ROWS, 0, nullptr);
  }
  HIPC(hipGetLastError());
  if (epi == EPI_RESID) HIPC(hipMemcpy(d_out, p.resid, (size_t)M * N * 4, hipMemcpyHostToDevice));
  MMArgs a{};
  a.W = d_w; a.N = N; a.K = K; a.M = M; a.eps = p.eps;
  if (nol) {
    HIPC(hipMemcpy(d_xf, p.xf, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_nw, p.norm_w, (size_t)K * 4, hipMemcpyHostToDevice));
    launch_ssq(d_xf, M, K, d_ssq, nullptr);  // the partials as the embedding writes them
    a.xf = d_xf; a.norm_w = d_nw; a.ssq = d_ssq; a.np = np;
  } else {
    HIPC(hipMemcpy(d_x, p.x, (size_t)M * K * 2, hipMemcpyHostToDevice));
    a.X = d_x; a.ldx = K;
    if (p.want_ssq) a.ssq = d_ssq, a.np = np;
  }
  if (epi == EPI_SWIGLU) {
    if (p.act_f32) a.actf = (float*)d_out;
    else a.act = (uint16_t*)d_out;
    a.lda = ld;
  } else {
    a.out = (float*)d_out; a.ldo = ld;
  }
  if (epi == EPI_QKV)
    if (int rc = qkv.upload("mx_matmul_probe", p, M, dev, a)) return rc;
  HIPC(hipDeviceSynchronize());

  int rc = -1;
  const char* who = "";
  std::vector<float> slab_host;  // the raw partials, taken before anything folds or finishes them
  auto grab_slabs = [&](int nslab, size_t stride) -> int {
    if (!p.slabs_out) return 0;
    HIPC(hipDeviceSynchronize());
    slab_host.resize((size_t)nslab * M * N);
    for (int k = 0; k < nslab; k++)
      HIPC(hipMemcpy(slab_host.data() + (size_t)k * M * N, d_slabs + k * stride, (size_t)M * N * 4,
                     hipMemcpyDeviceToHost));
    return 0;
  };
  if (path == 0) {
    who = "launch_mm";
    rc = launch_mm(epi, a, nullptr);
  } else if (path == 1) {
    who = "launch_mm_pers";
    rc = launch_mm_pers(epi, a, nullptr);
  } else if (path == 2 || path == 3) {
    who = "launch_mm_wide";
    rc = launch_mm_wide(epi, a, d_slabs, slab_stride, nullptr, false, path == 3);
    if (rc >= 0 && split_path) {
      if (rc < 1 || rc > kg) {
        hipDeviceSynchronize();
        return fail(MX_ERR_STATE, "launch_mm_wide split " + std::to_string(rc) + " outside canon_kgroups " +
                                      std::to_string(kg));
      }
      if (int e2 = grab_slabs(rc, slab_stride)) return e2;
      if (epi == EPI_QKV) launch_qkv_finish(a, d_slabs, rc, slab_stride, nullptr);
      else launch_resid_norm(nullptr, 0, (float*)d_out, d_slabs, rc, slab_stride, nullptr, M, N, p.eps, nullptr);
    }
  } else {
    who = "launch_gemm_split";
    rc = launch_gemm_split(epi, a, d_slabs, slab_total, p.target, nullptr);
    if (rc > 0 && epi == EPI_RESID)  // the engine's fold (slab stride M * N)
      launch_resid_norm(nullptr, 0, (float*)d_out, d_slabs, rc, (size_t)M * N, nullptr, M, N, p.eps, nullptr);
  }
  if (rc < 0) {
    hipDeviceSynchronize();
    return fail(MX_ERR_ARG, std::string("mx_matmul_probe: ") + who + " refused the shape");
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(p.out, d_out, out_bytes, hipMemcpyDeviceToHost));
  if (p.want_ssq) HIPC(hipMemcpy(p.ssq_out, d_ssq, (size_t)M * np * 4, hipMemcpyDeviceToHost));
  if (p.slabs_out) {
    if (path == 4) {
      if (slab_total) HIPC(hipMemcpy(p.slabs_out, d_slabs, slab_total * 4, hipMemcpyDeviceToHost));
    } else if (!slab_host.empty()) {
      memcpy(p.slabs_out, slab_host.data(), slab_host.size() * 4);
    }
  }
  if (p.split_out) *p.split_out = rc;
  if (p.packed_out) HIPC(hipMemcpy(p.packed_out, d_w, wbytes, hipMemcpyDeviceToHost));
  return epi == EPI_QKV ? qkv.download(p) : 0;
}

int mx_norm_probe(int device, int rows, int n, int M, const float* x, const float* slabs, int nslab, const float* w,
                  const int32_t* row_map, float eps, float* x_out, void* y_out) {
  if (rows < 1 || rows > PREFILL_ROWS || !x || !x_out)
    return fail(MX_ERR_ARG, "mx_norm_probe: 1 <= rows <= 4096, x and x_out required");
  if (n < 64 || n % 64 || n > 16384) return fail(MX_ERR_ARG, "mx_norm_probe: n a multiple of 64, <= 16384");
  if (nslab < 0 || nslab > 16 || (nslab > 0 && !slabs))
    return fail(MX_ERR_ARG, "mx_norm_probe: 0 <= nslab <= 16, slabs given when nslab > 0");
  if (w && !y_out) return fail(MX_ERR_ARG, "mx_norm_probe: w needs y_out");
  if (row_map) {
    if (nslab || !w || M < 1 || M > PREFILL_ROWS)
      return fail(MX_ERR_ARG, "mx_norm_probe: row_map: no slabs, w given, 1 <= M <= 4096");
    for (int i = 0; i < M; i++)
      if (row_map[i] < 0 || row_map[i] >= rows) return fail(MX_ERR_ARG, "mx_norm_probe: row_map entry out of range");
  } else if (M != rows) {
    return fail(MX_ERR_ARG, "mx_norm_probe: without row_map M == rows");
  }
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs dev;
  float *d_x = nullptr, *d_slabs = nullptr, *d_w = nullptr;
  uint16_t* d_y = nullptr;
  int* d_map = nullptr;
  const size_t xb = (size_t)(rows + PROBE_GUARD_ROWS) * n * 4, yb = (size_t)(M + PROBE_GUARD_ROWS) * n * 2;
  const size_t stride = (size_t)rows * n;
  if (!dev.alloc_ff(&d_x, xb) || (nslab && !dev.alloc(&d_slabs, stride * nslab * 4)) ||
      (w && (!dev.alloc(&d_w, (size_t)n * 4) || !dev.alloc_ff(&d_y, yb))) || (row_map && !dev.alloc(&d_map, (size_t)M * 4)))
    return fail(MX_ERR_HIP, "mx_norm_probe: device allocation");
  HIPC(hipMemcpy(d_x, x, stride * 4, hipMemcpyHostToDevice));
  if (nslab) HIPC(hipMemcpy(d_slabs, slabs, stride * nslab * 4, hipMemcpyHostToDevice));
  if (w) {
    HIPC(hipMemcpy(d_w, w, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (row_map) HIPC(hipMemcpy(d_map, row_map, (size_t)M * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  if (row_map) launch_rmsnorm(d_y, n, d_x, d_w, d_map, M, n, eps, nullptr);
  else launch_resid_norm(d_y, n, d_x, d_slabs, nslab, stride, d_w, M, n, eps, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(x_out, d_x, xb, hipMemcpyDeviceToHost));
  if (w) HIPC(hipMemcpy(y_out, d_y, yb, hipMemcpyDeviceToHost));
  return 0;
}

int mx_q8_matmul_plan(int epi, int M, int N, int K, int wq4, int on_load, int norm, mx_q8_plan* out) {
  if (!out) return fail(MX_ERR_ARG, "mx_q8_matmul_plan: null plan");
  if (epi < EPI_F32 || epi > EPI_SWIGLU || M < 1 || N < TILE_N || N % TILE_N || K < Q8_TILE_K || K % Q8_TILE_K)
    return fail(MX_ERR_ARG, "mx_q8_matmul_plan: epi 0..3, M >= 1, N a multiple of 16, K a multiple of 64");
  const Mq8Plan p = mq8_plan(epi, M, N, K, wq4 != 0, on_load != 0, norm != 0);
  *out = mx_q8_plan{p.kind, p.qp, p.qm, p.tpw, p.ks, p.rt, p.nb, p.bd, p.grid_y, p.w, p.grid,
                    on_load ? -1 : mq8_slab_ks(M, N, K), mq8_can_quantize_on_load(M, K, norm != 0) ? 1 : 0};
  return 0;
}

int mx_q8_matmul_probe(int device, const mx_q8_matmul_args* pa) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  if (!pa) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: null arguments");
  const mx_q8_matmul_args& p = *pa;
  const int path = p.path, epi = p.epi, M = p.M, N = p.N, K = p.K, act = p.act;
  const bool mm = path >= 0;  // path -1: quantise only
  if (path < -1 || path > 1 || act < 0 || act > 2 || (p.wq4 != 0 && p.wq4 != 1))
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: path -1..1, act 0..2, wq4 0 / 1");
  if (mm && (epi < EPI_F32 || epi > EPI_SWIGLU)) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: epi 0..3");
  if (K < Q8_TILE_K || K % Q8_TILE_K || K > 32768)
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: K a multiple of 64, <= 32768");
  if (mm && (N < TILE_N || N % TILE_N || N > (1 << 18) || (size_t)N * K > ((size_t)1 << 30) || !p.w || !p.out))
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: N a multiple of 16 (<= 2^18), N*K <= 2^30, w and out required");
  if (mm && epi == EPI_SWIGLU && N % 32) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: SWIGLU: N a multiple of 32");
  if (M < 1 || M > PREFILL_ROWS) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: 1 <= M <= PREFILL_ROWS rows");
  if (path == 1 && (M <= 16 || M > 32 || act == 2 || (epi != EPI_RESID && epi != EPI_QKV)))
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: path 1 (slabs): 17..32 pre-quantised rows, RESID or QKV");
  if (!p.xf) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: xf is required");
  int xrows = M, ldx = K;
  if (act == 0) {
    ldx = p.ldx ? p.ldx : K;
    if (ldx < K || ldx % 4 || ldx > 65536) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 0: K <= ldx <= 65536, ldx % 4 == 0");
    if (p.norm_w || p.row_map || p.nslab) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 0 takes no norm_w / row_map / slabs");
  } else if (act == 1) {
    xrows = p.xrows ? p.xrows : M;
    if (!p.norm_w || xrows < 1 || xrows > PREFILL_ROWS || (p.ldx && p.ldx != K))
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 1: norm_w given, 1 <= xrows <= PREFILL_ROWS, ldx = K");
    if (p.nslab < 0 || p.nslab > 8 || (p.nslab > 0 && (!p.fold_slabs || p.row_map || K > 16384)))
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 1: nslab 0..8 with fold_slabs, no row_map, K <= 16384");
    if (p.row_map) {
      for (int i = 0; i < M; i++)
        if (p.row_map[i] < 0 || p.row_map[i] >= xrows) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: row_map entry out of range");
    } else if (xrows != M) {
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 1 without row_map: xrows = M");
    }
  } else {
    if (path != 0 || p.row_map || p.nslab || (p.ldx && p.ldx != K))
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: act 2 (quantise on load): path 0, no row_map / slabs, ldx = K");
    if (!mq8_can_quantize_on_load(M, K, p.norm_w != nullptr))
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: mq8_can_quantize_on_load refuses M / K");
  }
  if (p.np && (act != 2 || !p.norm_w || p.np < 4 || p.np % 4 || p.np * 16 >= K))
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: np: act 2 with norm_w, a multiple of 4 in [4, K / 16)");
  if (p.want_ssq && (!mm || epi != EPI_RESID || path != 0 || !p.ssq_out || (act == 2 && p.norm_w)))
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: want_ssq: RESID on path 0, with ssq_out, no norm on load");
  if (mm && epi == EPI_RESID) {
    if (!p.resid) return fail(MX_ERR_ARG, "mx_q8_matmul_probe: RESID takes resid [M][N]");
    if (path == 1 && (!p.fold_w || N % 64 || N > 16384))
      return fail(MX_ERR_ARG, "mx_q8_matmul_probe: RESID slabs: fold_w [N], N a multiple of 64, <= 16384");
  }
  QkvOperand qkv;
  if (mm && epi == EPI_QKV)
    if (int rc = qkv.check("mx_q8_matmul_probe", p, M, N)) return rc;
  const size_t slab_stride = (size_t)MAX_ROWS * (mm ? N : 0), slab_total = path == 1 ? slab_stride * 8 : 0;  // ks <= 8
  if (path == 1 && p.slabs_out && p.slabs_cap < (uint64_t)8 * M * N)
    return fail(MX_ERR_ARG, "mx_q8_matmul_probe: slabs_out holds fewer than 8 * M * N floats");
  if (device >= 0) HIPC(hipSetDevice(device));

  DevBufs dev;
  const size_t bb = p.wq4 ? 18 : 34;
  const size_t raw_bytes = mm ? (size_t)N * (K / 32) * bb : 0;
  const size_t wbytes = mm ? (p.wq4 ? q4_matrix_bytes(N, K) : q8_matrix_bytes(N, K)) : 0;
  uint8_t *d_src = nullptr, *d_w = nullptr, *d_out = nullptr;
  float *d_xf = nullptr, *d_nw = nullptr, *d_ssq = nullptr, *d_slabs = nullptr, *d_fs = nullptr;
  float *d_xd = nullptr, *d_fw = nullptr, *d_nxd = nullptr;
  int8_t *d_xq = nullptr, *d_nxq = nullptr;
  int* d_map = nullptr;
  const int ld = !mm ? 0 : epi == EPI_SWIGLU ? N / 2 : epi == EPI_QKV ? qkv.n_q : N;
  const size_t out_bytes = (size_t)(M + PROBE_GUARD_ROWS) * ld * 4;
  const int xalloc = (act == 2 ? XQ_ON_LOAD_ROWS : xrows) + 16;  // f32 source rows; those past the caller's are NaN
  const size_t xf_bytes = (size_t)xalloc * ldx * 4;
  const int qrows = (M + 127) / 128 * 128 + PROBE_GUARD_ROWS;  // Q8_0 rows; those past M stay 0xFF (d_x NaN)
  const size_t xq_bytes = (size_t)qrows * K, xd_bytes = (size_t)qrows * (K / 32) * 4;
  const bool nol = act == 2 && p.norm_w;
  const int np = nol ? K / 16 : N / 16;
  const size_t ssq_bytes = (size_t)(nol ? XQ_ON_LOAD_ROWS : M + PROBE_GUARD_ROWS) * np * 4;
  const size_t fs_stride = (size_t)xrows * K;
  if (!dev.alloc_ff(&d_xf, xf_bytes) || !dev.alloc_ff(&d_xq, xq_bytes) || !dev.alloc_ff(&d_xd, xd_bytes) ||
      (p.norm_w && !dev.alloc(&d_nw, (size_t)K * 4)) || (p.row_map && !dev.alloc(&d_map, (size_t)M * 4)) ||
      (p.nslab && !dev.alloc(&d_fs, fs_stride * p.nslab * 4)))
    return fail(MX_ERR_HIP, "mx_q8_matmul_probe: device allocation");
  if (mm && (!dev.alloc(&d_src, raw_bytes) || !dev.alloc_ff(&d_w, wbytes) || !dev.alloc_ff(&d_out, out_bytes) ||
             ((nol || p.want_ssq) && !dev.alloc_ff(&d_ssq, ssq_bytes)) ||
             (slab_total && !dev.alloc_ff(&d_slabs, slab_total * 4))))
    return fail(MX_ERR_HIP, "mx_q8_matmul_probe: device allocation");
  if (path == 1 && epi == EPI_RESID &&
      (!dev.alloc(&d_fw, (size_t)N * 4) || !dev.alloc_ff(&d_nxq, (size_t)(M + PROBE_GUARD_ROWS) * N) ||
       !dev.alloc_ff(&d_nxd, (size_t)(M + PROBE_GUARD_ROWS) * (N / 32) * 4)))
    return fail(MX_ERR_HIP, "mx_q8_matmul_probe: device allocation");

  MMArgs a{};
  if (mm) {  // weights: packed on the device exactly as at model load
    HIPC(hipMemcpy(d_src, p.w, raw_bytes, hipMemcpyHostToDevice));
    auto pack = p.wq4 ? launch_pack_q4 : launch_pack_q8;
    if (epi == EPI_SWIGLU) {
      pack(d_w, d_src, N / 2, K, PACK_GATE, 0, nullptr);
      pack(d_w, d_src + (size_t)(N / 2) * (K / 32) * bb, N / 2, K, PACK_UP, 0, nullptr);
    } else {
      pack(d_w, d_src, N, K, PACK_ROWS, 0, nullptr);
    }
    HIPC(hipGetLastError());
    if (epi == EPI_RESID) HIPC(hipMemcpy(d_out, p.resid, (size_t)M * N * 4, hipMemcpyHostToDevice));
    a.W = reinterpret_cast<const uint16_t*>(d_w); a.N = N; a.K = K; a.M = M; a.eps = p.eps; a.wq4 = p.wq4;
  }
  HIPC(hipMemcpy(d_xf, p.xf, (size_t)(act == 2 ? M : xrows) * ldx * 4, hipMemcpyHostToDevice));
  if (p.norm_w) HIPC(hipMemcpy(d_nw, p.norm_w, (size_t)K * 4, hipMemcpyHostToDevice));
  if (p.row_map) HIPC(hipMemcpy(d_map, p.row_map, (size_t)M * 4, hipMemcpyHostToDevice));
  if (p.nslab) HIPC(hipMemcpy(d_fs, p.fold_slabs, fs_stride * p.nslab * 4, hipMemcpyHostToDevice));
  if (d_fw) {
    HIPC(hipMemcpy(d_fw, p.fold_w, (size_t)N * 4, hipMemcpyHostToDevice));
  }
  if (mm && epi == EPI_QKV)
    if (int rc = qkv.upload("mx_q8_matmul_probe", p, M, dev, a)) return rc;
  HIPC(hipDeviceSynchronize());

  // the operand, as mx_engine::quant_operand makes it (Q8_0 rows)
  if (act == 2) {
    a.xq = nullptr; a.xf = d_xf; a.norm_w = d_nw; a.np = p.np ? p.np : K / 16;
    if (nol) {
      launch_ssq(d_xf, M, K, d_ssq, nullptr);  // the partials as the embedding / the residual writers leave them
      a.ssq = d_ssq;
    }
  } else {
    if (act == 1) launch_rmsnorm_q8(d_xq, d_xd, d_xf, d_nw, d_map, M, K, p.eps, nullptr, d_fs, p.nslab, fs_stride);
    else launch_quantize_q8(d_xq, d_xd, d_xf, ldx, M, K, nullptr);
    HIPC(hipGetLastError());
    a.xq = d_xq; a.xd = d_xd;
  }
  if (mm) {
    if (epi == EPI_SWIGLU) {
      if (p.act_f32) a.actf = (float*)d_out;
      a.lda = ld;
    } else {
      a.out = (float*)d_out; a.ldo = ld;
    }
    if (p.want_ssq) a.ssq = d_ssq, a.np = np;
  }
  int rc = 0;
  const char* who = "";
  std::vector<float> slab_host;  // the raw partials, taken before anything folds or finishes them
  if (path == 0) {
    who = "launch_mq8";
    rc = launch_mq8(epi, a, nullptr);
  } else if (path == 1) {
    who = "launch_mq8_slab";
    rc = launch_mq8_slab(a, d_slabs, slab_stride, nullptr);
    if (rc > 8) {
      hipDeviceSynchronize();
      return fail(MX_ERR_STATE, "launch_mq8_slab split " + std::to_string(rc) + " above 8");
    }
    if (rc > 0) {
      if (p.slabs_out) {
        HIPC(hipDeviceSynchronize());
        slab_host.resize((size_t)rc * M * N);
        for (int k = 0; k < rc; k++)
          HIPC(hipMemcpy(slab_host.data() + (size_t)k * M * N, d_slabs + k * slab_stride, (size_t)M * N * 4,
                         hipMemcpyDeviceToHost));
      }
      if (epi == EPI_QKV) launch_qkv_finish(a, d_slabs, rc, slab_stride, nullptr);
      else launch_rmsnorm_q8(d_nxq, d_nxd, (float*)d_out, d_fw, nullptr, M, N, p.eps, nullptr, d_slabs, rc, slab_stride);
    }
  }
  if (rc < 0) {
    hipDeviceSynchronize();
    return fail(MX_ERR_ARG, std::string("mx_q8_matmul_probe: ") + who + " refused the shape");
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  if (mm) HIPC(hipMemcpy(p.out, d_out, out_bytes, hipMemcpyDeviceToHost));
  if (p.want_ssq) HIPC(hipMemcpy(p.ssq_out, d_ssq, (size_t)(M + PROBE_GUARD_ROWS) * np * 4, hipMemcpyDeviceToHost));
  if (p.slabs_out && !slab_host.empty()) memcpy(p.slabs_out, slab_host.data(), slab_host.size() * 4);
  if (p.split_out) *p.split_out = rc;
  if (p.packed_out && mm) HIPC(hipMemcpy(p.packed_out, d_w, wbytes, hipMemcpyDeviceToHost));
  if (p.xq_out) HIPC(hipMemcpy(p.xq_out, d_xq, (size_t)(M + PROBE_GUARD_ROWS) * K, hipMemcpyDeviceToHost));
  if (p.xd_out) HIPC(hipMemcpy(p.xd_out, d_xd, (size_t)(M + PROBE_GUARD_ROWS) * (K / 32) * 4, hipMemcpyDeviceToHost));
  if (p.x_out) HIPC(hipMemcpy(p.x_out, d_xf, (size_t)xrows * ldx * 4, hipMemcpyDeviceToHost));
  if (p.nxq_out && d_nxq) HIPC(hipMemcpy(p.nxq_out, d_nxq, (size_t)(M + PROBE_GUARD_ROWS) * N, hipMemcpyDeviceToHost));
  if (p.nxd_out && d_nxd)
    HIPC(hipMemcpy(p.nxd_out, d_nxd, (size_t)(M + PROBE_GUARD_ROWS) * (N / 32) * 4, hipMemcpyDeviceToHost));
  return mm && epi == EPI_QKV ? qkv.download(p) : 0;
}

int mx_q8_side_probe(int device, int mode, int N, int K, const void* blocks, const int32_t* ids, int M, void* out,
                     float* ssq_out) {
  if (mode < 0 || mode > 1 || !blocks || !out) return fail(MX_ERR_ARG, "mx_q8_side_probe: mode 0 / 1, blocks and out required");
  if (N < 1 || N > (1 << 18) || K < Q8_TILE_K || K % Q8_TILE_K || K > 32768 || (size_t)N * K > ((size_t)1 << 28))
    return fail(MX_ERR_ARG, "mx_q8_side_probe: 1 <= N <= 2^18, K a multiple of 64 (<= 32768), N*K <= 2^28");
  if (mode == 0 && N % TILE_N) return fail(MX_ERR_ARG, "mx_q8_side_probe: mode 0: N a multiple of 16");
  if (mode == 1) {
    if (!ids || M < 1 || M > PREFILL_ROWS) return fail(MX_ERR_ARG, "mx_q8_side_probe: mode 1: ids [M], 1 <= M <= PREFILL_ROWS");
    for (int i = 0; i < M; i++)
      if (ids[i] < 0 || ids[i] >= N) return fail(MX_ERR_ARG, "mx_q8_side_probe: id out of range");
  }
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs dev;
  uint8_t *d_src = nullptr, *d_w = nullptr, *d_out = nullptr;
  float* d_ssq = nullptr;
  int* d_ids = nullptr;
  const size_t raw = (size_t)N * (K / 32) * 34;
  if (!dev.alloc(&d_src, raw)) return fail(MX_ERR_HIP, "mx_q8_side_probe: device allocation");
  HIPC(hipMemcpy(d_src, blocks, raw, hipMemcpyHostToDevice));
  if (mode == 0) {  // packed Q8 tiles -> packed bf16 tiles
    const size_t ob = (size_t)(N + PROBE_GUARD_ROWS) * K * 2;
    if (!dev.alloc_ff(&d_w, q8_matrix_bytes(N, K)) || !dev.alloc_ff(&d_out, ob))
      return fail(MX_ERR_HIP, "mx_q8_side_probe: device allocation");
    launch_pack_q8(d_w, d_src, N, K, PACK_ROWS, 0, nullptr);
    if (launch_dequant_q8_tiles((uint16_t*)d_out, d_w, N, K, nullptr)) {
      hipDeviceSynchronize();
      return fail(MX_ERR_ARG, "mx_q8_side_probe: launch_dequant_q8_tiles refused the shape");
    }
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
    return 0;
  }
  const size_t ob = (size_t)(M + PROBE_GUARD_ROWS) * K * 4, sb = (size_t)(M + PROBE_GUARD_ROWS) * (K / 16) * 4;
  if (!dev.alloc_ff(&d_out, ob) || !dev.alloc(&d_ids, (size_t)M * 4) || (ssq_out && !dev.alloc_ff(&d_ssq, sb)))
    return fail(MX_ERR_HIP, "mx_q8_side_probe: device allocation");
  HIPC(hipMemcpy(d_ids, ids, (size_t)M * 4, hipMemcpyHostToDevice));
  launch_embed_q8((float*)d_out, d_src, d_ids, M, K, d_ssq, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
  if (ssq_out) HIPC(hipMemcpy(ssq_out, d_ssq, sb, hipMemcpyDeviceToHost));
  return 0;
}

int mx_kq_matmul_plan(int epi, int M, int N, int K, int on_load, int norm, int kq_n, const int32_t* kq_type,
                      const int32_t* kq_tile_end, int flags, mx_kq_plan* out) {
  if (!out || !kq_type || !kq_tile_end) return fail(MX_ERR_ARG, "mx_kq_matmul_plan: null plan or segments");
  if (epi < EPI_F32 || epi > EPI_SWIGLU || M < 1 || N < TILE_N || N % TILE_N || K < 256 || K % 256 || kq_n < 1 ||
      kq_n > 3 || flags < -1 || flags > 7)
    return fail(MX_ERR_ARG, "mx_kq_matmul_plan: epi 0..3, M >= 1, N a multiple of 16, K of 256, 1..3 segments, flags -1..7");
  const MkqEnv env = kq_probe_env(flags);
  const MkqPlan p = mkq_plan(epi, M, N, K, on_load != 0, norm != 0, kq_n, kq_type, kq_tile_end, env);
  *out = mx_kq_plan{p.kind, p.t, p.ks, p.nkw, p.tpw, p.nb, p.u, p.bd, p.ql, p.w, p.grid_x, p.grid_y,
                    on_load ? -1 : mkq_slab_ks(M, N, K, kq_n, kq_type, env),
                    on_load ? -1 : mkq_qkv_slab_ks(M, N, K, kq_n, kq_tile_end, env),
                    mkq_can_quantize_on_load(M, K, norm != 0) ? 1 : 0};
  return 0;
}

int mx_kq_matmul_probe(int device, const mx_kq_matmul_args* pa) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  if (!pa) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: null arguments");
  const mx_kq_matmul_args& p = *pa;
  const int path = p.path, epi = p.epi, M = p.M, N = p.N, K = p.K, act = p.act;
  const bool mm = path >= 0;  // path -1: quantise only
  if (path < -1 || path > 2 || act < 0 || act > 2) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: path -1..2, act 0..2");
  if (mm && (epi < EPI_F32 || epi > EPI_SWIGLU)) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: epi 0..3");
  if (K < 256 || K % 256 || K > 32768) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: K a multiple of 256, <= 32768");
  if (mm && (N < TILE_N || N % TILE_N || N > (1 << 18) || (size_t)N * K > ((size_t)1 << 30) || !p.w || !p.out))
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: N a multiple of 16 (<= 2^18), N*K <= 2^30, w and out required");
  if (mm && !kq_segments_ok(p.kq_n, p.kq_type, p.kq_tile_end, N))
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: 1..3 segments of type 12 / 13 / 14, tile ends increasing to N / 16");
  if (mm && epi == EPI_SWIGLU && (N % 32 || p.kq_n != 1))
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: SWIGLU: one segment, N a multiple of 32");
  if (M < 1 || M > PREFILL_ROWS) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: 1 <= M <= PREFILL_ROWS rows");
  if (path >= 1 && (M > MAX_ROWS || act == 2 || epi != (path == 1 ? EPI_RESID : EPI_QKV)))
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: paths 1 / 2 (slabs): <= 64 pre-quantised rows, RESID / QKV");
  if (!p.xf) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: xf is required");
  int xrows = M, ldx = K;
  if (act == 0) {
    ldx = p.ldx ? p.ldx : K;
    if (ldx < K || ldx % 4 || ldx > 65536) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: act 0: K <= ldx <= 65536, ldx % 4 == 0");
    if (p.norm_w || p.row_map) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: act 0 takes no norm_w / row_map");
  } else if (act == 1) {
    xrows = p.xrows ? p.xrows : M;
    if (!p.norm_w || xrows < 1 || xrows > PREFILL_ROWS || (p.ldx && p.ldx != K))
      return fail(MX_ERR_ARG, "mx_kq_matmul_probe: act 1: norm_w given, 1 <= xrows <= PREFILL_ROWS, ldx = K");
    if (p.row_map) {
      for (int i = 0; i < M; i++)
        if (p.row_map[i] < 0 || p.row_map[i] >= xrows) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: row_map entry out of range");
    } else if (xrows != M) {
      return fail(MX_ERR_ARG, "mx_kq_matmul_probe: act 1 without row_map: xrows = M");
    }
  } else {
    if (path != 0 || M != 1 || p.row_map || (p.ldx && p.ldx != K))
      return fail(MX_ERR_ARG, "mx_kq_matmul_probe: act 2 (quantise on load): path 0, one row, no row_map, ldx = K");
    if (!mkq_can_quantize_on_load(M, K, p.norm_w != nullptr))
      return fail(MX_ERR_ARG, "mx_kq_matmul_probe: mkq_can_quantize_on_load refuses K");
  }
  const bool nol = act == 2 && p.norm_w;
  if (p.ssq_in && !nol) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: ssq_in: act 2 with norm_w");
  if (p.want_ssq && (!mm || epi != EPI_RESID || path != 0 || !p.ssq_out || nol))
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: want_ssq: RESID on path 0, with ssq_out, no norm on load");
  if (mm && epi == EPI_RESID) {
    if (!p.resid) return fail(MX_ERR_ARG, "mx_kq_matmul_probe: RESID takes resid [M][N]");
    if (path == 1 && (!p.fold_w || N % 64 || N > 16384))
      return fail(MX_ERR_ARG, "mx_kq_matmul_probe: RESID slabs: fold_w [N], N a multiple of 64, <= 16384");
  }
  QkvOperand qkv;
  if (mm && epi == EPI_QKV)
    if (int rc = qkv.check("mx_kq_matmul_probe", p, M, N)) return rc;
  // the split the launcher will take (it dispatches on the same function): the slab buffer holds exactly ks slabs
  const int ks_plan = path == 1   ? mkq_slab_ks(M, N, K, p.kq_n, p.kq_type, mkq_env())
                      : path == 2 ? mkq_qkv_slab_ks(M, N, K, p.kq_n, p.kq_tile_end, mkq_env())
                                  : 0;
  const size_t slab_stride = mm ? (size_t)M * N : 0, slab_total = ks_plan > 0 ? slab_stride * ks_plan : 0;
  if (path >= 1 && p.slabs_out && p.slabs_cap < (uint64_t)slab_stride * 8)
    return fail(MX_ERR_ARG, "mx_kq_matmul_probe: slabs_out holds fewer than 8 * M * N floats");
  if (device >= 0) HIPC(hipSetDevice(device));

  DevBufs dev;
  const int SB = K / 256;
  size_t raw_bytes = 0, wbytes = 0, raw_off[3] = {0, 0, 0}, w_off[3] = {0, 0, 0};
  int seg_rows[3] = {0, 0, 0};
  if (mm)
    for (int i = 0; i < p.kq_n; i++) {
      seg_rows[i] = (p.kq_tile_end[i] - (i ? p.kq_tile_end[i - 1] : 0)) * TILE_N;
      raw_off[i] = raw_bytes, w_off[i] = wbytes;
      raw_bytes += (size_t)seg_rows[i] * SB * kq_block_bytes(p.kq_type[i]);
      wbytes += kq_matrix_bytes(p.kq_type[i], seg_rows[i], K);
    }
  uint8_t *d_src = nullptr, *d_w = nullptr, *d_out = nullptr;
  float *d_xf = nullptr, *d_nw = nullptr, *d_ssq = nullptr, *d_slabs = nullptr;
  float *d_xd = nullptr, *d_xb = nullptr, *d_fw = nullptr, *d_nxd = nullptr, *d_nxb = nullptr;
  int8_t *d_xq = nullptr, *d_nxq = nullptr;
  int* d_map = nullptr;
  const int ld = !mm ? 0 : epi == EPI_SWIGLU ? N / 2 : epi == EPI_QKV ? qkv.n_q : N;
  const size_t out_bytes = (size_t)(M + PROBE_GUARD_ROWS) * ld * 4;
  const size_t xf_bytes = (size_t)(act == 2 ? 1 : xrows) * ldx * 4;
  const int qrows = M + PROBE_GUARD_ROWS;  // Q8_K rows; those past M stay 0xFF
  const size_t xq_bytes = (size_t)qrows * K, xd_bytes = (size_t)qrows * SB * 4, xb_bytes = (size_t)qrows * (K / 32) * 4;
  const int np = nol ? K / 16 : N / 16;
  const size_t ssq_bytes = nol ? (size_t)np * 4 : (size_t)(M + PROBE_GUARD_ROWS) * np * 4;
  const bool fold_q8k = path == 1 && N % 256 == 0 && N <= 4096;  // launch_rmsnorm_q8k's fold; else launch_resid_norm
  if (!dev.alloc(&d_xf, xf_bytes) || (p.norm_w && !dev.alloc(&d_nw, (size_t)K * 4)) ||
      (p.row_map && !dev.alloc(&d_map, (size_t)M * 4)) ||
      (act != 2 && (!dev.alloc_ff(&d_xq, xq_bytes) || !dev.alloc_ff(&d_xd, xd_bytes) || !dev.alloc_ff(&d_xb, xb_bytes))))
    return fail(MX_ERR_HIP, "mx_kq_matmul_probe: device allocation");
  if (mm && (!dev.alloc(&d_src, raw_bytes) || !dev.alloc_ff(&d_w, wbytes) || !dev.alloc_ff(&d_out, out_bytes) ||
             ((nol || p.want_ssq) && !dev.alloc_ff(&d_ssq, ssq_bytes)) ||
             (slab_total && !dev.alloc_ff(&d_slabs, slab_total * 4))))
    return fail(MX_ERR_HIP, "mx_kq_matmul_probe: device allocation");
  if (fold_q8k && (!dev.alloc(&d_fw, (size_t)N * 4) || !dev.alloc_ff(&d_nxq, (size_t)qrows * N) ||
                   !dev.alloc_ff(&d_nxd, (size_t)qrows * (N / 256) * 4) ||
                   !dev.alloc_ff(&d_nxb, (size_t)qrows * (N / 32) * 4)))
    return fail(MX_ERR_HIP, "mx_kq_matmul_probe: device allocation");

  MMArgs a{};
  if (mm) {  // weights: every segment packed on the device exactly as at model load
    HIPC(hipMemcpy(d_src, p.w, raw_bytes, hipMemcpyHostToDevice));
    for (int i = 0; i < p.kq_n; i++) {
      const uint8_t* src = d_src + raw_off[i];
      int rc;
      if (epi == EPI_SWIGLU) {
        rc = launch_pack_kq(d_w, src, p.kq_type[0], N / 2, K, PACK_GATE, 0, nullptr);
        if (!rc)
          rc = launch_pack_kq(d_w, src + (size_t)(N / 2) * SB * kq_block_bytes(p.kq_type[0]), p.kq_type[0], N / 2, K, PACK_UP,
                              0, nullptr);
      } else {
        rc = launch_pack_kq(d_w + w_off[i], src, p.kq_type[i], seg_rows[i], K, PACK_ROWS, 0, nullptr);
      }
      if (rc) {
        hipDeviceSynchronize();
        return fail(MX_ERR_ARG, "mx_kq_matmul_probe: launch_pack_kq refused the shape");
      }
    }
    HIPC(hipGetLastError());
    if (epi == EPI_RESID) HIPC(hipMemcpy(d_out, p.resid, (size_t)M * N * 4, hipMemcpyHostToDevice));
    a.W = reinterpret_cast<const uint16_t*>(d_w); a.N = N; a.K = K; a.M = M; a.eps = p.eps;
    a.kq_n = p.kq_n;
    for (int i = 0; i < p.kq_n; i++) a.kq_type[i] = p.kq_type[i], a.kq_tile_end[i] = p.kq_tile_end[i], a.kq_off[i] = w_off[i];
  }
  HIPC(hipMemcpy(d_xf, p.xf, xf_bytes, hipMemcpyHostToDevice));
  if (act != 2) {
  }
  if (p.norm_w) HIPC(hipMemcpy(d_nw, p.norm_w, (size_t)K * 4, hipMemcpyHostToDevice));
  if (p.row_map) HIPC(hipMemcpy(d_map, p.row_map, (size_t)M * 4, hipMemcpyHostToDevice));
  if (d_fw) {
    HIPC(hipMemcpy(d_fw, p.fold_w, (size_t)N * 4, hipMemcpyHostToDevice));
  }
  if (mm && epi == EPI_QKV)
    if (int rc = qkv.upload("mx_kq_matmul_probe", p, M, dev, a)) return rc;

  // the operand, as mx_engine::quant_operand makes it (Q8_K rows)
  int rc = 0;
  const char* who = "";
  if (act == 2) {
    a.xq = nullptr; a.xf = d_xf; a.norm_w = d_nw; a.np = K / 16;
    if (nol) {
      if (p.ssq_in) HIPC(hipMemcpy(d_ssq, p.ssq_in, ssq_bytes, hipMemcpyHostToDevice));
      else launch_ssq(d_xf, 1, K, d_ssq, nullptr);  // the partials as the embedding / the residual writers leave them
      a.ssq = d_ssq;
    }
  } else {
    who = act == 1 ? "launch_rmsnorm_q8k" : "launch_quantize_q8k";
    rc = act == 1 ? launch_rmsnorm_q8k(d_xq, d_xd, d_xb, d_xf, d_nw, d_map, M, K, p.eps, nullptr)
                  : launch_quantize_q8k(d_xq, d_xd, d_xb, d_xf, ldx, M, K, nullptr);
    a.xq = d_xq; a.xd = d_xd; a.xb = d_xb;
  }
  if (mm && !rc) {
    if (epi == EPI_SWIGLU) {
      a.actf = (float*)d_out; a.lda = ld;
    } else {
      a.out = (float*)d_out; a.ldo = ld;
    }
    if (p.want_ssq) a.ssq = d_ssq, a.np = np;
    if (path == 0) {
      who = "launch_mkq";
      rc = launch_mkq(epi, a, nullptr);
    } else {
      who = path == 1 ? "launch_mkq_slab" : "launch_mkq_qkv_slab";
      rc = path == 1 ? launch_mkq_slab(a, d_slabs, slab_stride, nullptr) : launch_mkq_qkv_slab(a, d_slabs, slab_stride, nullptr);
      if (rc > 0 && rc != ks_plan) {
        hipDeviceSynchronize();
        return fail(MX_ERR_STATE, std::string(who) + " split " + std::to_string(rc) + ", planned " + std::to_string(ks_plan));
      }
      if (rc > 0 && path == 2) {
        launch_qkv_finish(a, d_slabs, rc, slab_stride, nullptr);
      } else if (rc > 0 && fold_q8k) {
        if (launch_rmsnorm_q8k(d_nxq, d_nxd, d_nxb, (float*)d_out, d_fw, nullptr, M, N, p.eps, nullptr, d_slabs, rc, slab_stride))
          who = "launch_rmsnorm_q8k (fold)", rc = -1;
      } else if (rc > 0) {
        launch_resid_norm(nullptr, 0, (float*)d_out, d_slabs, rc, slab_stride, nullptr, M, N, p.eps, nullptr);
      }
    }
  }
  if (rc < 0) {
    hipDeviceSynchronize();
    return fail(MX_ERR_ARG, std::string("mx_kq_matmul_probe: ") + who + " refused the shape");
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  if (mm) HIPC(hipMemcpy(p.out, d_out, out_bytes, hipMemcpyDeviceToHost));
  if (p.want_ssq) HIPC(hipMemcpy(p.ssq_out, d_ssq, ssq_bytes, hipMemcpyDeviceToHost));
  if (p.slabs_out && path >= 1 && rc > 0) HIPC(hipMemcpy(p.slabs_out, d_slabs, (size_t)rc * slab_stride * 4, hipMemcpyDeviceToHost));
  if (p.split_out) *p.split_out = rc;
  if (p.packed_out && mm) HIPC(hipMemcpy(p.packed_out, d_w, wbytes, hipMemcpyDeviceToHost));
  if (act != 2) {
    if (p.xq_out) HIPC(hipMemcpy(p.xq_out, d_xq, xq_bytes, hipMemcpyDeviceToHost));
    if (p.xd_out) HIPC(hipMemcpy(p.xd_out, d_xd, xd_bytes, hipMemcpyDeviceToHost));
    if (p.xb_out) HIPC(hipMemcpy(p.xb_out, d_xb, xb_bytes, hipMemcpyDeviceToHost));
  }
  if (d_nxq) {
    if (p.nxq_out) HIPC(hipMemcpy(p.nxq_out, d_nxq, (size_t)qrows * N, hipMemcpyDeviceToHost));
    if (p.nxd_out) HIPC(hipMemcpy(p.nxd_out, d_nxd, (size_t)qrows * (N / 256) * 4, hipMemcpyDeviceToHost));
    if (p.nxb_out) HIPC(hipMemcpy(p.nxb_out, d_nxb, (size_t)qrows * (N / 32) * 4, hipMemcpyDeviceToHost));
  }
  return mm && epi == EPI_QKV ? qkv.download(p) : 0;
}

int mx_kq_side_probe(int device, const mx_kq_side_args* pa) {
  if (!pa) return fail(MX_ERR_ARG, "mx_kq_side_probe: null arguments");
  const mx_kq_side_args& p = *pa;
  const int mode = p.mode, N = p.N, K = p.K, M = p.M;
  if (mode < 0 || mode > 4) return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 0..4");
  if (K < 256 || K % 256 || K > 32768) return fail(MX_ERR_ARG, "mx_kq_side_probe: K a multiple of 256, <= 32768");
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs dev;
  const int SB = K / 256;
  if (mode <= 2) {
    if (!p.blocks || !p.out || N < 1 || N > (1 << 18) || (size_t)N * K > ((size_t)1 << 28))
      return fail(MX_ERR_ARG, "mx_kq_side_probe: blocks and out required, 1 <= N <= 2^18, N*K <= 2^28");
    uint8_t *d_src = nullptr, *d_w = nullptr, *d_out = nullptr;
    if (mode == 0) {  // launch_pack_kq alone
      const int bb = kq_block_bytes(p.type);
      if (!bb || N % TILE_N || p.pack < PACK_ROWS || p.pack > PACK_UP || p.offset < 0 || p.offset % TILE_N ||
          p.offset > (1 << 18) || (p.pack != PACK_ROWS && p.offset))
        return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 0: type 12 / 13 / 14, N % 16, pack 0..2, offset % 16 (pack 0 only)");
      const int rows = p.pack == PACK_ROWS ? N + p.offset : 2 * N;
      const size_t raw = (size_t)N * SB * bb, wb = kq_matrix_bytes(p.type, rows, K);
      const size_t ob = wb + (size_t)PROBE_GUARD_ROWS * kq_tile_bytes(p.type);
      if (!dev.alloc(&d_src, raw) || !dev.alloc_ff(&d_w, ob)) return fail(MX_ERR_HIP, "mx_kq_side_probe: device allocation");
      HIPC(hipMemcpy(d_src, p.blocks, raw, hipMemcpyHostToDevice));
      if (launch_pack_kq(d_w, d_src, p.type, N, K, p.pack, p.offset, nullptr)) {
        hipDeviceSynchronize();
        return fail(MX_ERR_ARG, "mx_kq_side_probe: launch_pack_kq refused the shape");
      }
      HIPC(hipGetLastError());
      HIPC(hipDeviceSynchronize());
      HIPC(hipMemcpy(p.out, d_w, ob, hipMemcpyDeviceToHost));
      return 0;
    }
    if (mode == 1) {  // packed K-quant tiles -> packed bf16 tiles
      if (!kq_segments_ok(p.kq_n, p.kq_type, p.kq_tile_end, N))
        return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 1: 1..3 segments of type 12 / 13 / 14, tile ends increasing to N / 16");
      size_t raw = 0, wb = 0, raw_off[3], w_off[3];
      int rows[3], type[3], tile_end[3];
      for (int i = 0; i < p.kq_n; i++) {
        rows[i] = (p.kq_tile_end[i] - (i ? p.kq_tile_end[i - 1] : 0)) * TILE_N;
        type[i] = p.kq_type[i], tile_end[i] = p.kq_tile_end[i];
        raw_off[i] = raw, w_off[i] = wb;
        raw += (size_t)rows[i] * SB * kq_block_bytes(type[i]);
        wb += kq_matrix_bytes(type[i], rows[i], K);
      }
      const size_t ob = (size_t)(N + PROBE_GUARD_ROWS) * K * 2;
      if (!dev.alloc(&d_src, raw) || !dev.alloc_ff(&d_w, wb) || !dev.alloc_ff(&d_out, ob))
        return fail(MX_ERR_HIP, "mx_kq_side_probe: device allocation");
      HIPC(hipMemcpy(d_src, p.blocks, raw, hipMemcpyHostToDevice));
      int rc = 0;
      for (int i = 0; i < p.kq_n && !rc; i++)
        rc = launch_pack_kq(d_w + w_off[i], d_src + raw_off[i], type[i], rows[i], K, PACK_ROWS, 0, nullptr);
      if (!rc) rc = launch_dequant_kq((uint16_t*)d_out, d_w, K, p.kq_n, type, tile_end, w_off, nullptr);
      if (rc) {
        hipDeviceSynchronize();
        return fail(MX_ERR_ARG, "mx_kq_side_probe: launch_pack_kq / launch_dequant_kq refused the shape");
      }
      HIPC(hipGetLastError());
      HIPC(hipDeviceSynchronize());
      HIPC(hipMemcpy(p.out, d_out, ob, hipMemcpyDeviceToHost));
      return 0;
    }
    const int bb = kq_block_bytes(p.type);  // mode 2: GET_ROWS
    if (!bb || !p.ids || M < 1 || M > PREFILL_ROWS)
      return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 2: type 12 / 13 / 14, ids [M], 1 <= M <= PREFILL_ROWS");
    for (int i = 0; i < M; i++)
      if (p.ids[i] < 0 || p.ids[i] >= N) return fail(MX_ERR_ARG, "mx_kq_side_probe: id out of range");
    float* d_ssq = nullptr;
    int* d_ids = nullptr;
    const size_t raw = (size_t)N * SB * bb;
    const size_t ob = (size_t)(M + PROBE_GUARD_ROWS) * K * 4, sb = (size_t)(M + PROBE_GUARD_ROWS) * (K / 16) * 4;
    if (!dev.alloc(&d_src, raw) || !dev.alloc_ff(&d_out, ob) || !dev.alloc(&d_ids, (size_t)M * 4) ||
        (p.ssq_out && !dev.alloc_ff(&d_ssq, sb)))
      return fail(MX_ERR_HIP, "mx_kq_side_probe: device allocation");
    HIPC(hipMemcpy(d_src, p.blocks, raw, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_ids, p.ids, (size_t)M * 4, hipMemcpyHostToDevice));
    if (launch_embed_kq((float*)d_out, d_src, p.type, d_ids, M, K, d_ssq, nullptr)) {
      hipDeviceSynchronize();
      return fail(MX_ERR_ARG, "mx_kq_side_probe: launch_embed_kq refused the shape");
    }
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(p.out, d_out, ob, hipMemcpyDeviceToHost));
    if (p.ssq_out) HIPC(hipMemcpy(p.ssq_out, d_ssq, sb, hipMemcpyDeviceToHost));
    return 0;
  }
  // modes 3 / 4: the Q8_K quantiser on f32 rows
  const bool norm = mode == 4;
  const int ld = norm ? K : (p.ld ? p.ld : K);
  const int rows = norm ? (p.rows ? p.rows : M) : M;
  if (!p.x || !p.xq_out || !p.xd_out || !p.xb_out || M < 1 || M > PREFILL_ROWS || rows < 1 || rows > PREFILL_ROWS)
    return fail(MX_ERR_ARG, "mx_kq_side_probe: modes 3 / 4: x and xq / xd / xb outputs, 1 <= M, rows <= PREFILL_ROWS");
  if (ld < K || ld % 4 || ld > 65536 || (norm && p.ld && p.ld != K))
    return fail(MX_ERR_ARG, "mx_kq_side_probe: K <= ld <= 65536, ld % 4 == 0 (mode 4: ld = K)");
  if (!norm && (p.w || p.row_map || p.nslab || p.slabs)) return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 3 takes no w / row_map / slabs");
  if (norm) {
    if (!p.w || p.nslab < 0 || p.nslab > 8 || (p.nslab > 0) != (p.slabs != nullptr))
      return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 4: w [K], nslab 0..8 with slabs");
    if (p.row_map) {
      for (int i = 0; i < M; i++)
        if (p.row_map[i] < 0 || p.row_map[i] >= rows) return fail(MX_ERR_ARG, "mx_kq_side_probe: row_map entry out of range");
    } else if (rows != M) {
      return fail(MX_ERR_ARG, "mx_kq_side_probe: mode 4 without row_map: rows = M");
    }
  }
  float *d_x = nullptr, *d_w = nullptr, *d_slabs = nullptr, *d_xd = nullptr, *d_xb = nullptr;
  int8_t* d_xq = nullptr;
  int* d_map = nullptr;
  const int qrows = M + PROBE_GUARD_ROWS;
  const size_t x_bytes = (size_t)(rows + PROBE_GUARD_ROWS) * ld * 4, stride = (size_t)rows * K;
  const size_t xq_bytes = (size_t)qrows * K, xd_bytes = (size_t)qrows * SB * 4, xb_bytes = (size_t)qrows * (K / 32) * 4;
  if (!dev.alloc_ff(&d_x, x_bytes) || !dev.alloc_ff(&d_xq, xq_bytes) || !dev.alloc_ff(&d_xd, xd_bytes) ||
      !dev.alloc_ff(&d_xb, xb_bytes) ||
      (norm && !dev.alloc(&d_w, (size_t)K * 4)) || (p.row_map && !dev.alloc(&d_map, (size_t)M * 4)) ||
      (p.nslab && !dev.alloc(&d_slabs, stride * p.nslab * 4)))
    return fail(MX_ERR_HIP, "mx_kq_side_probe: device allocation");
  HIPC(hipMemcpy(d_x, p.x, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
  if (norm) HIPC(hipMemcpy(d_w, p.w, (size_t)K * 4, hipMemcpyHostToDevice));
  if (p.row_map) HIPC(hipMemcpy(d_map, p.row_map, (size_t)M * 4, hipMemcpyHostToDevice));
  if (p.nslab) HIPC(hipMemcpy(d_slabs, p.slabs, stride * p.nslab * 4, hipMemcpyHostToDevice));
  const int rc = norm ? launch_rmsnorm_q8k(d_xq, d_xd, d_xb, d_x, d_w, d_map, M, K, p.eps, nullptr, d_slabs, p.nslab, stride)
                      : launch_quantize_q8k(d_xq, d_xd, d_xb, d_x, ld, M, K, nullptr);
  if (rc) {
    hipDeviceSynchronize();
    return fail(MX_ERR_ARG, std::string("mx_kq_side_probe: ") + (norm ? "launch_rmsnorm_q8k" : "launch_quantize_q8k") +
                                " refused the shape");
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(p.xq_out, d_xq, xq_bytes, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.xd_out, d_xd, xd_bytes, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.xb_out, d_xb, xb_bytes, hipMemcpyDeviceToHost));
  if (p.x_out) HIPC(hipMemcpy(p.x_out, d_x, x_bytes, hipMemcpyDeviceToHost));
  return 0;
}

int mx_glue_probe(int device, const mx_glue_args* pa) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  if (!pa) return fail(MX_ERR_ARG, "mx_glue_probe: null arguments");
  const mx_glue_args& p = *pa;
  const int mode = p.mode, M = p.M, n = p.n;
  if (mode < 0 || mode > 7) return fail(MX_ERR_ARG, "mx_glue_probe: mode 0..7");
  if (mode == 0 || mode == 5 || mode == 6) {  // flat: count elements of src -> out [count + 4096]
    const size_t cnt = p.count, esz = mode == 6 ? 4 : 2;
    if (!p.src || !p.out || cnt < 1 || cnt > ((size_t)1 << 30))
      return fail(MX_ERR_ARG, "mx_glue_probe: flat modes: src and out required, 1 <= count <= 2^30");
    size_t sbytes = cnt * 4;
    if (mode == 0) {
      const int be = ggml_block_elems(p.type);
      sbytes = p.src_bytes;
      if (sbytes < 1 || sbytes > ((size_t)1 << 32)) return fail(MX_ERR_ARG, "mx_glue_probe: mode 0: 1 <= src_bytes <= 2^32");
      if (be && cnt % be == 0 && sbytes < cnt / be * glue_block_bytes(p.type))
        return fail(MX_ERR_ARG, "mx_glue_probe: mode 0: src_bytes is less than count elements of this type");
    } else if (cnt % 4) {
      return fail(MX_ERR_ARG, "mx_glue_probe: modes 5 / 6: count a multiple of 4");
    }
    if (device >= 0) HIPC(hipSetDevice(device));
    DevBufs dev;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    const size_t ob = (cnt + GLUE_GUARD_FLAT) * esz;
    if (!dev.alloc(&d_src, sbytes) || !dev.alloc_ff(&d_out, ob)) return fail(MX_ERR_HIP, "mx_glue_probe: device allocation");
    HIPC(hipMemcpy(d_src, p.src, sbytes, hipMemcpyHostToDevice));
    HIPC(hipDeviceSynchronize());
    if (mode == 0) {
      if (launch_dequant_bf16((uint16_t*)d_out, d_src, p.type, cnt, nullptr)) {
        hipDeviceSynchronize();
        return fail(MX_ERR_ARG, "mx_glue_probe: launch_dequant_bf16 refused the type or the count");
      }
    } else if (mode == 5) {
      launch_f32_to_bf16((uint16_t*)d_out, (const float*)d_src, cnt, nullptr);
    } else {
      launch_copy_f32((float*)d_out, (const float*)d_src, cnt, nullptr);
    }
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(p.out, d_out, ob, hipMemcpyDeviceToHost));
    return 0;
  }
  if (mode <= 4) {  // rows of the residual stream: x [M + 64][n], ssq [M + 64][n / 16]
    const bool has_x = mode != 2;
    if (n < 64 || n % 64 || n > 16384) return fail(MX_ERR_ARG, "mx_glue_probe: modes 1..4: n a multiple of 64, <= 16384");
    if (M < 1 || M > PREFILL_ROWS) return fail(MX_ERR_ARG, "mx_glue_probe: modes 1..4: 1 <= M <= 4096");
    if (!p.src || (has_x && !p.out) || (mode == 2 && !p.ssq_out))
      return fail(MX_ERR_ARG, "mx_glue_probe: modes 1..4: src required, out (not mode 2), ssq_out (mode 2)");
    int srows = M;
    if (mode == 1) {
      srows = p.N;
      if (!p.ids || srows < 1 || srows > (1 << 18)) return fail(MX_ERR_ARG, "mx_glue_probe: mode 1: ids [M], 1 <= N <= 2^18");
      for (int i = 0; i < M; i++)
        if (p.ids[i] < 0 || p.ids[i] >= srows) return fail(MX_ERR_ARG, "mx_glue_probe: id out of range");
    }
    if (device >= 0) HIPC(hipSetDevice(device));
    DevBufs dev;
    uint8_t* d_src = nullptr;
    float *d_x = nullptr, *d_ssq = nullptr;
    int* d_ids = nullptr;
    const size_t sbytes = (size_t)srows * n * ((mode == 1 || mode == 4) ? 2 : 4);
    const size_t xb = (size_t)(M + PROBE_GUARD_ROWS) * n * 4, qb = (size_t)(M + PROBE_GUARD_ROWS) * (n / 16) * 4;
    if (!dev.alloc(&d_src, sbytes) || (has_x && !dev.alloc_ff(&d_x, xb)) || (p.ssq_out && !dev.alloc_ff(&d_ssq, qb)) ||
        (mode == 1 && !dev.alloc(&d_ids, (size_t)M * 4)))
      return fail(MX_ERR_HIP, "mx_glue_probe: device allocation");
    HIPC(hipMemcpy(d_src, p.src, sbytes, hipMemcpyHostToDevice));
    if (d_ids) HIPC(hipMemcpy(d_ids, p.ids, (size_t)M * 4, hipMemcpyHostToDevice));
    HIPC(hipDeviceSynchronize());
    // ssq_out with want_ssq 0: the launcher gets NULL and the buffer returns as it was filled
    float* ssq_arg = p.want_ssq ? d_ssq : nullptr;
    if (mode == 1) launch_embed(d_x, (const uint16_t*)d_src, d_ids, M, n, ssq_arg, nullptr);
    else if (mode == 2) launch_ssq((const float*)d_src, M, n, d_ssq, nullptr);
    else if (mode == 3) launch_f32_in(d_x, (const float*)d_src, M, n, ssq_arg, nullptr);
    else launch_bf16_to_f32(d_x, (const uint16_t*)d_src, M, n, ssq_arg, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    if (has_x) HIPC(hipMemcpy(p.out, d_x, xb, hipMemcpyDeviceToHost));
    if (p.ssq_out) HIPC(hipMemcpy(p.ssq_out, d_ssq, qb, hipMemcpyDeviceToHost));
    return 0;
  }
  // mode 7: launch_argmax.  tok / ids_next / pos_next / hist_count [M + 4096], hist [M + 64][hist_stride]
  const int V = p.V, ldl = p.ldl, hs = p.hist_stride, mh = p.max_hist;
  if (M < 1 || M > PREFILL_ROWS || V < 1 || ldl < V || ldl > (1 << 20) || (size_t)M * ldl > ((size_t)1 << 27))
    return fail(MX_ERR_ARG, "mx_glue_probe: mode 7: 1 <= M <= 4096, 1 <= V <= ldl <= 2^20, M * ldl <= 2^27");
  if (!p.src || !p.pos || !p.hist_count || !p.tok_out || !p.ids_next_out || !p.pos_next_out || !p.hist_out || !p.hist_count_out)
    return fail(MX_ERR_ARG, "mx_glue_probe: mode 7: logits, pos, hist_count and the five outputs are required");
  if (hs < 1 || hs > 4096 || mh < 0 || mh > hs) return fail(MX_ERR_ARG, "mx_glue_probe: mode 7: 0 <= max_hist <= hist_stride <= 4096");
  for (int i = 0; i < M; i++)
    if (p.hist_count[i] < 0) return fail(MX_ERR_ARG, "mx_glue_probe: mode 7: negative hist_count");
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs dev;
  float *d_lg = nullptr, *d_wv = nullptr;
  int *d_wi = nullptr, *d_tok = nullptr, *d_ids = nullptr, *d_pos = nullptr, *d_hist = nullptr, *d_hc = nullptr;
  const size_t lb = (size_t)M * ldl * 4, fb = ((size_t)M + GLUE_GUARD_FLAT) * 4, wsb = (size_t)M * 64 * 4;
  const size_t hb = (size_t)(M + PROBE_GUARD_ROWS) * hs * 4;
  if (!dev.alloc(&d_lg, lb) || !dev.alloc_ff(&d_wv, wsb) || !dev.alloc_ff(&d_wi, wsb) || !dev.alloc_ff(&d_tok, fb) ||
      !dev.alloc_ff(&d_ids, fb) || !dev.alloc_ff(&d_pos, fb) || !dev.alloc_ff(&d_hc, fb) || !dev.alloc_ff(&d_hist, hb))
    return fail(MX_ERR_HIP, "mx_glue_probe: device allocation");
  HIPC(hipMemcpy(d_lg, p.src, lb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_pos, p.pos, (size_t)M * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_hc, p.hist_count, (size_t)M * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  launch_argmax(d_lg, ldl, M, V, d_wv, d_wi, (p.null_mask & 1) ? nullptr : d_tok, (p.null_mask & 2) ? nullptr : d_ids,
                (p.null_mask & 4) ? nullptr : d_pos, (p.null_mask & 8) ? nullptr : d_hist, hs, d_hc, mh, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(p.tok_out, d_tok, fb, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.ids_next_out, d_ids, fb, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.pos_next_out, d_pos, fb, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.hist_count_out, d_hc, fb, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(p.hist_out, d_hist, hb, hipMemcpyDeviceToHost));
  return 0;
}

int mx_draft_probe(int device, int R, const int32_t* tokens, int stride, const int32_t* lens, int D, int ngram,
                   const int32_t* pos0, const int32_t* slot0, int32_t* ids, int32_t* pos, int32_t* slot,
                   int32_t* n_draft) {
  if (!tokens || !lens || !pos0 || !slot0 || !ids || !pos || !slot || !n_draft || R < 1 || R > SPEC_MAX_REQ || D < 1 ||
      D > SPEC_MAX_DRAFT || R * (1 + D) > SPEC_ROWS || ngram < 1 || stride < 1 || stride > (1 << 20))
    return fail(MX_ERR_ARG, "mx_draft_probe: R 1..8, D 1..15, R (1 + D) <= 16, ngram >= 1, 1 <= stride <= 2^20");
  for (int r = 0; r < R; r++)
    if (lens[r] < 1 || lens[r] > stride || pos0[r] < 0 || pos0[r] > (1 << 30) - 1 - D || slot0[r] < 0)
      return fail(MX_ERR_ARG, "mx_draft_probe: 1 <= lens[r] <= stride, 0 <= pos0[r] < 2^30 - D, slot0[r] >= 0");
  if (device >= 0) HIPC(hipSetDevice(device));
  const int M = R * (1 + D);
  DevBufs bufs;
  int *d_tok, *d_len, *d_par, *d_i, *d_p, *d_s, *d_nd;
  if (!bufs.alloc(&d_tok, (size_t)R * stride * 4) || !bufs.alloc(&d_len, R * 4) || !bufs.alloc(&d_par, R * 2 * 4) ||
      !bufs.alloc_ff(&d_i, M * 4) || !bufs.alloc(&d_p, M * 4) || !bufs.alloc(&d_s, M * 4) || !bufs.alloc_ff(&d_nd, R * 4))
    return fail(MX_ERR_HIP, "mx_draft_probe: device allocation");
  std::vector<int32_t> par(2 * R), hp(M, -1), hs(M, -1);
  for (int r = 0; r < R; r++) {
    par[2 * r] = D, par[2 * r + 1] = ngram;
    hp[r * (1 + D)] = pos0[r], hs[r * (1 + D)] = slot0[r];
  }
  HIPC(hipMemcpy(d_tok, tokens, (size_t)R * stride * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_len, lens, R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_par, par.data(), R * 2 * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_p, hp.data(), M * 4, hipMemcpyHostToDevice));  // -1 = 0xFF bytes but for each row 0
  HIPC(hipMemcpy(d_s, hs.data(), M * 4, hipMemcpyHostToDevice));
  launch_spec_draft(d_tok, stride, d_len, d_par, R, D, d_i, d_p, d_s, d_nd, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(ids, d_i, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(pos, d_p, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(slot, d_s, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(n_draft, d_nd, R * 4, hipMemcpyDeviceToHost));
  return 0;
}

int mx_accept_probe(int device, int R, int D, int V, const float* logits, const int32_t* draft, const int32_t* n_draft,
                    const int32_t* pos0, int32_t* a, int32_t* emitted, int32_t* next_id, int32_t* new_pos,
                    int32_t* counts) {
  if (!logits || !draft || !n_draft || !pos0 || !a || !emitted || !next_id || !new_pos || !counts || R < 1 ||
      R > SPEC_MAX_REQ || D < 1 || D > SPEC_MAX_DRAFT || R * (1 + D) > SPEC_ROWS || V < 1 || V > (1 << 20))
    return fail(MX_ERR_ARG, "mx_accept_probe: R 1..8, D 1..15, R (1 + D) <= 16, 1 <= V <= 2^20");
  for (int r = 0; r < R; r++) {
    if (n_draft[r] < 0 || n_draft[r] > D || pos0[r] < 0 || pos0[r] > (1 << 30))
      return fail(MX_ERR_ARG, "mx_accept_probe: 0 <= n_draft[r] <= D, 0 <= pos0[r] <= 2^30");
    for (int j = 0; j < D; j++)
      if (draft[r * D + j] < 0 || draft[r * D + j] >= V) return fail(MX_ERR_ARG, "mx_accept_probe: draft id out of range");
  }
  if (device >= 0) HIPC(hipSetDevice(device));
  const int M = R * (1 + D), CS = 1 + D;  // the sequence buffer: one token already there, room for 1 + D more
  DevBufs bufs;
  float *d_lg, *d_wv;
  int *d_wi, *d_i, *d_p, *d_nd, *d_ctx, *d_len, *d_h, *d_hc, *d_cnt;
  if (!bufs.alloc(&d_lg, (size_t)M * V * 4) || !bufs.alloc(&d_wv, M * 64 * 4) || !bufs.alloc(&d_wi, M * 64 * 4) ||
      !bufs.alloc(&d_i, M * 4) || !bufs.alloc(&d_p, M * 4) || !bufs.alloc(&d_nd, R * 4) ||
      !bufs.alloc_ff(&d_ctx, (size_t)R * (CS + 1) * 4) || !bufs.alloc(&d_len, R * 4) || !bufs.alloc_ff(&d_h, M * 4) ||
      !bufs.alloc(&d_hc, R * 4) || !bufs.alloc(&d_cnt, R * 3 * 4))
    return fail(MX_ERR_HIP, "mx_accept_probe: device allocation");
  std::vector<int32_t> hi(M, -1), hp(M, -1), one(R, 1);
  for (int r = 0; r < R; r++) {
    hp[r * (1 + D)] = pos0[r];
    for (int j = 0; j < D; j++) hi[r * (1 + D) + 1 + j] = draft[r * D + j];
  }
  HIPC(hipMemcpy(d_lg, logits, (size_t)M * V * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_i, hi.data(), M * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_p, hp.data(), M * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_nd, n_draft, R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_len, one.data(), R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemset(d_hc, 0, R * 4));
  HIPC(hipMemset(d_cnt, 0, R * 3 * 4));
  launch_argmax_stage1(d_lg, V, M, V, d_wv, d_wi, nullptr);
  launch_spec_accept(d_wv, d_wi, R, D, d_i, d_p, d_nd, d_ctx, CS + 1, d_len, d_h, CS, d_hc, d_cnt, nullptr, 0, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  std::vector<int32_t> oi(M), op(M), ctx((size_t)R * (CS + 1)), hc(R);
  HIPC(hipMemcpy(oi.data(), d_i, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(op.data(), d_p, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(ctx.data(), d_ctx, ctx.size() * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(hc.data(), d_hc, R * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(emitted, d_h, M * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(counts, d_cnt, R * 3 * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < R; r++) {
    a[r] = hc[r] - 1;
    next_id[r] = oi[r * (1 + D)];
    new_pos[r] = op[r * (1 + D)];
    // the copy appended to the sequence must be the history's
    for (int j = 0; j < CS; j++)
      if (ctx[(size_t)r * (CS + 1) + 1 + j] != emitted[r * CS + j])
        return fail(MX_ERR_STATE, "mx_accept_probe: sequence and history disagree");
  }
  return 0;
}

int mx_pool_probe(int device, int rows, int n, const float* x, const float* w, float eps, int n_seq,
                  const int32_t* seq_begin, int chunk_rows, int pooling, int normalize, float* out) {
  // every index a kernel forms from these arguments is checked here: nothing is launched on a bad one
  constexpr int MAXR = 32768;
  if (!x || !w || !seq_begin || !out || rows < 1 || rows > MAXR || n < 64 || n % 64 || n > 16384 ||
      (size_t)rows * n > ((size_t)1 << 26))
    return fail(MX_ERR_ARG, "mx_pool_probe: 1 <= rows <= 32768, n a multiple of 64 in [64, 16384], rows * n <= 2^26, "
                            "non-null buffers");
  if (pooling < MX_POOL_NONE || pooling > MX_POOL_LAST || chunk_rows < 0 || chunk_rows % 16)
    return fail(MX_ERR_ARG, "mx_pool_probe: pooling 0..3, chunk_rows a multiple of 16 (0: one chunk)");
  if (n_seq < 1 || n_seq > rows || seq_begin[0] != 0 || seq_begin[n_seq] != rows)
    return fail(MX_ERR_ARG, "mx_pool_probe: seq_begin [n_seq + 1] must start at 0 and end at rows");
  for (int q = 0; q < n_seq; q++)
    if (seq_begin[q + 1] <= seq_begin[q]) return fail(MX_ERR_ARG, "mx_pool_probe: seq_begin must increase");
  if (device >= 0) HIPC(hipSetDevice(device));
  const int chunk = chunk_rows ? std::min(chunk_rows, rows) : rows;
  const size_t N = n, out_rows = (size_t)(pooling == MX_POOL_NONE ? rows : n_seq) + PROBE_GUARD_ROWS;
  const size_t tab_cap = embd_tab_ints(chunk, chunk);
  DevBufs bufs;
  float *d_x, *d_w, *d_y, *d_acc, *d_out;
  int* d_tab;
  if (!bufs.alloc(&d_x, (size_t)rows * N * 4) || !bufs.alloc(&d_w, N * 4) || !bufs.alloc_ff(&d_y, (size_t)chunk * N * 4) ||
      !bufs.alloc_ff(&d_acc, (size_t)n_seq * N * 4) || !bufs.alloc_ff(&d_out, out_rows * N * 4) ||
      !bufs.alloc(&d_tab, tab_cap * 4))
    return fail(MX_ERR_HIP, "mx_pool_probe: device allocation");
  HIPC(hipMemcpy(d_x, x, (size_t)rows * N * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_w, w, N * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  std::vector<int32_t> tab;
  for (int c0 = 0; c0 < rows; c0 += chunk) {
    const int c1 = std::min(rows, c0 + chunk);
    std::vector<EmbdSeg> segs;
    for (int q = 0; q < n_seq; q++) {
      const int a = std::max(seq_begin[q], c0), b = std::min(seq_begin[q + 1], c1);
      if (a < b)
        segs.push_back({a - c0, b - a, q, a - seq_begin[q], seq_begin[q + 1] - seq_begin[q],
                        pooling == MX_POOL_NONE ? a : q});
    }
    // MX_POOL_NONE: the rows go straight to their place in out; MEAN: to the chunk's scratch, as in the engine
    const int rc = embd_tail(d_x + (size_t)c0 * N, d_w, eps, n, segs, pooling, normalize != 0,
                             pooling == MX_POOL_NONE ? d_out : d_y, d_acc, d_out, d_tab, tab_cap, tab, nullptr);
    const hipError_t se = hipDeviceSynchronize();  // tab is reused by the next chunk
    if (rc) return rc;
    HIPC(se);
  }
  HIPC(hipMemcpy(out, d_out, out_rows * N * 4, hipMemcpyDeviceToHost));
  return 0;
}

int mx_kv_copy_probe(int device, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx, int n_copies,
                     const mx_kv_copy* copies, void* kcache, void* vcache) {
  // every index the kernel forms is checked before anything is launched: the geometry here, the table below
  if (!copies || !kcache || !vcache) return fail(MX_ERR_ARG, "mx_kv_copy_probe: non-null copies / caches");
  if (n_layer < 1 || n_layer > 256 || n_slots < 1 || n_slots > 4096 || n_head_kv < 1 || n_head_kv > 64 ||
      (head_dim != 64 && head_dim != 128) || n_ctx < 1 || n_ctx > (1 << 20))
    return fail(MX_ERR_ARG, "mx_kv_copy_probe: n_layer 1..256, n_slots 1..4096, n_head_kv 1..64, head_dim 64 or 128, "
                            "n_ctx 1..2^20");
  if (n_copies < 1 || n_copies > n_slots) return fail(MX_ERR_ARG, "mx_kv_copy_probe: 1 <= n_copies <= n_slots");
  KvGeom g;
  if (int rc = g.set("mx_kv_copy_probe", n_head_kv, head_dim, n_ctx, n_slots, n_layer)) return rc;
  const size_t cache_elems = g.cache_elems;
  // the table itself is the launcher's to judge (the scheduler relies on the same refusals): it checks the host
  // copy and launches nothing on a bad entry
  std::vector<KvCopy> tab(n_copies);
  for (int i = 0; i < n_copies; i++) tab[i] = {copies[i].src_slot, copies[i].dst_slot, copies[i].n_pos};
  if (device >= 0) HIPC(hipSetDevice(device));
  DevBufs bufs;
  _Float16 *d_k = nullptr, *d_v = nullptr;
  KvCopy* d_tab = nullptr;
  if (!bufs.alloc(&d_k, cache_elems * 2) || !bufs.alloc(&d_v, cache_elems * 2) ||
      !bufs.alloc(&d_tab, tab.size() * sizeof(KvCopy)))
    return fail(MX_ERR_HIP, "mx_kv_copy_probe: device allocation");
  HIPC(hipMemcpy(d_k, kcache, cache_elems * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_v, vcache, cache_elems * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(KvCopy), hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  if (launch_kv_copy(d_k, d_v, tab.data(), d_tab, n_copies, n_layer, n_slots, n_head_kv, head_dim, n_ctx, g.ctx_stride,
                     g.slot_stride, g.layer_kv_stride, nullptr))
    return fail(MX_ERR_ARG, "mx_kv_copy_probe: launch_kv_copy refused the table (a slot out of range, src == dst, n_pos "
                            "outside [1, n_ctx], a slot a destination twice or both a source and a destination)");
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(kcache, d_k, cache_elems * 2, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(vcache, d_v, cache_elems * 2, hipMemcpyDeviceToHost));
  return 0;
}

int mx_kv_pack_probe(int device, int dir, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                     int n_entries, const mx_kv_pack* entries, void* kcache, void* vcache, void* packed,
                     uint64_t packed_bytes) {
  // as mx_kv_copy_probe: the geometry is checked here, the table by the launchers, before anything is launched
  if (!entries || !kcache || !vcache || !packed)
    return fail(MX_ERR_ARG, "mx_kv_pack_probe: non-null entries / caches / packed");
  if (dir != 0 && dir != 1) return fail(MX_ERR_ARG, "mx_kv_pack_probe: dir 0 (pack) or 1 (unpack)");
  if (n_layer < 1 || n_layer > 256 || n_slots < 1 || n_slots > 4096 || n_head_kv < 1 || n_head_kv > 64 ||
      (head_dim != 64 && head_dim != 128) || n_ctx < 1 || n_ctx > (1 << 20))
    return fail(MX_ERR_ARG, "mx_kv_pack_probe: n_layer 1..256, n_slots 1..4096, n_head_kv 1..64, head_dim 64 or 128, "
                            "n_ctx 1..2^20");
  if (n_entries < 1 || n_entries > 4096) return fail(MX_ERR_ARG, "mx_kv_pack_probe: 1 <= n_entries <= 4096");
  if (packed_bytes < 16 || packed_bytes % 16 || packed_bytes > ((uint64_t)1 << 30))
    return fail(MX_ERR_ARG, "mx_kv_pack_probe: packed_bytes a multiple of 16, 16..2^30");
  KvGeom g;
  if (int rc = g.set("mx_kv_pack_probe", n_head_kv, head_dim, n_ctx, n_slots, n_layer)) return rc;
  const size_t cache_elems = g.cache_elems;
  std::vector<KvPack> tab(n_entries);
  for (int i = 0; i < n_entries; i++) {
    if (entries[i].offset16 > ((uint64_t)1 << 40)) return fail(MX_ERR_ARG, "mx_kv_pack_probe: an offset past the buffer");
    tab[i] = {entries[i].slot, entries[i].n_pos, (int64_t)entries[i].offset16};
  }
  if (device >= 0) HIPC(hipSetDevice(device));
  const size_t guard = dir == 0 ? MX_KV_PACK_GUARD_BYTES : 0;
  DevBufs bufs;
  _Float16 *d_k = nullptr, *d_v = nullptr;
  char* d_p = nullptr;
  KvPack* d_tab = nullptr;
  if (!bufs.alloc(&d_k, cache_elems * 2) || !bufs.alloc(&d_v, cache_elems * 2) ||
      !bufs.alloc(&d_p, packed_bytes + guard) || !bufs.alloc(&d_tab, tab.size() * sizeof(KvPack)))
    return fail(MX_ERR_HIP, "mx_kv_pack_probe: device allocation");
  HIPC(hipMemcpy(d_k, kcache, cache_elems * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_v, vcache, cache_elems * 2, hipMemcpyHostToDevice));
  if (dir == 0) HIPC(hipMemset(d_p, 0xFF, packed_bytes + guard));
  else HIPC(hipMemcpy(d_p, packed, packed_bytes, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(KvPack), hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  const int rc = dir == 0 ? launch_kv_pack(d_k, d_v, d_p, packed_bytes, tab.data(), d_tab, n_entries, n_layer, n_slots,
                                           n_head_kv, head_dim, n_ctx, g.ctx_stride, g.slot_stride, g.layer_kv_stride,
                                           nullptr)
                          : launch_kv_unpack(d_k, d_v, d_p, packed_bytes, tab.data(), d_tab, n_entries, n_layer,
                                             n_slots, n_head_kv, head_dim, n_ctx, g.ctx_stride, g.slot_stride,
                                             g.layer_kv_stride, nullptr);
  if (rc)
    return fail(MX_ERR_ARG, "mx_kv_pack_probe: the launcher refused the table (a slot out of range, n_pos outside "
                            "[1, n_ctx], an offset off a tile, an entry past the buffer, overlapping packed ranges or a "
                            "slot a destination twice)");
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(kcache, d_k, cache_elems * 2, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(vcache, d_v, cache_elems * 2, hipMemcpyDeviceToHost));
  if (dir == 0) HIPC(hipMemcpy(packed, d_p, packed_bytes + guard, hipMemcpyDeviceToHost));
  return 0;
}

int mx_lora_merge_probe(int device, int rows, int cols, int r, const uint16_t* w, const float* A, const float* B,
                        float scale, uint16_t* out, int iters, double* us_per_launch) {
  if (!w || !A || !B || !out || rows < 1 || rows > 65536 || cols < 1 || cols > 65536 ||
      (size_t)rows * cols > ((size_t)1 << 28) || r < 1 || r > 4096 || !std::isfinite(scale) || iters < 0 ||
      (iters > 0 && !us_per_launch))
    return fail(MX_ERR_ARG, "mx_lora_merge_probe: rows, cols 1..65536, rows * cols <= 2^28, r 1..4096, a finite "
                            "scale, iters >= 0 with us_per_launch");
  if (device >= 0) HIPC(hipSetDevice(device));
  const size_t n = (size_t)rows * cols;
  DevBufs dev;
  uint16_t* d_w = nullptr;
  float *d_a = nullptr, *d_b = nullptr;
  if (!dev.alloc_ff(&d_w, (n + GLUE_GUARD_FLAT) * 2) || !dev.alloc(&d_a, (size_t)r * cols * 4) ||
      !dev.alloc(&d_b, (size_t)rows * r * 4))
    return fail(MX_ERR_HIP, "mx_lora_merge_probe: device allocation");
  HIPC(hipMemcpy(d_w, w, n * 2, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_a, A, (size_t)r * cols * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_b, B, (size_t)rows * r * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  if (launch_lora_merge(d_w, d_a, d_b, rows, cols, r, scale, nullptr))
    return fail(MX_ERR_ARG, "mx_lora_merge_probe: launch_lora_merge refused");
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(out, d_w, (n + GLUE_GUARD_FLAT) * 2, hipMemcpyDeviceToHost));
  if (iters > 0) {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipError_t err = hipEventCreate(&t0);
    if (err == hipSuccess) err = hipEventCreate(&t1);
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
      launch_lora_merge(d_w, d_a, d_b, rows, cols, r, scale, nullptr);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(t0, nullptr);
    for (int i = 0; i < iters && err == hipSuccess; i++) {
      launch_lora_merge(d_w, d_a, d_b, rows, cols, r, scale, nullptr);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(t1, nullptr);
    if (err == hipSuccess) err = hipEventSynchronize(t1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
    if (t0) hipEventDestroy(t0);
    if (t1) hipEventDestroy(t1);
    if (err != hipSuccess) return fail(MX_ERR_HIP, std::string("mx_lora_merge_probe: ") + hipGetErrorString(err));
    *us_per_launch = (double)ms * 1e3 / iters;
  }
  return 0;
}

int mx_grammar_mask_probe(int device, const float* logits_host, int n, int V, int ldl, const uint32_t* masks,
                          const uint32_t* on, float* out) {
  if (!logits_host || !masks || !on || !out || n < 1 || n > MAX_ROWS || V < 1 || V > (1 << 20) || ldl < V ||
      ldl > (1 << 20) + 64)
    return fail(MX_ERR_ARG, "mx_grammar_mask_probe: 1 <= n <= 64 rows, 1 <= V <= 2^20, V <= ldl <= 2^20 + 64, masks, on and out");
  if (device >= 0) HIPC(hipSetDevice(device));
  const size_t elems = (size_t)n * ldl, nw = ((size_t)V + 31) / 32;
  DevBufs dev;
  float* d_l = nullptr;
  uint32_t *d_m = nullptr, *d_on = nullptr;
  if (!dev.alloc(&d_l, elems * 4) || !dev.alloc(&d_m, (size_t)n * nw * 4) || !dev.alloc(&d_on, (size_t)n * 4))
    return fail(MX_ERR_HIP, "mx_grammar_mask_probe: device allocation");
  HIPC(hipMemcpy(d_l, logits_host, elems * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_m, masks, (size_t)n * nw * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d_on, on, (size_t)n * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  if (launch_grammar_mask(d_l, ldl, n, V, d_m, d_on, nullptr))
    return fail(MX_ERR_ARG, "mx_grammar_mask_probe: launch_grammar_mask refused");
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(out, d_l, elems * 4, hipMemcpyDeviceToHost));
  return 0;
}

int mx_grammar_mask_time(int device, int n, int V, int ldl, const uint32_t* masks, int iters, double* us_per_launch) {
  if (!masks || !us_per_launch || n < 1 || n > MAX_ROWS || V < 1 || V > (1 << 20) || ldl < V || ldl > (1 << 20) + 64 ||
      iters < 1 || iters > 100000)
    return fail(MX_ERR_ARG, "mx_grammar_mask_time: 1 <= n <= 64 rows, 1 <= V <= 2^20, V <= ldl <= 2^20 + 64, masks, "
                            "1 <= iters <= 100000 and us_per_launch");
  if (device >= 0) HIPC(hipSetDevice(device));
  const size_t elems = (size_t)n * ldl, nw = ((size_t)V + 31) / 32;
  DevBufs dev;
  float* d_l = nullptr;
  uint32_t *d_m = nullptr, *d_on = nullptr;
  if (!dev.alloc(&d_l, elems * 4) || !dev.alloc(&d_m, (size_t)n * nw * 4) || !dev.alloc(&d_on, (size_t)n * 4))
    return fail(MX_ERR_HIP, "mx_grammar_mask_time: device allocation");
  HIPC(hipMemset(d_l, 0, elems * 4));
  HIPC(hipMemset(d_on, 1, (size_t)n * 4));  // every row on
  HIPC(hipMemcpy(d_m, masks, (size_t)n * nw * 4, hipMemcpyHostToDevice));
  HIPC(hipDeviceSynchronize());
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipError_t err = hipEventCreate(&t0);
  if (err == hipSuccess) err = hipEventCreate(&t1);
  for (int i = 0; i < 3 && err == hipSuccess; i++) {
    if (launch_grammar_mask(d_l, ldl, n, V, d_m, d_on, nullptr)) err = hipErrorInvalidValue;
    else err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(t0, nullptr);
  for (int i = 0; i < iters && err == hipSuccess; i++) {
    launch_grammar_mask(d_l, ldl, n, V, d_m, d_on, nullptr);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(t1, nullptr);
  if (err == hipSuccess) err = hipEventSynchronize(t1);
  float ms = 0.f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
  if (t0) hipEventDestroy(t0);
  if (t1) hipEventDestroy(t1);
  if (err != hipSuccess) return fail(MX_ERR_HIP, std::string("mx_grammar_mask_time: ") + hipGetErrorString(err));
  *us_per_launch = (double)ms * 1e3 / iters;
  return 0;
}

int mx_probe_copy(int device, size_t bytes, int iters, double* gbs, char* desc, int desc_len) {
  return probe_hbm(device, bytes, iters, false, gbs, desc, desc_len);
}

int mx_probe_read(int device, size_t bytes, int iters, double* gbs, char* desc, int desc_len) {
  return probe_hbm(device, bytes, iters, true, gbs, desc, desc_len);
}

}  // extern "C"
