// kernels.hip -- gfx950 (CDNA4) kernels of the MI355X-native LLaMA forward.
//
// They replace the ggml CPU ops that llama.cpp's llm_build_llama runs for the
// reference's hot call  self.model(prompt, max_tokens=100)
// (/root/reference/llama_p2p_network.py:125, model built at :19).  Numerics
// follow ggml's CPU semantics: bf16 weights, activations
// rounded to bf16 before each weight product, f32 accumulation, f16 K/V cache,
// f16-rounded q and probabilities in attention, double-sum RMSNorm.
//
// Decode is HBM-bound (≈1 flop/byte at one token, ≈32 at 32 tokens, both far
// below the ≈300 flop/byte ridge), so the design goal is streaming every
// weight byte once at full HBM rate:
//   * weights are pre-packed into 1 KiB MFMA A-operand tiles (kernels.h), so a
//     wave-instruction is one contiguous 1 KiB, non-temporal, 16 B/lane load;
//   * v_mfma_f32_16x16x32_bf16 does the dot products for 1..64 tokens (its
//     issue rate is ~25x what HBM can feed, so padding columns costs nothing);
//   * K is split across the waves of a work-group (register ring of U loads
//     in flight per wave), partial tiles are summed through LDS, and the
//     epilogue fuses RoPE + KV-cache store, SwiGLU, or the residual add.
#include "device_common.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace mx {

__global__ void synth_packed_kernel(uint16_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale,
                                    int mode, int offset) {
  const int KT = K / TILE_K;
  const size_t total = (size_t)N * K;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / K), col = (int)(i % K);
    dst[packed_index(packed_row(row, mode, offset), col, KT)] = (uint16_t)f2bf(synth_value(seed, tid, i, scale));
  }
}

__global__ void pack_kernel(uint16_t* dst, const uint16_t* src, int N, int K, int mode, int offset) {
  const int KT = K / TILE_K;
  const size_t total = (size_t)N * K;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / K), col = (int)(i % K);
    dst[packed_index(packed_row(row, mode, offset), col, KT)] = src[i];
  }
}

__global__ void synth_rowmajor_kernel(uint16_t* dst, size_t n, uint64_t seed, uint64_t tid, float scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = (uint16_t)f2bf(synth_value(seed, tid, i, scale));
}

__global__ void synth_norm_kernel(float* dst, size_t n, uint64_t seed, uint64_t tid, float scale) {
  // 1 + v rounded twice, as synth.py and the oracle (hipcc would otherwise contract it into an fma)
#pragma clang fp contract(off)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = 1.0f + synth_value(seed, tid, i, scale);
}

void launch_synth_packed(uint16_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                         int offset, hipStream_t s) {
  synth_packed_kernel<<<fill_grid((size_t)N * K), 256, 0, s>>>(dst, N, K, seed, tid, scale, mode, offset);
}
void launch_pack(uint16_t* dst, const uint16_t* src, int N, int K, int mode, int offset, hipStream_t s) {
  pack_kernel<<<fill_grid((size_t)N * K), 256, 0, s>>>(dst, src, N, K, mode, offset);
}
// NeoX -> adjacent-pair row order inside each head of d rows: dst row 2i + j of a head = src row
// j*d/2 + i, j in {0, 1}.  A row is row_bytes contiguous bytes of any supported type (bf16, or the blocks of that
// row), moved as T units; grid-stride over the units, so any shape runs and nothing is written past n_rows rows.
template <typename T>
__global__ void permute_rows_kernel(T* dst, const T* src, size_t n_rows, size_t row_units, int d) {
  const size_t total = n_rows * row_units;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / row_units, u = i % row_units;
    const size_t head = row / d;
    const int r = (int)(row % d);
    const size_t srow = head * d + (size_t)(r & 1) * (d / 2) + (r >> 1);
    dst[i] = src[srow * row_units + u];
  }
}
int launch_permute_rows_neox(void* dst, const void* src, size_t n_rows, size_t row_bytes, int d, hipStream_t s) {
  if (!dst || !src || dst == src || d < 2 || d % 2 || n_rows % d || row_bytes < 1) return -1;
  const bool a16 = row_bytes % 16 == 0 && ((uintptr_t)dst | (uintptr_t)src) % 16 == 0;
  const bool a2 = row_bytes % 2 == 0 && ((uintptr_t)dst | (uintptr_t)src) % 2 == 0;
  if (a16)
    permute_rows_kernel<u32x4><<<fill_grid(n_rows * (row_bytes / 16)), 256, 0, s>>>((u32x4*)dst, (const u32x4*)src,
                                                                                    n_rows, row_bytes / 16, d);
  else if (a2)  // e.g. a Q8_0 row of 448 columns: 14 blocks of 34 bytes
    permute_rows_kernel<uint16_t><<<fill_grid(n_rows * (row_bytes / 2)), 256, 0, s>>>(
        (uint16_t*)dst, (const uint16_t*)src, n_rows, row_bytes / 2, d);
  else
    permute_rows_kernel<uint8_t><<<fill_grid(n_rows * row_bytes), 256, 0, s>>>((uint8_t*)dst, (const uint8_t*)src,
                                                                               n_rows, row_bytes, d);
  return 0;
}
void launch_synth_rowmajor(uint16_t* dst, size_t n, uint64_t seed, uint64_t tid, float scale, hipStream_t s) {
  synth_rowmajor_kernel<<<fill_grid(n), 256, 0, s>>>(dst, n, seed, tid, scale);
}
void launch_synth_norm(float* dst, size_t n, uint64_t seed, uint64_t tid, float scale, hipStream_t s) {
  synth_norm_kernel<<<fill_grid(n), 256, 0, s>>>(dst, n, seed, tid, scale);
}

// ---------------------------------------------------------------------------
// GET_ROWS: token embedding, bf16 -> f32  
// ---------------------------------------------------------------------------
// One work-group per token; thread t converts 16-element tiles t, t+256, ... and, when ssq is
// given, writes each tile's sum of squares (the partials XS consumers reduce, see mm_kernel).
__global__ __launch_bounds__(256) void embed_kernel(float* x, const uint16_t* tok_embd, const int* ids, int n,
                                                    float* ssq) {
  const int c = blockIdx.x;
  const int id = ids[c];
  const u32x4* src = reinterpret_cast<const u32x4*>(tok_embd + (size_t)id * n);
  f32x4* dst = reinterpret_cast<f32x4*>(x + (size_t)c * n);
  for (int t = threadIdx.x; t < n / 16; t += blockDim.x) {
    f32x4 g[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 v = src[2 * t + h];
      f32x4 lo, hi;
      lo[0] = __uint_as_float(v[0] << 16); lo[1] = __uint_as_float(v[0] & 0xffff0000u);
      lo[2] = __uint_as_float(v[1] << 16); lo[3] = __uint_as_float(v[1] & 0xffff0000u);
      hi[0] = __uint_as_float(v[2] << 16); hi[1] = __uint_as_float(v[2] & 0xffff0000u);
      hi[2] = __uint_as_float(v[3] << 16); hi[3] = __uint_as_float(v[3] & 0xffff0000u);
      dst[4 * t + 2 * h] = lo;
      dst[4 * t + 2 * h + 1] = hi;
      g[2 * h] = lo;
      g[2 * h + 1] = hi;
    }
    if (ssq) ssq[(size_t)c * (n / 16) + t] = ssq16(g[0], g[1], g[2], g[3]);
  }
}

void launch_embed(float* x, const uint16_t* tok_embd, const int* ids, int M, int n, float* ssq, hipStream_t s) {
  embed_kernel<<<M, 256, 0, s>>>(x, tok_embd, ids, n, ssq);
}

// per-16-row-tile sums of squares of an existing residual stream (a pipeline stage's x_in)
__global__ __launch_bounds__(256) void ssq_kernel(const float* x, int n, float* ssq) {
  const int c = blockIdx.x;
  const f32x4* src = reinterpret_cast<const f32x4*>(x + (size_t)c * n);
  for (int t = threadIdx.x; t < n / 16; t += blockDim.x)
    ssq[(size_t)c * (n / 16) + t] = ssq16(src[4 * t], src[4 * t + 1], src[4 * t + 2], src[4 * t + 3]);
}

void launch_ssq(const float* x, int M, int n, float* ssq, hipStream_t s) { ssq_kernel<<<M, 256, 0, s>>>(x, n, ssq); }

// ---------------------------------------------------------------------------
// RMS_NORM + MUL(norm weight) -> bf16 activation  
// ggml: sum of x*x in double, scale = 1/sqrtf(mean + eps), y = (x*scale)*w;
// the bf16 rounding is the conversion ggml applies to src1 of the next MUL_MAT.
// ---------------------------------------------------------------------------
// x[r] += (sum of NS partial slabs in slab order; written back when NS > 0) -- the same expression
// as the <= 16-row EPI_RESID epilogues, x + (((s0 + s1) + s2) + ...); then, if y,
// y[c] = bf16((x[r] * 1/sqrtf(mean(x^2) + eps)) * w) with the sum of squares in double (ggml
// RMS_NORM + MUL), formed exactly as RMS_NORM on load forms it (device_common.h ssq16 / ssq_lane /
// ssq_wave: 16-value tile partials in LDS, then one wave's canonical row sum), so a row normalises
// to the same bits at every row count.  One 1024-thread work-group per row and every load issued
// up front: a single memory round trip, which is what a row of 4096-8192 floats costs at decode.
template <int NS, int IT>
__global__ __launch_bounds__(1024) void norm_kernel(uint16_t* y, int ldy, float* x, const float* slabs, size_t stride,
                                                    const float* w, const int* row_map, int n, float eps) {
  const int c = blockIdx.x;
  const int r = row_map ? row_map[c] : c;
  float* xr = x + (size_t)r * n;
  const int tid = threadIdx.x;
  f32x4 v[IT], g[IT], sl[IT][NS > 0 ? NS : 1];
  // the norm weight is loaded unconditionally (x stands in without y): behind `if (y)` the load made
  // hipcc wait for it alone (vmcnt(0)) before issuing x and the slabs -- two round trips, not one
  const float* wp = y ? w : xr;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int i = (it * 1024 + tid) * 4;
    v[it] = *reinterpret_cast<const f32x4*>(xr + i);
    g[it] = *reinterpret_cast<const f32x4*>(wp + i);
#pragma unroll
    for (int k = 0; k < NS; ++k) sl[it][k] = *reinterpret_cast<const f32x4*>(slabs + k * stride + (size_t)r * n + i);
  }
  if constexpr (NS > 0) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      f32x4 t = sl[it][0];
#pragma unroll
      for (int k = 1; k < NS; ++k) t += sl[it][k];
      v[it] += t;
      *reinterpret_cast<f32x4*>(xr + (it * 1024 + tid) * 4) = v[it];
    }
  }
  if (!y) return;
  __shared__ __attribute__((aligned(16))) float part[IT * 256];
  __shared__ float sc_sh;
#pragma unroll
  for (int it = 0; it < IT; ++it) {  // thread 4T+i holds values 4i..4i+3 of tile T (+256 it)
    double g = ssq4(v[it]);
    g += __shfl_xor(g, 1);
    g += __shfl_xor(g, 2);
    if ((tid & 3) == 0) part[it * 256 + (tid >> 2)] = (float)g;
  }
  __syncthreads();
  if (tid < 64) {
    f32x4 q[IT];
#pragma unroll
    for (int p = 0; p < IT; ++p) q[p] = *reinterpret_cast<const f32x4*>(part + 256 * p + 4 * tid);
    const double sum = ssq_wave(ssq_lane(q, tid, n / 16));
    if (tid == 0) sc_sh = rms_scale(sum, n, eps);
  }
  __syncthreads();
  const float scale = sc_sh;
  uint16_t* yr = y + (size_t)c * ldy;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    u32x2 o;
    o[0] = f2bf((v[it][0] * scale) * g[it][0]) | (f2bf((v[it][1] * scale) * g[it][1]) << 16);
    o[1] = f2bf((v[it][2] * scale) * g[it][2]) | (f2bf((v[it][3] * scale) * g[it][3]) << 16);
    *reinterpret_cast<u32x2*>(yr + (it * 1024 + tid) * 4) = o;
  }
}

template <int NS>
static void launch_norm_ns(uint16_t* y, int ldy, float* x, const float* slabs, size_t stride, const float* w,
                           const int* row_map, int M, int n, float eps, hipStream_t s) {
  if (n == 4096)
    norm_kernel<NS, 1><<<M, 1024, 0, s>>>(y, ldy, x, slabs, stride, w, row_map, n, eps);
  else if constexpr (NS <= 8)  // 16 slabs: n 4096 only (register budget)
    norm_kernel<NS, 2><<<M, 1024, 0, s>>>(y, ldy, x, slabs, stride, w, row_map, n, eps);
}

// n must be 4096 or 8192 for the 1024-thread layout; other widths use the generic path below
// (n % 64 == 0, n <= NORM_GENERIC_MAXN)
constexpr int NORM_GENERIC_MAXN = 16384;
__global__ __launch_bounds__(256) void norm_generic_kernel(uint16_t* y, int ldy, float* x, const float* slabs,
                                                           int nslab, size_t stride, const float* w,
                                                           const int* row_map, int n, float eps) {
  const int c = blockIdx.x;
  const int r = row_map ? row_map[c] : c;
  float* xr = x + (size_t)r * n;
  __shared__ __attribute__((aligned(16))) float part[NORM_GENERIC_MAXN / 16];
  __shared__ float sc_sh;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {  // n % 64 == 0: the 4 threads of a tile share a pass
    f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
    if (nslab) {
      f32x4 t = *reinterpret_cast<const f32x4*>(slabs + (size_t)r * n + i);
      for (int k = 1; k < nslab; ++k) t += *reinterpret_cast<const f32x4*>(slabs + k * stride + (size_t)r * n + i);
      v += t;
      *reinterpret_cast<f32x4*>(xr + i) = v;
    }
    double g = ssq4(v);
    g += __shfl_xor(g, 1);
    g += __shfl_xor(g, 2);
    if ((threadIdx.x & 3) == 0) part[i >> 4] = (float)g;
  }
  if (!y) return;
  __syncthreads();
  if (threadIdx.x < 64) {
    constexpr int P = NORM_GENERIC_MAXN / 4096;
    f32x4 q[P];
#pragma unroll
    for (int p = 0; p < P; ++p) q[p] = *reinterpret_cast<const f32x4*>(part + min(256 * p + 4 * (int)threadIdx.x, n / 16 - 4));
    const double sum = ssq_wave(ssq_lane(q, threadIdx.x, n / 16));
    if (threadIdx.x == 0) sc_sh = rms_scale(sum, n, eps);
  }
  __syncthreads();
  const float scale = sc_sh;
  uint16_t* yr = y + (size_t)c * ldy;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
    u32x2 o;
    o[0] = f2bf((v[0] * scale) * g[0]) | (f2bf((v[1] * scale) * g[1]) << 16);
    o[1] = f2bf((v[2] * scale) * g[2]) | (f2bf((v[3] * scale) * g[3]) << 16);
    *reinterpret_cast<u32x2*>(yr + i) = o;
  }
}

static void launch_norm_impl(uint16_t* y, int ldy, float* x, const float* slabs, int nslab, size_t stride,
                             const float* w, const int* row_map, int M, int n, float eps, hipStream_t s) {
  if ((n == 4096 || n == 8192) && (nslab == 0 || nslab == 1 || nslab == 2 || nslab == 4 || nslab == 8 ||
                                   (nslab == 16 && n == 4096))) {
    switch (nslab) {
      case 16: launch_norm_ns<16>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
      case 8: launch_norm_ns<8>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
      case 0: launch_norm_ns<0>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
      case 1: launch_norm_ns<1>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
      case 2: launch_norm_ns<2>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
      case 4: launch_norm_ns<4>(y, ldy, x, slabs, stride, w, row_map, M, n, eps, s); return;
    }
  }
  if (n % 64 || n > NORM_GENERIC_MAXN) return;  // init_common rejects such widths (engine.cpp)
  norm_generic_kernel<<<M, 256, 0, s>>>(y, ldy, x, slabs, nslab, stride, w, row_map, n, eps);
}

void launch_rmsnorm(uint16_t* y, int ldy, const float* x, const float* w, const int* row_map, int M, int n,
                    float eps, hipStream_t s) {
  launch_norm_impl(y, ldy, const_cast<float*>(x), nullptr, 0, 0, w, row_map, M, n, eps, s);
}

// ---------------------------------------------------------------------------
// Embeddings: the tail ggml's result_norm and pooling graph perform on the f32
// residual stream of the last layer -- final RMS_NORM + MUL kept in f32, pooling over the rows of a
// sequence, optional L2 normalisation.  Every sum has one order: the sums of squares are the canonical
// ones above (so a row gives the same bits at every row count and in every chunk), the mean adds a
// column's rows in position order inside one thread.
// ---------------------------------------------------------------------------
// y[dst[c]] = (x[src[c]] * scale) * w in f32: norm_kernel's layout (one 1024-thread work-group per row,
// every load issued up front) without the slabs and without the bf16 rounding
template <int IT>
__global__ __launch_bounds__(1024) void embd_norm_kernel(float* y, const float* x, const float* w, const int* src,
                                                         const int* dst, int n, float eps) {
  const int c = blockIdx.x;
  const float* xr = x + (size_t)(src ? src[c] : c) * n;
  float* yr = y + (size_t)(dst ? dst[c] : c) * n;
  const int tid = threadIdx.x;
  f32x4 v[IT], g[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int i = (it * 1024 + tid) * 4;
    v[it] = *reinterpret_cast<const f32x4*>(xr + i);
    g[it] = *reinterpret_cast<const f32x4*>(w + i);
  }
  __shared__ __attribute__((aligned(16))) float part[IT * 256];
  __shared__ float sc_sh;
#pragma unroll
  for (int it = 0; it < IT; ++it) {  // thread 4T+i holds values 4i..4i+3 of tile T (+256 it)
    double q = ssq4(v[it]);
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    if ((tid & 3) == 0) part[it * 256 + (tid >> 2)] = (float)q;
  }
  __syncthreads();
  if (tid < 64) {
    f32x4 q[IT];
#pragma unroll
    for (int p = 0; p < IT; ++p) q[p] = *reinterpret_cast<const f32x4*>(part + 256 * p + 4 * tid);
    const double sum = ssq_wave(ssq_lane(q, tid, n / 16));
    if (tid == 0) sc_sh = rms_scale(sum, n, eps);
  }
  __syncthreads();
  const float scale = sc_sh;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[it][j] * scale) * g[it][j];
    *reinterpret_cast<f32x4*>(yr + (it * 1024 + tid) * 4) = o;
  }
}

// The row sum of squares of v[0..n) (n % 64 == 0, n <= NORM_GENERIC_MAXN) in the canonical form, by a
// 256-thread work-group: every thread returns it.  part: NORM_GENERIC_MAXN / 16 floats of LDS.
__device__ __forceinline__ double row_ssq_256(const float* v, int n, float* part, double* sum_sh) {
  for (int i = threadIdx.x * 4; i < n; i += 1024) {  // n % 64 == 0: the 4 threads of a tile share a pass
    double q = ssq4(*reinterpret_cast<const f32x4*>(v + i));
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    if ((threadIdx.x & 3) == 0) part[i >> 4] = (float)q;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    constexpr int P = NORM_GENERIC_MAXN / 4096;
    f32x4 q[P];
#pragma unroll
    for (int p = 0; p < P; ++p)
      q[p] = *reinterpret_cast<const f32x4*>(part + min(256 * p + 4 * (int)threadIdx.x, n / 16 - 4));
    const double sum = ssq_wave(ssq_lane(q, threadIdx.x, n / 16));
    if (threadIdx.x == 0) *sum_sh = sum;
  }
  __syncthreads();
  return *sum_sh;
}

__global__ __launch_bounds__(256) void embd_norm_generic_kernel(float* y, const float* x, const float* w,
                                                                const int* src, const int* dst, int n, float eps) {
  const int c = blockIdx.x;
  const float* xr = x + (size_t)(src ? src[c] : c) * n;
  float* yr = y + (size_t)(dst ? dst[c] : c) * n;
  __shared__ __attribute__((aligned(16))) float part[NORM_GENERIC_MAXN / 16];
  __shared__ double sum_sh;
  const float scale = rms_scale(row_ssq_256(xr, n, part, &sum_sh), n, eps);
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] * scale) * g[j];
    *reinterpret_cast<f32x4*>(yr + i) = o;
  }
}

int launch_embd_norm(float* y, const float* x, const float* w, const int* src, const int* dst, int M, int n,
                     float eps, hipStream_t s) {
  if (M < 1 || n < 64 || n % 64 || n > NORM_GENERIC_MAXN) return -1;
  if (n == 4096)
    embd_norm_kernel<1><<<M, 1024, 0, s>>>(y, x, w, src, dst, n, eps);
  else if (n == 8192)
    embd_norm_kernel<2><<<M, 1024, 0, s>>>(y, x, w, src, dst, n, eps);
  else
    embd_norm_generic_kernel<<<M, 256, 0, s>>>(y, x, w, src, dst, n, eps);
  return 0;
}

// MEAN pooling.  Segment g (grid.y) = EMBD_SEG ints {first y row, rows (>= 1), accumulator row, output row,
// first, T}: the running sum of a sequence starts from its first row (first != 0) or from acc, takes the
// segment's rows in order, and goes back to acc (T == 0: the sequence continues in a later chunk) or,
// divided by T, to out.  A thread owns 4 columns from start to end: (((y0 + y1) + y2) + ...) / T.
__global__ __launch_bounds__(256) void embd_mean_kernel(const float* y, const int* seg, int n, float* acc, float* out) {
  const int* sg = seg + EMBD_SEG * blockIdx.y;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int rows = sg[1], T = sg[5];
  const float* yp = y + (size_t)sg[0] * n + i;
  float* ap = acc + (size_t)sg[2] * n + i;
  f32x4 a;
  int t = 0;
  if (sg[4]) {
    a = *reinterpret_cast<const f32x4*>(yp);
    t = 1;
  } else {
    a = *reinterpret_cast<const f32x4*>(ap);
  }
#pragma unroll 8
  for (; t < rows; ++t) a += *reinterpret_cast<const f32x4*>(yp + (size_t)t * n);
  if (T > 0) {
    const float d = (float)T;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = a[j] / d;
    *reinterpret_cast<f32x4*>(out + (size_t)sg[3] * n + i) = a;
  } else {
    *reinterpret_cast<f32x4*>(ap) = a;
  }
}

int launch_embd_mean(const float* y, const int* seg, int n_seg, int n, float* acc, float* out, hipStream_t s) {
  if (n_seg < 1 || n_seg > 65535 || n < 64 || n % 64) return -1;
  embd_mean_kernel<<<dim3((n / 4 + 255) / 256, n_seg), 256, 0, s>>>(y, seg, n, acc, out);
  return 0;
}

// v[rows[c]] /= ||v[rows[c]]|| in place, the sum of squares in the canonical form; a vector of norm 0
// stays as it is (llama-cpp-python's _normalize_embedding), so the result is never NaN
__global__ __launch_bounds__(256) void embd_l2_kernel(float* v, const int* rows, int n) {
  float* vr = v + (size_t)(rows ? rows[blockIdx.x] : blockIdx.x) * n;
  __shared__ __attribute__((aligned(16))) float part[NORM_GENERIC_MAXN / 16];
  __shared__ double sum_sh;
  const float nrm = (float)sqrt(row_ssq_256(vr, n, part, &sum_sh));
  if (nrm == 0.0f) return;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    f32x4 o = *reinterpret_cast<const f32x4*>(vr + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = o[j] / nrm;
    *reinterpret_cast<f32x4*>(vr + i) = o;
  }
}

int launch_embd_l2(float* v, const int* rows, int M, int n, hipStream_t s) {
  if (M < 1 || n < 64 || n % 64 || n > NORM_GENERIC_MAXN) return -1;
  embd_l2_kernel<<<M, 256, 0, s>>>(v, rows, n);
  return 0;
}

// ---------------------------------------------------------------------------
// MUL_MAT with bf16 weights for 1..64 tokens (decode GEMV / skinny GEMM) with
// fused epilogues.  
//
// Work-group = KS waves = RT row tiles (16 rows each) x all K; wave w owns the
// K-tiles [KT*w/KS, KT*(w+1)/KS).  Per K-tile a wave issues RT weight loads
// (1 KiB each, contiguous, non-temporal) and NB activation fragments, and
// RT*NB MFMAs.  A ring of U K-tiles per wave keeps U*RT weight loads in flight.
//
// XS (RMS_NORM on load, <= 4 tokens): there is no normalised activation
// buffer and no norm launch.  The kernel that last wrote the residual stream x
// (embedding, or an EPI_RESID GEMV) also wrote ssq[col][t] = sum of x^2 over
// the 16 rows of its tile t.  Every wave sums those partials in a fixed order
// (double, as ggml), derives 1/sqrt(mean+eps), and writes bf16((x*scale)*w) --
// the exact value ggml's RMS_NORM+MUL feeds MUL_MAT -- for its own K-slice into
// a wave-private LDS image that its B fragments are read from.
// ---------------------------------------------------------------------------
// XS operands of one wave, loaded BEFORE its weight ring (a load issued behind the ring waits
// for the ring: that ordering cost more than the norm launch it replaces).  Per column c < M:
// this lane's 4 partials of ssq (whole wave = all np <= 512 of them, 2 pieces) and 4 values of
// x and of w per 256-k piece of the wave's K-slice (nk <= 512: 2 pieces).
constexpr int XS_MAX_M = 4;
template <int MM = XS_MAX_M>
struct XsRegs {
  f32x4 q[MM][2], x[MM][2], g[2];
};

// Every load is unconditional, at a clamped address (lanes / rows past the end re-read valid data
// that xs_build ignores): a load behind a branch left hipcc's wait counts at the merge at zero, and
// each conditional load then waited for itself -- up to 2 + 4·MM serialised L2 round trips before
// the weight ring was even issued.
template <int MM>
__device__ __forceinline__ void xs_load(XsRegs<MM>& r, const MMArgs& a, int kbase, int nk, int lane) {
  const int i0 = lane * 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int i = i0 + 256 * p;
    const int ik = min(i, nk - 4), iq = min(i, a.np - 4);
    r.g[p] = *reinterpret_cast<const f32x4*>(a.norm_w + kbase + ik);
#pragma unroll
    for (int c = 0; c < MM; ++c) {
      const size_t cc = (size_t)min(c, a.M - 1);
      r.q[c][p] = *reinterpret_cast<const f32x4*>(a.ssq + cc * a.np + iq);
      r.x[c][p] = *reinterpret_cast<const f32x4*>(a.xf + cc * a.K + kbase + ik);
    }
  }
}

// scale per column from the partials (fixed-order lane sum, then a fixed xor tree: every lane
// agrees), then xs[c][k - kbase] = bf16((x * scale) * w): this wave's LDS image (only it reads it)
template <int MM>
__device__ __forceinline__ void xs_build(const XsRegs<MM>& r, const MMArgs& a, uint16_t* xs, int pitch, int nk,
                                         int lane) {
  const int i0 = lane * 4;
#pragma unroll
  for (int c = 0; c < MM; ++c) {
    if (c >= a.M) break;
    const float sc = rms_scale(ssq_wave(ssq_lane(r.q[c], lane, a.np)), a.K, a.eps);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int i = i0 + 256 * p;
      if (i < nk) {
        const f32x4 xv = r.x[c][p], g = r.g[p];
        u32x2 o;
        o[0] = f2bf((xv[0] * sc) * g[0]) | (f2bf((xv[1] * sc) * g[1]) << 16);
        o[1] = f2bf((xv[2] * sc) * g[2]) | (f2bf((xv[3] * sc) * g[3]) << 16);
        *reinterpret_cast<u32x2*>(xs + c * pitch + i) = o;
      }
    }
  }
}

// Canonical fold of the KS per-wave K-slice partials (batch invariance): with KS = 16
// the waves' slices are the 16 canonical slices, summed as G groups of 16/G consecutive slices (each
// group in slice order), then the group sums in order -- exactly the value the 17..64-row path forms
// (mm_wide: one work-group per group, each wave folding its slices as they end; the slabs then added
// in slab order).  get(ww) returns wave ww's partial.  KG > 0: the group count known at compile time
// (KG = 1: one plain sequential sum -- gate/up and the lm_head, whose 17..64-row launches do not split
// K); KG = 0: kgrp read at run time.  The reads are on the critical path of the persistent GEMVs'
// tile epilogue (wave 0, between barriers), so the compile-time forms keep them one unrolled chain.
template <int KS, int UNR = KS, int KG = 0, typename F>
__device__ __forceinline__ f32x4 kfold(const F& get, int kgrp) {
  if constexpr (KG == 1) {
    f32x4 s = get(0);
#pragma unroll UNR
    for (int ww = 1; ww < KS; ++ww) s += get(ww);
    return s;
  } else if constexpr (KG > 1) {
    // UNR as the caller asks (mm_pers_kernel's q|k|v finish: 3-way for 3 tiles per work-group)
    constexpr int m = KS / KG;
    f32x4 s = get(0), part = s;
#pragma unroll UNR
    for (int ww = 1; ww < KS; ++ww) {
      const f32x4 v = get(ww);
      if (ww % m) {
        part += v;
      } else {
        s = (ww == m) ? part : s + part;
        part = v;
      }
    }
    return KG == 1 ? part : s + part;
  }
  const int G = (kgrp > 0 && KS % kgrp == 0) ? kgrp : 1;
  const int mm = KS / G - 1;  // KS / G is a power of two
  f32x4 s = get(0), part = s;
#pragma unroll UNR
  for (int ww = 1; ww < KS; ++ww) {
    const f32x4 v = get(ww);
    if (ww & mm) {
      part += v;
    } else {
      s = (ww - 1 == mm) ? part : s + part;  // group (ww-1)/(mm+1) complete
      part = v;
    }
  }
  return KS - 1 == mm ? part : s + part;
}

// gate/up and the lm_head never split K in their 17..64-row launches: one canonical group
template <int EPI>
constexpr int epi_kg() { return (EPI == EPI_SWIGLU || EPI == EPI_F32) ? 1 : 0; }

template <int KS, int RT, int NB, int EPI, int U, bool XS>
__device__ __forceinline__ void mm_body(const MMArgs& a, int tile0) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int KT = a.K / TILE_K;
  const int kb = (KT * w) / KS, ke = (KT * (w + 1)) / KS;

  __shared__ f32x4 red[KS][RT][NB][64];
  extern __shared__ __attribute__((aligned(16))) uint16_t xs_dyn[];  // XS: per-wave [M][xs_pitch] images

  const u32x4* Wp[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
    Wp[r] = reinterpret_cast<const u32x4*>(a.W) + (size_t)(tile0 + r) * KT * 64 + lane;
  // B fragment source (lane -> token column, k offset); padded columns re-read a valid row (outputs dropped)
  const u32x4* Xp[NB];
  const int xs_pitch = (KT + KS - 1) / KS * TILE_K + 8;  // bf16 per image row (+16 B: conflict-free columns)
  uint16_t* xsw = xs_dyn + (size_t)w * a.M * xs_pitch;
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    int col = n * 16 + (lane & 15);
    col = col < a.M ? col : a.M - 1;
    if constexpr (XS)  // image k index = (kt - kb) * 32 + k within tile
      Xp[n] = reinterpret_cast<const u32x4*>(xsw + col * xs_pitch + (lane >> 4) * 8 - kb * TILE_K);
    else
      Xp[n] = reinterpret_cast<const u32x4*>(a.X + (size_t)col * a.ldx + (lane >> 4) * 8);
  }

  f32x4 acc[RT][NB];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mma = [&](const u32x4 (&wa)[RT], const u32x4 (&xb)[NB]) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int n = 0; n < NB; ++n)
        acc[r][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wa[r]),
                                                             __builtin_bit_cast(bf16x8, xb[n]), acc[r][n], 0, 0, 0);
  };

  XsRegs<> xr;
  if constexpr (XS) xs_load(xr, a, kb * TILE_K, (ke - kb) * TILE_K, lane);
  u32x4 ra[U][RT];
  int kt = kb;
  const int nfull = (ke - kb) / U;
  if (nfull > 0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < RT; ++r) ra[u][r] = __builtin_nontemporal_load(Wp[r] + (size_t)(kt + u) * 64);
  }
  if constexpr (XS) {
    xs_build(xr, a, xsw, xs_pitch, (ke - kb) * TILE_K, lane);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's image is in LDS
    __builtin_amdgcn_wave_barrier();
  }
  auto load_b = [&](u32x4 (&xb)[NB], int k) {
#pragma unroll
    for (int n = 0; n < NB; ++n) xb[n] = Xp[n][k * 4];
  };

  if (nfull > 0) {
    for (int ch = 1; ch < nfull; ++ch) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 xb[NB];
        load_b(xb, kt + u);
        mma(ra[u], xb);
#pragma unroll
        for (int r = 0; r < RT; ++r) ra[u][r] = __builtin_nontemporal_load(Wp[r] + (size_t)(kt + U + u) * 64);
      }
      kt += U;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 xb[NB];
      load_b(xb, kt + u);
      mma(ra[u], xb);
    }
    kt += U;
  }
  for (; kt < ke; ++kt) {
    u32x4 sa[RT], sb[NB];
#pragma unroll
    for (int r = 0; r < RT; ++r) sa[r] = __builtin_nontemporal_load(Wp[r] + (size_t)kt * 64);
    load_b(sb, kt);
    mma(sa, sb);
  }

  // ---- sum the KS partial tiles through LDS
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) red[w][r][n][lane] = acc[r][n];
  __syncthreads();

  // ---- epilogue.  unit = (r, n, lane): rows 16*(tile0+r) + 4*(lane>>4) + i, i<4; col n*16 + (lane&15)
  // SWIGLU tiles hold 8 gate rows (lanes 0-31 of the C layout) and the matching 8 up rows (lanes 32-63)
  constexpr int LU = (EPI == EPI_SWIGLU) ? 32 : 64;
  constexpr int UNITS = RT * NB * LU;
  for (int u = threadIdx.x; u < UNITS; u += 64 * KS) {
    const int l = u % LU;
    const int n = (u / LU) % NB;
    const int r = (u / LU) / NB;
    const int col = n * 16 + (l & 15);
    const f32x4 s = kfold<KS, KS, epi_kg<EPI>()>([&](int ww) { return red[ww][r][n][l]; }, a.kgrp);
    if constexpr (EPI == EPI_RESID) {
      // residual add, and this tile's share of the next RMS_NORM's sum of squares: a wave holds one
      // whole (r, n) unit block (LU = 64), so lanes l, l^16, l^32, l^48 hold the tile's 16 rows of col
      double q = 0.0;
      if (col < a.M) {
        f32x4* px = reinterpret_cast<f32x4*>(a.out + (size_t)col * a.ldo + (tile0 + r) * 16 + (l >> 4) * 4);
        const f32x4 xv = *px + s;
        *px = xv;
        q = ssq4(xv);
      }
      if (a.ssq) {
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        if (l < 16 && col < a.M) a.ssq[(size_t)col * a.np + tile0 + r] = (float)q;
      }
      continue;
    }
    if (col >= a.M) continue;
    f32x4 up = s;
    if constexpr (EPI == EPI_SWIGLU) up = kfold<KS, KS, 1>([&](int ww) { return red[ww][r][n][l + 32]; }, a.kgrp);
    epi_store<EPI>(a, tile0 + r, l, col, s, up);
  }
}

template <int KS, int RT, int NB, int EPI, int U, bool XS>
__global__ __launch_bounds__(64 * KS) void mm_kernel(MMArgs a) {
  mm_body<KS, RT, NB, EPI, U, XS>(a, blockIdx.x * RT);
}

template <int KS, int RT, int EPI, int U>
static int launch_mm_cfg(const MMArgs& a0, hipStream_t s) {
  MMArgs a = a0;
  a.kgrp = canon_kgroups(EPI, a.N, a.K);
  const int nb = (a.M + 15) / 16;
  if ((a.N / TILE_N) % RT) return -1;
  const int grid = a.N / (16 * RT);
  if (a.X == nullptr) {  // RMS_NORM on load (<= 4 tokens): per-wave LDS images of the K-slices
    const int KT = a.K / TILE_K;
    if (a.M > XS_MAX_M || !a.xf || !a.norm_w || !a.ssq || a.np * 16 != a.K || a.np > 512 || KT % KS ||
        a.K / KS > 512 || (a.K / KS) % 4)
      return -1;
    const size_t lds = (size_t)KS * a.M * (a.K / KS + 8) * 2;
    mm_kernel<KS, RT, 1, EPI, U, true><<<grid, 64 * KS, lds, s>>>(a);
    return 0;
  }
  if (nb == 1) {
    mm_kernel<KS, RT, 1, EPI, U, false><<<grid, 64 * KS, 0, s>>>(a);
  } else if (nb == 2) {
    if constexpr (KS * RT <= 32) mm_kernel<KS, RT, 2, EPI, U, false><<<grid, 64 * KS, 0, s>>>(a);
    else return -1;
  } else {
    if constexpr (KS * RT <= 16) mm_kernel<KS, RT, 4, EPI, U, false><<<grid, 64 * KS, 0, s>>>(a);
    else return -1;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Row-tile-persistent GEMV (<= 16 tokens; <= 4 with RMS_NORM on load).
//
// mm_kernel gives each work-group ONE 16-row tile, so a large N (gate/up: 1792 tiles) runs
// 7 rounds of work-groups and every round pays the ramp (first loads in flight) and, with
// RMS_NORM on load, the per-work-group norm prologue -- which is why gate/up kept a separate
// norm launch.  Here a grid of G work-groups walks tiles blockIdx.x, +G, +2G, ...: each wave's
// weight ring runs unbroken across tile seams (the next tile's first loads are issued while
// this tile's last MFMAs retire), the B fragments (the same for every tile) are loaded once
// into registers, and the RMS_NORM-on-load image is built once per work-group.  Partial tiles
// meet in a double-buffered LDS array behind a raw s_barrier that waits only for the LDS
// writes (a __syncthreads would also drain the ring); wave 0 finishes tile i while the other
// waves stream tile i+1.  Same epilogues (F32 / RESID + ssq partials / SWIGLU) and the same
// summation order per tile (K-slices in wave order) as mm_kernel, so results are bit-identical.
// ---------------------------------------------------------------------------
// EPI_ = EPI_QKV_BIAS: the EPI_QKV instance that is launched with a q/k/v bias (QB); a launch without one runs the
// EPI_QKV instance, compiled from the code it had before there was a bias
template <int KS, int NKW, int TPW, int EPI_, int U, bool XS, int KG>
__global__ __launch_bounds__(64 * KS) void mm_pers_kernel(MMArgs a) {
  constexpr bool QB = EPI_ == EPI_QKV_BIAS;
  constexpr int EPI = QB ? (int)EPI_QKV : EPI_;
  static_assert(NKW % U == 0 || (U % NKW == 0 && U / NKW <= TPW), "ring depth vs per-wave K-slice");
  constexpr int XM = XS_MAX_M;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  constexpr int KT = KS * NKW;
  const int kb = w * NKW;
  const int G = gridDim.x;

  __shared__ f32x4 red[2][KS][64];
  extern __shared__ __attribute__((aligned(16))) uint16_t xs_dyn[];

  // weights through a buffer resource sized to the matrix: the last tiles of a work-group may lie
  // past the end when TPW does not divide the tile count -- those loads return zeros and fetch
  // nothing, so every refill stays unconditional (no branch for hipcc's waitcnt merge)
  const int ntiles = a.N / TILE_N;
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(a.W), (short)0, (int)((size_t)ntiles * KT * 1024), 0x00020000);
  auto wld = [&](int i, int k) -> u32x4 {
    const unsigned off = ((unsigned)(blockIdx.x + i * G) * KT + kb + k) * 1024u + lane * 16u;
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 2 /* nt */));
  };

  const int col_raw = lane & 15;
  const int col = col_raw < a.M ? col_raw : a.M - 1;
  constexpr int xs_pitch = NKW * TILE_K + 8;
  uint16_t* xsw = xs_dyn + (size_t)w * XM * xs_pitch;

  XsRegs<XM> xr;
  if constexpr (XS) xs_load(xr, a, kb * TILE_K, NKW * TILE_K, lane);  // scale from all K/16 partials
  u32x4 ra[U];
#pragma unroll
  for (int f = 0; f < U; ++f) ra[f] = wld(f / NKW, f % NKW);
  // B fragments: registers, or -- a 16-deep K-slice (Llama-3-70B q|k|v, 16 waves: 128 VGPRs per lane)
  // with RMS_NORM on load -- read from the wave's LDS image at each MFMA (in registers they spilled
  // 11 VGPRs to scratch)
  constexpr bool BLDS = XS && NKW > 8;
  u32x4 xb[BLDS ? 1 : NKW];
  const u32x4* xp_lds = reinterpret_cast<const u32x4*>(xsw + col * xs_pitch + (lane >> 4) * 8);
  if constexpr (XS) {
    xs_build(xr, a, xsw, xs_pitch, NKW * TILE_K, lane);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's image is in LDS
    __builtin_amdgcn_wave_barrier();
    if constexpr (!BLDS) {
#pragma unroll
      for (int k = 0; k < NKW; ++k) xb[k] = xp_lds[k * 4];
    }
  } else {
    const u32x4* xp = reinterpret_cast<const u32x4*>(a.X + (size_t)col * a.ldx + (lane >> 4) * 8);
#pragma unroll
    for (int k = 0; k < NKW; ++k) xb[k] = xp[(kb + k) * 4];
  }

  // the epilogue's own loads -- the residual rows (RESID), the RoPE pairs of the q|k rows with pos /
  // slot (QKV) -- are issued when the tile starts, with its weight loads, so the tile's tail is one
  // barrier and the stores (loaded there, they were up to three dependent round trips long)
  int qpos = 0, qslot = 0;
  if constexpr (EPI == EPI_QKV) qpos = a.pos[col], qslot = a.slot[col];
  f32x4 pre[TPW];
  f32x4 qb[QB ? TPW : 1];  // QB (EPI_QKV, launched with a bias): the q|k|v bias of the tile's rows
  auto prefetch = [&](int i) {
    const int tile = min((int)blockIdx.x + i * G, ntiles - 1);
    if constexpr (EPI == EPI_QKV) pre[i] = qkv_cs(a, tile * 16 + (lane >> 4) * 4, qpos);
    if constexpr (QB) qb[i] = qkv_bias4(a, tile * 16 + (lane >> 4) * 4);
    if constexpr (EPI == EPI_RESID)
      pre[i] = *reinterpret_cast<const f32x4*>(a.out + (size_t)col * a.ldo + tile * 16 + (lane >> 4) * 4);
  };

  constexpr int LU = (EPI == EPI_SWIGLU) ? 32 : 64;
  auto finish = [&](int i) {  // after the barrier of tile i: wave 0 sums the KS partials, epilogue
    const int tile = blockIdx.x + i * G;
    if (w != 0 || tile >= ntiles) return;
    f32x4 (*rb)[64] = red[i & 1];
    const int l = lane;
    if constexpr (EPI == EPI_RESID) {
      const f32x4 s = kfold<KS, KS, KG>([&](int ww) { return rb[ww][l]; }, a.kgrp);
      double q = 0.0;
      if (col_raw < a.M) {
        f32x4* px = reinterpret_cast<f32x4*>(a.out + (size_t)col_raw * a.ldo + tile * 16 + (l >> 4) * 4);
        const f32x4 xv = pre[i] + s;
        *px = xv;
        q = ssq4(xv);
      }
      if (a.ssq) {
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        if (l < 16 && col_raw < a.M) a.ssq[(size_t)col_raw * a.np + tile] = (float)q;
      }
    } else {
      if (l >= LU || col_raw >= a.M) return;
      // partial unroll: fully unrolled, hipcc hoists all 2*KS LDS reads and spills the ring / B
      // registers around the epilogue (the reloads then wait for the whole ring)
      f32x4 s, up;
      if constexpr (EPI == EPI_SWIGLU) {  // one group (KG = 1): both sums in one interleaved chain
        static_assert(KG == 1, "gate/up folds its slices in one group");
        s = rb[0][l];
        up = rb[0][l + 32];
#pragma unroll 3
        for (int ww = 1; ww < KS; ++ww) {
          s += rb[ww][l];
          up += rb[ww][l + 32];
        }
      } else {
        // q|k|v: fully unrolled up to 2 tiles per group (8B, TinyLlama: faster, though the 8B form
        // spills 23 VGPRs), 3-way beyond (Llama-2-7B, 70B: 48 spills fully unrolled, 2.94 -> 2.66 ms
        // per one-token step; profiles/round6_wide_cfg_ab.txt)
        s = up = kfold<KS, (TPW >= 3 ? 3 : KS), KG>([&](int ww) { return rb[ww][l]; }, a.kgrp);
      }
      if constexpr (EPI == EPI_QKV) qkv_store_pre<QB>(a, tile * 16 + (l >> 4) * 4, col_raw, s, qpos, qslot, pre[i], qb[QB ? i : 0]);
      else epi_store<EPI>(a, tile, l, col_raw, s, up);
    }
  };
  auto publish = [&](int i, f32x4 acc) {
    red[i & 1][w][lane] = acc;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only: the ring stays in flight
    __builtin_amdgcn_s_barrier();
    finish(i);
  };

  // fully unrolled over the TPW tiles: a loop back-edge makes hipcc rename the ring registers
  // with moves that wait for the loads (vmcnt(0) at the loop header), draining the ring
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    prefetch(i);
#pragma unroll
    for (int k = 0; k < NKW; ++k) {
      const int f = i * NKW + k;  // flat ring position (compile-time after unrolling)
      const u32x4 bk = BLDS ? xp_lds[k * 4] : xb[BLDS ? 0 : k];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ra[f % U]),
                                                    __builtin_bit_cast(bf16x8, bk), acc, 0, 0, 0);
      if ((f + U) / NKW < TPW) ra[f % U] = wld((f + U) / NKW, (f + U) % NKW);
    }
    publish(i, acc);
  }
}

// grid = N / (16 * TPW) work-groups (every one walks exactly TPW tiles)
template <int KS, int NKW, int TPW, int EPI, int U, int KG>
static int launch_pers_kg(const MMArgs& a, hipStream_t s) {
  const int ntiles = a.N / TILE_N;
  const int grid = (ntiles + TPW - 1) / TPW;  // the last tiles of some work-groups are phantoms
  if (a.X == nullptr) {
    if (a.M > XS_MAX_M || !a.xf || !a.norm_w || !a.ssq || a.np * 16 != a.K || a.np > 512 || NKW * TILE_K > 512)
      return -1;
    const size_t lds = (size_t)KS * XS_MAX_M * (NKW * TILE_K + 8) * 2;
    if (EPI == EPI_QKV && a.qkv_bias) mm_pers_kernel<KS, NKW, TPW, EPI == EPI_QKV ? (int)EPI_QKV_BIAS : EPI, U, true, KG><<<grid, 64 * KS, lds, s>>>(a);
    else mm_pers_kernel<KS, NKW, TPW, EPI, U, true, KG><<<grid, 64 * KS, lds, s>>>(a);
  } else {
    if (EPI == EPI_QKV && a.qkv_bias) mm_pers_kernel<KS, NKW, TPW, EPI == EPI_QKV ? (int)EPI_QKV_BIAS : EPI, U, false, KG><<<grid, 64 * KS, 0, s>>>(a);
    else mm_pers_kernel<KS, NKW, TPW, EPI, U, false, KG><<<grid, 64 * KS, 0, s>>>(a);
  }
  return 0;
}

// the canonical group count as a template argument (1 for gate/up; 4 or 8 for the shapes' q|k|v and
// RESID launches, anything else read at run time)
template <int KS, int NKW, int TPW, int EPI, int U>
static int launch_pers_cfg(const MMArgs& a0, hipStream_t s) {
  MMArgs a = a0;
  a.kgrp = canon_kgroups(EPI, a.N, a.K);
  const int ntiles = a.N / TILE_N;
  if (a.K != KS * NKW * TILE_K || (size_t)ntiles * a.K * 32 >= (1ull << 31)) return -1;
  if constexpr (EPI == EPI_SWIGLU || EPI == EPI_F32) {
    return a.kgrp == 1 ? launch_pers_kg<KS, NKW, TPW, EPI, U, 1>(a, s) : -1;
  } else {
    if (a.kgrp == 4) return launch_pers_kg<KS, NKW, TPW, EPI, U, 4>(a, s);
    if (a.kgrp == 8) return launch_pers_kg<KS, NKW, TPW, EPI, U, 8>(a, s);
    return launch_pers_kg<KS, NKW, TPW, EPI, U, 0>(a, s);
  }
}

// Row-tile-persistent GEMVs for <= 16 tokens; -1 when the shape has no instantiation (callers
// fall back to launch_mm).  gate/up: K 4096 with 1025..1792 tiles (Llama-3-8B: 1792 = 256 x 7;
// Llama-2-7B's ff 11008: 1376 = 230 x 6), K 8192 with 3584 (Llama-3-70B, 256 x 14), K 2048 with 704
// (TinyLlama, 235 groups x <= 3); attn_output / ffn_down of h 4096 with K 4096 or 14336 and of
// TinyLlama's h 2048 (one tile per group, whole K-slice in flight); q|k|v of Llama-3-8B (384 tiles as
// 192 groups x 2), TinyLlama (160 x 1) and Llama-3-70B (640 as 214 x 3).  The tile-count template
// (TPW, fully unrolled) and the K-slice per wave (NKW, the ring) are compile-time; mm_kernel's K loop
// has a run-time trip count, and hipcc renames its ring across the back-edge with moves that wait for
// the loads (1-3 of its 4-deep ring in flight).  Other geometries take mm_kernel (measured: bench.py
// llama2_7b_geometry).  70B: attn_output's 16 B fragments per wave spill at 16 waves, ffn_down's 56
// do not fit.  The lm_head as a persistent
// GEMV with the output norm on load measured neutral at batch 1 (8B 2.804 vs 2.809 ms) and is not used.
bool mm_pers_supported(int epi, int M, int N, int K) {
  if (M < 1 || M > 16) return false;
  const int nt = N / TILE_N;
  if (epi == EPI_SWIGLU)
    return (K == 4096 && nt > 1024 && nt <= 1792) || (K == 8192 && nt == 3584) || (K == 2048 && nt == 704);
  if (epi == EPI_RESID)
    return (N == 4096 && (K == 4096 || K == 14336)) || (N == 2048 && (K == 2048 || K == 5632));
  if (epi == EPI_QKV)  // q|k|v of Llama-3-8B, TinyLlama, Llama-3-70B, Llama-2-7B (MHA: 768 tiles)
    return (K == 4096 && (nt == 384 || nt == 768)) || (K == 2048 && nt == 160) || (K == 8192 && nt == 640);
  return false;
}

int launch_mm_pers(int epi, const MMArgs& a, hipStream_t s) {
  if (!mm_pers_supported(epi, a.M, a.N, a.K)) return -1;
  const int ntiles = a.N / TILE_N;
  if (epi == EPI_SWIGLU) {
    if (a.K == 4096) {
      switch ((ntiles + 255) / 256) {  // tiles per work-group
        case 5: return launch_pers_cfg<16, 8, 5, EPI_SWIGLU, 8>(a, s);
        case 6: return launch_pers_cfg<16, 8, 6, EPI_SWIGLU, 8>(a, s);
        case 7: return launch_pers_cfg<16, 8, 7, EPI_SWIGLU, 8>(a, s);
      }
    }
    if (a.K == 8192 && ntiles == 3584) return launch_pers_cfg<16, 16, 14, EPI_SWIGLU, 4>(a, s);
    if (a.K == 2048 && ntiles == 704) return launch_pers_cfg<16, 4, 3, EPI_SWIGLU, 4>(a, s);
  } else if (epi == EPI_RESID) {
    if (a.N == 4096 && a.K == 4096) return launch_pers_cfg<16, 8, 1, EPI_RESID, 8>(a, s);
    if (a.N == 4096 && a.K == 14336) return launch_pers_cfg<16, 28, 1, EPI_RESID, 14>(a, s);
    if (a.N == 2048 && a.K == 2048) return launch_pers_cfg<16, 4, 1, EPI_RESID, 4>(a, s);
    if (a.N == 2048 && a.K == 5632) return launch_pers_cfg<16, 11, 1, EPI_RESID, 11>(a, s);
  } else if (epi == EPI_QKV) {
    if (a.K == 4096 && ntiles == 768) return launch_pers_cfg<16, 8, 3, EPI_QKV, 8>(a, s);  // 256 x 3
    if (a.K == 4096) return launch_pers_cfg<16, 8, 2, EPI_QKV, 8>(a, s);
    if (a.K == 2048) return launch_pers_cfg<16, 4, 1, EPI_QKV, 4>(a, s);
    if (a.K == 8192) return launch_pers_cfg<16, 16, 3, EPI_QKV, 4>(a, s);
  }
  return -1;
}

// Work-group geometry per (epilogue, token-column tiles), from tools/gemv_sweep.hip on MI355X
// (Llama-3-8B shapes; profiles/).  One column tile (<= 16 tokens): 16 waves split K, 4-deep
// ring.  Two or four tiles: several row tiles per wave so each activation fragment loaded
// from L2 feeds RT MFMAs (the activation stream otherwise exceeds the weight stream).
int launch_mm(int epi, const MMArgs& a, hipStream_t s) {
  if (a.M < 1 || a.M > MAX_ROWS || a.K % TILE_K != 0 || a.N % TILE_N != 0) return -1;
  const int ntiles = a.N / TILE_N;
  const int nb = (a.M + 15) / 16;
  if (nb == 1 || a.X == nullptr) {
    // (TinyLlama: deeper rings -- U = 11 for ffn_down, 8 for q|k|v and gate/up -- measured within
    // +-3 % of these, tools/gpu/r2ah.sh: the one-token launches there are latency-, not ring-bound)
    switch (epi) {
      case EPI_F32: return launch_mm_cfg<16, 1, EPI_F32, 4>(a, s);
      case EPI_RESID: return launch_mm_cfg<16, 1, EPI_RESID, 4>(a, s);
      case EPI_QKV:  // 16 waves = the 16 canonical K slices (round 1's 8-wave norm-on-load groups,
                     // profiles/round1_xs_probe.txt, folded two slices per wave: not batch-invariant)
        return launch_mm_cfg<16, 1, EPI_QKV, 4>(a, s);
      case EPI_SWIGLU: return launch_mm_cfg<16, 1, EPI_SWIGLU, 4>(a, s);
    }
    return -1;
  }
  if (nb == 2) {
    switch (epi) {
      case EPI_F32:
        return ntiles % 4 == 0 ? launch_mm_cfg<8, 4, EPI_F32, 4>(a, s) : launch_mm_cfg<8, 1, EPI_F32, 8>(a, s);
      case EPI_RESID: return launch_mm_cfg<4, 1, EPI_RESID, 8>(a, s);
      case EPI_QKV:
        return ntiles % 2 == 0 ? launch_mm_cfg<8, 2, EPI_QKV, 8>(a, s) : launch_mm_cfg<8, 1, EPI_QKV, 8>(a, s);
      case EPI_SWIGLU:
        return ntiles % 4 == 0 ? launch_mm_cfg<4, 4, EPI_SWIGLU, 4>(a, s) : launch_mm_cfg<4, 1, EPI_SWIGLU, 8>(a, s);
    }
    return -1;
  }
  switch (epi) {  // 3-4 column tiles (prefill chunks)
    case EPI_F32:
      return ntiles % 2 == 0 ? launch_mm_cfg<4, 2, EPI_F32, 4>(a, s) : launch_mm_cfg<4, 1, EPI_F32, 4>(a, s);
    case EPI_RESID: return launch_mm_cfg<4, 1, EPI_RESID, 8>(a, s);
    case EPI_QKV:
      return ntiles % 2 == 0 ? launch_mm_cfg<4, 2, EPI_QKV, 4>(a, s) : launch_mm_cfg<4, 1, EPI_QKV, 4>(a, s);
    case EPI_SWIGLU:
      return ntiles % 2 == 0 ? launch_mm_cfg<4, 2, EPI_SWIGLU, 4>(a, s) : launch_mm_cfg<4, 1, EPI_SWIGLU, 4>(a, s);
  }
  return -1;
}

// ---------------------------------------------------------------------------
// Wide GEMV for 17..64 token rows (32-sequence decode, prefill chunks).
//
// At 32 tokens the activation fragment per K-tile (16 tokens x 64 B per column
// tile) is as large as the weight tile, so re-reading it per wave from L2 costs
// as much as the weights (tools/gemv_sweep.hip).  Here the W waves of a
// work-group split ROWS and share one activation chunk [rows][128 k] staged in
// LDS (double-buffered, one barrier per chunk; plain register loads stay in
// flight across __syncthreads), so activation traffic drops to 16*NB/(16*W*RTW)
// of the weight traffic.  Each wave streams RTW weight tiles through a ring two
// chunks deep.  Small N is split over K across work-groups (grid.y); partial
// sums go to slabs [ksplit][token][N] that resid_norm / qkv_finish add in a
// fixed order, so results stay bit-reproducible.
// ---------------------------------------------------------------------------
// RG: the block's K range need not be whole 4-tile chunks (Llama-2's ffn_down, K 11008 = 344 tiles, split
// 8 ways = 43 tiles per block): the last chunk is partial -- its missing tiles' weight and activation
// loads re-read valid bytes (clamped) and their MFMAs are skipped (a wave-uniform branch).
template <int W, int RTW, int NB, int EPI, bool RG = false>
__global__ __launch_bounds__(64 * W) void mm_wide_kernel(MMArgs a) {
  constexpr int KCT = 4;             // K-tiles per staged activation chunk
  constexpr int KC = KCT * TILE_K;   // 128 k
  constexpr int PITCH = KC + 8;      // bf16 per LDS row: +16 B keeps fragment reads conflict-free
  constexpr int ROWS = 16 * NB;
  constexpr int SEGS = KC / 8;       // 16-B pieces per row and chunk
  constexpr int PIECES = ROWS * SEGS;
  constexpr int NT = 64 * W;
  constexpr int PPT = (PIECES + NT - 1) / NT;  // W need not divide the chunk (W = 3, 6, 7 fill 256 CUs)
  constexpr int U = 2 * KCT;         // weight ring: this chunk + the next
  __shared__ __attribute__((aligned(16))) uint16_t xs[2][ROWS][PITCH];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int KT = a.K / TILE_K;
  const int ks = blockIdx.y, nks = gridDim.y;
  const int kb = KT * ks / nks, ke = KT * (ks + 1) / nks;
  const int nkt = ke - kb;
  const int nch = RG ? (nkt + KCT - 1) / KCT : nkt / KCT;
  // a grid of ceil(tiles / (W*RTW)) groups may end in phantom waves (generic shapes): they re-read the
  // last tiles (their weight lines are in flight for the real wave anyway), stage activations and join
  // the barriers like the others, and store nothing
  const int tile_raw = (blockIdx.x * W + w) * RTW;
  const bool phantom = tile_raw + RTW > a.N / TILE_N;
  const int tile0 = phantom ? a.N / TILE_N - RTW : tile_raw;

  const u32x4* Wp[RTW];
#pragma unroll
  for (int r = 0; r < RTW; ++r) Wp[r] = reinterpret_cast<const u32x4*>(a.W) + (size_t)(tile0 + r) * KT * 64 + lane;
  auto wld = [&](int r, int t) {  // weight k-tile t of this block's range (RG: clamped into it)
    return __builtin_nontemporal_load(Wp[r] + (size_t)(kb + (RG ? min(t, nkt - 1) : t)) * 64);
  };

  // activation chunk staging: piece p -> (row, 16-B segment); rows >= M re-read row M-1 (outputs dropped)
  const u32x4* xsrc[PPT];
  int xrow[PPT], xseg[PPT], xlim[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = min(threadIdx.x + i * NT, PIECES - 1);  // ragged tail: re-stage the last piece
    xrow[i] = p / SEGS;
    xseg[i] = p % SEGS;
    const int rr = xrow[i] < a.M ? xrow[i] : a.M - 1;
    xsrc[i] = reinterpret_cast<const u32x4*>(a.X + (size_t)rr * a.ldx + (size_t)kb * TILE_K + xseg[i] * 8);
    xlim[i] = (nkt * TILE_K - 8 - xseg[i] * 8) / 8;  // RG: last 16-B piece of this row inside the range
  }
  // activation chunks are loaded TWO chunks ahead into alternating register sets: the wait for
  // chunk c+1's pieces (before its LDS store) then retires only loads issued before the weight
  // refills of chunk c+1, so 2 chunks of weight loads stay in flight across every barrier (one
  // chunk ahead, the wait drained the ring down to the current chunk's refills)
  u32x4 xr[2][PPT];
  auto load_x = [&](int set, int c) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) xr[set][i] = xsrc[i][RG ? min(c * (KC / 8), xlim[i]) : c * (KC / 8)];
  };
  auto store_x = [&](int set, int buf) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) *reinterpret_cast<u32x4*>(&xs[buf][xrow[i]][xseg[i] * 8]) = xr[set][i];
  };

  f32x4 acc[RTW][NB], tot[RTW][NB];
#pragma unroll
  for (int r = 0; r < RTW; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[r][n] = tot[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // canonical K slices (batch invariance): the MFMA chain restarts from zero at each of
  // the 16 slice starts [KT*j/16) and is added to tot at the slice's end -- the partials the <= 16-row
  // GEMVs form with one slice per wave and fold in the same order (kfold).  This block's K range is
  // slices [16 ks / nks, 16 (ks + 1) / nks) (nks divides 16).
  // With K < 512 some slices are empty (KT < 16): the <= 16-row fold adds their zero partials, which
  // leaves every sum unchanged, so they are skipped here (jend = end of the next non-empty slice).
  int jn = (16 * ks) / nks, jend = (KT * (jn + 1)) >> 4;
  while (jend <= kb && jn < 15) jend = (KT * (++jn + 1)) >> 4;
  if (a.kgrp < 0) jn = 15, jend = ke;  // full chain (prefill order): one fold, at the end
  bool have = false;  // tot holds a slice sum
  auto slice_fold = [&](int kg) {
    if (kg + 1 == jend) {
#pragma unroll
      for (int r = 0; r < RTW; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          tot[r][n] = have ? tot[r][n] + acc[r][n] : acc[r][n];
          acc[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      have = true;
      do jend = (KT * (++jn + 1)) >> 4;
      while (jend == kg + 1 && jn < 15);
    }
  };

  u32x4 ra[U][RTW];
  load_x(0, 0);
  load_x(1, nch > 1 ? 1 : 0);
#pragma unroll
  for (int u = 0; u < KCT; ++u)
#pragma unroll
    for (int r = 0; r < RTW; ++r) ra[u][r] = wld(r, u);
  if (nch > 1) {
#pragma unroll
    for (int u = 0; u < KCT; ++u)
#pragma unroll
      for (int r = 0; r < RTW; ++r) ra[KCT + u][r] = wld(r, KCT + u);
  }
  store_x(0, 0);
  __syncthreads();

  // one chunk: H = ring half = c & 1 (compile time), REFILL = load the chunk two ahead into that
  // half; activation set H receives chunk c+2, set 1-H (chunk c+1) goes to LDS at the end
  auto chunk = [&](auto Hc, auto Rc, int c) {
    constexpr int H = decltype(Hc)::value;
    constexpr bool REFILL = decltype(Rc)::value;
    const int buf = c & 1;
    load_x(H, c + 2 < nch ? c + 2 : nch - 1);  // past the end: re-read the last chunk (unconditional)
#pragma unroll
    for (int kk = 0; kk < KCT; ++kk) {
      const bool live = !RG || c * KCT + kk < nkt;  // wave-uniform
      if (live) {
        u32x4 xb[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n)
          xb[n] = *reinterpret_cast<const u32x4*>(&xs[buf][n * 16 + (lane & 15)][kk * 32 + (lane >> 4) * 8]);
#pragma unroll
        for (int r = 0; r < RTW; ++r)
#pragma unroll
          for (int n = 0; n < NB; ++n)
            acc[r][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ra[H * KCT + kk][r]),
                                                                 __builtin_bit_cast(bf16x8, xb[n]), acc[r][n], 0, 0, 0);
      }
      if constexpr (REFILL) {
#pragma unroll
        for (int r = 0; r < RTW; ++r) ra[H * KCT + kk][r] = wld(r, (c + 2) * KCT + kk);
      }
      if (live) slice_fold(kb + c * KCT + kk);
    }
    store_x(1 - H, buf ^ 1);
    __syncthreads();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using T = std::true_type;
  using F = std::false_type;
  int c = 0;
  for (; c + 3 < nch; c += 2) {
    chunk(I0{}, T{}, c);
    chunk(I1{}, T{}, c + 1);
  }
  const int rem = nch - c;
  if (rem == 3) {
    chunk(I0{}, T{}, c);
    chunk(I1{}, F{}, c + 1);
    chunk(I0{}, F{}, c + 2);
  } else if (rem == 2) {
    chunk(I0{}, F{}, c);
    chunk(I1{}, F{}, c + 1);
  } else if (rem == 1) {
    chunk(I0{}, F{}, c);
  }

  // epilogue straight from registers: this wave owns whole tiles (over this block's K range)
#pragma unroll
  for (int r = 0; r < RTW; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const f32x4 s = tot[r][n];
      f32x4 up = s;
      if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) up[i] = __shfl_xor(s[i], 32);
      }
      const int col = n * 16 + (lane & 15);
      if (phantom || col >= a.M || (EPI == EPI_SWIGLU && lane >= 32)) continue;
      if constexpr (EPI == EPI_SLAB) {
        const int row = (tile0 + r) * 16 + (lane >> 4) * 4;
        *reinterpret_cast<f32x4*>(a.out + (size_t)ks * a.slab_stride + (size_t)col * a.ldo + row) = s;
      } else {
        epi_store<EPI>(a, tile0 + r, lane, col, s, up);
      }
    }
}

// q/k/v split-K partials -> sum in slab order -> RoPE + q / KV-cache stores.  A work-group finishes
// 32 feature quads (128 features) of 64 token rows, each thread one quad of 8 rows: a 128-byte line of
// the tile-ordered K / V cache holds 8 positions x 8 dims (device_common.h kv_k_off / kv_v_off), so
// for the positions of a prompt chunk every line is written by ONE work-group instead of by up to 8 of
// the launch -- lines written in parts by several work-groups at once were what differed run to run
// when another process shared the GPU (profiles/round4_gpu_sharing.txt)
__global__ __launch_bounds__(256) void qkv_finish_kernel(MMArgs a, const float* slabs, int nslab, size_t stride) {
  const int N = a.n_q + 2 * a.n_kv;
  const int quads = N / 4, qblocks = (quads + 31) / 32;
  const int cb = blockIdx.x / qblocks, qb = blockIdx.x % qblocks;
  const int q = qb * 32 + (threadIdx.x & 31);
  if (q >= quads) return;
  const int row = q * 4;
  const int c0 = cb * 64 + (threadIdx.x >> 5) * 8;
  for (int c = 0; c < 8; ++c) {
    const int col = c0 + c;
    if (col >= a.M) break;
    f32x4 s = *reinterpret_cast<const f32x4*>(slabs + (size_t)col * N + row);
    for (int k = 1; k < nslab; ++k) s += *reinterpret_cast<const f32x4*>(slabs + k * stride + (size_t)col * N + row);
    qkv_store(a, row, col, s);
  }
}

void launch_qkv_finish(const MMArgs& a, const float* slabs, int nslab, size_t stride, hipStream_t s) {
  const int quads = (a.n_q + 2 * a.n_kv) / 4;
  const int grid = (a.M + 63) / 64 * ((quads + 31) / 32);
  qkv_finish_kernel<<<grid, 256, 0, s>>>(a, slabs, nslab, stride);
}

void launch_resid_norm(uint16_t* y, int ldy, float* x, const float* slabs, int nslab, size_t stride, const float* w,
                       int M, int n, float eps, hipStream_t s) {
  launch_norm_impl(y, ldy, x, slabs, nslab, stride, w, nullptr, M, n, eps, s);
}

template <int W, int RTW, int EPI>
static int launch_wide_cfg(const MMArgs& a, int ksplit, hipStream_t s, bool ragged_n = false) {
  const int ntiles = a.N / TILE_N;
  const int KT = a.K / TILE_K;
  if ((!ragged_n && ntiles % (W * RTW)) || ntiles < W * RTW || KT < ksplit * 4) return -1;
  dim3 grid((ntiles + W * RTW - 1) / (W * RTW), ksplit);
  const int nb = (a.M + 15) / 16;
  if (KT % (ksplit * 4) == 0) {
    if (nb <= 2) mm_wide_kernel<W, RTW, 2, EPI><<<grid, 64 * W, 0, s>>>(a);
    else mm_wide_kernel<W, RTW, 4, EPI><<<grid, 64 * W, 0, s>>>(a);
  } else {  // K ranges that are not whole chunks (generic shapes)
    if (nb <= 2) mm_wide_kernel<W, RTW, 2, EPI, true><<<grid, 64 * W, 0, s>>>(a);
    else mm_wide_kernel<W, RTW, 4, EPI, true><<<grid, 64 * W, 0, s>>>(a);
  }
  return 0;
}

// largest power-of-two split <= target whose K ranges hold at least 4 chunks (ranges that are not
// whole chunks run the RG form of mm_wide_kernel); the canonical K grouping requires it to divide 16
static int pick_ksplit(int KT, int target) {
  int k = 1;
  while (k * 2 <= target && k * 2 <= 16 && KT >= k * 2 * 16) k *= 2;
  return KT >= k * 4 ? k : 0;
}

// K split (work-groups along K, partial slabs) of the 17..64-row q|k|v / RESID launches -- a function
// of the shape only; it is also the canonical K grouping of every bf16 GEMV (canon_kgroups).
// Partial slabs are re-read by the reduce+norm that follows: 4 at most, 8 for ffn_down.
// cfg: 0: W4 RTW2 (qkv), 1: W2 RTW1 (K <= 8192), 2: W4 RTW1, 3: W3 RTW1 (qkv), 4: W4 RTW2 split 8
static int wide_split(int epi, int N, int K, int* cfg_out) {
  const int ntiles = N / TILE_N, KT = K / TILE_K;
  int cfg, groups;
  if (epi == EPI_QKV && ntiles % 3 == 0) cfg = 3, groups = ntiles / 3;
  else if (epi == EPI_RESID && K > 8192 && ntiles % 8 == 0 && ntiles / 8 <= 64) cfg = 4, groups = ntiles / 8;
  else if (epi == EPI_QKV && ntiles % 8 == 0) cfg = 0, groups = ntiles / 8;
  else if (K <= 8192 && ntiles % 2 == 0) cfg = 1, groups = ntiles / 2;
  else cfg = 2, groups = ntiles / 4;
  // split targets measured in round 5 (profiles/round5_wide_variants_rejected.txt D): q|k|v 4, attn_output 4,
  // ffn_down 8 beat every 2 / 4 / 8 combination tried
  int target = cfg == 4 ? 8 : (cfg == 3 || cfg == 1) ? 4
                            : std::min(4, std::max(1, (256 + groups - 1) / std::max(1, groups)));
  // A/B (read once): the split targets for q|k|v and RESID launches.  The canonical K grouping follows
  // the split (canon_kgroups calls this), so every row count changes together: results stay invariant
  static const int t_qkv = getenv("MX_WIDE_QKV_SPLIT") ? atoi(getenv("MX_WIDE_QKV_SPLIT")) : 0;
  static const int t_res = getenv("MX_WIDE_RESID_SPLIT") ? atoi(getenv("MX_WIDE_RESID_SPLIT")) : 0;
  if (epi == EPI_QKV && t_qkv > 0) target = t_qkv;
  if (epi == EPI_RESID && t_res > 0) target = t_res;
  // the engine's slab buffer and the attention's FIN path hold ATTN_FIN_MAXSLAB partials: no override above it
  target = std::min(target, ATTN_FIN_MAXSLAB);
  if (cfg_out) *cfg_out = cfg;
  return KT % 4 ? 0 : pick_ksplit(KT, target);
}

int canon_kgroups(int epi, int N, int K) {
  if (epi != EPI_QKV && epi != EPI_RESID) return 1;  // gate/up and the lm_head: one K range per 17..64-row tile
  const int g = wide_split(epi, N, K, nullptr);
  return g > 0 ? g : 1;
}

// Geometry from tools/gemv_sweep.hip (wide) on MI355X, Llama-3-8B shapes at 32 rows
// (profiles/round1_gemv_sweep_wide.txt): two row tiles per wave, K split until ~256 work-groups.
int launch_mm_wide(int epi, const MMArgs& a0, float* slabs, size_t slab_stride, hipStream_t s, bool qkv_finish,
                   bool full_chain) {
  MMArgs a = a0;
  a.kgrp = full_chain ? -1 : 0;
  if (a.M < 1 || a.M > MAX_ROWS || a.K % TILE_K != 0 || a.N % TILE_N != 0 || !a.X) return -1;
  const int ntiles = a.N / TILE_N, KT = a.K / TILE_K;
  if (KT % 4) return -1;
  // work-groups per launch are sized to the 256 CUs (tools/gemv_sweep.hip "odd" sweep,
  // profiles/round1_gemv_sweep_odd.txt): 7 or 3 waves per group where 8/4 would leave CUs idle
  switch (epi) {
    // shapes without a measured geometry (round 6): the largest row-tile grouping that
    // still gives >= 256 work-groups, so Llama-2-7B's gate/up (1376 tiles) runs 344 groups, not 172
    case EPI_F32: {
      static const int fc = getenv("MX_WIDE_F32_CFG") ? atoi(getenv("MX_WIDE_F32_CFG")) : 0;  // A/B (read once)
      if (fc == 1 && ntiles % 16 == 0) return launch_wide_cfg<8, 2, EPI_F32>(a, 1, s) ? -1 : 1;
      if (fc == 2 && ntiles % 8 == 0) return launch_wide_cfg<8, 1, EPI_F32>(a, 1, s) ? -1 : 1;
      if (fc == 3 && ntiles % 8 == 0) return launch_wide_cfg<4, 2, EPI_F32>(a, 1, s) ? -1 : 1;
      if (fc == 4) return launch_wide_cfg<7, 1, EPI_F32>(a, 1, s, true) ? -1 : 1;
      if (ntiles % 6 == 0) return launch_wide_cfg<3, 2, EPI_F32>(a, 1, s) ? -1 : 1;
      if (ntiles % 16 == 0 && ntiles / 16 >= 256) return launch_wide_cfg<8, 2, EPI_F32>(a, 1, s) ? -1 : 1;
      if (ntiles % 8 == 0 && ntiles / 8 >= 256) return launch_wide_cfg<4, 2, EPI_F32>(a, 1, s) ? -1 : 1;
      if (ntiles % 4 == 0) return launch_wide_cfg<4, 1, EPI_F32>(a, 1, s) ? -1 : 1;
      return launch_wide_cfg<2, 1, EPI_F32>(a, 1, s) ? -1 : 1;
    }
    case EPI_SWIGLU: {
      static const int sc = getenv("MX_WIDE_SWIGLU_CFG") ? atoi(getenv("MX_WIDE_SWIGLU_CFG")) : 0;  // A/B
      if (sc == 1) return launch_wide_cfg<4, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (sc == 2) return launch_wide_cfg<2, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (sc == 3) return launch_wide_cfg<8, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (sc == 4) return launch_wide_cfg<3, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (ntiles % 7 == 0 && ntiles / 7 >= 128) return launch_wide_cfg<7, 1, EPI_SWIGLU>(a, 1, s) ? -1 : 1;
      if (ntiles % 8 == 0 && ntiles / 8 >= 256) return launch_wide_cfg<4, 2, EPI_SWIGLU>(a, 1, s) ? -1 : 1;
      // otherwise one group per CU with as few waves as cover the tiles (Llama-2-7B: 1376 tiles -> 230
      // groups of 6, the last with 2 phantom waves; TinyLlama: 704 -> 235 of 3)
      const int wneed = (ntiles + 255) / 256;
      if (wneed <= 3) return launch_wide_cfg<3, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (wneed <= 4) return launch_wide_cfg<4, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      if (wneed <= 6) return launch_wide_cfg<6, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
      return launch_wide_cfg<8, 1, EPI_SWIGLU>(a, 1, s, true) ? -1 : 1;
    }
    case EPI_QKV:
    case EPI_RESID: {
      int cfg;
      int ksplit = wide_split(epi, a.N, a.K, &cfg);
      if (ksplit <= 0) return -1;
      if (full_chain) {  // one K range per output (the GEMM's order): the narrowest groups for parallelism
        ksplit = 1;
        cfg = (epi == EPI_QKV && ntiles % 3 == 0) ? 3 : ntiles % 2 == 0 ? 1 : 2;
      }
      MMArgs p = a;
      p.out = slabs;
      p.ldo = a.N;
      p.slab_stride = slab_stride;
      const int rc = (cfg == 0 || cfg == 4) ? launch_wide_cfg<4, 2, EPI_SLAB>(p, ksplit, s)
                   : cfg == 1 ? launch_wide_cfg<2, 1, EPI_SLAB>(p, ksplit, s)
                   : cfg == 3 ? launch_wide_cfg<3, 1, EPI_SLAB>(p, ksplit, s)
                              : launch_wide_cfg<4, 1, EPI_SLAB>(p, ksplit, s);
      if (rc) return -1;
      if (epi == EPI_QKV && qkv_finish) launch_qkv_finish(a, slabs, ksplit, slab_stride, s);
      return ksplit;
    }
  }
  return -1;
}

bool mm_can_norm_on_load(int M, int K) {
  constexpr int KS = 16;  // launch_mm's one-column-tile geometry
  return M <= XS_MAX_M && K % (32 * KS) == 0 && K / KS <= 512 && K / 16 <= 512;
}

// ---------------------------------------------------------------------------
// Attention for one query token per row (decode, and prefill rows alike):
// KQ = f16(q).K -> SOFT_MAX_EXT(scale, causal) -> f16(P).V   
//
// One work-group (8 waves) per (kv head, row); the G query heads of the GQA
// group are the rows of v_mfma_f32_16x16x32_f16 tiles, so q, K, P and V enter
// the matrix cores as f16 -- the same roundings ggml's f16 dot products apply.
// Wave w walks 32-position chunks w, w+8, ... with an online softmax; the 8
// partial (m, l, O) are merged through LDS and the normalised output is
// written as bf16 (the rounding ggml applies before attn_output).  K is stored
// [pos][d] (B operand of QK^T = contiguous 16 B per lane) and V transposed
// [d][pos] (B operand of P.V = contiguous 16 B per lane).
// ---------------------------------------------------------------------------
}  // namespace mx
#include "attn_body.h"
namespace mx {

template <int D, int G, int NW, bool FIN, int MS, bool QB>
__global__ __launch_bounds__(64 * NW) void attn_decode_kernel(AttnArgs a) {
  attn_decode_body<D, G, NW, FIN, MS, QB>(a, blockIdx.x, blockIdx.y);
}
// QB: the FIN instance that adds the q/k/v bias; a launch without one runs the instance without
template <int D, int G, int NW, bool FIN, int MS>
static void launch_attn_g(const AttnArgs& a, dim3 grid, hipStream_t s) {
  if (FIN && a.qkv_bias) attn_decode_kernel<D, G, NW, FIN, MS, FIN><<<grid, 64 * NW, 0, s>>>(a);
  else attn_decode_kernel<D, G, NW, FIN, MS, false><<<grid, 64 * NW, 0, s>>>(a);
}

template <int D, bool FIN, int NW, int MS = ATTN_FIN_MAXSLAB>
static void launch_attn_dfw(const AttnArgs& a, hipStream_t s) {
  dim3 grid(a.n_head_kv, a.M);
  switch (a.n_head / a.n_head_kv) {
    case 1: launch_attn_g<D, 1, NW, FIN, MS>(a, grid, s); break;
    case 2: launch_attn_g<D, 2, NW, FIN, MS>(a, grid, s); break;
    case 4: launch_attn_g<D, 4, NW, FIN, MS>(a, grid, s); break;
    case 5: launch_attn_g<D, 5, NW, FIN, MS>(a, grid, s); break;  // Qwen2.5-14B / 32B
    case 6: launch_attn_g<D, 6, NW, FIN, MS>(a, grid, s); break;  // Qwen2.5-1.5B
    case 7: launch_attn_g<D, 7, NW, FIN, MS>(a, grid, s); break;  // Qwen2.5-0.5B / 7B
    case 8: launch_attn_g<D, 8, NW, FIN, MS>(a, grid, s); break;
  }
}

// Waves per work-group: 8 for decode-sized grids (<= 64 rows: n_head_kv x M work-groups do not fill
// the chip, so each work-group splits its positions over more waves); 4 once the grid alone fills
// it (>= 128 rows, e.g. a prefill chunk whose rows are not 16-position blocks).  Measured in round 2
// (profiles/round2_attention.txt): 16 waves was slower at every size, 4 waves 2.3x faster at 4096
// rows and 7-20% slower at 1-32 rows.
// MHA models (one query head per kv head, Llama-2-7B: 32 kv heads) run 4 waves at every decode row count:
// a work-group then holds a single query row, and at decode context lengths most of 8 waves had no
// chunk (round 6: 18.9 us per 32-row layer of Llama-2-7B's geometry with 8).  The wave count is a
// function of the model, never of the row count, so the chunk-to-wave assignment and the merge order
// -- the attention's summation order -- stay the same at every batch size (batch invariance).
template <int D>
static void launch_attn_d(const AttnArgs& a, hipStream_t s) {
  static const bool nw4 = getenv("MX_ATTN_NW4") != nullptr;  // A/B: 4 waves for every model (read once)
  const bool mha = a.n_head == a.n_head_kv || nw4;
  if (a.slabs && mha && a.nslab <= 4) launch_attn_dfw<D, true, 4, 4>(a, s);
  else if (a.slabs && mha) launch_attn_dfw<D, true, 4>(a, s);  // MS = 4 would drop slabs 4..7
  else if (a.slabs && a.nslab <= 4) launch_attn_dfw<D, true, 8, 4>(a, s);  // Llama-3-8B's q|k|v splits K 4 ways
  else if (a.slabs) launch_attn_dfw<D, true, 8>(a, s);
  else if (a.M >= 128 || mha) launch_attn_dfw<D, false, 4>(a, s);
  else launch_attn_dfw<D, false, 8>(a, s);
}

void launch_attention(const AttnArgs& a, hipStream_t s) {
  if (a.head_dim == 64)
    launch_attn_d<64>(a, s);
  else
    launch_attn_d<128>(a, s);
}

// ---------------------------------------------------------------------------
// greedy sampler: argmax over the vocabulary, ties -> lowest id  
// ---------------------------------------------------------------------------
constexpr int ARGMAX_CHUNKS = 64;

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__global__ __launch_bounds__(256) void argmax_stage1(const float* logits, int ldl, int V, float* ws_val,
                                                     int* ws_idx) {
  const int ch = blockIdx.x, c = blockIdx.y;
  const int per = (V + ARGMAX_CHUNKS - 1) / ARGMAX_CHUNKS;
  const int b = ch * per, e = min(V, b + per);
  const float* lr = logits + (size_t)c * ldl;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = b + threadIdx.x; i < e; i += 256) better(bv, bi, lr[i], i);
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(bv, o);
    int oi = __shfl_xor(bi, o);
    better(bv, bi, ov, oi);
  }
  __shared__ float sv[4];
  __shared__ int si[4];
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = bv;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) better(bv, bi, sv[k], si[k]);
    ws_val[c * ARGMAX_CHUNKS + ch] = bv;
    ws_idx[c * ARGMAX_CHUNKS + ch] = bi;
  }
}

__global__ void argmax_stage2(const float* ws_val, const int* ws_idx, int* tok_out, int* ids_next, int* pos_next,
                              int* hist, int hist_stride, int* hist_count, int max_hist) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float bv = ws_val[c * ARGMAX_CHUNKS + lane];
  int bi = ws_idx[c * ARGMAX_CHUNKS + lane];
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(bv, o);
    int oi = __shfl_xor(bi, o);
    better(bv, bi, ov, oi);
  }
  if (lane == 0) {
    if (bi == 0x7fffffff) bi = 0;  // all-NaN row
    if (tok_out) tok_out[c] = bi;
    if (ids_next) ids_next[c] = bi;
    if (pos_next) pos_next[c] += 1;
    if (hist) {
      int n = hist_count[c];
      if (n < max_hist) hist[(size_t)c * hist_stride + n] = bi;
      hist_count[c] = n + 1;
    }
  }
}

// ---------------------------------------------------------------------------
// top-k candidates of each logits row, for the sampler chain (llama.cpp top_k, then top_p / min_p /
// temperature / draw on the host over k values instead of a sort of the whole vocabulary).  Order:
// value descending, ties by lower id -- the host sampler's comparator.  Selection by K passes of
// "largest element strictly after the previous pick in that order" (no mask, no sort).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool topk_after(float v, int i, float pv, int pi) {  // (v,i) comes after (pv,pi)
  return v < pv || (v == pv && i > pi);
}
__device__ __forceinline__ bool topk_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

template <int NT>
__device__ void topk_select(const float* val, const int* idx, int n, int K, float* ov, int* oi, float* sv, int* si) {
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < n; j += NT) {
      const float v = val[j];
      const int i = idx ? idx[j] : j;
      if (topk_after(v, i, pv, pi) && topk_better(v, i, bv, bi)) bv = v, bi = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o);
      const int i2 = __shfl_xor(bi, o);
      if (topk_better(v2, i2, bv, bi)) bv = v2, bi = i2;
    }
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __syncthreads();
    bv = sv[0];
    bi = si[0];
#pragma unroll
    for (int w2 = 1; w2 < NT / 64; ++w2)
      if (topk_better(sv[w2], si[w2], bv, bi)) bv = sv[w2], bi = si[w2];
    __syncthreads();
    if (threadIdx.x == 0) ov[k] = bv, oi[k] = bi;
    pv = bv;
    pi = bi;
  }
}

// stage 1: block b of row c selects the top K of its slice; stage 2: one block per row merges
__global__ __launch_bounds__(256) void topk_stage1(const float* logits, int ldl, int V, int K, float* cv, int* ci) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int c = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  const int lo = (int)((long long)V * b / nb), hi = (int)((long long)V * (b + 1) / nb);
  __shared__ int ids[4096];
  __shared__ float vals[4096];
  for (int j = threadIdx.x; j < hi - lo; j += 256) vals[j] = logits[(size_t)c * ldl + lo + j], ids[j] = lo + j;
  __syncthreads();
  topk_select<256>(vals, ids, hi - lo, K, cv + ((size_t)c * nb + b) * K, ci + ((size_t)c * nb + b) * K, sv, si);
}

__global__ __launch_bounds__(256) void topk_stage2(const float* cv, const int* ci, int n, int K, float* ov, int* oi) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int c = blockIdx.x;
  topk_select<256>(cv + (size_t)c * n, ci + (size_t)c * n, n, K, ov + (size_t)c * K, oi + (size_t)c * K, sv, si);
}

int launch_topk(const float* logits, int ldl, int M, int V, int K, float* ws_val, int* ws_idx, float* out_val,
                int* out_idx, hipStream_t s) {
  if (K < 1 || K > TOPK_MAX || M < 1) return -1;
  const int nb = std::min(64, std::max(1, (V + 2047) / 2048));
  if ((V + nb - 1) / nb > 4096) return -1;
  topk_stage1<<<dim3(nb, M), 256, 0, s>>>(logits, ldl, V, K, ws_val, ws_idx);
  topk_stage2<<<M, 256, 0, s>>>(ws_val, ws_idx, nb * K, K, out_val, out_idx);
  return 0;
}

void launch_argmax(const float* logits, int ldl, int M, int V, float* ws_val, int* ws_idx, int* tok_out,
                   int* ids_next, int* pos_next, int* hist, int hist_stride, int* hist_count, int max_hist,
                   hipStream_t s) {
  argmax_stage1<<<dim3(ARGMAX_CHUNKS, M), 256, 0, s>>>(logits, ldl, V, ws_val, ws_idx);
  argmax_stage2<<<M, 64, 0, s>>>(ws_val, ws_idx, tok_out, ids_next, pos_next, hist, hist_stride, hist_count,
                                 max_hist);
}

// ---------------------------------------------------------------------------
// Prompt-lookup speculative decoding (llama-cpp-python's LlamaPromptLookupDecoding).
// Request r of a speculating round owns rows [r(1+D), (r+1)(1+D)) of the forward: row 0 is its last
// token at its position p, rows 1..D the draft at p+1..p+D, all in the request's KV slot.
//
// spec_draft_kernel, one work-group per request: find_candidate_pred_tokens over ctx_tok[r][0..len).
// For g = min(ng, len-1) .. 1 the key is the last g tokens; thread t tests the windows t, t+256, ... of
// [0, len-g) in increasing order and keeps its first match, the work-group takes the minimum (wave
// butterfly, then LDS) -- the lowest matching index, whose continuation is never empty (i + g < len).
// The draft is ctx_tok[i+g .. min(i+g+d, len)), d = the request's own num_pred_tokens (<= D).
// Rows past n_draft repeat the last draft token (the last context token when n_draft = 0): they are
// forwarded but never accepted, and their K/V lands at positions past the sequence's end.  That is
// harmless: a position is read by attention only from rows at or after it, and the next step, starting
// at its new p <= the old p + n_draft + 1, rewrites every position p..p+D in its q|k|v epilogue before
// its attention launch reads any of them -- so no stale K/V past the accepted prefix is ever read.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spec_draft_kernel(const int* ctx_tok, int ctx_stride, const int* ctx_len,
                                                         const int* par, int D, int* ids, int* pos, int* slot,
                                                         int* n_draft) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int* tok = ctx_tok + (size_t)r * ctx_stride;
  const int len = ctx_len[r], d = min(par[2 * r], D), ng = par[2 * r + 1];
  const int base = r * (1 + D);
  __shared__ int sm[4];
  int found = 0x7fffffff, g = min(ng, len - 1);
  for (; g >= 1; --g) {
    const int* key = tok + (len - g);
    int best = 0x7fffffff;
    for (int i = tid; i < len - g; i += 256) {
      int k = 0;
      while (k < g && tok[i + k] == key[k]) ++k;
      if (k == g) {
        best = i;
        break;
      }
    }
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if ((tid & 63) == 0) sm[tid >> 6] = best;
    __syncthreads();
    found = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
    __syncthreads();
    if (found != 0x7fffffff) break;
  }
  const bool hit = found != 0x7fffffff;
  const int start = hit ? found + g : 0;
  const int n = hit ? max(0, min(d, len - start)) : 0;
  if (tid < D) {
    const int p = pos[base], sl = slot[base];
    const int t = tid < n ? tok[start + tid] : (n > 0 ? tok[start + n - 1] : tok[len - 1]);
    ids[base + 1 + tid] = t;
    pos[base + 1 + tid] = p + 1 + tid;
    slot[base + 1 + tid] = sl;
  }
  if (tid == 0) n_draft[r] = n;
}

// spec_accept_kernel, one wave per request, after argmax_stage1 over all R(1+D) logits rows: finishes
// the argmax of rows 0..n_draft exactly as argmax_stage2 (ties -> lowest id), a = the number of leading
// j < n_draft with argmax[j] == draft[j], and emits argmax[0..a]: appended to the round's history and
// to ctx_tok[r], argmax[a] becomes row 0's next id, position and length advance by a + 1.  cnt[r] =
// {steps, drafted, accepted} of the round so far; step_log[r][step] = {n_draft, a} lets the host count
// only the steps whose tokens it keeps.
__global__ __launch_bounds__(64) void spec_accept_kernel(const float* ws_val, const int* ws_idx, int D, int* ids,
                                                        int* pos, const int* n_draft, int* ctx_tok, int ctx_stride,
                                                        int* ctx_len, int* hist, int hist_stride, int* hist_count,
                                                        int* cnt, int* step_log, int max_steps) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int base = r * (1 + D), nd = min(n_draft[r], D);
  int mine = 0, a = 0;
  bool ok = true;
  for (int j = 0; j <= nd; ++j) {
    const int c = base + j;
    float bv = ws_val[c * ARGMAX_CHUNKS + lane];
    int bi = ws_idx[c * ARGMAX_CHUNKS + lane];
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(bv, o);
      int oi = __shfl_xor(bi, o);
      better(bv, bi, ov, oi);
    }
    if (bi == 0x7fffffff) bi = 0;  // all-NaN row
    if (lane == j) mine = bi;
    if (j < nd) {
      ok = ok && bi == ids[base + 1 + j];
      if (ok) a = j + 1;
    }
  }
  const int len = ctx_len[r], hc = hist_count[r];
  __syncthreads();  // every lane has read the drafts / length / count before any of them is rewritten
  if (lane <= a) {
    if (hc + lane < hist_stride) hist[(size_t)r * hist_stride + hc + lane] = mine;
    if (len + lane < ctx_stride) ctx_tok[(size_t)r * ctx_stride + len + lane] = mine;
  }
  if (lane == a) ids[base] = mine;
  if (lane == 0) {
    pos[base] += a + 1;
    ctx_len[r] = len + a + 1;
    hist_count[r] = hc + a + 1;
    const int st = cnt[3 * r];
    if (step_log && st < max_steps) {
      step_log[(r * max_steps + st) * 2] = nd;
      step_log[(r * max_steps + st) * 2 + 1] = a;
    }
    cnt[3 * r] = st + 1;
    cnt[3 * r + 1] += nd;
    cnt[3 * r + 2] += a;
  }
}

void launch_spec_draft(const int* ctx_tok, int ctx_stride, const int* ctx_len, const int* par, int R, int D, int* ids,
                       int* pos, int* slot, int* n_draft, hipStream_t s) {
  spec_draft_kernel<<<R, 256, 0, s>>>(ctx_tok, ctx_stride, ctx_len, par, D, ids, pos, slot, n_draft);
}

void launch_spec_accept(const float* ws_val, const int* ws_idx, int R, int D, int* ids, int* pos, const int* n_draft,
                        int* ctx_tok, int ctx_stride, int* ctx_len, int* hist, int hist_stride, int* hist_count,
                        int* cnt, int* step_log, int max_steps, hipStream_t s) {
  spec_accept_kernel<<<R, 64, 0, s>>>(ws_val, ws_idx, D, ids, pos, n_draft, ctx_tok, ctx_stride, ctx_len, hist,
                                      hist_stride, hist_count, cnt, step_log, max_steps);
}

void launch_argmax_stage1(const float* logits, int ldl, int M, int V, float* ws_val, int* ws_idx, hipStream_t s) {
  argmax_stage1<<<dim3(ARGMAX_CHUNKS, M), 256, 0, s>>>(logits, ldl, V, ws_val, ws_idx);
}

// ---------------------------------------------------------------------------
// Device sampling chain.  penalty_kernel: llama.cpp's penalties sampler over the row's window (the
// last last_n tokens of prompt + output: the n_win tokens given at the start of the run, then the
// tokens this run generated, hist[0..hist_count)).  Lane j holds window token j; the lane holding a
// token's first occurrence counts its occurrences and rewrites that one logit: divided by `repeat`
// when positive (multiplied otherwise), then count*freq + presence subtracted -- engine.cpp
// sample_host's arithmetic, in the same order.
// ---------------------------------------------------------------------------
// side_tok / side_val (optional, [M][SAMP_WIN]): the rewriting lane first saves (token, raw logit) there
// (-1 in every other lane), so logprob_gather_kernel still finds the raw value of a penalised token.
__global__ __launch_bounds__(64) void penalty_kernel(float* logits, int ldl, const SampRow* samp, const int* hist,
                                                     int hist_stride, const int* hist_count, int* side_tok,
                                                     float* side_val) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const SampRow& sp = samp[c];
  if (side_tok) side_tok[c * SAMP_WIN + lane] = -1;
  if (sp.last_n <= 0 || (sp.repeat == 1.0f && sp.freq == 0.0f && sp.presence == 0.0f)) return;
  const int nh = hist ? hist_count[c] : 0;
  const int total = sp.n_win + nh;
  const int n = min(sp.last_n, total);
  const int j = total - n + lane;
  int t = -1;
  if (lane < n) t = j < sp.n_win ? sp.win[j] : hist[(size_t)c * hist_stride + (j - sp.n_win)];
  int count = 0;
  bool first = lane < n;
  for (int o = 0; o < 64; ++o) {
    const int u = __shfl(t, o);
    count += (u == t && t >= 0) ? 1 : 0;
    if (o < lane && u == t) first = false;
  }
  if (first && t >= 0) {
    float* lp = logits + (size_t)c * ldl + t;
    float v = *lp;
    if (side_tok) side_tok[c * SAMP_WIN + lane] = t, side_val[c * SAMP_WIN + lane] = v;
    if (sp.repeat != 1.0f) v = v <= 0.f ? v * sp.repeat : v / sp.repeat;
    // one fused multiply-add, as this line always compiled for the device: said explicitly so that the host
    // sampler's rewrite_host (fmaf) and the device agree to the bit
    *lp = v - __fmaf_rn((float)count, sp.freq, sp.presence);
  }
}

// one wave per row over its top-k candidates: lane 0 runs samp_pick (the host sampler's code) on
// the k <= 64 candidates; draw index = draw0 + tokens this run already generated for the row
__global__ __launch_bounds__(64) void sample_kernel(const float* tk_val, const int* tk_idx, int K, const SampRow* samp,
                                                    int* tok_out, int* ids_next, int* pos_next, int* hist,
                                                    int hist_stride, int* hist_count, int max_hist) {
  const int c = blockIdx.x;
  if (threadIdx.x != 0) return;
  const SampRow& sp = samp[c];
  const int nh = hist ? hist_count[c] : 0;
  double p[TOPK_MAX], w[TOPK_MAX];
  const int k = max(1, min(sp.top_k, K));
  const int tok = samp_pick(tk_val + (size_t)c * K, tk_idx + (size_t)c * K, k, sp.temp, sp.top_p, sp.min_p,
                            samp_u01(sp.seed, (uint64_t)(sp.draw0 + nh)), p, w);
  if (tok_out) tok_out[c] = tok;
  if (ids_next) ids_next[c] = tok;
  if (pos_next) pos_next[c] += 1;
  if (hist) {
    if (nh < max_hist) hist[(size_t)c * hist_stride + nh] = tok;
    hist_count[c] = nh + 1;
  }
}

__global__ void logprob_finish_kernel(const float* part, int nb, float* ms, float* top, int K);  // below

// ---------------------------------------------------------------------------
// The rest of llama-cpp-python's chain, for rounds in which some row has a SampExt setting.
// These kernels are templates (LATE, always 0) for their place in the code object alone: a template kernel is
// emitted where it is first launched, after the GEMV and attention templates above.  Emitted ahead of them, as
// plain kernels are, they moved the decode GEMVs to other page offsets and the 32-row greedy decode of bench.py
// ran 0.4 % slower than before with byte-identical kernels (profiles/sampler_chain.txt).
// bias_kernel, ahead of the penalties: thread j adds entry j of the row's table to its logit (one f32 add; the
// table's tokens are distinct, so no two threads share an address) and first saves the raw value to
// bias_raw[c][j] for the log-prob gather.
// ---------------------------------------------------------------------------
template <int LATE = 0>
__global__ __launch_bounds__(SAMP_BIAS_MAX) void bias_kernel(float* logits, int ldl, int V, const SampExt* ext,
                                                             float* bias_raw) {
  const int c = blockIdx.x, j = threadIdx.x;
  const SampExt& x = ext[c];
  if (j >= min(x.n_bias, SAMP_BIAS_MAX)) return;
  const int t = x.bias_tok[j];
  if (t < 0 || t >= V) return;
  float* lp = logits + (size_t)c * ldl + t;
  const float v = *lp;
  if (bias_raw) bias_raw[c * SAMP_BIAS_MAX + j] = v;
  *lp = v + x.bias_val[j];
}

// sample_kernel with the tail-free and typical cuts of samp_pick; rows of Mirostat requests are left to
// miro_pick_kernel, rows with more than TOPK_MAX candidates to sample_wide_kernel (token and bookkeeping)
template <int LATE = 0>
__global__ __launch_bounds__(64) void sample_ext_kernel(const float* tk_val, const int* tk_idx, int K,
                                                        const SampRow* samp, const SampExt* ext, int* tok_out,
                                                        int* ids_next, int* pos_next, int* hist, int hist_stride,
                                                        int* hist_count, int max_hist) {
  const int c = blockIdx.x;
  if (threadIdx.x != 0) return;
  const SampRow& sp = samp[c];
  const SampExt& x = ext[c];
  if (x.miro == 2 || x.wide_k > TOPK_MAX) return;  // picked by miro_pick_kernel / sample_wide_kernel
  const int nh = hist ? hist_count[c] : 0;
  double p[TOPK_MAX], w[TOPK_MAX];
  float cv[TOPK_MAX];
  int ci[TOPK_MAX], ord[TOPK_MAX];
  const int k = max(1, min(sp.top_k, K));
  const int tok = samp_pick(tk_val + (size_t)c * K, tk_idx + (size_t)c * K, k, sp.temp, sp.top_p, sp.min_p,
                            samp_u01(sp.seed, (uint64_t)(sp.draw0 + nh)), p, w, x.tfs_z, x.typical_p, cv, ci, ord);
  if (tok_out) tok_out[c] = tok;
  if (ids_next) ids_next[c] = tok;
  if (pos_next) pos_next[c] += 1;
  if (hist) {
    if (nh < max_hist) hist[(size_t)c * hist_stride + nh] = tok;
    hist_count[c] = nh + 1;
  }
}

// ---------------------------------------------------------------------------
// Mirostat v2 over the whole vocabulary.  With y_i = x_i / temp (one f32 division, x the row after bias and
// penalties), m = max y and s = sum exp(y_i - m): log p_i = (y_i - m) - log s, the token's surprise is
// -log2 p_i.  Three passes in the slice structure of lse_topk_stage1 (nb <= 64 slices of <= 4096 columns):
//   miro_stage1        per slice (m_b, s_b) in f32; logprob_finish_kernel folds them to (m, log s)
//   miro_mass_kernel   per slice the f64 mass and the count of the tokens with surprise <= mu
//   miro_pick_kernel   one wave per row: folds the slice masses in slice order, finds the slice holding u S,
//                      then the token by an ordered scan of that slice (kept tokens by ascending id), and
//                      writes the token, its bookkeeping and the new mu (in place and into the step history)
// log p_i and the masses are f64 from the f32 inputs, and every sum has a fixed order (a thread's strided
// terms, the wave64 butterfly, the 4 waves; slices by index; the scan by id), so the pick of a row depends
// neither on M nor on its batch-mates.  Rows with miro != 2 are skipped by every pass.
// ---------------------------------------------------------------------------
template <int LATE = 0>
__global__ __launch_bounds__(256) void miro_stage1(const float* logits, int ldl, int V, const SampRow* samp,
                                                   const SampExt* ext, float* part) {
  __shared__ float red[4];
  const int c = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  float* po = part + ((size_t)c * nb + b) * 2;
  if (ext[c].miro != 2) {
    if (threadIdx.x == 0) po[0] = -INFINITY, po[1] = 0.f;
    return;
  }
  const float temp = samp[c].temp;
  const int lo = (int)((long long)V * b / nb), hi = (int)((long long)V * (b + 1) / nb);
  const float* lr = logits + (size_t)c * ldl;
  float m = -INFINITY;
  for (int j = lo + threadIdx.x; j < hi; j += 256) m = fmaxf(m, lr[j] / temp);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  if (m > -INFINITY)
    for (int j = lo + threadIdx.x; j < hi; j += 256) sum += expf(lr[j] / temp - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) po[0] = m, po[1] = ((red[0] + red[1]) + red[2]) + red[3];
}

// log p of one entry (f64) and whether Mirostat keeps it; the two kernels below share it, so they agree on
// every token
__device__ __forceinline__ bool miro_kept(float x, float temp, float m, float ls, float mu, double* p) {
  const double lp = ((double)(x / temp) - (double)m) - (double)ls;
  const bool kept = -lp * 1.4426950408889634 <= (double)mu;  // false for a NaN
  *p = kept ? exp(lp) : 0.0;
  return kept;
}

template <int LATE = 0>
__global__ __launch_bounds__(256) void miro_mass_kernel(const float* logits, int ldl, int V, const SampRow* samp,
                                                        const SampExt* ext, const float* ms, const float* mu,
                                                        double* mass, int* cnt) {
  __shared__ double red[4];
  __shared__ int redn[4];
  const int c = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  if (ext[c].miro != 2) return;
  const float temp = samp[c].temp, m = ms[c * 2], ls = ms[c * 2 + 1], muc = mu[c];
  const int lo = (int)((long long)V * b / nb), hi = (int)((long long)V * (b + 1) / nb);
  const float* lr = logits + (size_t)c * ldl;
  double sum = 0.0;
  int n = 0;
  if (m > -INFINITY)
    for (int j = lo + threadIdx.x; j < hi; j += 256) {
      double p;
      n += miro_kept(lr[j], temp, m, ls, muc, &p) ? 1 : 0;
      sum += p;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o), n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum, redn[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    mass[c * 64 + b] = ((red[0] + red[1]) + red[2]) + red[3];
    cnt[c * 64 + b] = redn[0] + redn[1] + redn[2] + redn[3];
  }
}

template <int LATE = 0>
__global__ __launch_bounds__(64) void miro_pick_kernel(const float* logits, int ldl, int V, int nb, const SampRow* samp,
                                                       const SampExt* ext, const float* ms, const double* mass,
                                                       const int* cnt, float* mu, float* mu_hist, int mu_stride,
                                                       int* tok_out, int* ids_next, int* pos_next, int* hist,
                                                       int hist_stride, int* hist_count, int max_hist) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const SampExt& x = ext[c];
  if (x.miro != 2) return;
  const SampRow& sp = samp[c];
  const float temp = sp.temp, m = ms[c * 2], ls = ms[c * 2 + 1], muc = mu[c];
  const float* lr = logits + (size_t)c * ldl;
  const int nh = hist ? hist_count[c] : 0;
  const double mb = lane < nb ? mass[c * 64 + lane] : 0.0;
  const int cb = lane < nb ? cnt[c * 64 + lane] : 0;
  double S = 0.0;
  int total = 0;
  for (int b = 0; b < nb; ++b) S += __shfl(mb, b), total += __shfl(cb, b);
  int tok = 0;
  double pp = 1.0;  // renormalised probability of the pick
  if (total == 0 || !(S > 0.0)) {
    // nothing within mu: the argmax alone, ties to the lowest id
    int best = 0x7fffffff;
    for (int j = lane; j < V; j += 64)
      if (lr[j] / temp == m) best = min(best, j);
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    tok = best == 0x7fffffff ? 0 : best;
  } else {
    const double u = samp_u01(sp.seed, (uint64_t)(sp.draw0 + nh)) * S;
    int sb = -1, last = 0;
    double base = 0.0, last_base = 0.0, cum = 0.0;
    for (int b = 0; b < nb; ++b) {
      const double mbb = __shfl(mb, b);
      if (__shfl(cb, b) > 0) {
        last = b, last_base = cum;
        if (sb < 0 && u < cum + mbb) sb = b, base = cum;
      }
      cum += mbb;
    }
    if (sb < 0) sb = last, base = last_base;  // u S rounded past the last boundary: the last kept token
    const int lo = (int)((long long)V * sb / nb), hi = (int)((long long)V * (sb + 1) / nb);
    int found = -1, lastk = -1;
    double pf = 0.0, pl = 0.0, run = base;
    for (int j0 = lo; j0 < hi && found < 0; j0 += 64) {
      const int j = j0 + lane;
      double p = 0.0;
      const bool kept = j < hi && miro_kept(lr[j], temp, m, ls, muc, &p);
      double incl = p;
      for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
      }
      const unsigned long long hit = __ballot(kept && u < run + incl), km = __ballot(kept);
      if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        found = j0 + l, pf = __shfl(p, l);
      }
      if (km) {
        const int l = 63 - __clzll((long long)km);
        lastk = j0 + l, pl = __shfl(p, l);
      }
      run += __shfl(incl, 63);
    }
    if (found < 0) found = lastk, pf = pl;
    tok = max(found, 0);
    pp = pf / S;
  }
  if (lane == 0) {
    const float mun = (float)((double)muc - (double)x.eta * (-log2(pp) - (double)x.tau));
    mu[c] = mun;
    if (mu_hist && nh < mu_stride) mu_hist[(size_t)c * mu_stride + nh] = mun;
    if (tok_out) tok_out[c] = tok;
    if (ids_next) ids_next[c] = tok;
    if (pos_next) pos_next[c] += 1;
    if (hist) {
      if (nh < max_hist) hist[(size_t)c * hist_stride + nh] = tok;
      hist_count[c] = nh + 1;
    }
  }
}

int miro_pick_host(const float* x, int V, float temp, float tau, float eta, double u01, float* mu) {
  float m = -INFINITY;
  for (int i = 0; i < V; i++) m = fmaxf(m, x[i] / temp);
  double s = 0.0;
  if (m > -INFINITY)
    for (int i = 0; i < V; i++) s += exp((double)(x[i] / temp) - (double)m);
  const double ls = log(s);
  double S = 0.0;
  int n = 0, first_max = -1;
  for (int i = 0; i < V; i++) {
    if (first_max < 0 && x[i] / temp == m) first_max = i;
    const double lp = ((double)(x[i] / temp) - (double)m) - ls;
    if (m > -INFINITY && -lp * 1.4426950408889634 <= (double)*mu) S += exp(lp), n++;
  }
  int tok = std::max(first_max, 0);
  double pp = 1.0;
  if (n > 0 && S > 0.0) {
    const double u = u01 * S;
    double cum = 0.0;
    for (int i = 0; i < V; i++) {
      const double lp = ((double)(x[i] / temp) - (double)m) - ls;
      if (!(-lp * 1.4426950408889634 <= (double)*mu)) continue;
      cum += exp(lp);
      tok = i, pp = exp(lp) / S;
      if (u < cum) break;
    }
  }
  *mu = (float)((double)*mu - (double)eta * (-log2(pp) - (double)tau));
  return tok;
}

// ---------------------------------------------------------------------------
// The candidate chain over more than TOPK_MAX candidates, up to the whole vocabulary: top_k ->
// top_p -> min_p -> temperature -> draw as samp_pick runs them, without a sort.  Every cut keeps a prefix of one
// total order (value descending, ties to the lower id), so the kept set is a bound (key, id) and the draw is a
// search for a cumulative weight in the same order.  One work-group of 1024 threads per wide row; the row is only
// read (it stays in L2 between the passes).
//   key      wide_dkey: the f32 bits made an unsigned integer that ascends as the value descends, -0.0 folded
//            into +0.0 first (the host comparator sees them equal: ties go by id)
//   sweep    wide_sweep: a pass over the row, thread t taking the groups of four columns t, t + 1024, ...
//   top_k    (k < V) the key at which the running count reaches k: 4 passes of 8 key bits over an integer
//            histogram in LDS
//   search   8 passes of 4 key bits.  A pass sums, per thread, the terms of the elements inside the bound whose
//            key shares the prefix found so far into 16 buckets by the next 4 bits (f64 terms from the f32 inputs,
//            and integer counts), reduces them (a thread's terms in sweep order, the wave64 butterfly, the 16
//            waves in order through LDS) and walks the 16 sums in order from the carried base to the bucket that
//            holds the target.  Elements below the prefix are in the carried base and take no exp; the first pass
//            also gives the total.  Two uses: top_p over e_i = exp(x_i - x0), and the draw over
//            w_i = exp(x_i / temp - x0 / temp) inside the final bound when more than 1024 candidates are kept.
//   ties     the elements of the key a search ends on have one term: the first j of them (by id) that reach the
//            target are taken; when that is not all of them the id of the j-th comes from an ordered scan by id
//            (wide_nth)
//   min_p    e_i >= min_p is monotone in the key: the last key that passes comes from a bisection of the key range
//   small    at most 1024 candidates (every top_k <= 1024; or the kept set once the cuts are known) are gathered
//            into LDS and ranked in the order, and one thread runs samp_pick's own loops over them
//            (wide_pick_small): top_p, min_p and the draw for top_k <= 1024, the draw alone after the searches.
//            A larger kept set takes the search for the draw.
// Nothing is added in an order that depends on M, the row index, the batch-mates or the run.
// ---------------------------------------------------------------------------
constexpr int WIDE_NT = 1024, WIDE_NW = WIDE_NT / 64, WIDE_NB = 16;

__device__ __forceinline__ uint32_t wide_dkey(float x) {
  if (x == 0.0f) x = 0.0f;  // -0.0 -> +0.0
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? b : 0x7fffffffu - b;
}
__device__ __forceinline__ float wide_val(uint32_t d) {
  return __uint_as_float((d & 0x80000000u) ? d : 0x7fffffffu - d);
}
struct WideBound {  // the prefix of the order: the elements with (key, id) <= (t, id)
  uint32_t t;
  int id;
};
__device__ __forceinline__ bool wide_in(uint32_t d, int i, WideBound b) { return d < b.t || (d == b.t && i <= b.id); }
constexpr int WIDE_CAP = 1024;  // kept sets up to this size are ordered in LDS and drawn from as samp_pick does
struct WideShared {
  double red[WIDE_NW][WIDE_NB], tot[WIDE_NB];
  int redn[WIDE_NW][WIDE_NB], totn[WIDE_NB];
  int wcnt[WIDE_NW];
  int found;
  int hist[256];
  int lhist[256 * 16];  // the histogram of a pass in 16 copies by lane: at most 4 lanes of a wave share an address
  double pe[WIDE_CAP];
  int gcount;
  uint32_t gkey[WIDE_CAP];
  int gid[WIDE_CAP], sid[WIDE_CAP];
  double sw[WIDE_CAP];
};
// one pass over the row: f(x_j, j) for every j < V.  Thread t takes the groups of four columns t, t + 1024, ...
// (one 16-byte load each when the row is aligned, four of them in flight before the first is worked on) and
// column 4 (V / 4) + t of the tail, whatever the alignment: the order of a thread's terms depends on V alone.
template <class F>
__device__ __forceinline__ void wide_sweep(const float* lr, int V, F f) {
  const int tid = threadIdx.x, n4 = V >> 2;
  const bool al = ((uintptr_t)lr & 15) == 0;
  auto load = [&](int q) {
    if (al) return reinterpret_cast<const float4*>(lr)[q];
    return make_float4(lr[4 * q], lr[4 * q + 1], lr[4 * q + 2], lr[4 * q + 3]);
  };
  for (int q0 = tid; q0 < n4; q0 += 4 * WIDE_NT) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * WIDE_NT;
      v[u] = q < n4 ? load(q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * WIDE_NT;
      if (q < n4) f(v[u].x, 4 * q), f(v[u].y, 4 * q + 1), f(v[u].z, 4 * q + 2), f(v[u].w, 4 * q + 3);
    }
  }
  const int j = 4 * n4 + tid;
  if (j < V) f(lr[j], j);
}
struct WideHit {
  uint32_t t;     // the key the search ended on
  int n_below;    // elements inside the bound before that key, and with it
  int n_at;
  double below;   // their terms before that key
  double total;   // all terms inside the bound
};
// MODE 0: counts; 1: e_i; 2: w_i
template <int MODE>
__device__ __forceinline__ double wide_term(float x, double x0, double temp, double m0) {
#pragma clang fp contract(off)
  if (MODE == 1) return exp((double)x - x0);
  if (MODE == 2) return exp((double)x / temp - m0);
  return 0.0;
}
template <int MODE>
__device__ __forceinline__ bool wide_reached(double target, double cum, int k, int ncum) {
  return MODE == 0 ? ncum >= k : MODE == 1 ? cum >= target : target < cum;
}
// the first key, in the order, at which the running count reaches k (MODE 0), the running e reaches q * total
// (MODE 1) or exceeds it (MODE 2); the last key inside the bound when none does
template <int MODE>
__device__ WideHit wide_search(const float* lr, int V, WideBound bd, double x0, double temp, double m0, double q, int k,
                               WideShared& sh) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint32_t prefix = 0;
  double base = 0.0, target = 0.0, total = 0.0;
  int nbase = 0, n_at = 0;
  for (int p = 0; p < 8; ++p) {
    const int shift = 28 - 4 * p;
    double acc[WIDE_NB];
    int cnt[WIDE_NB];
#pragma unroll
    for (int b = 0; b < WIDE_NB; ++b) acc[b] = 0.0, cnt[b] = 0;
    wide_sweep(lr, V, [&](float x, int j) {
      const uint32_t d = wide_dkey(x);
      if ((uint32_t)((uint64_t)d >> (shift + 4)) == prefix && wide_in(d, j, bd)) {
        const int bk = (int)((d >> shift) & 15u);
        const double e = wide_term<MODE>(x, x0, temp, m0);
#pragma unroll
        for (int b = 0; b < WIDE_NB; ++b) {
          if (MODE != 0) acc[b] += bk == b ? e : 0.0;
          cnt[b] += bk == b ? 1 : 0;
        }
      }
    });
#pragma unroll
    for (int b = 0; b < WIDE_NB; ++b) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        if (MODE != 0) acc[b] += __shfl_xor(acc[b], o);
        cnt[b] += __shfl_xor(cnt[b], o);
      }
      if (lane == 0) sh.red[wave][b] = acc[b], sh.redn[wave][b] = cnt[b];
    }
    __syncthreads();
    if (tid < WIDE_NB) {
      double a = 0.0;
      int n = 0;
      for (int w = 0; w < WIDE_NW; ++w) a += sh.red[w][tid], n += sh.redn[w][tid];
      sh.tot[tid] = a, sh.totn[tid] = n;
    }
    __syncthreads();
    if (p == 0) {
      for (int b = 0; b < WIDE_NB; ++b) total += sh.tot[b];
      target = q * total;
    }
    double cum = base, pb = base;
    int ncum = nbase, pn = nbase, pick = 0;
    n_at = 0;
    for (int b = 0; b < WIDE_NB; ++b) {
      const double tb = sh.tot[b];
      const int nb = sh.totn[b];
      if (nb > 0) {
        pb = cum, pn = ncum, pick = b, n_at = nb;
        if (wide_reached<MODE>(target, cum + tb, k, ncum + nb)) break;
      }
      cum += tb, ncum += nb;
    }
    base = pb, nbase = pn;
    prefix = (prefix << 4) | (uint32_t)pick;
  }
  return WideHit{prefix, nbase, n_at, base, total};
}
// the count cut: the key at which the running count of the order reaches k, by 4 passes of 8 key bits over an
// integer histogram in LDS (integer atomics: the counts do not depend on their order)
__device__ WideHit wide_count_search(const float* lr, int V, int k, WideShared& sh) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  int nbase = 0, n_at = 0;
  for (int p = 0; p < 4; ++p) {
    const int shift = 24 - 8 * p;
    for (int i = tid; i < 256 * 16; i += WIDE_NT) sh.lhist[i] = 0;
    __syncthreads();
    wide_sweep(lr, V, [&](float x, int j) {
      const uint32_t d = wide_dkey(x);
      if ((uint32_t)((uint64_t)d >> (shift + 8)) == prefix)
        atomicAdd(&sh.lhist[((d >> shift) & 255u) * 16 + (tid & 15)], 1);
    });
    __syncthreads();
    {  // bin tid / 4: four threads add 4 copies each
      int n = 0;
      for (int i = 0; i < 4; ++i) n += sh.lhist[(tid >> 2) * 16 + (tid & 3) * 4 + i];
      n += __shfl_xor(n, 1);
      n += __shfl_xor(n, 2);
      if ((tid & 3) == 0) sh.hist[tid >> 2] = n;
    }
    __syncthreads();
    int cum = nbase, pn = nbase, pick = 0;
    n_at = 0;
    for (int b = 0; b < 256; ++b) {
      const int nb = sh.hist[b];
      if (nb > 0) {
        pn = cum, pick = b, n_at = nb;
        if (cum + nb >= k) break;
      }
      cum += nb;
    }
    nbase = pn;
    prefix = (prefix << 8) | (uint32_t)pick;
    __syncthreads();  // every thread has read the histogram before the next pass clears it
  }
  return WideHit{prefix, nbase, n_at, 0.0, 0.0};
}
// the rest of the chain over a bound that holds at most WIDE_CAP candidates: they are gathered into LDS, each finds
// its rank in the order, the first kcut of them are the candidates, every thread forms one e_i and w_i, and one
// thread runs samp_pick's own loops (top_p, min_p, the draw) over them in that order -- the host sampler's
// additions in the host sampler's order.  Returns the token, or -1 when the bound holds more (nothing decided).
__device__ int wide_pick_small(const float* lr, int V, WideBound bd, int kcut, double x0, double temp, double m0,
                               float top_p, float min_p, double u01, WideShared& sh) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) sh.gcount = 0, sh.found = -1;
  __syncthreads();
  wide_sweep(lr, V, [&](float x, int j) {
    const uint32_t d = wide_dkey(x);
    const bool in = wide_in(d, j, bd);
    const unsigned long long bal = __ballot(in);
    if (bal) {
      int base = 0;
      const int leader = __ffsll((long long)bal) - 1;
      if (lane == leader) base = atomicAdd(&sh.gcount, __popcll(bal));
      base = __shfl(base, leader);
      const int slot = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (in && slot < WIDE_CAP) sh.gkey[slot] = d, sh.gid[slot] = j;
    }
  });
  __syncthreads();
  const int n = sh.gcount;
  if (n > WIDE_CAP || n < 1) {
    __syncthreads();
    return -1;
  }
  const int k = min(n, kcut);
  if (tid < n) {
    const uint32_t d = sh.gkey[tid];
    const int id = sh.gid[tid];
    int rank = 0;
    for (int s2 = 0; s2 < n; ++s2) {
      const uint32_t ds = sh.gkey[s2];
      rank += (ds < d || (ds == d && sh.gid[s2] < id)) ? 1 : 0;
    }
    sh.sid[rank] = id;
    sh.pe[rank] = wide_term<1>(wide_val(d), x0, temp, m0);
    sh.sw[rank] = wide_term<2>(wide_val(d), x0, temp, m0);
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += sh.pe[i];
    sh.tot[0] = sum;
  }
  __syncthreads();
  if (tid < k) sh.pe[tid] /= sh.tot[0];
  __syncthreads();
  if (tid == 0) {
    int keep = k;
    if (top_p < 1.0f) {
      double cum = 0.0;
      for (int i = 0; i < k; ++i) {
        cum += sh.pe[i];
        if (cum >= top_p) {
          keep = i + 1;
          break;
        }
      }
    }
    if (min_p > 0.f) {
      int kk = 1;
      for (int i = 1; i < keep; ++i)
        if (sh.pe[i] >= min_p * sh.pe[0]) kk = i + 1;
      keep = kk;
    }
    double s2 = 0.0;
    for (int i = 0; i < keep; ++i) s2 += sh.sw[i];
    const double u = u01 * s2;
    double acc = 0.0;
    int tok = sh.sid[keep - 1];
    for (int i = 0; i < keep; ++i) {
      acc += sh.sw[i];
      if (u < acc) {
        tok = sh.sid[i];
        break;
      }
    }
    sh.found = tok;
  }
  __syncthreads();
  const int f = sh.found;
  __syncthreads();
  return f;
}
// how many of the n_at elements of one key (term `each`), taken in order after `below`, it takes to reach the
// target: the smallest j >= 1, n_at when none does
template <int MODE>
__device__ int wide_ties(double below, double each, double target, int n_at) {
#pragma clang fp contract(off)
  if (n_at <= 1) return 1;
  if (!(each > 0.0)) return wide_reached<MODE>(target, below, 0, 0) ? 1 : n_at;
  int j = (int)fmin(fmax(ceil((target - below) / each), 1.0), (double)n_at);
  while (j > 1 && wide_reached<MODE>(target, below + (double)(j - 1) * each, 0, 0)) --j;
  while (j < n_at && !wide_reached<MODE>(target, below + (double)j * each, 0, 0)) ++j;
  return j;
}
// the id of the r-th element (r >= 1, by ascending id) whose key is t: the 16 waves count their segments of the
// row, then the wave holding the r-th scans its segment again
__device__ int wide_nth(const float* lr, int V, uint32_t t, int r, WideShared& sh) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int seg = ((V + WIDE_NW - 1) / WIDE_NW + 63) & ~63;
  const int lo = wave * seg, hi = min(V, lo + seg);
  int n = 0;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int j = j0 + lane;
    n += __popcll(__ballot(j < hi && wide_dkey(lr[j]) == t));
  }
  if (lane == 0) sh.wcnt[wave] = n;
  if (tid == 0) sh.found = -1;
  __syncthreads();
  int before = 0, ww = -1;
  for (int w = 0; w < WIDE_NW; ++w) {
    const int cw = sh.wcnt[w];
    if (ww < 0 && r <= before + cw) ww = w;
    if (ww < 0) before += cw;
  }
  if (wave == ww) {
    int run = before;
    for (int j0 = lo; j0 < hi; j0 += 64) {
      const int j = j0 + lane;
      const bool m = j < hi && wide_dkey(lr[j]) == t;
      const unsigned long long bal = __ballot(m);
      const int pc = __popcll(bal);
      if (r <= run + pc) {
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (m && run + rank + 1 == r) sh.found = j;
        break;
      }
      run += pc;
    }
  }
  __syncthreads();
  const int f = sh.found;
  __syncthreads();  // every thread has read it before the next call resets it
  return f;
}

template <int LATE = 0>
__global__ __launch_bounds__(WIDE_NT) void sample_wide_kernel(const float* logits, int ldl, int V, const SampRow* samp,
                                                              const SampExt* ext, const float* tk_val,
                                                              const int* tk_idx, int K, int* tok_out, int* ids_next,
                                                              int* pos_next, int* hist, int hist_stride,
                                                              int* hist_count, int max_hist) {
#pragma clang fp contract(off)
  __shared__ WideShared sh;
  const int c = blockIdx.x;
  const int kw = ext[c].wide_k;
  if (kw <= TOPK_MAX) return;
  const SampRow& sp = samp[c];
  const float* lr = logits + (size_t)c * ldl;
  const int nh = hist ? hist_count[c] : 0;
  const float x0f = tk_val[(size_t)c * K];  // the first candidate: the maximum, ties to the lowest id
  const int id0 = min(max(tk_idx[(size_t)c * K], 0), V - 1);
  int tok = id0;  // a row whose maximum is -inf has no distribution: its lowest id
  if (x0f > -INFINITY) {
    const double x0 = (double)x0f, temp = (double)sp.temp, m0 = x0 / temp;
    const uint32_t d0 = wide_dkey(x0f);
    WideBound bd{0xffffffffu, 0x7fffffff};
    const double u01 = samp_u01(sp.seed, (uint64_t)(sp.draw0 + nh));
    int f = -1;
    if (kw <= WIDE_CAP) {
      // few candidates: the count cut, then the whole chain over them in LDS.  The bound takes every element of
      // the last key; the rank cuts them to kw.
      if (kw < V) bd = WideBound{wide_count_search(lr, V, kw, sh).t, 0x7fffffff};
      f = wide_pick_small(lr, V, bd, kw, x0, temp, m0, sp.top_p, sp.min_p, u01, sh);
      bd = WideBound{0xffffffffu, 0x7fffffff};  // (more ties than the LDS holds: the general path, from the start)
    }
    if (f < 0) {
      int n_kept = V;  // -1 once a cut leaves it unknown
      if (kw < V) {  // top_k: the first kw of the order
        const WideHit h = wide_count_search(lr, V, kw, sh);
        const int r = min(max(kw - h.n_below, 1), max(h.n_at, 1));
        // all the elements of the last key: no id bound to look for
        bd = WideBound{h.t, r >= h.n_at ? 0x7fffffff : wide_nth(lr, V, h.t, r, sh)};
        n_kept = kw;
      }
      if (sp.top_p < 1.0f) {  // through the first candidate at which the running e reaches top_p * S
        const WideHit h = wide_search<1>(lr, V, bd, x0, temp, m0, (double)sp.top_p, 0, sh);
        const double each = wide_term<1>(wide_val(h.t), x0, temp, m0);
        const int j = wide_ties<1>(h.below, each, (double)sp.top_p * h.total, h.n_at);
        bd = WideBound{h.t, j >= h.n_at ? 0x7fffffff : wide_nth(lr, V, h.t, j, sh)};
        n_kept = h.n_below + j;
      }
      if (sp.min_p > 0.0f) {  // of those, through the last one with e_i >= min_p (p_i >= min_p p_0); the first stays
        const double mp = (double)sp.min_p;
        n_kept = -1;
        if (!(1.0 >= mp)) {
          bd = WideBound{d0, id0};
        } else {
          uint32_t lo = d0, hi = 0xff800000u;  // x0 .. -inf: no key between them is a NaN
          while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (wide_term<1>(wide_val(mid), x0, temp, m0) >= mp) lo = mid;
            else hi = mid - 1;
          }
          if (lo < bd.t) bd = WideBound{lo, 0x7fffffff};
        }
      }
      if (n_kept <= WIDE_CAP) f = wide_pick_small(lr, V, bd, 0x7fffffff, x0, temp, m0, 1.0f, 0.0f, u01, sh);
      if (f < 0) {  // a large kept set: the search
        const WideHit h = wide_search<2>(lr, V, bd, x0, temp, m0, u01, 0, sh);
        const double each = wide_term<2>(wide_val(h.t), x0, temp, m0);
        const int j = wide_ties<2>(h.below, each, u01 * h.total, h.n_at);
        f = wide_nth(lr, V, h.t, j, sh);
      }
    }
    tok = f >= 0 ? f : id0;
  }
  if (threadIdx.x == 0) {
    if (tok_out) tok_out[c] = tok;
    if (ids_next) ids_next[c] = tok;
    if (pos_next) pos_next[c] += 1;
    if (hist) {
      if (nh < max_hist) hist[(size_t)c * hist_stride + nh] = tok;
      hist_count[c] = nh + 1;
    }
  }
}

int launch_sample_wide(const float* logits, int ldl, int M, int V, const SampRow* samp, const SampExt* ext,
                       const float* tk_val, const int* tk_idx, int K, int* tok_out, int* ids_next, int* pos_next,
                       int* hist, int hist_stride, int* hist_count, int max_hist, hipStream_t s) {
  if (M < 1 || V < 1 || V > SAMP_WIDE_VMAX || ldl < V || K < 1 || !ext || !tk_val || !tk_idx) return -1;
  sample_wide_kernel<0><<<M, WIDE_NT, 0, s>>>(logits, ldl, V, samp, ext, tk_val, tk_idx, K, tok_out, ids_next, pos_next,
                                              hist, hist_stride, hist_count, max_hist);
  return 0;
}

int launch_sample_chain(float* logits, int ldl, int M, int V, const SampRow* samp, int K, float* ws_val, int* ws_idx,
                        float* tk_val, int* tk_idx, int* tok_out, int* ids_next, int* pos_next, int* hist,
                        int hist_stride, int* hist_count, int max_hist, hipStream_t s, int* side_tok,
                        float* side_val, const SampExtArgs* x) {
  if (K < 1 || K > TOPK_MAX || M < 1) return -1;
  if (x && x->any_wide && (!x->ext || V > SAMP_WIDE_VMAX)) return -1;
  const SampExt* ext = x ? x->ext : nullptr;
  const int nb = std::min(64, std::max(1, (V + 2047) / 2048));
  if (ext && x->any_miro && (!x->mu || !x->ws_f || !x->ws_d || !x->ws_i || (V + nb - 1) / nb > 4096)) return -1;
  if (ext) bias_kernel<0><<<M, SAMP_BIAS_MAX, 0, s>>>(logits, ldl, V, ext, x->bias_raw);
  penalty_kernel<<<M, 64, 0, s>>>(logits, ldl, samp, hist, hist_stride, hist_count, side_tok, side_val);
  if (launch_topk(logits, ldl, M, V, K, ws_val, ws_idx, tk_val, tk_idx, s)) return -1;
  if (!ext) {
    sample_kernel<<<M, 64, 0, s>>>(tk_val, tk_idx, K, samp, tok_out, ids_next, pos_next, hist, hist_stride, hist_count,
                                   max_hist);
    return 0;
  }
  sample_ext_kernel<0><<<M, 64, 0, s>>>(tk_val, tk_idx, K, samp, ext, tok_out, ids_next, pos_next, hist, hist_stride,
                                     hist_count, max_hist);
  if (x->any_miro) {
    float* part = x->ws_f;
    float* ms = x->ws_f + (size_t)M * 64 * 2;
    miro_stage1<0><<<dim3(nb, M), 256, 0, s>>>(logits, ldl, V, samp, ext, part);
    logprob_finish_kernel<<<M, 64, 0, s>>>(part, nb, ms, nullptr, 0);
    miro_mass_kernel<0><<<dim3(nb, M), 256, 0, s>>>(logits, ldl, V, samp, ext, ms, x->mu, x->ws_d, x->ws_i);
    miro_pick_kernel<0><<<M, 64, 0, s>>>(logits, ldl, V, nb, samp, ext, ms, x->ws_d, x->ws_i, x->mu, x->mu_hist,
                                      x->mu_stride, tok_out, ids_next, pos_next, hist, hist_stride, hist_count,
                                      max_hist);
  }
  if (x->any_wide &&
      launch_sample_wide(logits, ldl, M, V, samp, ext, tk_val, tk_idx, K, tok_out, ids_next, pos_next, hist,
                         hist_stride, hist_count, max_hist, s))
    return -1;
  return 0;
}

// ---------------------------------------------------------------------------
// Per-token log-probabilities over the raw lm_head logits row x[0..V): with m = max x and
// s = sum exp(x_i - m), logprob(i) = (x_i - m) - log(s) -- always in that form (never x_i - (m + log s):
// the rounded sum loses the result when |m| is large), f32 throughout, no atomics.  Stage 1 is
// topk_stage1 plus the slice's (m_b, s_b): the slice staged in LDS serves both, one HBM read of the
// row.  Every sum runs in a fixed order (a thread's strided terms, the wave64 butterfly, the 4 waves,
// then the slices by index), so a row's result does not depend on M or on its batch-mates.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lse_topk_stage1(const float* logits, int ldl, int V, int K, float* cv, int* ci,
                                                       float* part) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ float red[4];
  const int c = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  const int lo = (int)((long long)V * b / nb), hi = (int)((long long)V * (b + 1) / nb);
  __shared__ int ids[4096];
  __shared__ float vals[4096];
  float m = -INFINITY;
  for (int j = threadIdx.x; j < hi - lo; j += 256) {
    const float v = logits[(size_t)c * ldl + lo + j];
    vals[j] = v, ids[j] = lo + j;
    m = fmaxf(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();  // also: vals / ids complete
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  if (m > -INFINITY)
    for (int j = threadIdx.x; j < hi - lo; j += 256) sum += expf(vals[j] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float* p = part + ((size_t)c * nb + b) * 2;
    p[0] = m;
    p[1] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  if (K > 0)
    topk_select<256>(vals, ids, hi - lo, K, cv + ((size_t)c * nb + b) * K, ci + ((size_t)c * nb + b) * K, sv, si);
}

// one wave per row: merge the nb <= 64 slice partials (s = sum_b s_b exp(m_b - m), in index order),
// store (m, log s), and turn the row's merged top-k values into log-probabilities in place
__global__ __launch_bounds__(64) void logprob_finish_kernel(const float* part, int nb, float* ms, float* top, int K) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float mb = -INFINITY, sb = 0.f;
  if (lane < nb) mb = part[((size_t)c * nb + lane) * 2], sb = part[((size_t)c * nb + lane) * 2 + 1];
  float m = mb;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  const float term = sb > 0.f ? sb * expf(mb - m) : 0.f;
  float sum = 0.f;
  for (int b = 0; b < nb; ++b) sum += __shfl(term, b);
  const float ls = logf(sum);
  if (lane == 0) ms[c * 2] = m, ms[c * 2 + 1] = ls;
  if (lane < K) top[(size_t)c * K + lane] = (top[(size_t)c * K + lane] - m) - ls;
}

// one wave per row, after the pick: entry = [logprob of toks[c] | K top log-probs | K top ids (int bits)]
// at out[c * row_stride + step * (1 + 2K)], step = hist_count[c] - 1 (the token just appended; 0 without
// a history).  The token's raw logit comes from the penalty side table when the penalties rewrote it.
__global__ __launch_bounds__(64) void logprob_gather_kernel(const float* logits, int ldl, int V, int K, const int* toks,
                                                            const int* hist_count, int max_steps, const int* side_tok,
                                                            const float* side_val, const float* ms, const float* top,
                                                            const int* top_idx, float* out, size_t row_stride,
                                                            const SampExt* ext, const float* bias_raw) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int step = hist_count ? hist_count[c] - 1 : 0;
  if (step < 0 || step >= max_steps) return;
  float* o = out + (size_t)c * row_stride + (size_t)step * (1 + 2 * K);
  const int tok = toks[c];
  float raw = tok >= 0 && tok < V ? logits[(size_t)c * ldl + tok] : NAN;
  if (side_tok) {
    const bool hit = side_tok[c * SAMP_WIN + lane] == tok;
    const float sv = hit ? side_val[c * SAMP_WIN + lane] : 0.f;
    const unsigned long long mask = __ballot(hit);
    if (mask) raw = __shfl(sv, __ffsll((long long)mask) - 1);
  }
  if (ext) {  // a biased token: its value from before the bias (what the penalties saved was already biased)
    const int nbias = min(ext[c].n_bias, SAMP_BIAS_MAX);
    for (int j0 = 0; j0 < nbias; j0 += 64) {
      const int j = j0 + lane;
      const bool hit = j < nbias && ext[c].bias_tok[j] == tok;
      const float bv = hit ? bias_raw[c * SAMP_BIAS_MAX + j] : 0.f;
      const unsigned long long mask = __ballot(hit);
      if (mask) raw = __shfl(bv, __ffsll((long long)mask) - 1);
    }
  }
  if (lane == 0) o[0] = (raw - ms[c * 2]) - ms[c * 2 + 1];
  if (lane < K) {
    o[1 + lane] = top[(size_t)c * K + lane];
    reinterpret_cast<int*>(o)[1 + K + lane] = top_idx[(size_t)c * K + lane];
  }
}

int launch_logprob_stats(const float* logits, int ldl, int M, int V, int K, float* ws_val, int* ws_idx, float* part,
                         float* ms, float* top_lp, int* top_idx, hipStream_t s) {
  if (K < 0 || K > TOPK_MAX || K > V || M < 1 || V < 1) return -1;
  const int nb = std::min(64, std::max(1, (V + 2047) / 2048));
  if ((V + nb - 1) / nb > 4096) return -1;
  lse_topk_stage1<<<dim3(nb, M), 256, 0, s>>>(logits, ldl, V, K, ws_val, ws_idx, part);
  if (K > 0) topk_stage2<<<M, 256, 0, s>>>(ws_val, ws_idx, nb * K, K, top_lp, top_idx);
  logprob_finish_kernel<<<M, 64, 0, s>>>(part, nb, ms, top_lp, K);
  return 0;
}

int launch_logprob_gather(const float* logits, int ldl, int M, int V, int K, const int* toks, const int* hist_count,
                          int max_steps, const int* side_tok, const float* side_val, const float* ms,
                          const float* top_lp, const int* top_idx, float* out, size_t row_stride, hipStream_t s,
                          const SampExt* ext, const float* bias_raw) {
  if (K < 0 || K > TOPK_MAX || M < 1 || max_steps < 1 || row_stride < (size_t)max_steps * (1 + 2 * K)) return -1;
  if (ext && !bias_raw) ext = nullptr;
  logprob_gather_kernel<<<M, 64, 0, s>>>(logits, ldl, V, K, toks, hist_count, max_steps, side_tok, side_val, ms,
                                         top_lp, top_idx, out, row_stride, ext, bias_raw);
  return 0;
}

int launch_logprobs(const float* logits, int ldl, int M, int V, int K, const int* targets, float* ws_val, int* ws_idx,
                    float* part, float* ms, float* top_lp, int* top_idx, float* out, hipStream_t s) {
  if (launch_logprob_stats(logits, ldl, M, V, K, ws_val, ws_idx, part, ms, top_lp, top_idx, s)) return -1;
  return launch_logprob_gather(logits, ldl, M, V, K, targets, nullptr, 1, nullptr, nullptr, ms, top_lp, top_idx, out,
                               (size_t)(1 + 2 * K), s);
}

// ---------------------------------------------------------------------------
// pipeline hand-off of the residual stream in bf16 (half the bytes of f32 per stage boundary)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(uint16_t* dst, const float* src, size_t n4) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
    u32x2 o;
    o[0] = f2bf_nan(v[0]) | (f2bf_nan(v[1]) << 16);
    o[1] = f2bf_nan(v[2]) | (f2bf_nan(v[3]) << 16);
    reinterpret_cast<u32x2*>(dst)[i] = o;
  }
}

// one work-group per row; ssq as embed_kernel / ssq_kernel (per 16-element tile, double sum)
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(float* x, const uint16_t* src, int n, float* ssq) {
  const int c = blockIdx.x;
  const u32x4* s4 = reinterpret_cast<const u32x4*>(src + (size_t)c * n);
  f32x4* dst = reinterpret_cast<f32x4*>(x + (size_t)c * n);
  for (int t = threadIdx.x; t < n / 16; t += blockDim.x) {
    f32x4 g[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 v = s4[2 * t + h];
      f32x4 lo, hi;
      lo[0] = __uint_as_float(v[0] << 16); lo[1] = __uint_as_float(v[0] & 0xffff0000u);
      lo[2] = __uint_as_float(v[1] << 16); lo[3] = __uint_as_float(v[1] & 0xffff0000u);
      hi[0] = __uint_as_float(v[2] << 16); hi[1] = __uint_as_float(v[2] & 0xffff0000u);
      hi[2] = __uint_as_float(v[3] << 16); hi[3] = __uint_as_float(v[3] & 0xffff0000u);
      dst[4 * t + 2 * h] = lo;
      dst[4 * t + 2 * h + 1] = hi;
      g[2 * h] = lo;
      g[2 * h + 1] = hi;
    }
    if (ssq) ssq[(size_t)c * (n / 16) + t] = ssq16(g[0], g[1], g[2], g[3]);
  }
}

// f32 hand-off: a copy kernel, not hipMemcpyAsync -- a device-to-device memcpy may run on a copy
// engine, and the stage split must see exactly what the previous kernels wrote (the kernels' own
// ordering and cache rules, as the bf16 hand-off has); the receiving side writes the Σx² partials
// in the same pass (as ssq_kernel)
__global__ __launch_bounds__(256) void f32_copy_kernel(float* dst, const float* src, size_t n4) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
    reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
}
__global__ __launch_bounds__(256) void f32_in_kernel(float* x, const float* src, int n, float* ssq) {
  const int c = blockIdx.x;
  const f32x4* s4 = reinterpret_cast<const f32x4*>(src + (size_t)c * n);
  f32x4* d4 = reinterpret_cast<f32x4*>(x + (size_t)c * n);
  for (int t = threadIdx.x; t < n / 16; t += blockDim.x) {
    f32x4 g[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      g[h] = s4[4 * t + h];
      d4[4 * t + h] = g[h];
    }
    if (ssq) ssq[(size_t)c * (n / 16) + t] = ssq16(g[0], g[1], g[2], g[3]);
  }
}

void launch_copy_f32(float* dst, const float* src, size_t n, hipStream_t s) {
  const size_t n4 = n / 4;
  const int grid = (int)std::min<size_t>(1024, (n4 + 255) / 256);
  f32_copy_kernel<<<std::max(grid, 1), 256, 0, s>>>(dst, src, n4);
}

void launch_f32_in(float* x, const float* src, int M, int n, float* ssq, hipStream_t s) {
  f32_in_kernel<<<M, 256, 0, s>>>(x, src, n, ssq);
}

void launch_f32_to_bf16(uint16_t* dst, const float* src, size_t n, hipStream_t s) {
  const size_t n4 = n / 4;
  const int grid = (int)std::min<size_t>(1024, (n4 + 255) / 256);
  f32_to_bf16_kernel<<<std::max(grid, 1), 256, 0, s>>>(dst, src, n4);
}

void launch_bf16_to_f32(float* dst, const uint16_t* src, int M, int n, float* ssq, hipStream_t s) {
  bf16_to_f32_kernel<<<M, 256, 0, s>>>(dst, src, n, ssq);
}

}  // namespace mx

namespace mx {

// ---------------------------------------------------------------------------
// Prefill GEMM (> 64 rows): out = X[M][K] . W[N][K]^T with the decode epilogues, bf16 MFMA
// 16x16x32, f32 accumulation (SURVEY §8a a7, a11, a12 at prefill; §8d prefill FLOPs).  Block = 8
// waves, tile 256 weight rows x 256 tokens; wave (wn, wm) = 64 rows (4 packed row tiles) x 128
// tokens (8 column tiles).  Both operands staged global -> LDS by LDS-DMA (global_load_lds, 16 B
// per lane) in units of one 32-deep k-tile (16 KiB of A + 16 KiB of B) through a ring of NBUF
// buffers: NBUF-1 k-tiles in flight, one raw barrier per k-tile with a counted vmcnt (never 0
// before the tail), and the fragments of the next k-tile read into a second register set while
// this k-tile's MFMAs run (cdna_hip_programming.md §5 "Pipelining across barriers").  Against the
// round-1 form (two 64 KiB buffers, one 64-deep step in flight): +2-4 % at 512-4096 rows.
// The packed weight tiles are lane-linear 1 KiB A fragments, so a wave-instruction copies one
// tile verbatim; token rows are gathered per lane into the same lane-linear B-fragment images
// (lane l = token l&15, k 8(l>>4)..+8 of a 32-deep k-tile), so every ds_read_b128 is
// conflict-free without a swizzle.  Blocks are remapped so the token blocks of one weight block
// run on one XCD (shared L2); small GEMMs split K over grid.y into partial slabs (EPI_SLAB).
// ---------------------------------------------------------------------------
constexpr int GB_N = 256, GB_M = 256, GKC = 64;
constexpr int GEMM_NBUF = 4;  // k-tile buffers (5: 160 KiB, no faster; tools/gpu/r2x.sh)
typedef __attribute__((address_space(1))) const void gvoid;
typedef __attribute__((address_space(3))) void lvoid;

// gate/up split-K partials -> sum in slab order -> SwiGLU -> bf16 act (the EPI_SWIGLU epilogue's
// values: slab tile t holds gate rows 8t..8t+7 in rows 16t..16t+7 and the up rows after them)
__global__ __launch_bounds__(256) void swiglu_finish_kernel(MMArgs a, const float* slabs, int nslab, size_t stride) {
  const int quads = a.N / 8;  // 4-row groups of ffn rows
  const int total = a.M * quads;
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < total; u += gridDim.x * blockDim.x) {
    const int col = u / quads, fr = (u % quads) * 4;
    const int srow = (fr >> 3) * 16 + (fr & 7);
    const float* p = slabs + (size_t)col * a.N + srow;
    f32x4 g = *reinterpret_cast<const f32x4*>(p), up = *reinterpret_cast<const f32x4*>(p + 8);
    for (int k = 1; k < nslab; ++k) {
      g += *reinterpret_cast<const f32x4*>(p + k * stride);
      up += *reinterpret_cast<const f32x4*>(p + k * stride + 8);
    }
    f32x4 f;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = (g[i] / (1.0f + expf(-g[i]))) * up[i];
    u32x2 o;
    o[0] = f2bf(f[0]) | (f2bf(f[1]) << 16);
    o[1] = f2bf(f[2]) | (f2bf(f[3]) << 16);
    *reinterpret_cast<u32x2*>(a.act + (size_t)col * a.lda + fr) = o;
  }
}

// RW: row tiles per wave -- 4 (256-row blocks), 3 (192: Llama-3-8B q|k|v, N 6144 = 24 x 256 -> 384
// blocks = 1.5 rounds on 256 CUs, = 32 x 192 -> 512 = 2 full rounds), 2 or 1 (128 / 64 weight rows:
// grids too small to fill the CUs -- a few hundred prompt rows, or TinyLlama's N 2048 -- which
// round 6 no longer splits over K: one K range per output keeps prefill batch-invariant, and the
// row-block height does not change any output's summation order)
template <int EPI, int NBUF, int RW = 4>
__global__ __launch_bounds__(512, 1) void gemm_kernel(MMArgs a) {
  constexpr int BN = 64 * RW, AT = 4 * RW;  // rows per block, A (row) tiles per block
  __shared__ __attribute__((aligned(1024))) uint8_t lds[NBUF * 32768];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = w & 3, wm = w >> 2;
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, q = nwg / 8, rr = nwg % 8;
  const int wgid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
  const int nmb = (a.M + GB_M - 1) / GB_M;
  const int mb = wgid % nmb, nb = wgid / nmb;
  const int KT = a.K / TILE_K;
  const int ks = blockIdx.y, t0 = KT * ks / gridDim.y, t1 = KT * (ks + 1) / gridDim.y;
  const int m0 = mb * GB_M;
  const int r16 = lane & 15;

  // wave w copies A tiles 2w, 2w+1 (RW = 3: the last two waves repeat tile AT-1 -- the same bytes to
  // the same LDS slot, so every wave still issues 4 loads per k-tile for the counted waits) and B
  // (token) tiles 2w, 2w+1 of every k-tile.  Sources as a wave-uniform base + a 32-bit per-lane
  // offset (3 VGPRs instead of 8: the loop runs at the cap)
  const int at0 = min(w * 2, AT - 1), at1 = min(w * 2 + 1, AT - 1);
  const uint8_t* abase = reinterpret_cast<const uint8_t*>(a.W) + (size_t)(nb * AT + at0) * KT * 1024;
  const size_t astep = (size_t)(at1 - at0) * KT * 1024;  // the second row tile
  const uint32_t aoff = lane * 16;
  uint32_t boff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int tok = min(m0 + (w * 2 + i) * 16 + r16, a.M - 1);
    boff[i] = (uint32_t)tok * (uint32_t)a.ldx + 8 * (lane >> 4);
  }
  // k-tile min(kt, t1-1) into buffer kt % NBUF
  auto issue = [&](int kt_buf) {
    uint8_t* base = lds + (kt_buf % NBUF) * 32768;
    const int kt = min(kt_buf, t1 - 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = w * 2 + i, ta = i ? at1 : at0;
      __builtin_amdgcn_global_load_lds((gvoid*)(abase + i * astep + (size_t)kt * 1024 + aoff), (lvoid*)(base + ta * 1024),
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds((gvoid*)(a.X + boff[i] + (size_t)kt * TILE_K), (lvoid*)(base + 16384 + t * 1024),
                                       16, 0, 0);
    }
  };

  f32x4 acc[RW][8];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frags {
    u32x4 a[RW], b[8];
  };
  auto read = [&](Frags& f, int kt) {
    const uint8_t* Ab = lds + (kt % NBUF) * 32768;
    const uint8_t* Bb = Ab + 16384;
#pragma unroll
    for (int r = 0; r < RW; ++r) f.a[r] = *reinterpret_cast<const u32x4*>(Ab + (wn * RW + r) * 1024 + lane * 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) f.b[j] = *reinterpret_cast<const u32x4*>(Bb + (wm * 8 + j) * 1024 + lane * 16);
  };
  auto mfma = [&](const Frags& f) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < RW; ++r)
        acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f.a[r]),
                                                            __builtin_bit_cast(bf16x8, f.b[j]), acc[r][j], 0, 0, 0);
  };
  // Every k-tile step issues one k-tile's copies (the source clamped to the last k-tile past the
  // end: a few redundant copies into buffers nobody reads again), so the count of copies in flight
  // behind k-tile kt+1 is always NBUF-2 k-tiles and the waits are constants
  static_assert(NBUF == 4 || NBUF == 5, "vmcnt counts below assume a 4- or 5-buffer ring");

  // the fragments of k-tile kt+1 are read from LDS while k-tile kt's MFMAs run; every buffer holds
  // one k-tile: kt+1 (being read) and kt+2 .. kt+NBUF (in flight)
#pragma unroll
  for (int i = 0; i < NBUF; ++i) issue(t0 + i);
  Frags F0, F1;
  if constexpr (NBUF == 4) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // t0 landed, NBUF-1 k-tiles behind it
  else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read(F0, t0);
  // a step that is not the last: kt+1 < t1
  auto step = [&](Frags& cur, Frags& nxt, int kt) {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's reads of kt landed (the compiler sees it)
    if constexpr (NBUF == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // kt+1 landed (NBUF-2 k-tiles in flight)
    else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // kt+1 landed for every wave; nobody reads buffer kt any more
    asm volatile("" ::: "memory");
    issue(kt + NBUF);  // into buffer kt
    read(nxt, kt + 1);
    mfma(cur);
    // copies and reads each behind one MFMA, so the MFMA pipe runs while this wave issues them (all
    // reads then all MFMAs left it idle while both waves of a SIMD issued their copies and reads)
    if constexpr (RW >= 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
#pragma unroll
      for (int i = 0; i < RW + 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, RW * 8 - 4 - (RW + 8), 0);
    } else {  // 8 MFMAs for 4 copies and 9 reads
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
  };
  auto last = [&](Frags& cur) {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    mfma(cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail copies land before exit
  };
  // (the last step shares one body for both parities -- two copies of it spilled 128 VGPRs)
  int kt = t0;
  for (; kt + 2 < t1; kt += 2) {
    step(F0, F1, kt);
    step(F1, F0, kt + 1);
  }
  if (kt + 1 < t1) {
    step(F0, F1, kt);
    F0 = F1;
  }
  last(F0);

  const int tile0 = nb * AT + wn * RW;
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 sv = acc[r][j];
      f32x4 up = sv;
      if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) up[i] = __shfl_xor(sv[i], 32);
      }
      const int col = m0 + wm * 128 + j * 16 + r16;
      if (col >= a.M || (EPI == EPI_SWIGLU && lane >= 32)) continue;
      if constexpr (EPI == EPI_SLAB) {
        const int row = (tile0 + r) * 16 + (lane >> 4) * 4;
        *reinterpret_cast<f32x4*>(a.out + (size_t)ks * a.slab_stride + (size_t)col * a.ldo + row) = sv;
      } else {
        epi_store<EPI>(a, tile0 + r, lane, col, sv, up);
      }
    }
}

bool gemm_supported(int N, int K) { return N % GB_N == 0 && K % GKC == 0; }

template <int EPI>
static void launch_gemm_v(const MMArgs& a, dim3 grid, hipStream_t s) {
  gemm_kernel<EPI, GEMM_NBUF><<<grid, 512, 0, s>>>(a);
}

// K split that brings a small-M GEMM to ~target work-groups (at M <= 256 a Llama-3-8B
// GEMM has 16..112 of them, one per 256 weight rows: most CUs idle), bounded by the slab space
// and by >= 4 K-steps per split; 1 = no split
static int gemm_split(const MMArgs& a, size_t slab_floats, int target) {
  const int base = (a.N / GB_N) * ((a.M + GB_M - 1) / GB_M);
  const int NS = a.K / GKC;
  // a power of two (the resid_norm that folds RESID partials has 1024-thread forms for 2..16)
  int S = 1;
  while (S < 16 && 2 * S * base <= target + base / 2 && 2 * S * 4 <= NS && (size_t)2 * S * a.M * a.N <= slab_floats)
    S *= 2;
  return S;
}

int launch_gemm_split(int epi, const MMArgs& a, float* slabs, size_t slab_floats, int target, hipStream_t s) {
  if (a.M < 1 || !a.X || !gemm_supported(a.N, a.K)) return -1;
  const int S = (slabs && epi != EPI_F32 && target > 0) ? gemm_split(a, slab_floats, target) : 1;
  if (S == 1) return launch_gemm(epi, a, s) ? -1 : 0;
  MMArgs p = a;
  p.out = slabs;
  p.ldo = a.N;
  p.slab_stride = (size_t)a.M * a.N;
  dim3 grid((a.N / GB_N) * ((a.M + GB_M - 1) / GB_M), S);
  launch_gemm_v<EPI_SLAB>(p, grid, s);
  const int total = epi == EPI_SWIGLU ? a.M * a.N / 8 : a.M * a.N / 4;
  const int blocks = std::min((total + 255) / 256, 2048);
  if (epi == EPI_QKV) qkv_finish_kernel<<<blocks, 256, 0, s>>>(a, slabs, S, p.slab_stride);
  else if (epi == EPI_SWIGLU) swiglu_finish_kernel<<<blocks, 256, 0, s>>>(a, slabs, S, p.slab_stride);
  return epi == EPI_RESID ? S : 0;
}

// Row-block height (RW row tiles per wave, 64 RW weight rows per block) for an unsplit GEMM: the
// fewest (rounds of 256 blocks) x (per-block cost ~ RW + 1: the token fragments and copies every
// block pays whatever its height), ties to the taller block.  Llama-3-8B at 4096 rows keeps 256-row
// blocks (q|k|v 192); a 351-row chunk's attn_output / ffn_down take 64-row blocks (128 instead of
// 32 work-groups); TinyLlama's N 2048 GEMMs 128-row blocks.  MX_GEMM_RW (A/B): a fixed height.
static int gemm_rw(int N, int nm) {
  static const int fixed = getenv("MX_GEMM_RW") ? atoi(getenv("MX_GEMM_RW")) : 0;
  if (fixed >= 1 && fixed <= 4 && N % (64 * fixed) == 0) return fixed;
  int best = 4;
  long best_cost = -1;
  for (int rw = 4; rw >= 1; --rw) {
    if (N % (64 * rw)) continue;
    const long blocks = (long)(N / (64 * rw)) * nm;
    const long cost = (blocks + 255) / 256 * (rw + 1);
    if (best_cost < 0 || cost < best_cost) best = rw, best_cost = cost;
  }
  return best;
}

template <int EPI>
static void launch_gemm_rw(const MMArgs& a, int rw, int nm, hipStream_t s) {
  const int grid = (a.N / (64 * rw)) * nm;
  switch (rw) {
    case 4: gemm_kernel<EPI, GEMM_NBUF, 4><<<grid, 512, 0, s>>>(a); return;
    case 3: gemm_kernel<EPI, GEMM_NBUF, 3><<<grid, 512, 0, s>>>(a); return;
    case 2: gemm_kernel<EPI, GEMM_NBUF, 2><<<grid, 512, 0, s>>>(a); return;
    default: gemm_kernel<EPI, GEMM_NBUF, 1><<<grid, 512, 0, s>>>(a); return;
  }
}

int launch_gemm(int epi, const MMArgs& a, hipStream_t s) {
  if (a.M < 1 || !a.X || !gemm_supported(a.N, a.K)) return -1;
  const int nm = (a.M + GB_M - 1) / GB_M;
  const int rw = gemm_rw(a.N, nm);
  switch (epi) {
    case EPI_F32: launch_gemm_rw<EPI_F32>(a, rw, nm, s); return 0;
    case EPI_RESID: launch_gemm_rw<EPI_RESID>(a, rw, nm, s); return 0;
    case EPI_QKV: launch_gemm_rw<EPI_QKV>(a, rw, nm, s); return 0;
    case EPI_SWIGLU: launch_gemm_rw<EPI_SWIGLU>(a, rw, nm, s); return 0;
  }
  return -1;
}

}  // namespace mx

namespace mx {

// ---------------------------------------------------------------------------
// Prefill attention over blocks of 16 consecutive positions of one sequence (flash-style).
// (SURVEY §8a a10 at prefill)  Work-group = (kv head, 16-row block), one wave per query head
// of the GQA group: the 16 queries are the rows of the f16 MFMA tiles, so each K/V chunk feeds
// 16 queries instead of one (the per-row decode kernel re-reads the whole prefix for every
// query).  Same roundings as the decode kernel (f16 q, K, P, V; f32 online softmax over
// 32-position chunks); keys are visited in order, no cross-wave merge.
// ---------------------------------------------------------------------------
template <int D, int G>
__global__ __launch_bounds__(64 * G) void attn_prefill_kernel(AttnArgs a) {
  constexpr int CH = ATTN_CHUNK;
  constexpr int QK = D / 32, DT = D / 16;
  const int kvh = blockIdx.x, blk = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int r0 = blk * 16;
  const int slot = a.slot[r0];
  // per-row query positions: a block's rows are consecutive positions, possibly ending in copies of
  // its last row (the scheduler's padding near n_ctx); keys up to the block's last position
  int qpos[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qpos[i] = a.pos[min(r0 + 4 * q4 + i, a.M - 1)];
  const int hq = kvh * G + w;
  __shared__ __attribute__((aligned(16))) _Float16 Ps[G][16][CH + 8];

  // A operand of QK^T: rows = the block's 16 queries (rows past M re-read the last row)
  f16x8 qa[QK];
  {
    const int row = min(r0 + r16, a.M - 1);
    const float* qrow = a.q + (size_t)row * a.n_head * D + (size_t)hq * D;
#pragma unroll
    for (int kk = 0; kk < QK; ++kk) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qa[kk][j] = (_Float16)v0[j];
        qa[kk][4 + j] = (_Float16)v1[j];
      }
    }
  }
  const _Float16* Kb = a.kc + (size_t)slot * a.slot_stride + (size_t)kvh * a.ctx_stride * D;
  const _Float16* Vb = a.vc + (size_t)slot * a.slot_stride + (size_t)kvh * a.ctx_stride * D;
  float m_i[4], l_i[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_i[i] = -INFINITY;
    l_i[i] = 0.f;
  }
  f32x4 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int last = min(a.pos[min(r0 + 15, a.M - 1)], a.n_ctx - 1);  // newest key any query of the block sees
  for (int p0 = 0; p0 <= last; p0 += CH) {
    f16x8 kf[2][QK], vf[DT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kk = 0; kk < QK; ++kk)
        kf[t][kk] = *reinterpret_cast<const f16x8*>(Kb + (((size_t)(p0 / 16 + t) * QK + kk) * 64 + lane) * 8);
    const int pb = p0 + 8 * q4;
#pragma unroll
    for (int t = 0; t < DT; ++t)
      vf[t] = *reinterpret_cast<const f16x8*>(Vb + (((size_t)(p0 / 32) * DT + t) * 64 + lane) * 8);
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < QK; ++kk) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[kk], kf[t][kk], s[t], 0, 0, 0);
    }
    // C layout: rows = queries 4*q4+i (position qpos[i]), cols = keys p0 + 16t + r16; causal mask
    float e[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qp = qpos[i];
      const float v0 = (p0 + r16 <= qp) ? s[0][i] * a.scale : -INFINITY;
      const float v1 = (p0 + 16 + r16 <= qp) ? s[1][i] * a.scale : -INFINITY;
      const float mx = row16_max(fmaxf(v0, v1));
      const float m_new = fmaxf(m_i[i], mx);
      const float alpha = (m_new == -INFINITY) ? 1.f : expf(m_i[i] - m_new);
      e[0][i] = (m_new == -INFINITY) ? 0.f : expf(v0 - m_new);
      e[1][i] = (m_new == -INFINITY) ? 0.f : expf(v1 - m_new);
      const float ls = row16_sum(e[0][i] + e[1][i]);
      l_i[i] = l_i[i] * alpha + ls;
      m_i[i] = m_new;
#pragma unroll
      for (int t = 0; t < DT; ++t) o[t][i] *= alpha;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) Ps[w][4 * q4 + i][16 * t + r16] = (_Float16)e[t][i];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's P landed
    __builtin_amdgcn_wave_barrier();
    const f16x8 pa = *reinterpret_cast<const f16x8*>(&Ps[w][r16][8 * q4]);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      f16x8 vb = vf[t];
#pragma unroll
      for (int j = 0; j < 8; ++j) vb[j] = (pb + j <= last) ? vb[j] : (_Float16)0.f;  // never-written keys
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, vb, o[t], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();  // Ps[w] rewritten next chunk only after every lane read it
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + 4 * q4 + i;
    if (row >= a.M) continue;
    const float inv = 1.0f / l_i[i];
#pragma unroll
    for (int t = 0; t < DT; ++t)
      if (a.outf) a.outf[(size_t)row * a.ldo + (size_t)hq * D + t * 16 + r16] = o[t][i] * inv;
      else a.out[(size_t)row * a.ldo + (size_t)hq * D + t * 16 + r16] = (uint16_t)f2bf(o[t][i] * inv);
  }
}

template <int D>
static void launch_attn_prefill_d(const AttnArgs& a, hipStream_t s) {
  dim3 grid(a.n_head_kv, (a.M + 15) / 16);
  switch (a.n_head / a.n_head_kv) {
    case 1: attn_prefill_kernel<D, 1><<<grid, 64, 0, s>>>(a); break;
    case 2: attn_prefill_kernel<D, 2><<<grid, 128, 0, s>>>(a); break;
    case 4: attn_prefill_kernel<D, 4><<<grid, 256, 0, s>>>(a); break;
    case 5: attn_prefill_kernel<D, 5><<<grid, 320, 0, s>>>(a); break;
    case 6: attn_prefill_kernel<D, 6><<<grid, 384, 0, s>>>(a); break;
    case 7: attn_prefill_kernel<D, 7><<<grid, 448, 0, s>>>(a); break;
    case 8: attn_prefill_kernel<D, 8><<<grid, 512, 0, s>>>(a); break;
  }
}

void launch_attention_prefill(const AttnArgs& a, hipStream_t s) {
  if (a.head_dim == 64)
    launch_attn_prefill_d<64>(a, s);
  else
    launch_attn_prefill_d<128>(a, s);
}

// ---------------------------------------------------------------------------
// Q8_0 weights  (ggml-common.h block_q8_0, ggml-quants.c)
//
// A Q8_0 GGUF stores each weight row as blocks of 32: f16 scale d + 32 int8 q,
// w = q * d.  ggml's MUL_MAT quantises the f32 activation row to Q8_0 too
// (vec_dot_type of Q8_0) and takes per block (d_w * d_x) * sum(q_w * q_x).
// Here the weights are repacked into 1088-byte tiles (kernels.h) that feed
// v_mfma_i32_16x16x32_i8 directly: one MFMA per 16 rows x one block, the int32
// block sums scaled by d_w * d_x in f32.  Activations are quantised once per
// GEMV by their producer-side kernel (norm or launch_quantize_q8) into rows whose
// 64-k groups are permuted so a lane's 16-byte B fragment of both blocks is one
// load.  Decode reads 1.0625 bytes per weight instead of 2.
// ---------------------------------------------------------------------------

// permuted byte position of logical k in a Q8_0 activation row: within each 64-k group,
// lane group g reads 16 bytes = k 8g..8g+7 (block 0) then k 32+8g..32+8g+7 (block 1)
__device__ __forceinline__ int q8_perm(int k) {
  return (k & ~63) | (((k >> 3) & 3) << 4) | (((k >> 5) & 1) << 3) | (k & 7);
}

// ggml quantize_row_q8_0_ref on one block (weights): ties away from zero
__device__ __forceinline__ void q8_quant_ref(const float (&v)[32], uint16_t& dbits, int8_t (&q)[32]) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
  const float d = amax / 127.0f;
  const float id = d != 0.f ? 1.0f / d : 0.0f;
  dbits = __builtin_bit_cast(uint16_t, (_Float16)d);
#pragma unroll
  for (int j = 0; j < 32; ++j) q[j] = (int8_t)roundf(v[j] * id);
}

// place one block (row, block b) into its packed tile
__device__ __forceinline__ void q8_place(uint8_t* dst, int P, int b, int KT2, uint16_t dbits, const int8_t (&q)[32]) {
  uint8_t* tile = dst + ((size_t)(P >> 4) * KT2 + (b >> 1)) * Q8_TILE_BYTES;
  const int r = P & 15, half = b & 1;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w0 |= (uint32_t)(uint8_t)q[8 * g + j] << (8 * j);
      w1 |= (uint32_t)(uint8_t)q[8 * g + 4 + j] << (8 * j);
    }
    uint32_t* p = reinterpret_cast<uint32_t*>(tile + 16 * (g * 16 + r) + 8 * half);
    p[0] = w0;
    p[1] = w1;
  }
  *reinterpret_cast<uint16_t*>(tile + 1024 + 16 * (r >> 2) + 8 * half + 2 * (r & 3)) = dbits;
}

__global__ void pack_q8_kernel(uint8_t* dst, const uint8_t* src, int N, int K, int mode, int offset) {
  const int nb = K / 32;
  const size_t total = (size_t)N * nb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / nb), b = (int)(i % nb);
    const uint8_t* blk = src + i * 34;
    const uint16_t dbits = (uint16_t)(blk[0] | (blk[1] << 8));
    int8_t q[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) q[j] = (int8_t)blk[2 + j];
    q8_place(dst, packed_row(row, mode, offset), b, K / Q8_TILE_K, dbits, q);
  }
}

// ---- Q4_0 tiles (kernels.h): one lane's 4 bytes of a block -> the int8 A operand of its 8 values,
// q - 8 bytewise (q in 0..15: ((q | 0x80) - 8) ^ 0x80 is the int8 q - 8 without a borrow between bytes)
__device__ __forceinline__ long q4_operand(uint32_t d) {
  uint32_t lo = d & 0x0F0F0F0Fu, hi = (d >> 4) & 0x0F0F0F0Fu;
  lo = ((lo | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
  hi = ((hi | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
  return (long)(((unsigned long)hi << 32) | lo);
}

// The same operand times 16, in 4 VALU ops instead of 10: with x = d ^ 0x88, the nibble x & 0xF read
// as a signed 4-bit value is n - 8, so the byte (x & 0xF) << 4 read as int8 is 16 (n - 8) exactly.
// An int8 MFMA over it returns 16 x the block's integer sum; the caller takes the 16 out of the
// activation scale (d_x / 16: a power of two, so every rounding after it is unchanged).
__device__ __forceinline__ long q4_operand16(uint32_t d) {
  const uint32_t x = d ^ 0x88888888u;
  const uint32_t lo = (x << 4) & 0xF0F0F0F0u, hi = x & 0xF0F0F0F0u;
  return (long)(((unsigned long)hi << 32) | lo);
}

// place one Q4_0 block (row, block b; q = the 32 unsigned nibble values) into its packed tile
__device__ __forceinline__ void q4_place(uint8_t* dst, int P, int b, int KT2, uint16_t dbits, const uint8_t (&q)[32]) {
  uint8_t* tile = dst + ((size_t)(P >> 4) * KT2 + (b >> 1)) * Q4_TILE_BYTES;
  const int r = P & 15, half = b & 1;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (uint32_t)((q[8 * g + j] & 15) | ((q[8 * g + 4 + j] & 15) << 4)) << (8 * j);
    *reinterpret_cast<uint32_t*>(tile + 8 * (g * 16 + r) + 4 * half) = w;
  }
  *reinterpret_cast<uint16_t*>(tile + 512 + 16 * (r >> 2) + 8 * half + 2 * (r & 3)) = dbits;
}

// GGUF block_q4_0 {f16 d; uint8 qs[16]}: qs[j] low nibble = weight j, high nibble = weight j + 16
__global__ void pack_q4_kernel(uint8_t* dst, const uint8_t* src, int N, int K, int mode, int offset) {
  const int nb = K / 32;
  const size_t total = (size_t)N * nb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / nb), b = (int)(i % nb);
    const uint8_t* blk = src + i * 18;
    const uint16_t dbits = (uint16_t)(blk[0] | (blk[1] << 8));
    uint8_t q[32];
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] = blk[2 + j] & 15, q[16 + j] = blk[2 + j] >> 4;
    q4_place(dst, packed_row(row, mode, offset), b, K / Q8_TILE_K, dbits, q);
  }
}

// ggml quantize_row_q4_0_ref: d = (the value of largest magnitude) / -8, q = min(15, (int8)(x / d + 8.5))
// with x / d as x * (1 / d); no contraction (the oracle's C does the same operations: the pragma covers
// only operators written here -- HIP's __fmul_rn / __fadd_rn carry the header's contract flag and fuse)
__device__ __forceinline__ void q4_quant_ref(const float (&v)[32], uint16_t& dbits, uint8_t (&q)[32]) {
#pragma clang fp contract(off)
  float amax = 0.f, mx = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j)
    if (amax < fabsf(v[j])) amax = fabsf(v[j]), mx = v[j];
  const float d = mx / -8.0f;
  const float id = d != 0.f ? 1.0f / d : 0.0f;
  dbits = __builtin_bit_cast(uint16_t, (_Float16)d);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const float t = v[j] * id;
    const int qi = (int)(int8_t)(t + 8.5f);
    q[j] = (uint8_t)min(15, qi);
  }
}

__global__ void synth_q4_packed_kernel(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                                       int offset) {
  const int nb = K / 32;
  const size_t total = (size_t)N * nb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / nb), b = (int)(i % nb);
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = bf2f(f2bf(synth_value(seed, tid, (size_t)row * K + 32 * b + j, scale)));
    uint16_t dbits;
    uint8_t q[32];
    q4_quant_ref(v, dbits, q);
    q4_place(dst, packed_row(row, mode, offset), b, K / Q8_TILE_K, dbits, q);
  }
}

void launch_pack_q4(uint8_t* dst, const uint8_t* src, int N, int K, int mode, int offset, hipStream_t s) {
  pack_q4_kernel<<<fill_grid((size_t)N * (K / 32)), 256, 0, s>>>(dst, src, N, K, mode, offset);
}
void launch_synth_q4_packed(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                            int offset, hipStream_t s) {
  synth_q4_packed_kernel<<<fill_grid((size_t)N * (K / 32)), 256, 0, s>>>(dst, N, K, seed, tid, scale, mode, offset);
}

// synthetic Q8_0 matrix: the quantisation of the bf16 synthetic matrix (synth.py values -> bf16 -> f32)
__device__ __forceinline__ void q8_synth_block(uint64_t seed, uint64_t tid, size_t i0, float scale, uint16_t& dbits,
                                               int8_t (&q)[32]) {
  float v[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) v[j] = bf2f(f2bf(synth_value(seed, tid, i0 + j, scale)));
  q8_quant_ref(v, dbits, q);
}

__global__ void synth_q8_packed_kernel(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                                       int offset) {
  const int nb = K / 32;
  const size_t total = (size_t)N * nb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / nb), b = (int)(i % nb);
    uint16_t dbits;
    int8_t q[32];
    q8_synth_block(seed, tid, (size_t)row * K + 32 * b, scale, dbits, q);
    q8_place(dst, packed_row(row, mode, offset), b, K / Q8_TILE_K, dbits, q);
  }
}

__global__ void synth_q8_rowmajor_kernel(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale) {
  const size_t total = (size_t)N * (K / 32);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    uint16_t dbits;
    int8_t q[32];
    q8_synth_block(seed, tid, i * 32, scale, dbits, q);
    uint8_t* blk = dst + i * 34;
    blk[0] = (uint8_t)dbits;
    blk[1] = (uint8_t)(dbits >> 8);
#pragma unroll
    for (int j = 0; j < 32; ++j) blk[2 + j] = (uint8_t)q[j];
  }
}

// Packed Q8 tiles -> packed bf16 tiles (the prefill GEMM's A operand): ggml's dequantize_row_q8_0
// value d * q in f32, rounded to bf16 like the bf16 path's weights.  One thread per (Q8 tile, lane):
// its 16 bytes are row l&15's k 8(l>>4)..+8 of block 0 and of block 1, i.e. exactly lane l of the
// two bf16 tiles (2kt, 2kt+1) of the same rows.
__global__ void dequant_q8_tiles_kernel(uint16_t* dst, const uint8_t* W, int N, int K) {
  const int KT = K / Q8_TILE_K;
  const size_t total = (size_t)(N / TILE_N) * KT * 64;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const int lane = (int)(u & 63);
    const size_t t = u >> 6;  // Q8 tile index, nt-major
    const uint8_t* tile = W + t * Q8_TILE_BYTES;
    const u32x4 q = *reinterpret_cast<const u32x4*>(tile + 16 * lane);
    const int r = lane & 15;
    const uint16_t* dh = reinterpret_cast<const uint16_t*>(tile + 1024 + 16 * (r >> 2));
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float d = (float)__builtin_bit_cast(_Float16, dh[4 * b + (r & 3)]);
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t qw = q[2 * b + (j >> 1)];
        const float lo = d * (float)(int8_t)(qw >> (16 * (j & 1)));
        const float hi = d * (float)(int8_t)(qw >> (16 * (j & 1) + 8));
        o[j] = f2bf(lo) | (f2bf(hi) << 16);
      }
      *reinterpret_cast<u32x4*>(dst + ((t * 2 + b) * 64 + lane) * 8) = o;
    }
  }
}

int launch_dequant_q8_tiles(uint16_t* dst, const uint8_t* W, int N, int K, hipStream_t s) {
  if (N % TILE_N || K % Q8_TILE_K) return -1;
  const size_t total = (size_t)(N / TILE_N) * (K / Q8_TILE_K) * 64;
  dequant_q8_tiles_kernel<<<fill_grid(total), 256, 0, s>>>(dst, W, N, K);
  return 0;
}

void launch_pack_q8(uint8_t* dst, const uint8_t* src, int N, int K, int mode, int offset, hipStream_t s) {
  pack_q8_kernel<<<fill_grid((size_t)N * K / 32), 256, 0, s>>>(dst, src, N, K, mode, offset);
}
void launch_synth_q8_packed(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                            int offset, hipStream_t s) {
  synth_q8_packed_kernel<<<fill_grid((size_t)N * K / 32), 256, 0, s>>>(dst, N, K, seed, tid, scale, mode, offset);
}
void launch_synth_q8_rowmajor(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, hipStream_t s) {
  synth_q8_rowmajor_kernel<<<fill_grid((size_t)N * K / 32), 256, 0, s>>>(dst, N, K, seed, tid, scale);
}

// ---------------------------------------------------------------------------
// Any other GGUF block type -> bf16 at load (dequantize_row_* of ggml-quants.c in f32, one rounding
// per operation as the C code -- contraction is off here -- then round-to-nearest-even to bf16, a NaN
// staying a NaN: f2bf_nan).
// Used when a file's layer matrices are not all BF16 or all Q8_0 (Q4_K_M, Q5_K_M, Q4_0, F16 ...):
// the model then runs on the bf16 path.  gguf.py dequantize() is the same restatement.
// ---------------------------------------------------------------------------
__global__ void dequant_bf16_kernel(uint16_t* dst, const uint8_t* src, int type, size_t nblocks) {
#pragma clang fp contract(off)  // no fused multiply-subtract: one rounding per operation, as ggml's C
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nblocks; b += (size_t)gridDim.x * blockDim.x) {
    if (type == 0 || type == 1) {  // F32 / F16: "blocks" of 32 values
      uint16_t* y = dst + b * 32;
      for (int j = 0; j < 32; ++j)
        y[j] = (uint16_t)f2bf_nan(type == 0 ? reinterpret_cast<const float*>(src)[b * 32 + j]
                                        : (float)reinterpret_cast<const _Float16*>(src)[b * 32 + j]);
    } else if (type == 2) {  // Q4_0
      const uint8_t* x = src + b * 18;
      const float d = f16b(x);
      uint16_t* y = dst + b * 32;
      for (int j = 0; j < 16; ++j) {
        y[j] = (uint16_t)f2bf_nan((float)((x[2 + j] & 15) - 8) * d);
        y[j + 16] = (uint16_t)f2bf_nan((float)((x[2 + j] >> 4) - 8) * d);
      }
    } else if (type == 8) {  // Q8_0
      const uint8_t* x = src + b * 34;
      const float d = f16b(x);
      uint16_t* y = dst + b * 32;
      for (int j = 0; j < 32; ++j) y[j] = (uint16_t)f2bf_nan((float)(int8_t)x[2 + j] * d);
    } else if (type == 12 || type == 13) {  // Q4_K, Q5_K
      const bool q5 = type == 13;
      const uint8_t* x = src + b * (q5 ? 176 : 144);
      const float d = f16b(x), dmin = f16b(x + 2);
      const uint8_t* scales = x + 4;
      const uint8_t* qh = x + 16;
      const uint8_t* q = x + (q5 ? 48 : 16);
      uint16_t* y = dst + b * 256;
      for (int g = 0; g < 4; ++g) {
        int sc, m;
        scale_min_k4(2 * g, scales, sc, m);
        const float d1 = d * (float)sc, m1 = dmin * (float)m;
        scale_min_k4(2 * g + 1, scales, sc, m);
        const float d2 = d * (float)sc, m2 = dmin * (float)m;
        for (int l = 0; l < 32; ++l) {
          int lo = q[32 * g + l] & 15, hi = q[32 * g + l] >> 4;
          if (q5) {
            lo += (qh[l] & (1 << (2 * g))) ? 16 : 0;
            hi += (qh[l] & (2 << (2 * g))) ? 16 : 0;
          }
          y[64 * g + l] = (uint16_t)f2bf_nan(d1 * (float)lo - m1);
          y[64 * g + 32 + l] = (uint16_t)f2bf_nan(d2 * (float)hi - m2);
        }
      }
    } else if (type == 14) {  // Q6_K
      const uint8_t* x = src + b * 210;
      const uint8_t* ql = x;
      const uint8_t* qh = x + 128;
      const int8_t* sc = reinterpret_cast<const int8_t*>(x + 192);
      const float d = f16b(x + 208);
      uint16_t* y = dst + b * 256;
      for (int h = 0; h < 2; ++h)
        for (int l = 0; l < 32; ++l) {
          const int L0 = ql[64 * h + l], L1 = ql[64 * h + 32 + l], H = qh[32 * h + l];
          const int qv[4] = {((L0 & 15) | (((H >> 0) & 3) << 4)) - 32, ((L1 & 15) | (((H >> 2) & 3) << 4)) - 32,
                             ((L0 >> 4) | (((H >> 4) & 3) << 4)) - 32, ((L1 >> 4) | (((H >> 6) & 3) << 4)) - 32};
          for (int i = 0; i < 4; ++i)
            y[128 * h + 32 * i + l] = (uint16_t)f2bf_nan((d * (float)sc[8 * h + l / 16 + 2 * i]) * (float)qv[i]);
        }
    }
  }
}
int ggml_block_elems(int type) {
  switch (type) {
    case 0: case 1: case 2: case 8: return 32;
    case 12: case 13: case 14: return 256;
  }
  return 0;
}

int launch_dequant_bf16(uint16_t* dst, const uint8_t* src, int type, size_t n, hipStream_t s) {
  const int be = ggml_block_elems(type);
  if (!be || n % be) return -1;
  dequant_bf16_kernel<<<fill_grid(n / be), 256, 0, s>>>(dst, src, type, n / be);
  return 0;
}

// GET_ROWS of a Q8_0 token_embd (dequantize_row_q8_0): x = q * f32(d); thread = one block
// ssq (optional): the per-16-element-tile sums of squares quantise-on-load consumers reduce
__global__ __launch_bounds__(256) void embed_q8_kernel(float* x, const uint8_t* tok, const int* ids, int n,
                                                       float* ssq) {
  const int c = blockIdx.x;
  const uint8_t* row = tok + (size_t)ids[c] * (n / 32) * 34;
  for (int b = threadIdx.x; b < n / 32; b += blockDim.x) {
    const uint8_t* blk = row + (size_t)b * 34;
    const float d = (float)__builtin_bit_cast(_Float16, (uint16_t)(blk[0] | (blk[1] << 8)));
    float* xo = x + (size_t)c * n + 32 * b;
    double q[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
      const f32x4 v{(float)(int8_t)blk[2 + j] * d, (float)(int8_t)blk[3 + j] * d, (float)(int8_t)blk[4 + j] * d,
                    (float)(int8_t)blk[5 + j] * d};
      *reinterpret_cast<f32x4*>(xo + j) = v;
#pragma unroll
      for (int i = 0; i < 4; ++i) q[j >> 4] += (double)(v[i] * v[i]);
    }
    if (ssq) {
      ssq[(size_t)c * (n / 16) + 2 * b] = (float)q[0];
      ssq[(size_t)c * (n / 16) + 2 * b + 1] = (float)q[1];
    }
  }
}

void launch_embed_q8(float* x, const uint8_t* tok, const int* ids, int M, int n, float* ssq, hipStream_t s) {
  embed_q8_kernel<<<M, 256, 0, s>>>(x, tok, ids, n, ssq);
}

// Activation quantisation (ggml quantize_row_q8_0, vec_dot_type of Q8_0): 8 aligned lanes hold the
// 32 values of one block, 4 consecutive each (k = first of them).  d = amax/127, id = d ? 1/d : 0,
// q = round-half-even(v * id) (ggml's AVX2/NEON rounding), d kept as its f16 value.
__device__ __forceinline__ void q8_store_act(f32x4 v, int k, int8_t* qrow, float* drow) {
  float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  amax = fmaxf(amax, __shfl_xor(amax, 4));
  const float d = amax / 127.0f;
  const float id = d != 0.f ? 1.0f / d : 0.0f;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) w |= (uint32_t)(uint8_t)(int8_t)(int)__builtin_rintf(v[j] * id) << (8 * j);
  *reinterpret_cast<uint32_t*>(qrow + q8_perm(k)) = w;
  if ((k & 31) == 0) drow[k >> 5] = round_f16(d);
}

// RMS_NORM + MUL -> Q8_0 rows (norm_generic_kernel's arithmetic, then quantised)
__global__ __launch_bounds__(256) void norm_q8_kernel(int8_t* xq, float* xd, const float* x, const float* w,
                                                      const int* row_map, int n, float eps) {
  const int c = blockIdx.x;
  const int r = row_map ? row_map[c] : c;
  const float* xr = x + (size_t)r * n;
  double acc = 0.0;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)(v[j] * v[j]);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  const double sum = part[0] + part[1] + part[2] + part[3];
  const float scale = 1.0f / sqrtf((float)(sum / n) + eps);
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (v[j] * scale) * g[j];
    q8_store_act(y, i, xq + (size_t)c * n, xd + (size_t)c * (n / 32));
  }
}

// The same after folding the split-K slabs of the GEMV that wrote x (n <= 4096, 1024 threads, no
// row_map): x += slab 0 + slab 1 + ... (resid_norm's order), written back; one 4-value piece per
// thread with x and every slab loaded at once
template <int NS>
__global__ __launch_bounds__(1024) void norm_q8_fold_kernel(int8_t* xq, float* xd, float* x, const float* w, int n,
                                                            float eps, const float* slabs, size_t sstride) {
  const int c = blockIdx.x;
  float* xr = x + (size_t)c * n;
  const int i = threadIdx.x * 4;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  double acc = 0.0;
  if (i < n) {
    f32x4 sl[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sl[k] = *reinterpret_cast<const f32x4*>(slabs + k * sstride + (size_t)c * n + i);
    f32x4 t = sl[0];
#pragma unroll
    for (int k = 1; k < NS; ++k) t += sl[k];
    v = *reinterpret_cast<const f32x4*>(xr + i) + t;  // x + (s0 + s1 + ...): resid_norm's order (norm_kernel)
    *reinterpret_cast<f32x4*>(xr + i) = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)(v[j] * v[j]);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ double part[16];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) sum += part[k];
  const float scale = 1.0f / sqrtf((float)(sum / n) + eps);
  if (i < n) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (v[j] * scale) * g[j];
    q8_store_act(y, i, xq + (size_t)c * n, xd + (size_t)c * (n / 32));
  }
}


__global__ __launch_bounds__(256) void quantize_q8_kernel(int8_t* xq, float* xd, const float* src, int ld, int n) {
  const int c = blockIdx.x;
  for (int i = threadIdx.x * 4; i < n; i += 1024)
    q8_store_act(*reinterpret_cast<const f32x4*>(src + (size_t)c * ld + i), i, xq + (size_t)c * n,
                 xd + (size_t)c * (n / 32));
}

void launch_rmsnorm_q8(int8_t* xq, float* xd, const float* x, const float* w, const int* row_map, int M, int n,
                       float eps, hipStream_t s, const float* slabs, int nslab, size_t slab_stride) {
  if (nslab > 0 && (row_map || n > 4096 || (nslab != 1 && nslab != 2 && nslab != 4 && nslab != 8))) {  // fold first
    launch_resid_norm(nullptr, 0, const_cast<float*>(x), slabs, nslab, slab_stride, nullptr, M, n, eps, s);
    nslab = 0;
  }
  float* xw = const_cast<float*>(x);
  switch (nslab) {  // (row_map / n > 4096 were folded above)
    case 0: norm_q8_kernel<<<M, 256, 0, s>>>(xq, xd, x, w, row_map, n, eps); break;
    case 1: norm_q8_fold_kernel<1><<<M, 1024, 0, s>>>(xq, xd, xw, w, n, eps, slabs, slab_stride); break;
    case 2: norm_q8_fold_kernel<2><<<M, 1024, 0, s>>>(xq, xd, xw, w, n, eps, slabs, slab_stride); break;
    case 4: norm_q8_fold_kernel<4><<<M, 1024, 0, s>>>(xq, xd, xw, w, n, eps, slabs, slab_stride); break;
    default: norm_q8_fold_kernel<8><<<M, 1024, 0, s>>>(xq, xd, xw, w, n, eps, slabs, slab_stride); break;
  }
}
void launch_quantize_q8(int8_t* xq, float* xd, const float* src, int ld, int M, int n, hipStream_t s) {
  quantize_q8_kernel<<<M, 256, 0, s>>>(xq, xd, src, ld, n);
}

// Q8_0 x Q8_0 MUL_MAT: mm_kernel's work split (KS waves over K, RT row tiles, NB column tiles of
// 16 tokens, ring of U tiles per wave) over 1088-byte Q8 tiles; grid.y = groups of 16*NB tokens.
//
// QP > 0 (quantise on load, QM <= 4 tokens, a.xq == nullptr): no activation launch.  Each wave
// reads its K-slice of the f32 source rows (a.xf, row stride K) -- optionally RMS_NORM + MUL with
// the scale from the residual writers' ssq partials, as mm_kernel's XS path -- into registers
// BEFORE issuing its weight ring (QP float4 per lane and row: slice <= 256*QP), then quantises
// them to Q8_0 (8 lanes per block) into a wave-private LDS image its B fragments are read from.
//
// BD (one token): the block-diagonal form of kquant.hip's kq_compute_bd -- 16 consecutive 32-weight
// blocks (8 tiles) of the wave's K-slice share one MFMA accumulator, block j's B operand carrying the
// token's 32 q in column j only, so C column c is block c's exact int32 product for the tile's 16 rows;
// each lane scales its column once per 16 blocks by d_w * d_x of that block (ggml's per-block f32
// product), and one DPP row sum per tile adds the columns.  Same block integers and per-block f32
// products as the per-tile form; only the f32 summation order of the blocks differs.
template <int KS, int RT, int NB, int EPI, int U, int QP, int QM, bool Q4, bool BD = false>
__global__ __launch_bounds__(64 * KS) void mq8_kernel(MMArgs a) {
  static_assert(!BD || (RT == 1 && NB == 1 && 8 % U == 0), "block-diagonal form: one token, one tile, U | 8");
  constexpr int TB = Q4 ? Q4_TILE_BYTES : Q8_TILE_BYTES, SO = Q4 ? 512 : 1024;  // tile bytes, scale offset
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int KT = a.K / Q8_TILE_K;
  const int tile0 = blockIdx.x * RT;
  const int cb = blockIdx.y * 16 * NB;
  const int kb = (KT * w) / KS, ke = (KT * (w + 1)) / KS;

  __shared__ f32x4 red[KS][RT][NB][64];
  extern __shared__ __attribute__((aligned(16))) uint8_t ql_dyn[];  // QP: per-wave Q8 images

  const uint8_t* Wr[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) Wr[r] = reinterpret_cast<const uint8_t*>(a.W) + (size_t)(tile0 + r) * KT * TB;
  const int8_t* Xq[NB];
  const float* Xd[NB];
  // QP image: rows of QB bytes (slice + 16 pad), then QM*QS floats of block scales
  const int QB = (KT + KS - 1) / KS * Q8_TILE_K + 16, QS = (KT + KS - 1) / KS * 2;
  uint8_t* qimg = ql_dyn + (size_t)w * QM * (QB + 4 * QS);
  float* dimg = reinterpret_cast<float*>(qimg + QM * QB);
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    int col = cb + n * 16 + (lane & 15);
    col = col < a.M ? col : a.M - 1;  // padded columns re-read a valid row (outputs dropped)
    if constexpr (QP > 0) {
      Xq[n] = reinterpret_cast<const int8_t*>(qimg) + col * QB + (lane >> 4) * 16 - kb * Q8_TILE_K;
      Xd[n] = dimg + col * QS - 2 * kb;
    } else {
      Xq[n] = a.xq + (size_t)col * a.K + (lane >> 4) * 16;
      Xd[n] = a.xd + (size_t)col * (a.K / 32);
    }
  }

  f32x4 acc[RT][NB];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- QP: this wave's source values and norm operands, loaded before the weight ring
  constexpr int QPn = QP > 0 ? QP : 1, QMn = QP > 0 ? QM : 1;
  f32x4 xv[QMn][QPn], gv[QPn], sv[QMn][2];
  const int nk = (ke - kb) * Q8_TILE_K, kbase = kb * Q8_TILE_K;
  if constexpr (QP > 0) {
    // unconditional loads at clamped addresses (values past the slice / rows are never used): a
    // branch around any of them leaves the compiler's wait counts at the merge conservative, and the
    // image build below then waited for the whole weight ring (vmcnt(0)) instead of these loads
    const float* gsrc = a.norm_w ? a.norm_w : a.xf;
#pragma unroll
    for (int p = 0; p < QP; ++p) {
      const int i = max(0, min(lane * 4 + 256 * p, nk - 4));  // nk = 0: a wave with no K tiles
      gv[p] = *reinterpret_cast<const f32x4*>(gsrc + kbase + i);
#pragma unroll
      for (int c = 0; c < QM; ++c)
        xv[c][p] = *reinterpret_cast<const f32x4*>(a.xf + (size_t)min(c, a.M - 1) * a.K + kbase + i);
    }
    const float* ssrc = a.norm_w ? a.ssq : a.xf;
    const int np = a.norm_w ? a.np : 4;
#pragma unroll
    for (int c = 0; c < QM; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        sv[c][p] = *reinterpret_cast<const f32x4*>(ssrc + (size_t)min(c, a.M - 1) * np + min(lane * 4 + 256 * p, np - 4));
  }

  // one ring slot = one 64-k tile: RT weight tiles (int8 operands + scales) and, from global
  // memory, the NB activation fragments + block scales, loaded together ahead of their use
  struct Frag {
    u32x4 q[RT], d[RT], xb[NB];
    f32x2 dx[NB];
  };
  auto load_w = [&](Frag& f, int kt) {
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const uint8_t* t = Wr[r] + (size_t)kt * TB;
      if constexpr (Q4) {
        const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t) + lane);
        f.q[r] = u32x4{v[0], v[1], 0u, 0u};
      } else {
        f.q[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(t) + lane);
      }
      f.d[r] = *reinterpret_cast<const u32x4*>(t + SO + 16 * (lane >> 4));
    }
    if constexpr (QP == 0) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        f.xb[n] = *reinterpret_cast<const u32x4*>(Xq[n] + kt * Q8_TILE_K);
        f.dx[n] = *reinterpret_cast<const f32x2*>(Xd[n] + 2 * kt);
      }
    }
  };
  auto mma = [&](const Frag& f, int kt) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      u32x4 xb;
      f32x2 dx;
      if constexpr (QP > 0) {
        xb = *reinterpret_cast<const u32x4*>(Xq[n] + kt * Q8_TILE_K);
        dx = *reinterpret_cast<const f32x2*>(Xd[n] + 2 * kt);
      } else {
        xb = f.xb[n];
        dx = f.dx[n];
      }
      const long b0 = (long)(((unsigned long)xb[1] << 32) | xb[0]);
      const long b1 = (long)(((unsigned long)xb[3] << 32) | xb[2]);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const long a0 = Q4 ? q4_operand(f.q[r][0]) : (long)(((unsigned long)f.q[r][1] << 32) | f.q[r][0]);
        const long a1 = Q4 ? q4_operand(f.q[r][1]) : (long)(((unsigned long)f.q[r][3] << 32) | f.q[r][2]);
        const i32x4 p0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, i32x4{0, 0, 0, 0}, 0, 0, 0);
        const i32x4 p1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, i32x4{0, 0, 0, 0}, 0, 0, 0);
        const f16x8 dw = __builtin_bit_cast(f16x8, f.d[r]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[r][n][i] = fmaf((float)dw[i] * dx[0], (float)p0[i], acc[r][n][i]);
          acc[r][n][i] = fmaf((float)dw[4 + i] * dx[1], (float)p1[i], acc[r][n][i]);
        }
      }
    }
  };

  auto build_image = [&]() {  // QP: quantise the wave's K-slice into its LDS image
  if constexpr (QP > 0) {
#pragma unroll
    for (int c = 0; c < QM; ++c) {
      if (c >= a.M) break;
      float sc = 1.0f;
      if (a.norm_w) {
        double sum = 0.0;
#pragma unroll
        for (int p = 0; p < 2; ++p)
          if (lane * 4 + 256 * p < a.np)
#pragma unroll
            for (int j = 0; j < 4; ++j) sum += (double)sv[c][p][j];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
        sc = 1.0f / sqrtf((float)(sum / a.K) + a.eps);
      }
#pragma unroll
      for (int p = 0; p < QP; ++p) {
        const int i = lane * 4 + 256 * p;
        if (i < nk) {
          f32x4 v = xv[c][p];
          if (a.norm_w)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (v[j] * sc) * gv[p][j];
          q8_store_act(v, i, reinterpret_cast<int8_t*>(qimg) + c * QB, dimg + c * QS);
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's image is in LDS
    __builtin_amdgcn_wave_barrier();
  }
  };

  if constexpr (BD) {
    // ring = the weight int8 / nibble parts of the slice's tiles; per group of 8 tiles each lane's
    // own operands: the token's 8 q of block c (c = lane & 15: tile c >> 1, half c & 1), that block's
    // d_x, and the 4 rows' f16 d_w of that block -- loaded one group ahead
    const int c = lane & 15, q = lane >> 4;
    const int8_t* xq0 = QP > 0 ? reinterpret_cast<const int8_t*>(qimg) - kb * Q8_TILE_K : a.xq;
    const float* xd0 = QP > 0 ? dimg - 2 * kb : a.xd;
    u32x4 rq[U];
    auto load_q = [&](int u, int kt) {
      const uint8_t* t = Wr[0] + (size_t)max(0, min(kt, ke - 1)) * TB;
      if constexpr (Q4) {
        const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t) + lane);
        rq[u] = u32x4{v[0], v[1], 0u, 0u};
      } else {
        rq[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(t) + lane);
      }
    };
    struct GrpOps { u32x2 x, dw; float dx; };
    auto load_grp_w = [&](GrpOps& o, int g) {
      const int t = max(0, min(kb + 8 * g + (c >> 1), ke - 1));
      o.dw = *reinterpret_cast<const u32x2*>(Wr[0] + (size_t)t * TB + SO + 16 * q + 8 * (c & 1));
    };
    auto load_grp_x = [&](GrpOps& o, int g) {
      const int tt = kb + 8 * g + (c >> 1), t = max(0, min(tt, ke - 1));
      const u32x2 v = *reinterpret_cast<const u32x2*>(xq0 + (size_t)t * Q8_TILE_K + 16 * q + 8 * (c & 1));
      o.x = tt < ke ? v : u32x2{0u, 0u};  // blocks past the slice add nothing
      o.dx = xd0[2 * t + (c & 1)];
    };
    const int ng = (ke - kb + 7) / 8;
    GrpOps cur, nxt;
#pragma unroll
    for (int u = 0; u < U; ++u) load_q(u, kb + u);
    load_grp_w(cur, 0);
    if constexpr (QP == 0) load_grp_x(cur, 0);
    build_image();
    if constexpr (QP > 0) load_grp_x(cur, 0);
    f32x4 ab = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < ng; ++g) {
      load_grp_w(nxt, g + 1);
      load_grp_x(nxt, g + 1);
      i32x4 C0 = i32x4{0, 0, 0, 0}, C1 = i32x4{0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kt = kb + 8 * g + u;
        if (kt < ke) {  // (wave-uniform)
          const u32x4& f = rq[u % U];
          const long a0 = Q4 ? q4_operand(f[0]) : (long)(((unsigned long)f[1] << 32) | f[0]);
          const long a1 = Q4 ? q4_operand(f[1]) : (long)(((unsigned long)f[3] << 32) | f[2]);
          const bool on0 = c == 2 * u, on1 = c == 2 * u + 1;
          const long b0 = (long)(((unsigned long)(on0 ? cur.x[1] : 0u) << 32) | (on0 ? cur.x[0] : 0u));
          const long b1 = (long)(((unsigned long)(on1 ? cur.x[1] : 0u) << 32) | (on1 ? cur.x[0] : 0u));
          C0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, C0, 0, 0, 0);
          C1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, C1, 0, 0, 0);
        }
        load_q(u % U, kt + U);  // unconditional, clamped (the refill past the slice is unused)
      }
      const f16x4 dw = __builtin_bit_cast(f16x4, cur.dw);
#pragma unroll
      for (int i = 0; i < 4; ++i) ab[i] = fmaf((float)dw[i] * cur.dx, (float)(C0[i] + C1[i]), ab[i]);
      cur = nxt;
    }
    acc[0][0] = f32x4{row16_sum(ab[0]), row16_sum(ab[1]), row16_sum(ab[2]), row16_sum(ab[3])};
  } else {
  Frag ring[U];
  int kt = kb;
  const int nfull = (ke - kb) / U;
#pragma unroll
  for (int u = 0; u < U; ++u) load_w(ring[u], max(0, min(kt + u, ke - 1)));  // unconditional (see xs_load); unused when nfull == 0
  build_image();  // while the ring is in flight
  if (nfull > 0) {
    for (int ch = 1; ch < nfull; ++ch) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        mma(ring[u], kt + u);
        load_w(ring[u], kt + U + u);
      }
      kt += U;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) mma(ring[u], kt + u);
    kt += U;
  }
  for (; kt < ke; ++kt) {
    Frag f;
    load_w(f, kt);
    mma(f, kt);
  }
  }

#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) red[w][r][n][lane] = acc[r][n];
  __syncthreads();

  constexpr int LU = (EPI == EPI_SWIGLU) ? 32 : 64;
  constexpr int UNITS = RT * NB * LU;
  for (int u = threadIdx.x; u < UNITS; u += 64 * KS) {
    const int l = u % LU;
    const int n = (u / LU) % NB;
    const int r = (u / LU) / NB;
    const int col = cb + n * 16 + (l & 15);
    f32x4 s = red[0][r][n][l];
#pragma unroll
    for (int ww = 1; ww < KS; ++ww) s += red[ww][r][n][l];
    if constexpr (EPI == EPI_RESID) {  // residual add + this tile's ssq partial (see mm_kernel)
      double q = 0.0;
      if (col < a.M) {
        f32x4* px = reinterpret_cast<f32x4*>(a.out + (size_t)col * a.ldo + (tile0 + r) * 16 + (l >> 4) * 4);
        const f32x4 xv2 = *px + s;
        *px = xv2;
        q = ssq4(xv2);
      }
      if (a.ssq) {
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        if (l < 16 && col < a.M) a.ssq[(size_t)col * a.np + tile0 + r] = (float)q;
      }
      continue;
    }
    if (col >= a.M) continue;
    f32x4 up = s;
    if constexpr (EPI == EPI_SWIGLU) {
      up = red[0][r][n][l + 32];
#pragma unroll
      for (int ww = 1; ww < KS; ++ww) up += red[ww][r][n][l + 32];
    }
    epi_store<EPI>(a, tile0 + r, l, col, s, up);
  }
}

// quantise-on-load launch: 8 waves (the slice of K per wave <= 256*QP), QM row slots
template <int EPI, int QP, int QM, bool Q4>
static void launch_mq8_ql(const MMArgs& a, hipStream_t s) {
  const int KT = a.K / Q8_TILE_K;
  const int QB = (KT + 7) / 8 * Q8_TILE_K + 16, QS = (KT + 7) / 8 * 2;
  const size_t lds = (size_t)8 * QM * (QB + 4 * QS);
  if constexpr (QM == 1) mq8_kernel<8, 1, 1, EPI, 4, QP, QM, Q4, true><<<dim3(a.N / TILE_N, 1), 512, lds, s>>>(a);
  else mq8_kernel<8, 1, 1, EPI, 4, QP, QM, Q4><<<dim3(a.N / TILE_N, 1), 512, lds, s>>>(a);
}

template <int EPI, int QP, bool Q4>
static void launch_mq8_ql_m(const MMArgs& a, int qm, hipStream_t s) {
  if (qm == 1) launch_mq8_ql<EPI, QP, 1, Q4>(a, s);
  else if (qm == 2) launch_mq8_ql<EPI, QP, 2, Q4>(a, s);
  else launch_mq8_ql<EPI, QP, 4, Q4>(a, s);
}

// One token, K 4096 (Llama-3-8B gate/up): mq8_kernel's block-diagonal quantise-on-load form, but each
// work-group walks TPW tiles (blockIdx.x, +G, ...) with ONE quantised image -- the RMS_NORM + quantise
// prologue once per group instead of once per tile (1792 one-tile groups paid it ~4-5 us per launch,
// profiles/round5_quant_batch1_onload.txt) -- and its weight ring running across the tile seams (as
// mm_pers_kernel).  Per tile the arithmetic and summation order are mq8_kernel<8,1,1,EPI,4,2,1,Q4,true>'s,
// so the results are bit-identical.
template <int TPW, int EPI, bool Q4>
__global__ __launch_bounds__(512) void mq8_pers_ql_kernel(MMArgs a) {
  constexpr int KS = 8, NK = 8, U = 4, KT = KS * NK;  // 8 waves x 8 Q8 tiles = K 4096
  constexpr int TB = Q4 ? Q4_TILE_BYTES : Q8_TILE_BYTES, SO = Q4 ? 512 : 1024;
  constexpr int QB = NK * Q8_TILE_K + 16, QS = NK * 2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kb = w * NK, G = gridDim.x, ntiles = a.N / TILE_N;
  const int c = lane & 15, q = lane >> 4;
  __shared__ f32x4 red[2][KS][64];
  __shared__ __attribute__((aligned(16))) uint8_t qimg_all[KS][QB + 4 * QS];
  uint8_t* qimg = qimg_all[w];
  float* dimg = reinterpret_cast<float*>(qimg + QB);
  auto tile_of = [&](int i) { return min((int)blockIdx.x + i * G, ntiles - 1); };

  // prologue operands (this wave's 512-k slice of x, the norm weights, the ssq partials)
  f32x4 xv[2], gv[2], sv[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int i = lane * 4 + 256 * p;
    gv[p] = *reinterpret_cast<const f32x4*>(a.norm_w + kb * Q8_TILE_K + i);
    xv[p] = *reinterpret_cast<const f32x4*>(a.xf + kb * Q8_TILE_K + i);
    sv[p] = *reinterpret_cast<const f32x4*>(a.ssq + min(lane * 4 + 256 * p, a.np - 4));
  }
  // the weight ring, flat over (tile i, k-tile k): f = i * NK + k
  u32x4 rq[U];
  auto load_q = [&](int f) {
    const uint8_t* t = reinterpret_cast<const uint8_t*>(a.W) + ((size_t)tile_of(f / NK) * KT + kb + f % NK) * TB;
    if constexpr (Q4) {
      const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t) + lane);
      rq[f % U] = u32x4{v[0], v[1], 0u, 0u};
    } else {
      rq[f % U] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(t) + lane);
    }
  };
  auto load_dw = [&](int i) {  // this lane's 4 rows' f16 d_w of block c of tile i
    const int t = kb + (c >> 1);
    return *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint8_t*>(a.W) + ((size_t)tile_of(i) * KT + t) * TB +
                                           SO + 16 * q + 8 * (c & 1));
  };
#pragma unroll
  for (int f = 0; f < U; ++f) load_q(f);
  u32x2 dw = load_dw(0);

  // the image: RMS_NORM scale from the ssq partials (fixed-order double sum), then ggml's Q8_0 blocks
  {
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (lane * 4 + 256 * p < a.np)
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += (double)sv[p][j];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
    const float sc = 1.0f / sqrtf((float)(sum / a.K) + a.eps);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      f32x4 v = xv[p];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (v[j] * sc) * gv[p][j];
      q8_store_act(v, lane * 4 + 256 * p, reinterpret_cast<int8_t*>(qimg), dimg);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's image is in LDS
    __builtin_amdgcn_wave_barrier();
  }
  // this lane's block c of the slice: the same for every tile
  const u32x2 xq = *reinterpret_cast<const u32x2*>(qimg + (c >> 1) * Q8_TILE_K + 16 * q + 8 * (c & 1));
  const float dx = dimg[c];

  constexpr int LU = (EPI == EPI_SWIGLU) ? 32 : 64;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const u32x2 dwc = dw;
    if (i + 1 < TPW) dw = load_dw(i + 1);
    i32x4 C0 = i32x4{0, 0, 0, 0}, C1 = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int f = i * NK + k;
      const u32x4 r = rq[f % U];
      const long a0 = Q4 ? q4_operand(r[0]) : (long)(((unsigned long)r[1] << 32) | r[0]);
      const long a1 = Q4 ? q4_operand(r[1]) : (long)(((unsigned long)r[3] << 32) | r[2]);
      const bool on0 = c == 2 * k, on1 = c == 2 * k + 1;
      const long b0 = (long)(((unsigned long)(on0 ? xq[1] : 0u) << 32) | (on0 ? xq[0] : 0u));
      const long b1 = (long)(((unsigned long)(on1 ? xq[1] : 0u) << 32) | (on1 ? xq[0] : 0u));
      C0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, C0, 0, 0, 0);
      C1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, C1, 0, 0, 0);
      if (f + U < TPW * NK) load_q(f + U);
    }
    const f16x4 dwh = __builtin_bit_cast(f16x4, dwc);
    f32x4 ab = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) ab[j] = fmaf((float)dwh[j] * dx, (float)(C0[j] + C1[j]), ab[j]);
    red[i & 1][w][lane] = f32x4{row16_sum(ab[0]), row16_sum(ab[1]), row16_sum(ab[2]), row16_sum(ab[3])};
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only: the ring stays in flight
    __builtin_amdgcn_s_barrier();
    const int tile = (int)blockIdx.x + i * G;
    if (w == 0 && lane < LU && tile < ntiles && (lane & 15) < a.M) {
      f32x4 sum = red[i & 1][0][lane];
      f32x4 up = (EPI == EPI_SWIGLU) ? red[i & 1][0][lane + 32] : sum;
#pragma unroll
      for (int ww = 1; ww < KS; ++ww) {
        sum += red[i & 1][ww][lane];
        if constexpr (EPI == EPI_SWIGLU) up += red[i & 1][ww][lane + 32];
      }
      epi_store<EPI>(a, tile, lane, lane & 15, sum, up);
    }
  }
}

bool mq8_can_quantize_on_load(int M, int K, bool norm) {
  const int slice = (K / Q8_TILE_K + 7) / 8 * Q8_TILE_K;
  return M >= 1 && M <= XS_MAX_M && K % Q8_TILE_K == 0 && slice <= 2048 && (!norm || K / 16 <= 512);
}

// <= 16 tokens: 8 waves split K, one row tile each (tools/gpu/q8_probe.sh); 17..32 tokens: per
// epilogue, from tools/gpu/q8_probe32.sh (Llama-3-8B, 32 rows): more row tiles per wave for the wide
// matrices (each B fragment loaded from L2 feeds RT MFMAs), one for the 4096-row ones; more: 4 tiles
// (the shapes' configurations: mq8_gemv_cfg)
struct Mq8Cfg {
  int ks, rt, nb, bd;
};
static Mq8Cfg mq8_gemv_cfg(int epi, int M, int ntiles) {
  if (M == 1) return {8, 1, 1, 1};
  if (M <= 16) return {8, 1, 1, 0};
  if (M <= 32) {
    const int cfg = ntiles % 4 ? 0 : epi == EPI_QKV ? 1 : (epi == EPI_SWIGLU || epi == EPI_F32) ? 3 : 0;
    if (cfg == 1) return {8, 2, 2, 0};
    if (cfg == 3) return {4, 4, 2, 0};
    return {8, 1, 2, 0};
  }
  return {8, 1, 4, 0};
}

template <int EPI, bool Q4>
static int launch_mq8_epi(const MMArgs& a, const Mq8Plan& p, hipStream_t s) {
  const int ntiles = a.N / TILE_N;
  if (p.bd) {
    mq8_kernel<8, 1, 1, EPI, 4, 0, 1, Q4, true><<<dim3(ntiles, 1), 512, 0, s>>>(a);
  } else if (p.nb == 1) {
    mq8_kernel<8, 1, 1, EPI, 4, 0, 1, Q4><<<dim3(ntiles, 1), 512, 0, s>>>(a);
  } else if (p.nb == 2) {
    if (p.rt == 2) mq8_kernel<8, 2, 2, EPI, 2, 0, 1, Q4><<<dim3(ntiles / 2, 1), 512, 0, s>>>(a);
    else if (p.rt == 4) mq8_kernel<4, 4, 2, EPI, 2, 0, 1, Q4><<<dim3(ntiles / 4, 1), 256, 0, s>>>(a);
    else mq8_kernel<8, 1, 2, EPI, 4, 0, 1, Q4><<<dim3(ntiles, 1), 512, 0, s>>>(a);
  } else {
    mq8_kernel<8, 1, 4, EPI, 2, 0, 1, Q4><<<dim3(ntiles, p.grid_y), 512, 0, s>>>(a);
  }
  return 0;
}

// quantise on load, one token: tiles per work-group of mq8_pers_ql_kernel, 0 = the one-tile form.
// gate/up 7 tiles per group (1792 = 256 x 7); Q4_0 q|k|v 2 (384 = 192 x 2, as the bf16 mm_pers_kernel:
// 8.76 -> 7.85 us; Q8_0's measured 9.03 -> 9.23 us and keeps one tile per group)
static int mq8_pers_ql_tpw(int epi, bool q4, int M, int N, int K, bool norm) {
  static const bool pers = getenv("MX_NO_Q8_PERS_QL") == nullptr;  // MX_NO_Q8_PERS_QL=1: one tile per group (A/B)
  if (!(epi == EPI_SWIGLU || (epi == EPI_QKV && q4))) return 0;
  const int tpw = epi == EPI_SWIGLU ? 7 : 2;
  return pers && M == 1 && K == 4096 && norm && (N / TILE_N) % tpw == 0 ? tpw : 0;
}
// float4 per lane and row of the quantise-on-load prologue (a wave's K slice <= 256 * QP)
static int mq8_ql_qp(int K) {
  const int slice = (K / Q8_TILE_K + 7) / 8 * Q8_TILE_K;
  return slice <= 512 ? 2 : slice <= 1024 ? 4 : 8;
}

template <int EPI, bool Q4>
static int launch_mq8_ql_epi(const MMArgs& a, const Mq8Plan& p, hipStream_t s) {
  if constexpr (EPI == EPI_SWIGLU || (EPI == EPI_QKV && Q4)) {
    constexpr int TPW = EPI == EPI_SWIGLU ? 7 : 2;
    if (p.kind == MQ8_PERS_QL) {  // (norm on load: launch_mq8 has checked a.ssq and a.np == K / 16 = 256)
      mq8_pers_ql_kernel<TPW, EPI, Q4><<<a.N / TILE_N / TPW, 512, 0, s>>>(a);
      return 0;
    }
  }
  if (p.qp == 2) launch_mq8_ql_m<EPI, 2, Q4>(a, p.qm, s);
  else if (p.qp == 4) launch_mq8_ql_m<EPI, 4, Q4>(a, p.qm, s);
  else launch_mq8_ql_m<EPI, 8, Q4>(a, p.qm, s);
  return 0;
}

// ---------------------------------------------------------------------------
// int32 -> f32 without v_cvt_f32_i32: an int8 MFMA started from these bits (1.5 * 2^23) returns the
// bits of 12582912 + sumi, exact for |sumi| < 2^22 (a Q8_0 block: <= 32 * 127 * 127); subtracting
// 12582912 in f32 (packed, two values per instruction) leaves sumi exactly
constexpr int QG_MAGIC = 0x4B400000;

// Q8_0 GEMV for 17..32 tokens with the activations shared through LDS (mkq_wide_kernel's scheme in
// kquant.hip): each wave owns one 16-row tile over the whole K; the W waves of a work-group share
// each staged 256-k chunk of Q8_0 activation rows (32 tokens x 256 q, k permuted within 64-k groups
// as q8_perm; + the 8 block scales per token), double-buffered in LDS with the next-but-one chunk
// in registers, and each wave keeps a U-chunk ring of its weight tiles (4 Q8 tiles per chunk) in
// flight.  Per 64-k tile the arithmetic is mq8_kernel's (two exact int32 block products, each
// scaled by d_w * d_x in f32); the whole K stays in one wave, so the epilogue runs from registers.
// ---------------------------------------------------------------------------
template <int W, int EPI, int U, bool Q4>
__global__ __launch_bounds__(64 * W, 2) void mq8_wide_kernel(MMArgs a) {
  constexpr int TB = Q4 ? Q4_TILE_BYTES : Q8_TILE_BYTES, SO = Q4 ? 512 : 1024;  // tile bytes, scale offset
  constexpr int NB = 2, ROWS = 32;
  constexpr int QP = 256 + 16;     // int8 per LDS row (+16 B: conflict-free fragment reads)
  constexpr int NQ = ROWS * 16;    // 16-B pieces of q per chunk
  constexpr int ND = ROWS * 2;     // 16-B pieces of the block scales (8 floats per token)
  constexpr int PIECES = NQ + ND;
  constexpr int NT = 64 * W;
  constexpr int PPT = (PIECES + NT - 1) / NT;
  static_assert(U == 2 || U == 4, "ring depth");
  __shared__ __attribute__((aligned(16))) int8_t sq[2][ROWS][QP];
  __shared__ __attribute__((aligned(16))) float sd[2][ROWS][8];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
  const int KT = a.K / Q8_TILE_K;
  // grid.y > 1 (EPI_SLAB): this work-group's K range of 256-k chunks [cb, cb + NCH)
  const int NCHT = a.K / 256, cb = NCHT * blockIdx.y / gridDim.y, NCH = NCHT * (blockIdx.y + 1) / gridDim.y - cb;
  const int tile = blockIdx.x * W + w;
  const uint8_t* Wt = reinterpret_cast<const uint8_t*>(a.W) + ((size_t)tile * KT + cb * 4) * TB;

  const u32x4* xsrc[PPT];
  int xstep[PPT], xdst[PPT];
  bool xq_piece[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = min(tid + i * NT, PIECES - 1);
    if (p < NQ) {
      const int row = p / 16, rr = row < a.M ? row : a.M - 1;
      xsrc[i] = reinterpret_cast<const u32x4*>(a.xq + (size_t)rr * a.K + (size_t)cb * 256 + (p % 16) * 16);
      xstep[i] = 16;
      xdst[i] = row * QP + (p % 16) * 16;
      xq_piece[i] = true;
    } else {
      const int q = p - NQ, row = q / 2, rr = row < a.M ? row : a.M - 1;
      xsrc[i] = reinterpret_cast<const u32x4*>(a.xd + (size_t)rr * (a.K / 32) + cb * 8 + (q % 2) * 4);
      xstep[i] = 2;
      xdst[i] = row * 32 + (q % 2) * 16;
      xq_piece[i] = false;
    }
  }
  u32x4 xr[2][PPT];
  auto load_x = [&](int set, int ch) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) xr[set][i] = xsrc[i][ch * xstep[i]];
  };
  auto store_x = [&](int set, int buf) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      uint8_t* base = xq_piece[i] ? reinterpret_cast<uint8_t*>(&sq[buf][0][0]) : reinterpret_cast<uint8_t*>(&sd[buf][0][0]);
      u32x4 v = xr[set][i];
      if constexpr (Q4) {  // d_x / 16 for q4_operand16's 16 x (n - 8) operands
        const u32x4 v16 = __builtin_bit_cast(u32x4, __builtin_bit_cast(f32x4, v) * 0.0625f);
        v = xq_piece[i] ? v : v16;
      }
      *reinterpret_cast<u32x4*>(base + xdst[i]) = v;
    }
  };
  typedef std::conditional_t<Q4, u32x2, u32x4> QT;  // a lane's share of one tile: 8 B (Q4) / 16 B (Q8)
  struct Frag {
    QT q[4];
    u32x4 d[4];  // the chunk's 4 tiles: int8 (Q4: nibble) operands, f16 block scales of this lane's row group
  };
  Frag ring[U];
  auto load_w = [&](Frag& f, int ch) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* t = Wt + (size_t)(ch * 4 + k) * TB;
      if constexpr (Q4) {
        f.q[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(t) + lane);
      } else {
        f.q[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(t) + lane);
      }
      f.d[k] = *reinterpret_cast<const u32x4*>(t + SO + 16 * (lane >> 4));
    }
  };
  f32x4 acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x(0, 0);
  load_x(1, NCH > 1 ? 1 : 0);
#pragma unroll
  for (int u = 0; u < U; ++u) load_w(ring[u], u < NCH ? u : NCH - 1);
  store_x(0, 0);
  __syncthreads();

  auto step = [&](auto Hc, auto Rc, int ch) {
    constexpr int H = decltype(Hc)::value;
    constexpr int R = decltype(Rc)::value;
    const int buf = ch & 1;
    load_x(H, ch + 2 < NCH ? ch + 2 : NCH - 1);
    const Frag f = ring[R];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      long a0, a1;
      if constexpr (Q4) {
        a0 = q4_operand16(f.q[k][0]);
        a1 = q4_operand16(f.q[k][1]);
      } else {
        a0 = (long)(((unsigned long)f.q[k][1] << 32) | f.q[k][0]);
        a1 = (long)(((unsigned long)f.q[k][3] << 32) | f.q[k][2]);
      }
      const f16x8 dw = __builtin_bit_cast(f16x8, f.d[k]);
      // scaling on packed f32 pairs, int32 -> f32 by the magic accumulator start (QG_MAGIC)
      f32x2 w0[2], w1[2];
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        w0[pp] = f32x2{(float)dw[2 * pp], (float)dw[2 * pp + 1]};
        w1[pp] = f32x2{(float)dw[4 + 2 * pp], (float)dw[4 + 2 * pp + 1]};
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int row = n * 16 + (lane & 15);
        const u32x4 xb = *reinterpret_cast<const u32x4*>(&sq[buf][row][k * 64 + (lane >> 4) * 16]);
        const f32x2 dx = *reinterpret_cast<const f32x2*>(&sd[buf][row][2 * k]);
        const long b0 = (long)(((unsigned long)xb[1] << 32) | xb[0]);
        const long b1 = (long)(((unsigned long)xb[3] << 32) | xb[2]);
        const i32x4 mg = i32x4{QG_MAGIC, QG_MAGIC, QG_MAGIC, QG_MAGIC};
        const f32x4 x0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, mg, 0, 0, 0));
        const f32x4 x1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, mg, 0, 0, 0));
        const f32x2 dx0 = f32x2{dx[0], dx[0]}, dx1 = f32x2{dx[1], dx[1]};
        const f32x2 off = f32x2{12582912.0f, 12582912.0f};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          f32x2 c = f32x2{acc[n][2 * pp], acc[n][2 * pp + 1]};
          c = __builtin_elementwise_fma(w0[pp] * dx0, f32x2{x0[2 * pp], x0[2 * pp + 1]} - off, c);
          c = __builtin_elementwise_fma(w1[pp] * dx1, f32x2{x1[2 * pp], x1[2 * pp + 1]} - off, c);
          acc[n][2 * pp] = c[0];
          acc[n][2 * pp + 1] = c[1];
        }
      }
    }
    load_w(ring[R], min(ch + U, NCH - 1));  // past the end: re-read the last chunk (no branch)
    store_x(1 - H, buf ^ 1);
    __syncthreads();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  for (int ch = 0; ch < NCH; ch += U) {
    step(I0{}, I0{}, ch);
    if (ch + 1 < NCH) step(I1{}, I1{}, ch + 1);
    if constexpr (U == 4) {
      if (ch + 2 < NCH) step(I0{}, I2{}, ch + 2);
      if (ch + 3 < NCH) step(I1{}, I3{}, ch + 3);
    }
  }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const f32x4 sv = acc[n];
    f32x4 up = sv;
    if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
      for (int i = 0; i < 4; ++i) up[i] = __shfl_xor(sv[i], 32);
    }
    const int col = n * 16 + (lane & 15);
    if (col >= a.M || (EPI == EPI_SWIGLU && lane >= 32)) continue;
    if constexpr (EPI == EPI_SLAB)  // partial over this K range: slab blockIdx.y [token][N]
      *reinterpret_cast<f32x4*>(a.out + blockIdx.y * a.slab_stride + (size_t)col * a.ldo + tile * 16 + (lane >> 4) * 4) = sv;
    else
      epi_store<EPI>(a, tile, lane, col, sv, up);
  }
}

// The same GEMV with the MFMA operands swapped: the activations are A (token rows) and the weight tile
// is B, so a lane's C values are 4 TOKENS of ONE weight row (lane & 15).  Its two block scales d_w are
// then two f16 per tile (two 2-byte loads, two converts) instead of eight (4 rows x 2 blocks), and
// the 4 d_x of its tokens one 16-byte LDS read per block from a block-major d_x image; the products
// t = d_x * d_w, the int32 -> f32 (magic start) and the fma are unchanged, so the sums are bit-identical
// to mq8_wide_kernel's.  The weights come through a buffer resource with the tile offset in a scalar
// (no per-load 64-bit address arithmetic); the C layout is transposed back through LDS at the end
// (per wave, once) for the usual epilogues.  Used for Q4_0 (Llama-3-8B gate/up at 32 rows 23.5 vs
// 24.8 us); Q8_0 measured slower (27.5 vs 24.7 us: profiles/round5_quant_wide_variants.txt).
template <int W, int EPI, int U, bool Q4>
__global__ __launch_bounds__(64 * W) void mq8_wsw_kernel(MMArgs a) {
  constexpr int TB = Q4 ? Q4_TILE_BYTES : Q8_TILE_BYTES, SO = Q4 ? 512 : 1024;
  constexpr int NB = 2, ROWS = 32;
  constexpr int QP = 256 + 16;   // int8 per LDS row (+16 B: conflict-free fragment reads)
  constexpr int NQ = ROWS * 16;  // 16-B pieces of q per chunk
  constexpr int ND = ROWS * 2;   // 16-B pieces of the block scales (8 floats per token)
  constexpr int NT = 64 * W;
  constexpr int PPT = (NQ + NT - 1) / NT;
  static_assert(U == 2 || U == 4, "ring depth");
  static_assert(ND <= 64, "the block scales are staged by wave 0");
  __shared__ __attribute__((aligned(16))) int8_t sq[2][ROWS][QP];
  __shared__ __attribute__((aligned(16))) float sdt[2][8][ROWS];      // d_x block-major
  __shared__ __attribute__((aligned(16))) float tr[W][NB][16][20];    // epilogue transpose

  const int lane = threadIdx.x & 63, tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KT = a.K / Q8_TILE_K;
  // grid.y > 1 (EPI_SLAB): this work-group's K range of 256-k chunks [cb, cb + NCH)
  const int NCHT = a.K / 256, cb = NCHT * blockIdx.y / gridDim.y, NCH = NCHT * (blockIdx.y + 1) / gridDim.y - cb;
  const int tile = blockIdx.x * W + w;
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(a.W) + ((size_t)tile * KT + cb * 4) * TB), (short)0,
      NCH * 4 * TB, 0x00020000);
  const int r = lane & 15;
  const unsigned qoff = lane * (Q4 ? 8u : 16u), doff = SO + 16 * (r >> 2) + 4 * ((r & 3) >> 1);
  const unsigned dsh = 16 * (r & 1);

  const u32x4* xsrc[PPT];
  int xdst[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = min(tid + i * NT, NQ - 1);
    const int row = p / 16, rr = row < a.M ? row : a.M - 1;
    xsrc[i] = reinterpret_cast<const u32x4*>(a.xq + (size_t)rr * a.K + (size_t)cb * 256 + (p % 16) * 16);
    xdst[i] = row * QP + (p % 16) * 16;
  }
  const int drow = min(tid >> 1, ROWS - 1), drr = drow < a.M ? drow : a.M - 1, dhalf = tid & 1;
  const u32x4* dsrc = reinterpret_cast<const u32x4*>(a.xd + (size_t)drr * (a.K / 32) + cb * 8 + dhalf * 4);
  u32x4 xr[2][PPT], dr[2];
  auto load_x = [&](int set, int ch) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) xr[set][i] = xsrc[i][ch * 16];
    if (w == 0) dr[set] = dsrc[ch * 2];
  };
  auto store_x = [&](int set, int buf) {
#pragma unroll
    for (int i = 0; i < PPT; ++i)
      *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(&sq[buf][0][0]) + xdst[i]) = xr[set][i];
    if (w == 0) {
      f32x4 d = __builtin_bit_cast(f32x4, dr[set]);
      if constexpr (Q4) d = d * 0.0625f;  // d_x / 16 for q4_operand16's 16 x (n - 8) operands
#pragma unroll
      for (int e = 0; e < 4; ++e) sdt[buf][dhalf * 4 + e][drow] = d[e];
    }
  };
  typedef std::conditional_t<Q4, u32x2, u32x4> QT;
  struct Frag {
    QT q[4];
    // f16 d_w of blocks 0 / 1 of each tile: the dword holding this lane's row and its neighbour, the half
    // selected at use.  16-bit loads made hipcc mask or pack the ring as it arrived -- a wait for every
    // load, vmcnt(0), before each barrier (round 5: Llama-3-8B gate/up at 32 rows 23.35 -> 21.5 us)
    uint32_t d0[4], d1[4];
  };
  Frag ring[U];
  auto load_w = [&](Frag& f, int ch) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int so = (ch * 4 + k) * TB;
      if constexpr (Q4)
        f.q[k] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(wrs, qoff, so, 2));
      else
        f.q[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, qoff, so, 2));
      f.d0[k] = __builtin_amdgcn_raw_buffer_load_b32(wrs, doff, so, 0);
      f.d1[k] = __builtin_amdgcn_raw_buffer_load_b32(wrs, doff + 8, so, 0);
    }
  };
  f32x4 acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x(0, 0);
  load_x(1, NCH > 1 ? 1 : 0);
#pragma unroll
  for (int u = 0; u < U; ++u) load_w(ring[u], u < NCH ? u : NCH - 1);
  store_x(0, 0);
  __syncthreads();

  const int q4 = (lane >> 4) * 4;
  auto step = [&](auto Hc, auto Rc, int ch) {
    constexpr int H = decltype(Hc)::value;
    constexpr int R = decltype(Rc)::value;
    const int buf = ch & 1;
    load_x(H, ch + 2 < NCH ? ch + 2 : NCH - 1);
    const Frag f = ring[R];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      long b0, b1;
      if constexpr (Q4) {
        b0 = q4_operand16(f.q[k][0]);
        b1 = q4_operand16(f.q[k][1]);
      } else {
        b0 = (long)(((unsigned long)f.q[k][1] << 32) | f.q[k][0]);
        b1 = (long)(((unsigned long)f.q[k][3] << 32) | f.q[k][2]);
      }
      const float w0 = (float)__builtin_bit_cast(_Float16, (uint16_t)(f.d0[k] >> dsh));
      const float w1 = (float)__builtin_bit_cast(_Float16, (uint16_t)(f.d1[k] >> dsh));
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int row = n * 16 + (lane & 15);
        const u32x4 xb = *reinterpret_cast<const u32x4*>(&sq[buf][row][k * 64 + (lane >> 4) * 16]);
        const f32x4 dx0 = *reinterpret_cast<const f32x4*>(&sdt[buf][2 * k][n * 16 + q4]);
        const f32x4 dx1 = *reinterpret_cast<const f32x4*>(&sdt[buf][2 * k + 1][n * 16 + q4]);
        const long a0 = (long)(((unsigned long)xb[1] << 32) | xb[0]);
        const long a1 = (long)(((unsigned long)xb[3] << 32) | xb[2]);
        const i32x4 mg = i32x4{QG_MAGIC, QG_MAGIC, QG_MAGIC, QG_MAGIC};
        const f32x4 x0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, mg, 0, 0, 0));
        const f32x4 x1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, mg, 0, 0, 0));
        const f32x2 off = f32x2{12582912.0f, 12582912.0f};
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          f32x2 c = f32x2{acc[n][2 * pp], acc[n][2 * pp + 1]};
          c = __builtin_elementwise_fma(f32x2{dx0[2 * pp], dx0[2 * pp + 1]} * f32x2{w0, w0},
                                        f32x2{x0[2 * pp], x0[2 * pp + 1]} - off, c);
          c = __builtin_elementwise_fma(f32x2{dx1[2 * pp], dx1[2 * pp + 1]} * f32x2{w1, w1},
                                        f32x2{x1[2 * pp], x1[2 * pp + 1]} - off, c);
          acc[n][2 * pp] = c[0];
          acc[n][2 * pp + 1] = c[1];
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // one tile at a time (hoisted LDS reads of all four spill)
    }
    load_w(ring[R], min(ch + U, NCH - 1));  // past the end: re-read the last chunk (no branch)
    store_x(1 - H, buf ^ 1);
    __syncthreads();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  // 4 steps per trip either way: the ring's registers are renamed at the back-edge after a vmcnt(0), so
  // a 2-deep ring goes round twice per trip (21.5 -> 20.95 us; a 4-deep ring spills, 24.4 us; all
  // steps unconditional, or the chunk loop fully unrolled, spill 115-1850 VGPRs)
  for (int ch = 0; ch < NCH; ch += 4) {
    step(I0{}, I0{}, ch);
    if (ch + 1 < NCH) step(I1{}, I1{}, ch + 1);
    if constexpr (U == 4) {
      if (ch + 2 < NCH) step(I0{}, I2{}, ch + 2);
      if (ch + 3 < NCH) step(I1{}, I3{}, ch + 3);
    } else {
      if (ch + 2 < NCH) step(I0{}, I0{}, ch + 2);
      if (ch + 3 < NCH) step(I1{}, I1{}, ch + 3);
    }
  }
  // C^T -> the usual layout through this wave's tr
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[w][n][q4 + i][r] = acc[n][i];  // [token][weight row]
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's own writes, read back below
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = *reinterpret_cast<const f32x4*>(&tr[w][n][r][q4]);
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const f32x4 sv = acc[n];
    f32x4 up = sv;
    if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
      for (int i = 0; i < 4; ++i) up[i] = __shfl_xor(sv[i], 32);
    }
    const int col = n * 16 + (lane & 15);
    if (col >= a.M || (EPI == EPI_SWIGLU && lane >= 32)) continue;
    if constexpr (EPI == EPI_SLAB)
      *reinterpret_cast<f32x4*>(a.out + blockIdx.y * a.slab_stride + (size_t)col * a.ldo + tile * 16 + (lane >> 4) * 4) = sv;
    else
      epi_store<EPI>(a, tile, lane, col, sv, up);
  }
}

// 17..32 tokens, attn_output / ffn_down / q|k|v of a Q8_0 file: 4-wave groups, K split over grid.y
// until ~256 work-groups, partial slabs [ks][token][N] (folded by launch_rmsnorm_q8's FOLD form, or
// finished by the decode attention / launch_qkv_finish).  Returns ks, or -1 (use launch_mq8).
static bool mq8_wide_off() {
  static const bool off = getenv("MX_NO_Q8_WIDE") != nullptr;
  return off;
}
int mq8_slab_ks(int M, int N, int K) {
  if (mq8_wide_off() || M <= 16 || M > 32 || K < 256 || K % 256 || N < 64 || N % 64) return -1;
  const int ntiles = N / TILE_N, NCH = K / 256;
  int ks = 1;
  static const int tgt = getenv("MX_SLAB_TARGET") ? atoi(getenv("MX_SLAB_TARGET")) : 256;  // A/B
  while (ks < 8 && (ntiles / 4) * ks * 2 <= tgt && NCH / (ks * 2) >= 4) ks *= 2;
  return ks;
}
int launch_mq8_slab(const MMArgs& a, float* slabs, size_t slab_stride, hipStream_t s) {
  if (!a.xq || !a.xd) return -1;
  const int ks = mq8_slab_ks(a.M, a.N, a.K);
  if (ks < 0) return -1;
  const int ntiles = a.N / TILE_N;
  MMArgs p = a;
  p.out = slabs;
  p.ldo = a.N;
  p.slab_stride = slab_stride;
  if (a.wq4) mq8_wide_kernel<4, EPI_SLAB, 2, true><<<dim3(ntiles / 4, ks), 256, 0, s>>>(p);
  else mq8_wide_kernel<4, EPI_SLAB, 2, false><<<dim3(ntiles / 4, ks), 256, 0, s>>>(p);
  return ks;
}

// 17..32 tokens, gate/up or lm_head of a Q8_0 file: the LDS-shared form (MX_NO_Q8_WIDE=1: mq8_kernel)
// row tiles (waves) per work-group of the LDS-shared form, 0 = the shape has none
static int mq8_wide_w(int epi, int M, int N, int K) {
  const int ntiles = N / TILE_N;
  if (mq8_wide_off() || M <= 16 || M > 32 || K % 256) return 0;
  if (epi != EPI_SWIGLU && epi != EPI_F32) return 0;
  if (ntiles % 7 == 0 && ntiles / 7 >= 200) return 7;
  if (ntiles % 8 == 0 && ntiles / 8 >= 200) return 8;
  if (ntiles % 4 == 0) return 4;
  return 0;
}
static int launch_mq8_wide(int epi, const MMArgs& a, int w, hipStream_t s) {
  const int ntiles = a.N / TILE_N;
  auto go = [&](auto wc) {
    constexpr int W = decltype(wc)::value;
    if (a.wq4) {  // Q4_0: the swapped-operand form
      if (epi == EPI_SWIGLU) mq8_wsw_kernel<W, EPI_SWIGLU, 2, true><<<ntiles / W, 64 * W, 0, s>>>(a);
      else mq8_wsw_kernel<W, EPI_F32, 2, true><<<ntiles / W, 64 * W, 0, s>>>(a);
    } else {
      if (epi == EPI_SWIGLU) mq8_wide_kernel<W, EPI_SWIGLU, 2, false><<<ntiles / W, 64 * W, 0, s>>>(a);
      else mq8_wide_kernel<W, EPI_F32, 2, false><<<ntiles / W, 64 * W, 0, s>>>(a);
    }
    return 0;
  };
  if (w == 7) return go(std::integral_constant<int, 7>{});
  if (w == 8) return go(std::integral_constant<int, 8>{});
  if (w == 4) return go(std::integral_constant<int, 4>{});
  return -1;
}

// ---------------------------------------------------------------------------
// Q8_0 x Q8_0 prompt GEMM (>= Q8_GEMM_MIN_M rows): ggml's ggml_vec_dot_q8_0_q8_0 arithmetic -- per
// 32-weight block the exact int32 product of the two int8 vectors (v_mfma_i32_16x16x32_i8: K = one
// block), times d_w * d_x, summed in f32 -- as a blocked GEMM instead of the GEMV kernels above
// (which re-stream every weight tile once per 64 tokens).  Block = 8 waves, 256 weight rows (16 Q8
// tiles) x 128 tokens; wave (wn, wm) = 4 row tiles x 4 token tiles, 32 MFMAs per 64-deep k-step.
// Staged global -> LDS by LDS-DMA, one k-step (one Q8 tile column) per ring buffer: the 16 tiles'
// int8 parts (lane-linear 1 KiB A images, copied verbatim), the 128 tokens' q (gathered into the same
// lane-linear B images), the tiles' f16 d_w (64 B each) and the tokens' d_x (two floats each); the
// k-loop is gemm_kernel's (constant counted waits, copies and reads behind MFMAs).  The f32 scaling
// (per block and output: d_w * d_x, convert, fma) is VALU work of the same count as the MFMAs' MACs
// / 32 -- it, not the MFMA, bounds this kernel.
// ---------------------------------------------------------------------------
constexpr int Q8_GEMM_MIN_M = 256;
constexpr int QG_M = 128, QG_NBUF = 4;
// per buffer: A images [16][1 KiB], B images [8][1 KiB], then per wave w 256 B of scales: the d_x of
// tokens 16w..16w+15 ([token][2] floats, 128 B) and the d_w of tiles 2w, 2w+1 (64 B each)
constexpr int QG_A = 0, QG_B = 16384, QG_SC = QG_B + 8192, QG_BUF = QG_SC + 2048;

template <int EPI, bool Q4>
__global__ __launch_bounds__(512, 1) void q8gemm_kernel(MMArgs a) {
  constexpr int NBUF = QG_NBUF;
  // Q4 (Q4_0 tiles, ggml_vec_dot_q4_0_q8_0): 512-byte nibble parts (two tiles per copy, 8 bytes per
  // lane, expanded to the int8 q - 8 by q4_operand), scales at byte 512
  constexpr int TB = Q4 ? Q4_TILE_BYTES : Q8_TILE_BYTES, SO = Q4 ? 512 : 1024, AB = Q4 ? 512 : 1024;
  __shared__ __attribute__((aligned(1024))) uint8_t lds[NBUF * QG_BUF];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = w & 3, wm = w >> 2;
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, q = nwg / 8, rr = nwg % 8;
  const int wgid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
  const int nmb = (a.M + QG_M - 1) / QG_M;
  const int mb = wgid % nmb, nb = wgid / nmb;
  const int KT = a.K / Q8_TILE_K, KB = a.K / 32;
  const int t0 = 0, t1 = KT;
  const int m0 = mb * QG_M;

  // copies: wave w moves A tiles 2w, 2w+1 (int8 parts), token tile w, and in ONE 4-byte copy its
  // scales: lanes 0..31 the d_x of tokens 16w..16w+15 (one float each), lanes 32..63 the d_w of
  // tiles 2w, 2w+1 (one f16 pair each)
  const uint8_t* abase = reinterpret_cast<const uint8_t*>(a.W) + (size_t)(nb * 16 + 2 * w) * KT * TB;
  const size_t astep = (size_t)KT * TB;
  const int tokb = min(m0 + w * 16 + (lane & 15), a.M - 1);
  const int8_t* bsrc = a.xq + (size_t)tokb * a.K + (lane >> 4) * 16;
  const int tokd = min(m0 + w * 16 + ((lane & 31) >> 1), a.M - 1);
  const uint8_t* scsrc = lane < 32 ? reinterpret_cast<const uint8_t*>(a.xd + (size_t)tokd * KB + (lane & 1))
                                   : abase + (size_t)((lane >> 4) & 1) * astep + SO + 4 * (lane & 15);
  const int scstep = lane < 32 ? 8 : TB;  // bytes per k-step
  auto issue = [&](int kt_buf) {  // k-step min(kt_buf, t1-1) into buffer kt_buf % NBUF
    uint8_t* base = lds + (kt_buf % NBUF) * QG_BUF;
    const int kt = min(kt_buf, t1 - 1);
    if constexpr (Q4) {
      __builtin_amdgcn_global_load_lds((gvoid*)(abase + (lane >> 5) * astep + (size_t)kt * TB + (lane & 31) * 16),
                                       (lvoid*)(base + QG_A + w * 1024), 16, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((gvoid*)(abase + i * astep + (size_t)kt * TB + lane * 16),
                                         (lvoid*)(base + QG_A + (2 * w + i) * 1024), 16, 0, 0);
    }
    __builtin_amdgcn_global_load_lds((gvoid*)(bsrc + (size_t)kt * Q8_TILE_K), (lvoid*)(base + QG_B + w * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gvoid*)(scsrc + (size_t)kt * scstep), (lvoid*)(base + QG_SC + w * 256), 4, 0, 0);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frags {
    u32x4 a[4], b[4], dw[4];
    f32x2 dx[4];
  };
  auto read = [&](Frags& f, int kt) {
    const uint8_t* B0 = lds + (kt % NBUF) * QG_BUF;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (Q4) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(B0 + QG_A + (wn * 4 + r) * AB + lane * 8);
        f.a[r] = u32x4{v[0], v[1], 0u, 0u};
      } else {
        f.a[r] = *reinterpret_cast<const u32x4*>(B0 + QG_A + (wn * 4 + r) * AB + lane * 16);
      }
      const int T = wn * 4 + r;
      f.dw[r] = *reinterpret_cast<const u32x4*>(B0 + QG_SC + (T >> 1) * 256 + 128 + (T & 1) * 64 + 16 * (lane >> 4));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f.b[j] = *reinterpret_cast<const u32x4*>(B0 + QG_B + (wm * 4 + j) * 1024 + lane * 16);
      f.dx[j] = *reinterpret_cast<const f32x2*>(B0 + QG_SC + (wm * 4 + j) * 256 + (lane & 15) * 8);
    }
  };
  // The per-block f32 step is mq8_kernel's -- acc = fma(d_w * d_x, (float)sumi, acc), block 0 then
  // block 1 -- on packed f32 pairs.  (float)sumi without v_cvt_f32_i32 (not packable): the MFMA
  // starts from C = 0x4B400000, the bits of 1.5 * 2^23, so it returns the bits of 12582912 + sumi
  // exactly (|sumi| <= 32 * 127 * 127 < 2^22 keeps the exponent), and one packed subtract of
  // 12582912 leaves sumi exactly.  4 copies (Q4: 3) per wave and k-step, NBUF-2 k-steps in flight
  // behind the one being read.  Pipelined row tile by row tile: the 8 MFMAs of row tile r+1 go into
  // one of two result sets while row tile r is scaled from the other (64 result VGPRs instead of
  // 128), and the NEXT k-step's fragments are read from LDS while this one's MFMAs run (two fragment
  // sets, gemm_kernel's step).  Round 5: 1555 -> 1491 us for the Llama-3-8B gate/up at 4096 rows,
  // Q4_0 1647 -> 1530, against holding all 32 results at once and reading the k-step's fragments at
  // its top.  Unpacking Q4 at 16x (q4_operand16, d_w / 16) measured 1530 -> 1650 us here, rejected.
  auto mfma_r = [&](const Frags& f, auto Rc, f32x4 (&x)[4][2]) {
    constexpr int r = decltype(Rc)::value;
    const long a0 = Q4 ? q4_operand(f.a[r][0]) : (long)(((unsigned long)f.a[r][1] << 32) | f.a[r][0]);
    const long a1 = Q4 ? q4_operand(f.a[r][1]) : (long)(((unsigned long)f.a[r][3] << 32) | f.a[r][2]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long b0 = (long)(((unsigned long)f.b[j][1] << 32) | f.b[j][0]);
      const long b1 = (long)(((unsigned long)f.b[j][3] << 32) | f.b[j][2]);
      const i32x4 mg = i32x4{QG_MAGIC, QG_MAGIC, QG_MAGIC, QG_MAGIC};
      x[j][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, b0, mg, 0, 0, 0));
      x[j][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, b1, mg, 0, 0, 0));
    }
  };
  auto scale_r = [&](const Frags& f, auto Rc, const f32x4 (&x)[4][2]) {
    constexpr int r = decltype(Rc)::value;
    const f16x8 dw = __builtin_bit_cast(f16x8, f.dw[r]);
    f32x2 dwp[2][2];  // [block][row pair]
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) dwp[b][pp] = f32x2{(float)dw[4 * b + 2 * pp], (float)dw[4 * b + 2 * pp + 1]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 dx0 = f32x2{f.dx[j][0], f.dx[j][0]}, dx1 = f32x2{f.dx[j][1], f.dx[j][1]};
      const f32x2 off = f32x2{12582912.0f, 12582912.0f};
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        f32x2 c = f32x2{acc[r][j][2 * pp], acc[r][j][2 * pp + 1]};
        c = __builtin_elementwise_fma(dwp[0][pp] * dx0, f32x2{x[j][0][2 * pp], x[j][0][2 * pp + 1]} - off, c);
        c = __builtin_elementwise_fma(dwp[1][pp] * dx1, f32x2{x[j][1][2 * pp], x[j][1][2 * pp + 1]} - off, c);
        acc[r][j][2 * pp] = c[0];
        acc[r][j][2 * pp + 1] = c[1];
      }
    }
  };
  using R0 = std::integral_constant<int, 0>;
  using R1 = std::integral_constant<int, 1>;
  using R2 = std::integral_constant<int, 2>;
  using R3 = std::integral_constant<int, 3>;
  auto compute = [&](const Frags& f) {
    f32x4 xa[4][2], xb[4][2];
    mfma_r(f, R0{}, xa);
    mfma_r(f, R1{}, xb);
    scale_r(f, R0{}, xa);
    mfma_r(f, R2{}, xa);
    scale_r(f, R1{}, xb);
    mfma_r(f, R3{}, xb);
    scale_r(f, R2{}, xa);
    scale_r(f, R3{}, xb);
  };
#pragma unroll
  for (int i = 0; i < NBUF; ++i) issue(t0 + i);
  if constexpr (Q4) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");  // t0 landed, NBUF-1 k-steps behind it
  else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  Frags F0, F1;
  read(F0, t0);
  auto step = [&](Frags& cur, Frags& nxt, int kt) {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's reads of kt landed
    if constexpr (Q4) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // kt+1 landed (NBUF-2 k-steps in flight)
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // kt+1 landed for every wave; nobody reads buffer kt any more
    asm volatile("" ::: "memory");
    issue(kt + NBUF);  // into buffer kt
    read(nxt, kt + 1);
    compute(cur);
  };
  int kt = t0;
  for (; kt + 2 < t1; kt += 2) {
    step(F0, F1, kt);
    step(F1, F0, kt + 1);
  }
  if (kt + 1 < t1) {
    step(F0, F1, kt);
    F0 = F1;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  compute(F0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail copies land before exit

  const int tile0 = nb * 16 + wn * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 sv = acc[r][j];
      f32x4 up = sv;
      if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) up[i] = __shfl_xor(sv[i], 32);
      }
      const int col = m0 + wm * 64 + j * 16 + (lane & 15);
      if (col >= a.M || (EPI == EPI_SWIGLU && lane >= 32)) continue;
      epi_store<EPI>(a, tile0 + r, lane, col, sv, up);
    }
}

// A blocked grid of fewer than QG_MIN_GRID work-groups leaves most CUs idle for a whole K sweep;
// the GEMVs (one weight pass per 64 tokens, every CU busy) are then faster (Llama-3-8B attn_output /
// ffn_down at 256 rows: 32 blocks)
constexpr int QG_MIN_GRID = 64;
// work-groups of the blocked GEMM, 0 = the shape goes to the GEMVs
static int q8gemm_grid(int M, int N, int K) {
  if (M < Q8_GEMM_MIN_M || N % 256 || K % Q8_TILE_K) return 0;
  const int grid = (N / 256) * ((M + QG_M - 1) / QG_M);
  return grid < QG_MIN_GRID ? 0 : grid;
}
static int launch_q8gemm(int epi, const MMArgs& a, int grid, hipStream_t s) {
  auto go = [&](auto q4c) {
    constexpr bool Q4 = decltype(q4c)::value;
    switch (epi) {
      case EPI_F32: q8gemm_kernel<EPI_F32, Q4><<<grid, 512, 0, s>>>(a); return 0;
      case EPI_RESID: q8gemm_kernel<EPI_RESID, Q4><<<grid, 512, 0, s>>>(a); return 0;
      case EPI_QKV: q8gemm_kernel<EPI_QKV, Q4><<<grid, 512, 0, s>>>(a); return 0;
      case EPI_SWIGLU: q8gemm_kernel<EPI_SWIGLU, Q4><<<grid, 512, 0, s>>>(a); return 0;
    }
    return -1;
  };
  return a.wq4 ? go(std::true_type{}) : go(std::false_type{});
}

// The kernel a shape reaches: quantise on load (one tile per group, or mq8_pers_ql_kernel), else the blocked
// GEMM, else the LDS-shared 17..32-row form, else mq8_kernel.  launch_mq8 dispatches on this and on nothing else.
Mq8Plan mq8_plan(int epi, int M, int N, int K, bool wq4, bool on_load, bool norm) {
  Mq8Plan p{};
  if (epi < EPI_F32 || epi > EPI_SWIGLU || M < 1 || K < Q8_TILE_K || K % Q8_TILE_K || N < TILE_N || N % TILE_N) return p;
  if (on_load) {  // quantise on load from a.xf (+ RMS_NORM when norm_w)
    if (!mq8_can_quantize_on_load(M, K, norm)) return p;
    p.ks = 8, p.rt = 1, p.nb = 1, p.grid_y = 1;
    if ((p.tpw = mq8_pers_ql_tpw(epi, wq4, M, N, K, norm)) > 0) {
      p.kind = MQ8_PERS_QL, p.qp = 2, p.qm = 1, p.bd = 1;
      return p;
    }
    p.kind = MQ8_QL, p.qp = mq8_ql_qp(K), p.qm = M == 1 ? 1 : M == 2 ? 2 : 4, p.bd = M == 1;
    return p;
  }
  if ((p.grid = q8gemm_grid(M, N, K)) > 0) {
    p.kind = MQ8_GEMM;
    return p;
  }
  if ((p.w = mq8_wide_w(epi, M, N, K)) > 0) {
    p.kind = wq4 ? MQ8_WSW : MQ8_WIDE;
    return p;
  }
  const Mq8Cfg c = mq8_gemv_cfg(epi, M, N / TILE_N);
  p.kind = MQ8_GEMV, p.ks = c.ks, p.rt = c.rt, p.nb = c.nb, p.bd = c.bd, p.grid_y = c.nb == 4 ? (M + 63) / 64 : 1;
  return p;
}

int launch_mq8(int epi, const MMArgs& a, hipStream_t s) {
  if (epi == EPI_SWIGLU && !a.actf && !a.act) return -1;
  const bool on_load = !a.xq;
  if (on_load ? (!a.xf || (a.norm_w && (!a.ssq || a.np * 16 != a.K))) : !a.xd) return -1;
  const Mq8Plan p = mq8_plan(epi, a.M, a.N, a.K, a.wq4 != 0, on_load, a.norm_w != nullptr);
  if (p.kind == MQ8_NONE) return -1;
  if (p.kind == MQ8_GEMM) return launch_q8gemm(epi, a, p.grid, s);
  if (p.kind == MQ8_WIDE || p.kind == MQ8_WSW) return launch_mq8_wide(epi, a, p.w, s);
  auto go = [&](auto q4c) {
    constexpr bool Q4 = decltype(q4c)::value;
    const bool ql = p.kind != MQ8_GEMV;
    switch (epi) {
      case EPI_F32: return ql ? launch_mq8_ql_epi<EPI_F32, Q4>(a, p, s) : launch_mq8_epi<EPI_F32, Q4>(a, p, s);
      case EPI_RESID: return ql ? launch_mq8_ql_epi<EPI_RESID, Q4>(a, p, s) : launch_mq8_epi<EPI_RESID, Q4>(a, p, s);
      case EPI_QKV: return ql ? launch_mq8_ql_epi<EPI_QKV, Q4>(a, p, s) : launch_mq8_epi<EPI_QKV, Q4>(a, p, s);
      case EPI_SWIGLU: return ql ? launch_mq8_ql_epi<EPI_SWIGLU, Q4>(a, p, s) : launch_mq8_epi<EPI_SWIGLU, Q4>(a, p, s);
    }
    return -1;
  };
  return a.wq4 ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace mx

namespace mx {

// HBM streaming probes (bench.py hbm_probe): what a plain streaming kernel reaches on this box, so
// the decode kernels' fractions of the 8 TB/s spec can also be read against a measured stream.
// Each work-group owns 256*U consecutive 16-B words per pass (lane i moves words i, i+256, ...:
// coalesced, U loads in flight per lane), grid-stride; NT = non-temporal loads (what the GEMVs
// use for their once-read weights).  The host sweeps (U, grid, NT) and keeps the best.
template <int U, bool NT>
__global__ __launch_bounds__(256) void copy_probe_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                         size_t n16) {
  const size_t stride = (size_t)gridDim.x * 256 * U;
  for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n16; i += stride) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(src + i + 256 * u) : src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(v[u], dst + i + 256 * u);
  }
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void read_probe_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ sink,
                                                         size_t n16) {
  const size_t stride = (size_t)gridDim.x * 256 * U;
  u32x4 x = {0u, 0u, 0u, 0u};
  for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n16; i += stride) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(src + i + 256 * u) : src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < U; ++u) x ^= v[u];
  }
  // sink written only when the fold hits a sentinel (never for the probe's fill): keeps the loads live
  if (x[0] == 0x9e3779b9u && x[1] == 0x7f4a7c15u) sink[(size_t)blockIdx.x * 256 + threadIdx.x] = x;
}

// Prefix sharing (kernels.h KvCopy): grid (chunks of 256 * U 16-byte words, layer x kv head x K|V, copy), lane i of
// a work-group moves words i, i + 256, ... of its chunk (coalesced, U loads in flight per lane), in the shape
// of copy_probe_kernel.  A region prefix is a whole number of 256-word rows (32 positions x 64 dims x 2 B = 4 KiB),
// so a chunk is cut at a row and every lane of a work-group takes the same branch.  Plain loads and stores: a
// source may feed several copies, and the destination's prefill attention reads the copy next.
template <int U>
__global__ __launch_bounds__(256) void kv_copy_kernel(_Float16* kc, _Float16* vc, const KvCopy* __restrict__ tab,
                                                      int n_head_kv, int head_dim, int ctx_stride, size_t slot_stride,
                                                      size_t layer_kv_stride) {
  const KvCopy c = tab[blockIdx.z];
  const int P = min((c.n_pos + 31) & ~31, ctx_stride);
  const size_t n16 = (size_t)P * head_dim / 8;
  const size_t b0 = (size_t)blockIdx.x * 256 * U;
  if (b0 >= n16) return;
  const int lh = blockIdx.y >> 1, layer = lh / n_head_kv, head = lh % n_head_kv;
  _Float16* base = ((blockIdx.y & 1) ? vc : kc) + (size_t)layer * layer_kv_stride + (size_t)head * ctx_stride * head_dim;
  const u32x4* src = reinterpret_cast<const u32x4*>(base + (size_t)c.src * slot_stride) + b0 + threadIdx.x;
  u32x4* dst = reinterpret_cast<u32x4*>(base + (size_t)c.dst * slot_stride) + b0 + threadIdx.x;
  if (b0 + 256 * U <= n16) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[256 * u];
#pragma unroll
    for (int u = 0; u < U; ++u) dst[256 * u] = v[u];
  } else {
    const int rows = (int)((n16 - b0) / 256);
    for (int u = 0; u < rows; ++u) dst[256 * u] = src[256 * u];
  }
}

size_t kv_copy_bytes(const KvCopy* tab, int n, int n_layer, int n_head_kv, int head_dim, int ctx_stride) {
  size_t b = 0;
  for (int i = 0; i < n; i++)
    b += (size_t)std::min((tab[i].n_pos + 31) & ~31, ctx_stride) * head_dim * 2 * n_head_kv * n_layer * 2;
  return b;
}

int launch_kv_copy(_Float16* kc, _Float16* vc, const KvCopy* tab, const KvCopy* tab_dev, int n, int n_layer,
                   int n_slots, int n_head_kv, int head_dim, int n_ctx, int ctx_stride, size_t slot_stride,
                   size_t layer_kv_stride, hipStream_t s) {
  if (!kc || !vc || !tab || !tab_dev || n < 1 || n > 65535 || n_layer < 1 || n_slots < 1 || n_head_kv < 1 ||
      (head_dim != 64 && head_dim != 128) || n_ctx < 1 || ctx_stride < n_ctx || ctx_stride % 32 ||
      (size_t)n_layer * n_head_kv * 2 > 65535)
    return -1;
  std::vector<char> role(n_slots, 0);  // 1 source, 2 destination
  int max_pos = 0;
  for (int i = 0; i < n; i++) {
    const KvCopy& c = tab[i];
    if (c.src < 0 || c.src >= n_slots || c.dst < 0 || c.dst >= n_slots || c.src == c.dst) return -1;
    if (c.n_pos < 1 || c.n_pos > n_ctx) return -1;
    if (role[c.dst] || role[c.src] == 2) return -1;
    role[c.src] = 1;
    role[c.dst] = 2;
    max_pos = std::max(max_pos, c.n_pos);
  }
  constexpr int U = 4;
  const size_t n16 = (size_t)std::min((max_pos + 31) & ~31, ctx_stride) * head_dim / 8;
  const dim3 grid((unsigned)((n16 + 256 * U - 1) / (256 * U)), (unsigned)(n_layer * n_head_kv * 2), (unsigned)n);
  kv_copy_kernel<U><<<grid, 256, 0, s>>>(kc, vc, tab_dev, n_head_kv, head_dim, ctx_stride, slot_stride, layer_kv_stride);
  return 0;
}

template <int U, bool NT>
static void probe_launch(bool read_only, const uint4* src, uint4* dst, size_t n16, int grid, hipStream_t s) {
  const u32x4* sv = reinterpret_cast<const u32x4*>(src);
  u32x4* dv = reinterpret_cast<u32x4*>(dst);
  if (read_only) read_probe_kernel<U, NT><<<grid, 256, 0, s>>>(sv, dv, n16);
  else copy_probe_kernel<U, NT><<<grid, 256, 0, s>>>(sv, dv, n16);
}

int probe_variants() { return 3 * 2 * 3; }

// variant v: U in {4, 8, 16} x NT in {0, 1} x grid in {1024, 2048, 4096}; n16 % (256 * 16) == 0
int launch_probe(int v, bool read_only, const uint4* src, uint4* dst, size_t n16, hipStream_t s, char* desc,
                 int desc_len) {
  if (v < 0 || v >= probe_variants() || n16 % (256 * 16)) return -1;
  const int grids[3] = {1024, 2048, 4096};
  const int grid = grids[v % 3], nt = (v / 3) % 2, ui = v / 6;
  const int U = 4 << ui;
  if (desc) snprintf(desc, desc_len, "%d work-groups x 256 lanes, %d x 16-B loads in flight per lane%s", grid, U,
                     nt ? ", non-temporal" : "");
  switch (ui * 2 + nt) {
    case 0: probe_launch<4, false>(read_only, src, dst, n16, grid, s); break;
    case 1: probe_launch<4, true>(read_only, src, dst, n16, grid, s); break;
    case 2: probe_launch<8, false>(read_only, src, dst, n16, grid, s); break;
    case 3: probe_launch<8, true>(read_only, src, dst, n16, grid, s); break;
    case 4: probe_launch<16, false>(read_only, src, dst, n16, grid, s); break;
    case 5: probe_launch<16, true>(read_only, src, dst, n16, grid, s); break;
  }
  return 0;
}

}  // namespace mx
