// attn_split.hip -- long-context decode attention: a row's keys split over work-groups.
//
// attn_decode_kernel (kernels.hip) runs one work-group per (kv head, row): at one row and context 16384 eight
// work-groups read 64 MiB of K/V per Llama-3-8B layer.  Here a row whose context exceeds ATTN_SPLIT_T is cut into
// attn_nseg(ctx) segments of attn_seg_len(ctx) positions -- functions of the row's context alone, never of the row
// count, of n_ctx or of what shares the launch -- and work-group (kv head, row, segment) runs attn_decode_body's
// chunk stream over its segment: the same f16 MFMA tiles, log2-domain online softmax, partial-last-chunk masking
// and in-group wave merge.  A one-segment row (ctx <= ATTN_SPLIT_T) walks the chunks in attn_decode_body's order
// and stores acc / L from the same expressions, so its bits equal launch_attention's; a longer row stores
// its unnormalised partial (m, l, acc[D] per head) to the workspace and attn_merge_kernel -- the next launch, a
// kernel boundary being the cheapest grid-wide barrier on this chip -- folds the segments in
// segment order.  No atomics, no arrival counters: a long row's bits are a function of the row alone.
#include "device_common.h"
#include "attn_body.h"  // LOG2E

namespace mx {

namespace {

// workspace record of one (row, q head, segment): [m, l, -, -, acc[D]] f32 (acc 16-byte aligned)
__host__ __device__ constexpr int split_rec(int D) { return D + 4; }

// One (kv head, row, segment) by the NW waves of the calling work-group: wave w takes chunks first + w,
// first + w + NW, ... of the segment.  The chunk stream is attn_decode_body's non-FIN one, statement by statement.
template <int D, int G, int NW>
__device__ __forceinline__ void attn_split_body(const AttnArgs& a, float* __restrict__ ws, int kvh, int c, int seg) {
  constexpr int CH = ATTN_CHUNK;
  constexpr int QK = D / 32;  // k-steps of QK^T
  constexpr int DT = D / 16;  // d tiles of P.V
  const int t_ = threadIdx.x;
  const int lane = t_ & 63, w = __builtin_amdgcn_readfirstlane(t_ >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int pos = a.pos[c];
  const int slot = a.slot[c];
  const int ctx = min(pos + 1, a.n_ctx);
  const int nseg = attn_nseg(ctx);
  if (seg >= nseg) return;  // uniform over the work-group, before any barrier
  // chunks [first, (lim + CH - 1) / CH): the whole row, or this segment of it (segments are chunk multiples, so
  // only the row's last chunk is ever partial and the masks below compare with ctx as attn_decode_body's do)
  const int slen = attn_seg_len(ctx);
  const int first = nseg == 1 ? 0 : seg * (slen / CH);
  const int lim = nseg == 1 ? ctx : min(ctx, (seg + 1) * slen);

  __shared__ __attribute__((aligned(16))) _Float16 Ps[NW][16][CH + 8];
  __shared__ float Om[NW][G][D];
  __shared__ float Mm[NW][G], Ll[NW][G];

  const _Float16* Kb = a.kc + (size_t)slot * a.slot_stride + (size_t)kvh * a.ctx_stride * D;
  const _Float16* Vb = a.vc + (size_t)slot * a.slot_stride + (size_t)kvh * a.ctx_stride * D;
  struct KV {
    f16x8 k[2][QK], v[DT];
  };
  auto load = [&](KV& f, int ch) {
    const int p0 = ch * CH;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kk = 0; kk < QK; ++kk)
        f.k[t][kk] = *reinterpret_cast<const f16x8*>(Kb + (((size_t)(p0 / 16 + t) * QK + kk) * 64 + lane) * 8);
#pragma unroll
    for (int t = 0; t < DT; ++t)
      f.v[t] = *reinterpret_cast<const f16x8*>(Vb + (((size_t)(p0 / 32) * DT + t) * 64 + lane) * 8);
  };
  // the wave's first chunk is loaded before q: its latency overlaps the q load
  KV A;
  if ((first + w) * CH < lim) load(A, first + w);

  // A operand of QK^T: rows = heads of the group (rows >= G are zero)
  f16x8 qa[QK];
  {
    const float* qrow = a.q + (size_t)c * a.n_head * D + (size_t)(kvh * G + (r16 < G ? r16 : 0)) * D;
    const bool live = r16 < G;
#pragma unroll
    for (int kk = 0; kk < QK; ++kk) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qa[kk][j] = live ? (_Float16)v0[j] : (_Float16)0.f;
        qa[kk][4 + j] = live ? (_Float16)v1[j] : (_Float16)0.f;
      }
    }
  }

  float m_i[4], l_i[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_i[i] = -INFINITY;
    l_i[i] = 0.f;
  }
  f32x4 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](KV& f, int ch) {
    const int p0 = ch * CH;
    const int pb = p0 + 8 * q4;  // first position of this lane's P.V B fragment
    // S[head][pos] for two 16-position tiles
    f32x4 sc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < QK; ++kk) sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[kk], f.k[t][kk], sc[t], 0, 0, 0);
    }
    // online softmax in the log2 domain (scores pre-multiplied by log2 e, v_exp_f32 = 2^x):
    // C layout rows = heads 4*q4+i, cols = positions (lane r16)
    float e[2][4];
    const float sl2 = a.scale * LOG2E;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v0 = (p0 + r16 < ctx) ? sc[0][i] * sl2 : -INFINITY;
      const float v1 = (p0 + 16 + r16 < ctx) ? sc[1][i] * sl2 : -INFINITY;
      const float m_new = fmaxf(m_i[i], row16_max(fmaxf(v0, v1)));
      const float alpha = __builtin_amdgcn_exp2f(m_i[i] - m_new);  // 0 on the first chunk (m_i = -inf)
      e[0][i] = __builtin_amdgcn_exp2f(v0 - m_new);
      e[1][i] = __builtin_amdgcn_exp2f(v1 - m_new);
      l_i[i] = l_i[i] * alpha + row16_sum(e[0][i] + e[1][i]);
      m_i[i] = m_new;
#pragma unroll
      for (int t = 0; t < DT; ++t) o[t][i] *= alpha;
    }
    // P (f16) -> LDS as [head][pos], re-read as the A operand of P.V
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) Ps[w][4 * q4 + i][16 * t + r16] = (4 * q4 + i < G) ? (_Float16)e[t][i] : (_Float16)0.f;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes landed
    __builtin_amdgcn_wave_barrier();
    const f16x8 pa = *reinterpret_cast<const f16x8*>(&Ps[w][r16][8 * q4]);
    if (p0 + CH > ctx) {  // the partial last chunk: never-written positions must not reach P.V
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[t][j] = (pb + j < ctx) ? f.v[t][j] : (_Float16)0.f;
    }
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, f.v[t], o[t], 0, 0, 0);
    __builtin_amdgcn_wave_barrier();  // Ps[w] is rewritten next chunk only after every lane read it
  };
  for (int ch = first + w; ch * CH < lim; ch += NW) {
    if (ch != first + w) load(A, ch);
    compute(A, ch);
  }

  // merge the NW wave partials (a wave without a chunk in a short last segment holds m = -inf, l = 0)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h = 4 * q4 + i;
    if (h < G) {
#pragma unroll
      for (int t = 0; t < DT; ++t) Om[w][h][t * 16 + r16] = o[t][i];
      if (r16 == 0) {
        Mm[w][h] = m_i[i];
        Ll[w][h] = l_i[i];
      }
    }
  }
  __syncthreads();
  for (int idx = t_; idx < G * D; idx += 64 * NW) {
    const int h = idx / D, d = idx % D;
    float M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) M = fmaxf(M, Mm[ww][h]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      const float f = (Mm[ww][h] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(Mm[ww][h] - M);
      L += f * Ll[ww][h];
      acc += f * Om[ww][h][d];
    }
    if (nseg == 1) {  // attn_decode_body's store
      if (a.outf) {
        a.outf[(size_t)c * a.ldo + (kvh * G + h) * D + d] = acc / L;
      } else {
        a.out[(size_t)c * a.ldo + (kvh * G + h) * D + d] = (uint16_t)f2bf(acc / L);
      }
    } else {  // the segment's unnormalised partial, relative to its own max M
      float* rec = ws + (((size_t)c * a.n_head + (kvh * G + h)) * ATTN_NSEG_MAX + seg) * split_rec(D);
      rec[4 + d] = acc;
      if (d == 0) {
        rec[0] = M;
        rec[1] = L;
      }
    }
  }
}

template <int D, int G, int NW>
__global__ __launch_bounds__(64 * NW) void attn_split_kernel(AttnArgs a, float* ws) {
  attn_split_body<D, G, NW>(a, ws, blockIdx.x, blockIdx.y, blockIdx.z);
}

// One work-group of 256 threads per (kv head, row): a row of one segment was stored by
// attn_split_kernel and is left alone; otherwise thread (h, d) folds the row's segments in segment order --
// max over the segments, then L and acc as two running sums over f_s = 2^(m_s - M) -- and stores acc / L as
// attn_decode_body does.  Every segment of a split row holds at least one position, so every m_s is finite.
template <int D, int G>
__global__ __launch_bounds__(256) void attn_merge_kernel(AttnArgs a, const float* __restrict__ ws) {
  const int kvh = blockIdx.x, c = blockIdx.y;
  const int ctx = min(a.pos[c] + 1, a.n_ctx);
  const int nseg = attn_nseg(ctx);
  if (nseg == 1) return;
  for (int idx = threadIdx.x; idx < G * D; idx += 256) {
    const int h = idx / D, d = idx % D;
    const float* rec = ws + ((size_t)c * a.n_head + (kvh * G + h)) * ATTN_NSEG_MAX * split_rec(D);
    float M = -INFINITY;
#pragma unroll 8
    for (int sg = 0; sg < nseg; ++sg) M = fmaxf(M, rec[(size_t)sg * split_rec(D)]);
    float L = 0.f, acc = 0.f;
#pragma unroll 8
    for (int sg = 0; sg < nseg; ++sg) {
      const float* r = rec + (size_t)sg * split_rec(D);
      const float f = __builtin_amdgcn_exp2f(r[0] - M);
      L += f * r[1];
      acc += f * r[4 + d];
    }
    if (a.outf) {
      a.outf[(size_t)c * a.ldo + (kvh * G + h) * D + d] = acc / L;
    } else {
      a.out[(size_t)c * a.ldo + (kvh * G + h) * D + d] = (uint16_t)f2bf(acc / L);
    }
  }
}

template <int D, int G, int NW>
void launch_split_g(const AttnArgs& a, float* ws, hipStream_t s) {
  attn_split_kernel<D, G, NW><<<dim3(a.n_head_kv, a.M, ATTN_NSEG_MAX), 64 * NW, 0, s>>>(a, ws);
  attn_merge_kernel<D, G><<<dim3(a.n_head_kv, a.M), 256, 0, s>>>(a, ws);
}

// the wave count of launch_attn_d's non-FIN launches at <= 64 rows: 4 for MHA models (or MX_ATTN_NW4), else 8
template <int D>
int launch_split_d(const AttnArgs& a, float* ws, hipStream_t s) {
  static const bool nw4 = getenv("MX_ATTN_NW4") != nullptr;
  const int G = a.n_head / a.n_head_kv;
  if (G == 1 || nw4) {
    switch (G) {
      case 1: launch_split_g<D, 1, 4>(a, ws, s); return 0;
      case 2: launch_split_g<D, 2, 4>(a, ws, s); return 0;
      case 4: launch_split_g<D, 4, 4>(a, ws, s); return 0;
      case 5: launch_split_g<D, 5, 4>(a, ws, s); return 0;
      case 6: launch_split_g<D, 6, 4>(a, ws, s); return 0;
      case 7: launch_split_g<D, 7, 4>(a, ws, s); return 0;
      case 8: launch_split_g<D, 8, 4>(a, ws, s); return 0;
    }
    return -1;
  }
  switch (G) {
    case 2: launch_split_g<D, 2, 8>(a, ws, s); return 0;
    case 4: launch_split_g<D, 4, 8>(a, ws, s); return 0;
    case 5: launch_split_g<D, 5, 8>(a, ws, s); return 0;
    case 6: launch_split_g<D, 6, 8>(a, ws, s); return 0;
    case 7: launch_split_g<D, 7, 8>(a, ws, s); return 0;
    case 8: launch_split_g<D, 8, 8>(a, ws, s); return 0;
  }
  return -1;
}

}  // namespace

size_t attn_split_ws_floats(int M, int n_head, int head_dim) {
  return (size_t)M * n_head * ATTN_NSEG_MAX * split_rec(head_dim);
}

int launch_attention_merge(const AttnArgs& a, const float* ws, hipStream_t s) {
  if (!ws || a.M < 1 || a.M > MAX_ROWS || a.n_head_kv < 1 || a.n_head % a.n_head_kv) return -1;
  const int G = a.n_head / a.n_head_kv;
  const dim3 grid(a.n_head_kv, a.M);
#define MX_MERGE(D_)                                                                    \
  switch (G) {                                                                          \
    case 1: attn_merge_kernel<D_, 1><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 2: attn_merge_kernel<D_, 2><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 4: attn_merge_kernel<D_, 4><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 5: attn_merge_kernel<D_, 5><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 6: attn_merge_kernel<D_, 6><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 7: attn_merge_kernel<D_, 7><<<grid, 256, 0, s>>>(a, ws); return 0;             \
    case 8: attn_merge_kernel<D_, 8><<<grid, 256, 0, s>>>(a, ws); return 0;             \
  }
  if (a.head_dim == 64) { MX_MERGE(64) }
  if (a.head_dim == 128) { MX_MERGE(128) }
#undef MX_MERGE
  return -1;
}

int launch_attention_split(const AttnArgs& a, float* ws, hipStream_t s) {
  if (a.slabs || !a.q || !ws || a.M < 1 || a.M > MAX_ROWS || a.n_head_kv < 1 || a.n_head % a.n_head_kv) return -1;
  if (a.head_dim == 64) return launch_split_d<64>(a, ws, s);
  if (a.head_dim == 128) return launch_split_d<128>(a, ws, s);
  return -1;
}

}  // namespace mx
