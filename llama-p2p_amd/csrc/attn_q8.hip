// attn_q8.hip -- attention over a Q8_0 KV cache (mx_opts.kv_type = 8).
//
// The QKV writers keep storing f16 tiles, into a one-layer scratch cache; kv_quant_kernel turns the positions a
// forward stored into Q8_0 blocks of the layer's cache (34 bytes where f16 holds 64), and the attention kernels
// read only those: QK^T as one v_mfma_i32_16x16x32_i8 per block on a q quantised to Q8_0 in registers (ggml's
// vec_dot_q8_0_q8_0, what its flash attention does for a Q8_0 K), P.V as f16 MFMAs on f16(p d_v) and V's integers.
// Decode rows, long rows (a segment per work-group under §20's rule, merged by attn_merge_kernel) and prefill
// blocks share one chunk body (attn_q8_body.h).
#include "device_common.h"
#include "attn_q8_body.h"

namespace mx {

namespace {

// grid (kv head, row), D threads: 16 lanes (one DPP row) per block of 32 head-dim elements, two elements each;
// threads [0, D/2) take K's blocks, [D/2, D) V's.  A row at pos == n_ctx stored nothing and quantises nothing.
// ggml's quantize_row_q8_0_ref on the f16 values widened to f32.  Rows that repeat a (slot, pos) -- a prefill
// block's padding -- store the same bytes.
template <int D>
__global__ __launch_bounds__(D) void kv_quant_kernel(AttnArgs a) {
  constexpr int QK = D / 32;
  const int kvh = blockIdx.x, c = blockIdx.y;
  const int pos = a.pos[c], slot = a.slot[c];
  if (pos < 0 || pos >= a.n_ctx) return;  // uniform over the work-group
  const int t = threadIdx.x;
  const bool isv = t >= D / 2;
  const int u = isv ? t - D / 2 : t;
  const int b = u >> 4, d0 = 32 * b + 2 * (u & 15);
  const size_t so = (size_t)slot * a.slot_stride + (size_t)kvh * a.ctx_stride * D;
  float x0, x1;
  if (isv) {
    x0 = (float)a.vc[so + kv_v_off(pos, d0, D)];
    x1 = (float)a.vc[so + kv_v_off(pos, d0 + 1, D)];
  } else {
    const f16x2 k2 = *reinterpret_cast<const f16x2*>(a.kc + so + kv_k_off(pos, d0, D));
    x0 = (float)k2[0];
    x1 = (float)k2[1];
  }
  const float amax = row16_max(fmaxf(fabsf(x0), fabsf(x1)));
  float d, id;
  q8_block_scale(amax, d, id);
  const uint8_t q0 = (uint8_t)(int8_t)roundf(x0 * id), q1 = (uint8_t)(int8_t)roundf(x1 * id);
  const size_t reg = kvq_region_bytes(a.ctx_stride, D);
  uint8_t* base = (isv ? a.vq8 : a.kq8) + ((size_t)slot * a.n_head_kv + kvh) * reg;
  _Float16* sp = reinterpret_cast<_Float16*>(base + kvq_plane(a.ctx_stride, D));
  if (isv) {
    base[kvq_v_off(pos, d0, D)] = q0;
    base[kvq_v_off(pos, d0 + 1, D)] = q1;
    if ((u & 15) == 0) sp[kvq_vs_off(pos, b, D)] = (_Float16)d;
  } else {
    *reinterpret_cast<uint16_t*>(base + kvq_k_off(pos, d0, D)) = (uint16_t)(q0 | (q1 << 8));
    if ((u & 15) == 0) sp[kvq_ks_off(pos, b, D)] = (_Float16)d;
  }
}

// workspace record of one (row, q head, segment), as attn_split.hip writes it for attn_merge_kernel:
// [m, l, -, -, acc[D]] f32
__host__ __device__ constexpr int split_rec(int D) { return D + 4; }

// One work-group of NW waves per (kv head, row, segment); the G query heads of the group are the MFMA rows.  Wave w
// takes chunks first + w, first + w + NW, ... of its segment (the whole row when ws is null or the row is short) and
// has its first chunk's loads in flight before q is read.
template <int D, int G, int NW>
__global__ __launch_bounds__(64 * NW) void attn_q8_decode_kernel(AttnArgs a, float* __restrict__ ws) {
  constexpr int CH = ATTN_CHUNK, QK = D / 32, DT = D / 16;
  const int kvh = blockIdx.x, c = blockIdx.y, seg = blockIdx.z;
  const int t_ = threadIdx.x;
  const int lane = t_ & 63, w = __builtin_amdgcn_readfirstlane(t_ >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int pos = a.pos[c], slot = a.slot[c];
  const int ctx = min(pos + 1, a.n_ctx);
  const int nseg = ws ? attn_nseg(ctx) : 1;
  if (seg >= nseg) return;  // uniform over the work-group, before any barrier
  const int slen = attn_seg_len(ctx);
  const int first = nseg == 1 ? 0 : seg * (slen / CH);
  const int lim = nseg == 1 ? ctx : min(ctx, (seg + 1) * slen);

  __shared__ __attribute__((aligned(16))) float Ps[NW][16][KVQ_PS];
  __shared__ float Qd[NW][16][QK];
  __shared__ float Om[NW][G][D];
  __shared__ float Mm[NW][G], Ll[NW][G];

  const KvqRegion<D> R(a, slot, kvh);
  KvqFrag<D> A;
  if ((first + w) * CH < lim) R.load(A, (first + w) * CH, lane);

  long qa[QK];
  float dq[4][QK];
  q8_quantize_q<D>(a.q + (size_t)c * a.n_head * D + (size_t)(kvh * G + (r16 < G ? r16 : 0)) * D, r16 < G, lane, Qd[w], qa,
                   dq);

  float m_i[4], l_i[4];
  int qlast[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_i[i] = -INFINITY;
    l_i[i] = 0.f;
    qlast[i] = ctx - 1;
  }
  f32x4 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * LOG2E;
  for (int ch = first + w; ch * CH < lim; ch += NW) {
    if (ch != first + w) R.load(A, ch * CH, lane);
    q8_chunk<D>(A, qa, dq, ch * CH, qlast, ctx - 1, G, sl2, lane, Ps[w], m_i, l_i, o);
  }

  // merge the NW wave partials (a wave without a chunk holds m = -inf, l = 0)
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
    if (nseg == 1) {
      if (a.outf) a.outf[(size_t)c * a.ldo + (kvh * G + h) * D + d] = acc / L;
      else a.out[(size_t)c * a.ldo + (kvh * G + h) * D + d] = (uint16_t)f2bf(acc / L);
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

// Prefill: work-group (kv head, block of 16 consecutive positions of one sequence), one wave per query head of the
// group; the 16 queries are the MFMA rows, keys are visited in order (attn_prefill_kernel's form).  A block's rows
// may end in copies of its last row; rows past M re-read row M - 1 and are not stored.
template <int D, int G>
__global__ __launch_bounds__(64 * G) void attn_q8_prefill_kernel(AttnArgs a) {
  constexpr int CH = ATTN_CHUNK, QK = D / 32, DT = D / 16;
  const int kvh = blockIdx.x, r0 = blockIdx.y * 16;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int slot = a.slot[r0];
  const int hq = kvh * G + w;
  __shared__ __attribute__((aligned(16))) float Ps[G][16][KVQ_PS];
  __shared__ float Qd[G][16][QK];

  const int last = min(a.pos[min(r0 + 15, a.M - 1)], a.n_ctx - 1);  // newest key any query of the block sees
  const KvqRegion<D> R(a, slot, kvh);
  KvqFrag<D> A;
  R.load(A, 0, lane);
  int qlast[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qlast[i] = min(a.pos[min(r0 + 4 * q4 + i, a.M - 1)], a.n_ctx - 1);
  long qa[QK];
  float dq[4][QK];
  q8_quantize_q<D>(a.q + (size_t)min(r0 + r16, a.M - 1) * a.n_head * D + (size_t)hq * D, true, lane, Qd[w], qa, dq);

  float m_i[4], l_i[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_i[i] = -INFINITY;
    l_i[i] = 0.f;
  }
  f32x4 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * LOG2E;
  for (int p0 = 0; p0 <= last; p0 += CH) {
    if (p0) R.load(A, p0, lane);
    q8_chunk<D>(A, qa, dq, p0, qlast, last, 16, sl2, lane, Ps[w], m_i, l_i, o);
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

template <int D, int G, int NW>
void launch_q8_g(const AttnArgs& a, float* ws, hipStream_t s) {
  attn_q8_decode_kernel<D, G, NW><<<dim3(a.n_head_kv, a.M, ws ? ATTN_NSEG_MAX : 1), 64 * NW, 0, s>>>(a, ws);
}

// launch_attn_d's wave counts: 4 for MHA models and for >= 128 rows, else 8
template <int D>
int launch_q8_d(const AttnArgs& a, float* ws, hipStream_t s) {
  const int G = a.n_head / a.n_head_kv;
  if (G == 1 || a.M >= 128) {
    switch (G) {
      case 1: launch_q8_g<D, 1, 4>(a, ws, s); return 0;
      case 2: launch_q8_g<D, 2, 4>(a, ws, s); return 0;
      case 4: launch_q8_g<D, 4, 4>(a, ws, s); return 0;
      case 5: launch_q8_g<D, 5, 4>(a, ws, s); return 0;
      case 6: launch_q8_g<D, 6, 4>(a, ws, s); return 0;
      case 7: launch_q8_g<D, 7, 4>(a, ws, s); return 0;
      case 8: launch_q8_g<D, 8, 4>(a, ws, s); return 0;
    }
    return -1;
  }
  switch (G) {
    case 2: launch_q8_g<D, 2, 8>(a, ws, s); return 0;
    case 4: launch_q8_g<D, 4, 8>(a, ws, s); return 0;
    case 5: launch_q8_g<D, 5, 8>(a, ws, s); return 0;
    case 6: launch_q8_g<D, 6, 8>(a, ws, s); return 0;
    case 7: launch_q8_g<D, 7, 8>(a, ws, s); return 0;
    case 8: launch_q8_g<D, 8, 8>(a, ws, s); return 0;
  }
  return -1;
}

template <int D>
int launch_q8_prefill_d(const AttnArgs& a, hipStream_t s) {
  const dim3 grid(a.n_head_kv, (a.M + 15) / 16);
  switch (a.n_head / a.n_head_kv) {
    case 1: attn_q8_prefill_kernel<D, 1><<<grid, 64, 0, s>>>(a); return 0;
    case 2: attn_q8_prefill_kernel<D, 2><<<grid, 128, 0, s>>>(a); return 0;
    case 4: attn_q8_prefill_kernel<D, 4><<<grid, 256, 0, s>>>(a); return 0;
    case 5: attn_q8_prefill_kernel<D, 5><<<grid, 320, 0, s>>>(a); return 0;
    case 6: attn_q8_prefill_kernel<D, 6><<<grid, 384, 0, s>>>(a); return 0;
    case 7: attn_q8_prefill_kernel<D, 7><<<grid, 448, 0, s>>>(a); return 0;
    case 8: attn_q8_prefill_kernel<D, 8><<<grid, 512, 0, s>>>(a); return 0;
  }
  return -1;
}

bool q8_args_ok(const AttnArgs& a) {
  return a.kq8 && a.vq8 && a.pos && a.slot && a.M >= 1 && a.n_head_kv >= 1 && a.n_head % a.n_head_kv == 0 &&
         (a.head_dim == 64 || a.head_dim == 128) && a.ctx_stride % KV_POS_ALIGN == 0 && a.n_ctx <= a.ctx_stride;
}

}  // namespace

int launch_kv_quant(const AttnArgs& a, hipStream_t s) {
  if (!q8_args_ok(a) || !a.kc || !a.vc) return -1;
  const dim3 grid(a.n_head_kv, a.M);
  if (a.head_dim == 64) kv_quant_kernel<64><<<grid, 64, 0, s>>>(a);
  else kv_quant_kernel<128><<<grid, 128, 0, s>>>(a);
  return 0;
}

int launch_attention_q8(const AttnArgs& a, float* ws, hipStream_t s) {
  if (!q8_args_ok(a) || a.slabs || !a.q || (ws && a.M > MAX_ROWS)) return -1;
  if (a.head_dim == 64 ? launch_q8_d<64>(a, ws, s) : launch_q8_d<128>(a, ws, s)) return -1;
  return ws ? launch_attention_merge(a, ws, s) : 0;
}

int launch_attention_q8_prefill(const AttnArgs& a, hipStream_t s) {
  if (!q8_args_ok(a) || a.slabs || !a.q) return -1;
  return a.head_dim == 64 ? launch_q8_prefill_d<64>(a, s) : launch_q8_prefill_d<128>(a, s);
}

}  // namespace mx
