// attn_q8_body.h -- the pieces the Q8_0-cache attention kernels share (attn_q8.hip): the cache
// layout, the chunk loads, q's quantisation and one 32-position chunk of int8 QK^T, online softmax and f16 P.V.
#pragma once
#include "attn_body.h"  // LOG2E

namespace mx {

// Q8_0 KV cache.  Each (slot, kv head) region holds ctx_stride positions of K (and as many of V) as one Q8_0
// block per position and 32 consecutive head-dim elements: an int8 plane of ctx_stride * D bytes in the lane
// order of the MFMA operand that reads it, then the plane of the f16 block scales (a load never straddles both).
//   K int8: tile (pos/16, d/64) = 16 positions x 2 blocks, 1 KiB, lane = pos%16 + 16*((d%32)/8) holds 16 bytes:
//           d%8 of block 2j, then d%8 of block 2j+1 -- each half is the B operand of one v_mfma_i32_16x16x32_i8
//           (k = the block's 32 dims, n = positions)
//   K scales: [pos][D/32] f16 (the lane that owns score column pos reads its D/32 scales in one load)
//   V int8: tile (pos/32, d/32) = 32 positions x 1 block, 1 KiB, lane = d%16 + 16*((pos%32)/8) holds 16 bytes:
//           pos%8 of dim d%16, then pos%8 of dim 16 + d%16 -- each half, widened to f16, is the B operand of one
//           v_mfma_f32_16x16x32_f16 of P.V (k = positions, n = dims)
//   V scales: [pos/8][D/32][8] f16 (the 8 positions of a lane's A operand, per block, in one 16-byte load)
__host__ __device__ inline size_t kvq_plane(int ctx_stride, int D) { return (size_t)ctx_stride * D; }
__device__ __forceinline__ size_t kvq_k_off(int pos, int d, int D) {
  return ((size_t)(pos >> 4) * (D >> 6) + (d >> 6)) * 1024 + ((pos & 15) + 16 * ((d & 31) >> 3)) * 16 + ((d >> 5) & 1) * 8 +
         (d & 7);
}
__device__ __forceinline__ size_t kvq_v_off(int pos, int d, int D) {
  return ((size_t)(pos >> 5) * (D >> 5) + (d >> 5)) * 1024 + ((d & 15) + 16 * ((pos & 31) >> 3)) * 16 + ((d >> 4) & 1) * 8 +
         (pos & 7);
}
__device__ __forceinline__ size_t kvq_ks_off(int pos, int b, int D) { return (size_t)pos * (D >> 5) + b; }  // f16 index
__device__ __forceinline__ size_t kvq_vs_off(int pos, int b, int D) {
  return ((size_t)(pos >> 3) * (D >> 5) + b) * 8 + (pos & 7);
}

template <int N>
struct F16Vec;
template <>
struct F16Vec<2> { typedef f16x2 type; };
template <>
struct F16Vec<4> { typedef f16x4 type; };

// one 32-position chunk of a (slot, kv head) region in registers
template <int D>
struct KvqFrag {
  u32x4 k[2][D / 64], v[D / 32];
  typename F16Vec<D / 32>::type kd[2];  // this lane's score columns p0 + r16 and p0 + 16 + r16
  f16x8 vd[D / 32];                     // positions p0 + 8*q4 .. + 8 of every block
};

template <int D>
struct KvqRegion {
  const uint8_t *kq, *vq;
  const _Float16 *ks, *vs;
  __device__ __forceinline__ KvqRegion(const AttnArgs& a, int slot, int kvh) {
    const size_t reg = kvq_region_bytes(a.ctx_stride, D);
    const size_t o = ((size_t)slot * a.n_head_kv + kvh) * reg;
    kq = a.kq8 + o;
    vq = a.vq8 + o;
    ks = reinterpret_cast<const _Float16*>(kq + kvq_plane(a.ctx_stride, D));
    vs = reinterpret_cast<const _Float16*>(vq + kvq_plane(a.ctx_stride, D));
  }
  // every wave-level load below is one contiguous run (1 KiB tiles; 32 * D/32 scales)
  __device__ __forceinline__ void load(KvqFrag<D>& f, int p0, int lane) const {
    constexpr int QK = D / 32;
    const int r16 = lane & 15, q4 = lane >> 4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int j = 0; j < D / 64; ++j)
        f.k[t][j] = *reinterpret_cast<const u32x4*>(kq + ((size_t)(p0 / 16 + t) * (D / 64) + j) * 1024 + lane * 16);
      f.kd[t] = *reinterpret_cast<const typename F16Vec<QK>::type*>(ks + kvq_ks_off(p0 + 16 * t + r16, 0, D));
    }
#pragma unroll
    for (int b = 0; b < QK; ++b) {
      f.v[b] = *reinterpret_cast<const u32x4*>(vq + ((size_t)(p0 / 32) * QK + b) * 1024 + lane * 16);
      f.vd[b] = *reinterpret_cast<const f16x8*>(vs + kvq_vs_off(p0 + 8 * q4, b, D));
    }
  }
};

// ggml's quantize_row_q8_0_ref of one block, the part every lane of the block shares: d = amax / 127 in f32,
// id = d ? 1/d : 0 (q = roundf(x * id) is the caller's, d is stored or used as f16)
__device__ __forceinline__ void q8_block_scale(float amax, float& d, float& id) {
  d = amax / 127.0f;
  id = d != 0.f ? 1.0f / d : 0.0f;
}

// 8 int8 (two words, byte j = element j) -> f16x8, exact: 0x6400 | (x ^ 0x80) is the f16 1024 + (x + 128), and
// 1152 comes off again in packed f16 (every value involved is an integer below 2048)
__device__ __forceinline__ f16x8 i8x8_to_f16(uint32_t w0, uint32_t w1) {
  constexpr uint32_t C = 0x64646464u;
  const uint32_t x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
  u32x4 h;
  h[0] = __builtin_amdgcn_perm(C, x0, 0x04010400u);
  h[1] = __builtin_amdgcn_perm(C, x0, 0x04030402u);
  h[2] = __builtin_amdgcn_perm(C, x1, 0x04010400u);
  h[3] = __builtin_amdgcn_perm(C, x1, 0x04030402u);
  const f16x8 bias = {1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152};
  return __builtin_bit_cast(f16x8, h) - bias;
}

// The A operand of the int8 QK^T from an f32 q row: lane (r16, q4) holds elements 8*q4 .. +8 of every block of the
// row `qrow` of MFMA row r16; the row is quantised to Q8_0 per block as ggml's q_to_vec_dot does for a Q8_0 K (amax
// over the four lanes r16, r16 + 16, + 32, + 48 that share a block).  A dead row (live false) gives zeros.  The
// f16-rounded block scales go through qd ([16][D/32] floats of this wave's LDS) into the C layout: dq[i][kk] is the
// scale of MFMA row 4*q4 + i.
template <int D>
__device__ __forceinline__ void q8_quantize_q(const float* qrow, bool live, int lane, float (*qd)[D / 32],
                                              long (&qa)[D / 32], float (&dq)[4][D / 32]) {
  constexpr int QK = D / 32;
  const int r16 = lane & 15, q4 = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < QK; ++kk) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(qrow + kk * 32 + 8 * q4 + 4);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(v0[j]), fabsf(v1[j])));
    amax = fmaxf(amax, __shfl_xor(amax, 16));
    amax = fmaxf(amax, __shfl_xor(amax, 32));
    float d, id;
    q8_block_scale(amax, d, id);
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w0 |= (uint32_t)(uint8_t)(int8_t)roundf(v0[j] * id) << (8 * j);
      w1 |= (uint32_t)(uint8_t)(int8_t)roundf(v1[j] * id) << (8 * j);
    }
    qa[kk] = live ? (long)(((unsigned long)w1 << 32) | w0) : 0l;
    if (q4 == 0) qd[r16][kk] = live ? (float)(_Float16)d : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's scales landed
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int kk = 0; kk < QK; ++kk) dq[i][kk] = qd[4 * q4 + i][kk];
}

constexpr int KVQ_PS = ATTN_CHUNK + 4;  // floats per row of a wave's P tile (16-byte aligned rows)

// One chunk [p0, p0 + 32) for the 16 MFMA rows of this wave.  Row 4*q4 + i attends to keys <= qlast[i]; keys past
// `last` (>= every qlast) were never written and must not reach P.V; rows >= nlive are padding (their P is zero).
//   scores: per block one v_mfma_i32_16x16x32_i8 from a zero accumulator -- the exact integer sum -- then
//           s += (d_q d_k) (float)sumi in f32, blocks ascending (ggml's vec_dot_q8_0_q8_0)
//   softmax: online, log2 domain, DPP row reductions (attn_decode_body's)
//   P.V: P goes through LDS in f32; per block A = f16(p * d_v[pos][block]) -- the only rounding of the term -- and
//        B = V's int8 widened to f16 (exact), v_mfma_f32_16x16x32_f16 into the f32 accumulators
template <int D>
__device__ __forceinline__ void q8_chunk(const KvqFrag<D>& f, const long (&qa)[D / 32], const float (&dq)[4][D / 32],
                                         int p0, const int (&qlast)[4], int last, int nlive, float sl2, int lane,
                                         float (*Ps)[KVQ_PS], float (&m_i)[4], float (&l_i)[4], f32x4 (&o)[D / 16]) {
  constexpr int QK = D / 32, DT = D / 16, CH = ATTN_CHUNK;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int pb = p0 + 8 * q4;  // first position of this lane's P.V fragments
  f32x4 sc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < QK; ++kk) {
      const u32x4& kw = f.k[t][kk >> 1];
      const long b = (long)(((unsigned long)kw[2 * (kk & 1) + 1] << 32) | kw[2 * (kk & 1)]);
      const i32x4 sumi = __builtin_amdgcn_mfma_i32_16x16x32_i8(qa[kk], b, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const float dk = (float)f.kd[t][kk];
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[t][i] += (dq[i][kk] * dk) * (float)sumi[i];
    }
  }
  // C layout: rows = MFMA rows 4*q4 + i, cols = positions (lane r16); the selects drop whatever a never-written
  // position's bytes made of its score
  float e[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v0 = (p0 + r16 <= qlast[i]) ? sc[0][i] * sl2 : -INFINITY;
    const float v1 = (p0 + 16 + r16 <= qlast[i]) ? sc[1][i] * sl2 : -INFINITY;
    const float m_new = fmaxf(m_i[i], row16_max(fmaxf(v0, v1)));
    const bool none = m_new == -INFINITY;  // a prefill row whose keys all lie in later chunks: cannot happen for
                                           // chunk 0 (key 0 is every row's), kept as attn_prefill_kernel keeps it
    const float alpha = none ? 1.f : __builtin_amdgcn_exp2f(m_i[i] - m_new);  // 0 on the first chunk (m_i = -inf)
    e[0][i] = none ? 0.f : __builtin_amdgcn_exp2f(v0 - m_new);
    e[1][i] = none ? 0.f : __builtin_amdgcn_exp2f(v1 - m_new);
    l_i[i] = l_i[i] * alpha + row16_sum(e[0][i] + e[1][i]);
    m_i[i] = m_new;
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t][i] *= alpha;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) Ps[4 * q4 + i][16 * t + r16] = (4 * q4 + i < nlive) ? e[t][i] : 0.f;
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes landed
  __builtin_amdgcn_wave_barrier();
  const f32x4 pl = *reinterpret_cast<const f32x4*>(&Ps[r16][8 * q4]);
  const f32x4 ph = *reinterpret_cast<const f32x4*>(&Ps[r16][8 * q4 + 4]);
  const bool partial = p0 + CH > last + 1;  // wave-uniform
#pragma unroll
  for (int b = 0; b < QK; ++b) {
    f16x8 pa;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pa[j] = (_Float16)(pl[j] * (float)f.vd[b][j]);
      pa[4 + j] = (_Float16)(ph[j] * (float)f.vd[b][4 + j]);
    }
    if (partial) {  // a never-written scale may be a NaN: 0 * NaN must not reach the accumulators (V's bytes widen
                    // to finite values whatever they are)
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[j] = (pb + j <= last) ? pa[j] : (_Float16)0.f;
    }
    o[2 * b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, i8x8_to_f16(f.v[b][0], f.v[b][1]), o[2 * b], 0, 0, 0);
    o[2 * b + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, i8x8_to_f16(f.v[b][2], f.v[b][3]), o[2 * b + 1], 0, 0, 0);
  }
  __builtin_amdgcn_wave_barrier();  // Ps is rewritten next chunk only after every lane read it
}

}  // namespace mx
