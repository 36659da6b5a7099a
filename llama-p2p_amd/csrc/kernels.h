// kernels.h -- launch interface of the gfx950 kernels (kernels.hip).
//
// Every kernel here replaces one ggml CPU op of llama.cpp's llm_build_llama
// (the forward pass behind /root/reference/llama_p2p_network.py:125; see
// SURVEY.md §3.3 and §8a rows a5-a14).  Host code calls only these wrappers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace mx {

// Weight matrices live in HBM as bf16 "MFMA tiles": tile (nt, kt) holds rows
// [16nt, 16nt+16) x cols [32kt, 32kt+32) of W[N][K] (GGUF order) in exactly the
// lane order of the A operand of v_mfma_f32_16x16x32_bf16, 1 KiB per tile,
// tiles ordered nt-major so a wave streaming along K reads contiguous 1 KiB
// pieces: element (lane, j) of tile = W[16nt + (lane&15)][32kt + 8(lane>>4) + j].
constexpr int TILE_N = 16;
constexpr int TILE_K = 32;
constexpr int TILE_ELEMS = TILE_N * TILE_K;
constexpr int MAX_ROWS = 64;       // tokens per decode / logits forward (4 column tiles of 16)
constexpr int PREFILL_ROWS = 4096;  // tokens per prefill forward (GEMM path, no logits): ~0.3 GB of activations for 8B
constexpr int ATTN_CHUNK = 32;     // positions per attention wave-iteration
constexpr int KV_POS_ALIGN = 64;   // KV rows per slot are allocated in multiples of this
constexpr int ATTN_FIN_MAXSLAB = 8;  // split-K slabs the attention's FIN path can sum (the wide launchers split K at most 8 ways)

enum Epilogue : int {
  EPI_F32 = 0,     // out[col][row] = acc                         (lm_head logits)
  EPI_RESID = 1,   // x[col][row] += acc                          (attn_output, ffn_down)
  EPI_QKV = 2,     // rope(q,k); q -> f32 buffer, k/v -> f16 KV cache (attn_q/k/v)
  EPI_SWIGLU = 3,  // act = bf16(silu(gate) * up); tile = 8 gate + 8 up rows (ffn_gate/ffn_up)
  EPI_SLAB = 4,    // split-K partial: out = slab[ksplit][col][row] (reduced by resid_norm / qkv_finish)
  EPI_QKV_BIAS = 5,  // template tag only (mm_pers_kernel): EPI_QKV's instance for a launch with a q/k/v bias
};

struct AttnArgs {
  const float* q;        // [M][n_head*head_dim] f32 (post-RoPE)
  const _Float16* kc;    // [slots][n_head_kv][ctx_stride * head_dim], 1 KiB B-operand tiles (kernels.hip)
  const _Float16* vc;    // [slots][n_head_kv][ctx_stride * head_dim], 1 KiB B-operand tiles
  const int* pos;        // [M]  query position; attends to [0, pos]
  const int* slot;       // [M]
  uint16_t* out;         // bf16 [M][ldo] (src1 of attn_output)
  int ldo;
  float* outf;           // f32 [M][ldo] instead of out (Q8_0 models quantise it next)
  int M, n_head, n_head_kv, head_dim, n_ctx, ctx_stride;
  size_t slot_stride;
  float scale;
  // qkv still as split-K partial slabs (wide path): the kernel sums them in slab order, applies
  // RoPE, stores this position's K/V into the caches and keeps q and the new K/V in LDS
  const float* slabs;    // [nslab][M][n_q + 2*n_kv] or nullptr (q / caches already final)
  int nslab;
  size_t slab_stride;
  const float* rope_cs;  // [n_ctx][head_dim/2][2]
  _Float16 *kc_w, *vc_w; // writable views of kc / vc
  // diagnosis only (mx_profile_kernel with MX_ATTN_TRACE): per (row, kv head, wave) 8 wall-clock
  // stamps (100 MHz) at the kernel's phases; nullptr normally
  unsigned long long* trace;
  // q/k/v bias (Qwen2): f32 [n_q + 2*n_kv] in the packed QKV row order, added by the FIN path to
  // the summed slabs before RoPE; nullptr = none
  const float* qkv_bias;
};

struct MMArgs {
  const uint16_t* W;   // packed tiles
  int N, K;            // logical W[N][K]; for SWIGLU N = 2*n_ff (interleaved tiles)
  const uint16_t* X;   // activations bf16 [>=16*NB rows][ldx]
  int ldx;
  int M;               // valid columns (tokens)
  // RMS_NORM on load (X == nullptr, M <= 16): B = bf16((xf * scale) * norm_w), scale from ssq
  const float* xf;
  const float* norm_w;
  float eps;
  // per-16-row-tile sums of squares of the residual stream, [M][np]: read by RMS_NORM-on-load
  // consumers (np = K/16), written by EPI_RESID producers when non-null (np = N/16)
  float* ssq;
  int np;
  // epilogue operands
  float* out;          // EPI_F32: [M][ldo]; EPI_RESID: residual x [M][ldo]; EPI_QKV: q [M][ldo]
  int ldo;
  uint16_t* act;       // EPI_SWIGLU: bf16 [M][lda]
  int lda;
  float* actf;         // EPI_SWIGLU: f32 [M][lda] instead of act (Q8_0 models quantise it next)
  // Q8_0 weights (mq8_kernel): activations as Q8_0 rows, xq int8 [M][K] (k permuted within
  // 64-k groups, see q8_perm) and xd f32 [M][K/32] (the f16-rounded block scales)
  const int8_t* xq;
  const float* xd;
  // EPI_QKV
  int n_q, n_kv, head_dim;     // rows [0,n_q) q, [n_q,n_q+n_kv) k, rest v
  const int* pos;              // [M]
  const int* slot;             // [M]
  const float* rope_cs;        // [n_ctx][head_dim/2][2]
  _Float16* kc;                // K cache of this layer: [slots][n_head_kv][ctx_stride * head_dim] (tiled)
  _Float16* vc;                // V cache of this layer: [slots][n_head_kv][ctx_stride * head_dim] (tiled)
  int n_ctx, ctx_stride, n_head_kv;
  size_t slot_stride;          // elements per slot in kc/vc = n_head_kv*ctx_stride*head_dim
  size_t slab_stride;          // EPI_SLAB: floats between consecutive K-split partial slabs
  // K-quant weights (mkq_kernel): activations as Q8_K rows -- xq int8 [M][K] (permuted within each
  // super-block, kquant.hip), xd f32 [M][K/256], xb f32 [M][K/32] (sub-block sums of q) -- and W
  // as up to 3 row segments of one ggml type each (e.g. q|k Q4_K, v Q6_K): segment i holds packed
  // tiles [kq_tile_end[i-1], kq_tile_end[i]) at byte offset kq_off[i] from W
  const float* xb;
  int wq4;             // Q8_0-path GEMVs: W holds Q4_0 tiles (Q4_TILE_BYTES) instead of Q8 tiles
  int kq_n;
  int kq_type[3];
  int kq_tile_end[3];
  size_t kq_off[3];
  // bf16 GEMVs, batch invariance: K is cut into 16 canonical slices
  // [KT*j/16, KT*(j+1)/16) and a row's sum is ((slices of group 0) + (slices of group 1)) + ...
  // over kgrp groups of 16/kgrp consecutive slices -- set by the launchers from the shape alone
  // (canon_kgroups), never by the row count.  mm_wide_kernel: kgrp < 0 = one MFMA chain over the
  // whole K range (no slices): the prefill GEMM's order, for prompt chunks of <= 64 rows
  int kgrp;
  // EPI_QKV: q/k/v bias, f32 [N] in the packed row order, added to the finished sum before RoPE (ggml_add then
  // rope); nullptr = none
  const float* qkv_bias;
};



// packing / synthetic weights.  mode: PACK_ROWS (logical row r -> packed row r + offset),
// PACK_GATE / PACK_UP (ffn_gate / ffn_up rows interleaved by 8-row halves of each tile)
enum PackMode : int { PACK_ROWS = 0, PACK_GATE = 1, PACK_UP = 2 };
void launch_synth_packed(uint16_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                         int row_offset, hipStream_t s);
void launch_synth_rowmajor(uint16_t* dst, size_t n, uint64_t seed, uint64_t tid, float scale, hipStream_t s);
void launch_synth_norm(float* dst, size_t n, uint64_t seed, uint64_t tid, float scale, hipStream_t s);
void launch_pack(uint16_t* dst, const uint16_t* src_rowmajor, int N, int K, int mode, int row_offset,
                 hipStream_t s);
// Qwen2's NeoX RoPE as the kernels' adjacent-pair RoPE: the rows of attn_q / attn_k permuted inside each head of d
// rows, dst row 2i + j = src row j*d/2 + i (llama.cpp's permute for HF-Llama checkpoints).  Rows are row_bytes
// contiguous bytes (bf16, or the raw blocks of a row, before they are packed); dst != src.  -1 for bad arguments.
int launch_permute_rows_neox(void* dst, const void* src, size_t n_rows, size_t row_bytes, int d, hipStream_t s);

// forward-pass ops
// ssq (optional): per-16-element-tile sums of squares of each embedded row, [M][n_embd/16]
void launch_embed(float* x, const uint16_t* tok_embd, const int* ids, int M, int n_embd, float* ssq, hipStream_t s);
void launch_ssq(const float* x, int M, int n, float* ssq, hipStream_t s);
void launch_rmsnorm(uint16_t* y, int ldy, const float* x, const float* w, const int* row_map, int M, int n,
                    float eps, hipStream_t s);
// ---- embeddings: final RMS_NORM + MUL in f32, pooling, L2 normalisation; n % 64 == 0,
// n <= 16384 (-1 otherwise, nothing launched).  src / dst / rows: device row indices, nullptr = 0, 1, 2, ...
// norm: y[dst[c]] = (x[src[c]] * rms_scale(Σx², n, eps)) * w for c < M, Σx² the canonical sum of launch_rmsnorm
int launch_embd_norm(float* y, const float* x, const float* w, const int* src, const int* dst, int M, int n,
                     float eps, hipStream_t s);
// mean: seg [n_seg][EMBD_SEG] = {first y row, rows >= 1, acc row, out row, first, T}: the running sum of a
// sequence -- its first row (first != 0) or acc[acc row] -- plus the segment's rows of y in order goes to
// acc[acc row] (T == 0: more rows follow in a later chunk) or, divided by T, to out[out row]
constexpr int EMBD_SEG = 6;
int launch_embd_mean(const float* y, const int* seg, int n_seg, int n, float* acc, float* out, hipStream_t s);
// l2: v[rows[c]] /= ||v[rows[c]]|| in place for c < M (canonical Σv²); a vector of norm 0 is left as it is
int launch_embd_l2(float* v, const int* rows, int M, int n, hipStream_t s);
int launch_mm(int epi, const MMArgs& a, hipStream_t s);
// canonical K groups of a bf16 GEMV shape (= the K split of its 17..64-row mm_wide launch)
int canon_kgroups(int epi, int N, int K);
bool mm_can_norm_on_load(int M, int K);
// <= 16 rows, row-tile-persistent gate/up: -1 if the shape has no instantiation
bool mm_pers_supported(int epi, int M, int N, int K);
int launch_mm_pers(int epi, const MMArgs& a, hipStream_t s);
// 17..64 rows: activation chunks shared through LDS.  EPI_QKV / EPI_RESID run split-K into
// `slabs` ([ksplit][MAX_ROWS][N] floats, slab_stride apart); returns the split used (the caller
// folds RESID partials with launch_resid_norm; QKV partials are finished inside), or -1.
int launch_mm_wide(int epi, const MMArgs& a, float* slabs, size_t slab_stride, hipStream_t s,
                   bool qkv_finish = true, bool full_chain = false);  // EPI_QKV: false leaves the slabs to the attention kernel
// x[c] += sum of nslab partial slabs (fixed order); then, if y, y = bf16(rmsnorm(x) * w)
void launch_resid_norm(uint16_t* y, int ldy, float* x, const float* slabs, int nslab, size_t slab_stride,
                       const float* w, int M, int n, float eps, hipStream_t s);  // X == nullptr path (RMS_NORM fused into the GEMV) is legal
void launch_attention(const AttnArgs& a, hipStream_t s);
// rows in blocks of 16 consecutive positions of one sequence each (prefill chunks): one
// work-group per (kv head, block), the 16 queries share every K/V chunk
void launch_attention_prefill(const AttnArgs& a, hipStream_t s);
// prefill (> MAX_ROWS rows): MFMA GEMM over packed weights with the same epilogues (N % 256, K % 64)
bool gemm_supported(int N, int K);
int launch_gemm(int epi, const MMArgs& a, hipStream_t s);
// the same GEMM split over K when it has too few work-groups to fill the CUs (small prefills;
// ~target work-groups, 0 = never split): partials go to `slabs` ([S][M][N] floats, at most slab_floats); QKV / SWIGLU are finished
// inside; returns S for EPI_RESID (the caller folds the partials with launch_resid_norm, slab
// stride M*N), 0 when the epilogue ran in place, -1 on a bad shape
int launch_gemm_split(int epi, const MMArgs& a, float* slabs, size_t slab_floats, int target, hipStream_t s);
// ---- Q8_0 weights.  Packed tile = 16 rows x 64 k, Q8_TILE_BYTES:
// [0,1024): int8 A operands of two v_mfma_i32_16x16x32_i8, lane l = row l&15 holds 8 bytes of
// block 0 (k 8(l>>4)..+8) then 8 bytes of block 1 (k 32+8(l>>4)..+8); [1024,1088): f16 block
// scales, row group g = rows 4g..4g+3: [block 0 x 4 rows][block 1 x 4 rows].  Tiles nt-major.
constexpr int Q8_TILE_K = 64;
constexpr int Q8_TILE_BYTES = 1088;
inline size_t q8_matrix_bytes(int N, int K) { return (size_t)N / 16 * (K / Q8_TILE_K) * Q8_TILE_BYTES; }
void launch_pack_q8(uint8_t* dst, const uint8_t* src_blocks, int N, int K, int mode, int row_offset, hipStream_t s);
// ---- Q4_0 weights (GGUF type 2: 32 weights = f16 d + 16 bytes, q - 8) on the Q8_0
// path: a packed Q4 tile = 16 rows x 64 k in Q4_TILE_BYTES: [0,512) lane l = row l&15 holds 4 bytes of
// block 0 then 4 of block 1, its 8 values k 8(l>>4)..+8 as low nibbles (first 4) and high nibbles (last
// 4) of those bytes -- unpacked (and shifted by -8) into the int8 A operand of the same
// v_mfma_i32_16x16x32_i8 as a Q8 tile; [512,576): the f16 block scales as in a Q8 tile.  The activations
// are Q8_0 rows: ggml's ggml_vec_dot_q4_0_q8_0 (exact int32 block sums, scaled by d_w * d_x in f32).
constexpr int Q4_TILE_BYTES = 576;
inline size_t q4_matrix_bytes(int N, int K) { return (size_t)N / 16 * (K / Q8_TILE_K) * Q4_TILE_BYTES; }
void launch_pack_q4(uint8_t* dst, const uint8_t* src_blocks, int N, int K, int mode, int row_offset, hipStream_t s);
// synthetic Q4_0 matrix: ggml quantize_row_q4_0_ref of the bf16 synthetic values, packed
void launch_synth_q4_packed(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                            int row_offset, hipStream_t s);
// packed Q8 tiles of a [N][K] matrix -> packed bf16 tiles (prefill GEMM operand), values d*q -> bf16
int launch_dequant_q8_tiles(uint16_t* dst, const uint8_t* W, int N, int K, hipStream_t s);
void launch_synth_q8_packed(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, int mode,
                            int row_offset, hipStream_t s);
void launch_synth_q8_rowmajor(uint8_t* dst, int N, int K, uint64_t seed, uint64_t tid, float scale, hipStream_t s);
// any GGUF matrix type (F32 0, F16 1, Q4_0 2, Q8_0 8, Q4_K 12, Q5_K 13, Q6_K 14) -> bf16 row-major,
// n elements (ggml dequantize_row_*, then RNE to bf16); -1 for an unsupported type or ragged n
int ggml_block_elems(int type);
int launch_dequant_bf16(uint16_t* dst, const uint8_t* src, int type, size_t n, hipStream_t s);
// LoRA merge at load (lora.hip), in place on a bf16 row-major matrix w [rows][cols]:
// w' = bf16_rne(f32(w) + scale * sum_j B[n][j] A[j][k]), the sum and the update in f32 (plain VALU FMAs); A f32
// [r][cols], B f32 [rows][r], any rows, cols, r >= 1 (16-byte accesses when cols % 8 == 0).  -1: nothing launched.
int launch_lora_merge(uint16_t* w, const float* A, const float* B, int rows, int cols, int r, float scale,
                      hipStream_t s);
// Grammar mask (grammar.hip) on logits [M][ldl] with V valid columns: row i with on[i] != 0 gets
// -inf in every column t < V whose bit (masks[i][t >> 5] >> (t & 31)) & 1 is clear; nothing else is written and
// the rows are never read.  masks [M][ceil(V / 32)].  M 1..MAX_ROWS, ldl >= V.  -1: nothing launched.
int launch_grammar_mask(float* logits, int ldl, int M, int V, const uint32_t* masks, const uint32_t* on,
                        hipStream_t s);
void launch_embed_q8(float* x, const uint8_t* tok_embd_blocks, const int* ids, int M, int n_embd, float* ssq,
                     hipStream_t s);
// RMS_NORM + MUL, quantised to Q8_0 activation rows (xq [M][n], xd [M][n/32])
void launch_rmsnorm_q8(int8_t* xq, float* xd, const float* x, const float* w, const int* row_map, int M, int n,
                       float eps, hipStream_t s, const float* slabs = nullptr, int nslab = 0,
                      size_t slab_stride = 0);  // nslab: fold the producer's split-K slabs into x first
void launch_quantize_q8(int8_t* xq, float* xd, const float* src, int ld, int M, int n, hipStream_t s);
// Q8_0 x Q8_0 products for any M (column groups of <= 64 tokens on grid.y), same epilogues.
// a.xq == nullptr: quantise on load from f32 rows a.xf ([M][K]; RMS_NORM + MUL first when norm_w,
// scale from the ssq partials), for mq8_can_quantize_on_load(M, K, norm_w != nullptr).  EPI_RESID writes ssq
// partials when a.ssq.
int launch_mq8(int epi, const MMArgs& a, hipStream_t s);
// 17..32 tokens: split-K partial slabs ([ks][token][N]) for launch_rmsnorm_q8 to fold (attn_output /
// ffn_down) or the attention / launch_qkv_finish to finish (q|k|v); ks, or -1 (use launch_mq8)
int launch_mq8_slab(const MMArgs& a, float* slabs, size_t slab_stride, hipStream_t s);
bool mq8_can_quantize_on_load(int M, int K, bool norm);
// The kernel launch_mq8 reaches for a shape (a pure host function: launch_mq8 dispatches on its result).
// on_load: a.xq == nullptr; norm: a.norm_w given.  kind MQ8_NONE: launch_mq8 refuses the shape.
enum Mq8Kind : int {
  MQ8_NONE = 0,
  MQ8_QL = 1,       // mq8_kernel quantising on load: qp (float4 per lane and row), qm (row slots), bd (M == 1)
  MQ8_PERS_QL = 2,  // mq8_pers_ql_kernel: tpw tiles per work-group
  MQ8_GEMV = 3,     // mq8_kernel<ks, rt, nb> on Q8_0 rows, bd = the block-diagonal one-token form, grid_y
  MQ8_WIDE = 4,     // mq8_wide_kernel<w> (Q8_0 weights)
  MQ8_WSW = 5,      // mq8_wsw_kernel<w> (Q4_0 weights)
  MQ8_GEMM = 6,     // q8gemm_kernel on `grid` work-groups
};
struct Mq8Plan {
  int kind, qp, qm, tpw, ks, rt, nb, bd, grid_y, w, grid;
};
Mq8Plan mq8_plan(int epi, int M, int N, int K, bool wq4, bool on_load, bool norm);
// split of launch_mq8_slab for a shape, -1 = it refuses (the conditions on the shape alone)
int mq8_slab_ks(int M, int N, int K);

// ---- K-quant weights (GGUF Q4_K 12, Q5_K 13, Q6_K 14), kquant.hip.  Packed tile =
// 16 rows x 256 k (one super-block per row) in MFMA operand lane order: kq_tile_bytes(type) bytes
// (2368 / 2880 / 3360), tiles nt-major like the bf16 tiles.
int kq_tile_bytes(int type);  // 0 for a type without a K-quant tile
int kq_block_bytes(int type);  // GGUF block bytes per 256 weights (144 / 176 / 210)
inline size_t kq_matrix_bytes(int type, int N, int K) { return (size_t)N / 16 * (K / 256) * kq_tile_bytes(type); }
// GGUF blocks [N][K/256] -> packed tiles (packed_row modes as launch_pack); -1 for a bad type/shape
int launch_pack_kq(uint8_t* dst, const uint8_t* src_blocks, int type, int N, int K, int mode, int row_offset,
                   hipStream_t s);
// the synthetic model's GGUF blocks (synth.py kq_blocks), row-major
int launch_synth_kq_blocks(uint8_t* dst, int type, size_t nblocks, uint64_t seed, uint64_t tid, hipStream_t s);
// GET_ROWS of a K-quant token_embd (dequantize_row_q{4,5,6}_K, f32)
// ssq (optional): per-16-element-tile sums of squares of each embedded row (quantise-on-load consumers)
int launch_embed_kq(float* x, const uint8_t* tok_blocks, int type, const int* ids, int M, int n, float* ssq,
                    hipStream_t s);
// one token whose K-quant GEMVs quantise their Q8_K operand on load (xq == nullptr: xf, norm_w, ssq, np)
bool mkq_can_quantize_on_load(int M, int K, bool norm);
// RMS_NORM + MUL then Q8_K (xq [M][n], xd [M][n/256], xb [M][n/32]); plain Q8_K of f32 rows
// (nslab > 0: first fold the split-K slabs of the GEMV that wrote x into x, see launch_mkq_slab)
int launch_rmsnorm_q8k(int8_t* xq, float* xd, float* xb, const float* x, const float* w, const int* row_map, int M,
                       int n, float eps, hipStream_t s, const float* slabs = nullptr, int nslab = 0,
                       size_t slab_stride = 0);
int launch_quantize_q8k(int8_t* xq, float* xd, float* xb, const float* src, int ld, int M, int n, hipStream_t s);
// K-quant x Q8_K products for any M (grid.y: groups of 32 tokens), the usual epilogues (SWIGLU: actf)
int launch_mkq(int epi, const MMArgs& a, hipStream_t s);
// 17..32 tokens, attn_output / ffn_down: split-K partials into slabs ([ks][token][N], slab_stride apart)
// for launch_rmsnorm_q8k to fold; returns ks, or -1 when the shape has no such form (use launch_mkq)
int launch_mkq_slab(const MMArgs& a, float* slabs, size_t slab_stride, hipStream_t s);
// 17..32 tokens, q|k|v: split-K partial slabs for the attention's FIN path or launch_qkv_finish
int launch_mkq_qkv_slab(const MMArgs& a, float* slabs, size_t slab_stride, hipStream_t s);
// q/k/v split-K partial slabs -> sum in slab order -> RoPE + q / KV-cache stores (EPI_QKV's epilogue)
void launch_qkv_finish(const MMArgs& a, const float* slabs, int nslab, size_t slab_stride, hipStream_t s);
// The kernel launch_mkq reaches for a shape (a pure host function: launch_mkq and its sub-launchers dispatch
// on its result and on nothing else).  on_load: a.xq == nullptr; norm: a.norm_w given; the row segments as in
// MMArgs.  kind MKQ_NONE: launch_mkq refuses the shape.
enum MkqKind : int {
  MKQ_NONE = 0,
  MKQ_QKV_PERS = 1,  // mkq_pers_seg_kernel<ks, nkw, tpw, EPI_QKV, u>: one token, q|k|v, quantised on load
  MKQ_BD_TILE = 2,   // mkq_bd_tile_kernel<t, w, nkw (= K / 256), tpw, epi, u>: one token on load, whole-K waves
  MKQ_PERS = 3,      // mkq_pers_kernel<t, ks, nkw, tpw, nb, epi, u, ql, bd>
  MKQ_WIDE = 4,      // mkq_wide_kernel<t, w, nb, epi, u>: 17..32 rows, activations shared through LDS
  MKQ_GEMV = 5,      // mkq_kernel<ks, 1, nb, epi, u, ql, bd> on grid (grid_x, grid_y)
};
// the MX_NO_KQ_* / MX_SLAB_TARGET switches (read once per process by mkq_env)
struct MkqEnv {
  bool no_bd_tile, no_pers, no_wide;
  int slab_target;
};
const MkqEnv& mkq_env();
// t: the type of a single-segment matrix (0: chosen per work-group from the segments); nkw: super-blocks per
// wave and tile; tpw: tiles per work-group (MKQ_BD_TILE: per wave); w: waves that own whole tiles
struct MkqPlan {
  int kind, t, ks, nkw, tpw, nb, u, bd, ql, w, grid_x, grid_y;
};
MkqPlan mkq_plan(int epi, int M, int N, int K, bool on_load, bool norm, int kq_n, const int* kq_type,
                 const int* kq_tile_end, const MkqEnv& env);
// the split launch_mkq_slab / launch_mkq_qkv_slab take for a shape, -1 = refused (the conditions on the shape
// alone; both also need pre-quantised rows)
int mkq_slab_ks(int M, int N, int K, int kq_n, const int* kq_type, const MkqEnv& env);
int mkq_qkv_slab_ks(int M, int N, int K, int kq_n, const int* kq_tile_end, const MkqEnv& env);
// packed K-quant matrix (segments as in MMArgs) -> packed bf16 tiles [N/16][K/32] x 1 KiB (prefill GEMM)
int launch_dequant_kq(uint16_t* dst, const void* W, int K, int kq_n, const int* type, const int* tile_end,
                      const size_t* off, hipStream_t s);

// top-k (k <= TOPK_MAX) candidates per logits row, value descending, ties by lower id; ws: M*64*k
constexpr int TOPK_MAX = 64;
int launch_topk(const float* logits, int ldl, int M, int V, int K, float* ws_val, int* ws_idx, float* out_val,
                int* out_idx, hipStream_t s);
void launch_argmax(const float* logits, int ldl, int M, int V, float* ws_val, int* ws_idx, int* tok_out,
                   int* ids_next, int* pos_next, int* hist, int hist_stride, int* hist_count, int max_hist,
                   hipStream_t s);

// ---- prompt-lookup speculative decoding.  R requests, each with 1 + D rows of the forward
// (row r(1+D): its last token; the next D: the draft), R(1+D) <= SPEC_ROWS.
// draft: ctx_tok [R][ctx_stride] holds each request's tokens [0, ctx_len[r]) (ctx_len >= 1), par [R][2] =
// {num_pred_tokens (clamped to D), max_ngram_size}; reads pos / slot of each request's row 0 and writes
// ids / pos / slot of its rows 1..D and n_draft[r] (0..D).
// accept: ws_val / ws_idx = argmax_stage1's partials of all R(1+D) logits rows; per request emits
// argmax[0..a] to hist[r][hist_count[r]..] and ctx_tok[r][ctx_len[r]..], sets ids of row 0, adds a + 1 to
// pos of row 0, ctx_len and hist_count, and steps / drafted / accepted to cnt [R][3]; step_log (optional)
// [R][max_steps][2] = {n_draft, a} of step cnt[r][0].
constexpr int SPEC_ROWS = 16;      // rows of a speculating forward: the <= 16-row decode path
constexpr int SPEC_MAX_DRAFT = 15; // so num_pred_tokens <= 15 ...
constexpr int SPEC_MAX_REQ = 8;    // ... and at most 8 requests (D >= 1) share a round
void launch_spec_draft(const int* ctx_tok, int ctx_stride, const int* ctx_len, const int* par, int R, int D, int* ids,
                       int* pos, int* slot, int* n_draft, hipStream_t s);
void launch_argmax_stage1(const float* logits, int ldl, int M, int V, float* ws_val, int* ws_idx, hipStream_t s);
void launch_spec_accept(const float* ws_val, const int* ws_idx, int R, int D, int* ids, int* pos, const int* n_draft,
                        int* ctx_tok, int ctx_stride, int* ctx_len, int* hist, int hist_stride, int* hist_count,
                        int* cnt, int* step_log, int max_steps, hipStream_t s);

// ---- device sampling chain (llama-cpp-python 0.3's create_completion chain as
// engine.cpp restates it): penalties over the last last_n tokens -> top_k -> top_p -> min_p ->
// temperature -> draw; temperature <= 0 = greedy (after the penalties).  One SampRow per logits row.
constexpr int SAMP_WIN = 64;
struct SampRow {
  float temp, top_p, min_p, repeat, freq, presence;
  int top_k;    // 1..TOPK_MAX on the device path
  int last_n;   // penalty window (0..SAMP_WIN); 0 = no penalties
  uint64_t seed;
  int draw0;    // index of the row's next random draw = tokens the request sampled before this run
  int n_win;    // penalty window at the start of the run: the last n_win tokens of prompt + output
  int win[SAMP_WIN];
};
// counter-based uniform draw in [0, 1) (splitmix64 of seed and draw index): host and device agree
__host__ __device__ inline double samp_u01(uint64_t seed, uint64_t draw) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (draw + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
// tail-free sampling (llama.cpp's tail_free sampler, min_keep 1) over k > 2 candidates sorted by value: the
// |second differences| of the softmax, normalised (1 / (k - 2) each when their sum is <= 1e-6), summed in
// order; the candidates before the first index i >= 1 whose running sum exceeds z stay.  Returns the count.
__host__ __device__ inline int samp_tail_free(const float* vals, int k, float z, double* p, double* w) {
#pragma clang fp contract(off)  // no fused multiply-adds: the host and the device round alike
  const double mx = vals[0];
  double sum = 0;
  for (int i = 0; i < k; i++) sum += (p[i] = exp((double)vals[i] - mx));
  for (int i = 0; i < k; i++) p[i] /= sum;
  double s2 = 0;
  for (int i = 0; i < k - 2; i++) s2 += (w[i] = fabs((p[i] - p[i + 1]) - (p[i + 1] - p[i + 2])));
  for (int i = 0; i < k - 2; i++) w[i] = s2 > 1e-6 ? w[i] / s2 : 1.0 / (k - 2);
  double cum = 0;
  for (int i = 0; i < k - 2; i++) {
    cum += w[i];
    if (cum > z && i >= 1) return i;
  }
  return k;
}
// locally typical sampling (llama.cpp's typical sampler, min_keep 1): q = softmax, H its entropy (0 log 0 = 0),
// the candidates in order of |-log q_i - H| ascending (ties by rank: a stable sort) stay through the first one
// at which their running mass exceeds tp.  The kept ones go to cv / ci in value order again; returns the count.
// ord: scratch of k ints.  Up to TOPK_MAX candidates the sort is the insertion sort the device runs too.
__host__ __device__ inline int samp_typical(const float* vals, const int* ids, int k, float tp, double* p, double* w,
                                            float* cv, int* ci, int* ord) {
#pragma clang fp contract(off)
  const double mx = vals[0];
  double sum = 0;
  for (int i = 0; i < k; i++) sum += (p[i] = exp((double)vals[i] - mx));
  const double ls = log(sum);
  double H = 0;
  for (int i = 0; i < k; i++) {
    p[i] /= sum;
    if (p[i] > 0) H -= p[i] * (((double)vals[i] - mx) - ls);
  }
  for (int i = 0; i < k; i++) w[i] = fabs(-(((double)vals[i] - mx) - ls) - H), ord[i] = i;
#ifndef __HIP_DEVICE_COMPILE__
  if (k > 64) std::stable_sort(ord, ord + k, [w](int a, int b) { return w[a] < w[b]; });
  else
#endif
    for (int i = 1; i < k; i++) {
      const int o = ord[i];
      int j = i;
      for (; j > 0 && w[ord[j - 1]] > w[o]; j--) ord[j] = ord[j - 1];
      ord[j] = o;
    }
  int n = k;
  double cum = 0;
  for (int j = 0; j < k; j++) {
    cum += p[ord[j]];
    if (cum > tp) { n = j + 1; break; }
  }
  for (int j = 0; j < n; j++) w[ord[j]] = -1.0;  // kept (every |.| is >= 0)
  int m = 0;
  for (int i = 0; i < k; i++)
    if (w[i] < 0) cv[m] = vals[i], ci[m] = ids[i], m++;
  return m;
}
// [tail-free -> typical ->] top_p / min_p / temperature / draw over k candidates sorted by value (descending,
// ties lower id first); p and w are scratch of k doubles; cv, ci, ord scratch of k entries each, needed only
// with tfs_z < 1 or typical_p < 1.  The host sampler and the sample kernels both call this.
__host__ __device__ inline int samp_pick(const float* vals, const int* ids, int k, float temp, float top_p,
                                         float min_p, double u01, double* p, double* w, float tfs_z = 1.0f,
                                         float typical_p = 1.0f, float* cv = nullptr, int* ci = nullptr,
                                         int* ord = nullptr) {
  if (temp <= 0.f || k <= 1) return ids[0];
  if (tfs_z < 1.0f || typical_p < 1.0f) {
    if (!(vals[0] > -INFINITY)) return ids[0];  // every candidate banned (logit_bias): no distribution to cut
    if (tfs_z < 1.0f && k > 2) k = samp_tail_free(vals, k, tfs_z, p, w);
    if (typical_p < 1.0f) {
      k = samp_typical(vals, ids, k, typical_p, p, w, cv, ci, ord);
      vals = cv, ids = ci;
    }
    if (k <= 1) return ids[0];
  }
  const double mx = vals[0];
  double sum = 0;
  for (int i = 0; i < k; i++) sum += (p[i] = exp((double)vals[i] - mx));
  for (int i = 0; i < k; i++) p[i] /= sum;
  int keep = k;
  if (top_p < 1.0f) {
    double cum = 0;
    for (int i = 0; i < k; i++) {
      cum += p[i];
      if (cum >= top_p) { keep = i + 1; break; }
    }
  }
  if (min_p > 0.f) {
    int kk = 1;
    for (int i = 1; i < keep; i++)
      if (p[i] >= min_p * p[0]) kk = i + 1;
    keep = kk;
  }
  const double m0 = (double)vals[0] / temp;
  double s2 = 0;
  for (int i = 0; i < keep; i++) s2 += (w[i] = exp((double)vals[i] / temp - m0));
  const double u = u01 * s2;
  double acc = 0;
  for (int i = 0; i < keep; i++) {
    acc += w[i];
    if (u < acc) return ids[i];
  }
  return ids[keep - 1];
}
// ---- the rest of llama-cpp-python's chain: one SampExt per logits row beside its SampRow.
// logit_bias (x[t] += bias, ahead of the penalties; -inf bans), tail-free and locally typical between top_k and
// top_p, or Mirostat v2 over the whole vocabulary in place of top_k .. draw (miro == 2, temperature > 0 only).
constexpr int SAMP_BIAS_MAX = 256;
struct SampExt {
  float typical_p, tfs_z;  // 1 = off
  int miro;                // 2: Mirostat v2; 0: the candidate chain
  float tau, eta;
  int n_bias;              // distinct tokens inside the vocabulary
  int bias_tok[SAMP_BIAS_MAX];
  float bias_val[SAMP_BIAS_MAX];
  int wide_k;              // > TOPK_MAX: the row's candidates are its first wide_k tokens of the order (V: all of
                           // them) and sample_wide_kernel picks it; 0: any other row
};
// the largest vocabulary the whole-vocabulary kernels take (64 slices of 4096 columns)
constexpr int SAMP_WIDE_VMAX = 262144;
// Mirostat v2 of one row on the host, x = the row after bias and penalties: p = softmax(x / temp) over all V, kept =
// surprise -log2 p_i <= mu (the argmax, ties to the lowest id, when none is), the draw u01 over the kept mass walks
// the kept tokens by ascending id, mu -= eta (-log2 p'_tok - tau) with p' renormalised over the kept set.
int miro_pick_host(const float* x, int V, float temp, float tau, float eta, double u01, float* mu);
// workspace of the Mirostat kernels for M rows: floats / doubles / ints
inline size_t miro_ws_floats(int M) { return (size_t)M * 64 * 2 + (size_t)M * 2; }
inline size_t miro_ws_doubles(int M) { return (size_t)M * 64; }
inline size_t miro_ws_ints(int M) { return (size_t)M * 64; }
struct SampExtArgs {
  const SampExt* ext = nullptr;  // [M]; null: the chain as launch_sample_chain always ran it
  float* bias_raw = nullptr;     // [M][SAMP_BIAS_MAX] raw logits of the biased tokens (log-prob gather)
  float* mu = nullptr;           // [M] Mirostat state, updated in place ...
  float* mu_hist = nullptr;      // ... and [M][mu_stride] its value after each step of a run (step 0 without a history)
  int mu_stride = 1;
  float* ws_f = nullptr;         // miro_ws_floats(M)
  double* ws_d = nullptr;        // miro_ws_doubles(M)
  int* ws_i = nullptr;           // miro_ws_ints(M)
  bool any_miro = false;         // some row has miro == 2: the Mirostat launches run
  bool any_wide = false;         // some row has wide_k > 0: the wide launch runs (V <= SAMP_WIDE_VMAX)
};
// penalties (in place on the logits rows), top-k of K = max top_k of the rows, the draw, then the
// same token bookkeeping as launch_argmax (tok_out, ids_next, pos_next, history)
int launch_sample_chain(float* logits, int ldl, int M, int V, const SampRow* samp, int K, float* ws_val, int* ws_idx,
                        float* tk_val, int* tk_idx, int* tok_out, int* ids_next, int* pos_next, int* hist,
                        int hist_stride, int* hist_count, int max_hist, hipStream_t s, int* side_tok = nullptr,
                        float* side_val = nullptr,  // side_*: [M][SAMP_WIN] raw logits the penalties rewrote
                        const SampExtArgs* x = nullptr);  // with x->ext: bias first, tail-free / typical, Mirostat rows
// the pick of the rows with ext[c].wide_k > 0 (every other row is skipped), after launch_topk with K >= 1 wrote the
// rows' first candidate to tk_val / tk_idx [M][K]: the chain of samp_pick over wide_k > TOPK_MAX candidates without a
// sort, and the bookkeeping of sample_kernel.  The logits are only read.  V <= SAMP_WIDE_VMAX.
int launch_sample_wide(const float* logits, int ldl, int M, int V, const SampRow* samp, const SampExt* ext,
                       const float* tk_val, const int* tk_idx, int K, int* tok_out, int* ids_next, int* pos_next,
                       int* hist, int hist_stride, int* hist_count, int max_hist, hipStream_t s);
// ---- per-token log-probabilities, logprob(i) = (x_i - m) - log(sum exp(x - m)) over the raw logits row
// (DESIGN.md §9).  K = 0..min(TOPK_MAX, V) top entries per row (value descending, ties lower id first).
// stats: one read of the rows -> part [M][64][2] slice (max, sum) partials, ms [M][2] = (m, log s) and the
// top-K as log-probs (top_lp / top_idx [M][K]; ws as launch_topk).  gather: per row the entry
// [logprob of toks[c] | K top log-probs | K top ids as int bits] at out[c * row_stride + step * (1 + 2K)],
// step = hist_count[c] - 1 (0 when hist_count is null); side_* as written by launch_sample_chain.
int launch_logprob_stats(const float* logits, int ldl, int M, int V, int K, float* ws_val, int* ws_idx, float* part,
                         float* ms, float* top_lp, int* top_idx, hipStream_t s);
int launch_logprob_gather(const float* logits, int ldl, int M, int V, int K, const int* toks, const int* hist_count,
                          int max_steps, const int* side_tok, const float* side_val, const float* ms,
                          const float* top_lp, const int* top_idx, float* out, size_t row_stride, hipStream_t s,
                          const SampExt* ext = nullptr, const float* bias_raw = nullptr);  // as SampExtArgs
// both, for given target tokens: out [M][1 + 2K]
int launch_logprobs(const float* logits, int ldl, int M, int V, int K, const int* targets, float* ws_val, int* ws_idx,
                    float* part, float* ms, float* top_lp, int* top_idx, float* out, hipStream_t s);
// hand-off conversions of the residual stream (pipeline stages): f32 <-> bf16 rows (RNE), and the
// per-16-element sums of squares of the f32 rows made from bf16 (RMS_NORM-on-load consumers)
void launch_f32_to_bf16(uint16_t* dst, const float* src, size_t n, hipStream_t s);
void launch_copy_f32(float* dst, const float* src, size_t n, hipStream_t s);
void launch_f32_in(float* x, const float* src, int M, int n, float* ssq, hipStream_t s);  // + Σx² partials
void launch_bf16_to_f32(float* dst, const uint16_t* src, int M, int n, float* ssq, hipStream_t s);

// Prefix sharing: copy the K/V of positions [0, P), P = min(ceil32(n_pos), ctx_stride), of slot
// `src` to slot `dst`, for every layer, kv head, K and V of caches laid out [layer][slot][kv head][ctx_stride * D].
// Tiles are position-major (32 positions = two K position tiles = one V position tile), so that is one
// contiguous prefix of P * D elements per (layer, slot, kv head) region of each cache.
struct KvCopy {
  int32_t src, dst, n_pos;
};
// All copies of `tab` (host, n of them; tab_dev: its device copy, already enqueued on s) in one launch.
// Returns -1 and launches nothing unless 1 <= n, every slot is in [0, n_slots), src != dst, 1 <= n_pos <= n_ctx,
// no slot is a destination twice and none is both a source and a destination.
int launch_kv_copy(_Float16* kc, _Float16* vc, const KvCopy* tab, const KvCopy* tab_dev, int n, int n_layer,
                   int n_slots, int n_head_kv, int head_dim, int n_ctx, int ctx_stride, size_t slot_stride,
                   size_t layer_kv_stride, hipStream_t s);
// bytes the launch reads (= bytes it writes)
size_t kv_copy_bytes(const KvCopy* tab, int n, int n_layer, int n_head_kv, int head_dim, int ctx_stride);

// Host-RAM tier: the first P = min(ceil32(n_pos), ctx_stride) positions of slot `slot`, every
// layer, K and V, to or from the packed form packed[t][layer][K|V][kv head][32 * D] f16, t = 0 .. P/32 - 1, that
// starts at 16-byte word off16 of the packed buffer.  Each 32 * D block is the region's bytes [32t * D,
// 32(t+1) * D) verbatim, so the first P' positions of an entry (P' a multiple of 32) are its first P'/32 tiles of
// kv_pack_tile_bytes() each: one contiguous prefix.
struct KvPack {
  int32_t slot, n_pos;
  int64_t off16;
};
size_t kv_pack_tile_bytes(int n_layer, int n_head_kv, int head_dim);
// All entries of `tab` (host, n of them; tab_dev: its device copy, already enqueued on s) in one launch: slot ->
// packed (pack) or packed -> slot (unpack).  Returns -1 and launches nothing unless 1 <= n, every slot is in
// [0, n_slots), 1 <= n_pos <= n_ctx, every offset is a whole number of tiles, every entry ends inside the
// packed_bytes of the buffer, no two packed ranges overlap and (unpack) no slot is a destination twice.
int launch_kv_pack(const _Float16* kc, const _Float16* vc, void* packed, size_t packed_bytes, const KvPack* tab,
                   const KvPack* tab_dev, int n, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                   int ctx_stride, size_t slot_stride, size_t layer_kv_stride, hipStream_t s);
int launch_kv_unpack(_Float16* kc, _Float16* vc, const void* packed, size_t packed_bytes, const KvPack* tab,
                     const KvPack* tab_dev, int n, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                     int ctx_stride, size_t slot_stride, size_t layer_kv_stride, hipStream_t s);

// HBM streaming probes: variant v of probe_variants() (loads in flight, grid, non-temporal) of a
// read-only (XOR fold) or copy stream over n16 16-byte words (n16 % 4096 == 0); desc describes it
int probe_variants();
int launch_probe(int v, bool read_only, const uint4* src, uint4* dst, size_t n16, hipStream_t s, char* desc,
                 int desc_len);

}  // namespace mx
