// lora.hip -- the LoRA merge of the model loader: W' = bf16(W + scale * B A), in place on the
// bf16 row-major matrix the loader holds in its staging buffer, before launch_pack lays it out for the kernels.
//
// A translation unit of its own, like kvpack.hip: kernels.hip's code object stays byte for byte what it was.
#include "device_common.h"

namespace mx {

// W [rows][cols] bf16, A [r][cols] f32, B [rows][r] f32.  A work-group of 256 threads owns a tile of LORA_TR rows
// x LORA_TC columns: thread (ty, tx) = (tid / 32, tid % 32) the rows ty * 8 .. + 8 and the columns tx * 8 .. + 8,
// so a wave reads and writes 512 contiguous bytes of two rows with 16 bytes per lane.  The rank is walked in
// chunks of LORA_RC: A's chunk [RC][TC] and B's chunk, transposed to [RC][TR], are staged in LDS, zero-filled
// outside the matrix and past r, and every thread runs 64 f32 FMAs per rank step on two 16-byte LDS reads of
// each.  The W tile is loaded before the rank loop, so its HBM latency hides behind the first chunks.
// VEC: cols % 8 == 0, every row starts on a 16-byte boundary (all model matrices); otherwise W and A are
// accessed element by element with the same tiling.
constexpr int LORA_TR = 64, LORA_TC = 256, LORA_RC = 16, LORA_BS = LORA_TR + 4;

template <bool VEC>
__global__ __launch_bounds__(256) void lora_merge_kernel(uint16_t* __restrict__ w, const float* __restrict__ A,
                                                         const float* __restrict__ B, int rows, int cols, int r,
                                                         float scale) {
  __shared__ __attribute__((aligned(16))) float As[LORA_RC][LORA_TC];
  __shared__ __attribute__((aligned(16))) float Bs[LORA_RC][LORA_BS];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int row0 = blockIdx.y * LORA_TR, col0 = blockIdx.x * LORA_TC;
  const int c = col0 + tx * 8, rt = row0 + ty * 8;

  u32x4 wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    wv[i] = u32x4{0u, 0u, 0u, 0u};
    const int row = rt + i;
    if (row >= rows) continue;
    const size_t base = (size_t)row * cols + c;
    if (VEC) {
      if (c < cols) wv[i] = *reinterpret_cast<const u32x4*>(w + base);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c + e < cols) wv[i][e >> 1] |= (uint32_t)w[base + e] << (16 * (e & 1));
    }
  }

  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;

  for (int j0 = 0; j0 < r; j0 += LORA_RC) {
    // A chunk: 16 rank rows of 256 columns, 64 threads x 16 bytes per row.  A thread's 8 columns are kept as two
    // halves 128 floats apart (columns 8 tx .. + 4 at 4 tx, 8 tx + 4 .. + 4 at 128 + 4 tx), so the 16-byte LDS
    // reads of neighbouring lanes are contiguous
#pragma unroll
    for (int p = 0; p < LORA_RC / 4; ++p) {
      const int j = p * 4 + (tid >> 6), cc = (tid & 63) * 4, gc = col0 + cc;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (j0 + j < r) {
        const float* src = A + (size_t)(j0 + j) * cols + gc;
        if (VEC) {
          if (gc < cols) v = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gc + e < cols) v[e] = src[e];
        }
      }
      *reinterpret_cast<f32x4*>(&As[j][((cc >> 2) & 1) * 128 + (cc >> 3) * 4]) = v;
    }
    // B chunk, transposed: Bs[j][row]
#pragma unroll
    for (int p = 0; p < LORA_TR * LORA_RC / 256; ++p) {
      const int e = p * 256 + tid, lr = e / LORA_RC, j = e % LORA_RC;
      float v = 0.f;
      if (row0 + lr < rows && j0 + j < r) v = B[(size_t)(row0 + lr) * r + j0 + j];
      Bs[j][lr] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LORA_RC; ++j) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[j][tx * 4]);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[j][128 + tx * 4]);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Bs[j][ty * 8]);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Bs[j][ty * 8 + 4]);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float b = i < 4 ? b0[i & 3] : b1[i & 3];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = fmaf(b, e < 4 ? a0[e & 3] : a1[e & 3], acc[i][e]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = rt + i;
    if (row >= rows) continue;
    const size_t base = (size_t)row * cols + c;
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = f2bf(bf2f((wv[i][e >> 1] >> (16 * (e & 1))) & 0xffffu) + scale * acc[i][e]);
    if (VEC) {
      if (c < cols)
        *reinterpret_cast<u32x4*>(w + base) =
            u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c + e < cols) w[base + e] = (uint16_t)h[e];
    }
  }
}

int launch_lora_merge(uint16_t* w, const float* A, const float* B, int rows, int cols, int r, float scale,
                      hipStream_t s) {
  if (!w || !A || !B || rows < 1 || cols < 1 || r < 1) return -1;
  const size_t gy = ((size_t)rows + LORA_TR - 1) / LORA_TR;
  if (gy > 65535) return -1;
  const dim3 grid((unsigned)((cols + LORA_TC - 1) / LORA_TC), (unsigned)gy);
  // 16-byte accesses need every row of W and of A on a 16-byte boundary
  const bool vec = cols % 8 == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)A & 15) == 0;
  if (vec) lora_merge_kernel<true><<<grid, 256, 0, s>>>(w, A, B, rows, cols, r, scale);
  else lora_merge_kernel<false><<<grid, 256, 0, s>>>(w, A, B, rows, cols, r, scale);
  return 0;
}

}  // namespace mx
