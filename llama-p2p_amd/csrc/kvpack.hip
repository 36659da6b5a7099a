// kvpack.hip -- the host-RAM tier's two kernels: a KV slot's first positions to and from the packed,
// position-tile-major form that travels to pinned host memory.
//
// A translation unit of its own, so that kernels.hip's code object stays byte for byte what it was: kernels added
// there, even at its end, moved every decode kernel by 2560 B to other page offsets (the tables ahead of .text
// grew), and bench.py's 32-row greedy decode ran 0.2 % slower with identical kernels (DESIGN.md §13 met the same
// effect).
#include <algorithm>
#include <vector>

#include "device_common.h"

namespace mx {

// Host-RAM tier (kernels.h KvPack): the same streams as kv_copy_kernel with one side in the packed,
// position-tile-major form packed[t][layer][K|V][kv head][32 * D].  Grid (chunks of 256 * U 16-byte words of a
// region prefix, layer x kv head x K|V, entry); a row of 32 * D f16 (4 * D / 256 groups of 256 words) is one tile
// of one region, so every 256-word group a work-group moves lies in one tile, its lanes take the same branches
// and both sides of it are 256 consecutive words.  Plain loads and stores, no atomics, no LDS.
template <int U, bool UNPACK>
__device__ __forceinline__ void kv_pack_body(_Float16* kc, _Float16* vc, u32x4* packed, const KvPack& c,
                                             int n_layer, int n_head_kv, int head_dim, int ctx_stride,
                                             size_t slot_stride, size_t layer_kv_stride) {
  const int P = min((c.n_pos + 31) & ~31, ctx_stride);
  const size_t n16 = (size_t)P * head_dim / 8;
  const size_t b0 = (size_t)blockIdx.x * 256 * U;
  if (b0 >= n16) return;
  const int kv = blockIdx.y & 1, lh = blockIdx.y >> 1, layer = lh / n_head_kv, head = lh % n_head_kv;
  const size_t row16 = (size_t)head_dim * 4;                        // 16-byte words of one 32 * D block
  const size_t tile16 = (size_t)n_layer * 2 * n_head_kv * row16;    // ... of one position tile of the entry
  u32x4* reg = reinterpret_cast<u32x4*>((kv ? vc : kc) + (size_t)layer * layer_kv_stride +
                                        (size_t)c.slot * slot_stride + (size_t)head * ctx_stride * head_dim) +
               b0 + threadIdx.x;
  u32x4* pk = packed + (size_t)c.off16 + ((size_t)(layer * 2 + kv) * n_head_kv + head) * row16 + threadIdx.x;
  const int groups = (int)min((size_t)U, (n16 - b0) / 256);
  if (groups == U) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t w = b0 + 256 * u, t = w / row16;
      v[u] = UNPACK ? pk[t * tile16 + (w - t * row16)] : reg[256 * u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t w = b0 + 256 * u, t = w / row16;
      if (UNPACK) reg[256 * u] = v[u];
      else pk[t * tile16 + (w - t * row16)] = v[u];
    }
  } else {
    for (int u = 0; u < groups; ++u) {
      const size_t w = b0 + 256 * u, t = w / row16;
      if (UNPACK) reg[256 * u] = pk[t * tile16 + (w - t * row16)];
      else pk[t * tile16 + (w - t * row16)] = reg[256 * u];
    }
  }
}

template <int U>
__global__ __launch_bounds__(256) void kv_pack_kernel(const _Float16* kc, const _Float16* vc, u32x4* packed,
                                                      const KvPack* __restrict__ tab, int n_layer, int n_head_kv,
                                                      int head_dim, int ctx_stride, size_t slot_stride,
                                                      size_t layer_kv_stride) {
  kv_pack_body<U, false>(const_cast<_Float16*>(kc), const_cast<_Float16*>(vc), packed, tab[blockIdx.z], n_layer,
                         n_head_kv, head_dim, ctx_stride, slot_stride, layer_kv_stride);
}

template <int U>
__global__ __launch_bounds__(256) void kv_unpack_kernel(_Float16* kc, _Float16* vc, const u32x4* packed,
                                                        const KvPack* __restrict__ tab, int n_layer, int n_head_kv,
                                                        int head_dim, int ctx_stride, size_t slot_stride,
                                                        size_t layer_kv_stride) {
  kv_pack_body<U, true>(kc, vc, const_cast<u32x4*>(packed), tab[blockIdx.z], n_layer, n_head_kv, head_dim,
                        ctx_stride, slot_stride, layer_kv_stride);
}

size_t kv_pack_tile_bytes(int n_layer, int n_head_kv, int head_dim) {
  return (size_t)n_layer * 2 * n_head_kv * 32 * head_dim * 2;
}

// the checks of both directions; the grid's x extent on success, 0 on a refusal
static unsigned kv_pack_check(const void* kc, const void* vc, const void* packed, size_t packed16, const KvPack* tab,
                              const KvPack* tab_dev, int n, int n_layer, int n_slots, int n_head_kv, int head_dim,
                              int n_ctx, int ctx_stride, bool unpack, int U) {
  if (!kc || !vc || !packed || !tab || !tab_dev || n < 1 || n > 65535 || n_layer < 1 || n_slots < 1 ||
      n_head_kv < 1 || (head_dim != 64 && head_dim != 128) || n_ctx < 1 || ctx_stride < n_ctx || ctx_stride % 32 ||
      (size_t)n_layer * n_head_kv * 2 > 65535)
    return 0;
  const size_t tile16 = kv_pack_tile_bytes(n_layer, n_head_kv, head_dim) / 16;
  std::vector<char> dst(n_slots, 0);
  std::vector<std::pair<size_t, size_t>> ranges(n);  // [first, end) in 16-byte words
  int max_pos = 0;
  for (int i = 0; i < n; i++) {
    const KvPack& c = tab[i];
    if (c.slot < 0 || c.slot >= n_slots || c.n_pos < 1 || c.n_pos > n_ctx) return 0;
    if (c.off16 < 0 || (size_t)c.off16 % tile16) return 0;
    const size_t len = (size_t)(std::min((c.n_pos + 31) & ~31, ctx_stride) / 32) * tile16;
    if ((size_t)c.off16 > packed16 || len > packed16 - (size_t)c.off16) return 0;
    if (unpack && dst[c.slot]) return 0;
    dst[c.slot] = 1;
    ranges[i] = {(size_t)c.off16, (size_t)c.off16 + len};
    max_pos = std::max(max_pos, c.n_pos);
  }
  std::sort(ranges.begin(), ranges.end());
  for (int i = 1; i < n; i++)
    if (ranges[i].first < ranges[i - 1].second) return 0;
  const size_t n16 = (size_t)std::min((max_pos + 31) & ~31, ctx_stride) * head_dim / 8;
  return (unsigned)((n16 + 256 * U - 1) / (256 * U));
}

int launch_kv_pack(const _Float16* kc, const _Float16* vc, void* packed, size_t packed_bytes, const KvPack* tab,
                   const KvPack* tab_dev, int n, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                   int ctx_stride, size_t slot_stride, size_t layer_kv_stride, hipStream_t s) {
  constexpr int U = 4;
  const unsigned gx = kv_pack_check(kc, vc, packed, packed_bytes / 16, tab, tab_dev, n, n_layer, n_slots, n_head_kv,
                                    head_dim, n_ctx, ctx_stride, false, U);
  if (!gx) return -1;
  const dim3 grid(gx, (unsigned)(n_layer * n_head_kv * 2), (unsigned)n);
  kv_pack_kernel<U><<<grid, 256, 0, s>>>(kc, vc, reinterpret_cast<u32x4*>(packed), tab_dev, n_layer, n_head_kv,
                                         head_dim, ctx_stride, slot_stride, layer_kv_stride);
  return 0;
}

int launch_kv_unpack(_Float16* kc, _Float16* vc, const void* packed, size_t packed_bytes, const KvPack* tab,
                     const KvPack* tab_dev, int n, int n_layer, int n_slots, int n_head_kv, int head_dim, int n_ctx,
                     int ctx_stride, size_t slot_stride, size_t layer_kv_stride, hipStream_t s) {
  constexpr int U = 4;
  const unsigned gx = kv_pack_check(kc, vc, packed, packed_bytes / 16, tab, tab_dev, n, n_layer, n_slots, n_head_kv,
                                    head_dim, n_ctx, ctx_stride, true, U);
  if (!gx) return -1;
  const dim3 grid(gx, (unsigned)(n_layer * n_head_kv * 2), (unsigned)n);
  kv_unpack_kernel<U><<<grid, 256, 0, s>>>(kc, vc, reinterpret_cast<const u32x4*>(packed), tab_dev, n_layer,
                                           n_head_kv, head_dim, ctx_stride, slot_stride, layer_kv_stride);
  return 0;
}

}  // namespace mx
