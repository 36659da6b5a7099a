// grammar.hip -- the allowed-token mask of grammar-constrained sampling: the logit of every token
// a row's grammar state does not allow becomes -inf before the row's sampler reads it.
//
// A translation unit of its own, like lora.hip and kvpack.hip: kernels.hip's code object stays byte for byte what
// it was.
#include "device_common.h"

namespace mx {

// logits [M][ldl] f32 with V valid columns; masks [M][nw] (nw = ceil(V / 32); bit t & 31 of word t >> 5 set:
// token t is allowed); on [M]: 0 leaves the row alone, whatever its mask words hold.  One thread per 4 columns,
// so a wave covers 1 KiB of the row and 8 mask words.  The kernel never reads the row: a banned column gets -inf
// whatever it held (a NaN too), an allowed one is not touched, so its bits stay.  A group whose 4 columns are all
// banned is one 16-byte store (VEC: every row starts on a 16-byte boundary), a mixed group one 4-byte store per
// banned column; columns >= V count as allowed and are never written.
template <bool VEC>
__global__ __launch_bounds__(256) void grammar_mask_kernel(float* __restrict__ logits, int V, int ldl,
                                                           const uint32_t* __restrict__ masks, int nw,
                                                           const uint32_t* __restrict__ on) {
  const int row = blockIdx.y;
  if (!on[row]) return;
  const int g = blockIdx.x * 256 + threadIdx.x, c = g * 4;
  if (c >= V) return;
  uint32_t m = (masks[(size_t)row * nw + (g >> 3)] >> ((g & 7) * 4)) & 0xFu;
  if (V - c < 4) m |= (0xFu << (V - c)) & 0xFu;
  if (m == 0xFu) return;
  float* p = logits + (size_t)row * ldl + c;
  const float ninf = -__builtin_inff();
  if (VEC && m == 0u) {
    *reinterpret_cast<f32x4*>(p) = f32x4{ninf, ninf, ninf, ninf};
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!((m >> e) & 1u)) p[e] = ninf;
}

int launch_grammar_mask(float* logits, int ldl, int M, int V, const uint32_t* masks, const uint32_t* on,
                        hipStream_t s) {
  if (!logits || !masks || !on || M < 1 || M > MAX_ROWS || V < 1 || ldl < V) return -1;
  const int nw = (V + 31) / 32;
  const dim3 grid((unsigned)((V + 1023) / 1024), (unsigned)M);
  const bool vec = ldl % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  if (vec) grammar_mask_kernel<true><<<grid, 256, 0, s>>>(logits, V, ldl, masks, nw, on);
  else grammar_mask_kernel<false><<<grid, 256, 0, s>>>(logits, V, ldl, masks, nw, on);
  return 0;
}

}  // namespace mx
