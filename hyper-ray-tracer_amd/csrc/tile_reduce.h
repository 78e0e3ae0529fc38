/*
 * tile_reduce.h — the device side of accum.h's tile reduction, one copy for the kernels that reduce a tile's per-pixel
 * errors to its mean and max: accum_noise (accum.hip) and filter_err_reduce (filter.hip).  accum::tile_reduce is the
 * host's restatement; the fold order and the operand order of every step are the contract (accum.h).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "accum.h"

namespace hrt {
namespace accum {

/* One workgroup of NOISE_BLOCK threads.  (s, m) is thread j's fold of the values of pixels j, j + 256, ... in order
 * from (0, 0); sh_s and sh_m are NOISE_BLOCK floats of LDS each.  The halving tree x[j] = x[j] (op) x[j + st] for
 * st = 128 ... 1 runs through LDS across waves and through __shfl_down inside wave 0, lane j taking lane j + st's
 * value; thread 0 writes (x[0] * (1 / n), max).  Every thread of the workgroup calls it. */
__device__ __forceinline__ void tile_reduce_block(float s, float m, uint32_t n, float* sh_s, float* sh_m, float2* out) {
  const uint32_t j = threadIdx.x;
  sh_s[j] = s;
  sh_m[j] = m;
  __syncthreads();
  if (j < 128u) { /* st = 128, across waves */
    s = s + sh_s[j + 128u];
    m = larger(m, sh_m[j + 128u]);
  }
  __syncthreads();
  if (j < 128u) {
    sh_s[j] = s;
    sh_m[j] = m;
  }
  __syncthreads();
  if (j < 64u) { /* st = 64 across waves, then 32 ... 1 inside wave 0 */
    s = s + sh_s[j + 64u];
    m = larger(m, sh_m[j + 64u]);
    for (int off = 32; off >= 1; off >>= 1) {
      s = s + __shfl_down(s, off);
      m = larger(m, __shfl_down(m, off));
    }
    if (j == 0u) *out = make_float2(s * (1.0f / (float)n), m);
  }
}

}  // namespace accum
}  // namespace hrt
