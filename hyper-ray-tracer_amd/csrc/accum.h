/*
 * accum.h — the arithmetic of the sample accumulator (hrt_accum, include/hrt/hrt.h), the same code on the
 * device (render.hip accumulate_chunks / accum_merge / accum_resolve) and on the host (hrt_debug_accumulate
 * with on_device = 0), like hd_math.h and lane.h: built with -ffp-contract=off, f32 '/' and sqrt IEEE
 * correctly rounded on both sides, so the two give the same bits.
 *
 * The bits of an accumulated frame are defined by these functions alone:
 *   - a pass's sum of a pixel is its chunk sums added in chunk order starting from chunk 0's, which is what
 *     reduce_chunks adds up for hrt_render (pass_sum);
 *   - the accumulator takes the pass as ONE addend, acc + pass_sum, never chunk by chunk (add_pass);
 *   - a merge is dst + src (add_pass again);
 *   - the frame is sqrt(acc * (1 / samples)), reduce_chunks' expression (resolve_f32), and its 8-bit view is
 *     hrt_image_write's PPM rule on that value (quantize).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hrt/hd_math.h"

namespace hrt {
namespace accum {

/* A pass's sum of pixel i: partial is [n_chunks][n] records with the sum in .x .y .z (float4 on both sides). */
template <class F4>
HRT_HD Vec3 pass_sum(const F4* partial, uint32_t n_chunks, size_t n, size_t i) {
  const F4 a = partial[i];
  Vec3 sum = v3(a.x, a.y, a.z);
  for (uint32_t c = 1; c < n_chunks; c++) {
    const F4 b = partial[(size_t)c * n + i];
    sum = sum + v3(b.x, b.y, b.z);
  }
  return sum;
}

/* acc + sum: the pass (or the merged accumulator) is one addend */
HRT_HD Vec3 add_pass(Vec3 acc, Vec3 sum) { return acc + sum; }

/* 1 / samples, samples in [1, 2^32] */
HRT_HD float resolve_scale(uint64_t samples) { return 1.0f / (float)samples; }

/* the displayable pixel (application.rs:451-456: sqrt(sum / spp); alpha is 1) */
HRT_HD Vec3 resolve_f32(Vec3 acc, float scale) { return v3(sqrtf(acc.x * scale), sqrtf(acc.y * scale), sqrtf(acc.z * scale)); }

/* hrt_image_write's PPM rule (image_io.cpp): NaN -> 0, clamp to [0, 0.999], (u8)(256 v) */
HRT_HD uint8_t quantize(float v) {
  v = v != v ? 0.0f : (v < 0.0f ? 0.0f : (v > 0.999f ? 0.999f : v));
  return (uint8_t)(256.0f * v);
}

/* a resolved pixel as 4 x u8 in memory order r, g, b, 255 (one little-endian word) */
HRT_HD uint32_t resolve_rgba8(Vec3 px) {
  return (uint32_t)quantize(px.x) | ((uint32_t)quantize(px.y) << 8) | ((uint32_t)quantize(px.z) << 16) | 0xFF000000u;
}

}  // namespace accum
}  // namespace hrt
