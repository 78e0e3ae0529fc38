/*
 * accum.h — the arithmetic of the sample accumulator (hrt_accum, include/hrt/hrt.h), the same code on the
 * device (accum.hip accumulate_chunks / accum_merge / accum_resolve) and on the host (hrt_debug_accumulate
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

/* A pass's sum of pixel i: partial is [n_chunks][n] records with the sum in .x .y .z (float4 on both sides), a pointer
 * or anything indexed like one (accum_paths.h PathChunks, which makes each chunk sum when it is asked for). */
template <class Partial>
HRT_HD Vec3 pass_sum(const Partial& partial, uint32_t n_chunks, size_t n, size_t i) {
  const auto a = partial[i];
  Vec3 sum = v3(a.x, a.y, a.z);
  for (uint32_t c = 1; c < n_chunks; c++) {
    const auto b = partial[(size_t)c * n + i];
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

/* ---- the noise estimate (hrt_accum_noise; HRT_ACCUM_NOISE accumulators keep a second plane, m2, f32 per pixel).
 *
 * The bits of the noise plane and of the error are defined by these functions alone:
 *   - a sum's value is luma(s) = (s.x + s.y) + s.z; call a chunk sum's value Y_c and its sample count n_c (the count
 *     comes from lane.h chunk_range, the function the kernels split a pixel's samples by);
 *   - a chunk's term is (Y_c * Y_c) * (1.0f / (float)n_c) (chunk_term);
 *   - a pass's moment is its chunk terms added in chunk order starting from chunk 0's (pass_moment), and the plane
 *     takes it as ONE addend, m2 + pass_moment, as the sums take pass_sum (add_moment); a merge is dst.m2 + src.m2;
 *   - with N samples and K chunks held and Y = luma(acc): var = max((m2 - (Y * Y) * (1 / N)) * (1 / (K - 1)), 0)
 *     (variance) and err = sqrtf(var * (1 / N)) / max(Y * (1 / N), floor) (noise_err); K < 2 gives +inf.
 * This is the weighted batch-means estimator: E[sum_c Y_c^2 / n_c - Y^2 / N] = (K - 1) sigma^2 for batches of
 * unequal sizes, so var estimates the variance of ONE sample's value and err is the relative standard error of the
 * pixel's mean, with means below `floor` measured against the floor.
 * Rounding floor: m2 and (Y * Y) / N are two nearly equal f32 numbers on a converged pixel, so their difference
 * carries an absolute error of a few ulps of m2.  Against an f64 evaluation of the same chunk sums (64x36 `random`
 * at 126 spp in 3 passes, 32x32 `cornell` at 110 in 2) the f32 err differs by at most 1.3e-4 absolute, reached on
 * sky pixels whose true error is ~1e-9, and by at most 2.5e-4 relative wherever err > 1e-3; m2 itself agrees to
 * 2.2e-7 relative.  An err below ~2e-4 is therefore "converged", not a measurement. */
HRT_HD float luma(Vec3 s) { return (s.x + s.y) + s.z; }

HRT_HD float chunk_term(float y, uint32_t n_c) { return (y * y) * (1.0f / (float)n_c); }

/* A pass's moment of pixel i: partial as for pass_sum, count_of(c) = the samples of chunk c. */
template <class Partial, class CountOf>
HRT_HD float pass_moment(const Partial& partial, uint32_t n_chunks, size_t n, size_t i, CountOf count_of) {
  const auto a = partial[i];
  float m = chunk_term(luma(v3(a.x, a.y, a.z)), count_of(0u));
  for (uint32_t c = 1; c < n_chunks; c++) {
    const auto b = partial[(size_t)c * n + i];
    m = m + chunk_term(luma(v3(b.x, b.y, b.z)), count_of(c));
  }
  return m;
}

/* m2 + moment: the pass (or the merged plane) is one addend */
HRT_HD float add_moment(float m2, float moment) { return m2 + moment; }

/* 1 / (K - 1), K >= 2 chunks */
HRT_HD float chunks_scale(uint64_t chunks) { return 1.0f / (float)(chunks - 1u); }

/* x > lo ? x : lo, so a NaN x gives lo */
HRT_HD float at_least(float x, float lo) { return x > lo ? x : lo; }

/* inv_n = resolve_scale(N), inv_k1 = chunks_scale(K) */
HRT_HD float variance(float m2, float y, float inv_n, float inv_k1) { return at_least((m2 - (y * y) * inv_n) * inv_k1, 0.0f); }

/* few: K < 2, no estimate: +inf */
HRT_HD float noise_err(Vec3 acc, float m2, float inv_n, float inv_k1, bool few, float floor) {
  if (few) return __builtin_inff();
  const float y = luma(acc);
  return sqrtf(variance(m2, y, inv_n, inv_k1) * inv_n) / at_least(y * inv_n, floor);
}

/* The tile reduction of accum_noise, one workgroup of NOISE_BLOCK threads per tile: thread j folds the values of
 * pixels j, j + 256, ... of the tile's packed order, in order, into x[j] starting from 0 (an err is
 * never negative); then the halving tree x[j] = x[j] (op) x[j + s] for s = 128 ... 1.  The kernel runs the tree through LDS
 * across waves and through __shfl_down within a wave with the same operand order; tile_reduce is the host's
 * restatement, so the two agree bit for bit.  mean = x[0] * (1 / n). */
constexpr uint32_t NOISE_BLOCK = 256;
HRT_HD float larger(float a, float b) { return b > a ? b : a; }
inline void tile_reduce(const float* err, uint32_t n, float& mean, float& max) {
  float xs[NOISE_BLOCK], xm[NOISE_BLOCK];
  for (uint32_t j = 0; j < NOISE_BLOCK; j++) {
    float s = 0.0f, m = 0.0f;
    for (uint32_t k = j; k < n; k += NOISE_BLOCK) {
      s = s + err[k];
      m = larger(m, err[k]);
    }
    xs[j] = s;
    xm[j] = m;
  }
  for (uint32_t s = NOISE_BLOCK / 2; s >= 1; s >>= 1)
    for (uint32_t j = 0; j < s; j++) {
      xs[j] = xs[j] + xs[j + s];
      xm[j] = larger(xm[j], xm[j + s]);
    }
  mean = xs[0] * (1.0f / (float)n);
  max = xm[0];
}

}  // namespace accum
}  // namespace hrt
