/*
 * filter.h — the arithmetic of the a-trous preview filter, variance-guided (hrt_accum_resolve_filtered,
 * include/hrt/hrt.h) and feature-guided (hrt_accum_resolve_guided), the same code on the device (filter.hip) and on
 * the host (hrt_debug_filter / hrt_debug_guided with on_device = 0), like accum.h: built with -ffp-contract=off, f32
 * '/' and sqrtf IEEE correctly rounded on both sides, so the two give the same bits.
 *
 * The bits of a filtered frame are defined by these functions alone.
 *   Domain: the pixels the accumulator's tiles cover.  A neighbour off the image or covered by no tile is ABSENT and
 *   contributes to no sum.  On a raster plane a pixel is (c.x, c.y, c.z, v) and an absent one has v < 0.
 *   Inputs of pixel p, with inv_n and inv_k1 of p's tile (gather):
 *     c_p = (acc.x * inv_n, acc.y * inv_n, acc.z * inv_n), the linear radiance;
 *     v_p = accum::variance(m2_p, accum::luma(acc_p), inv_n, inv_k1) * inv_n, the variance of the mean;
 *     l_p = accum::luma(c_p), recomputed from c wherever it is used.
 *   Iteration i = 0 .. iterations - 1 with step s = 1 << i reads the planes (c, v) of the previous one, never in
 *   place (atrous_pixel):
 *     1. num = den = 0; for dy = -1..1 (outer), dx = -1..1 (inner) over present q = p + (dx, dy):
 *        g = G[dy + 1] * G[dx + 1], G = {1, 2, 1}; num = num + g * v_q, then den = den + g; vb = num / den.
 *     2. r = 1 / (sigma * sqrtf(vb) + 1e-6f).
 *     3. sc = (0, 0, 0), sv = sw = 0; for dy = -2..2 (outer), dx = -2..2 (inner) over present q = p + s * (dx, dy),
 *        the centre at its place in the order: d = fabsf(l_q - l_p) * r; t = at_least(1 - d * 0.5f, 0); e = t * t,
 *        e = e * e; w = (H[dy + 2] * H[dx + 2]) * e, H = {1/16, 1/4, 3/8, 1/4, 1/16};
 *        sc = sc + w * c_q per channel, sv = sv + (w * w) * v_q, sw = sw + w.
 *     4. c' = sc / sw per channel, v' = sv / (sw * sw); sw == 0 (only reachable through NaN): c' = c_p, v' = v_p.
 *   Output: sqrtf(c'.x), sqrtf(c'.y), sqrtf(c'.z), 1 (resolve), or accum::resolve_rgba8 of that.
 * The weight is a polynomial, (1 - d/2)^4 clamped at 0, because it has one form on host and device; an expf has not.
 *
 * The bits of a GUIDED frame (hrt_accum_resolve_guided; hrt_debug_guided): exactly this iteration (the same domain,
 * absent pixels, prefiltered variance, r, tap order, H, sv and sw), with further edge-stopping terms on the mean feature
 * planes (feature_pass.h mean_albedo, mean_normal) of pixel p and tap q.  After the luminance term e = (t * t)^2 of a tap
 * the ENABLED terms follow in this order (k_f = 1.0f / tolerance_f, computed once on the host; k_f == 0: the term is off
 * and is SKIPPED, not multiplied by one, so with all three off the frame is hrt_accum_resolve_filtered's bit for bit):
 *   normal: d = ((dx * dx + dy * dy) + dz * dz) of n_q - n_p; t = at_least(1.0f - d * k_n, 0); e = e * (t * t);
 *   albedo: the same on a_q - a_p with k_a;
 *   depth:  d = fabsf(z_q - z_p) / ((z_q + z_p) + 1e-6f); t = at_least(1.0f - d * k_z, 0); e = e * (t * t).
 * These weights are polynomials for the same reason.  The feature planes are constant across iterations; only (c, v)
 * ping-pongs.  Both filters are ONE function, atrous_pixel: the plain one is the guided one whose per-tap hook adds no
 * term.
 *
 * The bits of a DEMODULATED guided frame (hrt_accum_resolve_guided_ex with HRT_GUIDED_DEMODULATE; hrt_debug_guided_ex):
 * the filter runs on the radiance divided by the first-hit albedo, so that it averages irradiance across texture edges,
 * and the texture is multiplied back at full sharpness.  With a_p the xyz of pixel p's mean albedo (the bits
 * hrt_accum_features returns) and `floor` the caller's albedo floor (> 0):
 *   1. m_p = (at_least(a_p.x, floor), at_least(a_p.y, floor), at_least(a_p.z, floor)) (demod_divisor); a NaN albedo
 *      gives floor.
 *   2. The input of a present pixel replaces gather's (demodulate): d_p = (c_p.x / m_p.x, c_p.y / m_p.y, c_p.z / m_p.z);
 *      l = luma(c_p), l' = luma(d_p), g = l > 0 ? l' / l : 0.0f; v'_p = v_p * (g * g), which keeps the relative standard
 *      error of the luminance and is exact for a grey albedo.  Absent pixels stay absent, as they are.
 *   3. The iterations are exactly the ones above on the planes (d, v'), the feature terms reading the same mean planes.
 *   4. The last iteration's d' is remodulated (remodulate): c'' = (d'.x * m_p.x, d'.y * m_p.y, d'.z * m_p.z), then the
 *      output rule above on c''; the sw == 0 escape's pixel is remodulated like any other.  v' stays in demodulated
 *      units.
 * Without the flag none of this runs and floor is not read: the frame is the guided one bit for bit.
 *
 * The bits of the FILTERED NOISE ESTIMATE (hrt_accum_noise_filtered; hrt_debug_noise_filtered): the relative standard
 * error of the filtered frame's pixel as the filter itself propagates it.  With (c', v') pixel p's output of the LAST
 * iteration of any of the three filters above, the sw == 0 escape's pixel included, and `floor` the caller's (> 0):
 *   plain and guided (filtered_err): l' = luma(c'); err = sqrtf(v') / at_least(l', floor);
 *   demodulated (filtered_err_demod), the last iteration giving d' and v' in demodulated units: c'' = remodulate(d', m_p),
 *     l_d = luma(d'), l'' = luma(c''), gr = l_d > 0 ? l'' / l_d : 0.0f, v'' = v' * (gr * gr), then filtered_err of
 *     (c'', v''): the mirror of demodulate's step 2.
 * The last iteration writes err, packed, where a frame pixel would have gone (FORMAT_ERR); the frame is never written.
 * A tile's mean and max are accum::tile_reduce of its packed errs, the reduction of hrt_accum_noise.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "accum.h"

namespace hrt {
namespace filter {

constexpr uint32_t MAX_ITERATIONS = 5;

/* one pixel of a raster plane; v < 0: absent */
struct Px {
  Vec3 c;
  float v;
};
HRT_HD Px px(float x, float y, float z, float v) {
  Px p;
  p.c = v3(x, y, z);
  p.v = v;
  return p;
}
HRT_HD Px absent() { return px(0.0f, 0.0f, 0.0f, -1.0f); }
HRT_HD bool present(const Px& p) { return !(p.v < 0.0f); }

/* the plane's pixel from the accumulator's sums and moment */
HRT_HD Px gather(Vec3 acc, float m2, float inv_n, float inv_k1) {
  Px p;
  p.c = v3(acc.x * inv_n, acc.y * inv_n, acc.z * inv_n);
  p.v = accum::variance(m2, accum::luma(acc), inv_n, inv_k1) * inv_n;
  return p;
}

/* demodulation by the first-hit albedo a (the mean albedo plane's xyz): the divisor, the filter's input pixel in place
 * of gather's, and the last iteration's colour back in radiance */
HRT_HD Vec3 demod_divisor(Vec3 a, float floor) {
  return v3(accum::at_least(a.x, floor), accum::at_least(a.y, floor), accum::at_least(a.z, floor));
}
HRT_HD Px demodulate(const Px& p, Vec3 m) {
  Px d;
  d.c = v3(p.c.x / m.x, p.c.y / m.y, p.c.z / m.z);
  const float l = accum::luma(p.c), ld = accum::luma(d.c);
  const float g = l > 0.0f ? ld / l : 0.0f;
  d.v = p.v * (g * g);
  return d;
}
HRT_HD Vec3 remodulate(Vec3 d, Vec3 m) { return v3(d.x * m.x, d.y * m.y, d.z * m.z); }
/* the filtered noise estimate of a last iteration's pixel; the demodulated form takes the pixel before remodulation */
HRT_HD float filtered_err(Vec3 c, float v, float floor) { return sqrtf(v) / accum::at_least(accum::luma(c), floor); }
HRT_HD float filtered_err_demod(Vec3 d, float v, Vec3 m, float floor) {
  const Vec3 c = remodulate(d, m);
  const float ld = accum::luma(d), l = accum::luma(c);
  const float gr = ld > 0.0f ? l / ld : 0.0f;
  return filtered_err(c, v * (gr * gr), floor);
}
/* the option of a guided resolve: off, or on with the caller's albedo floor (> 0; not read when off) */
struct Demod {
  bool on;
  float floor;
};

HRT_HD float g_tap(int k) { return k == 1 ? 2.0f : 1.0f; }
HRT_HD float h_tap(int k) { return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f); }

/* the features of one raster pixel: the albedo plane's xyz, the normal plane's xyz and w */
struct Feat {
  Vec3 a, n;
  float z;
};
/* 1 / tolerance per term; 0: the term is off */
struct Terms {
  float kn, ka, kz;
};

HRT_HD float sq_dist(Vec3 q, Vec3 p) {
  const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
  return (dx * dx + dy * dy) + dz * dz;
}
/* the feature terms of tap q at pixel p onto the luminance weight e */
HRT_HD float feature_weight(float e, const Feat& q, const Feat& p, const Terms& K) {
  if (K.kn > 0.0f) {
    const float t = accum::at_least(1.0f - sq_dist(q.n, p.n) * K.kn, 0.0f);
    e = e * (t * t);
  }
  if (K.ka > 0.0f) {
    const float t = accum::at_least(1.0f - sq_dist(q.a, p.a) * K.ka, 0.0f);
    e = e * (t * t);
  }
  if (K.kz > 0.0f) {
    const float d = fabsf(q.z - p.z) / ((q.z + p.z) + 1e-6f);
    const float t = accum::at_least(1.0f - d * K.kz, 0.0f);
    e = e * (t * t);
  }
  return e;
}

/* atrous_pixel's per-tap hook: the luminance weight e of the tap at (qx, qy) -> the tap's weight.  The plain filter's
 * adds no term; the guided filter's applies feature_weight, feat(x, y) being the features of a PRESENT pixel. */
struct NoFeatures {
  HRT_HD float operator()(float e, int, int) const { return e; }
};
template <class FeatAt>
struct FeatureTerms {
  FeatAt feat;
  Feat fp;
  Terms K;
  HRT_HD float operator()(float e, int qx, int qy) const { return feature_weight(e, feat(qx, qy), fp, K); }
};
template <class FeatAt>
HRT_HD FeatureTerms<FeatAt> feature_terms(FeatAt feat, int x, int y, const Terms& K) {
  return FeatureTerms<FeatAt>{feat, feat(x, y), K};
}

/* One iteration at the PRESENT pixel (x, y) with step s.  at(x, y) gives the previous planes' pixel, absent() for a
 * pixel off the image. */
template <class At, class Weight>
HRT_HD Px atrous_pixel(At at, Weight weight, int x, int y, int s, float sigma) {
  const Px p = at(x, y);
  const float lp = accum::luma(p.c);
  float num = 0.0f, den = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const Px q = at(x + dx, y + dy);
      if (!present(q)) continue;
      const float g = g_tap(dy + 1) * g_tap(dx + 1);
      num = num + g * q.v;
      den = den + g;
    }
  const float vb = num / den;
  const float r = 1.0f / (sigma * sqrtf(vb) + 1e-6f);
  Vec3 sc = v3(0.0f, 0.0f, 0.0f);
  float sv = 0.0f, sw = 0.0f;
  for (int dy = -2; dy <= 2; dy++)
    for (int dx = -2; dx <= 2; dx++) {
      const Px q = at(x + s * dx, y + s * dy);
      if (!present(q)) continue;
      const float d = fabsf(accum::luma(q.c) - lp) * r;
      const float t = accum::at_least(1.0f - d * 0.5f, 0.0f);
      float e = t * t;
      e = e * e;
      e = weight(e, x + s * dx, y + s * dy);
      const float w = (h_tap(dy + 2) * h_tap(dx + 2)) * e;
      sc = sc + w * q.c;
      sv = sv + (w * w) * q.v;
      sw = sw + w;
    }
  if (sw == 0.0f) return p;
  Px o;
  o.c = sc / sw;
  o.v = sv / (sw * sw);
  return o;
}

/* the displayable pixel of a filtered one (alpha is 1) */
HRT_HD Vec3 resolve(const Px& p) { return v3(sqrtf(p.c.x), sqrtf(p.c.y), sqrtf(p.c.z)); }

/* The host's restatement of a whole raster: in and out are width x height x 4 f32 (c.xyz, v); absent pixels pass
 * through as they are.  albedo and normal: the two feature rasters (a.xyz, -) and (n.xyz, z) of the guided filter, read
 * at present pixels only, or both null: the plain filter (K is not read).  demod.on (the guided filter only): `in` is
 * gather's (c, v); its present pixels are demodulated before the first iteration and the last one's colour is
 * remodulated, so out is (c''.xyz, v' in demodulated units).  err (or null): width x height f32, the filtered noise
 * estimate of every present pixel against err_floor, 0 at an absent one. */
inline void filter_raster(const float* in, const float* albedo, const float* normal, uint32_t width, uint32_t height,
                          uint32_t iterations, float sigma, const Terms& K, const Demod& demod, float* out, float* err = nullptr,
                          float err_floor = 0.0f) {
  const size_t n = (size_t)width * height;
  std::vector<float> a(in, in + 4 * n), b(4 * n);
  auto divisor = [=](size_t k) { return demod_divisor(v3(albedo[k], albedo[k + 1], albedo[k + 2]), demod.floor); };
  if (demod.on)
    for (size_t k = 0; k < 4 * n; k += 4) {
      const Px p = px(a[k], a[k + 1], a[k + 2], a[k + 3]);
      if (!present(p)) continue;
      const Px d = demodulate(p, divisor(k));
      a[k] = d.c.x, a[k + 1] = d.c.y, a[k + 2] = d.c.z, a[k + 3] = d.v;
    }
  auto feat = [=](int x, int y) {
    const size_t k = 4 * ((size_t)y * width + (size_t)x);
    Feat f;
    f.a = v3(albedo[k], albedo[k + 1], albedo[k + 2]);
    f.n = v3(normal[k], normal[k + 1], normal[k + 2]);
    f.z = normal[k + 3];
    return f;
  };
  for (uint32_t i = 0; i < iterations; i++) {
    const float* src = a.data();
    auto at = [=](int x, int y) {
      if (x < 0 || y < 0 || x >= (int)width || y >= (int)height) return absent();
      const float* q = src + 4 * ((size_t)y * width + (size_t)x);
      return px(q[0], q[1], q[2], q[3]);
    };
    for (uint32_t y = 0; y < height; y++)
      for (uint32_t x = 0; x < width; x++) {
        const int s = 1 << i, ix = (int)x, iy = (int)y;
        Px o = at(ix, iy);
        if (present(o))
          o = albedo ? atrous_pixel(at, feature_terms(feat, ix, iy, K), ix, iy, s, sigma) : atrous_pixel(at, NoFeatures{}, ix, iy, s, sigma);
        float* d = b.data() + 4 * ((size_t)y * width + x);
        d[0] = o.c.x, d[1] = o.c.y, d[2] = o.c.z, d[3] = o.v;
      }
    a.swap(b);
  }
  if (err)
    for (size_t k = 0; k < 4 * n; k += 4) {
      const Vec3 c = v3(a[k], a[k + 1], a[k + 2]);
      if (!present(px(c.x, c.y, c.z, a[k + 3]))) err[k / 4] = 0.0f;
      else err[k / 4] = demod.on ? filtered_err_demod(c, a[k + 3], divisor(k), err_floor) : filtered_err(c, a[k + 3], err_floor);
    }
  if (demod.on)
    for (size_t k = 0; k < 4 * n; k += 4) {
      if (!present(px(a[k], a[k + 1], a[k + 2], a[k + 3]))) continue;
      const Vec3 c = remodulate(v3(a[k], a[k + 1], a[k + 2]), divisor(k));
      a[k] = c.x, a[k + 1] = c.y, a[k + 2] = c.z;
    }
  for (size_t k = 0; k < 4 * n; k++) out[k] = a[k];
}

/* ---- the launches of filter.hip, for the accumulator code in accum.hip (streams are hipStream_t) ---- */

/* One tile as filter_gather and the last filter_atrous see it.  The tile-block domain: a tile is cut into
 * BLOCK_W x BLOCK_H pixel blocks, row-major, and the tiles' blocks are numbered in tile order starting at blk0. */
constexpr uint32_t BLOCK_W = 32, BLOCK_H = 8;
struct alignas(16) FilterTile {
  uint32_t x, y, w, h; /* in plane coordinates: the image's minus the bounding box's corner */
  uint32_t off;        /* first pixel in the packed order */
  uint32_t blk0;       /* first block of the tile-block domain */
  float inv_n;         /* accum::resolve_scale(samples) */
  float inv_k1;        /* accum::chunks_scale(chunks) */
};
inline uint32_t tile_blocks(uint32_t w, uint32_t h) { return ((w + BLOCK_W - 1) / BLOCK_W) * ((h + BLOCK_H - 1) / BLOCK_H); }

/* format of the last iteration's packed output: HRT_ACCUM_F32, HRT_ACCUM_RGBA8, RAW: float4 (c', v'), or ERR: one f32,
 * the filtered noise estimate against launch_atrous' err_floor */
constexpr int32_t FORMAT_RAW = -1, FORMAT_ERR = -3;

/* acc, m2 (packed) -> plane (plane_w x plane_h float4) at the tiles' pixels */
void launch_gather(const void* d_acc, const float* d_m2, const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                   void* d_plane, uint32_t plane_w, void* stream);
/* launch_gather with the pixel demodulated by the mean albedo of the packed feature sums d_fa (inv = 1 / feature
 * samples): the same pass over the packed sums */
void launch_gather_demod(const void* d_acc, const float* d_m2, const void* d_fa, float inv, float floor, const FilterTile* d_tiles,
                         uint32_t n_tiles, uint32_t n_blocks, void* d_plane, uint32_t plane_w, void* stream);
/* the present pixels of a raster plane of n pixels that holds gather's (c, v), demodulated in place by the albedo raster
 * (hrt_debug_guided_ex; an accumulator's plane is demodulated where it is gathered) */
void launch_demodulate(void* d_plane, const void* d_albedo, size_t n, float floor, void* stream);
/* the packed feature sums (fa, fn) -> the two mean rasters (plane_w wide) at the tiles' pixels; inv = 1 / feature samples */
void launch_gather_features(const void* d_fa, const void* d_fn, const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                            float inv, void* d_albedo, void* d_normal, uint32_t plane_w, void* stream);
/* `iterations` of the filter from plane a (b is the other plane; both are written), the last one to d_out packed.
 * d_albedo and d_normal: the guided filter's feature rasters, or both null: the plain filter (K is not read).
 * demod.on (the guided filter only): plane a is demodulated, and the last iteration remodulates what it writes.
 * err_floor is read for FORMAT_ERR alone. */
void launch_atrous(void* d_a, void* d_b, const void* d_albedo, const void* d_normal, uint32_t plane_w, uint32_t plane_h,
                   const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks, uint32_t iterations, float sigma, const Terms& K,
                   const Demod& demod, int32_t format, void* d_out, void* stream, float err_floor = 0.0f);
/* the packed errs of every tile reduced to its (mean, max): accum.h tile_reduce, one workgroup per tile */
void launch_err_reduce(const float* d_err, const FilterTile* d_tiles, uint32_t n_tiles, void* d_mean_max, void* stream);

}  // namespace filter
}  // namespace hrt
