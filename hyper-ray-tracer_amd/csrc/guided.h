/*
 * guided.h — the arithmetic of the feature-guided a-trous filter (hrt_accum_resolve_guided, include/hrt/hrt.h), the
 * same code on the device (guided.hip) and on the host (hrt_debug_guided with on_device = 0), like filter.h: built
 * with -ffp-contract=off, so the two give the same bits.
 *
 * The bits of a guided frame: exactly filter.h's iteration (the same domain, absent pixels, prefiltered variance, r,
 * tap order, H, sv and sw), with further edge-stopping terms on the mean feature planes (feature_pass.h mean_albedo,
 * mean_normal) of pixel p and tap q.  After the luminance term e = (t * t)^2 of a tap the ENABLED terms follow in
 * this order (k_f = 1.0f / tolerance_f, computed once on the host; k_f == 0: the term is off and is SKIPPED, not
 * multiplied by one, so with all three off the frame is hrt_accum_resolve_filtered's bit for bit):
 *   normal: d = ((dx * dx + dy * dy) + dz * dz) of n_q - n_p; t = at_least(1.0f - d * k_n, 0); e = e * (t * t);
 *   albedo: the same on a_q - a_p with k_a;
 *   depth:  d = fabsf(z_q - z_p) / ((z_q + z_p) + 1e-6f); t = at_least(1.0f - d * k_z, 0); e = e * (t * t).
 * The weights are polynomials for filter.h's reason: one form on host and device.  The feature planes are constant
 * across iterations; only (c, v) ping-pongs.
 */
#pragma once
#include "filter.h"

namespace hrt {
namespace guided {

using filter::Px;

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

/* filter::atrous_pixel with the feature terms: at(x, y) gives the previous planes' pixel (absent() off the image),
 * feat(x, y) the features of a PRESENT pixel */
template <class At, class FeatAt>
HRT_HD Px guided_pixel(At at, FeatAt feat, int x, int y, int s, float sigma, const Terms& K) {
  const Px p = at(x, y);
  const Feat fp = feat(x, y);
  const float lp = accum::luma(p.c);
  float num = 0.0f, den = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const Px q = at(x + dx, y + dy);
      if (!filter::present(q)) continue;
      const float g = filter::g_tap(dy + 1) * filter::g_tap(dx + 1);
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
      if (!filter::present(q)) continue;
      const float d = fabsf(accum::luma(q.c) - lp) * r;
      const float t = accum::at_least(1.0f - d * 0.5f, 0.0f);
      float e = t * t;
      e = e * e;
      e = feature_weight(e, feat(x + s * dx, y + s * dy), fp, K);
      const float w = (filter::h_tap(dy + 2) * filter::h_tap(dx + 2)) * e;
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

/* The host's restatement of a whole raster, as filter::filter_raster: in and out are width x height x 4 f32 (c.xyz, v),
 * albedo and normal the two feature rasters (a.xyz, -) and (n.xyz, z), read at present pixels only. */
inline void guided_raster(const float* in, const float* albedo, const float* normal, uint32_t width, uint32_t height,
                          uint32_t iterations, float sigma, const Terms& K, float* out) {
  const size_t n = (size_t)width * height;
  std::vector<float> a(in, in + 4 * n), b(4 * n);
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
      if (x < 0 || y < 0 || x >= (int)width || y >= (int)height) return filter::absent();
      const float* q = src + 4 * ((size_t)y * width + (size_t)x);
      return filter::px(q[0], q[1], q[2], q[3]);
    };
    for (uint32_t y = 0; y < height; y++)
      for (uint32_t x = 0; x < width; x++) {
        const Px p = at((int)x, (int)y);
        const Px o = filter::present(p) ? guided_pixel(at, feat, (int)x, (int)y, 1 << i, sigma, K) : p;
        float* d = b.data() + 4 * ((size_t)y * width + x);
        d[0] = o.c.x, d[1] = o.c.y, d[2] = o.c.z, d[3] = o.v;
      }
    a.swap(b);
  }
  for (size_t k = 0; k < 4 * n; k++) out[k] = a[k];
}

/* ---- the launches of guided.hip, for accum.hip (streams are hipStream_t) ---- */

/* the steps whose feature planes are staged in LDS beside the colour plane: every step the colour plane is staged for
 * (step 4: 55 KB per block, and still the fastest); larger ones read everything from global memory */
constexpr uint32_t FEATURE_LDS_MAX_STEP = 4;

/* the packed feature sums (fa, fn) -> the two mean rasters (plane_w wide) at the tiles' pixels; inv = 1 / feature samples */
void launch_gather_features(const void* d_fa, const void* d_fn, const filter::FilterTile* d_tiles, uint32_t n_tiles,
                            uint32_t n_blocks, float inv, void* d_albedo, void* d_normal, uint32_t plane_w, void* stream);
/* filter::launch_atrous with the feature rasters */
void launch_guided(void* d_a, void* d_b, const void* d_albedo, const void* d_normal, uint32_t plane_w, uint32_t plane_h,
                   const filter::FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks, uint32_t iterations, float sigma,
                   const Terms& K, int32_t format, void* d_out, void* stream);

}  // namespace guided
}  // namespace hrt
