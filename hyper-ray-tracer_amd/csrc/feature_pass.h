/*
 * feature_pass.h — the first-hit features of one sample (hrt_accum_add_features, include/hrt/hrt.h), per-lane code like
 * lane.h: the same functions on the device (feature_pass.hip feature_kernel) and on the host (tests/native/feature_sim.hip),
 * built with -ffp-contract=off.
 *
 * first_hit_features does, for sample `sample` of pixel (px, py):
 *   1. start_sample: the draws a radiance sample of that index makes, so the features are the first hits of exactly
 *      the paths the accumulator renders;
 *   2. trace<CULL, FULL, FULL, false, false> over the reference node stream (0 .. P.main_end, t_min, +inf), which is
 *      what segment() does for ps.pk.segment == 0 (a ConstantMedium draws from its own keyed sub-stream);
 *   3. on a hit, make_record<FULL> and the material's record.
 * The four values:
 *   hit     1.0f on a hit, 0.0f on a miss;
 *   albedo  Lambertian / Isotropic: the texture value at the hit (tex_value); Metal: its albedo; Dielectric: (1, 1, 1);
 *           DiffuseLight: the emit texture's value, unclamped; a miss: P.background;
 *   normal  rec.n in world space, which faces the ray; (0, 0, 0) for a medium hit and for a miss;
 *   depth   closest * sqrtf(dot(rd, rd)) on a hit, 0 on a miss.
 * It makes no RNG draw beyond start_sample and the medium's sub-stream, and writes nothing.
 *
 * A pass sums its samples in index order into fa = (albedo.xyz, hit) and fn = (normal.xyz, depth), each from 0.0f
 * (add_sample), and the planes take the pass sum as one addend (add_pass).  The mean planes (mean_albedo,
 * mean_normal) are what hrt_accum_features returns and what the guided filter reads.
 */
#pragma once
#include "lane.h"

namespace hrt {
namespace features {

using namespace hrt::lane;

struct Features {
  float hit;
  Vec3 albedo, normal;
  float depth;
  uint32_t mat; /* the hit's material, G::NONE on a miss: for tests/native/feature_sim.hip (no kernel reads it) */
};

template <int CULL, bool FULL>
HRT_LANE Features first_hit_features(const KParams& P, const G::Node* __restrict__ nodes, const G::Prim* __restrict__ prims,
                                     uint32_t px, uint32_t py, uint32_t sample) {
  PathState ps;
  Counts cn{0u, 0u, 0u, 0u, 0u, 0u};
  start_sample(P, ps, px, py, sample);
  float closest = u2f(0x7f800000u);
  uint32_t winner = G::NONE;
  trace<CULL, FULL, FULL, false, false>(P, nodes, prims, 0u, P.main_end, ps.ro, ps.rd, ps.rtime, P.t_min, closest, winner, ps.pk, cn);
  Features f;
  if (winner == G::NONE) {
    f.hit = 0.0f;
    f.albedo = P.background;
    f.normal = v3(0.0f, 0.0f, 0.0f);
    f.depth = 0.0f;
    f.mat = G::NONE;
    return f;
  }
  const float tau = P.motion_uniform ? (ps.rtime - P.motion_t0) / P.motion_span : 0.0f;
  const Rec rec = make_record<FULL>(P, winner, closest, ps.ro, ps.rd, ps.rtime, tau);
  const G::Mat M = P.mats[rec.mat];
  f.hit = 1.0f;
  f.mat = rec.mat;
  if (M.kind == G::M_METAL) f.albedo = v3(M.a[0], M.a[1], M.a[2]);
  else if (M.kind == G::M_DIELECTRIC) f.albedo = v3(1.0f, 1.0f, 1.0f);
  else f.albedo = tex_value<FULL, false>(P, M.tex, rec.u, rec.v, rec.p, cn); /* Lambertian, Isotropic, DiffuseLight */
  f.normal = rec.n;
  f.depth = closest * sqrtf(dot(ps.rd, ps.rd));
  return f;
}

/* the two sums of a pass, or of the planes: fa = (albedo.xyz, hit), fn = (normal.xyz, depth) */
struct Sums {
  float4 fa, fn;
};
HRT_LANE_FI Sums zero_sums() {
  Sums s;
  s.fa = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  s.fn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return s;
}
HRT_LANE_FI float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
HRT_LANE_FI Sums add_sample(Sums s, const Features& f) {
  s.fa = add4(s.fa, make_float4(f.albedo.x, f.albedo.y, f.albedo.z, f.hit));
  s.fn = add4(s.fn, make_float4(f.normal.x, f.normal.y, f.normal.z, f.depth));
  return s;
}
/* samples [0, n) of the pass (P.sample_offset is the pass's first sample), in index order */
template <int CULL, bool FULL>
HRT_LANE Sums pass_sums(const KParams& P, const G::Node* __restrict__ nodes, const G::Prim* __restrict__ prims, uint32_t px,
                        uint32_t py, uint32_t n) {
  Sums s = zero_sums();
  for (uint32_t k = 0; k < n; k++) s = add_sample(s, first_hit_features<CULL, FULL>(P, nodes, prims, px, py, k));
  return s;
}
/* plane = plane + pass_sum */
HRT_LANE_FI Sums add_pass(Sums plane, const Sums& pass) {
  plane.fa = add4(plane.fa, pass.fa);
  plane.fn = add4(plane.fn, pass.fn);
  return plane;
}

/* the mean planes of nf feature samples: inv = 1.0f / (float)nf */
HRT_LANE_FI float4 mean_albedo(float4 fa, float inv) { return make_float4(fa.x * inv, fa.y * inv, fa.z * inv, fa.w * inv); }
HRT_LANE_FI float4 mean_normal(float4 fa, float4 fn, float inv) {
  const float z = fa.w > 0.0f ? fn.w * (1.0f / fa.w) : 0.0f;
  return make_float4(fn.x * inv, fn.y * inv, fn.z * inv, z);
}

/* ---- the launches of feature_pass.hip, for accum.hip (streams are hipStream_t) ---- */

/* One tile as feature_kernel sees it.  The tile-block domain (as filter.h's): a tile is cut into pixel blocks of
 * 64 pixels, row-major, one wave each, and the tiles' blocks are numbered in tile order starting at blk0. */
struct alignas(16) FeatureTile {
  uint32_t x, y, w, h; /* in image coordinates */
  uint32_t off;        /* first pixel in the packed order */
  uint32_t blk0;       /* first block of the tile-block domain */
  uint32_t pad[2];
};
/* a wave's block is (1 << log_bw) x (64 >> log_bw) pixels: 8 x 8, or HRT_FEATURE_BLOCK_W
 * (1 .. 64, a power of two), an A/B knob between bit-identical variants */
uint32_t block_log_w();
inline uint32_t tile_blocks(uint32_t w, uint32_t h, uint32_t log_bw) {
  const uint32_t bw = 1u << log_bw, bh = 64u >> log_bw;
  return ((w + bw - 1) / bw) * ((h + bh - 1) / bh);
}
/* one launch: samples [P.sample_offset, + P.spp) of every pixel of the tiles, added to the packed planes.
 * cull: layout.h CULL_*; full: the FULL instantiation (general scenes, and sphere scenes with heavy textures) */
void launch_features(int cull, bool full, const KParams& P, const FeatureTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                     uint32_t log_bw, void* d_fa, void* d_fn, void* stream);
/* (fa, fn) -> the mean planes, n pixels; either output may be null */
void launch_feature_means(const void* d_fa, const void* d_fn, size_t n, float inv, void* d_albedo, void* d_normal, void* stream);
/* dst += src for both planes */
void launch_feature_merge(void* d_fa, void* d_fn, const void* s_fa, const void* s_fn, size_t n, void* stream);

}  // namespace features
}  // namespace hrt
