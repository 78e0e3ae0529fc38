/*
 * query.h — ray queries (hrt_scene_intersect, hrt_camera_rays; include/hrt/hrt.h), per-lane code like feature_pass.h:
 * the same functions on the device (query.hip query_kernel, camera_rays_kernel) and on the host
 * (tests/native/query_sim.hip), built with -ffp-contract=off.
 *
 * query_ray does, for one ray of the caller's:
 *   1. valid_ray: an invalid ray is answered without a walk;
 *   2. trace<CULL, FULL, MEDIA, false, false> over the reference node stream (0 .. P.main_end) from ray.t_min with the
 *      closest starting at ray.t_max, which is what segment() does for a path's ray with that origin, direction and
 *      time; a ConstantMedium draws medium_xi(path_key(P.seed, ray.pixel, ray.sample), ray.segment, medium id);
 *   3. on a hit, make_record<FULL, true>: the render's record with (u, v) always computed.
 * It reads the ray, P's scene pointers, P.main_end, P.ln_e, the motion fields, P.seed and P.time0 / P.time1 (the
 * interval the rays' times lie in) and nothing else of P; it draws nothing but the medium's sub-stream and writes
 * nothing.  camera_ray is start_sample's ray for sample P.sample_offset + k of a pixel.
 */
#pragma once
#include "lane.h"

#ifndef HRT_QUERY_UV
#define HRT_QUERY_UV 1 /* 0 (A/B build only; the contract says always): a sphere's (u, v) as a render computes them, that is
                          under an image texture alone.  It prices sphere_uv's two f64 transcendentals per hit (README.md) */
#endif

namespace hrt {
namespace query {

using namespace hrt::lane;

HRT_LANE_FI bool finite_f(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* hrt.h "Invalid ray" */
HRT_LANE_FI bool valid_ray(const hrt_ray& r, float time0, float time1) {
  const bool fin = finite_f(r.origin[0]) && finite_f(r.origin[1]) && finite_f(r.origin[2]) && finite_f(r.direction[0]) &&
                   finite_f(r.direction[1]) && finite_f(r.direction[2]) && finite_f(r.time) && finite_f(r.t_min);
  if (!fin || r.t_max != r.t_max) return false;
  if (r.direction[0] == 0.0f && r.direction[1] == 0.0f && r.direction[2] == 0.0f) return false;
  if (!(r.t_min < r.t_max)) return false;
  return r.time >= time0 && r.time <= time1;
}

/* a ray and a hit as three 16-B accesses each (the records are 16-B aligned: the entry points check) */
HRT_LANE_FI hrt_ray load_ray(const hrt_ray* p) {
  const float4 a = ld4(p), b = ld4(reinterpret_cast<const float4*>(p) + 1), c = ld4(reinterpret_cast<const float4*>(p) + 2);
  hrt_ray r;
  r.origin[0] = a.x, r.origin[1] = a.y, r.origin[2] = a.z, r.t_min = a.w;
  r.direction[0] = b.x, r.direction[1] = b.y, r.direction[2] = b.z, r.t_max = b.w;
  r.time = c.x, r.pixel = f2u(c.y), r.sample = f2u(c.z), r.segment = f2u(c.w);
  return r;
}
HRT_LANE_FI void store_ray(hrt_ray* p, const hrt_ray& r) {
  float4* q = reinterpret_cast<float4*>(p);
  q[0] = make_float4(r.origin[0], r.origin[1], r.origin[2], r.t_min);
  q[1] = make_float4(r.direction[0], r.direction[1], r.direction[2], r.t_max);
  q[2] = make_float4(r.time, u2f(r.pixel), u2f(r.sample), u2f(r.segment));
}
HRT_LANE_FI void store_hit(hrt_hit* p, const hrt_hit& h) {
  float4* q = reinterpret_cast<float4*>(p);
  q[0] = make_float4(h.t, u2f(h.prim), u2f(h.material), u2f(h.flags));
  q[1] = make_float4(h.point[0], h.point[1], h.point[2], h.u);
  q[2] = make_float4(h.normal[0], h.normal[1], h.normal[2], h.v);
}

/* a miss (flags 0, t = the ray's t_max) or an invalid ray (HRT_HIT_INVALID, t = +0): no ids, every other field +0 */
HRT_LANE_FI hrt_hit no_hit(uint32_t flags, float t) {
  hrt_hit h;
  h.t = t;
  h.prim = G::NONE;
  h.material = G::NONE;
  h.flags = flags;
  h.point[0] = h.point[1] = h.point[2] = h.u = 0.0f;
  h.normal[0] = h.normal[1] = h.normal[2] = h.v = 0.0f;
  return h;
}

/* the closest hit of a VALID ray; pkey: path_key(seed, ray.pixel, ray.sample) */
template <int CULL, bool FULL, bool MEDIA>
HRT_LANE hrt_hit intersect_ray(const KParams& P, const G::Node* __restrict__ nodes, const G::Prim* __restrict__ prims,
                               const hrt_ray& ray, uint64_t pkey) {
  static_assert(FULL || !MEDIA, "a sphere scene holds no medium");
  Counts cn{0u, 0u, 0u, 0u, 0u, 0u};
  PathKey pk;
  pk.pkey = pkey;
  pk.segment = ray.segment;
  const Vec3 o = v3(ray.origin[0], ray.origin[1], ray.origin[2]), d = v3(ray.direction[0], ray.direction[1], ray.direction[2]);
  float closest = ray.t_max;
  uint32_t winner = G::NONE;
  trace<CULL, FULL, MEDIA, false, false>(P, nodes, prims, 0u, P.main_end, o, d, ray.time, ray.t_min, closest, winner, pk, cn);
  if (winner == G::NONE) return no_hit(0u, ray.t_max);
  const float tau = P.motion_uniform ? (ray.time - P.motion_t0) / P.motion_span : 0.0f;
  const Rec rec = make_record<FULL, HRT_QUERY_UV != 0>(P, winner, closest, o, d, ray.time, tau);
  hrt_hit h;
  h.t = closest;
  h.material = rec.mat;
  h.flags = HRT_HIT_HIT | (rec.front ? (uint32_t)HRT_HIT_FRONT : 0u);
  if constexpr (FULL) { /* winner is the leaf's node: its payload is the primitive, or the medium */
    const uint32_t kp = P.nodes[winner].kp;
    h.prim = kp & 0xFFFFFFu;
    if (((kp >> 24) & G::KIND_MASK) == G::K_MEDIUM) h.flags |= HRT_HIT_MEDIUM;
  } else {
    h.prim = winner;
  }
  h.point[0] = rec.p.x, h.point[1] = rec.p.y, h.point[2] = rec.p.z;
  h.normal[0] = rec.n.x, h.normal[1] = rec.n.y, h.normal[2] = rec.n.z;
  h.u = rec.u;
  h.v = rec.v;
  return h;
}

/* one ray of a batch, whatever it is */
template <int CULL, bool FULL, bool MEDIA>
HRT_LANE hrt_hit query_ray(const KParams& P, const G::Node* __restrict__ nodes, const G::Prim* __restrict__ prims,
                           const hrt_ray& ray) {
  if (!valid_ray(ray, P.time0, P.time1)) return no_hit(HRT_HIT_INVALID, 0.0f);
  return intersect_ray<CULL, FULL, MEDIA>(P, nodes, prims, ray, path_key(P.seed, ray.pixel, ray.sample));
}

/* the ray start_sample gives sample P.sample_offset + k of pixel (px, py), from P.t_min to +inf */
HRT_LANE hrt_ray camera_ray(const KParams& P, uint32_t px, uint32_t py, uint32_t k) {
  PathState ps;
  start_sample(P, ps, px, py, k);
  hrt_ray r;
  r.origin[0] = ps.ro.x, r.origin[1] = ps.ro.y, r.origin[2] = ps.ro.z;
  r.t_min = P.t_min;
  r.direction[0] = ps.rd.x, r.direction[1] = ps.rd.y, r.direction[2] = ps.rd.z;
  r.t_max = u2f(0x7f800000u);
  r.time = ps.rtime;
  r.pixel = py * P.W + px;
  r.sample = P.sample_offset + k;
  r.segment = 0u;
  return r;
}

/* ---- host side ---- */

/* the fields of P that camera_ray reads (start_sample's), as render.hip scene_params sets them */
inline void set_camera_params(KParams& P, const hrt_camera* cam, const hrt_render_params* p) {
  P.cam_origin = v3(cam->origin[0], cam->origin[1], cam->origin[2]);
  P.cam_llc = v3(cam->lower_left_corner[0], cam->lower_left_corner[1], cam->lower_left_corner[2]);
  P.cam_h = v3(cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]);
  P.cam_v = v3(cam->vertical[0], cam->vertical[1], cam->vertical[2]);
  P.cam_u = v3(cam->u[0], cam->u[1], cam->u[2]);
  P.cam_vv = v3(cam->v[0], cam->v[1], cam->v[2]);
  P.lens_radius = cam->lens_radius;
  P.time0 = cam->time0;
  P.time1 = cam->time1;
  P.W = p->width;
  P.H = p->height;
  set_pixel_rcp(P);
  P.spp = p->samples;
  P.max_depth = p->max_depth;
  P.sample_offset = p->sample_offset;
  P.t_min = p->t_min;
  P.seed = p->seed;
}

/* the params' own checks (hrt.h): known flags, reserved 0, a finite interval with time0 <= time1 */
inline bool query_params_ok(const hrt_query_params* q) {
  const uint32_t known = HRT_QUERY_SKIP_MEDIA | HRT_QUERY_NO_LDS | HRT_QUERY_REFERENCE_CULL;
  return (q->flags & ~known) == 0 && q->reserved == 0 && finite_f(q->time0) && finite_f(q->time1) && q->time0 <= q->time1;
}
/* the culling of a query: the scene's exact mode inside the interval its BVH boxes were built for (the test render.hip
 * plan makes on the camera's shutter), the reference test otherwise or on request; never an approximate mode */
inline int query_cull(const hrt_query_params* q, int scene_cull, float box_t0, float box_t1) {
  const bool inside = q->time0 >= box_t0 && q->time1 <= box_t1;
  return scene_cull == G::CULL_EXACT && inside && !(q->flags & HRT_QUERY_REFERENCE_CULL) ? (int)G::CULL_EXACT : (int)G::CULL_REFERENCE;
}

}  // namespace query
}  // namespace hrt
