/*
 * scatter.h — scatter queries (hrt_scene_scatter, hrt_camera_paths; include/hrt/hrt.h), per-lane code like query.h: the
 * same functions on the device (scatter.hip scatter_kernel, query.hip camera_paths_kernel) and on the host
 * (tests/native/scatter_sim.hip), built with -ffp-contract=off.
 *
 * scatter_step is the part of one ray_color step after world.hit (lane.h shade) for a path the CALLER holds: the hit
 * record comes from an hrt_hit instead of make_record, the path's state from an hrt_path instead of a PathState that
 * lives in registers for the whole path.  It reads the ray, the hit, the path, P.mats / P.texs / P.perlin / P.images,
 * P.n_mats and P.perlin_lds and nothing else of P; it draws from the path's own stream alone.  camera_path is
 * start_sample's ray (query.h camera_ray) together with the state start_sample leaves behind.
 */
#pragma once
#include "query.h"

namespace hrt {
namespace scatterq { /* not `scatter`: that is lane.h's function */

using namespace hrt::lane;
using hrt::query::load_ray;
using hrt::query::store_ray;

/* a hit and a path as three 16-B accesses each (the records are 16-B aligned: the entry points check) */
HRT_LANE_FI hrt_hit load_hit(const hrt_hit* p) {
  const float4 a = ld4(p), b = ld4(reinterpret_cast<const float4*>(p) + 1), c = ld4(reinterpret_cast<const float4*>(p) + 2);
  hrt_hit h;
  h.t = a.x, h.prim = f2u(a.y), h.material = f2u(a.z), h.flags = f2u(a.w);
  h.point[0] = b.x, h.point[1] = b.y, h.point[2] = b.z, h.u = b.w;
  h.normal[0] = c.x, h.normal[1] = c.y, h.normal[2] = c.z, h.v = c.w;
  return h;
}
/* the path's last 16 bytes: radiance and flags (what a finished path's lane reads, and nothing more) */
HRT_LANE_FI float4 load_path_tail(const hrt_path* p) { return ld4(reinterpret_cast<const float4*>(p) + 2); }
HRT_LANE_FI bool tail_done(const float4& tail) { return (f2u(tail.w) & (uint32_t)HRT_PATH_DONE) != 0u; }
HRT_LANE_FI hrt_path load_path(const hrt_path* p, const float4& tail) {
  const float4 a = ld4(p), b = ld4(reinterpret_cast<const float4*>(p) + 1);
  hrt_path q;
  q.rng[0] = f2u(a.x), q.rng[1] = f2u(a.y), q.rng[2] = f2u(a.z), q.rng[3] = f2u(a.w);
  q.throughput[0] = b.x, q.throughput[1] = b.y, q.throughput[2] = b.z, q.depth_left = f2u(b.w);
  q.radiance[0] = tail.x, q.radiance[1] = tail.y, q.radiance[2] = tail.z, q.flags = f2u(tail.w);
  return q;
}
HRT_LANE_FI void store_path(hrt_path* p, const hrt_path& q) {
  float4* o = reinterpret_cast<float4*>(p);
  o[0] = make_float4(u2f(q.rng[0]), u2f(q.rng[1]), u2f(q.rng[2]), u2f(q.rng[3]));
  o[1] = make_float4(q.throughput[0], q.throughput[1], q.throughput[2], u2f(q.depth_left));
  o[2] = make_float4(q.radiance[0], q.radiance[1], q.radiance[2], u2f(q.flags));
}

/* hrt.h rule 5: the path ends in this call, and hrt_scene_intersect answers its ray as invalid from now on */
HRT_LANE_FI void finish(hrt_ray& ray, hrt_path& path, uint32_t why) {
  path.flags |= why | (uint32_t)HRT_PATH_DONE;
  ray.t_max = ray.t_min;
}

/* One path's step (hrt.h "hrt_scene_scatter, for path i, in this order").  Returns false when nothing of the ray or the
 * path may be written (a path DONE on entry), true when both are to be stored. */
HRT_LANE bool scatter_step(const KParams& P, hrt_ray& ray, const hrt_hit& hit, hrt_path& path, Vec3 background) {
  if (path.flags & (uint32_t)HRT_PATH_DONE) return false;
  const uint32_t known = HRT_HIT_HIT | HRT_HIT_FRONT | HRT_HIT_MEDIUM | HRT_HIT_INVALID;
  const bool is_hit = (hit.flags & (uint32_t)HRT_HIT_HIT) != 0u;
  /* the material id is checked before any read; flags without HRT_HIT_HIT other than 0 are no record intersect writes */
  const bool bad_hit = (hit.flags & (uint32_t)HRT_HIT_INVALID) != 0u || (hit.flags & ~known) != 0u ||
                       (is_hit ? hit.material >= P.n_mats : hit.flags != 0u);
  if (bad_hit || (path.rng[0] | path.rng[1] | path.rng[2] | path.rng[3]) == 0u) { /* rng 0: random_in_unit_sphere would never end */
    finish(ray, path, HRT_PATH_INVALID);
    return true;
  }
  if (path.depth_left == 0u) { /* segment()'s depth cap: black, without a step (no path of hrt_camera_paths gets here) */
    finish(ray, path, HRT_PATH_DEPTH);
    return true;
  }
  PathState ps;
  ps.rng.s0 = path.rng[0], ps.rng.s1 = path.rng[1], ps.rng.s2 = path.rng[2], ps.rng.s3 = path.rng[3];
  ps.thr = v3(path.throughput[0], path.throughput[1], path.throughput[2]);
  ps.rad = v3(path.radiance[0], path.radiance[1], path.radiance[2]);
  ps.depth_left = path.depth_left;
  uint32_t why;
  if (!is_hit) { /* lane.h shade: the miss */
    ps.rad = ps.rad + mul_elem(ps.thr, background);
    why = HRT_PATH_MISSED;
  } else {
    Rec rec;
    rec.p = v3(hit.point[0], hit.point[1], hit.point[2]);
    rec.n = v3(hit.normal[0], hit.normal[1], hit.normal[2]);
    rec.u = hit.u;
    rec.v = hit.v;
    rec.front = (hit.flags & (uint32_t)HRT_HIT_FRONT) != 0u;
    rec.mat = hit.material;
    const G::Mat M = P.mats[rec.mat];
    Counts cn{0u, 0u, 0u, 0u, 0u, 0u};
    const Vec3 rd = v3(ray.direction[0], ray.direction[1], ray.direction[2]);
    const bool ended = scatter<true>(ps, rec, M.kind, v3(M.a[0], M.a[1], M.a[2]), M.a[3], M.a[0], rd,
                                     [&]() { return tex_value<true, false>(P, M.tex, rec.u, rec.v, rec.p, cn); });
    why = ended ? (uint32_t)HRT_PATH_ABSORBED : 0u;
    if (!ended) {
      ray.origin[0] = ps.ro.x, ray.origin[1] = ps.ro.y, ray.origin[2] = ps.ro.z;
      ray.direction[0] = ps.rd.x, ray.direction[1] = ps.rd.y, ray.direction[2] = ps.rd.z;
      ray.segment += 1u;
      ray.t_max = u2f(0x7f800000u);
      if (ps.depth_left == 0u) why = HRT_PATH_DEPTH;
    }
  }
  path.rng[0] = ps.rng.s0, path.rng[1] = ps.rng.s1, path.rng[2] = ps.rng.s2, path.rng[3] = ps.rng.s3;
  path.throughput[0] = ps.thr.x, path.throughput[1] = ps.thr.y, path.throughput[2] = ps.thr.z;
  path.radiance[0] = ps.rad.x, path.radiance[1] = ps.rad.y, path.radiance[2] = ps.rad.z;
  path.depth_left = ps.depth_left;
  if (why != 0u) finish(ray, path, why);
  return true;
}

/* one record pair of a batch, in place: a finished path's lane reads 16 bytes and writes nothing */
HRT_LANE void scatter_record(const KParams& P, hrt_ray* ray_at, const hrt_hit* hit_at, hrt_path* path_at, Vec3 background) {
  const float4 tail = load_path_tail(path_at);
  if (tail_done(tail)) return;
  hrt_path path = load_path(path_at, tail);
  hrt_ray ray = load_ray(ray_at);
  const hrt_hit hit = load_hit(hit_at);
  if (!scatter_step(P, ray, hit, path, background)) return;
  store_ray(ray_at, ray);
  store_path(path_at, path);
}

/* start_sample's ray (query.h camera_ray, word for word) and the state it leaves: the rng after the jitter, lens and
 * shutter draws, throughput 1, radiance +0, P.max_depth segments to go.  A depth cap of 0 starts the path finished. */
struct CameraPath {
  hrt_ray ray;
  hrt_path path;
};
HRT_LANE CameraPath camera_path(const KParams& P, uint32_t px, uint32_t py, uint32_t k) {
  PathState ps;
  start_sample(P, ps, px, py, k);
  CameraPath c;
  c.ray.origin[0] = ps.ro.x, c.ray.origin[1] = ps.ro.y, c.ray.origin[2] = ps.ro.z;
  c.ray.t_min = P.t_min;
  c.ray.direction[0] = ps.rd.x, c.ray.direction[1] = ps.rd.y, c.ray.direction[2] = ps.rd.z;
  c.ray.t_max = u2f(0x7f800000u);
  c.ray.time = ps.rtime;
  c.ray.pixel = py * P.W + px;
  c.ray.sample = P.sample_offset + k;
  c.ray.segment = 0u;
  c.path.rng[0] = ps.rng.s0, c.path.rng[1] = ps.rng.s1, c.path.rng[2] = ps.rng.s2, c.path.rng[3] = ps.rng.s3;
  c.path.throughput[0] = ps.thr.x, c.path.throughput[1] = ps.thr.y, c.path.throughput[2] = ps.thr.z;
  c.path.depth_left = ps.depth_left;
  c.path.radiance[0] = ps.rad.x, c.path.radiance[1] = ps.rad.y, c.path.radiance[2] = ps.rad.z;
  c.path.flags = 0u;
  if (ps.depth_left == 0u) finish(c.ray, c.path, HRT_PATH_DEPTH);
  return c;
}

/* ---- host side ---- */

/* the params' own checks (hrt.h): no flag is defined, both reserved words 0, a finite background */
inline bool scatter_params_ok(const hrt_scatter_params* sp) {
  return sp->flags == 0 && sp->reserved == 0 && sp->reserved2 == 0 && query::finite_f(sp->background[0]) &&
         query::finite_f(sp->background[1]) && query::finite_f(sp->background[2]);
}

}  // namespace scatterq
}  // namespace hrt
