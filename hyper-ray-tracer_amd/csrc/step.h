/*
 * step.h — path stepping (hrt_scene_step; include/hrt/hrt.h), per-lane code like query.h and scatter.h: the same
 * function on the device (step.hip step_kernel) and on the host, built with -ffp-contract=off.
 *
 * step_path is the loop a caller of hrt_scene_intersect and hrt_scene_scatter runs for one path, with the ray and the
 * path in registers between the rounds and no hit record in memory: up to `steps` times while the path is not DONE,
 * query.h query_ray and then scatter.h scatter_step on its answer, both unchanged.  No arithmetic is new, so the ray and
 * the path after it are bit for bit those after that many rounds of the two calls.  It reads of P what those two read
 * (P.background is scatter_step's background) and nothing else.
 */
#pragma once
#include "scatter.h"

namespace hrt {
namespace stepq {

using namespace hrt::lane;

struct Stepped {
  hrt_hit hit;     /* of the last intersect made (the invalid-ray record before the first) */
  uint32_t n_rays; /* valid rays walked: the intersects that did not answer HRT_HIT_INVALID */
};

/* `path` must not be DONE on entry and steps >= 1 (hrt.h rule 2: the caller leaves such a record alone), so at least one
 * intersect is made.  The loop is bounded by `steps`; scatter_step refuses the all-zero rng before any rejection loop. */
template <int CULL, bool FULL, bool MEDIA>
HRT_LANE Stepped step_path(const KParams& P, const G::Node* __restrict__ nodes, const G::Prim* __restrict__ prims, hrt_ray& ray,
                           hrt_path& path, uint32_t steps) {
  Stepped r;
  r.hit = query::no_hit(HRT_HIT_INVALID, 0.0f);
  r.n_rays = 0u;
  for (uint32_t k = 0; k < steps && (path.flags & (uint32_t)HRT_PATH_DONE) == 0u; k++) {
    r.hit = query::query_ray<CULL, FULL, MEDIA>(P, nodes, prims, ray);
    r.n_rays += (r.hit.flags & (uint32_t)HRT_HIT_INVALID) == 0u ? 1u : 0u;
    (void)scatterq::scatter_step(P, ray, r.hit, path, P.background);
  }
  return r;
}

/* ---- host side ---- */

/* the params' own checks (hrt.h): known flags, steps >= 1, reserved 0, a finite interval with time0 <= time1, a finite
 * background.  The flags are the HRT_QUERY_* ones bit for bit, so the two structs below carry them on. */
static_assert(HRT_STEP_SKIP_MEDIA == HRT_QUERY_SKIP_MEDIA && HRT_STEP_NO_LDS == HRT_QUERY_NO_LDS &&
                  HRT_STEP_REFERENCE_CULL == HRT_QUERY_REFERENCE_CULL,
              "the step flags are the query flags");
inline hrt_query_params step_query_params(const hrt_step_params* sp) {
  hrt_query_params q;
  q.flags = sp->flags;
  q.reserved = sp->reserved;
  q.time0 = sp->time0;
  q.time1 = sp->time1;
  q.seed = sp->seed;
  return q;
}
inline hrt_scatter_params step_scatter_params(const hrt_step_params* sp) {
  hrt_scatter_params s;
  s.flags = 0u;
  s.reserved = s.reserved2 = 0u;
  s.background[0] = sp->background[0], s.background[1] = sp->background[1], s.background[2] = sp->background[2];
  return s;
}
inline bool step_params_ok(const hrt_step_params* sp) {
  const hrt_query_params q = step_query_params(sp);
  const hrt_scatter_params s = step_scatter_params(sp);
  return sp->steps >= 1u && query::query_params_ok(&q) && scatterq::scatter_params_ok(&s);
}

}  // namespace stepq
}  // namespace hrt
