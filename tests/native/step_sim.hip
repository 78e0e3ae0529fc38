/*
 * step_sim.hip — TEST INFRASTRUCTURE: path stepping's per-lane code (hyper-ray-tracer_amd/csrc/step.h) on the host, one
 * path at a time, over the flattened scene of hrt_debug_scene_blob, as query_sim.hip runs query.h and scatter_sim.hip
 * scatter.h.  A lane of step_kernel executes exactly this for its path: leave a DONE path alone, else step_path and the
 * stores.  Built by the tests (host-only compile); not part of libhrt.
 */
#include <cstring>

#include "step.h"

using namespace hrt;
using namespace hrt::lane;
using namespace hrt::stepq;

namespace {

template <int CULL, bool FULL, bool MEDIA>
uint64_t batch(const KParams& P, hrt_ray* rays, hrt_path* paths, uint64_t n, hrt_hit* hits, uint32_t steps) {
  uint64_t walked = 0;
  for (uint64_t i = 0; i < n; i++) {
    const float4 tail = scatterq::load_path_tail(paths + i);
    if (scatterq::tail_done(tail)) continue;
    hrt_path path = scatterq::load_path(paths + i, tail);
    hrt_ray ray = query::load_ray(rays + i);
    const Stepped r = step_path<CULL, FULL, MEDIA>(P, P.nodes, P.prims, ray, path, steps);
    query::store_ray(rays + i, ray);
    scatterq::store_path(paths + i, path);
    if (hits) query::store_hit(hits + i, r.hit);
    walked += r.n_rays;
  }
  return walked;
}

template <int CULL>
uint64_t batch_cull(bool full, bool media, const KParams& P, hrt_ray* rays, hrt_path* paths, uint64_t n, hrt_hit* hits, uint32_t steps) {
  if (full && media) return batch<CULL, true, true>(P, rays, paths, n, hits, steps);
  if (full) return batch<CULL, true, false>(P, rays, paths, n, hits, steps);
  return batch<CULL, false, false>(P, rays, paths, n, hits, steps);
}

}  // namespace

/* hrt_scene_step_host's effect on rays[0 .. n), paths[0 .. n) and, when given, hits[0 .. n) (16-byte aligned records, in
 * place), *n_rays += the valid rays walked; n_mats: the scene's material count.  Returns 0, or 1 for a bad argument. */
extern "C" int step_sim(const void* blob, const hrt_blob_info* bi, const hrt_step_params* sp, hrt_ray* rays, hrt_path* paths, uint64_t n,
                        hrt_hit* hits, uint64_t* n_rays, uint32_t n_mats) {
  if (!blob || !bi || !sp || !step_params_ok(sp) || n >= (1ull << 32)) return 1;
  if (n == 0) return 0;
  if (!rays || !paths || ((uintptr_t)rays & 15u) || ((uintptr_t)paths & 15u) || ((uintptr_t)hits & 15u)) return 1;
  const uint8_t* base = (const uint8_t*)blob;
  KParams P;
  memset(&P, 0, sizeof(P));
  P.nodes = (const G::Node*)(base + bi->off_nodes);
  P.prims = (const G::Prim*)(base + bi->off_prims);
  P.insts = (const G::Inst*)(base + bi->off_insts);
  P.media = (const G::Medium*)(base + bi->off_media);
  P.mats = (const G::Mat*)(base + bi->off_mats);
  P.texs = (const G::Tex*)(base + bi->off_texs);
  P.perlin = (const G::Perlin*)(base + bi->off_perlin);
  P.images = base + bi->off_images;
  P.chains = (const float4*)(base + bi->off_chains);
  P.main_end = bi->main_end;
  P.ln_e = bi->ln_e;
  P.n_nodes = bi->n_nodes;
  P.n_prims = bi->n_prims;
  P.motion_uniform = bi->motion_uniform;
  P.motion_t0 = bi->motion_t0;
  P.motion_span = bi->motion_span;
  P.time0 = sp->time0;
  P.time1 = sp->time1;
  P.seed = sp->seed;
  P.n_mats = n_mats;
  P.background = v3(sp->background[0], sp->background[1], sp->background[2]);
  const hrt_query_params q = step_query_params(sp);
  const bool full = (bi->feature_mask & ~G::F_BASIC) != 0 || bi->walk_general;
  const bool media = full && (bi->feature_mask & G::F_MEDIUM) != 0 && !(sp->flags & HRT_STEP_SKIP_MEDIA);
  uint64_t walked;
  if (query::query_cull(&q, (int)bi->cull_mode, bi->box_t0, bi->box_t1) == G::CULL_EXACT)
    walked = batch_cull<G::CULL_EXACT>(full, media, P, rays, paths, n, hits, sp->steps);
  else
    walked = batch_cull<G::CULL_REFERENCE>(full, media, P, rays, paths, n, hits, sp->steps);
  if (n_rays) *n_rays += walked;
  return 0;
}
