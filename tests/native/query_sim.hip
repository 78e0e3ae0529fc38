/*
 * query_sim.hip — TEST INFRASTRUCTURE: the ray queries' per-lane code (hyper-ray-tracer_amd/csrc/query.h) on the host,
 * one ray at a time, over the flattened scene of hrt_debug_scene_blob, as feature_sim.hip runs feature_pass.h.  A lane
 * of query_kernel executes exactly query_ray for its ray, and a lane of camera_rays_kernel camera_ray for its pixel's
 * samples, so this reproduces what the kernels write.  Built by the tests (host-only compile); not part of libhrt.
 */
#include <cstring>

#include "query.h"

using namespace hrt;
using namespace hrt::lane;
using namespace hrt::query;

namespace {

KParams host_params(const void* blob, const hrt_blob_info* bi, const hrt_query_params* q) {
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
  P.time0 = q->time0;
  P.time1 = q->time1;
  P.seed = q->seed;
  return P;
}

template <int CULL, bool FULL, bool MEDIA>
void batch(const KParams& P, const hrt_ray* rays, uint64_t n, hrt_hit* hits) {
  for (uint64_t i = 0; i < n; i++) store_hit(hits + i, query_ray<CULL, FULL, MEDIA>(P, P.nodes, P.prims, load_ray(rays + i)));
}

template <int CULL>
void batch_cull(bool full, bool media, const KParams& P, const hrt_ray* rays, uint64_t n, hrt_hit* hits) {
  if (full && media) batch<CULL, true, true>(P, rays, n, hits);
  else if (full) batch<CULL, true, false>(P, rays, n, hits);
  else batch<CULL, false, false>(P, rays, n, hits);
}

}  // namespace

/* hrt_scene_intersect's answer for rays[0 .. n) (16-byte aligned records), through the instantiation the library's
 * dispatch picks: exact culling inside the blob's box interval and the reference test otherwise or on request, FULL for
 * every scene but a sphere scene with solid and checker textures only (full >= 0 forces it), media unless skipped.
 * Returns 0, or 1 for a bad argument (the entry point's HRT_ERR_INVALID_ARG cases). */
extern "C" int query_sim(const void* blob, const hrt_blob_info* bi, const hrt_query_params* q, const hrt_ray* rays, uint64_t n,
                         hrt_hit* hits, int full) {
  if (!blob || !bi || !q || !query_params_ok(q) || n >= (1ull << 32)) return 1;
  if (n == 0) return 0;
  if (!rays || !hits || ((uintptr_t)rays & 15u) || ((uintptr_t)hits & 15u)) return 1;
  const KParams P = host_params(blob, bi, q);
  if (full < 0) full = ((bi->feature_mask & ~G::F_BASIC) != 0 || bi->walk_general) ? 1 : 0;
  if (!full && (bi->feature_mask & ~G::F_BASIC) != 0) return 1; /* the sphere instantiation knows no other primitive */
  const bool media = full && (bi->feature_mask & G::F_MEDIUM) != 0 && !(q->flags & HRT_QUERY_SKIP_MEDIA);
  if (query_cull(q, (int)bi->cull_mode, bi->box_t0, bi->box_t1) == G::CULL_EXACT) batch_cull<G::CULL_EXACT>(full != 0, media, P, rays, n, hits);
  else batch_cull<G::CULL_REFERENCE>(full != 0, media, P, rays, n, hits);
  return 0;
}

/* hrt_camera_rays' rays for the region (x0, y0, w, h) as one tile: ray ((y * w + x) * p->samples + k).  Returns 0, or 1
 * for a bad argument. */
extern "C" int camera_rays_sim(const hrt_camera* cam, const hrt_render_params* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                               hrt_ray* rays) {
  if (!cam || !p || !rays || ((uintptr_t)rays & 15u) || p->width < 2 || p->height < 2 || p->width > 65535 || p->height > 65535 ||
      p->samples == 0 || w == 0 || h == 0 || (uint64_t)x0 + w > p->width || (uint64_t)y0 + h > p->height)
    return 1;
  KParams P;
  memset(&P, 0, sizeof(P));
  set_camera_params(P, cam, p);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++)
      for (uint32_t k = 0; k < p->samples; k++)
        store_ray(rays + ((size_t)y * w + x) * p->samples + k, camera_ray(P, x0 + x, y0 + y, k));
  return 0;
}
