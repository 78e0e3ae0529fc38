/*
 * scatter_sim.hip — TEST INFRASTRUCTURE: the scatter queries' per-lane code (hyper-ray-tracer_amd/csrc/scatter.h) on the
 * host, one path at a time, over the flattened scene of hrt_debug_scene_blob, as query_sim.hip runs query.h.  A lane of
 * scatter_kernel executes exactly scatter_record for its path, and a lane of camera_paths_kernel camera_path for its
 * pixel's samples, so this reproduces what the kernels write.  Built by the tests (host-only compile); not part of libhrt.
 */
#include <cstring>

#include "scatter.h"

using namespace hrt;
using namespace hrt::lane;
using namespace hrt::scatterq;

/* hrt_scene_scatter's effect on rays[0 .. n) and paths[0 .. n) (16-byte aligned records, in place), hits read only;
 * n_mats: the scene's material count (the blob's sections are padded, so the blob does not tell).  Returns 0, or 1 for a
 * bad argument (the entry point's HRT_ERR_INVALID_ARG cases). */
extern "C" int scatter_sim(const void* blob, const hrt_blob_info* bi, const hrt_scatter_params* sp, hrt_ray* rays, const hrt_hit* hits,
                           hrt_path* paths, uint64_t n, uint32_t n_mats) {
  if (!blob || !bi || !sp || !scatter_params_ok(sp) || n >= (1ull << 32)) return 1;
  if (n == 0) return 0;
  if (!rays || !hits || !paths || ((uintptr_t)rays & 15u) || ((uintptr_t)hits & 15u) || ((uintptr_t)paths & 15u)) return 1;
  const uint8_t* base = (const uint8_t*)blob;
  KParams P;
  memset(&P, 0, sizeof(P));
  P.mats = (const G::Mat*)(base + bi->off_mats);
  P.texs = (const G::Tex*)(base + bi->off_texs);
  P.perlin = (const G::Perlin*)(base + bi->off_perlin);
  P.images = base + bi->off_images;
  P.n_mats = n_mats;
  P.background = v3(sp->background[0], sp->background[1], sp->background[2]);
  for (uint64_t i = 0; i < n; i++) scatter_record(P, rays + i, hits + i, paths + i, P.background);
  return 0;
}

/* hrt_camera_paths' rays and paths for the region (x0, y0, w, h) as one tile: record ((y * w + x) * p->samples + k).
 * Returns 0, or 1 for a bad argument. */
extern "C" int camera_paths_sim(const hrt_camera* cam, const hrt_render_params* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                hrt_ray* rays, hrt_path* paths) {
  if (!cam || !p || !rays || !paths || ((uintptr_t)rays & 15u) || ((uintptr_t)paths & 15u) || p->width < 2 || p->height < 2 ||
      p->width > 65535 || p->height > 65535 || p->samples == 0 || w == 0 || h == 0 || (uint64_t)x0 + w > p->width ||
      (uint64_t)y0 + h > p->height)
    return 1;
  KParams P;
  memset(&P, 0, sizeof(P));
  query::set_camera_params(P, cam, p);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++)
      for (uint32_t k = 0; k < p->samples; k++) {
        const size_t at = ((size_t)y * w + x) * p->samples + k;
        const CameraPath c = camera_path(P, x0 + x, y0 + y, k);
        store_ray(rays + at, c.ray);
        store_path(paths + at, c.path);
      }
  return 0;
}
