/*
 * render_integrator.c — your own integrator on the C ABI alone: the `random` preset rendered WITHOUT a render call.
 * For every sample index k the loop of include/hrt/hrt.h "scatter queries" runs once, through the host variants:
 * hrt_camera_paths_host starts one path per pixel, then hrt_scene_intersect_host and hrt_scene_scatter_host take turns
 * until every path is DONE.  A path's radiance is the render's sample bit for bit, so the sums follow the accumulator
 * contract (a one-sample pass is added as acc = acc + pass_sum) and the frame is sqrtf(acc * (1.0f / samples)): what
 * an hrt_accum fed the same one-sample passes resolves to.  Between the two calls the paths are the program's own:
 * this is where a custom integrator would look at the hits, weight or kill paths, or write per-bounce AOVs.
 * Prints the rays traced and a checksum of the frame (FNV-1a over its bytes).
 *
 *   make -C examples && ./examples/render_integrator 256 144 16 integrator.pfm
 *                                                     W   H  spp
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "hrt/hrt.h"

#define CHECK(call)                                                                       \
  do {                                                                                    \
    hrt_status st_ = (call);                                                              \
    if (st_ != HRT_OK) {                                                                  \
      fprintf(stderr, "%s failed (status %d): %s\n", #call, (int)st_, hrt_last_error());  \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

int main(int argc, char** argv) {
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 256;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 144;
  uint32_t spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
  const char* path = argc > 4 ? argv[4] : "integrator.pfm";

  hrt_scene* s = NULL;
  hrt_preset_info info;
  CHECK(hrt_scene_create(&s));
  CHECK(hrt_preset_build(s, HRT_PRESET_RANDOM, 1, NULL, 0, 0, 0, &info));
  CHECK(hrt_scene_commit(s, 0));
  hrt_camera cam;
  CHECK(hrt_camera_init(&cam, info.look_from, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0, info.time1,
                        (int32_t)w, (int32_t)h));
  hrt_render_params p = {0};
  p.width = w;
  p.height = h;
  p.samples = 1; /* one path per pixel and pass */
  p.max_depth = 50;
  p.t_min = 0.001f;
  p.seed = 1;
  hrt_query_params q = {0};
  q.time0 = cam.time0;
  q.time1 = cam.time1;
  q.seed = p.seed;
  hrt_scatter_params sp = {0};
  for (int c = 0; c < 3; c++) p.background[c] = sp.background[c] = info.background[c];

  const size_t n = (size_t)w * h;
  const hrt_tile frame = {0, 0, w, h};
  hrt_ray* rays = (hrt_ray*)malloc(n * sizeof(hrt_ray));
  hrt_hit* hits = (hrt_hit*)malloc(n * sizeof(hrt_hit));
  hrt_path* paths = (hrt_path*)malloc(n * sizeof(hrt_path));
  float* rgba = (float*)calloc(4 * n, sizeof(float)); /* the sums, then the frame */
  if (!rays || !hits || !paths || !rgba) return 1;

  unsigned long long n_rays = 0;
  for (uint32_t k = 0; k < spp; k++) {
    p.sample_offset = k;
    CHECK(hrt_camera_paths_host(s, &cam, &p, &frame, 1, rays, paths));
    for (uint32_t round = 0; round < p.max_depth; round++) {
      size_t live = 0;
      for (size_t i = 0; i < n; i++) live += !(paths[i].flags & HRT_PATH_DONE);
      if (live == 0) break;
      CHECK(hrt_scene_intersect_host(s, &q, rays, n, hits));
      for (size_t i = 0; i < n; i++) n_rays += !(hits[i].flags & HRT_HIT_INVALID); /* a finished path's ray is not traced */
      CHECK(hrt_scene_scatter_host(s, &sp, rays, hits, paths, n));
    }
    for (size_t i = 0; i < n; i++)
      for (int c = 0; c < 3; c++) rgba[4 * i + c] = rgba[4 * i + c] + paths[i].radiance[c];
  }
  const float scale = 1.0f / (float)spp;
  for (size_t i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) rgba[4 * i + c] = sqrtf(rgba[4 * i + c] * scale);
    rgba[4 * i + 3] = 1.0f;
  }
  CHECK(hrt_image_write(path, rgba, w, h, HRT_IMAGE_PFM));
  uint64_t sum = 0xCBF29CE484222325ull;
  const unsigned char* bytes = (const unsigned char*)rgba;
  for (size_t i = 0; i < sizeof(float) * 4 * n; i++) sum = (sum ^ bytes[i]) * 0x100000001B3ull;
  printf("rays %llu checksum %016llx -> %s\n", n_rays, (unsigned long long)sum, path);
  free(rays);
  free(hits);
  free(paths);
  free(rgba);
  hrt_scene_destroy(s);
  return 0;
}
