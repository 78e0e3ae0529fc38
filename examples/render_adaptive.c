/*
 * render_adaptive.c — noise-driven refinement on the C ABI alone: the random-spheres scene (application.rs:497-565)
 * gets one pass over every tile, then further passes go only to the tiles whose mean relative error is still above
 * the target (hrt_accum_noise, hrt_accum_add_tiles), until none is left or a tile holds max_spp samples.  The sky
 * stops after the first pass; the glass and metal spheres take the samples.  The library holds the mechanism, this
 * loop is the policy.  The frame goes to a PFM.
 *
 *   make -C examples && ./examples/render_adaptive 400 225 25 32 0.02 512 adaptive.pfm
 *                                                   W   H tile spp/pass target max_spp
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 400;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 225;
  uint32_t tile = argc > 3 ? (uint32_t)atoi(argv[3]) : 25;
  uint32_t pass_spp = argc > 4 ? (uint32_t)atoi(argv[4]) : 32;
  float target = argc > 5 ? (float)atof(argv[5]) : 0.02f;
  uint32_t max_spp = argc > 6 ? (uint32_t)atoi(argv[6]) : 512;
  const char* out = argc > 7 ? argv[7] : "adaptive.pfm";
  const float floor = 0.05f; /* pixels darker than this (mean of r + g + b) are measured against it */

  hrt_scene* s = NULL;
  hrt_preset_info info;
  CHECK(hrt_scene_create(&s));
  CHECK(hrt_preset_build(s, HRT_PRESET_RANDOM, 1, NULL, 0, 0, 0, &info));
  CHECK(hrt_scene_commit(s, 0));
  hrt_camera cam;
  CHECK(hrt_camera_init(&cam, info.look_from, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0,
                        info.time1, (int32_t)w, (int32_t)h));
  hrt_render_params p = {0};
  p.width = w;
  p.height = h;
  p.samples = pass_spp;
  p.max_depth = 50;
  p.t_min = 0.001f;
  p.background[0] = info.background[0];
  p.background[1] = info.background[1];
  p.background[2] = info.background[2];
  p.seed = 1;

  uint32_t n_tiles = 0;
  CHECK(hrt_tile_grid(w, h, tile, 0, 1, NULL, 0, &n_tiles));
  hrt_tile* tiles = (hrt_tile*)malloc(sizeof(hrt_tile) * n_tiles);
  hrt_tile_noise* noise = (hrt_tile_noise*)malloc(sizeof(hrt_tile_noise) * n_tiles);
  uint32_t* todo = (uint32_t*)malloc(sizeof(uint32_t) * n_tiles);
  float* packed = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  float* frame = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  if (!tiles || !noise || !todo || !packed || !frame) return 1;
  CHECK(hrt_tile_grid(w, h, tile, 0, 1, tiles, n_tiles, &n_tiles));
  hrt_accum* acc = NULL;
  CHECK(hrt_accum_create_ex(s, w, h, tiles, n_tiles, HRT_ACCUM_NOISE, &acc));

  /* pass k of a tile is always samples [k * pass_spp, (k + 1) * pass_spp): the tiles still refined have taken every
   * pass so far, so one sample_offset serves them all */
  unsigned long long rays = 0, tile_passes = 0;
  uint32_t n_todo = n_tiles, passes = 0;
  for (uint32_t t = 0; t < n_tiles; t++) todo[t] = t;
  while (n_todo > 0) {
    hrt_render_stats stats;
    p.sample_offset = passes * pass_spp;
    if (passes == 0) CHECK(hrt_accum_add(acc, &cam, &p, NULL, &stats));
    else CHECK(hrt_accum_add_tiles(acc, &cam, &p, todo, n_todo, NULL, &stats));
    rays += (unsigned long long)stats.segments;
    tile_passes += n_todo;
    passes++;
    CHECK(hrt_accum_noise(acc, floor, NULL, NULL, noise));
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n_todo; i++) {
      const hrt_tile_noise* r = &noise[todo[i]];
      if (r->mean > target && r->samples < max_spp) todo[kept++] = todo[i];
    }
    n_todo = kept;
  }

  /* each tile resolves with its own sample count; the tiles are packed back to back, so scatter them into the frame */
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, packed));
  size_t off = 0;
  uint64_t most = 0;
  printf("samples per tile:");
  for (uint32_t t = 0; t < n_tiles; t++) {
    for (uint32_t y = 0; y < tiles[t].h; y++)
      memcpy(frame + 4 * ((size_t)(tiles[t].y + y) * w + tiles[t].x), packed + 4 * (off + (size_t)y * tiles[t].w),
             sizeof(float) * 4 * tiles[t].w);
    off += (size_t)tiles[t].w * tiles[t].h;
    if (noise[t].samples > most) most = noise[t].samples;
    printf(" %llu", (unsigned long long)noise[t].samples);
  }
  printf("\n");
  CHECK(hrt_image_write(out, frame, w, h, HRT_IMAGE_PFM));
  printf("%ux%u in %u tiles, %u passes of %u spp to a mean error of %g: %llu tile passes (a uniform render to %llu spp: %llu), "
         "%llu rays -> %s\n", w, h, n_tiles, passes, pass_spp, (double)target, tile_passes, (unsigned long long)most,
         (unsigned long long)(most / pass_spp) * n_tiles, rays, out);
  free(tiles);
  free(noise);
  free(todo);
  free(packed);
  free(frame);
  hrt_accum_destroy(acc);
  hrt_scene_destroy(s);
  return 0;
}
