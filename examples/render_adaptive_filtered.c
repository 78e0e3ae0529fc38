/*
 * render_adaptive_filtered.c — render_adaptive.c's refinement driven by the error of the DENOISED preview, on the C ABI
 * alone.  The random-spheres scene is refined twice to the same target: once on the raw per-pixel error
 * (hrt_accum_noise, render_adaptive.c's loop) and once on the estimate of the filtered frame's error
 * (hrt_accum_noise_filtered with every feature term off: the variance-only filter of hrt_accum_resolve_filtered).
 * The second stops as soon as the frame the user looks at, the filtered one, meets the target by the filter's own
 * variance estimate.  That estimate sees the filtered frame's variance and not its blur (include/hrt/hrt.h), so it is a
 * lower bound: read the two sample counts as what the policy saves, not as a promise about the picture.  The filtered
 * frame of the second run goes to a PFM.
 *
 *   make -C examples && ./examples/render_adaptive_filtered 400 225 25 32 0.02 512 adaptive_filtered.pfm
 *                                                            W   H tile spp/pass target max_spp
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
  const char* out = argc > 7 ? argv[7] : "adaptive_filtered.pfm";
  const float floor = 0.05f; /* pixels darker than this (mean of r + g + b) are measured against it */
  /* the preview whose error is estimated: 3 iterations, sigma 4, no feature term, no demodulation */
  const hrt_guided_ex_params g = {3, 4.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f, 0};
  const hrt_filter_params f = {3, 4.0f};

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

  /* policy 0: the raw error (render_adaptive.c).  policy 1: the filtered estimate.  A tile's filtered record moves with
   * its neighbours' passes, so policy 1 selects among ALL tiles after every pass and sends the next pass to the selected
   * tiles that hold the fewest samples; a tile's k-th pass is samples [k * pass_spp, (k + 1) * pass_spp) either way. */
  unsigned long long samples[2] = {0, 0};
  uint32_t passes[2] = {0, 0};
  hrt_accum* acc = NULL;
  for (int policy = 0; policy < 2; policy++) {
    if (acc) hrt_accum_destroy(acc);
    acc = NULL;
    CHECK(hrt_accum_create_ex(s, w, h, tiles, n_tiles, HRT_ACCUM_NOISE, &acc));
    p.sample_offset = 0;
    CHECK(hrt_accum_add(acc, &cam, &p, NULL, NULL));
    passes[policy] = 1;
    for (;;) {
      hrt_status st = policy ? hrt_accum_noise_filtered(acc, &g, floor, NULL, NULL, noise) : HRT_ERR_STATE;
      /* a tile with fewer than 2 chunks has no filtered estimate yet: the raw one answers +inf for it */
      if (st == HRT_ERR_STATE) st = hrt_accum_noise(acc, floor, NULL, NULL, noise);
      CHECK(st);
      uint64_t fewest = UINT64_MAX;
      for (uint32_t t = 0; t < n_tiles; t++)
        if (noise[t].mean > target && noise[t].samples < max_spp && noise[t].samples < fewest) fewest = noise[t].samples;
      if (fewest == UINT64_MAX) break;
      uint32_t n_todo = 0;
      for (uint32_t t = 0; t < n_tiles; t++)
        if (noise[t].mean > target && noise[t].samples == fewest) todo[n_todo++] = t;
      p.sample_offset = (uint32_t)fewest;
      CHECK(hrt_accum_add_tiles(acc, &cam, &p, todo, n_todo, NULL, NULL));
      passes[policy]++;
    }
    printf("samples per tile (%s):", policy ? "filtered estimate" : "raw error");
    for (uint32_t t = 0; t < n_tiles; t++) {
      samples[policy] += (unsigned long long)noise[t].samples * tiles[t].w * tiles[t].h;
      printf(" %llu", (unsigned long long)noise[t].samples);
    }
    printf("\n");
  }

  /* the frame the second policy refined: the filtered one; the tiles are packed back to back, so scatter them */
  CHECK(hrt_accum_resolve_filtered_host(acc, &f, HRT_ACCUM_F32, packed));
  size_t off = 0;
  for (uint32_t t = 0; t < n_tiles; t++) {
    for (uint32_t y = 0; y < tiles[t].h; y++)
      memcpy(frame + 4 * ((size_t)(tiles[t].y + y) * w + tiles[t].x), packed + 4 * (off + (size_t)y * tiles[t].w),
             sizeof(float) * 4 * tiles[t].w);
    off += (size_t)tiles[t].w * tiles[t].h;
  }
  CHECK(hrt_image_write(out, frame, w, h, HRT_IMAGE_PFM));
  printf("%ux%u in %u tiles, passes of %u spp to a mean error of %g: raw error %llu samples in %u passes, filtered estimate "
         "%llu samples in %u passes -> %s\n", w, h, n_tiles, pass_spp, (double)target, samples[0], passes[0], samples[1], passes[1], out);
  free(tiles);
  free(noise);
  free(todo);
  free(packed);
  free(frame);
  hrt_accum_destroy(acc);
  hrt_scene_destroy(s);
  return 0;
}
