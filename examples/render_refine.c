/*
 * render_refine.c — a frame that refines pass by pass, on the C ABI alone: the reference's viewer shows an image
 * that fills in while it renders; here the whole frame of the random-spheres scene (application.rs:497-565) is
 * there after the first pass of a few samples per pixel, and every further pass adds samples to the same
 * accumulator (hrt_accum).  A PPM preview is written after the first pass and the exact frame of all the samples
 * as a PFM at the end.
 *
 *   make -C examples && ./examples/render_refine 400 225 16 8 preview.ppm final.pfm
 *                                                 W   H  spp/pass passes
 */
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
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 400;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 225;
  uint32_t pass_spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
  uint32_t n_passes = argc > 4 ? (uint32_t)atoi(argv[4]) : 8;
  const char* preview = argc > 5 ? argv[5] : "preview.ppm";
  const char* out = argc > 6 ? argv[6] : "refined.pfm";

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

  const hrt_tile frame = {0, 0, w, h};
  hrt_accum* acc = NULL;
  CHECK(hrt_accum_create(s, w, h, &frame, 1, &acc));
  float* rgba = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  if (!rgba) return 1;
  unsigned long long rays = 0;
  for (uint32_t k = 0; k < n_passes; k++) {
    hrt_render_stats stats;
    p.sample_offset = k * pass_spp; /* this pass: samples [k * pass_spp, (k + 1) * pass_spp) of every pixel */
    CHECK(hrt_accum_add(acc, &cam, &p, NULL, &stats));
    rays += (unsigned long long)stats.segments;
    if (k == 0) { /* the whole frame, noisy, after the first few samples */
      CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, rgba));
      CHECK(hrt_image_write(preview, rgba, w, h, HRT_IMAGE_PPM));
    }
  }
  uint64_t samples = 0;
  CHECK(hrt_accum_samples(acc, &samples));
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(out, rgba, w, h, HRT_IMAGE_PFM));
  printf("%ux%u, %u passes of %u spp = %llu spp: %llu rays -> %s (preview after pass 1: %s)\n", w, h, n_passes, pass_spp,
         (unsigned long long)samples, rays, out, preview);
  free(rgba);
  hrt_accum_destroy(acc);
  hrt_scene_destroy(s);
  return 0;
}
