/*
 * render_denoise.c — a preview of a noisy scene, on the C ABI alone: render_refine.c's loop on the Cornell box
 * (application.rs:639-721), the scene the reference gives 10 000 samples per pixel because a few dozen are raw
 * Monte-Carlo noise.  The accumulator keeps the noise plane (HRT_ACCUM_NOISE), and after the last pass the frame is
 * written twice: as it is, and through the variance-guided a-trous filter (hrt_accum_resolve_filtered_host), which
 * smooths each pixel as far as its own estimated noise allows.  The filter reads the accumulator and changes nothing
 * in it: further passes and the plain resolve go on as if it had not run.  It is a preview for noisy scenes, not a
 * default: on a frame that is already clean it only blurs.
 *
 *   make -C examples && ./examples/render_denoise 256 256 16 4 3 4.0 plain.pfm filtered.pfm
 *                                                  W   H  spp/pass passes iterations sigma
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
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 256;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 256;
  uint32_t pass_spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
  uint32_t n_passes = argc > 4 ? (uint32_t)atoi(argv[4]) : 4;
  hrt_filter_params filter;
  filter.iterations = argc > 5 ? (uint32_t)atoi(argv[5]) : 3;
  filter.sigma = argc > 6 ? (float)atof(argv[6]) : 4.0f;
  const char* plain = argc > 7 ? argv[7] : "plain.pfm";
  const char* filtered = argc > 8 ? argv[8] : "filtered.pfm";

  hrt_scene* s = NULL;
  hrt_preset_info info;
  CHECK(hrt_scene_create(&s));
  CHECK(hrt_preset_build(s, HRT_PRESET_CORNELL, 1, NULL, 0, 0, 0, &info));
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
  CHECK(hrt_accum_create_ex(s, w, h, &frame, 1, HRT_ACCUM_NOISE, &acc));
  float* rgba = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  if (!rgba) return 1;
  unsigned long long rays = 0;
  for (uint32_t k = 0; k < n_passes; k++) {
    hrt_render_stats stats;
    p.sample_offset = k * pass_spp; /* this pass: samples [k * pass_spp, (k + 1) * pass_spp) of every pixel */
    CHECK(hrt_accum_add(acc, &cam, &p, NULL, &stats));
    rays += (unsigned long long)stats.segments;
  }
  uint64_t samples = 0;
  CHECK(hrt_accum_samples(acc, &samples));
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(plain, rgba, w, h, HRT_IMAGE_PFM));
  /* the same samples through the filter; a variance estimate needs two chunks, so one pass of very few samples is
   * refused with HRT_ERR_STATE */
  CHECK(hrt_accum_resolve_filtered_host(acc, &filter, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(filtered, rgba, w, h, HRT_IMAGE_PFM));
  printf("%ux%u, %u passes of %u spp = %llu spp: %llu rays -> %s, and %s through %u iterations at sigma %g\n", w, h, n_passes,
         pass_spp, (unsigned long long)samples, rays, plain, filtered, filter.iterations, (double)filter.sigma);
  free(rgba);
  hrt_accum_destroy(acc);
  hrt_scene_destroy(s);
  return 0;
}
