/*
 * render_demod.c — a preview of a noisy TEXTURED scene, on the C ABI alone: render_guided.c's loop on the random-spheres
 * scene, whose ground is a checker.  A filter that smooths radiance stops at every checker edge and leaves the noise on
 * both sides of it; with HRT_GUIDED_DEMODULATE (hrt_accum_resolve_guided_ex_host) the same filter runs on the radiance
 * divided by the first-hit albedo and the albedo is multiplied back, so it averages irradiance across the edges and the
 * texture stays sharp.  The frame is written three times: as it is, through the guided filter, and through the guided
 * filter with demodulation.  No resolve changes the accumulator.
 *
 *   make -C examples && ./examples/render_demod 480 270 8 2 16 plain.pfm guided.pfm demodulated.pfm
 *                                                W   H  spp/pass passes feature-samples
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
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 480;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 270;
  uint32_t pass_spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 8;
  uint32_t n_passes = argc > 4 ? (uint32_t)atoi(argv[4]) : 2;
  uint32_t feature_spp = argc > 5 ? (uint32_t)atoi(argv[5]) : 16;
  const char* plain = argc > 6 ? argv[6] : "plain.pfm";
  const char* guided = argc > 7 ? argv[7] : "guided.pfm";
  const char* demodulated = argc > 8 ? argv[8] : "demodulated.pfm";
  const hrt_guided_params guide = {3, 4.0f, 0.1f, 0.1f, 0.1f}; /* normal, albedo, depth tolerances */
  /* the same filter on the demodulated radiance, with the tolerances measured for it (README.md); albedo floor 0.01 */
  const hrt_guided_ex_params demod = {3, 4.0f, 0.05f, 0.2f, 0.2f, HRT_GUIDED_DEMODULATE, 0.01f, 0};

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
  CHECK(hrt_accum_create_ex(s, w, h, &frame, 1, HRT_ACCUM_NOISE | HRT_ACCUM_FEATURES, &acc));
  float* rgba = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  if (!rgba) return 1;
  for (uint32_t k = 0; k < n_passes; k++) {
    p.sample_offset = k * pass_spp;
    CHECK(hrt_accum_add(acc, &cam, &p, NULL, NULL));
  }
  /* the first hits of samples [0, feature_spp): the albedo plane the demodulation divides by */
  p.sample_offset = 0;
  p.samples = feature_spp;
  CHECK(hrt_accum_add_features(acc, &cam, &p, NULL));
  uint64_t samples = 0, feature_samples = 0;
  CHECK(hrt_accum_samples(acc, &samples));
  CHECK(hrt_accum_feature_samples(acc, &feature_samples));
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(plain, rgba, w, h, HRT_IMAGE_PFM));
  CHECK(hrt_accum_resolve_guided_host(acc, &guide, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(guided, rgba, w, h, HRT_IMAGE_PFM));
  CHECK(hrt_accum_resolve_guided_ex_host(acc, &demod, HRT_ACCUM_F32, rgba));
  CHECK(hrt_image_write(demodulated, rgba, w, h, HRT_IMAGE_PFM));
  printf("%ux%u, %llu spp and %llu feature samples -> %s, %s (guided), %s (guided, demodulated)\n", w, h,
         (unsigned long long)samples, (unsigned long long)feature_samples, plain, guided, demodulated);
  free(rgba);
  hrt_accum_destroy(acc);
  hrt_scene_destroy(s);
  return 0;
}
