/*
 * render_autofocus.c — autofocus on the C ABI alone: focus the camera on whatever lies under the centre pixel.  The
 * `random` preset is looked at through a pinhole (aperture 0) first: hrt_camera_rays_host gives the centre pixel's
 * camera ray, hrt_scene_intersect_host its closest hit, and t * |d| of that hit is the distance to focus at.  The
 * camera is then rebuilt with the preset's aperture and that focus distance, and the frame rendered.  Prints the
 * picked primitive, the depth and a checksum of the frame (FNV-1a over its bytes).
 *
 *   make -C examples && ./examples/render_autofocus 256 144 16 focus.pfm
 *                                                    W   H  spp
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
  const char* path = argc > 4 ? argv[4] : "focus.pfm";

  hrt_scene* s = NULL;
  hrt_preset_info info;
  CHECK(hrt_scene_create(&s));
  CHECK(hrt_preset_build(s, HRT_PRESET_RANDOM, 1, NULL, 0, 0, 0, &info));
  CHECK(hrt_scene_commit(s, 0));
  hrt_render_params p = {0};
  p.width = w;
  p.height = h;
  p.samples = 1;
  p.max_depth = 50;
  p.t_min = 0.001f;
  p.background[0] = info.background[0];
  p.background[1] = info.background[1];
  p.background[2] = info.background[2];
  p.seed = 1;

  /* the pick: sample 0 of the centre pixel through a pinhole */
  hrt_camera pinhole;
  CHECK(hrt_camera_init(&pinhole, info.look_from, info.look_at, info.fov, 0.0f, info.focus_dist, info.time0, info.time1,
                        (int32_t)w, (int32_t)h));
  const hrt_tile centre = {w / 2, h / 2, 1, 1};
  hrt_ray ray;
  hrt_hit hit;
  CHECK(hrt_camera_rays_host(s, &pinhole, &p, &centre, 1, &ray));
  hrt_query_params q = {0};
  q.time0 = pinhole.time0;
  q.time1 = pinhole.time1;
  q.seed = p.seed;
  CHECK(hrt_scene_intersect_host(s, &q, &ray, 1, &hit));
  if (!(hit.flags & HRT_HIT_HIT)) {
    fprintf(stderr, "the centre pixel sees the sky: nothing to focus on\n");
    return 1;
  }
  const float* d = ray.direction;
  const float depth = hit.t * sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);

  /* the frame, focused there */
  hrt_camera cam;
  CHECK(hrt_camera_init(&cam, info.look_from, info.look_at, info.fov, info.aperture, depth, info.time0, info.time1, (int32_t)w,
                        (int32_t)h));
  p.samples = spp;
  float* rgba = (float*)malloc(sizeof(float) * 4 * (size_t)w * h);
  if (!rgba) return 1;
  CHECK(hrt_render(s, &cam, &p, 0, 0, w, h, rgba, NULL));
  CHECK(hrt_image_write(path, rgba, w, h, HRT_IMAGE_PFM));
  uint64_t sum = 0xCBF29CE484222325ull;
  const unsigned char* bytes = (const unsigned char*)rgba;
  for (size_t i = 0; i < sizeof(float) * 4 * (size_t)w * h; i++) sum = (sum ^ bytes[i]) * 0x100000001B3ull;
  printf("prim %u material %u depth %.9g checksum %016llx -> %s\n", hit.prim, hit.material, (double)depth, (unsigned long long)sum,
         path);
  free(rgba);
  hrt_scene_destroy(s);
  return 0;
}
