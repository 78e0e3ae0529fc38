/*
 * render_wavefront.c — a wavefront integrator on the C ABI: the `random` preset rendered through hrt_camera_paths and
 * hrt_scene_step, on device buffers and live lists the host never reads between the rounds.
 * For every sample index k: hrt_camera_paths starts one path per pixel; then hrt_scene_step makes STEPS rounds of
 * intersect-and-scatter per call over the paths of the `in` list and writes those still live into the `out` list, the
 * two lists trading places from call to call.  The live count is read back every CHECK_EVERY calls only, and the ray
 * count stays on the device until the frame is done.  A path's radiance is the render's sample bit for bit, so the sums
 * follow the accumulator contract (a one-sample pass is added as acc = acc + pass_sum) and the frame is
 * sqrtf(acc * (1.0f / samples)): what an hrt_accum fed the same one-sample passes resolves to.
 * The HIP runtime is used for the buffers alone (hipMalloc, hipMemcpy, hipMemset, hipFree).
 * Prints the rays traced and a checksum of the frame (FNV-1a over its bytes).
 *
 *   make -C examples && ./examples/render_wavefront 256 144 16 wavefront.pfm
 *                                                    W   H  spp
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include "hrt/hrt.h"

#define STEPS 2       /* rounds per hrt_scene_step call */
#define CHECK_EVERY 4 /* calls between two looks at the live count */

#define CHECK(call)                                                                       \
  do {                                                                                    \
    hrt_status st_ = (call);                                                              \
    if (st_ != HRT_OK) {                                                                  \
      fprintf(stderr, "%s failed (status %d): %s\n", #call, (int)st_, hrt_last_error());  \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)
#define HIP(call)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));                   \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

int main(int argc, char** argv) {
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 256;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 144;
  uint32_t spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
  const char* path = argc > 4 ? argv[4] : "wavefront.pfm";

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
  hrt_step_params sp = {0};
  sp.steps = STEPS;
  sp.time0 = cam.time0;
  sp.time1 = cam.time1;
  sp.seed = p.seed;
  for (int c = 0; c < 3; c++) p.background[c] = sp.background[c] = info.background[c];

  const size_t n = (size_t)w * h;
  const hrt_tile frame = {0, 0, w, h};
  hrt_ray* d_rays = NULL;
  hrt_path* d_paths = NULL;
  uint64_t* d_n_rays = NULL;
  hrt_path_list lists[2] = {{NULL, NULL, (uint32_t)n, 0}, {NULL, NULL, (uint32_t)n, 0}};
  HIP(hipMalloc((void**)&d_rays, n * sizeof(hrt_ray)));
  HIP(hipMalloc((void**)&d_paths, n * sizeof(hrt_path)));
  HIP(hipMalloc((void**)&d_n_rays, sizeof(uint64_t)));
  HIP(hipMemset(d_n_rays, 0, sizeof(uint64_t)));
  for (int i = 0; i < 2; i++) {
    HIP(hipMalloc((void**)&lists[i].d_index, n * sizeof(uint32_t)));
    HIP(hipMalloc((void**)&lists[i].d_count, sizeof(uint32_t)));
  }
  hrt_path* paths = (hrt_path*)malloc(n * sizeof(hrt_path));
  float* rgba = (float*)calloc(4 * n, sizeof(float)); /* the sums, then the frame */
  if (!paths || !rgba) return 1;

  const uint32_t calls = (p.max_depth + STEPS - 1) / STEPS;
  for (uint32_t k = 0; k < spp; k++) {
    p.sample_offset = k;
    CHECK(hrt_camera_paths(s, &cam, &p, &frame, 1, d_rays, d_paths, NULL));
    const hrt_path_list* in = NULL; /* the first call takes every path */
    for (uint32_t call = 0; call < calls; call++) {
      const hrt_path_list* out = &lists[call & 1];
      CHECK(hrt_scene_step(s, &sp, d_rays, d_paths, n, NULL, in, out, d_n_rays, NULL));
      in = out;
      if ((call + 1) % CHECK_EVERY == 0) {
        uint32_t live = 0;
        HIP(hipMemcpy(&live, out->d_count, sizeof(live), hipMemcpyDeviceToHost));
        if (live == 0) break;
      }
    }
    HIP(hipMemcpy(paths, d_paths, n * sizeof(hrt_path), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
      for (int c = 0; c < 3; c++) rgba[4 * i + c] = rgba[4 * i + c] + paths[i].radiance[c];
  }
  unsigned long long n_rays = 0;
  HIP(hipMemcpy(&n_rays, d_n_rays, sizeof(uint64_t), hipMemcpyDeviceToHost));
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
  free(paths);
  free(rgba);
  for (int i = 0; i < 2; i++) {
    (void)hipFree(lists[i].d_index);
    (void)hipFree(lists[i].d_count);
  }
  (void)hipFree(d_n_rays);
  (void)hipFree(d_paths);
  (void)hipFree(d_rays);
  hrt_scene_destroy(s);
  return 0;
}
