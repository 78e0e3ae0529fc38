/*
 * render_accum_wavefront.c — a wavefront integrator that ends in an accumulator, on the C ABI: render_wavefront.c's loop
 * (hrt_camera_paths, then hrt_scene_step over two live lists on the device) in passes of PASS_SPP samples per pixel,
 * each pass deposited with hrt_accum_add_paths into an HRT_ACCUM_NOISE accumulator, which after the last pass resolves
 * through the variance-guided filter.  No path is downloaded and nothing is summed on the host.
 * The same passes then go through hrt_accum_add into a second accumulator, and the program exits non-zero unless the
 * two hold the same raw sums and resolve to the same filtered frame, byte for byte: hrt_accum_add_paths leaves an
 * accumulator where the render leaves it, so everything downstream of the sums cannot tell the two routes apart.
 * The HIP runtime is used for the buffers alone (hipMalloc, hipMemcpy, hipMemset, hipFree).
 *
 *   make -C examples && ./examples/render_accum_wavefront 256 144 4 wavefront_accum.pfm
 *                                                          W   H  passes
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include "hrt/hrt.h"

#define PASS_SPP 4    /* samples per pixel and pass: the batch holds W x H x PASS_SPP paths */
#define STEPS 2       /* rounds per hrt_scene_step call */
#define CHECK_EVERY 4 /* calls between two looks at the live count */
#define MAX_RANGES 8  /* sample ranges hrt_accum_download may report */

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
  uint32_t n_passes = argc > 3 ? (uint32_t)atoi(argv[3]) : 4;
  const char* path = argc > 4 ? argv[4] : "wavefront_accum.pfm";

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
  p.samples = PASS_SPP;
  p.max_depth = 50;
  p.t_min = 0.001f;
  p.seed = 1;
  hrt_step_params sp = {0};
  sp.steps = STEPS;
  sp.time0 = cam.time0;
  sp.time1 = cam.time1;
  sp.seed = p.seed;
  for (int c = 0; c < 3; c++) p.background[c] = sp.background[c] = info.background[c];
  hrt_filter_params filter = {3, 4.0f};

  const size_t n_px = (size_t)w * h, n = n_px * PASS_SPP;
  const hrt_tile frame = {0, 0, w, h};
  hrt_accum *acc = NULL, *rendered = NULL;
  CHECK(hrt_accum_create_ex(s, w, h, &frame, 1, HRT_ACCUM_NOISE, &acc));
  CHECK(hrt_accum_create_ex(s, w, h, &frame, 1, HRT_ACCUM_NOISE, &rendered));
  hrt_ray* d_rays = NULL;
  hrt_path* d_paths = NULL;
  uint64_t* d_n_rays = NULL;
  uint32_t* d_unfinished = NULL;
  hrt_path_list lists[2] = {{NULL, NULL, (uint32_t)n, 0}, {NULL, NULL, (uint32_t)n, 0}};
  HIP(hipMalloc((void**)&d_rays, n * sizeof(hrt_ray)));
  HIP(hipMalloc((void**)&d_paths, n * sizeof(hrt_path)));
  HIP(hipMalloc((void**)&d_n_rays, sizeof(uint64_t)));
  HIP(hipMemset(d_n_rays, 0, sizeof(uint64_t)));
  HIP(hipMalloc((void**)&d_unfinished, sizeof(uint32_t)));
  HIP(hipMemset(d_unfinished, 0, sizeof(uint32_t)));
  for (int i = 0; i < 2; i++) {
    HIP(hipMalloc((void**)&lists[i].d_index, n * sizeof(uint32_t)));
    HIP(hipMalloc((void**)&lists[i].d_count, sizeof(uint32_t)));
  }

  const uint32_t calls = (p.max_depth + STEPS - 1) / STEPS;
  unsigned long long rendered_rays = 0;
  for (uint32_t k = 0; k < n_passes; k++) {
    p.sample_offset = k * PASS_SPP;
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
    /* the pass: one kernel that reads the batch and adds to the sums and the noise plane */
    CHECK(hrt_accum_add_paths(acc, &cam, &p, NULL, 0, d_paths, n, -1, NULL, d_unfinished, NULL));
    hrt_render_stats stats;
    CHECK(hrt_accum_add(rendered, &cam, &p, NULL, &stats));
    rendered_rays += stats.segments;
  }
  unsigned long long n_rays = 0;
  uint32_t unfinished = 0;
  HIP(hipMemcpy(&n_rays, d_n_rays, sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(&unfinished, d_unfinished, sizeof(uint32_t), hipMemcpyDeviceToHost));

  /* the two routes: raw sums, sample ranges, then the filtered frames */
  float* sums[2] = {(float*)malloc(16 * n_px), (float*)malloc(16 * n_px)};
  float* rgba[2] = {(float*)malloc(16 * n_px), (float*)malloc(16 * n_px)};
  if (!sums[0] || !sums[1] || !rgba[0] || !rgba[1]) return 1;
  hrt_accum* both[2] = {acc, rendered};
  uint32_t ranges[2][2 * MAX_RANGES], n_ranges[2] = {0, 0};
  memset(ranges, 0, sizeof(ranges));
  for (int i = 0; i < 2; i++) {
    CHECK(hrt_accum_download(both[i], sums[i], ranges[i], MAX_RANGES, &n_ranges[i]));
    if (n_ranges[i] > MAX_RANGES) return 1; /* consecutive passes are one range */
    CHECK(hrt_accum_resolve_filtered_host(both[i], &filter, HRT_ACCUM_F32, rgba[i]));
  }
  const int same = unfinished == 0 && n_rays == rendered_rays && n_ranges[0] == n_ranges[1] &&
                   memcmp(ranges[0], ranges[1], sizeof(ranges[0])) == 0 && memcmp(sums[0], sums[1], 16 * n_px) == 0 &&
                   memcmp(rgba[0], rgba[1], 16 * n_px) == 0;
  CHECK(hrt_image_write(path, rgba[0], w, h, HRT_IMAGE_PFM));
  printf("rays %llu rendered %llu unfinished %u: the two accumulators %s -> %s\n", n_rays, rendered_rays, unfinished,
         same ? "agree" : "DIFFER", path);
  for (int i = 0; i < 2; i++) {
    free(sums[i]);
    free(rgba[i]);
    (void)hipFree(lists[i].d_index);
    (void)hipFree(lists[i].d_count);
  }
  (void)hipFree(d_unfinished);
  (void)hipFree(d_n_rays);
  (void)hipFree(d_paths);
  (void)hipFree(d_rays);
  hrt_accum_destroy(acc);
  hrt_accum_destroy(rendered);
  hrt_scene_destroy(s);
  return same ? 0 : 2;
}
