/*
 * render_resume.c — checkpoint and resume of a noise-driven refinement on the C ABI alone.  The policy is
 * render_adaptive.c's: one pass over every tile, then passes over the tiles whose mean relative error is still above the
 * target.  It runs twice on the random-spheres scene: once uninterrupted, and once stopped after two rounds, where the
 * whole accumulator state (sums, noise plane, each tile's sample ranges and chunk count) goes to a file
 * (hrt_accum_snapshot) and the accumulator is destroyed; a new one is created from what the file says
 * (hrt_accum_snapshot_info), restored (hrt_accum_restore) and refined to the end.  A tile's k-th pass is always samples
 * [k * pass_spp, (k + 1) * pass_spp), so the resumed run must give the uninterrupted run's frame and per-tile sample
 * counts bit for bit; the program says whether it does and exits non-zero if not.
 *
 *   make -C examples && ./examples/render_resume 64 36 16 40 0.05 400 resume.hrts
 *                                                W  H tile spp/pass target max_spp checkpoint
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

typedef struct {
  hrt_camera cam;
  hrt_render_params p; /* p.samples: the pass's spp */
  float target, floor;
  uint32_t max_spp;
} policy;

/* Refinement rounds on `acc` until no tile is left or `max_rounds` rounds ran (0: no limit).  Every round looks at the
 * noise records first when the accumulator holds samples, so a restored accumulator goes on where it stopped: the tiles
 * still above the target that hold n samples take samples [n, n + spp), one pass per distinct n. */
static int refine(hrt_accum* acc, const policy* po, uint32_t n_tiles, uint32_t max_rounds, uint32_t* rounds_out) {
  hrt_render_params p = po->p;
  hrt_tile_noise* noise = (hrt_tile_noise*)malloc(sizeof(hrt_tile_noise) * n_tiles);
  uint64_t* held = (uint64_t*)malloc(sizeof(uint64_t) * n_tiles);
  uint32_t* todo = (uint32_t*)malloc(sizeof(uint32_t) * n_tiles);
  uint8_t* want = (uint8_t*)malloc(n_tiles);
  if (!noise || !held || !todo || !want) return 1;
  uint32_t rounds = 0;
  for (;;) {
    CHECK(hrt_accum_tile_samples(acc, held));
    int any = 0;
    for (uint32_t t = 0; t < n_tiles; t++) any |= held[t] != 0;
    if (!any) { /* the first pass: every tile */
      p.sample_offset = 0;
      CHECK(hrt_accum_add(acc, &po->cam, &p, NULL, NULL));
    } else {
      CHECK(hrt_accum_noise(acc, po->floor, NULL, NULL, noise));
      uint32_t n_want = 0;
      for (uint32_t t = 0; t < n_tiles; t++) {
        want[t] = noise[t].mean > po->target && noise[t].samples < po->max_spp;
        n_want += want[t];
      }
      if (n_want == 0) break;
      while (n_want > 0) { /* one pass per distinct sample count, ascending */
        uint64_t least = UINT64_MAX;
        for (uint32_t t = 0; t < n_tiles; t++)
          if (want[t] && held[t] < least) least = held[t];
        uint32_t n_todo = 0;
        for (uint32_t t = 0; t < n_tiles; t++)
          if (want[t] && held[t] == least) todo[n_todo++] = t, want[t] = 0;
        p.sample_offset = (uint32_t)least;
        CHECK(hrt_accum_add_tiles(acc, &po->cam, &p, todo, n_todo, NULL, NULL));
        n_want -= n_todo;
      }
    }
    rounds++;
    if (max_rounds && rounds == max_rounds) break;
  }
  if (rounds_out) *rounds_out = rounds;
  free(noise);
  free(held);
  free(todo);
  free(want);
  return 0;
}

int main(int argc, char** argv) {
  uint32_t w = argc > 1 ? (uint32_t)atoi(argv[1]) : 64;
  uint32_t h = argc > 2 ? (uint32_t)atoi(argv[2]) : 36;
  uint32_t tile = argc > 3 ? (uint32_t)atoi(argv[3]) : 16;
  uint32_t pass_spp = argc > 4 ? (uint32_t)atoi(argv[4]) : 40;
  float target = argc > 5 ? (float)atof(argv[5]) : 0.05f;
  uint32_t max_spp = argc > 6 ? (uint32_t)atoi(argv[6]) : 400;
  const char* path = argc > 7 ? argv[7] : "resume.hrts";

  hrt_scene* s = NULL;
  hrt_preset_info info;
  CHECK(hrt_scene_create(&s));
  CHECK(hrt_preset_build(s, HRT_PRESET_RANDOM, 1, NULL, 0, 0, 0, &info));
  CHECK(hrt_scene_commit(s, 0));
  policy po;
  memset(&po, 0, sizeof(po));
  CHECK(hrt_camera_init(&po.cam, info.look_from, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0,
                        info.time1, (int32_t)w, (int32_t)h));
  po.p.width = w;
  po.p.height = h;
  po.p.samples = pass_spp;
  po.p.max_depth = 50;
  po.p.t_min = 0.001f;
  po.p.background[0] = info.background[0];
  po.p.background[1] = info.background[1];
  po.p.background[2] = info.background[2];
  po.p.seed = 1;
  po.target = target;
  po.floor = 0.05f;
  po.max_spp = max_spp;

  uint32_t n_tiles = 0;
  CHECK(hrt_tile_grid(w, h, tile, 0, 1, NULL, 0, &n_tiles));
  hrt_tile* tiles = (hrt_tile*)malloc(sizeof(hrt_tile) * n_tiles);
  if (!tiles) return 1;
  CHECK(hrt_tile_grid(w, h, tile, 0, 1, tiles, n_tiles, &n_tiles));
  const size_t frame_bytes = sizeof(float) * 4 * (size_t)w * h;
  float* whole = (float*)malloc(frame_bytes);
  float* resumed = (float*)malloc(frame_bytes);
  uint64_t* held_whole = (uint64_t*)malloc(sizeof(uint64_t) * n_tiles);
  uint64_t* held_resumed = (uint64_t*)malloc(sizeof(uint64_t) * n_tiles);
  if (!whole || !resumed || !held_whole || !held_resumed) return 1;

  /* 1. uninterrupted */
  hrt_accum* acc = NULL;
  uint32_t rounds_whole = 0, rounds_after = 0;
  CHECK(hrt_accum_create_ex(s, w, h, tiles, n_tiles, HRT_ACCUM_NOISE, &acc));
  if (refine(acc, &po, n_tiles, 0, &rounds_whole)) return 1;
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, whole));
  CHECK(hrt_accum_tile_samples(acc, held_whole));
  hrt_accum_destroy(acc);

  /* 2. two rounds, then the state goes to a file and the accumulator away */
  CHECK(hrt_accum_create_ex(s, w, h, tiles, n_tiles, HRT_ACCUM_NOISE, &acc));
  if (refine(acc, &po, n_tiles, 2, NULL)) return 1;
  uint64_t size = 0;
  CHECK(hrt_accum_snapshot(acc, NULL, 0, &size));
  void* blob = malloc((size_t)size);
  if (!blob) return 1;
  CHECK(hrt_accum_snapshot(acc, blob, size, &size));
  hrt_accum_destroy(acc);
  acc = NULL;
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(blob, 1, (size_t)size, f) != (size_t)size || fclose(f) != 0) {
    fprintf(stderr, "cannot write %s\n", path);
    return 1;
  }
  free(blob);

  /* 3. a new accumulator from what the file says, restored and refined to the end */
  f = fopen(path, "rb");
  if (!f || fseek(f, 0, SEEK_END) != 0) return 1;
  const long file_size = ftell(f);
  rewind(f);
  blob = malloc((size_t)file_size);
  if (file_size <= 0 || !blob || fread(blob, 1, (size_t)file_size, f) != (size_t)file_size) return 1;
  fclose(f);
  hrt_snapshot_info si;
  CHECK(hrt_accum_snapshot_info(blob, (uint64_t)file_size, &si, NULL, 0));
  hrt_tile* saved_tiles = (hrt_tile*)malloc(sizeof(hrt_tile) * si.n_tiles);
  if (!saved_tiles) return 1;
  CHECK(hrt_accum_snapshot_info(blob, (uint64_t)file_size, &si, saved_tiles, si.n_tiles));
  CHECK(hrt_accum_create_ex(s, si.width, si.height, saved_tiles, si.n_tiles, si.flags, &acc));
  CHECK(hrt_accum_restore(acc, blob, (uint64_t)file_size));
  free(blob);
  if (refine(acc, &po, si.n_tiles, 0, &rounds_after)) return 1;
  CHECK(hrt_accum_resolve_host(acc, HRT_ACCUM_F32, resumed));
  CHECK(hrt_accum_tile_samples(acc, held_resumed));
  hrt_accum_destroy(acc);

  const int same_frame = memcmp(whole, resumed, frame_bytes) == 0;
  const int same_samples = si.n_tiles == n_tiles && memcmp(held_whole, held_resumed, sizeof(uint64_t) * n_tiles) == 0;
  printf("samples per tile:");
  for (uint32_t t = 0; t < n_tiles; t++) printf(" %llu", (unsigned long long)held_resumed[t]);
  printf("\n%ux%u in %u tiles: %u rounds uninterrupted; 2 rounds, a checkpoint of %llu bytes (%s), %u more rounds\n", w, h,
         n_tiles, rounds_whole, (unsigned long long)file_size, si.uniform ? "tiles alike" : "tiles differ", rounds_after);
  printf("frame: %s, samples per tile: %s\n", same_frame ? "identical" : "DIFFERENT", same_samples ? "identical" : "DIFFERENT");
  free(tiles);
  free(saved_tiles);
  free(whole);
  free(resumed);
  free(held_whole);
  free(held_resumed);
  hrt_scene_destroy(s);
  return same_frame && same_samples ? 0 : 1;
}
