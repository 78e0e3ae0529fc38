/*
 * threads.c — TEST INFRASTRUCTURE ONLY: the re-entrancy contract of hrt.h (rendering, the ray queries and hrt_scene_step
 * are re-entrant per scene; different accumulators of a scene may be used from different threads; hrt_last_error and
 * hrt_last_launch are per thread), driven from 8 pthreads through the C ABI.  The HIP runtime is used for device buffers
 * and streams alone.  tests/test_gpu_threads.py builds and runs it.
 *
 *   threads OUT_DIR
 *
 * Serial phase: every job of the table runs once on the main thread and its outputs, stats (segments, samples, pixels),
 * hrt_last_launch().kernel and, for the refused calls, status and hrt_last_error() text are kept.  The serial frames of
 * the render jobs go to OUT_DIR as PFM, where the Python test holds them to the oracle.
 * Concurrent phase: one thread per job, released together by a barrier, ROUNDS times; after its job a thread compares
 * everything it produced with the serial record, byte for byte.  One line per job and round; exit 1 on any difference.
 *
 * The work is bounded: ROUNDS, the jobs and the launches per job are constants (57 launches per run of the table, 228
 * in all), and no loop waits for anything to happen.
 *
 *   R1  random   hrt_render 64x36, 8 spp, the preset camera, stats (synchronous: holds the slot mutex while it waits)
 *   R2  random   hrt_render of a 37x19 frame, one call per 16-px tile, a second camera, stats
 *   R3  random   hrt_render_tiles_device on the thread's stream, no stats: one 1920x1080 frame (the only large input: a
 *                few milliseconds on the GPU, so the others find a launch in flight), three 64x36 frames from a third
 *                camera, hrt_scene_synchronize
 *   R4  cornell  hrt_render 32x32, 8 spp, stats: the general kernel, while R1's thread reports the sphere kernel
 *   A1  random   an accumulator with a noise plane, 64x36 in 16-px tiles: hrt_accum_add at offsets 0, 16, 32, then
 *                resolve_host, noise, resolve_filtered_host
 *   A2  random   an accumulator with a ragged three-tile split: a full pass, hrt_accum_add_tiles over two tiles, snapshot,
 *                restore into a third accumulator, both resolved
 *   Q1  random   hrt_camera_paths (64x36, 2 samples), the intersect + scatter loop to the depth cap, then on fresh paths
 *                the hrt_scene_step loop over live lists (steps = 2).  The cap is Q1_DEPTH = 12, not the renders' 50: 32
 *                launches per run instead of 127, which keeps the whole run under 300
 *   L1  its own  three times: create, two_spheres, commit, hrt_render 16x16 at 4 spp, destroy; between them two calls on
 *                `random` that are refused before any device work (a tile outside the image, a width of 1)
 * So six threads launch on the one `random` scene (more callers than the 4 launch slots), three cameras render through
 * its leaf lists at once, two threads run passes on different accumulators of it, one thread commits and destroys a
 * scene meanwhile, and two kernels report through hrt_last_launch on two threads.
 */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include "hrt/hrt.h"

#define ROUNDS 3
#define N_JOBS 8
#define MAX_OUT 4
#define MAX_STATS 2
#define MAX_REFUSED 4
#define N_DEV 7
#define Q1_DEPTH 12
#define Q1_STEPS 2

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
#define NEED(cond)                                       \
  do {                                                   \
    if (!(cond)) {                                       \
      fprintf(stderr, "%s does not hold\n", #cond);      \
      return 1;                                          \
    }                                                    \
  } while (0)

/* what one run of a job produced */
typedef struct Result {
  void* out[MAX_OUT];
  size_t bytes[MAX_OUT];
  int n_out;
  uint64_t stats[MAX_STATS][3]; /* segments, samples, pixels */
  int n_stats;
  char kernel[160];
  int32_t refused_status[MAX_REFUSED];
  char refused_text[MAX_REFUSED][256];
  int n_refused;
} Result;

typedef struct Job Job;
struct Job {
  const char* name;
  int (*run)(Job*, Result*);
  hipStream_t stream;
  void* dev[N_DEV]; /* device buffers, made at the first (serial) run and reused */
  Result serial;
  int bad; /* rounds that failed or differed */
};

/* the committed scenes and the cameras, read-only once the serial phase begins */
static struct {
  hrt_scene *random, *cornell;
  hrt_preset_info ri, ci;
  hrt_camera cam0;      /* random, the preset camera, 64x36 */
  hrt_camera cam1;      /* random, a second look_from, 37x19 */
  hrt_camera cam2;      /* random, a third look_from, 64x36 */
  hrt_camera cam2_big;  /* ... at 1920x1080 */
  hrt_camera cam_box;   /* cornell, 32x32 */
} S;
static const float LOOK_FROM_1[3] = {10.0f, 3.0f, 5.0f};
static const float LOOK_FROM_2[3] = {12.0f, 1.5f, -2.0f};
static pthread_barrier_t g_barrier;

static hrt_render_params params(const hrt_preset_info* info, uint32_t w, uint32_t h, uint32_t spp, uint32_t offset) {
  hrt_render_params p;
  memset(&p, 0, sizeof(p));
  p.width = w;
  p.height = h;
  p.samples = spp;
  p.max_depth = 50;
  p.sample_offset = offset;
  p.t_min = 0.001f;
  p.seed = 1;
  for (int c = 0; c < 3; c++) p.background[c] = info->background[c];
  return p;
}

static int put(Result* r, const void* data, size_t bytes) {
  if (r->n_out == MAX_OUT) return 1;
  void* copy = malloc(bytes ? bytes : 1);
  if (!copy) return 1;
  memcpy(copy, data, bytes);
  r->out[r->n_out] = copy;
  r->bytes[r->n_out++] = bytes;
  return 0;
}
static void put_stats(Result* r, const hrt_render_stats* st) {
  r->stats[r->n_stats][0] = st->segments;
  r->stats[r->n_stats][1] = st->samples;
  r->stats[r->n_stats++][2] = st->pixels;
}
static void put_refused(Result* r, hrt_status st) {
  r->refused_status[r->n_refused] = st;
  snprintf(r->refused_text[r->n_refused++], 256, "%s", hrt_last_error());
}
static int put_kernel(Result* r) {
  hrt_launch_info li;
  CHECK(hrt_last_launch(&li));
  snprintf(r->kernel, sizeof(r->kernel), "%s", li.kernel);
  return 0;
}
static void result_free(Result* r) {
  for (int i = 0; i < r->n_out; i++) free(r->out[i]);
  memset(r, 0, sizeof(*r));
}
/* NULL when equal, else what differs first */
static const char* result_diff(const Result* a, const Result* b) {
  if (a->n_out != b->n_out) return "the number of outputs";
  for (int i = 0; i < a->n_out; i++)
    if (a->bytes[i] != b->bytes[i] || memcmp(a->out[i], b->out[i], a->bytes[i]) != 0) return "an output's bytes";
  if (a->n_stats != b->n_stats || memcmp(a->stats, b->stats, sizeof(a->stats)) != 0) return "the stats";
  if (strcmp(a->kernel, b->kernel) != 0) return "the kernel of hrt_last_launch";
  if (a->n_refused != b->n_refused) return "the number of refused calls";
  for (int i = 0; i < a->n_refused; i++)
    if (a->refused_status[i] != b->refused_status[i] || strcmp(a->refused_text[i], b->refused_text[i]) != 0)
      return "a refused call's status or hrt_last_error text";
  return NULL;
}
static void* dev(Job* j, int k, size_t bytes) {
  if (!j->dev[k] && hipMalloc(&j->dev[k], bytes) != hipSuccess) j->dev[k] = NULL;
  return j->dev[k];
}

/* ---- the jobs ---- */
static int job_r1(Job* j, Result* r) {
  (void)j;
  float img[64 * 36 * 4];
  hrt_render_params p = params(&S.ri, 64, 36, 8, 0);
  hrt_render_stats st;
  memset(&st, 0, sizeof(st));
  CHECK(hrt_render(S.random, &S.cam0, &p, 0, 0, 64, 36, img, &st));
  put_stats(r, &st);
  if (put_kernel(r)) return 1;
  return put(r, img, sizeof(img));
}

static int job_r2(Job* j, Result* r) {
  (void)j;
  enum { W = 37, H = 19, T = 16 };
  float frame[W * H * 4], tile[T * T * 4];
  hrt_tile tiles[8];
  uint32_t n = 0;
  CHECK(hrt_tile_grid(W, H, T, 0, 1, tiles, 8, &n));
  NEED(n == 6);
  hrt_render_params p = params(&S.ri, W, H, 8, 0);
  hrt_render_stats sum;
  memset(&sum, 0, sizeof(sum));
  for (uint32_t i = 0; i < n; i++) {
    const hrt_tile t = tiles[i];
    hrt_render_stats st;
    memset(&st, 0, sizeof(st));
    CHECK(hrt_render(S.random, &S.cam1, &p, t.x, t.y, t.w, t.h, tile, &st));
    for (uint32_t y = 0; y < t.h; y++)
      memcpy(&frame[((size_t)(t.y + y) * W + t.x) * 4], &tile[(size_t)y * t.w * 4], (size_t)t.w * 16);
    sum.segments += st.segments;
    sum.samples += st.samples;
    sum.pixels += st.pixels;
  }
  put_stats(r, &sum);
  if (put_kernel(r)) return 1;
  return put(r, frame, sizeof(frame));
}

static int job_r3(Job* j, Result* r) {
  enum { BW = 1920, BH = 1080, W = 64, H = 36, FRAMES = 3 };
  const size_t big_bytes = (size_t)BW * BH * 16, small_bytes = (size_t)W * H * 16;
  float* d_big = (float*)dev(j, 0, big_bytes);
  float* d_small = (float*)dev(j, 1, FRAMES * small_bytes);
  NEED(d_big && d_small);
  const hrt_tile big = {0, 0, BW, BH}, small = {0, 0, W, H};
  hrt_render_params p = params(&S.ri, BW, BH, 8, 0);
  CHECK(hrt_render_tiles_device(S.random, &S.cam2_big, &p, &big, 1, d_big, j->stream, NULL));
  for (uint32_t k = 0; k < FRAMES; k++) {
    p = params(&S.ri, W, H, 8, 8 * k);
    CHECK(hrt_render_tiles_device(S.random, &S.cam2, &p, &small, 1, d_small + k * (small_bytes / 4), j->stream, NULL));
  }
  if (put_kernel(r)) return 1;
  CHECK(hrt_scene_synchronize(S.random));
  void* host = malloc(big_bytes);
  NEED(host);
  HIP(hipMemcpy(host, d_big, big_bytes, hipMemcpyDeviceToHost));
  int rc = put(r, host, big_bytes);
  HIP(hipMemcpy(host, d_small, FRAMES * small_bytes, hipMemcpyDeviceToHost));
  rc = rc || put(r, host, FRAMES * small_bytes);
  free(host);
  return rc;
}

static int job_r4(Job* j, Result* r) {
  (void)j;
  float img[32 * 32 * 4];
  hrt_render_params p = params(&S.ci, 32, 32, 8, 0);
  hrt_render_stats st;
  memset(&st, 0, sizeof(st));
  CHECK(hrt_render(S.cornell, &S.cam_box, &p, 0, 0, 32, 32, img, &st));
  put_stats(r, &st);
  if (put_kernel(r)) return 1;
  return put(r, img, sizeof(img));
}

static int job_a1(Job* j, Result* r) {
  enum { W = 64, H = 36, N_TILES = 12 };
  static float frame[W * H * 4]; /* one thread runs this job */
  hrt_tile tiles[N_TILES];
  uint32_t n = 0;
  CHECK(hrt_tile_grid(W, H, 16, 0, 1, tiles, N_TILES, &n));
  NEED(n == N_TILES);
  hrt_accum* a = NULL;
  CHECK(hrt_accum_create_ex(S.random, W, H, tiles, n, HRT_ACCUM_NOISE, &a));
  for (uint32_t k = 0; k < 3; k++) {
    hrt_render_params p = params(&S.ri, W, H, 16, 16 * k);
    hrt_render_stats st;
    memset(&st, 0, sizeof(st));
    CHECK(hrt_accum_add(a, &S.cam0, &p, j->stream, k == 0 ? &st : NULL));
    if (k == 0) put_stats(r, &st);
  }
  if (put_kernel(r)) return 1;
  CHECK(hrt_accum_resolve_host(a, HRT_ACCUM_F32, frame));
  if (put(r, frame, sizeof(frame))) return 1;
  hrt_tile_noise recs[N_TILES];
  memset(recs, 0, sizeof(recs));
  CHECK(hrt_accum_noise(a, 0.05f, NULL, j->stream, recs));
  if (put(r, recs, sizeof(recs))) return 1;
  const hrt_filter_params f = {3, 4.0f};
  CHECK(hrt_accum_resolve_filtered_host(a, &f, HRT_ACCUM_F32, frame));
  if (put(r, frame, sizeof(frame))) return 1;
  hrt_accum_destroy(a);
  return 0;
}

static int job_a2(Job* j, Result* r) {
  enum { W = 64, H = 36 };
  static float frame_a[W * H * 4], frame_b[W * H * 4]; /* one thread runs this job */
  const hrt_tile tiles[3] = {{0, 0, 40, 36}, {40, 0, 24, 20}, {40, 20, 24, 16}};
  const uint32_t two[2] = {0, 2};
  hrt_accum *a = NULL, *b = NULL;
  CHECK(hrt_accum_create(S.random, W, H, tiles, 3, &a));
  hrt_render_params p = params(&S.ri, W, H, 8, 0);
  CHECK(hrt_accum_add(a, &S.cam0, &p, j->stream, NULL));
  p.sample_offset = 8;
  hrt_render_stats st;
  memset(&st, 0, sizeof(st));
  CHECK(hrt_accum_add_tiles(a, &S.cam0, &p, two, 2, j->stream, &st));
  put_stats(r, &st);
  if (put_kernel(r)) return 1;
  uint64_t size = 0;
  CHECK(hrt_accum_snapshot(a, NULL, 0, &size));
  void* blob = malloc(size);
  NEED(blob);
  CHECK(hrt_accum_snapshot(a, blob, size, &size));
  CHECK(hrt_accum_create(S.random, W, H, tiles, 3, &b));
  CHECK(hrt_accum_restore(b, blob, size));
  int rc = put(r, blob, size);
  free(blob);
  CHECK(hrt_accum_resolve_host(a, HRT_ACCUM_F32, frame_a));
  CHECK(hrt_accum_resolve_host(b, HRT_ACCUM_F32, frame_b));
  NEED(memcmp(frame_a, frame_b, sizeof(frame_a)) == 0); /* the restore contract */
  rc = rc || put(r, frame_a, sizeof(frame_a)) || put(r, frame_b, sizeof(frame_b));
  hrt_accum_destroy(b);
  hrt_accum_destroy(a);
  return rc;
}

static int cmp_u32(const void* a, const void* b) {
  const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return x < y ? -1 : x > y;
}

static int job_q1(Job* j, Result* r) {
  enum { W = 64, H = 36, SPP = 2, N = W * H * SPP };
  static hrt_path paths_a[N], paths_b[N]; /* one thread runs this job */
  static uint32_t live[N + 1];
  hrt_ray* d_rays = (hrt_ray*)dev(j, 0, N * sizeof(hrt_ray));
  hrt_path* d_paths = (hrt_path*)dev(j, 1, N * sizeof(hrt_path));
  hrt_hit* d_hits = (hrt_hit*)dev(j, 2, N * sizeof(hrt_hit));
  uint32_t* d_index = (uint32_t*)dev(j, 3, 2 * N * sizeof(uint32_t));
  uint32_t* d_count = (uint32_t*)dev(j, 4, 4 * sizeof(uint32_t)); /* the two lists' counts, the kept list's */
  uint32_t* d_kept = (uint32_t*)dev(j, 5, N * sizeof(uint32_t));
  uint64_t* d_n_rays = (uint64_t*)dev(j, 6, sizeof(uint64_t));
  NEED(d_rays && d_paths && d_hits && d_index && d_count && d_kept && d_n_rays);
  const hrt_tile frame = {0, 0, W, H};
  hrt_render_params p = params(&S.ri, W, H, SPP, 0);
  p.max_depth = Q1_DEPTH;
  hrt_query_params q;
  memset(&q, 0, sizeof(q));
  q.time0 = S.cam0.time0;
  q.time1 = S.cam0.time1;
  q.seed = p.seed;
  hrt_scatter_params sc;
  memset(&sc, 0, sizeof(sc));
  hrt_step_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.steps = Q1_STEPS;
  sp.time0 = q.time0;
  sp.time1 = q.time1;
  sp.seed = p.seed;
  for (int c = 0; c < 3; c++) sc.background[c] = sp.background[c] = p.background[c];

  /* the two calls in turn, Q1_DEPTH rounds: every path is DONE afterwards */
  CHECK(hrt_camera_paths(S.random, &S.cam0, &p, &frame, 1, d_rays, d_paths, j->stream));
  for (int round = 0; round < Q1_DEPTH; round++) {
    CHECK(hrt_scene_intersect(S.random, &q, d_rays, N, d_hits, j->stream));
    CHECK(hrt_scene_scatter(S.random, &sc, d_rays, d_hits, d_paths, N, j->stream));
  }
  HIP(hipMemcpyAsync(paths_a, d_paths, sizeof(paths_a), hipMemcpyDeviceToHost, j->stream));

  /* fresh paths through the fused call over two live lists; the list the second call wrote is kept */
  CHECK(hrt_camera_paths(S.random, &S.cam0, &p, &frame, 1, d_rays, d_paths, j->stream));
  HIP(hipMemsetAsync(d_n_rays, 0, sizeof(uint64_t), j->stream));
  const hrt_path_list lists[2] = {{d_index, d_count, N, 0}, {d_index + N, d_count + 1, N, 0}};
  const hrt_path_list* in = NULL;
  for (int call = 0; call < Q1_DEPTH / Q1_STEPS; call++) {
    const hrt_path_list* out = &lists[call & 1];
    CHECK(hrt_scene_step(S.random, &sp, d_rays, d_paths, N, NULL, in, out, d_n_rays, j->stream));
    in = out;
    if (call == 1) {
      HIP(hipMemcpyAsync(d_kept, out->d_index, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, j->stream));
      HIP(hipMemcpyAsync(d_count + 2, out->d_count, sizeof(uint32_t), hipMemcpyDeviceToDevice, j->stream));
    }
  }
  if (put_kernel(r)) return 1;
  uint64_t n_rays = 0;
  uint32_t kept = 0;
  HIP(hipMemcpyAsync(paths_b, d_paths, sizeof(paths_b), hipMemcpyDeviceToHost, j->stream));
  HIP(hipMemcpyAsync(&n_rays, d_n_rays, sizeof(n_rays), hipMemcpyDeviceToHost, j->stream));
  HIP(hipMemcpyAsync(&kept, d_count + 2, sizeof(kept), hipMemcpyDeviceToHost, j->stream));
  HIP(hipStreamSynchronize(j->stream));
  NEED(kept <= N);
  HIP(hipMemcpy(live + 1, d_kept, kept * sizeof(uint32_t), hipMemcpyDeviceToHost));
  /* the list's order is not part of the contract: compare it as a sorted set */
  live[0] = kept;
  qsort(live + 1, kept, sizeof(uint32_t), cmp_u32);
  for (int i = 0; i < N; i++) NEED((paths_b[i].flags & HRT_PATH_DONE) != 0);
  NEED(memcmp(paths_a, paths_b, sizeof(paths_a)) == 0); /* step's contract: the two calls' records, bit for bit */
  return put(r, paths_b, sizeof(paths_b)) || put(r, &n_rays, sizeof(n_rays)) || put(r, live, (kept + 1) * sizeof(uint32_t));
}

static int job_l1(Job* j, Result* r) {
  enum { W = 16, H = 16 };
  float frames[3][W * H * 4];
  float* d_unused = (float*)dev(j, 0, W * H * 16);
  NEED(d_unused);
  for (int it = 0; it < 3; it++) {
    hrt_scene* s = NULL;
    hrt_preset_info info;
    hrt_camera cam;
    CHECK(hrt_scene_create(&s));
    CHECK(hrt_preset_build(s, HRT_PRESET_TWO_SPHERES, 1, NULL, 0, 0, 0, &info));
    CHECK(hrt_scene_commit(s, 0));
    CHECK(hrt_camera_init(&cam, info.look_from, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0, info.time1, W, H));
    hrt_render_params p = params(&info, W, H, 4, 0);
    hrt_render_stats st;
    memset(&st, 0, sizeof(st));
    CHECK(hrt_render(s, &cam, &p, 0, 0, W, H, frames[it], &st));
    if (it == 0) put_stats(r, &st);
    if (put_kernel(r)) return 1;
    hrt_scene_destroy(s);
    if (it == 2) break;
    /* two calls that are refused before any device work, on the scene the other threads are launching on */
    hrt_render_params q = params(&S.ri, 64, 36, 8, 0);
    if (it == 0) {
      const hrt_tile outside = {60, 30, 16, 16};
      put_refused(r, hrt_render_tiles_device(S.random, &S.cam0, &q, &outside, 1, d_unused, j->stream, NULL));
    } else {
      const hrt_tile inside = {0, 0, 1, 1};
      q.width = 1;
      put_refused(r, hrt_render_tiles_device(S.random, &S.cam0, &q, &inside, 1, d_unused, j->stream, NULL));
    }
    NEED(r->refused_status[r->n_refused - 1] == HRT_ERR_INVALID_ARG);
  }
  return put(r, frames, sizeof(frames));
}

/* name and function; the rest starts zeroed */
static Job g_jobs[N_JOBS] = {
    {"R1", job_r1},
    {"R2", job_r2},
    {"R3", job_r3},
    {"R4", job_r4},
    {"A1", job_a1},
    {"A2", job_a2},
    {"Q1", job_q1},
    {"L1", job_l1},
};

static void* worker(void* arg) {
  Job* j = (Job*)arg;
  /* the launch record is the thread's: the main thread has launched, this one has not */
  hrt_launch_info li;
  const int fresh = hrt_last_launch(&li) == HRT_ERR_STATE;
  for (int round = 0; round < ROUNDS; round++) {
    pthread_barrier_wait(&g_barrier);
    Result r;
    memset(&r, 0, sizeof(r));
    const int rc = j->run(j, &r);
    const char* diff = rc ? "the job failed" : result_diff(&r, &j->serial);
    if (!diff && round == 0 && !fresh) diff = "hrt_last_launch answered on a thread that had not launched";
    if (diff) {
      j->bad++;
      printf("round %d %s DIFFERS: %s\n", round, j->name, diff);
    } else {
      printf("round %d %s equal\n", round, j->name);
    }
    result_free(&r);
  }
  return NULL;
}

static int write_pfm(const char* dir, const char* name, const void* rgba, uint32_t w, uint32_t h) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s.pfm", dir, name);
  CHECK(hrt_image_write(path, (const float*)rgba, w, h, HRT_IMAGE_PFM));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: threads OUT_DIR\n");
    return 2;
  }
  const char* dir = argv[1];
  setvbuf(stdout, NULL, _IOLBF, 0); /* a run that is cut short still shows how far it came */
  if (hrt_abi_version() != HRT_ABI_VERSION) {
    fprintf(stderr, "libhrt.so has another ABI version\n");
    return 1;
  }
  /* the scenes, committed once */
  CHECK(hrt_scene_create(&S.random));
  CHECK(hrt_preset_build(S.random, HRT_PRESET_RANDOM, 1, NULL, 0, 0, 0, &S.ri));
  CHECK(hrt_scene_commit(S.random, 0));
  CHECK(hrt_scene_create(&S.cornell));
  CHECK(hrt_preset_build(S.cornell, HRT_PRESET_CORNELL, 1, NULL, 0, 0, 0, &S.ci));
  CHECK(hrt_scene_commit(S.cornell, 0));
  const hrt_preset_info* ri = &S.ri;
  CHECK(hrt_camera_init(&S.cam0, ri->look_from, ri->look_at, ri->fov, ri->aperture, ri->focus_dist, ri->time0, ri->time1, 64, 36));
  CHECK(hrt_camera_init(&S.cam1, LOOK_FROM_1, ri->look_at, ri->fov, ri->aperture, ri->focus_dist, ri->time0, ri->time1, 37, 19));
  CHECK(hrt_camera_init(&S.cam2, LOOK_FROM_2, ri->look_at, ri->fov, ri->aperture, ri->focus_dist, ri->time0, ri->time1, 64, 36));
  CHECK(hrt_camera_init(&S.cam2_big, LOOK_FROM_2, ri->look_at, ri->fov, ri->aperture, ri->focus_dist, ri->time0, ri->time1, 1920, 1080));
  const hrt_preset_info* ci = &S.ci;
  CHECK(hrt_camera_init(&S.cam_box, ci->look_from, ci->look_at, ci->fov, ci->aperture, ci->focus_dist, ci->time0, ci->time1, 32, 32));
  for (int k = 0; k < N_JOBS; k++) HIP(hipStreamCreateWithFlags(&g_jobs[k].stream, hipStreamNonBlocking));

  /* ---- serial phase ---- */
  for (int k = 0; k < N_JOBS; k++) {
    Job* j = &g_jobs[k];
    if (j->run(j, &j->serial)) {
      fprintf(stderr, "serial %s failed\n", j->name);
      return 1;
    }
    printf("serial %s segments=%llu kernel=%s\n", j->name, (unsigned long long)(j->serial.n_stats ? j->serial.stats[0][0] : 0),
           j->serial.kernel);
  }
  /* the table must keep two kernels reporting on two threads */
  if (strcmp(g_jobs[0].serial.kernel, g_jobs[3].serial.kernel) == 0) {
    fprintf(stderr, "R1 and R4 ran the same kernel\n");
    return 1;
  }
  if (write_pfm(dir, "R1", g_jobs[0].serial.out[0], 64, 36) || write_pfm(dir, "R2", g_jobs[1].serial.out[0], 37, 19) ||
      write_pfm(dir, "R3", g_jobs[2].serial.out[1], 64, 36) || write_pfm(dir, "R4", g_jobs[3].serial.out[0], 32, 32))
    return 1;
  fflush(stdout);

  /* ---- concurrent phase ---- */
  pthread_t threads[N_JOBS];
  if (pthread_barrier_init(&g_barrier, NULL, N_JOBS) != 0) return 1;
  for (int k = 0; k < N_JOBS; k++)
    if (pthread_create(&threads[k], NULL, worker, &g_jobs[k]) != 0) {
      fprintf(stderr, "pthread_create failed\n");
      return 1; /* the process ends, and the threads already waiting at the barrier with it */
    }
  int bad = 0;
  for (int k = 0; k < N_JOBS; k++) {
    pthread_join(threads[k], NULL);
    bad += g_jobs[k].bad;
  }
  pthread_barrier_destroy(&g_barrier);

  for (int k = 0; k < N_JOBS; k++) {
    Job* j = &g_jobs[k];
    result_free(&j->serial);
    for (int d = 0; d < N_DEV; d++)
      if (j->dev[d]) (void)hipFree(j->dev[d]);
    (void)hipStreamDestroy(j->stream);
  }
  hrt_scene_destroy(S.cornell);
  hrt_scene_destroy(S.random);
  if (bad) {
    fprintf(stderr, "%d job rounds failed or differed from the serial run\n", bad);
    return 1;
  }
  printf("threads: ok\n");
  return 0;
}
