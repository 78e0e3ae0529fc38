/*
 * scene_threads_tsan.cpp — TEST INFRASTRUCTURE ONLY: the host half of a scene (scene.cpp, presets.cpp, knobs.cpp,
 * image_io.cpp: the constructors, BvhNode::new, the walk-stream builders, the host part of hrt_scene_commit) built
 * from several threads at once, under ThreadSanitizer (tests/test_scene_threads.py compiles the four files with this
 * driver; no HIP object is linked, so the two symbols they need from render.hip are the stubs below).
 * Every preset of the table is built and committed once serially and its hrt_debug_scene_blob kept; then all of them
 * are built again, each on a thread of its own, released together, and every blob must equal its serial one byte for
 * byte.  Two more threads make argument errors of different kinds and each must read its own hrt_last_error() text.
 * A race shows up as a TSan report (exit 66), a difference as exit 2.
 */
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hrt/hrt.h"
#include "scene_internal.h"

/* render.hip's half of commit and destruction: there is no device here */
namespace hrt {
hrt_status device_upload(hrt_scene*, int) { return HRT_OK; }
void device_release(hrt_scene*) {}
}  // namespace hrt

namespace {

struct Job {
  int32_t preset;
  const char* name;
};
const Job JOBS[] = {
    {HRT_PRESET_RANDOM, "random"},
    {HRT_PRESET_TWO_SPHERES, "two_spheres"},
    {HRT_PRESET_TWO_PERLIN_SPHERES, "two_perlin_spheres"},
    {HRT_PRESET_SIMPLE_LIGHT, "simple_light"},
    {HRT_PRESET_CORNELL, "cornell"},
    {HRT_PRESET_CORNELL_SMOKE, "cornell_smoke"},
    {HRT_PRESET_FINAL, "final"},
    {HRT_PRESET_FEATURES, "features"},
    {HRT_PRESET_MOTION, "motion"},
    {HRT_PRESET_RANDOM, "random (second)"},
    {HRT_PRESET_FINAL, "final (second)"},
};
constexpr int N_JOBS = (int)(sizeof(JOBS) / sizeof(JOBS[0]));
constexpr int N_ERR = 2;
constexpr int ERR_ROUNDS = 200; /* error calls per error thread, while the builders run */

/* a small RGB8 "earth" so `final` has an image texture */
constexpr uint32_t IW = 64, IH = 32;
std::vector<uint8_t> g_image;

pthread_barrier_t g_barrier;

/* build + commit + blob of one preset; empty on failure (the message is printed) */
std::vector<uint8_t> build_blob_of(const Job& j) {
  std::vector<uint8_t> blob;
  hrt_scene* s = nullptr;
  hrt_preset_info info;
  uint64_t size = 0;
  hrt_status st = hrt_scene_create(&s);
  if (st == HRT_OK) st = hrt_preset_build(s, j.preset, 1, g_image.data(), IW, IH, 3, &info);
  if (st == HRT_OK) st = hrt_scene_commit(s, 0);
  if (st == HRT_OK) st = hrt_debug_scene_blob(s, nullptr, 0, &size, nullptr);
  if (st == HRT_OK) {
    blob.resize(size);
    st = hrt_debug_scene_blob(s, blob.data(), size, &size, nullptr);
  }
  if (st != HRT_OK) {
    fprintf(stderr, "%s: status %d: %s\n", j.name, (int)st, hrt_last_error());
    blob.clear();
  }
  hrt_scene_destroy(s);
  return blob;
}

struct BuildArg {
  int job;
  std::vector<uint8_t> blob;
};
void* build_thread(void* p) {
  BuildArg* a = static_cast<BuildArg*>(p);
  pthread_barrier_wait(&g_barrier);
  a->blob = build_blob_of(JOBS[a->job]);
  return nullptr;
}

struct ErrArg {
  int kind;
  int bad; /* calls whose status or text were not this thread's own */
};
void* error_thread(void* p) {
  ErrArg* a = static_cast<ErrArg*>(p);
  hrt_scene* s = nullptr;
  if (hrt_scene_create(&s) != HRT_OK) {
    a->bad = ERR_ROUNDS;
    pthread_barrier_wait(&g_barrier);
    return nullptr;
  }
  pthread_barrier_wait(&g_barrier);
  for (int k = 0; k < ERR_ROUNDS; k++) {
    hrt_status st;
    const char* want;
    if (a->kind == 0) {
      st = hrt_scene_create(nullptr); /* a null out */
      want = "null out";
    } else {
      st = hrt_scene_set_root(s, 123456u); /* a node id that does not exist */
      want = "bad node id";
    }
    if (st != HRT_ERR_INVALID_ARG || strcmp(hrt_last_error(), want) != 0) a->bad++;
  }
  hrt_scene_destroy(s);
  return nullptr;
}

}  // namespace

int main() {
  g_image.resize((size_t)IW * IH * 3);
  for (size_t i = 0; i < g_image.size(); i++) g_image[i] = (uint8_t)((i * 37u) & 255u);

  std::vector<std::vector<uint8_t>> serial(N_JOBS);
  for (int j = 0; j < N_JOBS; j++) {
    serial[j] = build_blob_of(JOBS[j]);
    if (serial[j].empty()) return 1;
  }
  /* the serial phase is itself repeatable: the second build of a preset equals the first */
  if (serial[0] != serial[9] || serial[6] != serial[10]) {
    fprintf(stderr, "two serial builds of one preset differ\n");
    return 2;
  }

  pthread_barrier_init(&g_barrier, nullptr, N_JOBS + N_ERR);
  std::vector<BuildArg> builds(N_JOBS);
  std::vector<ErrArg> errs(N_ERR);
  std::vector<pthread_t> threads(N_JOBS + N_ERR);
  for (int j = 0; j < N_JOBS; j++) {
    builds[j].job = j;
    if (pthread_create(&threads[j], nullptr, build_thread, &builds[j]) != 0) return 1;
  }
  for (int e = 0; e < N_ERR; e++) {
    errs[e] = ErrArg{e, 0};
    if (pthread_create(&threads[N_JOBS + e], nullptr, error_thread, &errs[e]) != 0) return 1;
  }
  for (pthread_t& t : threads) pthread_join(t, nullptr);
  pthread_barrier_destroy(&g_barrier);

  int bad = 0;
  for (int j = 0; j < N_JOBS; j++) {
    const bool same = !builds[j].blob.empty() && builds[j].blob == serial[j];
    printf("%-20s %8zu bytes, threaded vs serial %s\n", JOBS[j].name, serial[j].size(), same ? "identical" : "DIFFER");
    bad += !same;
  }
  for (int e = 0; e < N_ERR; e++) {
    printf("error thread %d: %d of %d calls read another text\n", e, errs[e].bad, ERR_ROUNDS);
    bad += errs[e].bad != 0;
  }
  if (!bad) printf("scene_threads_tsan: ok\n");
  return bad ? 2 : 0;
}
