/* render_host.h — the host helpers render.hip (the render kernels and the device runtime) and accum.hip (the sample
 * accumulator) share.  Each is declared here once; the comment says which of the two files defines it. */
#pragma once
#include <algorithm>
#include <new>
#include <utility>

#include "kernel_common.h"

namespace hrt {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    hip_check(hipGetDevice(&prev), "hipGetDevice");
    if (dev >= 0 && dev != prev) hip_check(hipSetDevice(dev), "hipSetDevice");
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class F>
hrt_status hguard(F&& f) {
  try {
    f();
    return HRT_OK;
  } catch (const HipError& e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_error("out of host memory");
    return HRT_ERR_OOM;
  } catch (const std::exception& e) {
    set_error(e.what());
    return HRT_ERR_INVALID_ARG;
  }
}

/* An owned device buffer, freed with its owner: on every exit path of a call (the debug entry points throw through
 * hip_check), or with the accumulator that keeps it as a member.  Empty until alloc() (`what`: the hip_check label), or
 * made at once and filled from src if given.  The free is on the calling thread's current device and its result is
 * ignored. */
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  explicit DevBuf(size_t bytes, const void* src = nullptr) : DevBuf() { /* delegating: a throw below still frees p */
    alloc(bytes, "hipMalloc(debug)");
    if (src) hip_check(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice), "hipMemcpy");
  }
  void alloc(size_t bytes, const char* what) {
    DevBuf fresh;
    hip_check(hipMalloc((void**)&fresh.p, bytes), what);
    *this = std::move(fresh);
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p); /* o frees what this held */
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

/* hrt_render's device output buffers (scene_internal.h out_pool; render.hip): taken and given back under the
 * pool's mutex; a buffer too small for a call is freed and replaced */
struct OutBuf {
  void* ptr;
  size_t cap;
};
OutBuf out_pool_take(hrt_scene* s, size_t bytes);
void out_pool_give(hrt_scene* s, OutBuf b);

constexpr uint32_t STREAM_MAX_BLOCKS = 4096; /* reduce_chunks' cap: larger frames take further trips of the loop */
inline uint32_t stream_blocks(size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, STREAM_MAX_BLOCKS); }

/* Where the sums of a launch go: into a frame (hrt_render_tiles_device: d_rgba = sqrt(sum / spp)), or added to an
 * accumulator's raw sums (hrt_accum_add: d_acc), optionally with the accumulated frame resolved to d_preview by
 * the kernel that adds the pass. */
struct SumsDest {
  float* d_rgba = nullptr;
  float4* d_acc = nullptr;
  int preview = -1;          /* HRT_ACCUM_* format of d_preview, -1: none */
  void* d_preview = nullptr;
  float preview_scale = 0.0f; /* 1 / the accumulator's samples after this pass */
  /* mapped: the pass goes through accumulate_chunks' tile map (a HRT_ACCUM_NOISE accumulator, or a pass over a subset
   * of the accumulator's tiles): launched tile i lands at pixel acc_offs[i] of the accumulator, and d_m2 (or null)
   * takes the pass's moment */
  bool mapped = false;
  float* d_m2 = nullptr;
  const uint32_t* acc_offs = nullptr;
};

/* render.hip: one render launch of a tile set, up to where its sums go (dst) */
void render_launch(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles,
                   const SumsDest& dst, void* stream, hrt_render_stats* stats, bool* launched);
/* render.hip: the kernel parameters of a feature pass over samples [p->sample_offset, + p->samples) and the
 * instantiation its plan names (cull: layout.h CULL_EXACT or CULL_REFERENCE); an approximate plan is HRT_ERR_UNSUPPORTED */
lane::KParams feature_params(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, int& cull, bool& full);
/* render.hip: the knobs in effect now and at the scene's commit, into the thread's launch record (hrt_last_launch);
 * called right after resident_grid has written that record */
void launch_knobs(const hrt_scene* s);
/* render.hip: the checks every kernel entry point makes on (cam, p) (check_render_args), for query.hip */
void check_render_params(const hrt_camera* cam, const hrt_render_params* p);
/* render.hip: a render's sample chunks (lane.h frame_chunks) */
void chunk_schedule(const hrt_scene* s, const hrt_render_params* p, uint32_t& chunk, uint32_t& n_head, uint32_t& first,
                    uint32_t& n_tail);

/* accum.hip: acc[i] += the pass sum of partial[.][i] (accumulate_chunks), format >= 0: with the frame after the pass
 * resolved to out; _mapped: through the launch's tile table `tiles` (on the device), with the pass's moment added to
 * m2 (or null), the chunk sizes being those of the schedule (chunk, chunk_head, chunk_first) */
void launch_accumulate(int format, const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale, void* out,
                       hipStream_t stream);
void launch_accumulate_mapped(int format, const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale, void* out,
                              float* m2, const gpu::TileDev* tiles, uint32_t n_tiles, uint32_t chunk, uint32_t chunk_head,
                              uint32_t chunk_first, hipStream_t stream);

}  // namespace hrt
