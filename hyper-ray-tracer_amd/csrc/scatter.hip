/*
 * scatter.hip — scatter queries: the kernel and entry points of hrt_scene_scatter (per-lane code: scatter.h; the
 * contract: include/hrt/hrt.h).  hrt_camera_paths is in query.hip, next to hrt_camera_rays.
 *
 *   scatter_kernel   one lane per path, a plain grid over the batch: there is no walk, so a lane's work is one
 *                    material's scatter and one texture lookup, bounded by the draws' rejection loops (a path with the
 *                    all-zero rng state, on which they would never end, is refused: scatter.h), and nothing needs a
 *                    claim counter.  A lane reads its path's last 16 bytes first and leaves if the path is DONE: a
 *                    wave of finished paths touches 16 of its 144 bytes per lane.  Otherwise it reads the three
 *                    records and writes the ray and the path back as three 16-B accesses each.  Materials, textures
 *                    and images are read from global memory; no LDS.  The kernel of scenes without a noise texture.
 *   scatter_staged_kernel  the kernel of scenes whose Perlin tables fit SCATTER_PERLIN_MAX_BYTES: a resident grid whose
 *                    workgroups stage the tables in LDS once (stage_perlin) and then stride over the batch, so that
 *                    the 12 KB per table are copied once per workgroup and not once per 256 paths.  Measured on
 *                    earth_perlin, 8.3 M paths: 0.47 ms against 0.58 with the tables in global memory, and 0.24
 *                    against 0.32 in a late round.  HRT_SCATTER_PERLIN_LDS=0 runs scatter_kernel
 *                    instead (perlin_lds = 0): the same records.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernel_common.h"
#include "query_host.h"

using namespace hrt;
using namespace hrt::scatterq;

namespace {

constexpr int SCATTER_THREADS = 256;

__global__ __launch_bounds__(SCATTER_THREADS) void scatter_kernel(KParams P, hrt_ray* rays, const hrt_hit* __restrict__ hits,
                                                                  hrt_path* paths, uint32_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * SCATTER_THREADS + threadIdx.x; /* n < 2^32: the grid has at most 2^24 blocks */
  if (i >= n) return;
  scatter_record(P, rays + i, hits + i, paths + i, P.background);
}

/* perlin_at: where the tables go in the dynamic LDS, in float4s, from the host (a multiple of PERLIN_LDS_ALIGN bytes:
 * this kernel declares no static __shared__, so the dynamic LDS starts at address 0 and offset and address agree) */
__global__ __launch_bounds__(SCATTER_THREADS) void scatter_staged_kernel(KParams P, hrt_ray* rays, const hrt_hit* __restrict__ hits,
                                                                         hrt_path* paths, uint32_t n, uint32_t perlin_at) {
  extern __shared__ float4 lds[];
  KParams Q = P;
  Q.perlin = kern::stage_perlin(lds + perlin_at, P.perlin, P.n_perlin);
  Q.perlin_lds = 1u;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * SCATTER_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * SCATTER_THREADS + threadIdx.x; i < n; i += stride)
    scatter_record(Q, rays + i, hits + i, paths + i, Q.background);
}

constexpr size_t SCATTER_PERLIN_MAX_BYTES = 4 * sizeof(G::Perlin); /* 48 KB: three workgroups a CU keep their tables */

/* the argument checks of both entry points, before any device call */
void check_scatter_args(const hrt_scene* s, const hrt_scatter_params* sp, const void* rays, const void* hits, const void* paths,
                        uint64_t n, bool on_device, const char* who) {
  if (!s || !sp) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null argument"};
  if (!scatter_params_ok(sp))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": bad scatter params (flags 0, reserved 0, a finite background)"};
  if (n >= (1ull << 32)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": n must be below 2^32"};
  if (n != 0 && (!rays || !hits || !paths)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null buffer"};
  if (n != 0 && on_device && (!aligned16(rays) || !aligned16(hits) || !aligned16(paths)))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the records must be 16-byte aligned"};
  if (!s->committed || !s->d_blob) throw HipError{HRT_ERR_STATE, "scene not committed"};
}

}  // namespace

extern "C" {

hrt_status hrt_scene_scatter(hrt_scene* s, const hrt_scatter_params* sp, hrt_ray* d_rays, const hrt_hit* d_hits, hrt_path* d_paths,
                             uint64_t n, void* stream_) {
  return hguard([&] {
    check_scatter_args(s, sp, d_rays, d_hits, d_paths, n, true, "hrt_scene_scatter");
    if (n == 0) return;
    DeviceGuard dg(s->device);
    const KParams kp = scene_scatter_params(s, sp);
    const uint32_t grid = (uint32_t)((n + (SCATTER_THREADS - 1)) / SCATTER_THREADS);
    const char* staged = knob_env("HRT_SCATTER_PERLIN_LDS"); /* A/B: "0" leaves the Perlin tables in global memory (the same records) */
    const size_t smem = kp.n_perlin * sizeof(G::Perlin);
    if (!(staged && strcmp(staged, "0") == 0) && smem > 0 && smem <= SCATTER_PERLIN_MAX_BYTES) {
      const int resident = resident_grid((const void*)scatter_staged_kernel, SCATTER_THREADS, s->device, smem, true, "scatter_staged_kernel");
      hipLaunchKernelGGL(scatter_staged_kernel, dim3(std::min<uint32_t>((uint32_t)resident, grid)), dim3(SCATTER_THREADS), smem,
                         (hipStream_t)stream_, kp, d_rays, d_hits, d_paths, (uint32_t)n, 0u);
      hip_check(hipGetLastError(), "scatter_staged_kernel launch");
      launch_knobs(s);
      return;
    }
    hipLaunchKernelGGL(scatter_kernel, dim3(grid), dim3(SCATTER_THREADS), 0, (hipStream_t)stream_, kp, d_rays, d_hits, d_paths,
                       (uint32_t)n);
    hip_check(hipGetLastError(), "scatter_kernel launch");
  });
}

hrt_status hrt_scene_scatter_host(hrt_scene* s, const hrt_scatter_params* sp, hrt_ray* rays, const hrt_hit* hits, hrt_path* paths,
                                  uint64_t n) {
  hrt_status st = hguard([&] { check_scatter_args(s, sp, rays, hits, paths, n, false, "hrt_scene_scatter_host"); });
  if (st != HRT_OK || n == 0) return st;
  return hguard([&] {
    DeviceGuard dg(s->device);
    DevBuf<hrt_ray> d_rays((size_t)n * sizeof(hrt_ray), rays);
    DevBuf<hrt_hit> d_hits((size_t)n * sizeof(hrt_hit), hits);
    DevBuf<hrt_path> d_paths((size_t)n * sizeof(hrt_path), paths);
    const hrt_status r = hrt_scene_scatter(s, sp, d_rays.p, d_hits.p, d_paths.p, n, nullptr);
    if (r != HRT_OK) throw HipError{r, hrt_last_error()};
    hip_check(hipMemcpy(rays, d_rays.p, (size_t)n * sizeof(hrt_ray), hipMemcpyDeviceToHost), "hipMemcpy(rays)");
    hip_check(hipMemcpy(paths, d_paths.p, (size_t)n * sizeof(hrt_path), hipMemcpyDeviceToHost), "hipMemcpy(paths)");
  });
}

}  // extern "C"
