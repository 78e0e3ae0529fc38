/*
 * query.hip — ray queries: the kernels and entry points of hrt_scene_intersect and hrt_camera_rays (per-lane code:
 * query.h; the contract: include/hrt/hrt.h).
 *
 *   query_kernel        one lane per ray, a persistent grid (resident_grid).  A wave takes blocks of 64 consecutive
 *                       rays with one atomicAdd on the call's block counter, so a batch whose rays take walks of very
 *                       different lengths still balances.  A large batch takes up to QUERY_CLAIM_MAX blocks per
 *                       atomicAdd (claim_blocks): at one block each the atomics on ONE address bound the call.  LDS: the workgroup stages the reference node stream and the
 *                       primitive records once (stage_scene) when they fit the budget that keeps two workgroups on a
 *                       CU (layout.h LDS_SCENE_MAX_BYTES); otherwise, or under HRT_QUERY_NO_LDS, the walk reads them
 *                       from global memory as feature_kernel does.  A lane reads its ray and writes its hit as three
 *                       16-B accesses each.  Every loop is bounded by the ray count and the walk's skip links point
 *                       forward (lane.h trace_ray), so every launch ends.
 *   camera_rays_kernel  one lane per pixel over the tile-block domain of features.hip; the lane writes its pixel's
 *                       samples' rays in index order.
 *   camera_paths_kernel the same domain and rays for hrt_camera_paths, with each ray's starting path (scatter.h
 *                       camera_path) written beside it.
 */
#include <hip/hip_runtime.h>

#include <vector>

#include "feature_pass.h"
#include "kernel_common.h"
#include "query.h"
#include "query_host.h"

using namespace hrt;
using namespace hrt::query;
using hrt::features::FeatureTile;

namespace {

template <bool LDS>
constexpr int query_threads() { return LDS ? 512 : 256; }

template <int CULL, bool FULL, bool MEDIA, bool LDS>
__global__ __launch_bounds__(query_threads<LDS>()) void query_kernel(KParams P, const hrt_ray* __restrict__ rays, uint32_t n,
                                                                     hrt_hit* __restrict__ hits, uint32_t* __restrict__ counter,
                                                                     uint32_t claim) {
  extern __shared__ float4 lds[];
  const G::Node* nodes = P.nodes;
  const G::Prim* prims = P.prims;
  if constexpr (LDS) kern::stage_scene(P, lds, nodes, prims);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_blocks = (n + (QUERY_BLOCK - 1u)) / QUERY_BLOCK; /* n < 2^32: no wrap after the division */
  for (;;) {
    uint32_t b0 = 0;
    if (lane == 0u) b0 = atomicAdd(counter, claim);
    b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0); /* every lane is active here: lane 0's claim */
    if (b0 >= n_blocks) break; /* n_blocks <= 2^26 and each wave overshoots once, by claim <= 64: the counter cannot wrap */
    const uint32_t b1 = min(b0 + claim, n_blocks);
    for (uint32_t b = b0; b < b1; b++) {
      const uint64_t i = (uint64_t)b * QUERY_BLOCK + lane;
      if (i < n) {
        const hrt_ray ray = load_ray(rays + i);
        store_hit(hits + i, query_ray<CULL, FULL, MEDIA>(P, nodes, prims, ray));
      }
    }
  }
}

__global__ __launch_bounds__(64) void camera_rays_kernel(KParams P, FeatureTile one, const FeatureTile* __restrict__ tiles,
                                                         uint32_t n_tiles, uint32_t log_bw, hrt_ray* __restrict__ rays) {
  const FeatureTile T = n_tiles == 1u ? one : tile_of_block(tiles, n_tiles, blockIdx.x);
  const uint32_t bw = 1u << log_bw, bh = 64u >> log_bw;
  const uint32_t nbx = (T.w + bw - 1) / bw, k = blockIdx.x - T.blk0;
  const uint32_t lx = (k % nbx) * bw + (threadIdx.x & (bw - 1)), ly = (k / nbx) * bh + (threadIdx.x >> log_bw);
  if (lx >= T.w || ly >= T.h) return;
  const size_t at = ((size_t)T.off + (size_t)ly * T.w + lx) * P.spp; /* < 2^32: the entry point checks */
  for (uint32_t j = 0; j < P.spp; j++) store_ray(rays + at + j, camera_ray(P, T.x + lx, T.y + ly, j));
}

__global__ __launch_bounds__(64) void camera_paths_kernel(KParams P, FeatureTile one, const FeatureTile* __restrict__ tiles,
                                                          uint32_t n_tiles, uint32_t log_bw, hrt_ray* __restrict__ rays,
                                                          hrt_path* __restrict__ paths) {
  const FeatureTile T = n_tiles == 1u ? one : tile_of_block(tiles, n_tiles, blockIdx.x);
  const uint32_t bw = 1u << log_bw, bh = 64u >> log_bw;
  const uint32_t nbx = (T.w + bw - 1) / bw, k = blockIdx.x - T.blk0;
  const uint32_t lx = (k % nbx) * bw + (threadIdx.x & (bw - 1)), ly = (k / nbx) * bh + (threadIdx.x >> log_bw);
  if (lx >= T.w || ly >= T.h) return;
  const size_t at = ((size_t)T.off + (size_t)ly * T.w + lx) * P.spp; /* < 2^32: the entry point checks */
  for (uint32_t j = 0; j < P.spp; j++) {
    const scatterq::CameraPath c = scatterq::camera_path(P, T.x + lx, T.y + ly, j);
    store_ray(rays + at + j, c.ray);
    scatterq::store_path(paths + at + j, c.path);
  }
}

template <int CULL, bool FULL, bool MEDIA, bool LDS>
void launch_one(const KParams& P, int device, size_t smem, const hrt_ray* rays, uint32_t n, hrt_hit* hits, uint32_t* counter,
                hipStream_t stream) {
  const void* fn = (const void*)query_kernel<CULL, FULL, MEDIA, LDS>;
  const int block = query_threads<LDS>();
  const uint32_t n_blocks = (n + (QUERY_BLOCK - 1u)) / QUERY_BLOCK;
  const int resident = resident_grid(fn, block, device, LDS ? smem : 0, LDS, __PRETTY_FUNCTION__);
  /* no more workgroups than there are claims for their waves */
  const uint32_t claim = claim_blocks(n_blocks), n_claims = (n_blocks + claim - 1u) / claim, waves = (uint32_t)(block / 64);
  const uint32_t grid = std::min<uint32_t>((uint32_t)resident, (n_claims + waves - 1u) / waves);
  hipLaunchKernelGGL((query_kernel<CULL, FULL, MEDIA, LDS>), dim3(grid), dim3(block), LDS ? smem : 0, stream, P, rays, n, hits,
                     counter, claim);
  hip_check(hipGetLastError(), "query_kernel launch");
}

template <int CULL, bool LDS>
void launch_cull(bool full, bool media, const KParams& P, int device, size_t smem, const hrt_ray* rays, uint32_t n, hrt_hit* hits,
                 uint32_t* counter, hipStream_t stream) {
  if (full && media) launch_one<CULL, true, true, LDS>(P, device, smem, rays, n, hits, counter, stream);
  else if (full) launch_one<CULL, true, false, LDS>(P, device, smem, rays, n, hits, counter, stream);
  else launch_one<CULL, false, false, LDS>(P, device, smem, rays, n, hits, counter, stream);
}

/* the instantiation a query runs: exact or reference culling (query.h query_cull), FULL for general scenes (and sphere
 * scenes whose textures or walk stream need it, as the feature pass), media on or off, the scene in LDS or not */
void launch_query(const hrt_scene* s, const hrt_query_params* q, const KParams& P, const hrt_ray* rays, uint32_t n, hrt_hit* hits,
                  uint32_t* counter, hipStream_t stream) {
  const int cull = query_cull(q, s->cull_mode, s->box_t0, s->box_t1);
  const bool full = (s->feature_mask & ~G::F_BASIC) != 0 || s->w_general;
  const bool media = full && (s->feature_mask & G::F_MEDIUM) != 0 && !(q->flags & HRT_QUERY_SKIP_MEDIA);
  const size_t smem = s->g_nodes.size() * sizeof(G::Node) + s->g_prims.size() * sizeof(G::Prim);
  const bool lds = !(q->flags & HRT_QUERY_NO_LDS) && smem <= G::LDS_SCENE_MAX_BYTES;
  if (cull == G::CULL_EXACT) {
    if (lds) launch_cull<G::CULL_EXACT, true>(full, media, P, s->device, smem, rays, n, hits, counter, stream);
    else launch_cull<G::CULL_EXACT, false>(full, media, P, s->device, smem, rays, n, hits, counter, stream);
  } else {
    if (lds) launch_cull<G::CULL_REFERENCE, true>(full, media, P, s->device, smem, rays, n, hits, counter, stream);
    else launch_cull<G::CULL_REFERENCE, false>(full, media, P, s->device, smem, rays, n, hits, counter, stream);
  }
  launch_knobs(s);
}

/* the argument checks of both intersect entry points, before any device call */
void check_query_args(const hrt_scene* s, const hrt_query_params* q, const void* rays, uint64_t n, const void* hits, bool on_device,
                      const char* who) {
  if (!s || !q) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null argument"};
  if (!query_params_ok(q))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": bad query params (known flags, reserved 0, finite time0 <= time1)"};
  if (n >= (1ull << 32)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": n must be below 2^32"};
  if (n != 0 && (!rays || !hits)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null buffer"};
  if (n != 0 && on_device && (!aligned16(rays) || !aligned16(hits)))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the records must be 16-byte aligned"};
  if (!s->committed || !s->d_blob) throw HipError{HRT_ERR_STATE, "scene not committed"};
}

/* the tile table of a camera-rays call and its counts: tiles inside the image, their pixels x samples below 2^32 */
std::vector<FeatureTile> ray_tiles(const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles, uint32_t log_bw,
                                   uint64_t& n_pixels, uint32_t& n_blocks) {
  std::vector<FeatureTile> ft(n_tiles);
  uint64_t off = 0, blk = 0;
  for (uint32_t i = 0; i < n_tiles; i++) {
    const hrt_tile& t = tiles[i];
    if (t.w == 0 || t.h == 0 || (uint64_t)t.x + t.w > p->width || (uint64_t)t.y + t.h > p->height)
      throw HipError{HRT_ERR_INVALID_ARG, "tile outside the image"};
    if (off * p->samples >= (1ull << 32) || blk >= (1ull << 31))
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_camera_rays: 2^32 rays or more"};
    ft[i] = FeatureTile{t.x, t.y, t.w, t.h, (uint32_t)off, (uint32_t)blk, {0u, 0u}};
    off += (uint64_t)t.w * t.h;
    blk += features::tile_blocks(t.w, t.h, log_bw);
  }
  if (off * p->samples >= (1ull << 32) || blk >= (1ull << 31)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_camera_rays: 2^32 rays or more"};
  n_pixels = off;
  n_blocks = (uint32_t)blk;
  return ft;
}

void check_camera_args(const hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles,
                       const void* rays, bool on_device, const char* who) {
  if (!s || !cam || !p || !tiles || n_tiles == 0 || !rays) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null argument"};
  if (on_device && !aligned16(rays)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the records must be 16-byte aligned"};
  check_render_params(cam, p);
  if (!s->committed || !s->d_blob) throw HipError{HRT_ERR_STATE, "scene not committed"};
}

/* the launch of hrt_camera_rays (d_paths null) and hrt_camera_paths, after the argument checks */
void camera_launch(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles,
                   hrt_ray* d_rays, hrt_path* d_paths, void* stream_) {
  const uint32_t log_bw = features::block_log_w();
  uint64_t n_pixels = 0;
  uint32_t n_blocks = 0;
  const std::vector<FeatureTile> ft = ray_tiles(p, tiles, n_tiles, log_bw, n_pixels, n_blocks);
  hipStream_t stream = (hipStream_t)stream_;
  DeviceGuard dg(s->device);
  KParams kp;
  memset(&kp, 0, sizeof(kp));
  set_camera_params(kp, cam, p);
  FeatureTile* d_tiles = nullptr;
  if (n_tiles > 1) { /* the table goes to the device in stream order; the call then waits, so `ft` outlives the copy */
    hip_check(hipMallocAsync((void**)&d_tiles, ft.size() * sizeof(FeatureTile), stream), "hipMallocAsync(ray tiles)");
    try {
      hip_check(hipMemcpyAsync(d_tiles, ft.data(), ft.size() * sizeof(FeatureTile), hipMemcpyHostToDevice, stream),
                "hipMemcpyAsync(ray tiles)");
    } catch (...) {
      (void)hipFreeAsync(d_tiles, stream);
      throw;
    }
  }
  if (d_paths)
    hipLaunchKernelGGL(camera_paths_kernel, dim3(n_blocks), dim3(64), 0, stream, kp, ft[0], d_tiles, n_tiles, log_bw, d_rays, d_paths);
  else
    hipLaunchKernelGGL(camera_rays_kernel, dim3(n_blocks), dim3(64), 0, stream, kp, ft[0], d_tiles, n_tiles, log_bw, d_rays);
  const hipError_t launched = hipGetLastError();
  if (d_tiles) {
    (void)hipFreeAsync(d_tiles, stream);
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize(ray tiles)");
  }
  hip_check(launched, d_paths ? "camera_paths_kernel launch" : "camera_rays_kernel launch");
}

}  // namespace

extern "C" {

hrt_status hrt_scene_intersect(hrt_scene* s, const hrt_query_params* q, const hrt_ray* d_rays, uint64_t n, hrt_hit* d_hits,
                               void* stream_) {
  return hguard([&] {
    check_query_args(s, q, d_rays, n, d_hits, true, "hrt_scene_intersect");
    if (n == 0) return;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard dg(s->device);
    const KParams kp = scene_query_params(s, q);
    /* the call's own block counter, allocated, zeroed and freed in stream order: calls on any streams are independent */
    uint32_t* counter = nullptr;
    hip_check(hipMallocAsync((void**)&counter, sizeof(uint32_t), stream), "hipMallocAsync(query counter)");
    try {
      hip_check(hipMemsetAsync(counter, 0, sizeof(uint32_t), stream), "hipMemsetAsync(query counter)");
      launch_query(s, q, kp, d_rays, (uint32_t)n, d_hits, counter, stream);
    } catch (...) {
      (void)hipFreeAsync(counter, stream);
      throw;
    }
    hip_check(hipFreeAsync(counter, stream), "hipFreeAsync(query counter)");
  });
}

hrt_status hrt_scene_intersect_host(hrt_scene* s, const hrt_query_params* q, const hrt_ray* rays, uint64_t n, hrt_hit* hits) {
  hrt_status st = hguard([&] { check_query_args(s, q, rays, n, hits, false, "hrt_scene_intersect_host"); });
  if (st != HRT_OK || n == 0) return st;
  return hguard([&] {
    DeviceGuard dg(s->device);
    DevBuf<hrt_ray> d_rays((size_t)n * sizeof(hrt_ray), rays);
    DevBuf<hrt_hit> d_hits((size_t)n * sizeof(hrt_hit));
    const hrt_status r = hrt_scene_intersect(s, q, d_rays.p, n, d_hits.p, nullptr);
    if (r != HRT_OK) throw HipError{r, hrt_last_error()};
    hip_check(hipMemcpy(hits, d_hits.p, (size_t)n * sizeof(hrt_hit), hipMemcpyDeviceToHost), "hipMemcpy(hits)");
  });
}

hrt_status hrt_camera_rays(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles,
                           hrt_ray* d_rays, void* stream_) {
  return hguard([&] {
    check_camera_args(s, cam, p, tiles, n_tiles, d_rays, true, "hrt_camera_rays");
    camera_launch(s, cam, p, tiles, n_tiles, d_rays, nullptr, stream_);
  });
}

hrt_status hrt_camera_rays_host(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                                uint32_t n_tiles, hrt_ray* rays) {
  uint64_t n_pixels = 0;
  hrt_status st = hguard([&] {
    check_camera_args(s, cam, p, tiles, n_tiles, rays, false, "hrt_camera_rays_host");
    uint32_t n_blocks = 0;
    (void)ray_tiles(p, tiles, n_tiles, features::block_log_w(), n_pixels, n_blocks);
  });
  if (st != HRT_OK) return st;
  return hguard([&] {
    DeviceGuard dg(s->device);
    const size_t bytes = (size_t)n_pixels * p->samples * sizeof(hrt_ray);
    DevBuf<hrt_ray> d_rays(bytes);
    const hrt_status r = hrt_camera_rays(s, cam, p, tiles, n_tiles, d_rays.p, nullptr);
    if (r != HRT_OK) throw HipError{r, hrt_last_error()};
    hip_check(hipMemcpy(rays, d_rays.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy(rays)");
  });
}

hrt_status hrt_camera_paths(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles, uint32_t n_tiles,
                            hrt_ray* d_rays, hrt_path* d_paths, void* stream_) {
  return hguard([&] {
    if (!d_paths) throw HipError{HRT_ERR_INVALID_ARG, "hrt_camera_paths: null argument"};
    if (!aligned16(d_paths)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_camera_paths: the records must be 16-byte aligned"};
    check_camera_args(s, cam, p, tiles, n_tiles, d_rays, true, "hrt_camera_paths");
    camera_launch(s, cam, p, tiles, n_tiles, d_rays, d_paths, stream_);
  });
}

hrt_status hrt_camera_paths_host(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                                 uint32_t n_tiles, hrt_ray* rays, hrt_path* paths) {
  uint64_t n_pixels = 0;
  hrt_status st = hguard([&] {
    if (!paths) throw HipError{HRT_ERR_INVALID_ARG, "hrt_camera_paths_host: null argument"};
    check_camera_args(s, cam, p, tiles, n_tiles, rays, false, "hrt_camera_paths_host");
    uint32_t n_blocks = 0;
    (void)ray_tiles(p, tiles, n_tiles, features::block_log_w(), n_pixels, n_blocks);
  });
  if (st != HRT_OK) return st;
  return hguard([&] {
    DeviceGuard dg(s->device);
    const size_t n = (size_t)n_pixels * p->samples;
    DevBuf<hrt_ray> d_rays(n * sizeof(hrt_ray));
    DevBuf<hrt_path> d_paths(n * sizeof(hrt_path));
    const hrt_status r = hrt_camera_paths(s, cam, p, tiles, n_tiles, d_rays.p, d_paths.p, nullptr);
    if (r != HRT_OK) throw HipError{r, hrt_last_error()};
    hip_check(hipMemcpy(rays, d_rays.p, n * sizeof(hrt_ray), hipMemcpyDeviceToHost), "hipMemcpy(rays)");
    hip_check(hipMemcpy(paths, d_paths.p, n * sizeof(hrt_path), hipMemcpyDeviceToHost), "hipMemcpy(paths)");
  });
}

}  // extern "C"
