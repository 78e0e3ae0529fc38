/*
 * filter.hip — the kernels of the variance-guided a-trous filter (hrt_accum_resolve_filtered; arithmetic: filter.h).
 *
 *   filter_gather   packed sums and m2 -> one raster plane of float4 (c.xyz, v) over the tiles' bounding box, so a
 *                   neighbour is address arithmetic.  Pixels no tile covers keep the v < 0 the plane was filled with.
 *   filter_atrous   one iteration, a 32 x 8 pixel block per 256-thread workgroup.  Steps up to LDS_MAX_STEP stage the
 *                   block and its halo of 2 * step pixels in LDS once (the prefilter's 1-pixel reach lies inside it);
 *                   larger steps read their 25 taps from global memory.  An iteration but the last runs over the
 *                   plane's blocks and writes the other plane; the last runs over the tiles' blocks (filter.h
 *                   FilterTile) and writes the PACKED output in the requested format itself.
 *
 * LDS layout: rows of (32 + 4 * step) float4, linear.  A wave is two block rows of 32 lanes; a tap is the same offset
 * for every lane, so each 16-lane group of a 16-byte LDS read (lanes {0-3, 12-15, 20-27} etc.) reads 16 distinct
 * 16-byte slots whose indices are distinct modulo 16: all 64 banks once, no conflict, for any row pitch.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "filter.h"
#include "kernel_common.h"

using namespace hrt;
using namespace hrt::filter;

namespace {

constexpr uint32_t BLOCK = BLOCK_W * BLOCK_H;
static_assert(BLOCK == 256, "filter_atrous is written for 256-thread workgroups");

__device__ inline Px load_px(const float4* plane, size_t i) {
  const float4 q = plane[i];
  return px(q.x, q.y, q.z, q.w);
}
__device__ inline float4 as_f4(const Px& p) { return make_float4(p.c.x, p.c.y, p.c.z, p.v); }

/* block b of the tile-block domain -> its tile (the last one whose blk0 <= b) and the block's corner in that tile */
__device__ inline FilterTile tile_of_block(const FilterTile* __restrict__ tiles, uint32_t n_tiles, uint32_t b, uint32_t& bx,
                                           uint32_t& by) {
  uint32_t lo = 0, hi = n_tiles;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tiles[mid].blk0 <= b) lo = mid;
    else hi = mid;
  }
  const FilterTile T = tiles[lo];
  const uint32_t nbx = (T.w + BLOCK_W - 1) / BLOCK_W, k = b - T.blk0;
  bx = (k % nbx) * BLOCK_W;
  by = (k / nbx) * BLOCK_H;
  return T;
}

__global__ __launch_bounds__(BLOCK) void filter_gather(const float4* __restrict__ acc, const float* __restrict__ m2,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles,
                                                       float4* __restrict__ plane, uint32_t plane_w) {
  uint32_t bx, by;
  const FilterTile T = tile_of_block(tiles, n_tiles, blockIdx.x, bx, by);
  const uint32_t lx = bx + threadIdx.x % BLOCK_W, ly = by + threadIdx.x / BLOCK_W;
  if (lx >= T.w || ly >= T.h) return;
  const size_t i = (size_t)T.off + (size_t)ly * T.w + lx;
  const float4 a = acc[i];
  plane[(size_t)(T.y + ly) * plane_w + (T.x + lx)] = as_f4(gather(v3(a.x, a.y, a.z), m2[i], T.inv_n, T.inv_k1));
}

/* STEP: the step staged in LDS, or 0: taps from global memory with the step in `step`.
 * FORMAT: -2: an inner iteration over the plane's blocks, to the plane `out`; else the last one over the tiles'
 * blocks, to the packed `out` as FORMAT_RAW, HRT_ACCUM_F32 or HRT_ACCUM_RGBA8. */
constexpr int32_t FORMAT_PLANE = -2;
template <int STEP, int32_t FORMAT>
__global__ __launch_bounds__(BLOCK) void filter_atrous(const float4* __restrict__ in, uint32_t plane_w, uint32_t plane_h,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step, float sigma,
                                                       void* __restrict__ out) {
  constexpr int HALO = 2 * STEP, RW = (int)BLOCK_W + 2 * HALO, RH = (int)BLOCK_H + 2 * HALO;
  __shared__ float4 sh[STEP ? RW * RH : 1];
  /* the block's corner on the plane, the pixels of it this launch owns, and where a packed result goes */
  uint32_t x0, y0, own_w, own_h, row_w = 0;
  size_t packed0 = 0;
  if constexpr (FORMAT == FORMAT_PLANE) {
    const uint32_t nbx = (plane_w + BLOCK_W - 1) / BLOCK_W;
    x0 = (blockIdx.x % nbx) * BLOCK_W;
    y0 = (blockIdx.x / nbx) * BLOCK_H;
    own_w = plane_w - x0;
    own_h = plane_h - y0;
  } else {
    uint32_t bx, by;
    const FilterTile T = tile_of_block(tiles, n_tiles, blockIdx.x, bx, by);
    x0 = T.x + bx;
    y0 = T.y + by;
    own_w = T.w - bx;
    own_h = T.h - by;
    row_w = T.w;
    packed0 = (size_t)T.off + (size_t)by * T.w + bx;
  }
  const int tx = (int)(threadIdx.x % BLOCK_W), ty = (int)(threadIdx.x / BLOCK_W);
  if constexpr (STEP != 0) {
    for (int k = (int)threadIdx.x; k < RW * RH; k += (int)BLOCK) {
      const int gx = (int)x0 - HALO + k % RW, gy = (int)y0 - HALO + k / RW;
      const bool inside = gx >= 0 && gy >= 0 && gx < (int)plane_w && gy < (int)plane_h;
      sh[k] = inside ? in[(size_t)gy * plane_w + (size_t)gx] : as_f4(absent());
    }
    __syncthreads();
  }
  if ((uint32_t)tx >= own_w || (uint32_t)ty >= own_h) return;
  const int x = (int)x0 + tx, y = (int)y0 + ty;
  Px o;
  if constexpr (STEP != 0) {
    const int ox = HALO - (int)x0, oy = HALO - (int)y0;
    const float4* staged = sh;
    auto at = [=](int qx, int qy) {
      const float4 q = staged[(qy + oy) * RW + (qx + ox)];
      return px(q.x, q.y, q.z, q.w);
    };
    const Px p = at(x, y);
    o = present(p) ? atrous_pixel(at, x, y, STEP, sigma) : p;
  } else {
    auto at = [=](int qx, int qy) {
      if (qx < 0 || qy < 0 || qx >= (int)plane_w || qy >= (int)plane_h) return absent();
      return load_px(in, (size_t)qy * plane_w + (size_t)qx);
    };
    const Px p = at(x, y);
    o = present(p) ? atrous_pixel(at, x, y, step, sigma) : p;
  }
  if constexpr (FORMAT == FORMAT_PLANE) {
    static_cast<float4*>(out)[(size_t)y * plane_w + (size_t)x] = as_f4(o);
  } else {
    const size_t i = packed0 + (size_t)ty * row_w + (size_t)tx;
    if constexpr (FORMAT == FORMAT_RAW) {
      static_cast<float4*>(out)[i] = as_f4(o);
    } else {
      const Vec3 d = resolve(o);
      if constexpr (FORMAT == HRT_ACCUM_F32) static_cast<float4*>(out)[i] = make_float4(d.x, d.y, d.z, 1.0f);
      else static_cast<uint32_t*>(out)[i] = accum::resolve_rgba8(d);
    }
  }
}

template <int STEP, int32_t FORMAT>
void launch_one(const float4* in, uint32_t plane_w, uint32_t plane_h, const FilterTile* tiles, uint32_t n_tiles, uint32_t blocks,
                int step, float sigma, void* out, hipStream_t stream) {
  hipLaunchKernelGGL((filter_atrous<STEP, FORMAT>), dim3(blocks), dim3(BLOCK), 0, stream, in, plane_w, plane_h, tiles, n_tiles, step,
                     sigma, out);
  hip_check(hipGetLastError(), "filter_atrous launch");
}
/* the largest step staged in LDS: LDS_MAX_STEP, or HRT_FILTER_LDS_STEP (0, 1, 2, 4 or 8), an A/B knob between
 * bit-identical variants for measuring where the switch belongs */
uint32_t lds_max_step() {
  const char* v = knob_env("HRT_FILTER_LDS_STEP");
  return v ? (uint32_t)atoi(v) : LDS_MAX_STEP;
}
template <int32_t FORMAT>
void launch_step(const float4* in, uint32_t plane_w, uint32_t plane_h, const FilterTile* tiles, uint32_t n_tiles, uint32_t blocks,
                 int step, float sigma, void* out, hipStream_t stream) {
  const int lds = (uint32_t)step <= lds_max_step() ? step : 0;
  if (lds == 1) launch_one<1, FORMAT>(in, plane_w, plane_h, tiles, n_tiles, blocks, step, sigma, out, stream);
  else if (lds == 2) launch_one<2, FORMAT>(in, plane_w, plane_h, tiles, n_tiles, blocks, step, sigma, out, stream);
  else if (lds == 4) launch_one<4, FORMAT>(in, plane_w, plane_h, tiles, n_tiles, blocks, step, sigma, out, stream);
  else if (lds == 8) launch_one<8, FORMAT>(in, plane_w, plane_h, tiles, n_tiles, blocks, step, sigma, out, stream);
  else launch_one<0, FORMAT>(in, plane_w, plane_h, tiles, n_tiles, blocks, step, sigma, out, stream);
}

}  // namespace

namespace hrt {
namespace filter {

void launch_gather(const void* d_acc, const float* d_m2, const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                   void* d_plane, uint32_t plane_w, void* stream) {
  hipLaunchKernelGGL(filter_gather, dim3(n_blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const float4*)d_acc, d_m2, d_tiles, n_tiles,
                     (float4*)d_plane, plane_w);
  hip_check(hipGetLastError(), "filter_gather launch");
}

void launch_atrous(void* d_a, void* d_b, uint32_t plane_w, uint32_t plane_h, const FilterTile* d_tiles, uint32_t n_tiles,
                   uint32_t n_blocks, uint32_t iterations, float sigma, int32_t format, void* d_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t plane_blocks = ((plane_w + BLOCK_W - 1) / BLOCK_W) * ((plane_h + BLOCK_H - 1) / BLOCK_H);
  float4 *src = (float4*)d_a, *dst = (float4*)d_b;
  for (uint32_t i = 0; i + 1 < iterations; i++) {
    launch_step<FORMAT_PLANE>(src, plane_w, plane_h, d_tiles, n_tiles, plane_blocks, 1 << i, sigma, dst, stream);
    std::swap(src, dst);
  }
  const int step = 1 << (iterations - 1);
  if (format == FORMAT_RAW) launch_step<FORMAT_RAW>(src, plane_w, plane_h, d_tiles, n_tiles, n_blocks, step, sigma, d_out, stream);
  else if (format == HRT_ACCUM_F32) launch_step<HRT_ACCUM_F32>(src, plane_w, plane_h, d_tiles, n_tiles, n_blocks, step, sigma, d_out, stream);
  else launch_step<HRT_ACCUM_RGBA8>(src, plane_w, plane_h, d_tiles, n_tiles, n_blocks, step, sigma, d_out, stream);
}

}  // namespace filter
}  // namespace hrt
