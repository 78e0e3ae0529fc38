/*
 * guided.hip — the kernels of the feature-guided a-trous filter (hrt_accum_resolve_guided; arithmetic: guided.h).
 *
 *   guided_gather   packed feature sums -> the two mean feature rasters over the tiles' bounding box, once per resolve
 *                   (the colour plane is filter.hip's filter_gather).
 *   guided_atrous   filter.hip's filter_atrous with the feature terms: one iteration, a 32 x 8 pixel block per
 *                   256-thread workgroup, the same two domains (the plane's blocks for an inner iteration, the tiles'
 *                   blocks and the packed output for the last).  Steps up to filter::LDS_MAX_STEP stage the colour
 *                   plane's block and halo in LDS; steps up to FEATURE_LDS_MAX_STEP stage the two feature planes behind
 *                   it (dynamic LDS: 1 or 3 planes of (32 + 4 step) x (8 + 4 step) float4); otherwise a tap's features
 *                   come from global memory.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "feature_pass.h"
#include "guided.h"
#include "kernel_common.h"

using namespace hrt;
using namespace hrt::filter;
using namespace hrt::guided;

namespace {

constexpr uint32_t BLOCK = BLOCK_W * BLOCK_H;
static_assert(BLOCK == 256, "guided_atrous is written for 256-thread workgroups");

__device__ inline float4 as_f4(const Px& p) { return make_float4(p.c.x, p.c.y, p.c.z, p.v); }
__device__ inline Feat as_feat(const float4 a, const float4 n) {
  Feat f;
  f.a = v3(a.x, a.y, a.z);
  f.n = v3(n.x, n.y, n.z);
  f.z = n.w;
  return f;
}

/* block b of the tile-block domain -> its tile and the block's corner in it (as filter.hip's) */
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

__global__ __launch_bounds__(BLOCK) void guided_gather(const float4* __restrict__ fa, const float4* __restrict__ fn,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, float inv,
                                                       float4* __restrict__ albedo, float4* __restrict__ normal, uint32_t plane_w) {
  uint32_t bx, by;
  const FilterTile T = tile_of_block(tiles, n_tiles, blockIdx.x, bx, by);
  const uint32_t lx = bx + threadIdx.x % BLOCK_W, ly = by + threadIdx.x / BLOCK_W;
  if (lx >= T.w || ly >= T.h) return;
  const size_t i = (size_t)T.off + (size_t)ly * T.w + lx, o = (size_t)(T.y + ly) * plane_w + (T.x + lx);
  const float4 a = fa[i];
  albedo[o] = features::mean_albedo(a, inv);
  normal[o] = features::mean_normal(a, fn[i], inv);
}

/* STEP: the step staged in LDS, or 0: taps from global memory with the step in `step`.  feat_lds (STEP != 0 only):
 * the feature planes are staged too.  FORMAT: as filter_atrous. */
constexpr int32_t FORMAT_PLANE = -2;
template <int STEP, int32_t FORMAT>
__global__ __launch_bounds__(BLOCK) void guided_atrous(const float4* __restrict__ in, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ normal, uint32_t plane_w, uint32_t plane_h,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step, float sigma,
                                                       Terms K, uint32_t feat_lds, void* __restrict__ out) {
  constexpr int HALO = 2 * STEP, RW = (int)BLOCK_W + 2 * HALO, RH = (int)BLOCK_H + 2 * HALO;
  extern __shared__ float4 sh[];
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
      const size_t g = (size_t)gy * plane_w + (size_t)gx;
      sh[k] = inside ? in[g] : as_f4(absent());
      if (feat_lds) {
        float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vn = va;
        if (inside) {
          va = albedo[g];
          vn = normal[g];
        }
        sh[RW * RH + k] = va;
        sh[2 * RW * RH + k] = vn;
      }
    }
    __syncthreads();
  }
  if ((uint32_t)tx >= own_w || (uint32_t)ty >= own_h) return;
  const int x = (int)x0 + tx, y = (int)y0 + ty;
  auto feat_global = [=](int qx, int qy) {
    const size_t g = (size_t)qy * plane_w + (size_t)qx;
    return as_feat(albedo[g], normal[g]);
  };
  Px o;
  if constexpr (STEP != 0) {
    const int ox = HALO - (int)x0, oy = HALO - (int)y0;
    const float4* staged = sh;
    auto at = [=](int qx, int qy) {
      const float4 q = staged[(qy + oy) * RW + (qx + ox)];
      return px(q.x, q.y, q.z, q.w);
    };
    /* one call site for both sources of the features, so that guided_pixel is inlined (a wave-uniform branch per tap) */
    auto feat = [=](int qx, int qy) {
      if (!feat_lds) return feat_global(qx, qy);
      const int k = (qy + oy) * RW + (qx + ox);
      return as_feat(staged[RW * RH + k], staged[2 * RW * RH + k]);
    };
    const Px p = at(x, y);
    o = present(p) ? guided_pixel(at, feat, x, y, STEP, sigma, K) : p;
  } else {
    auto at = [=](int qx, int qy) {
      if (qx < 0 || qy < 0 || qx >= (int)plane_w || qy >= (int)plane_h) return absent();
      const float4 q = in[(size_t)qy * plane_w + (size_t)qx];
      return px(q.x, q.y, q.z, q.w);
    };
    const Px p = at(x, y);
    o = present(p) ? guided_pixel(at, feat_global, x, y, step, sigma, K) : p;
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

struct Planes {
  const float4 *in, *albedo, *normal;
  uint32_t w, h;
};

template <int STEP, int32_t FORMAT>
void launch_one(const Planes& P, const FilterTile* tiles, uint32_t n_tiles, uint32_t blocks, int step, float sigma, const Terms& K,
                bool feat_lds, void* out, hipStream_t stream) {
  constexpr size_t area = (size_t)(BLOCK_W + 4 * STEP) * (BLOCK_H + 4 * STEP);
  const size_t smem = STEP ? area * sizeof(float4) * (feat_lds ? 3 : 1) : 0;
  hipLaunchKernelGGL((guided_atrous<STEP, FORMAT>), dim3(blocks), dim3(BLOCK), smem, stream, P.in, P.albedo, P.normal, P.w, P.h, tiles,
                     n_tiles, step, sigma, K, feat_lds ? 1u : 0u, out);
  hip_check(hipGetLastError(), "guided_atrous launch");
}
/* the largest step whose colour plane (HRT_FILTER_LDS_STEP, as filter.hip) and feature planes (HRT_GUIDED_LDS_STEP)
 * are staged in LDS: A/B knobs between bit-identical variants */
uint32_t knob_step(const char* name, uint32_t dflt) {
  const char* v = knob_env(name);
  return v ? (uint32_t)atoi(v) : dflt;
}
template <int32_t FORMAT>
void launch_step(const Planes& P, const FilterTile* tiles, uint32_t n_tiles, uint32_t blocks, int step, float sigma, const Terms& K,
                 void* out, hipStream_t stream) {
  const uint32_t colour_max = std::min(knob_step("HRT_FILTER_LDS_STEP", LDS_MAX_STEP), 4u); /* 3 planes of step 8 exceed 64 KB */
  const int lds = (uint32_t)step <= colour_max ? step : 0;
  const bool fl = lds != 0 && (uint32_t)step <= knob_step("HRT_GUIDED_LDS_STEP", FEATURE_LDS_MAX_STEP);
  if (lds == 1) launch_one<1, FORMAT>(P, tiles, n_tiles, blocks, step, sigma, K, fl, out, stream);
  else if (lds == 2) launch_one<2, FORMAT>(P, tiles, n_tiles, blocks, step, sigma, K, fl, out, stream);
  else if (lds == 4) launch_one<4, FORMAT>(P, tiles, n_tiles, blocks, step, sigma, K, fl, out, stream);
  else launch_one<0, FORMAT>(P, tiles, n_tiles, blocks, step, sigma, K, false, out, stream);
}

}  // namespace

namespace hrt {
namespace guided {

void launch_gather_features(const void* d_fa, const void* d_fn, const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                            float inv, void* d_albedo, void* d_normal, uint32_t plane_w, void* stream) {
  hipLaunchKernelGGL(guided_gather, dim3(n_blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const float4*)d_fa, (const float4*)d_fn, d_tiles,
                     n_tiles, inv, (float4*)d_albedo, (float4*)d_normal, plane_w);
  hip_check(hipGetLastError(), "guided_gather launch");
}

void launch_guided(void* d_a, void* d_b, const void* d_albedo, const void* d_normal, uint32_t plane_w, uint32_t plane_h,
                   const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks, uint32_t iterations, float sigma, const Terms& K,
                   int32_t format, void* d_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t plane_blocks = ((plane_w + BLOCK_W - 1) / BLOCK_W) * ((plane_h + BLOCK_H - 1) / BLOCK_H);
  float4 *src = (float4*)d_a, *dst = (float4*)d_b;
  Planes P{src, (const float4*)d_albedo, (const float4*)d_normal, plane_w, plane_h};
  for (uint32_t i = 0; i + 1 < iterations; i++) {
    P.in = src;
    launch_step<FORMAT_PLANE>(P, d_tiles, n_tiles, plane_blocks, 1 << i, sigma, K, dst, stream);
    std::swap(src, dst);
  }
  P.in = src;
  const int step = 1 << (iterations - 1);
  if (format == FORMAT_RAW) launch_step<FORMAT_RAW>(P, d_tiles, n_tiles, n_blocks, step, sigma, K, d_out, stream);
  else if (format == HRT_ACCUM_F32) launch_step<HRT_ACCUM_F32>(P, d_tiles, n_tiles, n_blocks, step, sigma, K, d_out, stream);
  else launch_step<HRT_ACCUM_RGBA8>(P, d_tiles, n_tiles, n_blocks, step, sigma, K, d_out, stream);
}

}  // namespace guided
}  // namespace hrt
