/*
 * filter.hip — the kernels of the a-trous preview filter, variance-guided (hrt_accum_resolve_filtered) and
 * feature-guided (hrt_accum_resolve_guided); arithmetic: filter.h.
 *
 *   filter_gather   packed sums and m2 -> one raster plane of float4 (c.xyz, v) over the tiles' bounding box, so a
 *                   neighbour is address arithmetic.  Pixels no tile covers keep the v < 0 the plane was filled with.
 *   guided_gather   packed feature sums -> the two mean feature rasters over the same box, once per guided resolve.
 *   filter_atrous   one iteration, a 32 x 8 pixel block per 256-thread workgroup.  A staged step keeps the block and its
 *                   halo of 2 * step pixels in LDS (the prefilter's 1-pixel reach lies inside it); the other steps read
 *                   their 25 taps from global memory.  An iteration but the last runs over the plane's blocks and
 *                   writes the other plane; the last runs over the tiles' blocks (filter.h FilterTile) and writes the
 *                   PACKED output in the requested format itself.
 *   guided_atrous   the same body (atrous_iteration) with the feature terms.  A staged step may stage the two feature
 *                   planes behind the colour plane (dynamic LDS: 1 or 3 planes); otherwise a tap's features come from
 *                   global memory.
 *   demod_gather, guided_atrous_demod   a DEMODULATED guided resolve (filter.h) adds no pass and no raster: its gather
 *                   divides the pixel by its mean albedo where the colour plane is written, from the packed feature sums,
 *                   and its LAST iteration multiplies the albedo of the centre pixel (at hand for the feature terms, in
 *                   LDS when the features are staged) back where the packed output is written.  The inner iterations are
 *                   guided_atrous itself.  demod_raster does the gather's part for a raster of hrt_debug_guided_ex.
 *   filter_atrous_err, guided_atrous_err   the LAST iteration of hrt_accum_noise_filtered: the same body, which writes
 *                   the filtered noise estimate (filter.h filtered_err), packed f32, and no frame.
 *   filter_err_reduce   the packed errs -> each tile's (mean, max), accum_noise's reduction (tile_reduce.h).
 *
 * LDS layout: rows of (32 + 4 * step) float4, linear.  A wave is two block rows of 32 lanes; a tap is the same offset
 * for every lane, so each 16-lane group of a 16-byte LDS read (lanes {0-3, 12-15, 20-27} etc.) reads 16 distinct
 * 16-byte slots whose indices are distinct modulo 16: all 64 banks once, no conflict, for any row pitch.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "feature_pass.h"
#include "filter.h"
#include "kernel_common.h"
#include "tile_reduce.h"

using namespace hrt;
using namespace hrt::filter;

namespace {

constexpr uint32_t BLOCK = BLOCK_W * BLOCK_H;
static_assert(BLOCK == 256, "the a-trous kernels are written for 256-thread workgroups");

/* Which steps are staged in LDS.  `planes` staged planes of a step take lds_bytes, and a workgroup has LDS_LIMIT.
 * The rule: the plain filter (1 plane) may stage every step up to 8; the guided filter's 3 planes of step 8 exceed
 * the limit, so it stages no step above 4, the colour plane alone included (its kernels end at step 4).  Within
 * that, the defaults and their A/B knobs (bit-identical variants; DESIGN.md sections 6.7 and 6.8):
 * HRT_FILTER_LDS_STEP, the largest step whose colour plane is staged, and HRT_GUIDED_LDS_STEP, the largest staged
 * step whose feature planes are staged too (step 4: 55 KB per block, and still the fastest). */
constexpr size_t LDS_LIMIT = 64 * 1024;
constexpr size_t lds_bytes(uint32_t step, uint32_t planes) {
  return step ? (size_t)(BLOCK_W + 4 * step) * (BLOCK_H + 4 * step) * sizeof(float4) * planes : 0;
}
constexpr uint32_t PLAIN_STAGED_MAX = 8, GUIDED_STAGED_MAX = 4;
static_assert(lds_bytes(PLAIN_STAGED_MAX, 1) <= LDS_LIMIT && lds_bytes(GUIDED_STAGED_MAX, 3) <= LDS_LIMIT &&
                  lds_bytes(2 * GUIDED_STAGED_MAX, 3) > LDS_LIMIT,
              "the staged steps fit a workgroup's LDS, and the guided filter's next one does not");
constexpr uint32_t LDS_MAX_STEP = 4, FEATURE_LDS_MAX_STEP = 4;

__device__ inline Px load_px(const float4* plane, size_t i) {
  const float4 q = plane[i];
  return px(q.x, q.y, q.z, q.w);
}
__device__ inline float4 as_f4(const Px& p) { return make_float4(p.c.x, p.c.y, p.c.z, p.v); }
__device__ inline Feat as_feat(const float4 a, const float4 n) {
  Feat f;
  f.a = v3(a.x, a.y, a.z);
  f.n = v3(n.x, n.y, n.z);
  f.z = n.w;
  return f;
}

/* block b of the tile-block domain -> its tile and the block's corner in that tile */
__device__ inline FilterTile tile_and_corner(const FilterTile* __restrict__ tiles, uint32_t n_tiles, uint32_t b, uint32_t& bx,
                                             uint32_t& by) {
  const FilterTile T = tile_of_block(tiles, n_tiles, b);
  const uint32_t nbx = (T.w + BLOCK_W - 1) / BLOCK_W, k = b - T.blk0;
  bx = (k % nbx) * BLOCK_W;
  by = (k / nbx) * BLOCK_H;
  return T;
}

__global__ __launch_bounds__(BLOCK) void filter_gather(const float4* __restrict__ acc, const float* __restrict__ m2,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles,
                                                       float4* __restrict__ plane, uint32_t plane_w) {
  uint32_t bx, by;
  const FilterTile T = tile_and_corner(tiles, n_tiles, blockIdx.x, bx, by);
  const uint32_t lx = bx + threadIdx.x % BLOCK_W, ly = by + threadIdx.x / BLOCK_W;
  if (lx >= T.w || ly >= T.h) return;
  const size_t i = (size_t)T.off + (size_t)ly * T.w + lx;
  const float4 a = acc[i];
  plane[(size_t)(T.y + ly) * plane_w + (T.x + lx)] = as_f4(gather(v3(a.x, a.y, a.z), m2[i], T.inv_n, T.inv_k1));
}

/* filter_gather for a demodulated resolve: the same pass, the pixel divided by its mean albedo (the bits guided_gather
 * writes to the albedo raster, from the same packed sums) */
__global__ __launch_bounds__(BLOCK) void demod_gather(const float4* __restrict__ acc, const float* __restrict__ m2,
                                                      const float4* __restrict__ fa, float inv, float floor,
                                                      const FilterTile* __restrict__ tiles, uint32_t n_tiles,
                                                      float4* __restrict__ plane, uint32_t plane_w) {
  uint32_t bx, by;
  const FilterTile T = tile_and_corner(tiles, n_tiles, blockIdx.x, bx, by);
  const uint32_t lx = bx + threadIdx.x % BLOCK_W, ly = by + threadIdx.x / BLOCK_W;
  if (lx >= T.w || ly >= T.h) return;
  const size_t i = (size_t)T.off + (size_t)ly * T.w + lx;
  const float4 a = acc[i], al = features::mean_albedo(fa[i], inv);
  const Px p = gather(v3(a.x, a.y, a.z), m2[i], T.inv_n, T.inv_k1);
  plane[(size_t)(T.y + ly) * plane_w + (T.x + lx)] = as_f4(demodulate(p, demod_divisor(v3(al.x, al.y, al.z), floor)));
}

/* a raster that holds gather's (c, v), demodulated in place by the albedo raster at its present pixels */
__global__ __launch_bounds__(BLOCK) void demod_raster(float4* __restrict__ plane, const float4* __restrict__ albedo, size_t n,
                                                      float floor) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const Px p = load_px(plane, i);
  if (!present(p)) return;
  const float4 al = albedo[i];
  plane[i] = as_f4(demodulate(p, demod_divisor(v3(al.x, al.y, al.z), floor)));
}

__global__ __launch_bounds__(BLOCK) void guided_gather(const float4* __restrict__ fa, const float4* __restrict__ fn,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, float inv,
                                                       float4* __restrict__ albedo, float4* __restrict__ normal, uint32_t plane_w) {
  uint32_t bx, by;
  const FilterTile T = tile_and_corner(tiles, n_tiles, blockIdx.x, bx, by);
  const uint32_t lx = bx + threadIdx.x % BLOCK_W, ly = by + threadIdx.x / BLOCK_W;
  if (lx >= T.w || ly >= T.h) return;
  const size_t i = (size_t)T.off + (size_t)ly * T.w + lx, o = (size_t)(T.y + ly) * plane_w + (T.x + lx);
  const float4 a = fa[i];
  albedo[o] = features::mean_albedo(a, inv);
  normal[o] = features::mean_normal(a, fn[i], inv);
}

/* the feature source of an iteration: none (the plain filter), or the two rasters, the terms and whether this
 * launch staged the rasters in LDS behind the colour plane (STEP != 0 only) */
struct NoPlanes {
  static constexpr bool guided = false;
};
struct FeaturePlanes {
  static constexpr bool guided = true, demod = false;
  const float4 *albedo, *normal;
  Terms K;
  uint32_t lds;
};
/* the feature planes of a demodulated resolve's LAST iteration, which remodulates the pixel it writes by the centre's
 * albedo (filter.h): the flag is compile time, so the other instantiations are what they are without it */
struct DemodPlanes : FeaturePlanes {
  static constexpr bool demod = true;
  float floor;
};

/* One iteration, the body of both kernels.  sh: the workgroup's LDS.
 * STEP: the step staged in LDS, or 0: taps from global memory with the step in `step`.
 * FORMAT: -2: an inner iteration over the plane's blocks, to the plane `out`; else the last one over the tiles'
 * blocks, to the packed `out` as FORMAT_RAW, HRT_ACCUM_F32 or HRT_ACCUM_RGBA8, or as FORMAT_ERR: the filtered noise
 * estimate against err_floor (filter.h), one f32 where the frame's pixel would have gone; the frame is not written. */
constexpr int32_t FORMAT_PLANE = -2;
template <int STEP, int32_t FORMAT, class Features>
__device__ __forceinline__ void atrous_iteration(float4* sh, const Features F, const float4* __restrict__ in, uint32_t plane_w,
                                                 uint32_t plane_h, const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step,
                                                 float sigma, void* __restrict__ out, float err_floor = 0.0f) {
  constexpr int HALO = 2 * STEP, RW = (int)BLOCK_W + 2 * HALO, RH = (int)BLOCK_H + 2 * HALO;
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
    const FilterTile T = tile_and_corner(tiles, n_tiles, blockIdx.x, bx, by);
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
      if constexpr (Features::guided) {
        if (F.lds) {
          float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vn = va;
          if (inside) {
            va = F.albedo[g];
            vn = F.normal[g];
          }
          sh[RW * RH + k] = va;
          sh[2 * RW * RH + k] = vn;
        }
      }
    }
    __syncthreads();
  }
  if ((uint32_t)tx >= own_w || (uint32_t)ty >= own_h) return;
  /* The pixel and its taps are addressed from the origin (cx, cy) on the plane: the staged block's corner when every
   * tap source is staged, so that no LDS address holds a plane coordinate; the plane's own when some source may be
   * global memory (a step that is not staged; the guided filter's features, by the runtime switch F.lds). */
  constexpr bool LOCAL = STEP != 0 && !Features::guided;
  const int cx = LOCAL ? (int)x0 - HALO : 0, cy = LOCAL ? (int)y0 - HALO : 0;
  const int x = LOCAL ? tx + HALO : (int)x0 + tx, y = LOCAL ? ty + HALO : (int)y0 + ty, s = STEP ? STEP : step;
  const int ox = LOCAL ? 0 : HALO - (int)x0, oy = LOCAL ? 0 : HALO - (int)y0; /* (x, y) -> the staged block's */
  const float4* staged = sh;
  auto at = [=](int qx, int qy) {
    if constexpr (STEP != 0) {
      return load_px(staged, (qy + oy) * RW + (qx + ox));
    } else {
      if (qx < 0 || qy < 0 || qx >= (int)plane_w || qy >= (int)plane_h) return absent();
      return load_px(in, (size_t)qy * plane_w + (size_t)qx);
    }
  };
  const Px p = at(x, y);
  Px o;
  [[maybe_unused]] float err = 0.0f;
  if constexpr (Features::guided) {
    /* one call site for both sources of the features, so that atrous_pixel is inlined (a wave-uniform branch per tap) */
    auto feat = [=](int qx, int qy) {
      if (STEP == 0 || !F.lds) {
        const size_t g = (size_t)qy * plane_w + (size_t)qx;
        return as_feat(F.albedo[g], F.normal[g]);
      }
      const int k = (qy + oy) * RW + (qx + ox);
      return as_feat(staged[RW * RH + k], staged[2 * RW * RH + k]);
    };
    o = present(p) ? atrous_pixel(at, feature_terms(feat, x, y, F.K), x, y, s, sigma) : p;
    if constexpr (Features::demod) {
      /* the centre's albedo is the one the feature terms hold already */
      if constexpr (FORMAT == FORMAT_ERR) {
        if (present(p)) err = filtered_err_demod(o.c, o.v, demod_divisor(feat(x, y).a, F.floor), err_floor);
      } else {
        if (present(p)) o.c = remodulate(o.c, demod_divisor(feat(x, y).a, F.floor));
      }
    } else if constexpr (FORMAT == FORMAT_ERR) {
      err = filtered_err(o.c, o.v, err_floor);
    }
  } else {
    o = present(p) ? atrous_pixel(at, NoFeatures{}, x, y, s, sigma) : p;
    if constexpr (FORMAT == FORMAT_ERR) err = filtered_err(o.c, o.v, err_floor);
  }
  if constexpr (FORMAT == FORMAT_PLANE) {
    static_cast<float4*>(out)[(size_t)(y + cy) * plane_w + (size_t)(x + cx)] = as_f4(o);
  } else {
    const size_t i = packed0 + (size_t)ty * row_w + (size_t)tx;
    if constexpr (FORMAT == FORMAT_ERR) {
      static_cast<float*>(out)[i] = err;
    } else if constexpr (FORMAT == FORMAT_RAW) {
      static_cast<float4*>(out)[i] = as_f4(o);
    } else {
      const Vec3 d = resolve(o);
      if constexpr (FORMAT == HRT_ACCUM_F32) static_cast<float4*>(out)[i] = make_float4(d.x, d.y, d.z, 1.0f);
      else static_cast<uint32_t*>(out)[i] = accum::resolve_rgba8(d);
    }
  }
}

template <int STEP, int32_t FORMAT>
__global__ __launch_bounds__(BLOCK) void filter_atrous(const float4* __restrict__ in, uint32_t plane_w, uint32_t plane_h,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step, float sigma,
                                                       void* __restrict__ out) {
  __shared__ float4 sh[STEP ? lds_bytes(STEP, 1) / sizeof(float4) : 1];
  atrous_iteration<STEP, FORMAT>(sh, NoPlanes{}, in, plane_w, plane_h, tiles, n_tiles, step, sigma, out);
}

template <int STEP, int32_t FORMAT>
__global__ __launch_bounds__(BLOCK) void guided_atrous(const float4* __restrict__ in, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ normal, uint32_t plane_w, uint32_t plane_h,
                                                       const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step, float sigma,
                                                       Terms K, uint32_t feat_lds, void* __restrict__ out) {
  extern __shared__ float4 sh_planes[];
  atrous_iteration<STEP, FORMAT>(sh_planes, FeaturePlanes{albedo, normal, K, feat_lds}, in, plane_w, plane_h, tiles, n_tiles, step,
                                 sigma, out);
}

/* guided_atrous as the last iteration of a demodulated resolve: the packed pixel is remodulated where it is written */
template <int STEP, int32_t FORMAT>
__global__ __launch_bounds__(BLOCK) void guided_atrous_demod(const float4* __restrict__ in, const float4* __restrict__ albedo,
                                                             const float4* __restrict__ normal, uint32_t plane_w, uint32_t plane_h,
                                                             const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step,
                                                             float sigma, Terms K, uint32_t feat_lds, float floor,
                                                             void* __restrict__ out) {
  static_assert(FORMAT != FORMAT_PLANE, "only the last iteration remodulates");
  extern __shared__ float4 sh_planes[];
  atrous_iteration<STEP, FORMAT>(sh_planes, DemodPlanes{{albedo, normal, K, feat_lds}, floor}, in, plane_w, plane_h, tiles, n_tiles,
                                 step, sigma, out);
}

/* The last iteration as the filtered noise estimate (FORMAT_ERR): kernels of their own, so that the frame formats'
 * kernels keep their arguments and their code.  DEMOD: the last iteration of a demodulated resolve. */
template <int STEP>
__global__ __launch_bounds__(BLOCK) void filter_atrous_err(const float4* __restrict__ in, uint32_t plane_w, uint32_t plane_h,
                                                           const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step,
                                                           float sigma, float err_floor, float* __restrict__ out) {
  __shared__ float4 sh[STEP ? lds_bytes(STEP, 1) / sizeof(float4) : 1];
  atrous_iteration<STEP, FORMAT_ERR>(sh, NoPlanes{}, in, plane_w, plane_h, tiles, n_tiles, step, sigma, out, err_floor);
}
template <int STEP, bool DEMOD>
__global__ __launch_bounds__(BLOCK) void guided_atrous_err(const float4* __restrict__ in, const float4* __restrict__ albedo,
                                                           const float4* __restrict__ normal, uint32_t plane_w, uint32_t plane_h,
                                                           const FilterTile* __restrict__ tiles, uint32_t n_tiles, int step,
                                                           float sigma, Terms K, uint32_t feat_lds, float albedo_floor,
                                                           float err_floor, float* __restrict__ out) {
  extern __shared__ float4 sh_planes[];
  if constexpr (DEMOD)
    atrous_iteration<STEP, FORMAT_ERR>(sh_planes, DemodPlanes{{albedo, normal, K, feat_lds}, albedo_floor}, in, plane_w, plane_h, tiles,
                                       n_tiles, step, sigma, out, err_floor);
  else
    atrous_iteration<STEP, FORMAT_ERR>(sh_planes, FeaturePlanes{albedo, normal, K, feat_lds}, in, plane_w, plane_h, tiles, n_tiles, step,
                                       sigma, out, err_floor);
}

/* The tile reduce of the packed errs: one workgroup per tile, accum_noise's fold and tree (tile_reduce.h) */
__global__ __launch_bounds__(accum::NOISE_BLOCK) void filter_err_reduce(const float* __restrict__ err, const FilterTile* __restrict__ tiles,
                                                                        float2* __restrict__ out) {
  __shared__ float sh_s[accum::NOISE_BLOCK], sh_m[accum::NOISE_BLOCK];
  const FilterTile T = tiles[blockIdx.x];
  const uint32_t n = T.w * T.h;
  float s = 0.0f, m = 0.0f;
  for (uint32_t k = threadIdx.x; k < n; k += accum::NOISE_BLOCK) {
    const float e = err[(size_t)T.off + k];
    s = s + e;
    m = accum::larger(m, e);
  }
  accum::tile_reduce_block(s, m, n, sh_s, sh_m, out + blockIdx.x);
}

/* one iteration's launch; albedo and normal null: the plain filter; demod.on: the last iteration of a demodulated one */
struct Iteration {
  const float4 *in, *albedo, *normal;
  uint32_t w, h;
  const FilterTile* tiles;
  uint32_t n_tiles, blocks;
  int step;
  float sigma;
  Terms K;
  void* out;
  hipStream_t stream;
  Demod demod;
  float err_floor; /* FORMAT_ERR */
};

/* the last iteration as the filtered noise estimate */
template <int STEP>
void launch_err(const Iteration& I, bool feat_lds) {
  if (!I.albedo) {
    hipLaunchKernelGGL((filter_atrous_err<STEP>), dim3(I.blocks), dim3(BLOCK), 0, I.stream, I.in, I.w, I.h, I.tiles, I.n_tiles, I.step,
                       I.sigma, I.err_floor, (float*)I.out);
    hip_check(hipGetLastError(), "filter_atrous_err launch");
  } else if constexpr (STEP <= GUIDED_STAGED_MAX) {
    const size_t lds = lds_bytes(STEP, feat_lds ? 3 : 1);
    if (I.demod.on)
      hipLaunchKernelGGL((guided_atrous_err<STEP, true>), dim3(I.blocks), dim3(BLOCK), lds, I.stream, I.in, I.albedo, I.normal, I.w, I.h,
                         I.tiles, I.n_tiles, I.step, I.sigma, I.K, feat_lds ? 1u : 0u, I.demod.floor, I.err_floor, (float*)I.out);
    else
      hipLaunchKernelGGL((guided_atrous_err<STEP, false>), dim3(I.blocks), dim3(BLOCK), lds, I.stream, I.in, I.albedo, I.normal, I.w, I.h,
                         I.tiles, I.n_tiles, I.step, I.sigma, I.K, feat_lds ? 1u : 0u, 0.0f, I.err_floor, (float*)I.out);
    hip_check(hipGetLastError(), "guided_atrous_err launch");
  }
}
template <int STEP, int32_t FORMAT>
void launch_one(const Iteration& I, bool feat_lds) {
  if constexpr (FORMAT == FORMAT_ERR) return launch_err<STEP>(I, feat_lds);
  else if (!I.albedo) {
    hipLaunchKernelGGL((filter_atrous<STEP, FORMAT>), dim3(I.blocks), dim3(BLOCK), 0, I.stream, I.in, I.w, I.h, I.tiles, I.n_tiles,
                       I.step, I.sigma, I.out);
    hip_check(hipGetLastError(), "filter_atrous launch");
  } else if constexpr (STEP <= GUIDED_STAGED_MAX) {
    const size_t lds = lds_bytes(STEP, feat_lds ? 3 : 1);
    if constexpr (FORMAT != FORMAT_PLANE) {
      if (I.demod.on) {
        hipLaunchKernelGGL((guided_atrous_demod<STEP, FORMAT>), dim3(I.blocks), dim3(BLOCK), lds, I.stream, I.in, I.albedo, I.normal, I.w,
                           I.h, I.tiles, I.n_tiles, I.step, I.sigma, I.K, feat_lds ? 1u : 0u, I.demod.floor, I.out);
        hip_check(hipGetLastError(), "guided_atrous_demod launch");
        return;
      }
    }
    hipLaunchKernelGGL((guided_atrous<STEP, FORMAT>), dim3(I.blocks), dim3(BLOCK), lds, I.stream, I.in, I.albedo, I.normal, I.w, I.h,
                       I.tiles, I.n_tiles, I.step, I.sigma, I.K, feat_lds ? 1u : 0u, I.out);
    hip_check(hipGetLastError(), "guided_atrous launch");
  }
}
uint32_t knob_steps(const char* v, uint32_t dflt) { return v ? (uint32_t)atoi(v) : dflt; }
template <int32_t FORMAT>
void launch_step(const Iteration& I) {
  const bool guided = I.albedo != nullptr;
  const uint32_t step = (uint32_t)I.step;
  const uint32_t colour_max = std::min(knob_steps(knob_env("HRT_FILTER_LDS_STEP"), LDS_MAX_STEP), guided ? GUIDED_STAGED_MAX : PLAIN_STAGED_MAX);
  const uint32_t lds = step <= colour_max ? step : 0;
  const bool fl = guided && lds != 0 && step <= knob_steps(knob_env("HRT_GUIDED_LDS_STEP"), FEATURE_LDS_MAX_STEP);
  if (lds == 1) launch_one<1, FORMAT>(I, fl);
  else if (lds == 2) launch_one<2, FORMAT>(I, fl);
  else if (lds == 4) launch_one<4, FORMAT>(I, fl);
  else if (lds == 8) launch_one<8, FORMAT>(I, fl);
  else launch_one<0, FORMAT>(I, false);
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

void launch_gather_demod(const void* d_acc, const float* d_m2, const void* d_fa, float inv, float floor, const FilterTile* d_tiles,
                         uint32_t n_tiles, uint32_t n_blocks, void* d_plane, uint32_t plane_w, void* stream) {
  hipLaunchKernelGGL(demod_gather, dim3(n_blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const float4*)d_acc, d_m2, (const float4*)d_fa, inv,
                     floor, d_tiles, n_tiles, (float4*)d_plane, plane_w);
  hip_check(hipGetLastError(), "demod_gather launch");
}

void launch_demodulate(void* d_plane, const void* d_albedo, size_t n, float floor, void* stream) {
  hipLaunchKernelGGL(demod_raster, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, (float4*)d_plane,
                     (const float4*)d_albedo, n, floor);
  hip_check(hipGetLastError(), "demod_raster launch");
}

void launch_gather_features(const void* d_fa, const void* d_fn, const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks,
                            float inv, void* d_albedo, void* d_normal, uint32_t plane_w, void* stream) {
  hipLaunchKernelGGL(guided_gather, dim3(n_blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const float4*)d_fa, (const float4*)d_fn, d_tiles,
                     n_tiles, inv, (float4*)d_albedo, (float4*)d_normal, plane_w);
  hip_check(hipGetLastError(), "guided_gather launch");
}

void launch_atrous(void* d_a, void* d_b, const void* d_albedo, const void* d_normal, uint32_t plane_w, uint32_t plane_h,
                   const FilterTile* d_tiles, uint32_t n_tiles, uint32_t n_blocks, uint32_t iterations, float sigma, const Terms& K,
                   const Demod& demod, int32_t format, void* d_out, void* stream, float err_floor) {
  const uint32_t plane_blocks = ((plane_w + BLOCK_W - 1) / BLOCK_W) * ((plane_h + BLOCK_H - 1) / BLOCK_H);
  float4 *src = (float4*)d_a, *dst = (float4*)d_b;
  Iteration I{src, (const float4*)d_albedo, (const float4*)d_normal, plane_w, plane_h, d_tiles, n_tiles, plane_blocks, 1, sigma, K, dst,
              (hipStream_t)stream, Demod{false, 0.0f}, err_floor};
  for (uint32_t i = 0; i + 1 < iterations; i++) {
    I.in = src, I.out = dst, I.step = 1 << i;
    launch_step<FORMAT_PLANE>(I);
    std::swap(src, dst);
  }
  I.in = src, I.out = d_out, I.step = 1 << (iterations - 1), I.blocks = n_blocks;
  if (d_albedo) I.demod = demod; /* the last iteration remodulates */
  if (format == FORMAT_ERR) launch_step<FORMAT_ERR>(I);
  else if (format == FORMAT_RAW) launch_step<FORMAT_RAW>(I);
  else if (format == HRT_ACCUM_F32) launch_step<HRT_ACCUM_F32>(I);
  else launch_step<HRT_ACCUM_RGBA8>(I);
}

void launch_err_reduce(const float* d_err, const FilterTile* d_tiles, uint32_t n_tiles, void* d_mean_max, void* stream) {
  hipLaunchKernelGGL(filter_err_reduce, dim3(n_tiles), dim3(accum::NOISE_BLOCK), 0, (hipStream_t)stream, d_err, d_tiles, (float2*)d_mean_max);
  hip_check(hipGetLastError(), "filter_err_reduce launch");
}

}  // namespace filter
}  // namespace hrt
