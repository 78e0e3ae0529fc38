/*
 * accum.hip — the sample accumulator (hrt_accum, include/hrt/hrt.h): its streaming kernels (arithmetic: accum.h), host
 * state and entry points.  A pass is render.hip's render_launch, which ends in launch_accumulate{,_mapped} below; the
 * samples and chunks each tile then holds are accum_ledger.h's book; the filtered and the guided resolve's kernels are
 * filter.hip's and the feature pass's features.hip's.
 */
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "accum.h"
#include "accum_ledger.h"
#include "accum_paths.h"
#include "accum_snapshot.h"
#include "feature_pass.h"
#include "filter.h"
#include "query_host.h"
#include "render_host.h"
#include "tile_reduce.h"

using namespace hrt;
using namespace hrt::lane;
using namespace hrt::kern;

namespace {

/* ---- the kernels.  Plain streaming kernels: a grid-stride loop over pixels, one 16-B load or store per lane and
 * array (consecutive lanes, consecutive float4s). */
/* a resolved pixel to out[i]: RGBA f32 with alpha 1, or 4 x u8 with alpha 255 */
template <int FORMAT>
__host__ __device__ inline void store_resolved(void* out, size_t i, Vec3 acc, float scale) {
  const Vec3 px = accum::resolve_f32(acc, scale);
  if constexpr (FORMAT == HRT_ACCUM_F32) static_cast<float4*>(out)[i] = make_float4(px.x, px.y, px.z, 1.0f);
  else static_cast<uint32_t*>(out)[i] = accum::resolve_rgba8(px);
}

/* acc[i] += the pass sum of partial[.][i]; FORMAT >= 0: the frame after the pass goes to out in the same trip
 * (scale = 1 / the samples then held), so a preview after every pass is this one kernel after the megakernel */
template <int FORMAT>
__host__ __device__ inline void accumulate_pixel(const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale,
                                                 void* out, size_t i) {
  const float4 a = acc[i];
  const Vec3 sum = accum::add_pass(v3(a.x, a.y, a.z), accum::pass_sum(partial, n_chunks, n, i));
  acc[i] = make_float4(sum.x, sum.y, sum.z, 0.0f);
  if constexpr (FORMAT >= 0) store_resolved<FORMAT>(out, i, sum, scale);
}
/* the samples of a pass's chunk c: lane.h chunk_range on the pass's schedule (the function the render kernels split
 * a pixel's samples by), or the caller's table (hrt_debug_noise) */
struct ChunkCounts {
  const uint32_t* sizes; /* null: the schedule below */
  uint32_t chunk, chunk_head, chunk_first;
  __host__ __device__ uint32_t operator()(uint32_t c) const {
    if (sizes) return sizes[c];
    KParams P; /* chunk_range reads these three fields alone */
    P.chunk = chunk;
    P.chunk_head = chunk_head;
    P.chunk_first = chunk_first;
    uint32_t s0, s1;
    chunk_range(P, c, s0, s1);
    return s1 - s0;
  }
};
/* What accumulate_chunks<FORMAT, true> takes beyond the plain kernel's arguments: the noise plane and the tile map.
 * The map is the launch's own tile table: per launched tile out_off = the source offset in the launch's packed sums,
 * acc_off = the destination offset in the accumulator, w * h = the pixel count, so a pass over a subset of an
 * accumulator's tiles is one megakernel launch and this one kernel. */
template <bool MOMENTS>
struct MomentArgs {};
template <>
struct MomentArgs<true> {
  float* m2; /* n_px f32 packed as acc (accum.h pass_moment / add_moment); null: the accumulator keeps none */
  const G::TileDev* tiles;
  uint32_t n_tiles;
  ChunkCounts counts;
};
/* launch pixel i -> its pixel in the accumulator: the last tile whose out_off <= i */
__host__ __device__ inline size_t mapped_pixel(const G::TileDev* tiles, uint32_t n_tiles, size_t i) {
  uint32_t lo = 0, hi = n_tiles;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tiles[mid].out_off <= i) lo = mid;
    else hi = mid;
  }
  return (size_t)tiles[lo].acc_off + (i - tiles[lo].out_off);
}
template <int FORMAT>
__host__ __device__ inline void accumulate_pixel_mapped(const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale,
                                                        void* out, size_t i, const MomentArgs<true>& M) {
  const size_t d = mapped_pixel(M.tiles, M.n_tiles, i);
  const float4 a = acc[d];
  const Vec3 sum = accum::add_pass(v3(a.x, a.y, a.z), accum::pass_sum(partial, n_chunks, n, i));
  acc[d] = make_float4(sum.x, sum.y, sum.z, 0.0f);
  if (M.m2) M.m2[d] = accum::add_moment(M.m2[d], accum::pass_moment(partial, n_chunks, n, i, M.counts));
  if constexpr (FORMAT >= 0) store_resolved<FORMAT>(out, d, sum, scale);
}
template <int FORMAT, bool MOMENTS = false>
__global__ __launch_bounds__(256) void accumulate_chunks(const float4* __restrict__ partial, float4* __restrict__ acc, size_t n,
                                                         uint32_t n_chunks, float scale, void* __restrict__ out,
                                                         MomentArgs<MOMENTS> M) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if constexpr (MOMENTS) accumulate_pixel_mapped<FORMAT>(partial, acc, n, n_chunks, scale, out, i, M);
    else accumulate_pixel<FORMAT>(partial, acc, n, n_chunks, scale, out, i);
  }
}

/* ---- caller-traced paths into the accumulator (hrt_accum_add_paths; arithmetic: accum_paths.h).  A path is three
 * float4s and the pass reads the last of each: the radiance and the flags.  One launch, no partial buffer. */
constexpr uint32_t PATHS_BLOCK = 256;
constexpr uint32_t PATHS_STAGE = 2048; /* 16-B slots of accumulate_paths' staging buffer: 32 KB, five workgroups a CU */
struct PathArgs {
  const float4* paths; /* n_px x samples records of three float4s, a pixel's consecutive */
  float4* acc;
  float* m2;  /* null: the accumulator keeps no noise plane */
  void* out;  /* FORMAT >= 0: the frame after the pass, at `scale` */
  float scale;
  const G::TileDev* tiles; /* launch pixel -> accumulator pixel (mapped_pixel); n_tiles = 0: onto itself */
  uint32_t n_tiles;
  uint32_t n_px, samples, n_chunks;
  accum::PathSchedule schedule;
  uint32_t* live; /* null, or takes the number of records that are not PATH_DONE */
  uint32_t run, pitch; /* staged kernel: pixels a workgroup stages per trip, slots from a pixel's row to the next */
};
/* a pixel's records where the caller left them, and their last 16 bytes staged in LDS */
struct GlobalRecords {
  const float4* first;
  __host__ __device__ float4 operator()(uint32_t k) const { return first[3 * (size_t)k + 2]; }
};
__host__ __device__ inline uint32_t path_not_done(const float4& tail) {
  uint32_t flags;
  memcpy(&flags, &tail.w, sizeof(flags));
  return (flags & (uint32_t)HRT_PATH_DONE) == 0u ? 1u : 0u;
}
/* pixel i of the launch: add(acc, m2) is accum_paths.h add_paths on its records, or add_paths_in_place on its staged row */
template <int FORMAT, class Add>
__host__ __device__ inline void add_paths_pixel(const PathArgs& A, size_t i, Add&& add) {
  const size_t d = A.n_tiles ? mapped_pixel(A.tiles, A.n_tiles, i) : i;
  const float4 a = A.acc[d];
  const Vec3 sum = add(v3(a.x, a.y, a.z), A.m2 ? A.m2 + d : nullptr);
  A.acc[d] = make_float4(sum.x, sum.y, sum.z, 0.0f);
  if constexpr (FORMAT >= 0) store_resolved<FORMAT>(A.out, d, sum, A.scale);
}
template <int FORMAT>
__host__ __device__ inline void add_paths_pixel_global(const PathArgs& A, size_t i) {
  const GlobalRecords records{A.paths + 3 * (i * A.samples)};
  add_paths_pixel<FORMAT>(A, i, [&](Vec3 acc, float* m2) { return accum::add_paths(records, A.schedule, A.n_chunks, acc, m2); });
}
/* STAGED: a workgroup takes runs of A.run consecutive pixels.  It loads the last 16 bytes of the run's records with
 * consecutive lanes on consecutive records (a wave instruction touches 24 cache lines, each once) into LDS rows of
 * A.pitch slots, pitch odd, so the lanes of a ds_read_b128 group land on 16 different slots of the bank row; then one
 * lane per pixel folds its row in order, chunk sum c into slot c of the row, and adds the pass from those slots.  Not STAGED (a pixel's records exceed the buffer): a lane walks its pixel's
 * records in global memory.  Every loop is bounded by the pixel count, the samples or the chunks; no workgroup waits
 * on another.  A wave adds its count of unfinished records with one atomic as it leaves, as step_kernel its rays. */
template <int FORMAT, bool STAGED>
__global__ __launch_bounds__(PATHS_BLOCK) void accumulate_paths(PathArgs A) {
  uint32_t not_done = 0;
  if constexpr (STAGED) {
    __shared__ float4 stage[PATHS_STAGE];
    const uint32_t S = A.samples, n_runs = (A.n_px + A.run - 1u) / A.run;
    const uint32_t dq = PATHS_BLOCK / S, dk = PATHS_BLOCK - dq * S;
    for (uint32_t r = blockIdx.x; r < n_runs; r += gridDim.x) {
      const uint32_t px0 = r * A.run, cnt = min(A.run, A.n_px - px0), n_rec = cnt * S;
      const float4* first = A.paths + 3 * ((size_t)px0 * S);
      uint32_t q = threadIdx.x / S, k = threadIdx.x - q * S; /* record j of the run: sample k of its pixel q */
      for (uint32_t j = threadIdx.x; j < n_rec; j += PATHS_BLOCK) {
        const float4 tail = first[3 * (size_t)j + 2];
        not_done += path_not_done(tail);
        stage[q * A.pitch + k] = tail; /* q < cnt <= run, k < S <= pitch, run x pitch <= PATHS_STAGE */
        q += dq;
        k += dk;
        if (k >= S) {
          k -= S;
          q++;
        }
      }
      __syncthreads();
      if (threadIdx.x < cnt) {
        float4* row = stage + threadIdx.x * A.pitch;
        add_paths_pixel<FORMAT>(A, (size_t)px0 + threadIdx.x,
                                [&](Vec3 acc, float* m2) { return accum::add_paths_in_place(row, A.schedule, A.n_chunks, acc, m2); });
      }
      __syncthreads();
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n_px; i += (size_t)gridDim.x * blockDim.x) {
      const GlobalRecords records{A.paths + 3 * (i * A.samples)};
      if (A.live)
        for (uint32_t k = 0; k < A.samples; k++) not_done += path_not_done(records(k));
      add_paths_pixel_global<FORMAT>(A, i);
    }
  }
  if (A.live) {
    for (int o = 32; o > 0; o >>= 1) not_done += (uint32_t)__shfl_xor((int)not_done, o);
    if ((threadIdx.x & 63u) == 0u && not_done != 0u) atomicAdd(A.live, not_done);
  }
}

/* dst += src */
__global__ __launch_bounds__(256) void accum_merge(float4* __restrict__ dst, const float4* __restrict__ src, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = dst[i], b = src[i];
    const Vec3 sum = accum::add_pass(v3(a.x, a.y, a.z), v3(b.x, b.y, b.z));
    dst[i] = make_float4(sum.x, sum.y, sum.z, 0.0f);
  }
}
/* ... of the noise planes */
__global__ __launch_bounds__(256) void accum_merge_m2(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = accum::add_moment(dst[i], src[i]);
}

/* One selected tile of hrt_accum_merge_tiles: its pixels [off, off + n) of the packed order are pixels [sel, sel + n)
 * of the launch, which runs over the selected tiles' pixels alone. */
struct alignas(16) MergeTile {
  uint32_t off, n, sel, pad;
};
/* dst += src (and dst.m2 += src.m2) on the selected tiles; a pixel of the launch finds its tile as mapped_pixel does:
 * the last tile whose sel <= i.  No other pixel is read or written. */
template <bool MOMENTS>
__global__ __launch_bounds__(256) void accum_merge_tiles(float4* __restrict__ dst, const float4* __restrict__ src,
                                                         float* __restrict__ dst_m2, const float* __restrict__ src_m2,
                                                         const MergeTile* __restrict__ tiles, uint32_t n_tiles, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = n_tiles;
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (tiles[mid].sel <= i) lo = mid;
      else hi = mid;
    }
    const size_t d = (size_t)tiles[lo].off + (i - tiles[lo].sel);
    const float4 a = dst[d], b = src[d];
    const Vec3 sum = accum::add_pass(v3(a.x, a.y, a.z), v3(b.x, b.y, b.z));
    dst[d] = make_float4(sum.x, sum.y, sum.z, 0.0f);
    if constexpr (MOMENTS) dst_m2[d] = accum::add_moment(dst_m2[d], src_m2[d]);
  }
}

/* One tile of an accumulator as accum_noise and accum_resolve_tiles see it: its pixels [off, off + n) of the packed
 * order, and the scales of the samples and chunks it holds. */
struct alignas(16) NoiseTile {
  uint32_t off, n;
  float inv_n;  /* accum::resolve_scale(samples) */
  float inv_k1; /* accum::chunks_scale(chunks) */
  uint32_t few; /* fewer than 2 chunks: no estimate */
  uint32_t pad[3];
};
/* The error of every pixel of a tile (optionally stored to err, packed as acc) reduced to the tile's mean and max:
 * one workgroup of 256 per tile, the fixed order of accum.h tile_reduce. */
__global__ __launch_bounds__(accum::NOISE_BLOCK) void accum_noise(const float4* __restrict__ acc, const float* __restrict__ m2,
                                                                  const NoiseTile* __restrict__ tiles, float floor,
                                                                  float* __restrict__ err, float2* __restrict__ out) {
  __shared__ float sh_s[accum::NOISE_BLOCK], sh_m[accum::NOISE_BLOCK];
  const NoiseTile T = tiles[blockIdx.x];
  const uint32_t j = threadIdx.x;
  float s = 0.0f, m = 0.0f;
  for (uint32_t k = j; k < T.n; k += accum::NOISE_BLOCK) {
    const size_t d = (size_t)T.off + k;
    const float4 a = acc[d];
    const float e = accum::noise_err(v3(a.x, a.y, a.z), m2[d], T.inv_n, T.inv_k1, T.few != 0u, floor);
    if (err) err[d] = e;
    s = s + e;
    m = accum::larger(m, e);
  }
  accum::tile_reduce_block(s, m, T.n, sh_s, sh_m, out + blockIdx.x);
}

template <int FORMAT>
__global__ __launch_bounds__(256) void accum_resolve(const float4* __restrict__ acc, size_t n, float scale, void* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = acc[i];
    store_resolved<FORMAT>(out, i, v3(a.x, a.y, a.z), scale);
  }
}
/* ... of an accumulator whose tiles hold different sample counts: tile t resolves with its own 1 / N_t.  A
 * workgroup per tile (further tiles in further trips), its lanes over the tile's consecutive pixels. */
template <int FORMAT>
__global__ __launch_bounds__(256) void accum_resolve_tiles(const float4* __restrict__ acc, const NoiseTile* __restrict__ tiles,
                                                           uint32_t n_tiles, void* __restrict__ out) {
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const NoiseTile T = tiles[t];
    for (uint32_t k = threadIdx.x; k < T.n; k += blockDim.x) {
      const size_t d = (size_t)T.off + k;
      const float4 a = acc[d];
      store_resolved<FORMAT>(out, d, v3(a.x, a.y, a.z), T.inv_n);
    }
  }
}

/* ---- the launches.  f(std::integral_constant<int, FORMAT>{}) for the HRT_ACCUM_* format; NONE: with FORMAT = -1, no resolved output,
 * for any other value, which otherwise the entry points have refused (accum_format) */
template <bool NONE = false, class F>
void with_format(int format, F&& f) {
  if (format == HRT_ACCUM_F32) f(std::integral_constant<int, HRT_ACCUM_F32>{});
  else if (format == HRT_ACCUM_RGBA8 || !NONE) f(std::integral_constant<int, HRT_ACCUM_RGBA8>{});
  else if constexpr (NONE) f(std::integral_constant<int, -1>{});
}

template <bool MOMENTS>
void accumulate(int format, const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale, void* out,
                const MomentArgs<MOMENTS>& M, hipStream_t stream) {
  with_format<true>(format, [&](auto fc) {
    constexpr int F = decltype(fc)::value;
    hipLaunchKernelGGL((accumulate_chunks<F, MOMENTS>), dim3(stream_blocks(n)), dim3(256), 0, stream, partial, acc, n, n_chunks,
                       F < 0 ? 0.0f : scale, F < 0 ? nullptr : out, M);
  });
  hip_check(hipGetLastError(), "accumulate_chunks launch");
}
void resolve_pixels(int32_t format, const float4* acc, size_t n, float scale, void* d_out, hipStream_t stream) {
  with_format(format, [&](auto fc) {
    hipLaunchKernelGGL((accum_resolve<decltype(fc)::value>), dim3(stream_blocks(n)), dim3(256), 0, stream, acc, n, scale, d_out);
  });
  hip_check(hipGetLastError(), "accum_resolve launch");
}

/* accumulate_paths over A.n_px > 0 pixels: staged while a pixel's row fits the buffer (rows of samples | 1 slots) */
void launch_accumulate_paths(int format, PathArgs A, hipStream_t stream) {
  A.pitch = A.samples | 1u;
  A.run = A.pitch <= PATHS_STAGE ? std::min(PATHS_BLOCK, PATHS_STAGE / A.pitch) : 0u;
  with_format<true>(format, [&](auto fc) {
    constexpr int F = decltype(fc)::value;
    if (F < 0) A.scale = 0.0f, A.out = nullptr;
    if (A.run) {
      const uint32_t n_runs = (A.n_px + A.run - 1u) / A.run;
      hipLaunchKernelGGL((accumulate_paths<F, true>), dim3(std::min(n_runs, STREAM_MAX_BLOCKS)), dim3(PATHS_BLOCK), 0, stream, A);
    } else {
      hipLaunchKernelGGL((accumulate_paths<F, false>), dim3(stream_blocks(A.n_px)), dim3(PATHS_BLOCK), 0, stream, A);
    }
  });
  hip_check(hipGetLastError(), "accumulate_paths launch");
}

/* what makes two passes samples of the same frame: everything of (camera, params) but samples and sample_offset */
struct FrameIdentity {
  hrt_camera cam;
  uint32_t width, height, max_depth, flags;
  float t_min, background[3];
  uint64_t seed;
};
FrameIdentity frame_identity(const hrt_camera* cam, const hrt_render_params* p) {
  FrameIdentity id;
  memset(&id, 0, sizeof(id));
  id.cam = *cam;
  id.width = p->width;
  id.height = p->height;
  id.max_depth = p->max_depth;
  id.flags = p->flags;
  id.t_min = p->t_min;
  for (int k = 0; k < 3; k++) id.background[k] = p->background[k];
  id.seed = p->seed;
  return id;
}
bool same_identity(const FrameIdentity& a, const FrameIdentity& b) {
  return memcmp(&a.cam, &b.cam, sizeof(hrt_camera)) == 0 && a.width == b.width && a.height == b.height &&
         a.max_depth == b.max_depth && a.flags == b.flags && memcmp(&a.t_min, &b.t_min, sizeof(float)) == 0 &&
         memcmp(a.background, b.background, sizeof(a.background)) == 0 && a.seed == b.seed;
}

}  // namespace

void hrt::launch_accumulate(int format, const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale, void* out,
                            hipStream_t stream) {
  accumulate(format, partial, acc, n, n_chunks, scale, out, MomentArgs<false>{}, stream);
}
void hrt::launch_accumulate_mapped(int format, const float4* partial, float4* acc, size_t n, uint32_t n_chunks, float scale, void* out,
                                   float* m2, const gpu::TileDev* tiles, uint32_t n_tiles, uint32_t chunk, uint32_t chunk_head,
                                   uint32_t chunk_first, hipStream_t stream) {
  const MomentArgs<true> M{m2, tiles, n_tiles, ChunkCounts{nullptr, chunk, chunk_head, chunk_first}};
  accumulate(format, partial, acc, n, n_chunks, scale, out, M, stream);
}

struct hrt_accum {
  hrt_scene* scene = nullptr;
  int device = -1;
  uint32_t width = 0, height = 0;
  std::vector<hrt_tile> tiles;
  size_t n_px = 0;
  /* The host copies of d_ntiles, d_ftiles, d_mtiles and d_ptiles, which stream-ordered copies read.  Every device buffer below is an
   * owning DevBuf, freed with the accumulator (hrt_accum_destroy); these are declared before them all, so they go after
   * them, when the frees have waited for the device. */
  std::vector<NoiseTile> h_ntiles;
  std::vector<filter::FilterTile> h_ftiles;
  std::vector<MergeTile> h_mtiles;
  std::vector<G::TileDev> h_ptiles;
  DevBuf<float4> d_acc; /* n_px raw sums (x, y, z; w = 0), packed as the tiles are */
  bool has_identity = false;
  FrameIdentity identity;
  AccumLedger ledger; /* the samples and chunks (K) every tile holds */
  bool invalid = false; /* a pass was stopped by the walk watchdog: the sums are incomplete until a reset */
  DevBuf<float> d_m2; /* HRT_ACCUM_NOISE: n_px moments (accum.h), packed as d_acc */
  std::vector<uint32_t> tile_off; /* first pixel of each tile in the packed order */
  DevBuf<NoiseTile> d_ntiles; /* n_tiles records for accum_noise / accum_resolve_tiles (host copy: h_ntiles) */
  DevBuf<float2> d_nout; /* n_tiles x (mean, max) */
  /* The filtered resolve's buffers (filter.h), made by the first hrt_accum_resolve_filtered: two raster planes over
   * the tiles' bounding box and the tiles in plane coordinates.  f_state: 0 not made yet, 1 made, -1 the tiles overlap */
  int f_state = 0;
  uint32_t f_w = 0, f_h = 0, f_blocks = 0;
  DevBuf<float4> d_fplane[2];
  DevBuf<filter::FilterTile> d_ftiles;
  /* HRT_ACCUM_FEATURES: the two planes of first-hit feature sums (feature_pass.h: fa = (albedo.xyz, hit), fn = (normal.xyz,
   * depth)), packed as d_acc, the feature samples held (a ledger of its own: every feature pass covers every tile) and
   * the tiles as feature_kernel sees them */
  DevBuf<float4> d_fa, d_fn;
  AccumLedger f_ledger;
  DevBuf<features::FeatureTile> d_feat_tiles;
  uint32_t feat_blocks = 0, feat_log_bw = 0;
  /* the guided resolve's two mean feature rasters over the planes' bounding box, made by the first guided resolve */
  DevBuf<float4> d_gplane[2];
  /* hrt_accum_noise_filtered's packed per-pixel errs when the caller keeps none (n_px f32), made by the first such call;
   * scratch like the rasters: not part of a snapshot */
  DevBuf<float> d_ferr;
  /* hrt_accum_merge_tiles' table of the selected tiles, made by the first such merge (host copy: h_mtiles) */
  DevBuf<MergeTile> d_mtiles;
  /* hrt_accum_add_paths' tile map of a pass over a subset of the tiles, made by the first such pass (host copy: h_ptiles) */
  DevBuf<G::TileDev> d_ptiles;
};

namespace {

void accum_usable(const hrt_accum* a) {
  if (a->invalid) throw HipError{HRT_ERR_STATE, "the accumulator holds an incomplete pass (walk watchdog): reset it"};
}
void accum_format(int32_t format) {
  if (format != HRT_ACCUM_F32 && format != HRT_ACCUM_RGBA8) throw HipError{HRT_ERR_INVALID_ARG, "unknown HRT_ACCUM_* format"};
}
/* the floor of a noise estimate's denominator */
void noise_floor(float floor, const char* who) {
  if (!(floor > 0.0f)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": floor must be > 0"};
}
void check_identity(const hrt_accum* a, const FrameIdentity& id) {
  if (id.width != a->width || id.height != a->height)
    throw HipError{HRT_ERR_INVALID_ARG, "the params' width and height are not the accumulator's"};
  if (a->has_identity && !same_identity(a->identity, id))
    throw HipError{HRT_ERR_INVALID_ARG, "another frame identity (camera, max_depth, flags, t_min, background, seed) than the accumulator's"};
}
void check_range(AccumLedger::Refusal why) {
  if (why == AccumLedger::BAD_RANGE) throw HipError{HRT_ERR_INVALID_ARG, "empty sample range, or one that ends past 2^32"};
  if (why == AccumLedger::OVERLAP) throw HipError{HRT_ERR_INVALID_ARG, "the sample range overlaps samples the accumulator holds"};
}
void accum_uniform(const hrt_accum* a, hrt_status st, const char* what) {
  if (!a->ledger.uniform()) throw HipError{st, what};
}
void accum_holds_samples(const hrt_accum* a) {
  if (a->ledger.empty()) throw HipError{HRT_ERR_STATE, "the accumulator holds no samples"};
}
/* the samples a pass adds, and the identity the accumulator takes from the pass (or merge, or upload) that went in */
SampleRange pass_range(const hrt_render_params* p) { return SampleRange{p->sample_offset, (uint64_t)p->sample_offset + p->samples}; }
void adopt_identity(hrt_accum* a, const FrameIdentity& id) {
  a->identity = id;
  a->has_identity = true;
}
/* the record of n pixels from `off` on that hold `samples` samples in `chunks` chunks */
NoiseTile noise_tile(uint32_t off, uint32_t n, uint64_t samples, uint64_t chunks) {
  NoiseTile T;
  memset(&T, 0, sizeof(T));
  T.off = off;
  T.n = n;
  T.inv_n = samples ? accum::resolve_scale(samples) : 0.0f;
  T.few = chunks < 2 ? 1u : 0u;
  T.inv_k1 = chunks < 2 ? 0.0f : accum::chunks_scale(chunks);
  return T;
}
/* the records accum_noise and accum_resolve_tiles read, from the ledger, onto the device (stream-ordered; h_ntiles
 * stays alive with the accumulator) */
void upload_noise_tiles(hrt_accum* a, hipStream_t stream) {
  const size_t nt = a->tiles.size();
  a->h_ntiles.resize(nt);
  for (size_t t = 0; t < nt; t++)
    a->h_ntiles[t] = noise_tile(a->tile_off[t], a->tiles[t].w * a->tiles[t].h, a->ledger.samples(t), a->ledger.chunks(t));
  hip_check(hipMemcpyAsync(a->d_ntiles.p, a->h_ntiles.data(), nt * sizeof(NoiseTile), hipMemcpyHostToDevice, stream),
            "hipMemcpyAsync(noise tiles)");
}
/* the (mean, max) a reduction left in d_nout, waited for, with what the ledger says each tile holds */
void read_tile_noise(hrt_accum* a, hipStream_t stream, hrt_tile_noise* tiles_out) {
  const size_t nt = a->tiles.size();
  std::vector<float2> rec(nt);
  hip_check(hipMemcpyAsync(rec.data(), a->d_nout.p, nt * sizeof(float2), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(noise records)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize(noise)");
  for (size_t t = 0; t < nt; t++) {
    tiles_out[t].mean = rec[t].x;
    tiles_out[t].max = rec[t].y;
    tiles_out[t].samples = a->ledger.samples(t);
    tiles_out[t].chunks = a->ledger.chunks(t);
  }
}
/* tiles that hold different sample counts resolve each with its own (accum_resolve_tiles); every tile needs samples */
void launch_resolve_tiles(hrt_accum* a, int32_t format, void* d_out, hipStream_t stream) {
  const uint32_t nt = (uint32_t)a->tiles.size(), blocks = std::min(nt, STREAM_MAX_BLOCKS);
  for (uint32_t t = 0; t < nt; t++)
    if (a->ledger.samples(t) == 0) throw HipError{HRT_ERR_STATE, "a tile of the accumulator holds no samples"};
  upload_noise_tiles(a, stream);
  with_format(format, [&](auto fc) {
    hipLaunchKernelGGL((accum_resolve_tiles<decltype(fc)::value>), dim3(blocks), dim3(256), 0, stream, (const float4*)a->d_acc.p,
                       (const NoiseTile*)a->d_ntiles.p, nt, d_out);
  });
  hip_check(hipGetLastError(), "accum_resolve_tiles launch");
}
void launch_resolve(hrt_accum* a, int32_t format, void* d_out, hipStream_t stream) {
  if (!a->ledger.uniform()) return launch_resolve_tiles(a, format, d_out, stream);
  resolve_pixels(format, a->d_acc.p, a->n_px, accum::resolve_scale(a->ledger.samples(0)), d_out, stream);
}

/* ---- the filtered calls.  One description of a call, whichever public struct it came in: the variance-guided filter
 * (hrt_filter_params), with the feature terms (hrt_guided_params), with the demodulation option (hrt_guided_ex_params) */
constexpr filter::Demod NO_DEMOD{false, 0.0f};
struct FilterCall {
  uint32_t iterations;
  float sigma;
  filter::Terms K;
  filter::Demod demod;
  bool guided;            /* reads the feature planes; false: the variance-only filter, which asks for none */
  float err_floor = 0.0f; /* of the filtered noise estimate (filter::FORMAT_ERR), not read otherwise */
};

/* the argument checks, in the order the refusals are documented in: iterations and sigma, the tolerances, reserved, the
 * flags and the floor.  Nothing changes on an error */
void filter_args(uint32_t iterations, float sigma) {
  if (iterations < 1 || iterations > filter::MAX_ITERATIONS) throw HipError{HRT_ERR_INVALID_ARG, "filter: iterations outside [1, 5]"};
  if (!(sigma > 0.0f)) throw HipError{HRT_ERR_INVALID_ARG, "filter: sigma must be > 0"};
}
/* a tolerance as filter.h takes it */
float guided_term(float tolerance) {
  if (!(tolerance >= 0.0f)) throw HipError{HRT_ERR_INVALID_ARG, "guided filter: a tolerance is negative or NaN"};
  return tolerance > 0.0f ? 1.0f / tolerance : 0.0f;
}
/* the HRT_GUIDED_* flags and, with HRT_GUIDED_DEMODULATE, the floor (not read otherwise) */
filter::Demod guided_ex_option(uint32_t flags, float albedo_floor) {
  if (flags & ~(uint32_t)HRT_GUIDED_DEMODULATE) throw HipError{HRT_ERR_INVALID_ARG, "guided filter: unknown HRT_GUIDED_* flag bits"};
  if (!(flags & HRT_GUIDED_DEMODULATE)) return NO_DEMOD;
  if (!(albedo_floor > 0.0f)) throw HipError{HRT_ERR_INVALID_ARG, "guided filter: albedo_floor must be > 0 with HRT_GUIDED_DEMODULATE"};
  return filter::Demod{true, albedo_floor};
}
FilterCall filter_call(const hrt_filter_params* f) {
  filter_args(f->iterations, f->sigma);
  return FilterCall{f->iterations, f->sigma, filter::Terms{}, NO_DEMOD, false};
}
FilterCall filter_call(const hrt_guided_params* g) {
  filter_args(g->iterations, g->sigma);
  return FilterCall{g->iterations, g->sigma, filter::Terms{guided_term(g->normal), guided_term(g->albedo), guided_term(g->depth)}, NO_DEMOD, true};
}
FilterCall filter_call(const hrt_guided_ex_params* g) {
  filter_args(g->iterations, g->sigma);
  const filter::Terms K{guided_term(g->normal), guided_term(g->albedo), guided_term(g->depth)};
  if (g->reserved != 0) throw HipError{HRT_ERR_INVALID_ARG, "hrt_guided_ex_params: reserved must be 0"};
  return FilterCall{g->iterations, g->sigma, K, guided_ex_option(g->flags, g->albedo_floor), true};
}
/* no term and no flag: the variance-only filter (the noise estimates take it without feature planes; a guided resolve
 * stays guided) */
bool variance_only(const filter::Terms& K, const filter::Demod& demod) { return !demod.on && K.kn == 0.0f && K.ka == 0.0f && K.kz == 0.0f; }

uint64_t feature_samples(const hrt_accum* a) { return a->f_ledger.samples(0); }
void features_flag(const hrt_accum* a, const char* who) {
  if (!a->d_fa.p) throw HipError{HRT_ERR_STATE, std::string(who) + ": the accumulator was created without HRT_ACCUM_FEATURES"};
}
/* what the accumulator must hold for the call, in the documented order: usable, the feature planes (guided), the noise
 * plane, samples, two chunks in every tile, feature samples (guided) */
void filtered_state(const hrt_accum* a, const FilterCall& c, const char* who) {
  const auto refuse = [who](const char* why) { throw HipError{HRT_ERR_STATE, std::string(who) + why}; }; /* no string on the way through */
  accum_usable(a);
  if (c.guided) features_flag(a, who);
  if (!a->d_m2.p) refuse(": the accumulator was created without HRT_ACCUM_NOISE");
  accum_holds_samples(a);
  for (size_t t = 0; t < a->tiles.size(); t++)
    if (a->ledger.samples(t) == 0 || a->ledger.chunks(t) < 2) refuse(": a tile holds no samples or fewer than 2 chunks (no variance estimate)");
  if (c.guided && feature_samples(a) == 0) refuse(": the accumulator holds no feature samples");
}

/* whether the tiles, relative to (x0, y0), lie inside a w x h raster and cover no pixel twice and none that `absent`
 * (of the pixel's raster index) names */
enum class TileCover { OK, OUTSIDE, OVERLAP };
template <class Absent>
TileCover tile_cover(const hrt_tile* tiles, size_t n_tiles, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, Absent&& absent) {
  std::vector<bool> covered((size_t)w * h, false);
  for (size_t t = 0; t < n_tiles; t++) {
    const hrt_tile& T = tiles[t];
    if (T.w == 0 || T.h == 0 || T.x < x0 || T.y < y0 || T.x - x0 >= w || T.y - y0 >= h || T.w > w - (T.x - x0) || T.h > h - (T.y - y0))
      return TileCover::OUTSIDE;
    for (uint32_t y = T.y - y0; y < T.y - y0 + T.h; y++)
      for (uint32_t x = T.x - x0; x < T.x - x0 + T.w; x++) {
        const size_t k = (size_t)y * w + x;
        if (covered[k] || absent(k)) return TileCover::OVERLAP;
        covered[k] = true;
      }
  }
  return TileCover::OK;
}

/* the planes and the tile records, once per accumulator: its tiles never change.  Built into locals and moved in at the
 * end: a failure half-way leaves nothing made and f_state 0 */
void filter_prepare(hrt_accum* a, hipStream_t stream) {
  if (a->f_state < 0) throw HipError{HRT_ERR_UNSUPPORTED, "filtered resolve: the accumulator's tiles overlap"};
  if (a->f_state > 0) return;
  uint32_t x0 = UINT32_MAX, y0 = UINT32_MAX, x1 = 0, y1 = 0;
  for (const hrt_tile& t : a->tiles) {
    x0 = std::min(x0, t.x), y0 = std::min(y0, t.y);
    x1 = std::max(x1, t.x + t.w), y1 = std::max(y1, t.y + t.h);
  }
  const uint32_t w = x1 - x0, h = y1 - y0;
  const size_t area = (size_t)w * h;
  if (tile_cover(a->tiles.data(), a->tiles.size(), x0, y0, w, h, [](size_t) { return false; }) != TileCover::OK) {
    a->f_state = -1;
    throw HipError{HRT_ERR_UNSUPPORTED, "filtered resolve: the accumulator's tiles overlap"};
  }
  std::vector<filter::FilterTile> ft(a->tiles.size());
  uint64_t blocks = 0;
  for (size_t t = 0; t < ft.size(); t++) {
    const hrt_tile& T = a->tiles[t];
    ft[t] = filter::FilterTile{T.x - x0, T.y - y0, T.w, T.h, a->tile_off[t], (uint32_t)blocks, 0.0f, 0.0f};
    blocks += filter::tile_blocks(T.w, T.h);
  }
  if (blocks >= (1ull << 31)) throw HipError{HRT_ERR_UNSUPPORTED, "filtered resolve: too many tile blocks for one launch"};
  DevBuf<float4> plane[2];
  DevBuf<filter::FilterTile> d_ft;
  for (DevBuf<float4>& pl : plane) pl.alloc(area * sizeof(float4), "hipMalloc(filter plane)");
  d_ft.alloc(ft.size() * sizeof(filter::FilterTile), "hipMalloc(filter tiles)");
  /* pixels no tile covers are absent: v < 0 (0xBFBFBFBF is -1.498).  filter_gather writes the covered ones of
   * plane 0 alone and every iteration passes absent pixels on, so once is enough; it is waited for, so that a
   * later resolve on another stream finds it done */
  if (a->n_px != area) {
    hip_check(hipMemsetAsync(plane[0].p, 0xBF, area * sizeof(float4), stream), "hipMemsetAsync(filter plane)");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize(filter plane)");
  }
  for (int k = 0; k < 2; k++) a->d_fplane[k] = std::move(plane[k]);
  a->d_ftiles = std::move(d_ft);
  a->h_ftiles.swap(ft);
  a->f_w = w, a->f_h = h, a->f_blocks = (uint32_t)blocks;
  a->f_state = 1;
}
/* the sums and m2 gathered onto plane 0; demod.on: demodulated by the mean albedo in the same pass */
void filter_gather_plane(hrt_accum* a, const filter::Demod& demod, hipStream_t stream) {
  filter_prepare(a, stream);
  upload_noise_tiles(a, stream); /* each tile's own 1 / N and 1 / (K - 1) */
  const uint32_t nt = (uint32_t)a->tiles.size();
  for (uint32_t t = 0; t < nt; t++) {
    a->h_ftiles[t].inv_n = a->h_ntiles[t].inv_n;
    a->h_ftiles[t].inv_k1 = a->h_ntiles[t].inv_k1;
  }
  hip_check(hipMemcpyAsync(a->d_ftiles.p, a->h_ftiles.data(), nt * sizeof(filter::FilterTile), hipMemcpyHostToDevice, stream),
            "hipMemcpyAsync(filter tiles)");
  if (demod.on)
    filter::launch_gather_demod(a->d_acc.p, a->d_m2.p, a->d_fa.p, 1.0f / (float)feature_samples(a), demod.floor, a->d_ftiles.p, nt, a->f_blocks,
                                a->d_fplane[0].p, a->f_w, stream);
  else
    filter::launch_gather(a->d_acc.p, a->d_m2.p, a->d_ftiles.p, nt, a->f_blocks, a->d_fplane[0].p, a->f_w, stream);
}
/* A filtered call after its checks: the colour plane gathered, the feature rasters if the call is guided, then the
 * iterations.  c.demod.on: the plane is gathered demodulated and the last iteration remodulates.  format
 * filter::FORMAT_ERR: d_out takes the filtered noise estimate against c.err_floor.  (A call that is not guided carries
 * no term and no option: filter_call, variance_only.) */
void launch_filtered(hrt_accum* a, const FilterCall& c, int32_t format, void* d_out, hipStream_t stream) {
  filter_gather_plane(a, c.demod, stream);
  const uint32_t nt = (uint32_t)a->tiles.size();
  float4 *albedo = nullptr, *normal = nullptr;
  if (c.guided) {
    /* the two feature rasters, once: a present pixel's features are written by every resolve ([1] is made last, so a
     * failure between the two makes both again) */
    if (!a->d_gplane[1].p)
      for (DevBuf<float4>& pl : a->d_gplane) pl.alloc((size_t)a->f_w * a->f_h * sizeof(float4), "hipMalloc(feature raster)");
    albedo = a->d_gplane[0].p, normal = a->d_gplane[1].p;
    filter::launch_gather_features(a->d_fa.p, a->d_fn.p, a->d_ftiles.p, nt, a->f_blocks, 1.0f / (float)feature_samples(a), albedo, normal,
                                   a->f_w, stream);
  }
  filter::launch_atrous(a->d_fplane[0].p, a->d_fplane[1].p, albedo, normal, a->f_w, a->f_h, a->d_ftiles.p, nt, a->f_blocks, c.iterations,
                        c.sigma, c.K, c.demod, format, d_out, stream, c.err_floor);
}

/* hrt_accum_resolve_host / _filtered_host after their checks: `launch` resolves into a buffer of the scene's pool on
 * the null stream, once the passes the caller queued on any stream are done, and the buffer is copied to out */
template <class Launch>
void resolve_to_host(hrt_accum* a, int32_t format, void* out, const char* copy, Launch&& launch) {
  DeviceGuard dg(a->device);
  struct PoolBuf {
    hrt_scene* scene;
    OutBuf b;
    ~PoolBuf() { out_pool_give(scene, b); }
  } buf{a->scene, out_pool_take(a->scene, a->n_px * 16 + 16)};
  hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  launch(buf.b.ptr);
  hip_check(hipMemcpy(out, buf.b.ptr, a->n_px * (format == HRT_ACCUM_F32 ? 16u : 4u), hipMemcpyDeviceToHost), copy);
}

/* K of a pass: the chunks its schedule sums a pixel's samples in */
uint64_t pass_chunks(const hrt_scene* s, const hrt_render_params* p) {
  uint32_t chunk = 0, n_head = 0, first = 0, n_tail = 0;
  chunk_schedule(s, p, chunk, n_head, first, n_tail);
  return (uint64_t)n_head + n_tail;
}

/* A pass into every tile (idx null: hrt_accum_add, hrt_accum_add_resolve, hrt_accum_add_paths) or into tiles[idx[0..n)]
 * alone (hrt_accum_add_tiles, hrt_accum_add_paths): checks first (nothing changes on an error), then
 * launch(tiles, n_tiles, dst, &launched), the one thing a rendered pass and a pass of caller-traced paths differ in, which
 * makes its own checks before its first device call and sets launched once sums may have changed; then the ledger */
template <class Launch>
void accum_pass(const char* who, hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n,
                int32_t format, void* d_out, Launch&& launch) {
  accum_usable(a);
  if (d_out) accum_uniform(a, HRT_ERR_UNSUPPORTED, (std::string(who) + ": the accumulator's tiles hold different passes").c_str());
  const size_t nt = a->tiles.size();
  std::vector<uint8_t> taken(idx ? nt : 0, 0);
  std::vector<hrt_tile> sub; /* the launch's tiles and where each lands in the accumulator */
  std::vector<uint32_t> offs;
  for (uint32_t i = 0; idx && i < n; i++) {
    if (idx[i] >= nt || taken[idx[i]]) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": a tile index out of range or given twice"};
    taken[idx[i]] = 1;
    sub.push_back(a->tiles[idx[i]]);
    offs.push_back(a->tile_off[idx[i]]);
  }
  const FrameIdentity id = frame_identity(cam, p);
  check_identity(a, id);
  const SampleRange r = pass_range(p);
  if (p->samples != 0) check_range(a->ledger.may_add(r, idx, n)); /* samples = 0: check_render_args reports it */
  SumsDest dst;
  dst.d_acc = a->d_acc.p;
  dst.d_m2 = a->d_m2.p;
  /* a subset always takes the mapped kernel (launched tile i is the accumulator's tile idx[i]); the whole frame only
   * with a noise plane: without, the plain kernel, as ever (the tiles map onto themselves) */
  dst.mapped = idx || a->d_m2.p;
  dst.acc_offs = idx ? offs.data() : nullptr;
  if (d_out) { /* the whole frame of a uniform accumulator: every tile holds samples(0) */
    dst.preview = format;
    dst.d_preview = d_out;
    dst.preview_scale = accum::resolve_scale(a->ledger.samples(0) + p->samples);
  }
  bool launched = false;
  try {
    launch(idx ? sub.data() : a->tiles.data(), idx ? n : (uint32_t)nt, dst, &launched);
  } catch (...) {
    if (launched) a->invalid = true; /* the pass is (partly) in the sums and cannot be taken out again */
    throw;
  }
  adopt_identity(a, id);
  a->ledger.record(r, pass_chunks(a->scene, p), idx, n);
}
/* ... rendered (render.hip render_launch, which ends in accumulate_chunks) */
void accum_add(const char* who, hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n,
               int32_t format, void* d_out, void* stream, hrt_render_stats* stats) {
  accum_pass(who, a, cam, p, idx, n, format, d_out, [&](const hrt_tile* tiles, uint32_t n_tiles, const SumsDest& dst, bool* launched) {
    render_launch(a->scene, cam, p, tiles, n_tiles, dst, stream, stats, launched);
  });
}
/* ... of the caller's paths (accumulate_paths): hrt_accum_add_paths after the checks that need no accumulator.
 * batch(): the records and the live counter (or null) in device memory, asked for once every check has passed (the host
 * variant makes them then); after(): what the call still does on the device once the kernel is enqueued (the host variant
 * waits and reads the counter), so that a failure there leaves the accumulator marked as the sums are: changed */
struct PathBatch {
  const hrt_path* d_paths;
  uint32_t* d_live;
};
template <class Batch, class After>
void accum_add_paths(const char* who, hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n,
                     Batch&& batch, After&& after, uint64_t n_paths, int32_t format, void* d_out, hipStream_t stream) {
  accum_pass(who, a, cam, p, idx, n, format, d_out, [&](const hrt_tile* tiles, uint32_t n_tiles, const SumsDest& dst, bool* launched) {
    check_render_params(cam, p);
    uint64_t n_px = 0;
    for (uint32_t i = 0; i < n_tiles; i++) n_px += (uint64_t)tiles[i].w * tiles[i].h;
    if (n_paths >= (1ull << 32) || n_paths != n_px * p->samples)
      throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": n_paths is not (the tiles' pixels) x samples, or not below 2^32"};
    uint32_t chunk = 0, n_head = 0, first = 0, n_tail = 0;
    chunk_schedule(a->scene, p, chunk, n_head, first, n_tail);
    PathArgs A;
    memset(&A, 0, sizeof(A));
    A.acc = dst.d_acc, A.m2 = dst.d_m2;
    A.out = dst.d_preview, A.scale = dst.preview_scale;
    A.n_px = (uint32_t)n_px, A.samples = p->samples, A.n_chunks = n_head + n_tail;
    A.schedule = accum::PathSchedule{chunk, n_head, first};
    DeviceGuard dg(a->device);
    const PathBatch b = batch();
    A.paths = reinterpret_cast<const float4*>(b.d_paths), A.live = b.d_live;
    if (dst.acc_offs) { /* a subset: launched tile i is the accumulator's tile at acc_offs[i] (mapped_pixel reads the two offsets) */
      std::vector<G::TileDev> td(n_tiles);
      uint32_t off = 0;
      for (uint32_t i = 0; i < n_tiles; i++) {
        td[i] = G::TileDev{tiles[i].x, tiles[i].y, tiles[i].w, tiles[i].h, (tiles[i].w + 7) / 8, 0u, off, dst.acc_offs[i]};
        off += tiles[i].w * tiles[i].h;
      }
      if (!a->d_ptiles.p) a->d_ptiles.alloc(a->tiles.size() * sizeof(G::TileDev), "hipMalloc(path tiles)");
      a->h_ptiles.swap(td); /* stays alive with the accumulator, as h_mtiles does */
      hip_check(hipMemcpyAsync(a->d_ptiles.p, a->h_ptiles.data(), n_tiles * sizeof(G::TileDev), hipMemcpyHostToDevice, stream),
                "hipMemcpyAsync(path tiles)");
      A.tiles = a->d_ptiles.p, A.n_tiles = n_tiles;
    }
    launch_accumulate_paths(dst.preview, A, stream);
    *launched = true;
    after();
  });
}

/* A merge's preconditions beyond usable, in the order they are refused in: the same noise plane or none, uniform on
 * both sides (hrt_accum_merge alone: hrt_accum_merge_tiles is the merge for tiles that hold different passes), the
 * same device, image and tiles, the same feature planes or none */
void merge_compatible(const hrt_accum* dst, const hrt_accum* src, const char* who, bool uniform) {
  const auto refuse = [who](hrt_status st, const char* why) { throw HipError{st, std::string(who) + why}; };
  if ((dst->d_m2.p != nullptr) != (src->d_m2.p != nullptr))
    refuse(HRT_ERR_INVALID_ARG, ": one accumulator keeps a noise plane (HRT_ACCUM_NOISE), the other none");
  if (uniform && !(dst->ledger.uniform() && src->ledger.uniform()))
    refuse(HRT_ERR_UNSUPPORTED, ": the accumulator's tiles hold different passes");
  if (dst->device != src->device || dst->width != src->width || dst->height != src->height || dst->tiles.size() != src->tiles.size() ||
      memcmp(dst->tiles.data(), src->tiles.data(), dst->tiles.size() * sizeof(hrt_tile)) != 0)
    refuse(HRT_ERR_INVALID_ARG, ": the accumulators differ in device, image size or tiles");
  if ((dst->d_fa.p != nullptr) != (src->d_fa.p != nullptr))
    refuse(HRT_ERR_INVALID_ARG, ": one accumulator keeps feature planes (HRT_ACCUM_FEATURES), the other none");
}

/* ---- snapshots (accum_snapshot.h is the codec; here: the accumulator's state into and out of its State) ---- */
uint32_t accum_flags(const hrt_accum* a) { return (a->d_m2.p ? HRT_ACCUM_NOISE : 0u) | (a->d_fa.p ? HRT_ACCUM_FEATURES : 0u); }
/* the identity's 128 bytes as hrt.h lays them out; width and height are the accumulator's */
void identity_bytes(const FrameIdentity& id, uint8_t* out) {
  static_assert(sizeof(hrt_camera) == 96, "the snapshot layout holds 96 camera bytes");
  memcpy(out, &id.cam, 96);
  snapshot::put32(out + 96, id.max_depth);
  snapshot::put32(out + 100, id.flags);
  memcpy(out + 104, &id.t_min, 4);
  memcpy(out + 108, id.background, 12);
  snapshot::put64(out + 120, id.seed);
}
FrameIdentity identity_from(const uint8_t* in, uint32_t width, uint32_t height) {
  FrameIdentity id;
  memset(&id, 0, sizeof(id));
  memcpy(&id.cam, in, 96);
  id.width = width;
  id.height = height;
  id.max_depth = snapshot::get32(in + 96);
  id.flags = snapshot::get32(in + 100);
  memcpy(&id.t_min, in + 104, 4);
  memcpy(id.background, in + 108, 12);
  id.seed = snapshot::get64(in + 120);
  return id;
}
snapshot::State snapshot_state(const hrt_accum* a) {
  snapshot::State s;
  s.flags = accum_flags(a);
  s.width = a->width;
  s.height = a->height;
  for (const hrt_tile& t : a->tiles) s.tiles.push_back(snapshot::Tile{t.x, t.y, t.w, t.h});
  s.has_identity = a->has_identity;
  if (a->has_identity) identity_bytes(a->identity, s.identity);
  s.records = a->ledger.records();
  if (a->d_fa.p) s.f_ranges = *a->f_ledger.ranges(); /* every feature pass covers every tile: always the shared record */
  snapshot::layout(s);
  return s;
}
void snapshot_decode(const void* blob, uint64_t size, snapshot::State& s, const char* who) {
  const snapshot::Error e = snapshot::decode(blob, size, s);
  if (e != snapshot::OK) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": malformed snapshot: " + snapshot::error_text(e)};
}

}  // namespace

extern "C" {

hrt_status hrt_accum_create(hrt_scene* s, uint32_t width, uint32_t height, const hrt_tile* tiles, uint32_t n_tiles,
                            hrt_accum** out) {
  return hrt_accum_create_ex(s, width, height, tiles, n_tiles, 0, out);
}

hrt_status hrt_accum_create_ex(hrt_scene* s, uint32_t width, uint32_t height, const hrt_tile* tiles, uint32_t n_tiles,
                               uint32_t flags, hrt_accum** out) {
  return hguard([&] {
    if (!s || !tiles || !out || n_tiles == 0) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_create: null argument or no tiles"};
    *out = nullptr;
    if (flags & ~(uint32_t)(HRT_ACCUM_NOISE | HRT_ACCUM_FEATURES)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_create_ex: unknown flag"};
    if (width < 2 || height < 2 || width > 65535 || height > 65535)
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_create: 2 <= width, height <= 65535"};
    uint64_t n_px = 0;
    for (uint32_t i = 0; i < n_tiles; i++) {
      const hrt_tile& t = tiles[i];
      if (t.w == 0 || t.h == 0 || (uint64_t)t.x + t.w > width || (uint64_t)t.y + t.h > height)
        throw HipError{HRT_ERR_INVALID_ARG, "tile outside the image"};
      n_px += (uint64_t)t.w * t.h;
    }
    if (n_px >= (1ull << 32)) throw HipError{HRT_ERR_UNSUPPORTED, "more than 2^32 pixels in one accumulator"};
    if (!s->committed || !s->d_blob) throw HipError{HRT_ERR_STATE, "scene not committed"};
    DeviceGuard dg(s->device);
    std::unique_ptr<hrt_accum> a(new hrt_accum()); /* a failure below frees what was made, on the device dg has set */
    a->scene = s;
    a->device = s->device;
    a->width = width;
    a->height = height;
    a->tiles.assign(tiles, tiles + n_tiles);
    a->n_px = (size_t)n_px;
    a->ledger = AccumLedger(n_tiles);
    a->tile_off.resize(n_tiles);
    for (uint32_t i = 0, off = 0; i < n_tiles; i++) {
      a->tile_off[i] = off;
      off += tiles[i].w * tiles[i].h;
    }
    a->d_acc.alloc(a->n_px * sizeof(float4), "hipMalloc(accumulator)");
    hip_check(hipMemset(a->d_acc.p, 0, a->n_px * sizeof(float4)), "hipMemset(accumulator)");
    a->d_ntiles.alloc(n_tiles * sizeof(NoiseTile), "hipMalloc(accumulator tiles)");
    if (flags & HRT_ACCUM_NOISE) {
      a->d_m2.alloc(a->n_px * sizeof(float), "hipMalloc(noise plane)");
      hip_check(hipMemset(a->d_m2.p, 0, a->n_px * sizeof(float)), "hipMemset(noise plane)");
      a->d_nout.alloc(n_tiles * sizeof(float2), "hipMalloc(noise records)");
    }
    if (flags & HRT_ACCUM_FEATURES) {
      a->f_ledger = AccumLedger(n_tiles);
      a->feat_log_bw = features::block_log_w();
      std::vector<features::FeatureTile> ft(n_tiles);
      uint64_t blocks = 0;
      for (uint32_t i = 0; i < n_tiles; i++) {
        ft[i] = features::FeatureTile{tiles[i].x, tiles[i].y, tiles[i].w, tiles[i].h, a->tile_off[i], (uint32_t)blocks, {0u, 0u}};
        blocks += features::tile_blocks(tiles[i].w, tiles[i].h, a->feat_log_bw);
      }
      if (blocks >= (1ull << 31)) throw HipError{HRT_ERR_UNSUPPORTED, "HRT_ACCUM_FEATURES: too many tile blocks for one launch"};
      a->feat_blocks = (uint32_t)blocks;
      for (DevBuf<float4>* pl : {&a->d_fa, &a->d_fn}) {
        pl->alloc(a->n_px * sizeof(float4), "hipMalloc(feature plane)");
        hip_check(hipMemset(pl->p, 0, a->n_px * sizeof(float4)), "hipMemset(feature plane)");
      }
      a->d_feat_tiles.alloc(n_tiles * sizeof(features::FeatureTile), "hipMalloc(feature tiles)");
      hip_check(hipMemcpy(a->d_feat_tiles.p, ft.data(), n_tiles * sizeof(features::FeatureTile), hipMemcpyHostToDevice),
                "hipMemcpy(feature tiles)");
    }
    *out = a.release();
  });
}

void hrt_accum_destroy(hrt_accum* a) {
  if (!a) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(a->device);
  delete a; /* its device buffers go with it (DevBuf); freeing one waits for the work that uses it */
  if (prev >= 0) (void)hipSetDevice(prev);
}

hrt_status hrt_accum_reset(hrt_accum* a, void* stream) {
  return hguard([&] {
    if (!a) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_reset: null accumulator"};
    DeviceGuard dg(a->device);
    hip_check(hipMemsetAsync(a->d_acc.p, 0, a->n_px * sizeof(float4), (hipStream_t)stream), "hipMemsetAsync(accumulator)");
    if (a->d_m2.p) hip_check(hipMemsetAsync(a->d_m2.p, 0, a->n_px * sizeof(float), (hipStream_t)stream), "hipMemsetAsync(noise plane)");
    for (float4* pl : {a->d_fa.p, a->d_fn.p})
      if (pl) hip_check(hipMemsetAsync(pl, 0, a->n_px * sizeof(float4), (hipStream_t)stream), "hipMemsetAsync(feature plane)");
    a->ledger.clear();
    a->f_ledger.clear();
    a->has_identity = false;
    a->invalid = false;
  });
}

hrt_status hrt_accum_add(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, void* stream,
                         hrt_render_stats* stats) {
  return hguard([&] {
    if (!a || !cam || !p) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add: null argument"};
    accum_add("hrt_accum_add", a, cam, p, nullptr, 0, -1, nullptr, stream, stats);
  });
}

hrt_status hrt_accum_add_resolve(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, int32_t format,
                                 void* d_out, void* stream, hrt_render_stats* stats) {
  return hguard([&] {
    if (!a || !cam || !p || !d_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add_resolve: null argument"};
    accum_format(format);
    accum_add("hrt_accum_add_resolve", a, cam, p, nullptr, 0, format, d_out, stream, stats);
  });
}

hrt_status hrt_accum_samples(const hrt_accum* a, uint64_t* samples) {
  return hguard([&] {
    if (!a || !samples) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_samples: null argument"};
    accum_uniform(a, HRT_ERR_STATE, "hrt_accum_samples: the accumulator's tiles hold different passes (hrt_accum_tile_samples)");
    *samples = a->ledger.samples(0);
  });
}

hrt_status hrt_accum_tile_samples(const hrt_accum* a, uint64_t* per_tile) {
  return hguard([&] {
    if (!a || !per_tile) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_tile_samples: null argument"};
    for (size_t t = 0; t < a->tiles.size(); t++) per_tile[t] = a->ledger.samples(t);
  });
}

hrt_status hrt_accum_add_tiles(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n,
                               void* stream, hrt_render_stats* stats) {
  return hguard([&] {
    if (!a || !cam || !p || !idx || n == 0) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add_tiles: null argument or no tiles"};
    accum_add("hrt_accum_add_tiles", a, cam, p, idx, n, -1, nullptr, stream, stats);
  });
}

/* the checks of hrt_accum_add_paths{,_host} that need no accumulator state */
static void add_paths_args(const char* who, const hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx,
                           uint32_t n_idx, const hrt_path* paths, uint64_t n_paths, int32_t format, const void* d_out) {
  const auto refuse = [who](const char* why) { throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + why}; };
  if (!a || !cam || !p || !paths) refuse(": null argument");
  if ((idx != nullptr) != (n_idx != 0)) refuse(": a tile list needs both idx and n_idx");
  if (n_paths >= (1ull << 32)) refuse(": n_paths must be below 2^32");
  if (format != -1) accum_format(format);
  if (format >= 0 && !d_out) refuse(": a preview format needs d_out");
  if (format >= 0 && idx) refuse(": a pass over a subset of the tiles has no preview");
}

hrt_status hrt_accum_add_paths(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n_idx,
                               const hrt_path* d_paths, uint64_t n_paths, int32_t format, void* d_out, uint32_t* d_live, void* stream) {
  return hguard([&] {
    add_paths_args("hrt_accum_add_paths", a, cam, p, idx, n_idx, d_paths, n_paths, format, d_out);
    if (!aligned16(d_paths)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add_paths: the records must be 16-byte aligned"};
    if (((uintptr_t)d_live & 3u) != 0) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add_paths: d_live must be 4-byte aligned"};
    accum_add_paths("hrt_accum_add_paths", a, cam, p, idx, n_idx, [&] { return PathBatch{d_paths, d_live}; }, [] {}, n_paths, format,
                    format >= 0 ? d_out : nullptr, (hipStream_t)stream);
  });
}

hrt_status hrt_accum_add_paths_host(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n_idx,
                                    const hrt_path* paths, uint64_t n_paths, uint32_t* live) {
  return hguard([&] {
    add_paths_args("hrt_accum_add_paths_host", a, cam, p, idx, n_idx, paths, n_paths, -1, nullptr);
    /* both run inside the pass, under its device guard, once every check has passed: the copies in, then the wait and
     * the counter; the buffers go before the guard does */
    DevBuf<hrt_path> d_paths;
    DevBuf<uint32_t> d_live;
    const auto copy_in = [&] {
      const uint32_t zero = 0;
      if (live) d_live = DevBuf<uint32_t>(sizeof(uint32_t), &zero);
      d_paths = DevBuf<hrt_path>((size_t)n_paths * sizeof(hrt_path), paths);
      return PathBatch{d_paths.p, d_live.p};
    };
    const auto wait = [&] {
      hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize(paths)");
      uint32_t counted = 0;
      if (live) hip_check(hipMemcpy(&counted, d_live.p, sizeof(counted), hipMemcpyDeviceToHost), "hipMemcpy(live count)");
      d_paths = DevBuf<hrt_path>();
      d_live = DevBuf<uint32_t>();
      if (live) *live += counted;
    };
    accum_add_paths("hrt_accum_add_paths_host", a, cam, p, idx, n_idx, copy_in, wait, n_paths, -1, nullptr, nullptr);
  });
}

hrt_status hrt_accum_noise(hrt_accum* a, float floor, float* d_err, void* stream_, hrt_tile_noise* tiles_out) {
  return hguard([&] {
    if (!a || !tiles_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_noise: null argument"};
    noise_floor(floor, "hrt_accum_noise");
    accum_usable(a);
    if (!a->d_m2.p) throw HipError{HRT_ERR_STATE, "hrt_accum_noise: the accumulator was created without HRT_ACCUM_NOISE"};
    accum_holds_samples(a);
    DeviceGuard dg(a->device);
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t nt = (uint32_t)a->tiles.size();
    upload_noise_tiles(a, stream);
    hipLaunchKernelGGL(accum_noise, dim3(nt), dim3(accum::NOISE_BLOCK), 0, stream, (const float4*)a->d_acc.p, (const float*)a->d_m2.p,
                       (const NoiseTile*)a->d_ntiles.p, floor, d_err, a->d_nout.p);
    hip_check(hipGetLastError(), "accum_noise launch");
    read_tile_noise(a, stream, tiles_out);
  });
}

hrt_status hrt_debug_accum_moments(hrt_accum* a, float* m2_out) {
  return hguard([&] {
    if (!a || !m2_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_accum_moments: null argument"};
    if (!a->d_m2.p) throw HipError{HRT_ERR_STATE, "hrt_debug_accum_moments: the accumulator was created without HRT_ACCUM_NOISE"};
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(m2_out, a->d_m2.p, a->n_px * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(moments)");
  });
}

hrt_status hrt_accum_resolve(hrt_accum* a, int32_t format, void* d_out, void* stream) {
  return hguard([&] {
    if (!a || !d_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve: null argument"};
    accum_format(format);
    accum_usable(a);
    accum_holds_samples(a);
    DeviceGuard dg(a->device);
    launch_resolve(a, format, d_out, (hipStream_t)stream);
  });
}

hrt_status hrt_accum_resolve_host(hrt_accum* a, int32_t format, void* out) {
  return hguard([&] {
    if (!a || !out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_host: null argument"};
    accum_format(format);
    accum_usable(a);
    accum_holds_samples(a);
    resolve_to_host(a, format, out, "hipMemcpy(resolve)", [&](void* d_out) { launch_resolve(a, format, d_out, nullptr); });
  });
}

hrt_status hrt_accum_resolve_filtered(hrt_accum* a, const hrt_filter_params* f, int32_t format, void* d_out, void* stream) {
  return hguard([&] {
    if (!a || !f || !d_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_filtered: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(f);
    filtered_state(a, c, "hrt_accum_resolve_filtered");
    DeviceGuard dg(a->device);
    launch_filtered(a, c, format, d_out, (hipStream_t)stream);
  });
}

hrt_status hrt_accum_resolve_filtered_host(hrt_accum* a, const hrt_filter_params* f, int32_t format, void* out) {
  return hguard([&] {
    if (!a || !f || !out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_filtered_host: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(f);
    filtered_state(a, c, "hrt_accum_resolve_filtered_host");
    resolve_to_host(a, format, out, "hipMemcpy(filtered resolve)", [&](void* d_out) { launch_filtered(a, c, format, d_out, nullptr); });
  });
}

hrt_status hrt_accum_add_features(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, void* stream) {
  return hguard([&] {
    if (!a || !cam || !p) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_add_features: null argument"};
    accum_usable(a);
    features_flag(a, "hrt_accum_add_features");
    const FrameIdentity id = frame_identity(cam, p);
    check_identity(a, id);
    check_range(a->f_ledger.may_add(pass_range(p)));
    DeviceGuard dg(a->device);
    int cull = 0;
    bool full = false;
    const KParams kp = feature_params(a->scene, cam, p, cull, full);
    features::launch_features(cull, full, kp, a->d_feat_tiles.p, (uint32_t)a->tiles.size(), a->feat_blocks, a->feat_log_bw, a->d_fa.p,
                              a->d_fn.p, stream);
    adopt_identity(a, id);
    a->f_ledger.record(pass_range(p), 0);
  });
}

hrt_status hrt_accum_feature_samples(const hrt_accum* a, uint64_t* samples) {
  return hguard([&] {
    if (!a || !samples) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_feature_samples: null argument"};
    features_flag(a, "hrt_accum_feature_samples");
    *samples = feature_samples(a);
  });
}

hrt_status hrt_accum_features(hrt_accum* a, void* d_albedo, void* d_normal, void* stream) {
  return hguard([&] {
    if (!a || (!d_albedo && !d_normal)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_features: null argument"};
    accum_usable(a);
    features_flag(a, "hrt_accum_features");
    if (feature_samples(a) == 0) throw HipError{HRT_ERR_STATE, "hrt_accum_features: the accumulator holds no feature samples"};
    DeviceGuard dg(a->device);
    features::launch_feature_means(a->d_fa.p, a->d_fn.p, a->n_px, 1.0f / (float)feature_samples(a), d_albedo, d_normal, stream);
  });
}

hrt_status hrt_accum_features_host(hrt_accum* a, float* albedo, float* normal) {
  return hguard([&] {
    if (!a || (!albedo && !normal)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_features_host: null argument"};
    accum_usable(a);
    features_flag(a, "hrt_accum_features_host");
    if (feature_samples(a) == 0) throw HipError{HRT_ERR_STATE, "hrt_accum_features_host: the accumulator holds no feature samples"};
    DeviceGuard dg(a->device);
    const size_t bytes = a->n_px * sizeof(float4);
    DevBuf<float4> d_al(bytes), d_no(bytes);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    features::launch_feature_means(a->d_fa.p, a->d_fn.p, a->n_px, 1.0f / (float)feature_samples(a), d_al.p, d_no.p, nullptr);
    if (albedo) hip_check(hipMemcpy(albedo, d_al.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy(albedo plane)");
    if (normal) hip_check(hipMemcpy(normal, d_no.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy(normal plane)");
  });
}

hrt_status hrt_debug_accum_features(hrt_accum* a, float* fa_out, float* fn_out) {
  return hguard([&] {
    if (!a || !fa_out || !fn_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_accum_features: null argument"};
    features_flag(a, "hrt_debug_accum_features");
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(fa_out, a->d_fa.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(feature sums)");
    hip_check(hipMemcpy(fn_out, a->d_fn.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(feature sums)");
  });
}

hrt_status hrt_accum_resolve_guided(hrt_accum* a, const hrt_guided_params* g, int32_t format, void* d_out, void* stream) {
  return hguard([&] {
    if (!a || !g || !d_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_guided: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(g);
    filtered_state(a, c, "hrt_accum_resolve_guided");
    DeviceGuard dg(a->device);
    launch_filtered(a, c, format, d_out, (hipStream_t)stream);
  });
}

hrt_status hrt_accum_resolve_guided_host(hrt_accum* a, const hrt_guided_params* g, int32_t format, void* out) {
  return hguard([&] {
    if (!a || !g || !out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_guided_host: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(g);
    filtered_state(a, c, "hrt_accum_resolve_guided_host");
    resolve_to_host(a, format, out, "hipMemcpy(guided resolve)", [&](void* d_out) { launch_filtered(a, c, format, d_out, nullptr); });
  });
}

hrt_status hrt_accum_resolve_guided_ex(hrt_accum* a, const hrt_guided_ex_params* g, int32_t format, void* d_out, void* stream) {
  return hguard([&] {
    if (!a || !g || !d_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_guided_ex: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(g);
    filtered_state(a, c, "hrt_accum_resolve_guided_ex");
    DeviceGuard dg(a->device);
    launch_filtered(a, c, format, d_out, (hipStream_t)stream);
  });
}

hrt_status hrt_accum_resolve_guided_ex_host(hrt_accum* a, const hrt_guided_ex_params* g, int32_t format, void* out) {
  return hguard([&] {
    if (!a || !g || !out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_resolve_guided_ex_host: null argument"};
    accum_format(format);
    const FilterCall c = filter_call(g);
    filtered_state(a, c, "hrt_accum_resolve_guided_ex_host");
    resolve_to_host(a, format, out, "hipMemcpy(guided resolve)", [&](void* d_out) { launch_filtered(a, c, format, d_out, nullptr); });
  });
}

hrt_status hrt_accum_noise_filtered(hrt_accum* a, const hrt_guided_ex_params* g, float floor, float* d_err, void* stream_,
                                    hrt_tile_noise* tiles_out) {
  return hguard([&] {
    if (!a || !g || !tiles_out) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_noise_filtered: null argument"};
    noise_floor(floor, "hrt_accum_noise_filtered");
    FilterCall c = filter_call(g);
    c.guided = !variance_only(c.K, c.demod);
    c.err_floor = floor;
    filtered_state(a, c, "hrt_accum_noise_filtered");
    DeviceGuard dg(a->device);
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_err) {
      filter_prepare(a, stream); /* the refusal of overlapping tiles comes before anything is made */
      if (!a->d_ferr.p) a->d_ferr.alloc(a->n_px * sizeof(float), "hipMalloc(filtered noise plane)");
      d_err = a->d_ferr.p;
    }
    launch_filtered(a, c, filter::FORMAT_ERR, d_err, stream);
    filter::launch_err_reduce(d_err, a->d_ftiles.p, (uint32_t)a->tiles.size(), a->d_nout.p, stream);
    read_tile_noise(a, stream, tiles_out);
  });
}

hrt_status hrt_accum_merge(hrt_accum* dst, const hrt_accum* src, void* stream) {
  return hguard([&] {
    if (!dst || !src || dst == src) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_merge: null argument, or an accumulator into itself"};
    accum_usable(dst);
    accum_usable(src);
    merge_compatible(dst, src, "hrt_accum_merge", true);
    const bool feats = src->d_fa.p && !src->f_ledger.empty();
    if (src->ledger.empty() && !feats) return;
    check_identity(dst, src->identity);
    if (!src->ledger.empty())
      for (const SampleRange& r : *src->ledger.ranges()) check_range(dst->ledger.may_add(r));
    if (feats)
      for (const SampleRange& r : *src->f_ledger.ranges()) check_range(dst->f_ledger.may_add(r));
    DeviceGuard dg(dst->device);
    if (feats) {
      features::launch_feature_merge(dst->d_fa.p, dst->d_fn.p, src->d_fa.p, src->d_fn.p, dst->n_px, stream);
      dst->f_ledger.merge(src->f_ledger);
      adopt_identity(dst, src->identity);
    }
    if (src->ledger.empty()) return;
    hipLaunchKernelGGL(accum_merge, dim3(stream_blocks(dst->n_px)), dim3(256), 0, (hipStream_t)stream, dst->d_acc.p,
                       (const float4*)src->d_acc.p, dst->n_px);
    hip_check(hipGetLastError(), "accum_merge launch");
    if (dst->d_m2.p) {
      hipLaunchKernelGGL(accum_merge_m2, dim3(stream_blocks(dst->n_px)), dim3(256), 0, (hipStream_t)stream, dst->d_m2.p,
                         (const float*)src->d_m2.p, dst->n_px);
      hip_check(hipGetLastError(), "accum_merge_m2 launch");
    }
    dst->ledger.merge(src->ledger);
    adopt_identity(dst, src->identity);
  });
}

hrt_status hrt_accum_download(hrt_accum* a, float* sums, uint32_t* ranges, uint32_t cap, uint32_t* n_ranges) {
  return hguard([&] {
    if (!a || !n_ranges) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_download: null argument"};
    accum_usable(a);
    accum_uniform(a, HRT_ERR_UNSUPPORTED, "hrt_accum_download: the accumulator's tiles hold different passes");
    const std::vector<SampleRange>& held = *a->ledger.ranges();
    *n_ranges = (uint32_t)held.size();
    if (!sums || cap < held.size()) return;
    if (!ranges && !held.empty()) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_download: null ranges"};
    for (size_t i = 0; i < held.size(); i++) {
      ranges[2 * i] = (uint32_t)held[i].begin;
      ranges[2 * i + 1] = (uint32_t)held[i].end; /* 2^32 wraps to 0 */
    }
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(sums, a->d_acc.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(download)");
  });
}

hrt_status hrt_accum_upload(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const float* sums,
                            const uint32_t* ranges, uint32_t n_ranges) {
  return hguard([&] {
    if (!a || !cam || !p || !sums || (!ranges && n_ranges)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_upload: null argument"};
    accum_usable(a);
    if (a->d_m2.p) throw HipError{HRT_ERR_UNSUPPORTED, "hrt_accum_upload: the noise plane of a HRT_ACCUM_NOISE accumulator does not travel"};
    accum_uniform(a, HRT_ERR_UNSUPPORTED, "hrt_accum_upload: the accumulator's tiles hold different passes");
    const FrameIdentity id = frame_identity(cam, p);
    check_identity(a, id);
    /* the ranges must be addable one after the other: checked on a copy, so an error changes nothing */
    AccumLedger held = a->ledger;
    for (uint32_t i = 0; i < n_ranges; i++) {
      const SampleRange r{ranges[2 * i], ranges[2 * i + 1] == 0 ? (1ull << 32) : ranges[2 * i + 1]};
      check_range(held.may_add(r));
      held.record(r, 0);
    }
    if (n_ranges == 0) return;
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (a->ledger.empty()) { /* no samples: the sums as they are */
      hip_check(hipMemcpy(a->d_acc.p, sums, a->n_px * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy(upload)");
    } else {
      DevBuf<float4> tmp(a->n_px * sizeof(float4));
      hip_check(hipMemcpy(tmp.p, sums, a->n_px * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy(upload)");
      hipLaunchKernelGGL(accum_merge, dim3(stream_blocks(a->n_px)), dim3(256), 0, nullptr, a->d_acc.p, (const float4*)tmp.p, a->n_px);
      hip_check(hipGetLastError(), "accum_merge launch");
      hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    adopt_identity(a, id);
    a->ledger = held;
  });
}

hrt_status hrt_accum_merge_tiles(hrt_accum* dst, const hrt_accum* src, void* stream) {
  return hguard([&] {
    if (!dst || !src || dst == src) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_merge_tiles: null argument, or an accumulator into itself"};
    accum_usable(dst);
    accum_usable(src);
    merge_compatible(dst, src, "hrt_accum_merge_tiles", false);
    const bool feats = src->d_fa.p && !src->f_ledger.empty();
    if (src->ledger.empty() && !feats) return;
    check_identity(dst, src->identity);
    if (!dst->ledger.may_merge(src->ledger))
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_merge_tiles: a tile's sample ranges overlap samples the accumulator's tile holds"};
    if (feats)
      for (const SampleRange& r : *src->f_ledger.ranges()) check_range(dst->f_ledger.may_add(r));
    DeviceGuard dg(dst->device);
    /* the tiles for which src holds samples, and the launch's pixels */
    const uint32_t nt = (uint32_t)dst->tiles.size();
    std::vector<MergeTile> sel;
    uint64_t n_sel = 0;
    for (uint32_t t = 0; t < nt; t++) {
      if (src->ledger.samples(t) == 0) continue;
      const uint32_t n = dst->tiles[t].w * dst->tiles[t].h;
      sel.push_back(MergeTile{dst->tile_off[t], n, (uint32_t)n_sel, 0u});
      n_sel += n;
    }
    if (!sel.empty() && !dst->d_mtiles.p) dst->d_mtiles.alloc(nt * sizeof(MergeTile), "hipMalloc(merge tiles)");
    if (feats) {
      features::launch_feature_merge(dst->d_fa.p, dst->d_fn.p, src->d_fa.p, src->d_fn.p, dst->n_px, stream);
      dst->f_ledger.merge(src->f_ledger);
      adopt_identity(dst, src->identity);
    }
    if (sel.empty()) return;
    dst->h_mtiles.swap(sel); /* stays alive with the accumulator, as h_ntiles does */
    const uint32_t n_tiles = (uint32_t)dst->h_mtiles.size();
    hip_check(hipMemcpyAsync(dst->d_mtiles.p, dst->h_mtiles.data(), n_tiles * sizeof(MergeTile), hipMemcpyHostToDevice, (hipStream_t)stream),
              "hipMemcpyAsync(merge tiles)");
    if (dst->d_m2.p)
      hipLaunchKernelGGL((accum_merge_tiles<true>), dim3(stream_blocks(n_sel)), dim3(256), 0, (hipStream_t)stream, dst->d_acc.p,
                         (const float4*)src->d_acc.p, dst->d_m2.p, (const float*)src->d_m2.p, (const MergeTile*)dst->d_mtiles.p, n_tiles, (size_t)n_sel);
    else
      hipLaunchKernelGGL((accum_merge_tiles<false>), dim3(stream_blocks(n_sel)), dim3(256), 0, (hipStream_t)stream, dst->d_acc.p,
                         (const float4*)src->d_acc.p, (float*)nullptr, (const float*)nullptr, (const MergeTile*)dst->d_mtiles.p, n_tiles,
                         (size_t)n_sel);
    hip_check(hipGetLastError(), "accum_merge_tiles launch");
    dst->ledger.merge_tiles(src->ledger);
    adopt_identity(dst, src->identity);
  });
}

hrt_status hrt_accum_snapshot(hrt_accum* a, void* out, uint64_t cap, uint64_t* size) {
  return hguard([&] {
    if (!a || !size) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_snapshot: null argument"};
    accum_usable(a);
    const snapshot::State s = snapshot_state(a);
    *size = s.bytes;
    if (!out) return;
    if (cap < s.bytes) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_snapshot: the buffer is smaller than the snapshot"};
    uint8_t* b = static_cast<uint8_t*>(out);
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    snapshot::encode_head(s, b);
    hip_check(hipMemcpy(b + s.off_sums, a->d_acc.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(snapshot sums)");
    if (a->d_m2.p) hip_check(hipMemcpy(b + s.off_m2, a->d_m2.p, a->n_px * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(snapshot m2)");
    if (a->d_fa.p) {
      hip_check(hipMemcpy(b + s.off_fa, a->d_fa.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(snapshot fa)");
      hip_check(hipMemcpy(b + s.off_fn, a->d_fn.p, a->n_px * sizeof(float4), hipMemcpyDeviceToHost), "hipMemcpy(snapshot fn)");
    }
    snapshot::zero_pads(s, b);
    snapshot::seal(s, b);
  });
}

hrt_status hrt_accum_restore(hrt_accum* a, const void* blob, uint64_t size) {
  return hguard([&] {
    if (!a || !blob) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_restore: null argument"};
    accum_usable(a);
    if (!a->ledger.empty() || !a->f_ledger.empty())
      throw HipError{HRT_ERR_STATE, "hrt_accum_restore: the accumulator holds samples: reset it first"};
    snapshot::State s;
    snapshot_decode(blob, size, s, "hrt_accum_restore");
    if (s.flags != accum_flags(a) || s.width != a->width || s.height != a->height || s.tiles.size() != a->tiles.size())
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_restore: the snapshot's flags, image size or tile count are not the accumulator's"};
    for (size_t t = 0; t < s.tiles.size(); t++) {
      const hrt_tile& T = a->tiles[t];
      if (s.tiles[t].x != T.x || s.tiles[t].y != T.y || s.tiles[t].w != T.w || s.tiles[t].h != T.h)
        throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_restore: the snapshot's tile list is not the accumulator's"};
    }
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    DeviceGuard dg(a->device);
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize"); /* a reset's memsets, on whatever stream */
    try {
      hip_check(hipMemcpy(a->d_acc.p, b + s.off_sums, a->n_px * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy(restore sums)");
      if (a->d_m2.p) hip_check(hipMemcpy(a->d_m2.p, b + s.off_m2, a->n_px * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(restore m2)");
      if (a->d_fa.p) {
        hip_check(hipMemcpy(a->d_fa.p, b + s.off_fa, a->n_px * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy(restore fa)");
        hip_check(hipMemcpy(a->d_fn.p, b + s.off_fn, a->n_px * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy(restore fn)");
      }
      hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    } catch (...) {
      a->invalid = true; /* some planes are the snapshot's, some not: only a reset makes it usable again */
      throw;
    }
    a->ledger = AccumLedger(a->tiles.size(), std::move(s.records));
    if (a->d_fa.p) {
      std::vector<AccumLedger::Record> fr(1);
      fr[0].ranges = std::move(s.f_ranges);
      a->f_ledger = AccumLedger(a->tiles.size(), std::move(fr));
    }
    a->has_identity = s.has_identity;
    if (s.has_identity) a->identity = identity_from(s.identity, a->width, a->height);
  });
}

hrt_status hrt_accum_snapshot_info(const void* blob, uint64_t size, hrt_snapshot_info* info, hrt_tile* tiles, uint32_t cap) {
  return hguard([&] {
    if (!blob || !info) throw HipError{HRT_ERR_INVALID_ARG, "hrt_accum_snapshot_info: null argument"};
    snapshot::State s;
    snapshot_decode(blob, size, s, "hrt_accum_snapshot_info");
    memset(info, 0, sizeof(*info));
    info->version = snapshot::VERSION;
    info->flags = s.flags;
    info->width = s.width;
    info->height = s.height;
    info->n_tiles = (uint32_t)s.tiles.size();
    info->uniform = s.records.size() == 1 ? 1u : 0u;
    info->n_pixels = s.n_px;
    info->bytes = s.bytes;
    if (tiles && cap >= s.tiles.size())
      for (size_t t = 0; t < s.tiles.size(); t++) tiles[t] = hrt_tile{s.tiles[t].x, s.tiles[t].y, s.tiles[t].w, s.tiles[t].h};
  });
}

hrt_status hrt_debug_accumulate(int32_t on_device, const float* partial, uint32_t n_chunks, uint32_t n, float* acc_inout,
                                uint64_t samples, int32_t format, void* out) {
  return hguard([&] {
    if (!partial || !acc_inout || n_chunks == 0 || format < -1 || format > HRT_ACCUM_RGBA8 ||
        (format >= 0 && (!out || samples == 0 || samples > (1ull << 32))))
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_accumulate: bad argument"};
    if (n == 0) return;
    const float scale = format >= 0 ? accum::resolve_scale(samples) : 0.0f;
    const size_t out_bytes = format < 0 ? 0 : (size_t)n * (format == HRT_ACCUM_F32 ? 16u : 4u);
    if (!on_device) {
      const float4* hp = reinterpret_cast<const float4*>(partial);
      float4* ha = reinterpret_cast<float4*>(acc_inout);
      with_format<true>(format, [&](auto fc) {
        for (size_t i = 0; i < n; i++) accumulate_pixel<decltype(fc)::value>(hp, ha, n, n_chunks, scale, out, i);
      });
      return;
    }
    /* the real kernels on the calling thread's current device: the fused accumulate + resolve, and the separate
     * resolve of the same sums, which must agree */
    const size_t p_bytes = (size_t)n_chunks * n * sizeof(float4), a_bytes = (size_t)n * sizeof(float4);
    DevBuf<float4> d_partial(p_bytes, partial), d_acc(a_bytes, acc_inout);
    DevBuf<uint8_t> d_out(out_bytes + 16), d_out2(out_bytes + 16);
    launch_accumulate(format, d_partial.p, d_acc.p, n, n_chunks, scale, d_out.p, nullptr);
    hip_check(hipMemcpy(acc_inout, d_acc.p, a_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    if (format < 0) return;
    resolve_pixels(format, d_acc.p, n, scale, d_out2.p, nullptr);
    std::vector<uint8_t> second(out_bytes);
    hip_check(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(second.data(), d_out2.p, out_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    if (memcmp(out, second.data(), out_bytes) != 0)
      throw HipError{HRT_ERR_STATE, "hrt_debug_accumulate: accumulate_chunks' fused resolve and accum_resolve differ"};
  });
}

hrt_status hrt_debug_noise(int32_t on_device, const float* partial, const uint32_t* sizes, uint32_t n_chunks, uint32_t n,
                           float* acc_inout, float* m2_inout, uint64_t samples, uint64_t chunks, float floor, float* err_out,
                           float* mean_max_out) {
  return hguard([&] {
    if (!partial || !sizes || !acc_inout || !m2_inout || !err_out || !mean_max_out || n_chunks == 0 || n == 0 || samples == 0 ||
        samples > (1ull << 32))
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_noise: bad argument"};
    for (uint32_t c = 0; c < n_chunks; c++)
      if (sizes[c] == 0) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_noise: an empty chunk"};
    noise_floor(floor, "hrt_debug_noise");
    const NoiseTile T = noise_tile(0, n, samples, chunks);
    const G::TileDev map{0, 0, n, 1, (n + 7) / 8, 0, 0, 0}; /* one tile: the launch's pixels onto themselves */
    if (!on_device) {
      const float4* hp = reinterpret_cast<const float4*>(partial);
      float4* ha = reinterpret_cast<float4*>(acc_inout);
      const MomentArgs<true> M{m2_inout, &map, 1u, ChunkCounts{sizes, 0, 0, 0}};
      for (size_t i = 0; i < n; i++) accumulate_pixel_mapped<-1>(hp, ha, n, n_chunks, 0.0f, nullptr, i, M);
      for (size_t i = 0; i < n; i++)
        err_out[i] = accum::noise_err(v3(ha[i].x, ha[i].y, ha[i].z), m2_inout[i], T.inv_n, T.inv_k1, T.few != 0u, floor);
      accum::tile_reduce(err_out, n, mean_max_out[0], mean_max_out[1]);
      return;
    }
    /* the real kernels on the calling thread's current device */
    const size_t p_bytes = (size_t)n_chunks * n * sizeof(float4), a_bytes = (size_t)n * sizeof(float4), m_bytes = (size_t)n * sizeof(float);
    DevBuf<float4> d_partial(p_bytes, partial), d_acc(a_bytes, acc_inout);
    DevBuf<float> d_m2(m_bytes, m2_inout), d_err(m_bytes);
    DevBuf<uint32_t> d_sizes(n_chunks * sizeof(uint32_t), sizes);
    DevBuf<G::TileDev> d_map(sizeof(G::TileDev), &map);
    DevBuf<NoiseTile> d_tile(sizeof(NoiseTile), &T);
    DevBuf<float2> d_rec(sizeof(float2));
    const MomentArgs<true> M{d_m2.p, d_map.p, 1u, ChunkCounts{d_sizes.p, 0, 0, 0}};
    accumulate(-1, d_partial.p, d_acc.p, n, n_chunks, 0.0f, nullptr, M, nullptr);
    hipLaunchKernelGGL(accum_noise, dim3(1), dim3(accum::NOISE_BLOCK), 0, nullptr, (const float4*)d_acc.p, (const float*)d_m2.p,
                       (const NoiseTile*)d_tile.p, floor, d_err.p, d_rec.p);
    hip_check(hipGetLastError(), "accum_noise launch");
    hip_check(hipMemcpy(acc_inout, d_acc.p, a_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(m2_inout, d_m2.p, m_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(err_out, d_err.p, m_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(mean_max_out, d_rec.p, sizeof(float2), hipMemcpyDeviceToHost), "hipMemcpy");
  });
}

hrt_status hrt_debug_accum_paths(int32_t on_device, const hrt_path* paths, uint32_t n_px, uint32_t samples, const uint32_t* sched3,
                                 float* acc_inout, float* m2_inout, uint64_t total_samples, int32_t format, void* out,
                                 uint32_t* live_out) {
  return hguard([&] {
    if (!paths || !sched3 || !acc_inout || samples == 0 || (uint64_t)n_px * samples >= (1ull << 32) || format < -1 ||
        format > HRT_ACCUM_RGBA8 || (format >= 0 && (!out || total_samples == 0 || total_samples > (1ull << 32))))
      throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_accum_paths: bad argument"};
    /* the schedule must cut [0, samples) into chunks that are not empty: K is where they end */
    const accum::PathSchedule schedule{sched3[0], sched3[1], sched3[2]};
    uint32_t n_chunks = 0;
    for (uint32_t end = 0; end != samples; n_chunks++) {
      uint32_t s0 = 0, s1 = 0;
      if (schedule.chunk_head != 0) schedule.range(n_chunks, s0, s1);
      if (s0 != end || s1 <= s0 || s1 > samples) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_accum_paths: not a schedule of `samples` samples"};
      end = s1;
    }
    if (live_out) *live_out = 0;
    if (n_px == 0) return;
    const G::TileDev map{0, 0, n_px, 1, (n_px + 7) / 8, 0, 0, 0}; /* one tile: the launch's pixels onto themselves */
    PathArgs A;
    memset(&A, 0, sizeof(A));
    A.scale = format >= 0 ? accum::resolve_scale(total_samples) : 0.0f;
    A.n_tiles = 1;
    A.n_px = n_px, A.samples = samples, A.n_chunks = n_chunks;
    A.schedule = schedule;
    const size_t n = (size_t)n_px * samples;
    const size_t out_bytes = format < 0 ? 0 : (size_t)n_px * (format == HRT_ACCUM_F32 ? 16u : 4u);
    if (!on_device) {
      A.paths = reinterpret_cast<const float4*>(paths);
      A.acc = reinterpret_cast<float4*>(acc_inout), A.m2 = m2_inout, A.out = out, A.tiles = &map;
      with_format<true>(format, [&](auto fc) {
        for (size_t i = 0; i < n_px; i++) add_paths_pixel_global<decltype(fc)::value>(A, i);
      });
      for (size_t j = 0; live_out && j < n; j++) *live_out += path_not_done(A.paths[3 * j + 2]);
      return;
    }
    /* the real kernel on the calling thread's current device, and the separate resolve of the same sums, which must
     * agree with the fused one */
    const size_t a_bytes = (size_t)n_px * sizeof(float4), m_bytes = (size_t)n_px * sizeof(float);
    const uint32_t zero = 0;
    DevBuf<float4> d_paths(n * sizeof(hrt_path), paths), d_acc(a_bytes, acc_inout);
    DevBuf<float> d_m2(m_bytes, m2_inout);
    DevBuf<uint8_t> d_out(out_bytes + 16), d_out2(out_bytes + 16);
    DevBuf<G::TileDev> d_map(sizeof(G::TileDev), &map);
    DevBuf<uint32_t> d_live(sizeof(uint32_t), &zero);
    A.paths = d_paths.p;
    A.acc = d_acc.p, A.m2 = m2_inout ? d_m2.p : nullptr, A.out = d_out.p, A.tiles = d_map.p;
    A.live = live_out ? d_live.p : nullptr;
    launch_accumulate_paths(format, A, nullptr);
    hip_check(hipMemcpy(acc_inout, d_acc.p, a_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    if (m2_inout) hip_check(hipMemcpy(m2_inout, d_m2.p, m_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    if (live_out) hip_check(hipMemcpy(live_out, d_live.p, sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
    if (format < 0) return;
    resolve_pixels(format, d_acc.p, n_px, A.scale, d_out2.p, nullptr);
    std::vector<uint8_t> second(out_bytes);
    hip_check(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(second.data(), d_out2.p, out_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    if (memcmp(out, second.data(), out_bytes) != 0)
      throw HipError{HRT_ERR_STATE, "hrt_debug_accum_paths: accumulate_paths' fused resolve and accum_resolve differ"};
  });
}

/* the checks the four hrt_debug_* raster entry points share: the arguments and the raster's size, and the terms */
static void debug_raster_args(const char* who, bool arguments, uint32_t width, uint32_t height) {
  if (!arguments || width == 0 || height == 0 || width > 65535 || height > 65535)
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null argument or no tiles, or a width or height outside [1, 65535]"};
}
static filter::Terms debug_terms(const char* who, float kn, float ka, float kz) {
  if (!(kn >= 0.0f) || !(ka >= 0.0f) || !(kz >= 0.0f)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": a negative or NaN term"};
  return filter::Terms{kn, ka, kz};
}

/* hrt_debug_filter, hrt_debug_guided and hrt_debug_guided_ex after their checks; albedo and normal null: the plain
 * filter */
static void debug_atrous(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                         uint32_t height, uint32_t iterations, float sigma, const filter::Terms& K, const filter::Demod& demod,
                         float* out) {
  if (!on_device) return filter::filter_raster(raster, albedo, normal, width, height, iterations, sigma, K, demod, out);
  /* the real kernels on the calling thread's current device: one tile that covers the raster, so the packed
   * order of the last iteration's output is the raster's */
  const size_t bytes = (size_t)width * height * sizeof(float4);
  const filter::FilterTile T{0, 0, width, height, 0, 0, 0.0f, 0.0f};
  DevBuf<float4> d_a(bytes, raster), d_b(bytes), d_al(albedo ? bytes : 0, albedo), d_no(normal ? bytes : 0, normal), d_out(bytes);
  DevBuf<filter::FilterTile> d_tile(sizeof(filter::FilterTile), &T);
  if (demod.on) filter::launch_demodulate(d_a.p, d_al.p, (size_t)width * height, demod.floor, nullptr);
  filter::launch_atrous(d_a.p, d_b.p, albedo ? d_al.p : nullptr, normal ? d_no.p : nullptr, width, height, d_tile.p, 1,
                        filter::tile_blocks(width, height), iterations, sigma, K, demod, filter::FORMAT_RAW, d_out.p, nullptr);
  hip_check(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
}

hrt_status hrt_debug_filter(int32_t on_device, const float* raster, uint32_t width, uint32_t height, uint32_t iterations,
                            float sigma, float* out) {
  return hguard([&] {
    debug_raster_args("hrt_debug_filter", raster && out, width, height);
    filter_args(iterations, sigma);
    debug_atrous(on_device, raster, nullptr, nullptr, width, height, iterations, sigma, filter::Terms{}, NO_DEMOD, out);
  });
}

hrt_status hrt_debug_guided(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                            uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, float* out) {
  return hguard([&] {
    debug_raster_args("hrt_debug_guided", raster && albedo && normal && out, width, height);
    filter_args(iterations, sigma);
    const filter::Terms K = debug_terms("hrt_debug_guided", kn, ka, kz);
    debug_atrous(on_device, raster, albedo, normal, width, height, iterations, sigma, K, NO_DEMOD, out);
  });
}

hrt_status hrt_debug_guided_ex(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                               uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, uint32_t flags,
                               float albedo_floor, float* out) {
  return hguard([&] {
    debug_raster_args("hrt_debug_guided_ex", raster && albedo && normal && out, width, height);
    filter_args(iterations, sigma);
    const filter::Terms K = debug_terms("hrt_debug_guided_ex", kn, ka, kz);
    const filter::Demod demod = guided_ex_option(flags, albedo_floor);
    debug_atrous(on_device, raster, albedo, normal, width, height, iterations, sigma, K, demod, out);
  });
}

hrt_status hrt_debug_noise_filtered(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                                    uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, uint32_t flags,
                                    float albedo_floor, float floor, const hrt_tile* tiles, uint32_t n_tiles, float* err_out,
                                    float* mean_max_out) {
  return hguard([&] {
    debug_raster_args("hrt_debug_noise_filtered", raster && tiles && n_tiles != 0 && err_out && mean_max_out, width, height);
    filter_args(iterations, sigma);
    const filter::Terms K = debug_terms("hrt_debug_noise_filtered", kn, ka, kz);
    const filter::Demod demod = guided_ex_option(flags, albedo_floor);
    noise_floor(floor, "hrt_debug_noise_filtered");
    const bool plain = variance_only(K, demod);
    if (!plain && (!albedo || !normal)) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_noise_filtered: a term or the flag needs the feature rasters"};
    /* the tiles lie inside the raster, overlap nowhere and cover present pixels only */
    const size_t area = (size_t)width * height;
    const TileCover cover = tile_cover(tiles, n_tiles, 0, 0, width, height, [&](size_t k) { return raster[4 * k + 3] < 0.0f; });
    if (cover == TileCover::OUTSIDE) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_noise_filtered: a tile is empty or leaves the raster"};
    if (cover == TileCover::OVERLAP) throw HipError{HRT_ERR_INVALID_ARG, "hrt_debug_noise_filtered: tiles overlap or cover an absent pixel"};
    std::vector<filter::FilterTile> ft(n_tiles);
    size_t off = 0, blocks = 0;
    for (uint32_t t = 0; t < n_tiles; t++) {
      const hrt_tile& T = tiles[t];
      ft[t] = filter::FilterTile{T.x, T.y, T.w, T.h, (uint32_t)off, (uint32_t)blocks, 0.0f, 0.0f};
      off += (size_t)T.w * T.h;
      blocks += filter::tile_blocks(T.w, T.h);
    }
    const float* al = plain ? nullptr : albedo;
    const float* no = plain ? nullptr : normal;
    if (!on_device) {
      std::vector<float> out(4 * area), err(area);
      filter::filter_raster(raster, al, no, width, height, iterations, sigma, K, demod, out.data(), err.data(), floor);
      for (uint32_t t = 0; t < n_tiles; t++) {
        const filter::FilterTile& T = ft[t];
        for (uint32_t y = 0; y < T.h; y++)
          for (uint32_t x = 0; x < T.w; x++) err_out[(size_t)T.off + (size_t)y * T.w + x] = err[(size_t)(T.y + y) * width + (T.x + x)];
        accum::tile_reduce(err_out + T.off, T.w * T.h, mean_max_out[2 * t], mean_max_out[2 * t + 1]);
      }
      return;
    }
    /* the real kernels on the calling thread's current device */
    const size_t bytes = area * sizeof(float4);
    DevBuf<float4> d_a(bytes, raster), d_b(bytes), d_al(al ? bytes : 0, al), d_no(no ? bytes : 0, no);
    DevBuf<float> d_err(off * sizeof(float));
    DevBuf<float2> d_rec(n_tiles * sizeof(float2));
    DevBuf<filter::FilterTile> d_tiles(n_tiles * sizeof(filter::FilterTile), ft.data());
    if (demod.on) filter::launch_demodulate(d_a.p, d_al.p, area, demod.floor, nullptr);
    filter::launch_atrous(d_a.p, d_b.p, al ? d_al.p : nullptr, no ? d_no.p : nullptr, width, height, d_tiles.p, n_tiles, (uint32_t)blocks,
                          iterations, sigma, K, demod, filter::FORMAT_ERR, d_err.p, nullptr, floor);
    filter::launch_err_reduce(d_err.p, d_tiles.p, n_tiles, d_rec.p, nullptr);
    hip_check(hipMemcpy(err_out, d_err.p, off * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(mean_max_out, d_rec.p, n_tiles * sizeof(float2), hipMemcpyDeviceToHost), "hipMemcpy");
  });
}

}  // extern "C"
