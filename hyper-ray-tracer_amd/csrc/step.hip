/*
 * step.hip — path stepping: the kernel and entry points of hrt_scene_step (per-lane code: step.h; the contract:
 * include/hrt/hrt.h).
 *
 *   step_kernel   query_kernel's shape (query.hip): one lane per item of the DOMAIN - the batch, or a list of path
 *                 indices whose length is in device memory - on a persistent grid whose waves take blocks of 64
 *                 consecutive items, `claim` blocks per claim.  The item count is not known to the host, which sizes
 *                 the grid from the list's capacity; so a wave's FIRST claim is fixed by its place in the grid (wave w
 *                 of workgroup g takes claim g * waves + w) and only the later ones go through the call's counter.  A
 *                 workgroup whose first claim already lies beyond the count leaves before it stages anything: a late
 *                 round with a few hundred live paths copies the scene once, not once per resident workgroup.
 *                 LDS: the scene as query_kernel stages it, and behind it, at a PERLIN_LDS_ALIGN offset the host
 *                 computes, the Perlin tables when both fit LDS_SCENE_MAX_BYTES (stage_perlin).
 *                 A lane reads its index, then its path's last 16 bytes and leaves if the path is DONE; otherwise it
 *                 reads the path and the ray, runs step_path (up to `steps` rounds of query_ray and scatter_step in
 *                 registers) and stores the ray and the path as 16-B accesses, and the last hit only when the caller
 *                 wants it.  The out list takes one ballot of the lanes still live per block and one atomicAdd of the
 *                 popcounts per wave and claim (OUT_GROUP), and each lane writes at base + its rank.  A wave sums its valid rays in a register
 *                 and adds them with one 64-bit atomic as it leaves.
 *                 No workgroup waits on another: no spin, no look-back, no grid barrier.  Every loop is bounded by the
 *                 item count, by `steps` or by the walk's forward skip links (lane.h trace_ray), so every launch ends.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernel_common.h"
#include "query_host.h"
#include "step.h"

using namespace hrt;
using namespace hrt::stepq;

namespace {

constexpr uint32_t PERLIN_GLOBAL = 0xFFFFFFFFu; /* StepArgs::perlin_at: the tables stay in global memory */

struct StepArgs {
  hrt_ray* rays;
  hrt_path* paths;
  hrt_hit* hits;              /* null: the hits are not kept */
  const uint32_t* in_index;   /* null: the domain is [0, n) */
  const uint32_t* in_count;
  uint32_t* out_index;        /* null: no out list */
  uint32_t* out_count;
  unsigned long long* n_rays; /* null: not counted */
  uint32_t* counter;          /* the call's claim counter, zeroed in stream order */
  uint32_t n, in_capacity, claim, steps;
  uint32_t perlin_at; /* where the Perlin tables go in the dynamic LDS, in float4s (a multiple of PERLIN_LDS_ALIGN bytes:
                         the kernel declares no static __shared__, so offset and address agree), or PERLIN_GLOBAL */
};

/* Blocks per append to the out list.  One atomicAdd a block put 129 600 atomics of a full 8.3 M-path round on ONE address:
 * on earth_perlin the step with an out list took 1.36 ms where the step without took 0.65 and the pair 0.95
 * (measured before this constant existed).  So a wave appends once per claim, and a claim is at most
 * this many blocks: a group's ballots live in one register, two lanes each. */
constexpr uint32_t OUT_GROUP = 32;
static_assert(OUT_GROUP <= 32, "a block's ballot takes two lanes of the wave's mask register");

template <bool LDS>
constexpr int step_threads() { return LDS ? 768 : 256; }

template <int CULL, bool FULL, bool MEDIA, bool LDS>
__global__ __launch_bounds__(step_threads<LDS>()) void step_kernel(KParams P, StepArgs A) {
  extern __shared__ float4 lds[];
  constexpr uint32_t WAVES = (uint32_t)step_threads<LDS>() / 64u;
  const uint32_t count = A.in_index ? min(*A.in_count, A.in_capacity) : A.n;
  const uint32_t n_blocks = (count + (QUERY_BLOCK - 1u)) / QUERY_BLOCK; /* count < 2^32: no wrap after the division */
  /* the workgroup's first claim (its wave 0's) is past the domain, so are its other waves' and all it would claim later */
  if ((uint64_t)blockIdx.x * WAVES * A.claim >= n_blocks) return;
  const G::Node* nodes = P.nodes;
  const G::Prim* prims = P.prims;
  if (A.perlin_at != PERLIN_GLOBAL) {
    P.perlin = kern::stage_perlin(lds + A.perlin_at, P.perlin, P.n_perlin);
    P.perlin_lds = 1u;
  }
  if constexpr (LDS) kern::stage_scene(P, lds, nodes, prims); /* ends in the barrier that also covers the tables */
  else if (A.perlin_at != PERLIN_GLOBAL) __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t dynamic0 = gridDim.x * WAVES * A.claim; /* the blocks the fixed first claims cover */
  uint32_t b0 = (blockIdx.x * WAVES + (threadIdx.x >> 6)) * A.claim;
  b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
  uint32_t my_rays = 0;
  while (b0 < n_blocks) { /* n_blocks <= 2^26 and each wave overshoots once, by claim <= 32: the counter cannot wrap */
    const uint32_t b1 = min(b0 + A.claim, n_blocks);
    { /* one claim: its blocks, then one append to the out list for all of them (the host keeps claim <= OUT_GROUP) */
      const uint32_t g0 = b0, g1 = b1;
      /* the ballot of block g0 + j (which of its lanes' items are still live): its low half in lane j, its high half in lane
       * j + 32 of ONE register, written by per-lane selects and read back by v_readlane (OUT_GROUP <= 32) */
      uint32_t masks = 0, total = 0;
      for (uint32_t b = g0; b < g1; b++) {
        const uint64_t k = (uint64_t)b * QUERY_BLOCK + lane;
        bool live = false; /* not DONE on entry and not DONE now */
        if (k < count) {
          const uint32_t i = A.in_index ? A.in_index[k] : (uint32_t)k;
          if (i < A.n) { /* an entry past the batch is skipped, never dereferenced */
            const float4 tail = scatterq::load_path_tail(A.paths + i);
            if (!scatterq::tail_done(tail)) {
              hrt_path path = scatterq::load_path(A.paths + i, tail);
              hrt_ray ray = query::load_ray(A.rays + i);
              const Stepped r = step_path<CULL, FULL, MEDIA>(P, nodes, prims, ray, path, A.steps);
              query::store_ray(A.rays + i, ray);
              scatterq::store_path(A.paths + i, path);
              if (A.hits) query::store_hit(A.hits + i, r.hit);
              my_rays += r.n_rays;
              live = (path.flags & (uint32_t)HRT_PATH_DONE) == 0u;
            }
          }
        }
        if (A.out_index) { /* wave-uniform; every lane of the wave is here */
          const unsigned long long mask = __ballot(live);
          const uint32_t j = b - g0;
          total += (uint32_t)__popcll(mask);
          masks = lane == j ? (uint32_t)mask : (lane == j + 32u ? (uint32_t)(mask >> 32) : masks);
        }
      }
      if (total) { /* wave-uniform, 0 without an out list: one atomicAdd for the group, then block by block at base + rank */
        uint32_t at = 0;
        if (lane == 0u) at = atomicAdd(A.out_count, total);
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
        for (uint32_t b = g0; b < g1; b++) {
          const uint32_t j = b - g0;
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)masks, (int)j);
          const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)masks, (int)(j + 32u));
          if (((lane < 32u ? lo : hi) >> (lane & 31u)) & 1u) { /* the index again: 4 bytes a live path, against a register held across the walk */
            const uint64_t k = (uint64_t)b * QUERY_BLOCK + lane;
            /* at + rank < the live paths of the domain <= its capacity <= out's (the host checks) */
            A.out_index[at + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u))] = A.in_index ? A.in_index[k] : (uint32_t)k;
          }
          at += (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
        }
      }
    }
    uint32_t next = 0;
    if (lane == 0u) next = atomicAdd(A.counter, A.claim);
    b0 = dynamic0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)next); /* every lane is active here: lane 0's claim */
  }
  if (A.n_rays) {
    for (int o = 32; o > 0; o >>= 1) my_rays += (uint32_t)__shfl_xor((int)my_rays, o);
    if (lane == 0u && my_rays != 0u) atomicAdd(A.n_rays, (unsigned long long)my_rays);
  }
}

template <int CULL, bool FULL, bool MEDIA, bool LDS>
void step_kernel_launch(const KParams& P, int device, size_t smem, StepArgs A, uint32_t domain_cap, hipStream_t stream) {
  const void* fn = (const void*)step_kernel<CULL, FULL, MEDIA, LDS>;
  const int block = step_threads<LDS>();
  const uint32_t n_blocks = (domain_cap + (QUERY_BLOCK - 1u)) / QUERY_BLOCK;
  const int resident = resident_grid(fn, block, device, smem, smem != 0, __PRETTY_FUNCTION__);
  /* no more workgroups than the largest domain has claims for their waves */
  A.claim = std::min(claim_blocks(n_blocks), OUT_GROUP); /* HRT_QUERY_CLAIM may ask for up to 64 */
  const uint32_t n_claims = (n_blocks + A.claim - 1u) / A.claim, waves = (uint32_t)(block / 64);
  const uint32_t grid = std::min<uint32_t>((uint32_t)resident, (n_claims + waves - 1u) / waves);
  hipLaunchKernelGGL((step_kernel<CULL, FULL, MEDIA, LDS>), dim3(grid), dim3(block), smem, stream, P, A);
  hip_check(hipGetLastError(), "step_kernel launch");
}

template <int CULL, bool LDS>
void launch_cull(bool full, bool media, const KParams& P, int device, size_t smem, const StepArgs& A, uint32_t domain_cap,
                 hipStream_t stream) {
  if (full && media) step_kernel_launch<CULL, true, true, LDS>(P, device, smem, A, domain_cap, stream);
  else if (full) step_kernel_launch<CULL, true, false, LDS>(P, device, smem, A, domain_cap, stream);
  else step_kernel_launch<CULL, false, false, LDS>(P, device, smem, A, domain_cap, stream);
}

/* the instantiation a step runs: launch_query's choice (query.hip) of culling, FULL, media and the scene in LDS, and the
 * Perlin tables behind the scene (or at 0 without it) when both fit the budget */
void launch(const hrt_scene* s, const hrt_step_params* sp, KParams P, StepArgs A, uint32_t domain_cap, hipStream_t stream) {
  const hrt_query_params q = step_query_params(sp);
  const int cull = query::query_cull(&q, s->cull_mode, s->box_t0, s->box_t1);
  const bool full = (s->feature_mask & ~G::F_BASIC) != 0 || s->w_general;
  const bool media = full && (s->feature_mask & G::F_MEDIUM) != 0 && !(sp->flags & HRT_STEP_SKIP_MEDIA);
  const size_t scene_bytes = s->g_nodes.size() * sizeof(G::Node) + s->g_prims.size() * sizeof(G::Prim);
  const bool no_lds = (sp->flags & HRT_STEP_NO_LDS) != 0;
  const bool lds = !no_lds && scene_bytes <= G::LDS_SCENE_MAX_BYTES;
  size_t smem = lds ? scene_bytes : 0;
  const char* staged = knob_env("HRT_SCATTER_PERLIN_LDS"); /* A/B: "0" leaves the Perlin tables in global memory (the same records) */
  const size_t at = (smem + G::PERLIN_LDS_ALIGN - 1) / G::PERLIN_LDS_ALIGN * G::PERLIN_LDS_ALIGN; /* stage_perlin */
  const size_t tables = P.n_perlin * sizeof(G::Perlin);
  A.perlin_at = PERLIN_GLOBAL;
  if (!no_lds && !(staged && strcmp(staged, "0") == 0) && tables > 0 && at + tables <= G::LDS_SCENE_MAX_BYTES) {
    A.perlin_at = (uint32_t)(at / 16u);
    smem = at + tables;
  }
  if (cull == G::CULL_EXACT) {
    if (lds) launch_cull<G::CULL_EXACT, true>(full, media, P, s->device, smem, A, domain_cap, stream);
    else launch_cull<G::CULL_EXACT, false>(full, media, P, s->device, smem, A, domain_cap, stream);
  } else {
    if (lds) launch_cull<G::CULL_REFERENCE, true>(full, media, P, s->device, smem, A, domain_cap, stream);
    else launch_cull<G::CULL_REFERENCE, false>(full, media, P, s->device, smem, A, domain_cap, stream);
  }
  launch_knobs(s);
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0; }
bool list_ok(const hrt_path_list* l) {
  return l->d_index && l->d_count && aligned_to(l->d_index, 4) && aligned_to(l->d_count, 4) && l->reserved == 0;
}

/* the argument checks of both entry points, before any device call */
void check_step_args(const hrt_scene* s, const hrt_step_params* sp, const void* rays, const void* paths, uint64_t n, const void* hits,
                     const hrt_path_list* in, const hrt_path_list* out, const void* n_rays, bool on_device, const char* who) {
  if (!s || !sp) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null argument"};
  if (!step_params_ok(sp))
    throw HipError{HRT_ERR_INVALID_ARG,
                   std::string(who) + ": bad step params (known flags, steps >= 1, reserved 0, finite time0 <= time1, a finite background)"};
  if (n >= (1ull << 32)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": n must be below 2^32"};
  if (n != 0 && (!rays || !paths)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": null buffer"};
  if (n != 0 && on_device && (!aligned16(rays) || !aligned16(paths) || !aligned16(hits)))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the records must be 16-byte aligned"};
  if (on_device && !aligned_to(n_rays, 8)) throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the ray count must be 8-byte aligned"};
  if ((in && !list_ok(in)) || (out && !list_ok(out)))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": bad path list (device pointers, 4-byte aligned, reserved 0)"};
  if (out && (uint64_t)out->capacity < (in ? (uint64_t)in->capacity : n))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the out list is smaller than the domain"};
  if (in && out && (in->d_index == out->d_index || in->d_count == out->d_count || (const void*)in->d_index == (const void*)out->d_count ||
                    (const void*)in->d_count == (const void*)out->d_index))
    throw HipError{HRT_ERR_INVALID_ARG, std::string(who) + ": the out list shares a pointer with the in list"};
  if (!s->committed || !s->d_blob) throw HipError{HRT_ERR_STATE, "scene not committed"};
}

}  // namespace

extern "C" {

hrt_status hrt_scene_step(hrt_scene* s, const hrt_step_params* sp, hrt_ray* d_rays, hrt_path* d_paths, uint64_t n, hrt_hit* d_hits,
                          const hrt_path_list* in, const hrt_path_list* out, uint64_t* d_n_rays, void* stream_) {
  return hguard([&] {
    check_step_args(s, sp, d_rays, d_paths, n, d_hits, in, out, d_n_rays, true, "hrt_scene_step");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard dg(s->device);
    if (out) hip_check(hipMemsetAsync(out->d_count, 0, sizeof(uint32_t), stream), "hipMemsetAsync(out count)");
    const uint32_t domain_cap = in ? in->capacity : (uint32_t)n;
    if (n == 0 || domain_cap == 0) return;
    const hrt_query_params q = step_query_params(sp);
    const hrt_scatter_params sc = step_scatter_params(sp);
    KParams kp = scene_query_params(s, &q); /* query_ray's fields, then scatter_step's on top: the two sets are disjoint */
    const KParams ks = scene_scatter_params(s, &sc);
    kp.n_mats = ks.n_mats, kp.n_texs = ks.n_texs, kp.n_perlin = ks.n_perlin, kp.perlin_lds = ks.perlin_lds;
    kp.background = ks.background;
    StepArgs A;
    memset(&A, 0, sizeof(A));
    A.rays = d_rays, A.paths = d_paths, A.hits = d_hits;
    A.in_index = in ? in->d_index : nullptr, A.in_count = in ? in->d_count : nullptr, A.in_capacity = in ? in->capacity : 0u;
    A.out_index = out ? out->d_index : nullptr, A.out_count = out ? out->d_count : nullptr;
    A.n_rays = (unsigned long long*)d_n_rays;
    A.n = (uint32_t)n, A.steps = sp->steps;
    /* the call's own claim counter, allocated, zeroed and freed in stream order: calls on any streams are independent */
    hip_check(hipMallocAsync((void**)&A.counter, sizeof(uint32_t), stream), "hipMallocAsync(step counter)");
    try {
      hip_check(hipMemsetAsync(A.counter, 0, sizeof(uint32_t), stream), "hipMemsetAsync(step counter)");
      launch(s, sp, kp, A, domain_cap, stream);
    } catch (...) {
      (void)hipFreeAsync(A.counter, stream);
      throw;
    }
    hip_check(hipFreeAsync(A.counter, stream), "hipFreeAsync(step counter)");
  });
}

hrt_status hrt_scene_step_host(hrt_scene* s, const hrt_step_params* sp, hrt_ray* rays, hrt_path* paths, uint64_t n, hrt_hit* hits,
                               uint64_t* n_rays) {
  hrt_status st = hguard([&] { check_step_args(s, sp, rays, paths, n, hits, nullptr, nullptr, n_rays, false, "hrt_scene_step_host"); });
  if (st != HRT_OK || n == 0) return st;
  return hguard([&] {
    DeviceGuard dg(s->device);
    DevBuf<hrt_ray> d_rays((size_t)n * sizeof(hrt_ray), rays);
    DevBuf<hrt_path> d_paths((size_t)n * sizeof(hrt_path), paths);
    DevBuf<hrt_hit> d_hits;
    if (hits) d_hits = DevBuf<hrt_hit>((size_t)n * sizeof(hrt_hit), hits); /* a path DONE on entry keeps the caller's hit */
    const uint64_t zero = 0;
    DevBuf<uint64_t> d_count;
    if (n_rays) d_count = DevBuf<uint64_t>(sizeof(uint64_t), &zero);
    const hrt_status r = hrt_scene_step(s, sp, d_rays.p, d_paths.p, n, d_hits.p, nullptr, nullptr, d_count.p, nullptr);
    if (r != HRT_OK) throw HipError{r, hrt_last_error()};
    hip_check(hipMemcpy(rays, d_rays.p, (size_t)n * sizeof(hrt_ray), hipMemcpyDeviceToHost), "hipMemcpy(rays)");
    hip_check(hipMemcpy(paths, d_paths.p, (size_t)n * sizeof(hrt_path), hipMemcpyDeviceToHost), "hipMemcpy(paths)");
    if (hits) hip_check(hipMemcpy(hits, d_hits.p, (size_t)n * sizeof(hrt_hit), hipMemcpyDeviceToHost), "hipMemcpy(hits)");
    if (n_rays) {
      uint64_t walked = 0;
      hip_check(hipMemcpy(&walked, d_count.p, sizeof(walked), hipMemcpyDeviceToHost), "hipMemcpy(ray count)");
      *n_rays += walked;
    }
  });
}

}  // extern "C"
