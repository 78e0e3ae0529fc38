/* query_host.h — the host helpers the query translation units share (query.hip: hrt_scene_intersect and the camera
 * calls; scatter.hip: hrt_scene_scatter; step.hip: hrt_scene_step): the kernel parameters a committed scene gives each
 * per-lane function, the claim size of the persistent query grids, the alignment check of the record buffers. */
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "render_host.h"
#include "scatter.h"

namespace hrt {

constexpr uint32_t QUERY_BLOCK = 64; /* rays per block: one wave's worth */
/* Blocks per atomicAdd.  One address takes an atomic every ~12 ns whatever the grid, so a call's claims must stay few
 * next to its time: at one block per claim the 129 600 atomics of 8.3 M rays took 1.57 ms by themselves.  A claim must
 * also stay short next to the call, because the launch ends on its last claims and a wave should make several.  Measured
 * on those 8.3 M rays, coherent / incoherent, at 1 / 2 / 3 / 4 / 6 / 8 / 16 / 32 blocks per claim: 1.60 / 1.14 / 1.08 /
 * 1.09 / 1.13 / 1.19 / 1.37 / 2.06 ms and 1.63 / 1.40 / 1.38 / 1.39 / 1.44 / 1.51 / 1.64 / 2.16 ms
 * (profiles/query.jsonl query_claim).  So batches below QUERY_CLAIM_FROM blocks (1 M rays: 0.2 ms of atomics at most)
 * claim block by block, larger ones as many blocks as keep the claims near that number, at most QUERY_CLAIM_MAX. */
constexpr uint32_t QUERY_CLAIM_FROM = 16384, QUERY_CLAIM_MAX = 4;
/* HRT_QUERY_CLAIM = 1 .. 64: that many blocks per claim whatever the batch (an A/B knob: hits do not depend on it) */
inline uint32_t claim_blocks(uint32_t n_blocks) {
  const char* v = knob_env("HRT_QUERY_CLAIM");
  const long k = v ? strtol(v, nullptr, 10) : 0;
  if (k >= 1 && k <= 64) return (uint32_t)k;
  return std::min(std::max(n_blocks / QUERY_CLAIM_FROM, 1u), QUERY_CLAIM_MAX);
}

/* what query_ray reads of the committed scene (query.h) */
inline lane::KParams scene_query_params(const hrt_scene* s, const hrt_query_params* q) {
  lane::KParams kp;
  memset(&kp, 0, sizeof(kp));
  const uint8_t* base = (const uint8_t*)s->d_blob;
  kp.nodes = (const gpu::Node*)(base + s->off_nodes);
  kp.prims = (const gpu::Prim*)(base + s->off_prims);
  kp.insts = (const gpu::Inst*)(base + s->off_insts);
  kp.media = (const gpu::Medium*)(base + s->off_media);
  kp.mats = (const gpu::Mat*)(base + s->off_mats);
  kp.texs = (const gpu::Tex*)(base + s->off_texs);
  kp.perlin = (const gpu::Perlin*)(base + s->off_perlin);
  kp.images = base + s->off_images;
  kp.chains = (const float4*)(base + s->off_chains);
  kp.main_end = s->main_end;
  kp.ln_e = s->ln_e;
  kp.n_nodes = (uint32_t)s->g_nodes.size();
  kp.n_prims = (uint32_t)s->g_prims.size();
  kp.motion_uniform = s->motion_uniform ? 1u : 0u;
  kp.motion_t0 = s->motion_t0;
  kp.motion_span = s->motion_span;
  kp.time0 = q->time0;
  kp.time1 = q->time1;
  kp.seed = q->seed;
  return kp;
}

/* what scatter_step reads of the committed scene (scatter.h) */
inline lane::KParams scene_scatter_params(const hrt_scene* s, const hrt_scatter_params* sp) {
  lane::KParams kp;
  memset(&kp, 0, sizeof(kp));
  const uint8_t* base = (const uint8_t*)s->d_blob;
  kp.mats = (const gpu::Mat*)(base + s->off_mats);
  kp.texs = (const gpu::Tex*)(base + s->off_texs);
  kp.perlin = (const gpu::Perlin*)(base + s->off_perlin);
  kp.images = base + s->off_images;
  kp.n_mats = (uint32_t)s->g_mats.size();
  kp.n_texs = (uint32_t)s->g_texs.size();
  kp.n_perlin = (uint32_t)s->perlin.size();
  kp.perlin_lds = 0u;
  kp.background = v3(sp->background[0], sp->background[1], sp->background[2]);
  return kp;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace hrt
