/*
 * primary_list_wide.hip — TEST INFRASTRUCTURE: the camera segment's 16-entry leaf lists (csrc/primary_list.h
 * build_cell_wide: a cell's record and its extension record) held against the walk they replace (csrc/lane.h),
 * on the host, over the flattened scene of hrt_debug_scene_blob.  The wide counterpart of primary_list.hip, whose
 * rays it reuses: every pixel of the cell x the samples from start_sample, plus the footprint's four corners at
 * the jitter's two ends with nine lens samples each.  Built by tests/test_primary_lists_wide.py (host-only
 * compile); not part of libhrt.
 */
#include <cstring>
#include <vector>

#include "lane.h"
#include "primary_list.h"

using namespace hrt;
using namespace hrt::lane;

namespace {

KParams make_params(const void* blob, const hrt_blob_info* bi, const hrt_camera* cam, const hrt_render_params* p) {
  const uint8_t* base = (const uint8_t*)blob;
  KParams P;
  memset(&P, 0, sizeof(P));
  P.motion_uniform = bi->motion_uniform;
  P.motion_t0 = bi->motion_t0;
  P.motion_span = bi->motion_span;
  P.walk = base + bi->off_walk;
  P.walk_bytes = bi->walk_bytes;
  P.walk_end = bi->walk_bytes;
  P.walk_half = 16u;
  P.cam_origin = v3(cam->origin[0], cam->origin[1], cam->origin[2]);
  P.cam_llc = v3(cam->lower_left_corner[0], cam->lower_left_corner[1], cam->lower_left_corner[2]);
  P.cam_h = v3(cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]);
  P.cam_v = v3(cam->vertical[0], cam->vertical[1], cam->vertical[2]);
  P.cam_u = v3(cam->u[0], cam->u[1], cam->u[2]);
  P.cam_vv = v3(cam->v[0], cam->v[1], cam->v[2]);
  P.lens_radius = cam->lens_radius;
  P.time0 = cam->time0;
  P.time1 = cam->time1;
  P.W = p->width;
  P.H = p->height;
  set_pixel_rcp(P);
  P.spp = p->samples;
  P.max_depth = p->max_depth;
  P.sample_offset = p->sample_offset;
  P.t_min = p->t_min;
  P.seed = p->seed;
  return P;
}

bool listable(const hrt_blob_info* bi) {
  return bi->walk_bytes > 0 && !bi->walk_general && !bi->walk_c16 && bi->walk_hot == 0 &&
         (bi->walk_half == 0 || bi->walk_half == 16u) && bi->walk_bytes <= plist::PL_MAX_WALK_BYTES;
}

/* start_sample's ray for the pixel position (x, y) = (px + jitter) and the lens sample `disk` (lane.h start_sample) */
void camera_ray(const KParams& P, float xu, float xv, float dx, float dy, Vec3& ro, Vec3& rd) {
  const float aw = (float)P.W - 1.0f, ah = (float)P.H - 1.0f;
  const float qu = xu * P.rw1, qv = xv * P.rh1;
  const float u = fmaf(fmaf(-qu, aw, xu), P.rw1, qu);
  const float v = fmaf(fmaf(-qv, ah, xv), P.rh1, qv);
  const Vec3 rdk = P.lens_radius * v3(dx, dy, 0.0f);
  const Vec3 offset = P.cam_u * rdk.x + P.cam_vv * rdk.y;
  ro = P.cam_origin + offset;
  rd = (((P.cam_llc + u * P.cam_h) + v * P.cam_v) - P.cam_origin) - offset;
}

struct CellStats {
  uint64_t rays, nan_rays;
  uint64_t walk_nodes, walk_leaf; /* the stream walk: node steps, leaves handed to walk_leaf_test */
  uint64_t list_steps, list_leaf; /* the list walk over both records: box steps, leaves handed to walk_leaf_test */
  uint64_t missing;               /* leaves the stream walk tested that are on neither record (a usable list) */
  uint64_t mismatch;              /* rays whose list walk gives other (closest, winner) bits */
  uint64_t hull_out;              /* rays outside the cell's padded hull */
};
constexpr int CELL_STATS_WORDS = 9;
static_assert(sizeof(CellStats) == CELL_STATS_WORDS * sizeof(uint64_t), "CellStats is nine u64");

void check_ray(const KParams& P, const WalkSrc& src, const plist::Beam& B, const uint16_t* e16, Vec3 ro, Vec3 rd, float time,
               CellStats& st) {
  const float inf = u2f(0x7f800000u);
  {
    const double o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
    bool in = true;
    for (int k = 0; k < 3; k++)
      in = in && o[k] >= B.Llo[k] && o[k] <= B.Lhi[k] && o[k] + d[k] >= B.Tlo[k] && o[k] + d[k] <= B.Thi[k];
    if (!in) st.hull_out++;
  }
  TRay r;
  set_ray(r, ro, rd, time, P);
  Counts cn{0u, 0u, 0u, 0u, 0u, 0u};
  st.rays++;
  const bool usable = e16[0] != plist::PL_OVERFLOW;
  float closest = inf;
  uint32_t winner = G::NONE, node = 0u;
  while (node < P.walk_end) {
    const uint32_t at = node;
    walk_box<true, WM_HOST, HRT_BOX_FMA != 0, true>(src, node, r, P.t_min, closest, cn);
    st.walk_nodes++;
    if (!walk_pending(node)) continue;
    st.walk_leaf++;
    if (usable && !nan_mode(r)) {
      bool on = false;
      for (uint32_t j = 0; j < plist::PL_CAP_WIDE; j++) on = on || e16[j] == (at >> 4);
      if (!on) st.missing++;
    }
    walk_prim<true, WM_HOST>(P, src, node, r, closest, winner, cn);
  }
  if (nan_mode(r)) st.nan_rays++;
  if (!usable || nan_mode(r)) return;
  /* the list walk as the kernel's camera phase makes it: the record's entries to the first unused one, and the
   * extension record's only behind a full record */
  float lc = inf;
  uint32_t lw = G::NONE;
  for (uint32_t half = 0; half < 2; half++) {
    const uint16_t* e = e16 + plist::PL_CAP * half;
    for (uint32_t j = 0; j < plist::PL_CAP && e[j] != plist::PL_UNUSED; j++) {
      st.list_steps++;
      uint32_t leaf;
      if (list_step<true, WM_HOST>(src, (uint32_t)e[j] << 4, r, P.t_min, lc, cn, leaf)) {
        st.list_leaf++;
        walk_leaf_test<true, WM_HOST>(P, src, leaf, r, lc, lw, cn);
      }
    }
    if (e[plist::PL_CAP - 1] == plist::PL_UNUSED) break;
  }
  if (f2u(lc) != f2u(closest) || lw != winner) st.mismatch++;
}

}  // namespace

extern "C" {

int plw_listable(const hrt_blob_info* bi) { return listable(bi) ? 1 : 0; }

/* The wide lists of n cells (cells[2 i], cells[2 i + 1] = bx, by) at capacity cap in [1, 16]: records[16 i ..] the
 * record's entries then the extension record's, counts[i] the leaves the cell's beam meets.  records may be null
 * (a count-only pass). */
int plw_build(const void* blob, const hrt_blob_info* bi, const hrt_camera* cam, const hrt_render_params* p, uint32_t cap,
              const uint32_t* cells, uint32_t n, uint16_t* records, uint32_t* counts) {
  if (!listable(bi) || cap < 1 || cap > plist::PL_CAP_WIDE) return 1;
  const KParams P = make_params(blob, bi, cam, p);
  for (uint32_t i = 0; i < n; i++) {
    plist::Record rec, ext;
    counts[i] = plist::build_cell_wide(P, cells[2 * i], cells[2 * i + 1], cap, rec, ext);
    if (records) {
      memcpy(records + 16 * i, rec.e, sizeof(rec.e));
      memcpy(records + 16 * i + 8, ext.e, sizeof(ext.e));
    }
  }
  return 0;
}

/* build_cell's records (capacity cap in [1, 8]) of the same cells: records[8 i ..] */
int plw_build_narrow(const void* blob, const hrt_blob_info* bi, const hrt_camera* cam, const hrt_render_params* p, uint32_t cap,
                     const uint32_t* cells, uint32_t n, uint16_t* records, uint32_t* counts) {
  if (!listable(bi) || cap < 1 || cap > plist::PL_CAP) return 1;
  const KParams P = make_params(blob, bi, cam, p);
  for (uint32_t i = 0; i < n; i++) {
    plist::Record rec;
    counts[i] = plist::build_cell(P, cells[2 * i], cells[2 * i + 1], cap, rec);
    memcpy(records + 8 * i, rec.e, sizeof(rec.e));
  }
  return 0;
}

/* One cell: its wide list against the walks of its camera rays (primary_list.hip pl_check_cell's rays).
 * out: CellStats as 9 u64; count: the leaves the beam meets. */
int plw_check_cell(const void* blob, const hrt_blob_info* bi, const hrt_camera* cam, const hrt_render_params* p, uint32_t cap,
                   uint32_t bx, uint32_t by, uint64_t* out, uint32_t* count) {
  if (!listable(bi) || cap < 1 || cap > plist::PL_CAP_WIDE) return 1;
  const KParams P = make_params(blob, bi, cam, p);
  if (8u * bx >= P.W || 8u * by >= P.H) return 2;
  WalkSrc src;
  src.base = P.walk;
  src.half = 16u;
  plist::Record rec, ext;
  *count = plist::build_cell_wide(P, bx, by, cap, rec, ext);
  uint16_t e16[plist::PL_CAP_WIDE];
  memcpy(e16, rec.e, sizeof(rec.e));
  memcpy(e16 + plist::PL_CAP, ext.e, sizeof(ext.e));
  const plist::Beam B = plist::cell_beam(P, bx, by);
  CellStats st;
  memset(&st, 0, sizeof(st));
  const uint32_t x1 = 8u * bx + 8u < P.W ? 8u * bx + 8u : P.W, y1 = 8u * by + 8u < P.H ? 8u * by + 8u : P.H;
  for (uint32_t py = 8u * by; py < y1; py++)
    for (uint32_t px = 8u * bx; px < x1; px++)
      for (uint32_t s = 0; s < P.spp; s++) {
        PathState ps;
        init_path_state(ps);
        start_sample(P, ps, px, py, s);
        check_ray(P, src, B, e16, ps.ro, ps.rd, ps.rtime, st);
      }
  const float top = 1.0f - 0x1p-24f, rim = 0.99999994f, dg = 0.7071067f;
  const float disk[9][2] = {{0.0f, 0.0f}, {rim, 0.0f}, {-rim, 0.0f}, {0.0f, rim}, {0.0f, -rim},
                            {dg, dg}, {dg, -dg}, {-dg, dg}, {-dg, -dg}};
  const float times[2] = {P.time0, P.time1};
  for (int cy = 0; cy < 2; cy++)
    for (int cx = 0; cx < 2; cx++) {
      const float xu = (float)(cx ? x1 - 1u : 8u * bx) + (cx ? top : 0.0f);
      const float xv = (float)(cy ? y1 - 1u : 8u * by) + (cy ? top : 0.0f);
      for (int d = 0; d < 9; d++) {
        Vec3 ro, rd;
        camera_ray(P, xu, xv, disk[d][0], disk[d][1], ro, rd);
        check_ray(P, src, B, e16, ro, rd, times[d & 1], st);
      }
    }
  memcpy(out, &st, sizeof(st));
  return 0;
}

}  // extern "C"
