/*
 * primary_list.h — the per-cell leaf lists of the camera segment ("Camera beams"), the same
 * code on the device (render.hip build_primary_lists) and on the host (tests/native/primary_list.hip,
 * scripts/price_primary.py), like accum.h and lane.h.
 *
 * A CELL is a frame-aligned 8x8 pixel square (px >> 3, py >> 3).  Every camera ray of a cell, whatever its
 * sample, jitter and lens point, lies in one thin beam, so the walk-stream leaves such a ray's walk can hand to
 * walk_leaf_test are the few whose inflated box the beam meets.  The builder lists them in leaf (pre-order)
 * order; the sphere kernel then tests a camera ray against its cell's list instead of walking the hierarchy
 * (render_sphere.hip).
 *
 * A list holds up to 16 leaves in two 16-B records of two tables: the cell's record (entries 0 .. 7, what
 * build_cell fills) and its extension record (entries 8 .. 15, build_cell_wide).  A cell with more leaves than
 * the capacity gets an overflow record and its rays walk the stream.  The builder walks the stream with the
 * beam as a ray would, leaving by its skip link every subtree whose inner box the beam misses, so a cell costs
 * a few dozen box tests, not one per leaf.  A launch builds the lists once per view (render.hip: the scene keeps
 * them while the stream, the camera, the frame size and the capacity stay the same).
 *
 * Soundness: a leaf is left out only if its box [C - E, C + E], inflated as lane.h box_ce inflates it and padded
 * for every f32 rounding between the camera and the slab comparison, misses a hull of all the cell's rays in
 * real arithmetic (f64 here, whose own rounding is 2^-29 of the smallest pad).  The hull only has to hold the
 * rays, and the list only has to hold the leaves: both may be loose.
 *
 * The hull.  start_sample's ray is o = O + offset, d = T - o with the lens point o in the disk O + R (x u + y v),
 * x^2 + y^2 <= 1, and the target T = llc + s h + t vert on the focus plane, s in [8 bx, 8 bx + 8] / (W - 1), t
 * likewise (the jitter is in [0, 1], both ends included: px + gen_f32() may round up to px + 1).  A ray point is
 * P(l) = (1 - l) o + l T for the ray parameter l >= 0 (the walk's t: t_min > 0 keeps rays forward).  Per world
 * axis k, with o_k in [Llo, Lhi] and T_k in [Tlo, Thi]:
 *   0 <= l <= 1:  P_k in [(1 - l) Llo + l Tlo, (1 - l) Lhi + l Thi]
 *   l >= 1:       P_k in [(1 - l) Lhi + l Tlo, (1 - l) Llo + l Thi]
 * both ends linear in l, so "P_k(l) can lie in [lo_k, hi_k]" is an interval of l per axis and piece, and a box
 * is missed when the three axes' intervals have no common l in either piece.  The axes share l, so the hull's
 * cross-section at each depth is the beam's own bounding box there, not the bounding box of the whole beam.
 *
 * The pads (HRT_PL_NO_PAD builds leave them out, to show that the test of the lists can fail):
 *   - the ray: o and d are a handful of f32 operations on numbers no larger than mag_k = |O_k| + |llc_k| +
 *     |h_k| + |vert_k| + R; each rounds by at most 2^-24 of that, and the quotients s, t by 2^-24 relative.  The
 *     lens range is padded by 2^-20 mag_k and the target range by twice that (T stands for o + d here, so it
 *     carries both errors); the lens radius by 2^-20 relative (the disk sample's own rounding);
 *   - the inflation: box_ce inflates by EXACT_MARGIN x dist with dist = max_k (|C_k - o_k| + E_k) rounded in f32;
 *     the builder takes the largest dist over the padded lens range, times 1 + 2^-13;
 *   - the slab arithmetic: m = fma(C, 1/d, -(o / d)) errs by 2^-24 (|o_k| + |C_k - o_k|) in position units
 *     (section 4, the fused form), and t = fma(dist, MARGIN, E) by 2^-23 relative; the box is padded by
 *     2^-18 (|o_k|max + |C_k| + E_k) per axis, 64 times the first and 32 times the second.
 */
#pragma once
#include <stdint.h>

#include "lane.h"

namespace hrt {
namespace plist {

namespace G = hrt::gpu;

constexpr uint32_t PL_CAP = 8;          /* entries of a record (8 x u16 = 16 B) */
constexpr uint32_t PL_CAP_WIDE = 16;    /* entries of a list: a record and its extension record */
constexpr uint32_t PL_UNUSED = 0xFFFFu; /* an unused entry */
constexpr uint32_t PL_OVERFLOW = 0xFFFEu; /* entry 0 of an overflow record: the cell's rays take the walk */
/* entries are node-part offsets / 16: the stream must end within 65 535 units, below the two codes */
constexpr uint32_t PL_MAX_WALK_BYTES = 65535u * 16u;

struct alignas(16) Record {
  uint16_t e[PL_CAP];
};
static_assert(sizeof(Record) == 16, "a leaf list is one 16-byte record");

HRT_HD uint32_t cells_x(uint32_t W) { return (W + 7u) >> 3; }
HRT_HD uint32_t cells_y(uint32_t H) { return (H + 7u) >> 3; }

#ifdef HRT_PL_NO_PAD
constexpr double PL_PAD = 0.0;
#else
constexpr double PL_PAD = 1.0;
#endif

HRT_HD double dmin(double a, double b) { return a < b ? a : b; }
HRT_HD double dmax(double a, double b) { return a > b ? a : b; }
HRT_HD double dabs(double a) { return a < 0.0 ? -a : a; }

/* the beam of one cell: per world axis the range of lens points and of focus-plane targets, padded */
struct Beam {
  double Llo[3], Lhi[3], Tlo[3], Thi[3];
  double omax[3]; /* max |o_k| over the lens range */
};

HRT_HD Beam cell_beam(const lane::KParams& P, uint32_t bx, uint32_t by) {
  const double O[3] = {P.cam_origin.x, P.cam_origin.y, P.cam_origin.z};
  const double llc[3] = {P.cam_llc.x, P.cam_llc.y, P.cam_llc.z};
  const double h[3] = {P.cam_h.x, P.cam_h.y, P.cam_h.z}, vt[3] = {P.cam_v.x, P.cam_v.y, P.cam_v.z};
  const double u[3] = {P.cam_u.x, P.cam_u.y, P.cam_u.z}, vv[3] = {P.cam_vv.x, P.cam_vv.y, P.cam_vv.z};
  const double R = dabs((double)P.lens_radius) * (1.0 + PL_PAD * 0x1p-20);
  const double rel = 1.0 + PL_PAD * 0x1p-22; /* s, t: the quotient's rounding */
  const double s0 = 8.0 * bx / ((double)P.W - 1.0) / rel, s1 = (8.0 * bx + 8.0) / ((double)P.W - 1.0) * rel;
  const double t0 = 8.0 * by / ((double)P.H - 1.0) / rel, t1 = (8.0 * by + 8.0) / ((double)P.H - 1.0) * rel;
  Beam b;
  for (int k = 0; k < 3; k++) {
    const double mag = dabs(O[k]) + dabs(llc[k]) + dabs(h[k]) + dabs(vt[k]) + R;
    const double pad = PL_PAD * 0x1p-20 * mag;
    /* the disk's extent along axis k is R sqrt(u_k^2 + v_k^2) */
    const double ext = R * sqrt(u[k] * u[k] + vv[k] * vv[k]) * (1.0 + PL_PAD * 0x1p-40);
    b.Llo[k] = O[k] - ext - pad;
    b.Lhi[k] = O[k] + ext + pad;
    b.Tlo[k] = llc[k] + dmin(s0 * h[k], s1 * h[k]) + dmin(t0 * vt[k], t1 * vt[k]) - 2.0 * pad;
    b.Thi[k] = llc[k] + dmax(s0 * h[k], s1 * h[k]) + dmax(t0 * vt[k], t1 * vt[k]) + 2.0 * pad;
    b.omax[k] = dmax(dabs(b.Llo[k]), dabs(b.Lhi[k]));
  }
  return b;
}

/* [a, b] cut to the l with p + l q <= c (the interval's ends relaxed by the division's rounding) */
HRT_HD void cut_le(double p, double q, double c, double& a, double& b) {
  if (q == 0.0) {
    if (!(p <= c)) b = a - 1.0;
    return;
  }
  const double x = (c - p) / q, slack = 1e-9 * (1.0 + dabs(x));
  if (q > 0.0) b = dmin(b, x + slack);
  else a = dmax(a, x - slack);
}

/* can a ray of the beam reach the box [lo, hi] (per axis)?  false only when none can */
HRT_HD bool beam_meets(const Beam& B, const double* lo, const double* hi) {
  const double inf = __builtin_huge_val();
  /* 0 <= l <= 1: lower end Llo + l (Tlo - Llo) <= hi, upper end Lhi + l (Thi - Lhi) >= lo */
  double a = 0.0, b = 1.0;
  for (int k = 0; k < 3; k++) {
    if (hi[k] < inf) cut_le(B.Llo[k], B.Tlo[k] - B.Llo[k], hi[k], a, b);
    if (lo[k] > -inf) cut_le(-B.Lhi[k], -(B.Thi[k] - B.Lhi[k]), -lo[k], a, b);
  }
  if (a <= b) return true;
  /* l >= 1: lower end Lhi + l (Tlo - Lhi) <= hi, upper end Llo + l (Thi - Llo) >= lo */
  a = 1.0;
  b = inf;
  for (int k = 0; k < 3; k++) {
    if (hi[k] < inf) cut_le(B.Lhi[k], B.Tlo[k] - B.Lhi[k], hi[k], a, b);
    if (lo[k] > -inf) cut_le(-B.Llo[k], -(B.Thi[k] - B.Llo[k]), -lo[k], a, b);
  }
  return a <= b;
}

/* the node part's box (C, E) against the beam, inflated and padded as the header says */
HRT_HD bool leaf_in_beam(const Beam& B, const float4& c, const float4& e) {
  const double C[3] = {c.x, c.y, c.z}, E[3] = {e.x, e.y, e.z};
  double dist = 0.0;
  for (int k = 0; k < 3; k++) dist = dmax(dist, dmax(dabs(C[k] - B.Llo[k]), dabs(C[k] - B.Lhi[k])) + E[k]);
  const double infl = (double)G::EXACT_MARGIN * dist * (1.0 + PL_PAD * 0x1p-13);
  double lo[3], hi[3];
  for (int k = 0; k < 3; k++) {
    const double w = E[k] + infl + PL_PAD * 0x1p-18 * (B.omax[k] + dabs(C[k]) + E[k]);
    lo[k] = C[k] - w; /* E = +inf (a leaf without a box): -inf, +inf */
    hi[k] = C[k] + w;
  }
  return beam_meets(B, lo, hi);
}

/* The leaf list of cell (bx, by) over the walk stream `walk` (32-B node parts, 16 B between a part's halves,
 * laid out whole: layout.h), cap in [1, PL_CAP_WIDE] entries: entries 0 .. 7 in `rec`, entries 8 .. 15 in the
 * extension record `ext` (all unused for a list of at most 8).  Returns the number of leaves the builder meets
 * (more than cap: `rec` is an overflow record, `ext` unused).  A full first record (e[7] used) is all that tells
 * a reader that the extension may hold more.
 * The stream is walked as a ray walks it, with the beam in the ray's place: a node part, inner or leaf, whose
 * padded inflated box the beam misses is left by its skip link, an inner node the beam meets by its pass link
 * (its first child), a leaf by its skip (its successor).  Pruning by inner nodes is sound by the argument of the
 * header: the walk hands a leaf to walk_leaf_test only after its ray passed every ancestor's inflated box, and a
 * beam that misses an ancestor's padded inflated box holds no such ray. */
HRT_HD uint32_t build_cell_wide(const lane::KParams& P, uint32_t bx, uint32_t by, uint32_t cap, Record& rec, Record& ext) {
  const Beam B = cell_beam(P, bx, by);
  for (uint32_t j = 0; j < PL_CAP; j++) rec.e[j] = ext.e[j] = (uint16_t)PL_UNUSED;
  uint32_t n = 0;
  /* the builder's watchdog: a walk visits a node part (32 B) at most once, so more steps than the stream has
   * parts mean links that cycle (a corrupt stream: inner skip links are followed here).  The cell then gets an
   * overflow record and its rays take the stream walk, whose own watchdog reports the scene. */
  uint32_t steps_left = P.walk_end / 32u + 1u;
  for (uint32_t off = 0; off < P.walk_end;) {
    if (steps_left-- == 0u) {
      n = PL_CAP_WIDE + 1u;
      break;
    }
    const float4 a = *reinterpret_cast<const float4*>(P.walk + off);
    const float4 b = *reinterpret_cast<const float4*>(P.walk + off + 16u);
    const uint32_t pass = f2u(b.w);
    if (!leaf_in_beam(B, a, b)) {
      off = f2u(a.w);
      continue;
    }
    if (!lane::walk_pending(pass)) {
      off = pass;
      continue;
    }
    if (n < cap) {
      if (n < PL_CAP) rec.e[n] = (uint16_t)(off >> 4);
      else ext.e[n - PL_CAP] = (uint16_t)(off >> 4);
    }
    n++;
    off = f2u(a.w);
  }
  if (n > cap) {
    for (uint32_t j = 0; j < PL_CAP; j++) rec.e[j] = ext.e[j] = (uint16_t)PL_UNUSED;
    rec.e[0] = (uint16_t)PL_OVERFLOW;
  }
  return n;
}

/* The list of at most cap <= PL_CAP entries: build_cell_wide's first record. */
HRT_HD uint32_t build_cell(const lane::KParams& P, uint32_t bx, uint32_t by, uint32_t cap, Record& rec) {
  Record ext;
  return build_cell_wide(P, bx, by, cap < PL_CAP ? cap : PL_CAP, rec, ext);
}

}  // namespace plist
}  // namespace hrt
