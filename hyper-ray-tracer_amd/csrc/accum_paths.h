/*
 * accum_paths.h — a batch of caller-traced paths added to the sample accumulator as ONE pass (hrt_accum_add_paths,
 * include/hrt/hrt.h): the same code on the device (accum.hip accumulate_paths) and on the host (hrt_debug_accum_paths
 * with on_device = 0), like accum.h: built with -ffp-contract=off, all arithmetic in f32.
 *
 * No arithmetic is new.  The batch is packed as hrt_camera_paths packs it: a pixel's S = p->samples records are
 * consecutive, record k being sample p->sample_offset + k.  A render sums a pixel's samples chunk by chunk (lane.h
 * chunk_range on the pass's schedule; kernel_common.h finish_sample: sum = v3(0, 0, 0), then sum = sum + rad sample
 * by sample) and hands the chunk sums to accum.h: pass_sum, add_pass, and with a noise plane pass_moment, add_moment.
 * Here the chunk sums are made from the records' radiance in that order (PathChunks) and handed to the same functions.
 * A record's radiance is taken as the three floats it holds, whatever its flags.
 */
#pragma once
#include "accum.h"
#include "lane.h"

namespace hrt {
namespace accum {

/* the pass's schedule (render_host.h chunk_schedule): the samples of chunk c, and as pass_moment's count_of */
struct PathSchedule {
  uint32_t chunk, chunk_head, chunk_first;
  HRT_HD void range(uint32_t c, uint32_t& s0, uint32_t& s1) const {
    lane::KParams P; /* chunk_range reads these three fields alone */
    P.chunk = chunk;
    P.chunk_head = chunk_head;
    P.chunk_first = chunk_first;
    lane::chunk_range(P, c, s0, s1);
  }
  HRT_HD uint32_t operator()(uint32_t c) const {
    uint32_t s0, s1;
    range(c, s0, s1);
    return s1 - s0;
  }
};

/* chunk c's sum of one pixel.  records(k): record k of the pixel, its radiance in .x .y .z. */
template <class Records>
HRT_HD Vec3 chunk_sum(const Records& records, const PathSchedule& schedule, uint32_t c) {
  uint32_t s0, s1;
  schedule.range(c, s0, s1);
  Vec3 sum = v3(0.0f, 0.0f, 0.0f);
  for (uint32_t k = s0; k < s1; k++) {
    const auto r = records(k);
    sum = sum + v3(r.x, r.y, r.z);
  }
  return sum;
}

/* One pixel's chunk sums, presented as pass_sum and pass_moment read `partial` (n = 1, i = 0: entry c is chunk c's
 * sum), each made when it is asked for: for records that cannot be written over (the host's, a kernel's in global
 * memory).  With a noise plane every chunk is then folded twice, once for the sum and once for the moment. */
template <class Records>
struct PathChunks {
  const Records& records;
  PathSchedule schedule;
  struct Sum {
    float x, y, z;
  };
  HRT_HD Sum operator[](size_t c) const {
    const Vec3 sum = chunk_sum(records, schedule, (uint32_t)c);
    return Sum{sum.x, sum.y, sum.z};
  }
};

/* acc and (m2 not null) *m2 of one pixel after the pass whose chunk sums `chunks` holds as `partial` holds them */
template <class Chunks>
HRT_HD Vec3 add_chunk_sums(const Chunks& chunks, const PathSchedule& schedule, uint32_t n_chunks, Vec3 acc, float* m2) {
  if (m2) *m2 = add_moment(*m2, pass_moment(chunks, n_chunks, 1, 0, schedule));
  return add_pass(acc, pass_sum(chunks, n_chunks, 1, 0));
}
/* ... of its records */
template <class Records>
HRT_HD Vec3 add_paths(const Records& records, const PathSchedule& schedule, uint32_t n_chunks, Vec3 acc, float* m2) {
  return add_chunk_sums(PathChunks<Records>{records, schedule}, schedule, n_chunks, acc, m2);
}
/* ... of its records staged in a row of F4 that may be written over: chunk c's sum goes to row[c] first, which is safe in
 * place because chunk c begins at sample s0 >= c (no chunk is empty), so slot c has been read by then; every record is
 * then folded once, and the sums and the moment read the same n_chunks slots. */
template <class F4>
HRT_HD Vec3 add_paths_in_place(F4* row, const PathSchedule& schedule, uint32_t n_chunks, Vec3 acc, float* m2) {
  const auto records = [row](uint32_t k) { return row[k]; };
  for (uint32_t c = 0; c < n_chunks; c++) {
    const Vec3 sum = chunk_sum(records, schedule, c);
    row[c].x = sum.x, row[c].y = sum.y, row[c].z = sum.z;
  }
  return add_chunk_sums(static_cast<const F4*>(row), schedule, n_chunks, acc, m2);
}

}  // namespace accum
}  // namespace hrt
