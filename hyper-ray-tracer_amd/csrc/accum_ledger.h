/* accum_ledger.h — which samples, in how many chunks, every tile of a sample accumulator (accum.hip hrt_accum)
 * holds.  Host only and free of HIP, so tests/test_accum_ledger.py drives it without a GPU. */
#pragma once
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

namespace hrt {

/* the sorted, disjoint, coalesced [begin, end) sample ranges an accumulator holds (ends up to 2^32) */
struct SampleRange {
  uint64_t begin, end;
};
inline bool ranges_overlap(const std::vector<SampleRange>& have, const SampleRange& r) {
  for (const SampleRange& h : have)
    if (r.begin < h.end && h.begin < r.end) return true;
  return false;
}
/* r is non-empty and overlaps nothing in `have` */
inline void ranges_insert(std::vector<SampleRange>& have, SampleRange r) {
  size_t at = 0;
  while (at < have.size() && have[at].begin < r.begin) at++;
  have.insert(have.begin() + at, r);
  for (size_t i = 0; i + 1 < have.size();) {
    if (have[i].end == have[i + 1].begin) {
      have[i].end = have[i + 1].end;
      have.erase(have.begin() + i + 1);
    } else {
      i++;
    }
  }
}
inline uint64_t ranges_total(const std::vector<SampleRange>& have) {
  uint64_t n = 0;
  for (const SampleRange& h : have) n += h.end - h.begin;
  return n;
}

/* One record while every tile holds the same passes (a pass over 8160 tiles is one insert); a record per tile from
 * the first pass over a subset of the tiles until every tile holds the same ranges AND chunks again. */
class AccumLedger {
 public:
  enum Refusal { ADDABLE = 0, BAD_RANGE, OVERLAP }; /* BAD_RANGE: empty, or its end past 2^32 */
  /* what a tile (or, shared, every tile) holds */
  struct Record {
    std::vector<SampleRange> ranges;
    uint64_t chunks = 0;
  };
  explicit AccumLedger(size_t n_tiles = 0) : n_tiles_(n_tiles), held_(1) {}
  /* from records() of a ledger of n_tiles tiles (a decoded snapshot): one record, or one per tile */
  AccumLedger(size_t n_tiles, std::vector<Record> records) : n_tiles_(n_tiles), held_(std::move(records)) { rejoin(); }

  bool uniform() const { return held_.size() == 1; }
  bool empty() const { return uniform() && held_[0].ranges.empty(); } /* tiles that differ hold samples */
  /* the ranges every tile holds; null while the tiles differ */
  const std::vector<SampleRange>* ranges() const { return uniform() ? &held_[0].ranges : nullptr; }
  uint64_t samples(size_t t) const { return ranges_total(of(t).ranges); }
  uint64_t chunks(size_t t) const { return of(t).chunks; }

  /* may r be added to tiles idx[0..n) (in range, each once; null: every tile)?  Nothing changes. */
  Refusal may_add(const SampleRange& r, const uint32_t* idx = nullptr, size_t n = 0) const {
    if (r.begin >= r.end || r.end > (1ull << 32)) return BAD_RANGE;
    if (uniform()) return ranges_overlap(held_[0].ranges, r) ? OVERLAP : ADDABLE;
    for (size_t i = 0; i < (idx ? n : n_tiles_); i++)
      if (ranges_overlap(held_[idx ? idx[i] : i].ranges, r)) return OVERLAP;
    return ADDABLE;
  }
  /* a pass of k chunks over r, which may_add() allowed, on the same tiles */
  void record(const SampleRange& r, uint64_t k, const uint32_t* idx = nullptr, size_t n = 0) {
    if (uniform() && idx) held_.resize(n_tiles_, Held(held_[0])); /* the first subset pass: every tile starts from the shared record */
    for (size_t i = 0; i < (idx ? n : held_.size()); i++) add(held_[idx ? idx[i] : i], r, k);
    rejoin();
  }
  /* the ranges and chunks of src, which may_add() allowed one by one; both uniform() */
  void merge(const AccumLedger& src) {
    for (const SampleRange& r : src.held_[0].ranges) add(held_[0], r, 0);
    held_[0].chunks += src.held_[0].chunks;
  }
  void clear() { held_.assign(1, Held()); }

  /* the records as held: one while uniform(), else one per tile (the snapshot codec writes them as they are) */
  const std::vector<Record>& records() const { return held_; }
  /* may src (of the same tiles) be merged tile by tile: for every tile, src's ranges disjoint from this one's? */
  bool may_merge(const AccumLedger& src) const {
    for (size_t t = 0; t < n_tiles_; t++)
      for (const SampleRange& r : src.of(t).ranges)
        if (ranges_overlap(of(t).ranges, r)) return false;
    return true;
  }
  /* every tile for which src holds samples takes src's ranges and chunks (may_merge() allowed it); the others stay as
   * they are.  Two uniform() ledgers: merge(). */
  void merge_tiles(const AccumLedger& src) {
    if (uniform() && src.uniform()) return merge(src);
    if (uniform()) held_.resize(n_tiles_, Held(held_[0]));
    for (size_t t = 0; t < n_tiles_; t++) {
      const Held& s = src.of(t);
      if (s.ranges.empty()) continue;
      for (const SampleRange& r : s.ranges) add(held_[t], r, 0);
      held_[t].chunks += s.chunks;
    }
    rejoin();
  }

 private:
  using Held = Record;
  /* one record again once every tile holds the same passes (e.g. the pass went to all of them) */
  void rejoin() {
    for (const Held& h : held_) {
      const auto &x = held_[0].ranges, &y = h.ranges;
      if (h.chunks != held_[0].chunks || x.size() != y.size() ||
          (!x.empty() && memcmp(x.data(), y.data(), x.size() * sizeof(SampleRange)) != 0))
        return;
    }
    held_.resize(1);
  }
  static void add(Held& h, const SampleRange& r, uint64_t k) {
    ranges_insert(h.ranges, r);
    h.chunks += k;
  }
  const Held& of(size_t t) const { return held_[uniform() ? 0 : t]; }
  size_t n_tiles_;
  std::vector<Held> held_; /* one record for every tile, or one per tile while the tiles hold DIFFERENT passes */
};

}  // namespace hrt
