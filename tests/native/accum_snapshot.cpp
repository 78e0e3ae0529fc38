/* csrc/accum_snapshot.h (the snapshot codec) and the ledger members it needs (records, construction from records,
 * may_merge, merge_tiles) behind a C interface for tests/test_accum_snapshot.py, which links this file with
 * accum_ledger.cpp: the ledgers here are that file's handles. */
#include "accum_snapshot.h"

using hrt::AccumLedger;
using hrt::SampleRange;
namespace snap = hrt::snapshot;

extern "C" {

int ledger_may_merge(const void* dst, const void* src) {
  return static_cast<const AccumLedger*>(dst)->may_merge(*static_cast<const AccumLedger*>(src));
}
void ledger_merge_tiles(void* dst, const void* src) { static_cast<AccumLedger*>(dst)->merge_tiles(*static_cast<const AccumLedger*>(src)); }
uint32_t ledger_n_records(const void* l) { return (uint32_t)static_cast<const AccumLedger*>(l)->records().size(); }
uint64_t ledger_record_chunks(const void* l, uint32_t rec) { return static_cast<const AccumLedger*>(l)->records()[rec].chunks; }
/* record rec's ranges as (begin, end) pairs into out[2 * cap]; returns their number */
uint32_t ledger_record_ranges(const void* l, uint32_t rec, uint64_t* out, uint32_t cap) {
  const std::vector<SampleRange>& r = static_cast<const AccumLedger*>(l)->records()[rec].ranges;
  for (size_t i = 0; i < r.size() && i < cap; i++) out[2 * i] = r[i].begin, out[2 * i + 1] = r[i].end;
  return (uint32_t)r.size();
}
/* n_records records: chunks[i], n_ranges[i] and their (begin, end) pairs one after the other in `ranges` */
void* ledger_from_records(uint32_t n_tiles, uint32_t n_records, const uint64_t* chunks, const uint32_t* n_ranges, const uint64_t* ranges) {
  std::vector<AccumLedger::Record> recs(n_records);
  for (uint32_t i = 0; i < n_records; i++) {
    recs[i].chunks = chunks[i];
    for (uint32_t k = 0; k < n_ranges[i]; k++, ranges += 2) recs[i].ranges.push_back(SampleRange{ranges[0], ranges[1]});
  }
  return new AccumLedger(n_tiles, std::move(recs));
}

/* what snap_decode found, beside the tile list, the identity bytes and the two ledgers */
struct SnapView {
  uint32_t flags, width, height, n_tiles, has_identity, n_records, n_feature_ranges, pad;
  uint64_t n_px, off_sums, off_m2, off_fa, off_fn, bytes;
};

/* The blob of an accumulator with these tiles (n_tiles x (x, y, w, h)), identity (128 bytes, or null: none), ledgers
 * (features null: no feature ledger) and planes (null where the flags have none).  Returns its size; written when
 * cap >= that. */
uint64_t snap_encode(uint32_t flags, uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t n_tiles, const uint8_t* identity,
                     const void* ledger, const void* features, const void* sums, const void* m2, const void* fa, const void* fn,
                     uint8_t* out, uint64_t cap) {
  snap::State s;
  s.flags = flags, s.width = width, s.height = height;
  for (uint32_t t = 0; t < n_tiles; t++) s.tiles.push_back(snap::Tile{tiles[4 * t], tiles[4 * t + 1], tiles[4 * t + 2], tiles[4 * t + 3]});
  s.has_identity = identity != nullptr;
  if (identity) memcpy(s.identity, identity, snap::IDENTITY_BYTES);
  s.records = static_cast<const AccumLedger*>(ledger)->records();
  if (features) s.f_ranges = *static_cast<const AccumLedger*>(features)->ranges();
  snap::layout(s);
  if (cap < s.bytes) return s.bytes;
  snap::encode_head(s, out);
  memcpy(out + s.off_sums, sums, 16 * s.n_px);
  if (s.off_m2) memcpy(out + s.off_m2, m2, 4 * s.n_px);
  if (s.off_fa) memcpy(out + s.off_fa, fa, 16 * s.n_px), memcpy(out + s.off_fn, fn, 16 * s.n_px);
  snap::zero_pads(s, out);
  snap::seal(s, out);
  return s.bytes;
}

/* snapshot::decode: returns its Error; on OK fills view, tiles (when tile_cap >= n_tiles), identity (128 bytes) and
 * makes the two ledgers (ledger_free them) */
int snap_decode(const void* blob, uint64_t size, SnapView* view, uint32_t* tiles, uint32_t tile_cap, uint8_t* identity, void** ledger,
                void** features) {
  snap::State s;
  const snap::Error e = snap::decode(blob, size, s);
  if (e != snap::OK) return e;
  *view = SnapView{s.flags, s.width, s.height, (uint32_t)s.tiles.size(), s.has_identity ? 1u : 0u, (uint32_t)s.records.size(),
                   (uint32_t)s.f_ranges.size(), 0u, s.n_px, s.off_sums, s.off_m2, s.off_fa, s.off_fn, s.bytes};
  for (size_t t = 0; t < s.tiles.size() && s.tiles.size() <= tile_cap; t++)
    tiles[4 * t] = s.tiles[t].x, tiles[4 * t + 1] = s.tiles[t].y, tiles[4 * t + 2] = s.tiles[t].w, tiles[4 * t + 3] = s.tiles[t].h;
  memcpy(identity, s.identity, snap::IDENTITY_BYTES);
  *ledger = new AccumLedger(s.tiles.size(), std::move(s.records));
  std::vector<AccumLedger::Record> fr(1);
  fr[0].ranges = std::move(s.f_ranges);
  *features = new AccumLedger(s.tiles.size(), std::move(fr));
  return snap::OK;
}

uint64_t snap_checksum(const uint8_t* p, uint64_t n_words) { return snap::checksum(p, n_words); }

}  // extern "C"
