/* accum_snapshot.h — the codec of an accumulator snapshot (hrt_accum_snapshot / _restore / _snapshot_info,
 * include/hrt/hrt.h states the layout): header, tile list, frame identity, the two ledgers, plane offsets, validation
 * and checksum.  Host only and free of HIP, like accum_ledger.h, so tests/test_accum_snapshot.py drives it without a
 * GPU and tests/native/accum_snapshot_san.cpp under the sanitizers; accum.hip adds the device copies of the planes.
 * A blob is untrusted input: the decoder checks every length against `size` before it reads. */
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "accum_ledger.h"

namespace hrt {
namespace snapshot {

constexpr uint32_t MAGIC = 0x53545248u; /* "HRTS" */
constexpr uint32_t VERSION = 1;
constexpr uint32_t FLAG_NOISE = 1, FLAG_FEATURES = 4; /* HRT_ACCUM_NOISE, HRT_ACCUM_FEATURES */
constexpr size_t IDENTITY_BYTES = 128; /* camera 96, max_depth, flags, t_min, background[3], seed */
constexpr size_t HEADER_BYTES = 56 + IDENTITY_BYTES;

struct Tile {
  uint32_t x, y, w, h;
};

/* everything of a snapshot but the planes' contents */
struct State {
  uint32_t flags = 0, width = 0, height = 0;
  std::vector<Tile> tiles;
  bool has_identity = false;
  uint8_t identity[IDENTITY_BYTES] = {0};
  std::vector<AccumLedger::Record> records; /* 1 (every tile holds this) or one per tile */
  std::vector<SampleRange> f_ranges;        /* the feature ledger's */
  /* filled by layout(): pixels, byte offsets of the planes in the blob (0: no such plane), the blob's size */
  uint64_t n_px = 0, off_sums = 0, off_m2 = 0, off_fa = 0, off_fn = 0, bytes = 0;
};

enum Error {
  OK = 0,
  SHORT,      /* shorter than its own header, tile list or ledgers say */
  MAGIC_VERSION,
  SIZE,       /* the size field is not the byte count given, or not what the layout adds up to */
  FIELDS,     /* unknown flags, bad image size, tile outside the image, a pixel count that is not the tiles', reserved != 0 */
  RECORDS,    /* a record count that is neither 1 nor n_tiles; chunks without samples; feature ranges without the flag */
  RANGES,     /* unsorted, overlapping, adjacent (not coalesced), empty or past 2^32 */
  IDENTITY,   /* has_identity == 0 together with samples or identity bytes, or a value other than 0 / 1 */
  CHECKSUM
};

inline uint64_t round16(uint64_t n) { return (n + 15u) & ~(uint64_t)15u; }

inline void put32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline void put64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint32_t get32(const uint8_t* p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i);
  return v;
}
inline uint64_t get64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

/* The checksum of the n_words little-endian u64 words at p (hrt.h states it): four lanes of h = (h ^ word) * P, word j
 * into lane j mod 4, folded at the end.  Every step is a bijection of its lane, so any change confined to one word
 * (a flipped bit) changes the result. */
inline uint64_t checksum(const uint8_t* p, uint64_t n_words) {
  const uint64_t P = 0x100000001B3ull;
  uint64_t h[4];
  for (int i = 0; i < 4; i++) h[i] = 0xCBF29CE484222325ull + (uint64_t)i;
  uint64_t j = 0;
  for (; j + 4 <= n_words; j += 4)
    for (int i = 0; i < 4; i++) {
      uint64_t w;
      memcpy(&w, p + 8 * (j + i), 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
      w = __builtin_bswap64(w);
#endif
      h[i] = (h[i] ^ w) * P;
    }
  for (; j < n_words; j++) h[j & 3u] = (h[j & 3u] ^ get64(p + 8 * j)) * P;
  uint64_t r = h[0];
  for (int i = 1; i < 4; i++) r = (r * P) ^ h[i];
  r = (r ^ n_words) * P;
  return r ^ (r >> 32);
}

/* n_px, the planes' offsets and the blob's size from flags, tiles, records and f_ranges */
inline void layout(State& s) {
  s.n_px = 0;
  for (const Tile& t : s.tiles) s.n_px += (uint64_t)t.w * t.h;
  uint64_t at = HEADER_BYTES + 16ull * s.tiles.size();
  for (const AccumLedger::Record& r : s.records) at += 16 + 16ull * r.ranges.size();
  at += 16ull * s.f_ranges.size();
  at = round16(at);
  s.off_sums = at, at += 16 * s.n_px;
  s.off_m2 = s.off_fa = s.off_fn = 0;
  if (s.flags & FLAG_NOISE) s.off_m2 = at, at += round16(4 * s.n_px);
  if (s.flags & FLAG_FEATURES) {
    s.off_fa = at, at += 16 * s.n_px;
    s.off_fn = at, at += 16 * s.n_px;
  }
  s.bytes = at + 8;
}

/* Everything before the planes into out[0, s.off_sums), after layout(s).  The caller then fills the planes (the pad
 * after m2, [off_m2 + 4 n_px, round16) with zeros: zero_pads) and calls seal. */
inline void encode_head(const State& s, uint8_t* out) {
  memset(out, 0, (size_t)s.off_sums);
  put32(out + 0, MAGIC);
  put32(out + 4, VERSION);
  put64(out + 8, s.bytes);
  put32(out + 16, s.flags);
  put32(out + 20, s.width);
  put32(out + 24, s.height);
  put32(out + 28, (uint32_t)s.tiles.size());
  put64(out + 32, s.n_px);
  put32(out + 40, s.has_identity ? 1u : 0u);
  put32(out + 44, (uint32_t)s.records.size());
  put32(out + 48, (uint32_t)s.f_ranges.size());
  put32(out + 52, 0);
  if (s.has_identity) memcpy(out + 56, s.identity, IDENTITY_BYTES);
  uint8_t* p = out + HEADER_BYTES;
  for (const Tile& t : s.tiles) {
    put32(p, t.x), put32(p + 4, t.y), put32(p + 8, t.w), put32(p + 12, t.h);
    p += 16;
  }
  for (const AccumLedger::Record& r : s.records) {
    put64(p, r.chunks), put64(p + 8, r.ranges.size());
    p += 16;
    for (const SampleRange& g : r.ranges) put64(p, g.begin), put64(p + 8, g.end), p += 16;
  }
  for (const SampleRange& g : s.f_ranges) put64(p, g.begin), put64(p + 8, g.end), p += 16;
}
inline void zero_pads(const State& s, uint8_t* out) {
  if (s.off_m2) memset(out + s.off_m2 + 4 * s.n_px, 0, (size_t)(round16(4 * s.n_px) - 4 * s.n_px));
}
inline void seal(const State& s, uint8_t* out) { put64(out + s.bytes - 8, checksum(out, (s.bytes - 8) / 8)); }

/* n ranges at p (the caller has checked that they lie inside the blob): sorted, disjoint, coalesced, non-empty, <= 2^32 */
inline bool read_ranges(const uint8_t* p, uint64_t n, std::vector<SampleRange>& out) {
  out.resize((size_t)n);
  for (uint64_t i = 0; i < n; i++) {
    const SampleRange r{get64(p + 16 * i), get64(p + 16 * i + 8)};
    if (r.begin >= r.end || r.end > (1ull << 32)) return false;
    if (i > 0 && r.begin <= out[(size_t)i - 1].end) return false;
    out[(size_t)i] = r;
  }
  return true;
}

/* The blob's header, tile list and ledgers into s, its layout computed and held against the size field, then the
 * checksum.  s is meaningful only when OK is returned. */
inline Error decode(const void* blob, uint64_t size, State& s) {
  const uint8_t* b = static_cast<const uint8_t*>(blob);
  if (!b || size < HEADER_BYTES + 8) return SHORT;
  if (get32(b) != MAGIC || get32(b + 4) != VERSION) return MAGIC_VERSION;
  if (get64(b + 8) != size || size % 8 != 0) return SIZE;
  s = State();
  s.flags = get32(b + 16);
  s.width = get32(b + 20);
  s.height = get32(b + 24);
  const uint64_t n_tiles = get32(b + 28), n_px = get64(b + 32), n_records = get32(b + 44), n_f = get32(b + 48);
  const uint32_t has_id = get32(b + 40);
  if ((s.flags & ~(FLAG_NOISE | FLAG_FEATURES)) || s.width < 2 || s.height < 2 || s.width > 65535 || s.height > 65535 ||
      n_tiles == 0 || get32(b + 52) != 0)
    return FIELDS;
  if (has_id > 1) return IDENTITY;
  s.has_identity = has_id == 1;
  memcpy(s.identity, b + 56, IDENTITY_BYTES);
  if (!s.has_identity)
    for (size_t i = 0; i < IDENTITY_BYTES; i++)
      if (s.identity[i]) return IDENTITY;
  uint64_t at = HEADER_BYTES; /* at <= size - 8 throughout: the checksum's 8 bytes are never ledger */
  const uint64_t end = size - 8;
  if (n_tiles > (end - at) / 16) return SHORT;
  s.tiles.resize((size_t)n_tiles);
  for (Tile& t : s.tiles) {
    t = Tile{get32(b + at), get32(b + at + 4), get32(b + at + 8), get32(b + at + 12)};
    at += 16;
    if (t.w == 0 || t.h == 0 || (uint64_t)t.x + t.w > s.width || (uint64_t)t.y + t.h > s.height) return FIELDS;
  }
  if (n_records != 1 && n_records != n_tiles) return RECORDS;
  if (n_f != 0 && !(s.flags & FLAG_FEATURES)) return RECORDS;
  bool samples = false;
  s.records.resize((size_t)n_records);
  for (AccumLedger::Record& r : s.records) {
    if (end - at < 16) return SHORT;
    r.chunks = get64(b + at);
    const uint64_t n = get64(b + at + 8);
    at += 16;
    if (n > (end - at) / 16) return SHORT;
    if (!read_ranges(b + at, n, r.ranges)) return RANGES;
    at += 16 * n;
    if (n == 0 && r.chunks != 0) return RECORDS;
    samples = samples || n != 0;
  }
  if (n_f > (end - at) / 16) return SHORT;
  if (!read_ranges(b + at, n_f, s.f_ranges)) return RANGES;
  if ((samples || n_f != 0) && !s.has_identity) return IDENTITY;
  layout(s);
  if (s.n_px != n_px || s.n_px >= (1ull << 32)) return FIELDS;
  if (s.bytes != size) return SIZE;
  if (get64(b + size - 8) != checksum(b, (size - 8) / 8)) return CHECKSUM;
  return OK;
}

inline const char* error_text(Error e) {
  switch (e) {
    case OK: return "ok";
    case SHORT: return "the blob is shorter than its header, tile list or ledgers say";
    case MAGIC_VERSION: return "not an accumulator snapshot (magic), or another format version";
    case SIZE: return "the blob's size field is not its byte count";
    case FIELDS: return "bad flags, image size, tile list or pixel count";
    case RECORDS: return "a record count that is neither 1 nor the tile count, or a record that cannot be";
    case RANGES: return "sample ranges unsorted, overlapping, not coalesced, empty or past 2^32";
    case IDENTITY: return "samples without a frame identity";
    default: return "bad checksum";
  }
}

}  // namespace snapshot
}  // namespace hrt
