/* The snapshot decoder (csrc/accum_snapshot.h) on hostile input, as a stand-alone program for a sanitizer build
 * (tests/test_accum_snapshot.py compiles it with -fsanitize=address,undefined and runs it as a child process).
 * Every blob handed to the decoder lives in a heap block of exactly its size, so a read past `size` is a report.
 * Fed: a good blob of each flag combination, uniform and per-tile; every truncation of it; every single flipped bit of
 * its header and ledgers, one in each plane and in the checksum; random mutations of header and ledger bytes with the
 * checksum made good again, so that the checks behind the checksum's are reached; and random byte strings, with and
 * without a good magic, version and size field.  Exit status 0: the good blobs decoded to what went in, everything
 * else that was changed was refused or decoded consistently, and no sanitizer spoke. */
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>

#include "accum_snapshot.h"

using hrt::AccumLedger;
using hrt::SampleRange;
namespace snap = hrt::snapshot;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      failures++;                                                 \
    }                                                             \
  } while (0)

/* decode a copy of b[0, n) that lives in a block of exactly n bytes */
static snap::Error decode_exact(const uint8_t* b, size_t n, snap::State& s) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) memcpy(copy.get(), b, n);
  return snap::decode(n ? copy.get() : nullptr, n, s);
}

static std::vector<uint8_t> make_blob(uint32_t flags, bool per_tile, std::mt19937& rng, snap::State& s) {
  s = snap::State();
  s.flags = flags, s.width = 5, s.height = 4;
  s.tiles = {snap::Tile{0, 0, 3, 2}, snap::Tile{3, 0, 2, 2}, snap::Tile{0, 2, 5, 1}};
  s.has_identity = true;
  for (uint8_t& v : s.identity) v = (uint8_t)rng();
  AccumLedger l(s.tiles.size());
  l.record(SampleRange{0, 8}, 2);
  l.record(SampleRange{(1ull << 32) - 4, 1ull << 32}, 1);
  if (per_tile) {
    const uint32_t idx[2] = {2, 0};
    l.record(SampleRange{8, 12}, 3, idx, 2);
  }
  s.records = l.records();
  if (flags & snap::FLAG_FEATURES) s.f_ranges = {SampleRange{0, 4}, SampleRange{16, 20}};
  snap::layout(s);
  std::vector<uint8_t> b(s.bytes);
  snap::encode_head(s, b.data());
  for (uint64_t i = s.off_sums; i < s.bytes - 8; i++) b[i] = (uint8_t)rng();
  snap::zero_pads(s, b.data());
  snap::seal(s, b.data());
  return b;
}

/* a decoded state never describes more than the blob holds */
static void consistent(const snap::State& s, size_t size) {
  EXPECT(s.bytes == size);
  EXPECT(s.off_sums + 16 * s.n_px <= size - 8);
  EXPECT(s.records.size() == 1 || s.records.size() == s.tiles.size());
  if (s.off_fn) EXPECT(s.off_fn + 16 * s.n_px == size - 8);
}

int main() {
  std::mt19937 rng(12345);
  for (uint32_t flags : {0u, snap::FLAG_NOISE, snap::FLAG_FEATURES, snap::FLAG_NOISE | snap::FLAG_FEATURES})
    for (int per_tile = 0; per_tile < 2; per_tile++) {
      snap::State in, out;
      const std::vector<uint8_t> good = make_blob(flags, per_tile != 0, rng, in);
      EXPECT(decode_exact(good.data(), good.size(), out) == snap::OK);
      EXPECT(out.flags == flags && out.tiles.size() == 3 && out.n_px == in.n_px && out.records.size() == (per_tile ? 3u : 1u));
      EXPECT(out.off_sums == in.off_sums && out.off_m2 == in.off_m2 && out.off_fa == in.off_fa && out.off_fn == in.off_fn);
      EXPECT(memcmp(out.identity, in.identity, snap::IDENTITY_BYTES) == 0 && out.f_ranges.size() == in.f_ranges.size());
      for (size_t r = 0; r < out.records.size(); r++) {
        EXPECT(out.records[r].chunks == in.records[r].chunks && out.records[r].ranges.size() == in.records[r].ranges.size());
        EXPECT(memcmp(out.records[r].ranges.data(), in.records[r].ranges.data(), sizeof(SampleRange) * in.records[r].ranges.size()) == 0);
      }
      /* every truncation, and one byte too many */
      for (size_t n = 0; n < good.size(); n++) EXPECT(decode_exact(good.data(), n, out) != snap::OK);
      std::vector<uint8_t> longer(good);
      longer.push_back(0);
      EXPECT(decode_exact(longer.data(), longer.size(), out) != snap::OK);
      /* every bit of header and ledgers; one in each plane; every bit of the checksum */
      std::vector<size_t> bits;
      for (size_t i = 0; i < 8 * in.off_sums; i++) bits.push_back(i);
      for (uint64_t off : {in.off_sums, in.off_m2, in.off_fa, in.off_fn})
        if (off) bits.push_back(8 * (off + rng() % (4 * in.n_px)) + rng() % 8);
      for (size_t i = 8 * (good.size() - 8); i < 8 * good.size(); i++) bits.push_back(i);
      for (size_t bit : bits) {
        std::vector<uint8_t> bad(good);
        bad[bit / 8] ^= (uint8_t)(1u << (bit % 8));
        EXPECT(decode_exact(bad.data(), bad.size(), out) != snap::OK);
      }
      /* mutations behind a good checksum: the other checks must hold on their own */
      for (int round = 0; round < 4000; round++) {
        std::vector<uint8_t> bad(good);
        const int n_mut = 1 + (int)(rng() % 3);
        for (int m = 0; m < n_mut; m++) {
          const size_t at = rng() % (size_t)in.off_sums;
          bad[at] = (rng() & 1u) ? (uint8_t)rng() : (uint8_t)(bad[at] + ((rng() & 1u) ? 1 : -1));
        }
        snap::put64(bad.data() + bad.size() - 8, snap::checksum(bad.data(), (bad.size() - 8) / 8));
        if (decode_exact(bad.data(), bad.size(), out) == snap::OK) consistent(out, bad.size());
      }
    }
  /* random byte strings */
  for (int round = 0; round < 20000; round++) {
    const size_t n = rng() % 600;
    std::vector<uint8_t> b(n);
    for (uint8_t& v : b) v = (uint8_t)rng();
    if ((round & 1) && n >= 16) { /* past the first three checks */
      snap::put32(b.data(), snap::MAGIC);
      snap::put32(b.data() + 4, snap::VERSION);
      snap::put64(b.data() + 8, n);
      if ((round & 2) && n >= 56) { /* plausible fields, random counts */
        snap::put32(b.data() + 16, (uint32_t)(rng() % 8));
        snap::put32(b.data() + 20, 2 + (uint32_t)(rng() % 64));
        snap::put32(b.data() + 24, 2 + (uint32_t)(rng() % 64));
        snap::put32(b.data() + 28, (uint32_t)(rng() % 5));
        snap::put32(b.data() + 40, (uint32_t)(rng() % 2));
        snap::put32(b.data() + 44, (uint32_t)(rng() % 5));
        snap::put32(b.data() + 48, (round & 4) ? (uint32_t)rng() : (uint32_t)(rng() % 3));
        snap::put32(b.data() + 52, 0);
      }
    }
    snap::State out;
    if (decode_exact(b.data(), n, out) == snap::OK) consistent(out, n);
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("accum_snapshot_san: ok\n");
  return 0;
}
