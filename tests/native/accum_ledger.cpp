/* csrc/accum_ledger.h behind a C interface for tests/test_accum_ledger.py: one call per member function. */
#include "accum_ledger.h"

using hrt::AccumLedger;
using hrt::SampleRange;

extern "C" {

void* ledger_new(uint32_t n_tiles) { return new AccumLedger(n_tiles); }
void ledger_free(void* l) { delete static_cast<AccumLedger*>(l); }

int ledger_uniform(const void* l) { return static_cast<const AccumLedger*>(l)->uniform(); }
int ledger_empty(const void* l) { return static_cast<const AccumLedger*>(l)->empty(); }
uint64_t ledger_samples(const void* l, uint32_t t) { return static_cast<const AccumLedger*>(l)->samples(t); }
uint64_t ledger_chunks(const void* l, uint32_t t) { return static_cast<const AccumLedger*>(l)->chunks(t); }
/* the shared range list as (begin, end) pairs into out[2 * cap]; returns its length, or -1: the tiles differ */
int32_t ledger_ranges(const void* l, uint64_t* out, uint32_t cap) {
  const std::vector<SampleRange>* held = static_cast<const AccumLedger*>(l)->ranges();
  if (!held) return -1;
  const std::vector<SampleRange>& r = *held;
  for (size_t i = 0; i < r.size() && i < cap; i++) out[2 * i] = r[i].begin, out[2 * i + 1] = r[i].end;
  return (int32_t)r.size();
}

/* idx null: every tile.  may_add returns AccumLedger::Refusal (0 addable, 1 bad range, 2 overlap) */
int ledger_may_add(const void* l, uint64_t begin, uint64_t end, const uint32_t* idx, uint32_t n) {
  return static_cast<const AccumLedger*>(l)->may_add(SampleRange{begin, end}, idx, n);
}
void ledger_record(void* l, uint64_t begin, uint64_t end, uint64_t k, const uint32_t* idx, uint32_t n) {
  static_cast<AccumLedger*>(l)->record(SampleRange{begin, end}, k, idx, n);
}
void ledger_merge(void* dst, const void* src) { static_cast<AccumLedger*>(dst)->merge(*static_cast<const AccumLedger*>(src)); }
void ledger_clear(void* l) { static_cast<AccumLedger*>(l)->clear(); }

}  // extern "C"
