// Appending a device-loaded batch to a session that already holds documents (append_gpu.hip).
//
// The device loader interns a batch's strings in a fingerprint table of its own (json_gpu.hip).  To
// append, the table is seeded with every string the session's pool already holds, under its existing
// id, before the new batch's emit pass: the new batch's occurrences of those strings resolve to the old
// ids, new strings take pool space after the old pool, and the loader's table-full doubling and its
// byte-for-byte verify pass treat old and new strings alike.  Node links are document-relative and string
// ids pool-wide already, so the new batch's columns join the session's by plain copies (capi.cpp).
#pragma once
#include <stdint.h>

#include "guard_types.h"

namespace gg {

// towner of a seeded slot: no document owns it, its bytes are in the pool already (json_own_kernel skips it)
constexpr unsigned long long kSeededOwner = ~0ull;

#ifdef __HIPCC__
// The intern table's probe start (intern_mix64, the one definition: json_gpu.hip intern_slot and the
// seeding kernel must probe alike) and its key for a string whose decoded bytes hash to `h` (FNV-1a over little-endian 4-byte
// words, the last partial word zero-extended, json_gpu.hip string_occurrence) and are `len` long.
__device__ inline uint64_t intern_mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
__device__ inline uint64_t intern_key64(uint64_t h, uint32_t len, uint64_t fp_mask) {
  return (intern_mix64(h ^ ((uint64_t)len * 0x9E3779B97F4A7C15ull)) & fp_mask) | 1ull;
}
#endif

// the loader's intern table (device pointers), as json_gpu.hip JArgs holds it
struct SeedTable {
  unsigned long long* tkey;
  uint32_t* tlen;
  unsigned long long* towner;
  uint32_t* tid;
  uint64_t tmask;
  uint64_t fp_mask;
  uint32_t* bad;        // batch-wide refusal word; `bad_table` is stored there when a probe run finds no slot
  uint32_t bad_table;
};

// Inserts the n strings pool[off[i] .. off[i] + len[i]) (device pointers; off ascending, 16-byte
// aligned, strings zero padded to 16 bytes) under id off[i].  Null stream, not waited for.
void append_seed_table(const SeedTable& T, const uint8_t* pool, const uint32_t* off, const uint32_t* len, uint32_t n);

}  // namespace gg
