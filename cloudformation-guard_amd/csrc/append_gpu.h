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

// ---- the intern state a session keeps in HBM between device loads ------------------------------------
// The table a load leaves (keys, lengths, ids; the owners are that load's document indices and mean
// nothing to the next one) and the pool with its cursor.  The next load carries the table into its working
// table instead of seeding it from the host, and only the strings it adds come back to the host.  Blocks
// from dev_alloc; the pool block holds pool_cap + 16 bytes, zero past pool_used only once a load has
// cleared it.
struct InternResident {
  unsigned long long* tkey = nullptr;
  uint32_t* tlen = nullptr;
  uint32_t* tid = nullptr;
  uint64_t slots = 0;          // a power of two, at least 2^16; 0: no state
  uint8_t* pool = nullptr;
  uint64_t pool_cap = 0;
  uint64_t pool_used = 0;      // the cursor: equals the host pool's size while the state is valid
  uint64_t fp_mask = 0;        // the keys were derived under this mask
  uint64_t strings = 0;        // occupied slots (sizes the next working table)
  uint64_t host_strings = 0;   // the host index's string count when the state was left
};

// Builds the working table `to` from the resident one: every occupied slot keeps its key, length and id and
// becomes a seeded slot (kSeededOwner).  The same size: a straight copy of the slots.  A larger `to` (its
// keys zeroed by the caller): every occupied slot is inserted with intern_slot's probe sequence -- the
// probe start is a function of the stored key, so no pool byte is read; a probe run that finds no slot
// stores to.bad_table in *to.bad.  Null stream, not waited for.
void intern_carry(const InternResident& from, const SeedTable& to);

// The occupied slots of T whose id is at or behind `threshold` (the pool size before the load: the strings
// the load added), densely as (off[i], len[i]) pairs; *count (device, zeroed here) receives their number.
// At most `cap` pairs are written, the count is the true one.  Table order inside a workgroup's 1024 slots,
// workgroups in the order they finish.  Null stream, not waited for.
void intern_compact(const SeedTable& T, uint32_t threshold, uint32_t* off, uint32_t* len, uint32_t* count, uint32_t cap);

}  // namespace gg
