// Device append (append_gpu.h): the intern table seeded from the session's pool.
#include "append_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

namespace gg {
namespace {

#define ACHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e_)); } while (0)

// One wave per run of 64 strings, a lane per string.  The list is ascending by pool offset and the
// strings are short (keys, type names: mostly one 16-byte pool slot), so a wave's first loads cover one
// contiguous stretch of the pool; a longer string's lane goes on in 16-byte steps.  The fingerprint is
// the loader's: FNV-1a over the string's little-endian words, then the partial last word (zero when the
// length is a multiple of four) -- a serial recurrence per string, which is why a string is not split
// across lanes.  The insert is intern_slot's (json_gpu.hip): CAS on the key, the winner fills the slot.
// A slot that already holds the key belongs to another old string with the same (narrowed) fingerprint:
// it keeps the first one's id, and the verify pass refuses every new document that uses the second.
__global__ void __launch_bounds__(256) append_seed_kernel(SeedTable T, const uint8_t* __restrict__ pool,
                                                          const uint32_t* __restrict__ off, const uint32_t* __restrict__ len, uint32_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t o = off[i], L = len[i];
    const uint4* p = (const uint4*)(pool + o);   // ids are 16-byte pool slots
    uint64_t h = 0xcbf29ce484222325ull;
    uint32_t last = 0;
    for (uint32_t done = 0; done < L; done += 16, p++) {
      const uint4 v = *p;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t at = done + 4 * k;
        if (at + 4 <= L) h = (h ^ w[k]) * 0x100000001b3ull;
        else if (at < L) last = w[k] & ((1u << (8u * (L - at))) - 1u);
      }
    }
    h = (h ^ last) * 0x100000001b3ull;
    const unsigned long long key = intern_key64(h, L, T.fp_mask);
    uint64_t idx = intern_mix64(key) & T.tmask;
    bool placed = false;
    for (uint32_t probe = 0; probe < 1024 && !placed; probe++) {
      const unsigned long long k = T.tkey[idx];
      if (k == key) { placed = true; break; }
      if (k == 0) {
        const unsigned long long old = atomicCAS(&T.tkey[idx], 0ull, key);
        if (old == 0) {
          T.tlen[idx] = L;
          T.towner[idx] = kSeededOwner;
          T.tid[idx] = o;
          placed = true;
          break;
        }
        if (old == key) { placed = true; break; }
      }
      idx = (idx + 1) & T.tmask;
    }
    if (!placed) atomicCAS(T.bad, 0u, T.bad_table);   // the loader doubles the table and runs again
  }
}

// Four consecutive slots of a table per lane: two 16-byte loads of keys, one of lengths, one of ids
// (tables hold a power of two of at least 2^16 slots, in 256-byte aligned blocks).
struct Slots4 {
  unsigned long long key[4];
  uint32_t len[4], id[4];
};
__device__ inline Slots4 load_slots4(const unsigned long long* __restrict__ tkey, const uint32_t* __restrict__ tlen,
                                     const uint32_t* __restrict__ tid, uint64_t q) {
  const ulonglong2 k01 = ((const ulonglong2*)tkey)[2 * q], k23 = ((const ulonglong2*)tkey)[2 * q + 1];
  const uint4 L = ((const uint4*)tlen)[q], I = ((const uint4*)tid)[q];
  return Slots4{{k01.x, k01.y, k23.x, k23.y}, {L.x, L.y, L.z, L.w}, {I.x, I.y, I.z, I.w}};
}

// The resident table into a load's working table, a lane per four slots.  The same size: the slots are
// copied where they are, 16 bytes a store, and the owners written beside them (seeded where the slot is
// occupied).  REHASH, into a larger table whose keys are zero: each occupied slot probes from
// intern_mix64(key) as intern_slot does and takes the first free slot by CAS; the keys of one table are
// distinct, so a CAS that loses lost to another key and the probe goes on.  The lanes of a wave scatter
// over the new table (the mix decorrelates neighbours), which the loads' 16-byte reads pay for: a slot is
// 20 bytes read against three stores.
template <bool REHASH>
__global__ void __launch_bounds__(256) intern_carry_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ slen,
                                                           const uint32_t* __restrict__ sid, uint64_t squads, SeedTable T) {
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < squads; q += (uint64_t)gridDim.x * blockDim.x) {
    const Slots4 s = load_slots4(skey, slen, sid, q);
    if (!REHASH) {
      ((ulonglong2*)T.tkey)[2 * q] = make_ulonglong2(s.key[0], s.key[1]);
      ((ulonglong2*)T.tkey)[2 * q + 1] = make_ulonglong2(s.key[2], s.key[3]);
      ((uint4*)T.tlen)[q] = make_uint4(s.len[0], s.len[1], s.len[2], s.len[3]);
      ((uint4*)T.tid)[q] = make_uint4(s.id[0], s.id[1], s.id[2], s.id[3]);
      ((ulonglong2*)T.towner)[2 * q] = make_ulonglong2(s.key[0] ? kSeededOwner : 0ull, s.key[1] ? kSeededOwner : 0ull);
      ((ulonglong2*)T.towner)[2 * q + 1] = make_ulonglong2(s.key[2] ? kSeededOwner : 0ull, s.key[3] ? kSeededOwner : 0ull);
      continue;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const unsigned long long key = s.key[j];
      if (!key) continue;
      uint64_t idx = intern_mix64(key) & T.tmask;
      bool placed = false;
      for (uint32_t probe = 0; probe < 1024; probe++) {
        if (T.tkey[idx] == 0 && atomicCAS(&T.tkey[idx], 0ull, key) == 0) {
          T.tlen[idx] = s.len[j];
          T.towner[idx] = kSeededOwner;
          T.tid[idx] = s.id[j];
          placed = true;
          break;
        }
        idx = (idx + 1) & T.tmask;
      }
      if (!placed) atomicCAS(T.bad, 0u, T.bad_table);   // the loader doubles the table and runs again
    }
  }
}

// The strings a load added, out of the table: one workgroup per 1024 slots, a lane per four.  A slot is
// selected when it is occupied and its id is at or behind the threshold.  Each of a lane's four slots is
// one ballot; a lane's place in its wave is the selected slots of the lanes below it (popcounts of the four
// ballots under its lane mask) plus its own earlier ones, so a wave writes in table order.  The waves'
// totals meet in LDS, wave 0's first lane scans the four and takes the workgroup's base with the one
// atomic, and every lane stores its pairs at base + wave offset + place.
__global__ void __launch_bounds__(256) intern_compact_kernel(const unsigned long long* __restrict__ tkey, const uint32_t* __restrict__ tlen,
                                                             const uint32_t* __restrict__ tid, uint64_t quads, uint32_t threshold,
                                                             uint32_t* __restrict__ off, uint32_t* __restrict__ len,
                                                             uint32_t* __restrict__ count, uint32_t cap) {
  __shared__ uint32_t wave_total[4];
  __shared__ uint32_t wave_base[4];
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  Slots4 s{};
  if (q < quads) s = load_slots4(tkey, tlen, tid, q);
  const unsigned long long below = (1ull << lane) - 1ull;
  bool sel[4];
  uint32_t place = 0, total = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    sel[j] = q < quads && s.key[j] != 0 && s.id[j] >= threshold;
    const unsigned long long b = __ballot(sel[j]);
    place += (uint32_t)__popcll(b & below);
    total += (uint32_t)__popcll(b);
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < 4; w++) { wave_base[w] = sum; sum += wave_total[w]; }
    const uint32_t base = sum ? atomicAdd(count, sum) : 0u;
    for (uint32_t w = 0; w < 4; w++) wave_base[w] += base;
  }
  __syncthreads();
  uint32_t at = wave_base[wave] + place;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    if (!sel[j]) continue;
    if (at < cap) { off[at] = s.id[j]; len[at] = s.len[j]; }
    at++;
  }
}

uint32_t grid_of(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 65536ull); }

}  // namespace

void append_seed_table(const SeedTable& T, const uint8_t* pool, const uint32_t* off, const uint32_t* len, uint32_t n) {
  if (!n) return;
  hipLaunchKernelGGL(append_seed_kernel, dim3(grid_of(n)), dim3(256), 0, 0, T, pool, off, len, n);
  ACHK(hipGetLastError());
}

void intern_carry(const InternResident& from, const SeedTable& to) {
  const uint64_t quads = from.slots / 4;
  if (!quads) return;
  if (to.tmask + 1 < from.slots) throw std::runtime_error("intern carry: the working table is smaller than the resident one");
  if (to.tmask + 1 == from.slots)
    hipLaunchKernelGGL(intern_carry_kernel<false>, dim3(grid_of(quads)), dim3(256), 0, 0, from.tkey, from.tlen, from.tid, quads, to);
  else
    hipLaunchKernelGGL(intern_carry_kernel<true>, dim3(grid_of(quads)), dim3(256), 0, 0, from.tkey, from.tlen, from.tid, quads, to);
  ACHK(hipGetLastError());
}

void intern_compact(const SeedTable& T, uint32_t threshold, uint32_t* off, uint32_t* len, uint32_t* count, uint32_t cap) {
  const uint64_t quads = (T.tmask + 1) / 4;
  ACHK(hipMemsetAsync(count, 0, 4, nullptr));
  // a workgroup per 1024 slots: 2^28 slots, the loader's largest table, are 262144 workgroups
  hipLaunchKernelGGL(intern_compact_kernel, dim3((uint32_t)((quads + 255) / 256)), dim3(256), 0, 0, T.tkey, T.tlen, T.tid, quads, threshold,
                     off, len, count, cap);
  ACHK(hipGetLastError());
}

}  // namespace gg
