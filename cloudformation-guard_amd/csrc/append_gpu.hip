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

uint32_t grid_of(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 65536ull); }

}  // namespace

void append_seed_table(const SeedTable& T, const uint8_t* pool, const uint32_t* off, const uint32_t* len, uint32_t n) {
  if (!n) return;
  hipLaunchKernelGGL(append_seed_kernel, dim3(grid_of(n)), dim3(256), 0, 0, T, pool, off, len, n);
  ACHK(hipGetLastError());
}

}  // namespace gg
