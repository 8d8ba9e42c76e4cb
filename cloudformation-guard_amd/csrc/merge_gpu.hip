// Input-parameter merge on the device loader's arena (see merge_gpu.h).
//
// merge_into_last (doc_loader.cpp) is the specification: for document d with nn nodes at nbase[d]
// the tail starts at O = nn and holds, in this order,
//   [O, O + np)            the parameters' nodes, child / key-block / parent links moved by O
//   R = O + np             the merged root (the parameters' kind and location)
//   [E, E + n), E = R + 1  shallow copies of the parameters' root entries, then of the document's
//                          (n = both counts); the document's keys take the document root's
//                          location with the key-path flag
//   list roots:            two detached list parents, one per side
//   key-block roots:       the parameters' key block, then one key per document entry
// Work split: one wave per document, four waves per workgroup.  The workgroup stages the template
// (nodes, marks, sorted key ids: 48 bytes a node) in LDS once when it fits kLdsTemplate; a larger
// one is read in place through the same code (every wave reads the same lines, so they stay in L2).
// A lane moves 16 bytes at a time: half a node per lane, so a wave's stores into the tail are
// contiguous kilobytes.  The conflict check gives each lane one of the document's root entries, 64
// a round: a binary search of its key id in the template's sorted ids (ids are batch-wide interned,
// so equal ids are equal strings), and a ballot picks the first hit in the document's own order.
#include "merge_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <unordered_map>

#include "dev_cache.h"
#include "host_format.h"

namespace gg {
namespace {

#define MCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e_)); } while (0)

// LDS a workgroup spends on the template: a quarter of what it may address without opting in, so
// five workgroups (20 waves) share a CU's 160 KB; ~680 parameter nodes fit
constexpr uint32_t kLdsTemplate = 32u << 10;
constexpr uint32_t kMaxFails = 64;
// control block: [0] the lowest failing document, [1] failure records written, then the records
constexpr uint32_t kCtlWords = 4 + 4 * kMaxFails;

struct MergeArgs {
  MergeArena A;
  const uint32_t* tmpl;   // MergeTemplate::words
  uint32_t words;
  uint32_t np, root, kind, count, first, kblock, nkb, nkeys;
  uint32_t* ctl;
};

__device__ inline void put_node(DNode* dst, uint4 lo, uint4 hi) {
  uint4* p = (uint4*)dst;
  p[0] = lo;
  p[1] = hi;
}

// the template's node half `idx` (even: kind, count, a, b; odd: key_off, key_len, key_hash, parent)
// as it stands in a document whose tail starts at O
__device__ inline uint4 rebased(uint4 v, uint32_t idx, uint32_t O) {
  if (idx & 1u) {
    if (v.w != NONE) v.w += O;
  } else if (v.x == K_LIST || v.x == K_MAP) {
    v.z += O;
    if (v.x == K_MAP && v.w) v.w += O;
  }
  return v;
}

template <bool STAGED>
__global__ void __launch_bounds__(256) merge_params_kernel(MergeArgs M) {
  extern __shared__ uint4 staged[];
  if (STAGED) {
    for (uint32_t i = threadIdx.x; i < M.words / 4; i += blockDim.x) staged[i] = ((const uint4*)M.tmpl)[i];
    __syncthreads();
  }
  const uint32_t* T = STAGED ? (const uint32_t*)staged : M.tmpl;
  const uint4* TN = (const uint4*)T;
  const uint32_t np = M.np;
  const uint32_t *TL = T + 8ull * np, *TC = TL + np, *TKL = TC + np, *TKC = TKL + np, *KEYS = TKC + np;
  const MergeArena& A = M.A;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
  const bool is_map = M.kind == K_MAP, is_list = M.kind == K_LIST;
  for (uint32_t d = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; d < A.ndocs; d += waves) {
    const uint64_t nb = A.node_base[d];
    const uint32_t O = A.n_nodes[d];
    const uint32_t tail = (uint32_t)(A.node_base[d + 1] - nb) - O;
    if (!tail) continue;   // refused by the count pass: no nodes, no tail
    DNode* N = A.nodes + nb;
    // the whole tail as placeholders (the fix / verify pass's `dead` nodes): an unmerged document's
    auto kill = [&]() {
      for (uint32_t r = lane; r < tail; r += 64) {
        put_node(N + O + r, make_uint4(K_NULL, 0, 0, 0), make_uint4(NONE, 0, 0, NONE));
        const uint64_t g = nb + O + r;
        A.line[g] = 0; A.col[g] = 0; A.kline[g] = 0; A.kcol[g] = 0;
      }
    };
    auto fail = [&](uint32_t why, uint32_t aux, uint32_t len) {
      if (lane == 0) {
        // only a document below every failure seen so far can be the first: a handful of records
        const uint32_t old = atomicMin(&M.ctl[0], d);
        if (d < old) {
          const uint32_t slot = atomicAdd(&M.ctl[1], 1u);
          if (slot < kMaxFails) ((uint4*)(M.ctl + 4))[slot] = make_uint4(d, why, aux, len);
        }
      }
      kill();
    };
    if (A.doc_bad[d]) { kill(); continue; }   // refused after the count pass: the host builds it
    const uint4 r0 = ((const uint4*)N)[0];    // a device-loaded root is the document's node 0
    const uint32_t bkind = r0.x;
    const bool cont = bkind == K_MAP || bkind == K_LIST;
    const uint32_t bcount = cont ? r0.y : 0u, ba = cont ? r0.z : 0u;
    if (!((is_map || is_list) && bkind == M.kind)) { fail(MERGE_INCOMPATIBLE, bkind, 0); continue; }
    // the reservation is the host's sum over the count pass's root count: what the root says now must
    // be that count and its entries must lie inside the document, or nothing is written
    const uint32_t n = M.count + bcount;
    const uint64_t want = (uint64_t)np + 1 + n + (is_list ? 2u : 0u) + (is_map && M.kblock ? (uint64_t)M.nkb + bcount : 0u);
    if (want != tail || (uint64_t)ba + bcount > O) { fail(MERGE_LAYOUT, 0, 0); continue; }

    if (is_map) {
      bool conflict = false;
      uint32_t ckey = 0, clen = 0;
      for (uint32_t j0 = 0; j0 < bcount && !conflict; j0 += 64) {
        const uint32_t j = j0 + lane;
        bool hit = false;
        uint32_t kid = 0, klen = 0;
        if (j < bcount) {
          const uint4 kh = ((const uint4*)(N + ba + j))[1];
          kid = kh.z; klen = kh.y;
          uint32_t lo = 0, hi = M.nkeys;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (KEYS[mid] < kid) lo = mid + 1; else hi = mid;
          }
          hit = lo < M.nkeys && KEYS[lo] == kid;
        }
        const uint64_t m = __ballot(hit);
        if (m) {
          const int src = __ffsll((unsigned long long)m) - 1;
          ckey = __shfl(kid, src); clen = __shfl(klen, src);
          conflict = true;
        }
      }
      if (conflict) { fail(MERGE_DUPLICATE, ckey, clen); continue; }
    }

    // 1. the parameters' nodes and marks
    {
      uint4* dst = (uint4*)(N + O);
      for (uint32_t idx = lane; idx < 2 * np; idx += 64) dst[idx] = rebased(TN[idx], idx, O);
      const uint64_t g0 = nb + O;
      for (uint32_t i = lane; i < np; i += 64) {
        A.line[g0 + i] = TL[i]; A.col[g0 + i] = TC[i]; A.kline[g0 + i] = TKL[i]; A.kcol[g0 + i] = TKC[i];
      }
    }
    // 2. the merged root at the parameters' location
    const uint32_t R = O + np, E = R + 1, V = E + n;
    if (lane == 0) {
      put_node(N + R, make_uint4(M.kind, n, E, is_map && M.kblock ? V : 0u), make_uint4(NONE, 0, 0, NONE));
      A.line[nb + R] = TL[M.root]; A.col[nb + R] = TC[M.root]; A.kline[nb + R] = 0; A.kcol[nb + R] = 0;
    }
    // 3. its entries: the parameters', then the document's
    const uint32_t bl = A.line[nb] | kKeyPathExt, bc = A.col[nb];
    for (uint32_t j = lane; j < n; j += 64) {
      const bool mine = j < M.count;
      uint4 lo, hi;
      uint32_t l, c, kl, kc;
      if (mine) {
        const uint32_t s = M.first + j;
        lo = rebased(TN[2 * s], 0, O); hi = TN[2 * s + 1];
        l = TL[s]; c = TC[s]; kl = TKL[s]; kc = TKC[s];
      } else {
        const uint32_t s = ba + (j - M.count);
        lo = ((const uint4*)(N + s))[0]; hi = ((const uint4*)(N + s))[1];
        l = A.line[nb + s]; c = A.col[nb + s]; kl = bl; kc = bc;
      }
      if (is_map) hi.w = R;
      else { hi.w = mine ? V : V + 1; kl = 0; kc = 0; }
      put_node(N + E + j, lo, hi);
      const uint64_t g = nb + E + j;
      A.line[g] = l; A.col[g] = c; A.kline[g] = kl; A.kcol[g] = kc;
    }
    if (is_list) {
      // each side's copies hang under a detached list node, so every element keeps its own index
      if (lane < 2) {
        put_node(N + V + lane, make_uint4(K_LIST, lane ? bcount : M.count, lane ? E + M.count : E, 0), make_uint4(NONE, 0, 0, NONE));
        const uint64_t g = nb + V + lane;
        A.line[g] = 0; A.col[g] = 0; A.kline[g] = 0; A.kcol[g] = 0;
      }
    } else if (M.kblock) {
      // the merged keys: the parameters' block, then the document's keys as step 3 marked them
      const uint32_t nk = M.nkb + bcount;
      for (uint32_t j = lane; j < nk; j += 64) {
        uint4 hi;
        uint32_t kl, kc;
        if (j < M.nkb) { const uint32_t s = M.kblock + j; hi = TN[2 * s + 1]; kl = TKL[s]; kc = TKC[s]; }
        else { hi = ((const uint4*)(N + ba + (j - M.nkb)))[1]; kl = bl; kc = bc; }
        hi.w = R;
        put_node(N + V + j, make_uint4(K_NULL, nk, 0, 0), hi);
        const uint64_t g = nb + V + j;
        A.line[g] = 0; A.col[g] = 0; A.kline[g] = kl; A.kcol[g] = kc;
      }
    }
  }
}

__global__ void __launch_bounds__(256) root_counts_kernel(const uint16_t* counts, const uint64_t* off, const uint32_t* n_cont,
                                                          const uint32_t* doc_bad, uint32_t ndocs, uint32_t* out) {
  for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < ndocs; d += gridDim.x * blockDim.x)
    out[d] = doc_bad[d] ? NONE : (n_cont[d] ? (uint32_t)counts[off[d] >> 1] : 0u);   // the root is container 0; a scalar root has none
}

template <typename T>
struct Dev {
  T* p = nullptr;
  explicit Dev(size_t n) { MCHK(dev_alloc(&p, std::max<size_t>(n, 1) * sizeof(T))); }
  ~Dev() { dev_free_on(p, nullptr); }
};

}  // namespace

void merge_shape(const DocBatch& P, MergeTemplate& t) {
  const uint64_t pbase = P.base[0];
  const uint64_t pend = P.base.size() > 1 ? P.base[1] : P.nodes.size();
  const uint32_t np = (uint32_t)(pend - pbase);
  const DNode& A = P.nodes[pbase + P.roots[0]];
  t.np = np; t.root = P.roots[0]; t.kind = A.kind;
  const bool cont = A.kind == K_MAP || A.kind == K_LIST;
  t.count = cont ? A.count : 0; t.first = cont ? A.a : 0;
  t.kblock = A.kind == K_MAP ? A.b : 0;
  t.nkb = t.kblock ? P.nodes[pbase + t.kblock].count : 0;
  t.nkeys = A.kind == K_MAP ? A.count : 0;
  if ((uint64_t)t.first + t.count > np || (uint64_t)t.kblock + t.nkb > np || t.root >= np)
    throw std::runtime_error("input parameters: the root's entries lie outside its document");
}

void merge_template(DocBatch& b, const DocBatch& P, MergeTemplate& t) {
  const uint64_t pbase = P.base[0];
  const uint32_t np = t.np;
  t.words.assign(((size_t)12 * np + t.nkeys + 3) & ~(size_t)3, 0);
  std::unordered_map<uint32_t, uint32_t> sid;   // P string id -> b string id
  auto str_id = [&](uint32_t off, uint32_t len) {
    auto it = sid.find(off);
    if (it != sid.end()) return it->second;
    const uint32_t id = b.intern(P.bytes.data() + off, len, fnv1a(P.bytes.data() + off, len));
    sid[off] = id;
    return id;
  };
  uint32_t* W = t.words.data();
  for (uint32_t i = 0; i < np; i++) {
    DNode n = P.nodes[pbase + i];
    if (n.kind == K_STRING || n.kind == K_REGEX) { n.a = str_id(n.a, n.count); n.b = n.a; }
    if (n.key_off != NONE) { n.key_off = str_id(n.key_off, n.key_len); n.key_hash = n.key_off; }
    memcpy(W + 8ull * i, &n, sizeof n);
    W[8ull * np + i] = P.line[pbase + i]; W[9ull * np + i] = P.col[pbase + i];
    W[10ull * np + i] = P.kline[pbase + i]; W[11ull * np + i] = P.kcol[pbase + i];
  }
  uint32_t* keys = W + 12ull * np;
  for (uint32_t j = 0; j < t.nkeys; j++) keys[j] = W[8ull * (t.first + j) + 6];   // key_hash: the key's id
  std::sort(keys, keys + t.nkeys);
}

void merge_root_counts(const uint16_t* counts, const uint64_t* off, const uint32_t* n_cont, const uint32_t* doc_bad,
                       uint32_t ndocs, uint32_t* out) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)ndocs + 255) / 256, 65536ull);
  hipLaunchKernelGGL(root_counts_kernel, dim3(grid), dim3(256), 0, 0, counts, off, n_cont, doc_bad, ndocs, out);
  MCHK(hipGetLastError());
}

float merge_params_device(const MergeArena& A, const MergeTemplate& t, MergeFail& fail) {
  fail = MergeFail{};
  if (!A.ndocs) return 0;
  Dev<uint32_t> d_tmpl(t.words.size()), d_ctl(kCtlWords);
  MCHK(hipMemcpy(d_tmpl.p, t.words.data(), t.words.size() * 4, hipMemcpyHostToDevice));
  std::vector<uint32_t> ctl(kCtlWords, 0);
  ctl[0] = NONE;
  MCHK(hipMemcpy(d_ctl.p, ctl.data(), kCtlWords * 4, hipMemcpyHostToDevice));
  MergeArgs M{};
  M.A = A; M.tmpl = d_tmpl.p; M.words = (uint32_t)t.words.size();
  M.np = t.np; M.root = t.root; M.kind = t.kind; M.count = t.count; M.first = t.first; M.kblock = t.kblock; M.nkb = t.nkb;
  M.nkeys = t.nkeys; M.ctl = d_ctl.p;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)A.ndocs + 3) / 4, 65536ull);   // a wave per document
  const size_t bytes = t.words.size() * 4;
  hipEvent_t e0, e1;
  MCHK(hipEventCreate(&e0));
  MCHK(hipEventCreate(&e1));
  MCHK(hipEventRecord(e0));
  if (bytes <= kLdsTemplate) hipLaunchKernelGGL(merge_params_kernel<true>, dim3(grid), dim3(256), bytes, 0, M);
  else hipLaunchKernelGGL(merge_params_kernel<false>, dim3(grid), dim3(256), 0, 0, M);
  MCHK(hipGetLastError());
  MCHK(hipEventRecord(e1));
  MCHK(hipEventSynchronize(e1));
  float ms = 0;
  MCHK(hipEventElapsedTime(&ms, e0, e1));
  MCHK(hipEventDestroy(e0));
  MCHK(hipEventDestroy(e1));
  MCHK(hipMemcpy(ctl.data(), d_ctl.p, kCtlWords * 4, hipMemcpyDeviceToHost));
  if (ctl[0] != NONE) {
    fail.doc = ctl[0];
    fail.lost = true;
    for (uint32_t k = 0; k < std::min(ctl[1], kMaxFails); k++) {
      const uint32_t* r = &ctl[4 + 4 * k];
      if (r[0] == fail.doc) { fail.why = r[1]; fail.aux = r[2]; fail.len = r[3]; fail.lost = false; }
    }
  }
  return ms;
}

void merge_fail_error(const DocBatch& b, const MergeTemplate& t, const MergeFail& f, LoadError& err) {
  if (f.why == MERGE_DUPLICATE) {
    err.kind = "MultipleValues";
    err.msg = "Key " + std::string(b.bytes.data() + f.aux, f.len) + ", already exists in map";
  } else {
    err.kind = "IncompatibleError";
    err.msg = std::string("Types are not compatible for merges ") + merge_type_info(t.kind) + ", " + merge_type_info(f.aux);
  }
}

}  // namespace gg
