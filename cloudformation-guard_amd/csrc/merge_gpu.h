// `validate -i` on the device loader: PathAwareValue::merge (path_value.rs:889-919) of the input
// parameters into every document of a device-loaded batch, restating merge_into_last
// (doc_loader.cpp) as one kernel over the loader's unpacked arena (merge_gpu.hip).
//
// The loader reserves, after each accepted document's nodes, the tail merge_into_last appends --
// the parameters' nodes, the merged root, the shallow entry copies, the two detached list parents of
// a list root, the key block of a root that carries one -- and the kernel fills it, so the arena is
// the host path's node for node and a resident arena stays resident.
#pragma once
#include <stdint.h>

#include <vector>

#include "doc_loader.h"

namespace gg {

// The merged parameter document, ready for the device: string ids interned into the batch's pool,
// links still relative to the parameters' own first node (the kernel rebases them per document).
struct MergeTemplate {
  // one upload: np nodes (8 words each), then the line, col, kline, kcol columns (np words each),
  // then the root entries' key ids in ascending order (count words, map roots only), padded to 16 bytes
  std::vector<uint32_t> words;
  uint32_t np = 0;       // nodes
  uint32_t root = 0;     // the parameters' root node
  uint32_t kind = 0;     // its kind
  uint32_t count = 0;    // its entries ...
  uint32_t first = 0;    // ... and the first of them
  uint32_t kblock = 0;   // its key block (a map with a repeated key), 0 = none
  uint32_t nkb = 0;      // keys in that block
  uint32_t nkeys = 0;    // sorted key ids (count for a map root, else 0)
  // nodes the merge appends to a document whose root has `children` entries
  uint64_t tail(uint32_t children) const {
    return (uint64_t)np + 1 + count + children + (kind == K_LIST ? 2u : 0u) + (kind == K_MAP && kblock ? (uint64_t)nkb + children : 0u);
  }
};

// The shape of P's document 0 (everything but `words`): what the tail reservation needs, before the
// batch's pool exists on the host.
void merge_shape(const DocBatch& P, MergeTemplate& t);
// Fills `words` for a shaped template, interning P's strings into b's pool (new strings append).
void merge_template(DocBatch& b, const DocBatch& P, MergeTemplate& t);

enum : uint32_t { MERGE_INCOMPATIBLE = 1, MERGE_DUPLICATE = 2, MERGE_LAYOUT = 3 };
// the first failing document in document order (doc == NONE: every document merged)
struct MergeFail {
  uint32_t doc = NONE;
  uint32_t why = 0;    // MERGE_*
  uint32_t aux = 0;    // INCOMPATIBLE: the document root's kind; DUPLICATE: the key's string id
  uint32_t len = 0;    // DUPLICATE: the key's length
  bool lost = false;   // more failures than the error array holds and the first one's record is not among them
};

// the unpacked arena of a device load (device pointers; node_base has ndocs + 1 entries)
struct MergeArena {
  DNode* nodes;
  uint32_t *line, *col, *kline, *kcol;
  const uint64_t* node_base;
  const uint32_t* n_nodes;    // per document: its own nodes (the tail starts there)
  const uint32_t* doc_bad;    // per document: refused (its tail becomes placeholders)
  uint32_t ndocs;
};

// root child count of every document after the count pass (NONE for a refused document): counts is
// the pass's 16-bit container counts, a document's first container at off[d] / 2
void merge_root_counts(const uint16_t* counts, const uint64_t* off, const uint32_t* n_cont, const uint32_t* doc_bad,
                       uint32_t ndocs, uint32_t* out);

// Runs the merge on the null stream and waits for it; returns the kernel's time in ms.
float merge_params_device(const MergeArena& A, const MergeTemplate& t, MergeFail& fail);

// the reference's error for `f` (kind MultipleValues / IncompatibleError), as merge_into_last words it
void merge_fail_error(const DocBatch& b, const MergeTemplate& t, const MergeFail& f, LoadError& err);

}  // namespace gg
