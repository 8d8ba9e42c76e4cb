// GPU document loader: strict-JSON documents -> the columnar node arena,
// parsed on the MI355X: a lane per document, or a workgroup per document for large ones.  Produces exactly the arena the host JSON fast path builds
// (doc_loader.cpp load_json_fast: same node layout, marks and scalar typing), with string ids
// interned batch-wide on the device.  Replaces, for JSON input, the reference's
// Loader::load + PathAwareValue::try_from (guard/src/rules/libyaml/loader.rs:31-195,
// guard/src/rules/path_value.rs:414-478).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "append_gpu.h"
#include "doc_loader.h"

namespace gg {

struct GpuLoadStats {
  double kernel_ms = 0;        // parse + intern kernels (HIP events)
  double h2d_ms = 0, d2h_ms = 0;
  uint64_t text_bytes = 0, nodes = 0, distinct_strings = 0, pool_bytes = 0;
  uint32_t table_retries = 0;   // intern-table doublings
  uint64_t refused_docs = 0;    // documents outside the device subset, built by the host loader
  uint64_t coop_docs = 0;       // documents the cooperative kernels parsed (a workgroup per document)
  uint64_t seeded_strings = 0;  // strings the seeding kernel inserted (0: the resident table was carried, or nothing to seed)
  uint64_t index_strings = 0;   // strings the load added, the ones the host index adopts
};

// Routing: a document of at least `coop_min` bytes is parsed cooperatively instead of by one lane: one that
// opens with { or [ after leading whitespace by a workgroup (json_coop.inc), any other one -- block-style
// YAML -- by a workgroup's line index and a lane per segment (yaml_coop.inc; *yaml is set then).
// gpu_json_coop_min() is GG_JSON_COOP_MIN (default 65536; 0 sends every document that way), the one
// threshold for both formats.  GG_YAML_COOP=0|1 turns only the YAML path off or on; GG_YAML_DEVICE=0 turns
// every YAML path off; gpu_yaml_coop_on() reads the two switches, once per load.
uint64_t gpu_json_coop_min();
bool gpu_yaml_coop_on();
bool gpu_json_coop_doc(const char* text, size_t len, uint64_t coop_min, bool yaml_coop, bool* yaml = nullptr);

// Appends `n` documents (texts[i] of lens[i] bytes, named names[i]) to the EMPTY batch `out`.
// A document outside the subset the device parser proves identical to the host loader (libyaml-only
// syntax, duplicate keys, nesting past 64, a float beyond the exact fast path, a raw character libyaml
// reads specially) is refused on its own: with `refused` non-null its index is appended there and
// `out` holds an empty placeholder for it (the caller builds it with the host loader); with
// `refused` null the whole batch is refused.  Returns false with `why` set when the batch is refused
// (batch-wide limits, or strict mode); `out` is then unchanged.  With `keep_nodes` non-null the
// device copy of out.nodes (dev_alloc'ed, out.nodes.size() DNodes) is handed to the caller, who
// frees it with dev_free (dev_cache.h): the session packs its arena from it instead of uploading the nodes again.
//
// With `resident` non-null as well (and no document refused) the per-node columns stay in HBM: out.nodes,
// line, col, kline, kcol are left EMPTY, the device copies are handed over in *resident (node count
// st.nodes; the caller owns every pointer, dev_free), and only the pool, the intern index, bases and names
// reach the host.  The session copies the columns down when a host consumer first needs them
// (capi.cpp ensure_host_arena); a job whose reports are all rendered on the device never does.
struct ResidentArena {
  uint32_t* line = nullptr;    // per node mark
  uint32_t* col = nullptr;
  uint32_t* kline = nullptr;   // per map-entry node: its key's mark
  uint32_t* kcol = nullptr;
  uint64_t nodes = 0;          // 0: the columns came down to the host (out is complete)
};
//
// With `merge` (and merge->params) the input parameters' document 0 is merged into every accepted document
// on the device (merge_gpu.h): each document's nodes are followed by the tail merge_into_last appends, its
// root is the merged root, and the arena is the one the host loader + merge_into_last build.  A refused
// document keeps its placeholder, unmerged: the caller merges the one it builds.  When a document's
// merge fails the load still returns true with the first such document (in document order) in
// merge->fail_doc and the reference's error in merge->fail; the batch is then not to be evaluated.
//
// With `append_to` (a batch that holds documents already; `out` is still a fresh batch) the load is one that
// appends: every string of append_to's pool is seeded into the intern table under its id before the
// new documents intern (append_gpu.h), so out.bytes opens with append_to's pool byte for byte, a string the
// two share keeps its id, new strings follow, and out's index covers both.  st.distinct_strings and
// st.pool_bytes count what the load added.  out's nodes, bases and roots are its own documents' only: the
// caller puts them behind append_to's.
//
// With `intern` as well the loader's interning state stays in HBM across loads (append_gpu.h InternResident).
// intern->from, the state the last load left for append_to (the caller checks that append_to's pool and
// index are still the ones it was left for), replaces the seeding: the working table is carried from it on
// the device (intern_carry) before every run of the emit pass, the working pool is its block when that has
// room and a larger block with the old bytes copied device to device otherwise, and nothing of append_to's
// strings is listed, sorted or sent.  The passes never write into from's table, nor below its pool's
// cursor.  intern->next receives the state after this load (slots 0: none -- a document was refused to the
// host or the parameter merge added strings on the host, so the device no longer holds every string);
// next.pool may be from->pool.  The caller owns next: it commits it with the batch or frees it
// (intern_resident_free).  With intern->in_place set on return, out.bytes holds only the bytes the load added
// (pool offsets from append_to's size on) and out's index is empty: add_off / add_len list the added
// strings and the caller extends append_to's own pool and index with them.
struct InternCarry {
  const InternResident* from = nullptr;
  InternResident next;
  bool in_place = false;
  std::vector<uint32_t> add_off, add_len;
};
// hands r's blocks back to the block cache (dev_free); a pool block it shares with `sharing` stays
void intern_resident_free(InternResident& r, const InternResident* sharing = nullptr);

struct ParamMerge {
  const DocBatch* params = nullptr;
  uint32_t fail_doc = NONE;
  LoadError fail;
};
bool gpu_load_json(DocBatch& out, const char* const* texts, const size_t* lens, const std::vector<std::string>& names,
                   size_t n, GpuLoadStats& st, std::string& why, std::vector<uint32_t>* refused = nullptr,
                   void** keep_nodes = nullptr, ResidentArena* resident = nullptr, ParamMerge* merge = nullptr,
                   const DocBatch* append_to = nullptr, InternCarry* intern = nullptr);

}  // namespace gg
