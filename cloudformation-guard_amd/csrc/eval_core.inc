// Evaluator core, compiled three times by eval_kernel.hip: GG_LANE=0 (one tile per wavefront,
// all lanes in lock-step on identical state), GG_LANE=1 (one tile per lane) and GG_LANE=0 with
// GG_VERBOSE=1 (wave mode recording the whole EventRecord tree for guard-ffi's verbose output:
// nothing suppressed or rolled back, no shortcut that skips an evaluation the reference records).
#if defined(GG_VERBOSE) && GG_VERBOSE
static constexpr bool VB = true;
#else
static constexpr bool VB = false;
#endif
static const uint32_t SYN_BIT = 0x40000000u;
static const uint32_t KEY_BIT = 0x20000000u;
#if GG_LANE
// lane mode: one tile per lane, 64 KB heap per lane; tiles that outgrow it are re-run in wave mode
static const uint32_t FRAMES_BYTES = 4096;
static const uint32_t RECS_BYTES = 24576;   // default record staging (LaunchArgs::lane_recs_bytes may enlarge it)
#else
// wave mode: frame and record regions are per launch (LaunchArgs::wave_frames_bytes / _recs_bytes)
#endif

enum FrameKind : uint32_t { F_ROOT = 0, F_BLOCK = 1, F_VALUE = 2, F_PARAM = 3 };

struct Frame {
  uint32_t kind, parent, root, block;
  uint32_t cache;   // persist offset of per-let cache (16 B each: state, off, n, pad)
  uint32_t call;    // F_PARAM: param clause id
  uint32_t params;  // F_PARAM: persist offset of per-param views (8 B each: off, n)
  uint32_t prule;   // F_PARAM: param rule id
};

struct View { uint32_t off, n; };

// Program references.  Lane mode runs only programs staged in LDS (eval_kernel.hip hands the
// others to wave mode), so every program array but the regex DFA tables is read with ds_read
// through an LDS-typed pointer; wave mode keeps generic pointers (its program may be in HBM).
#undef PG
#undef PROG
#if GG_LANE
// The workgroup's LDS-staged rules program (eval_kernel.hip stage_program fills it): lane-mode
// program reads address it directly, a fixed LDS address, instead of first loading a pointer.
__shared__ DevProg g_prog;
#define PROG(c) g_prog
#else
#define PROG(c) (*(c).P)
#endif
#if GG_LANE && defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) const DevProg* ProgRef;
#define PG(c, f) ((__attribute__((address_space(3))) const std::remove_pointer_t<decltype(DevProg::f)>*)(g_prog.f))
#elif GG_LANE
typedef const DevProg* ProgRef;
#define PG(c, f) (g_prog.f)   // host pass of this translation unit: parsed, never run
#else
typedef const DevProg* ProgRef;
#define PG(c, f) ((c).P->f)
#endif

#if GG_LANE
// What every lane of a wave shares, once per wave in LDS: the interleaved heap region, the arena
// bases and the heap layout.  Per-lane state (Ctx, 64 copies per wave) keeps only per-tile values,
// so the wave's LDS footprint -- which bounds how many waves a CU holds -- stays small.
struct WaveConst {
  uint8_t* heap;         // the wave's 64 interleaved lane heaps
  const DNodeP* nodes;   // packed arena (DevBatch::nodes)
  const uint32_t* klen;  // key-length column
  const char* db;        // string pool
  const uint32_t* tix;   // resource-type column
  uint32_t fcap, rcap;   // frame region / record staging bytes
  uint32_t type_key;     // string id of "Type"
  Rec* recs;             // global record arena (direct record writes)
  uint32_t rchunk;       // record slots per document reserved per batch (0: every record staged)
  uint32_t rstride;      // record slot stride of a batch's chunk (documents per batch)
  uint32_t group;        // lanes per document (LaunchArgs::lane_group)
  uint32_t split_on;     // lane groups may split walks (LaunchArgs::lane_group bit 16 clear; GG_SPLIT_WALK=0 sets it)
  uint32_t sguard;       // LaunchArgs::stack_guard
  uint32_t syn_off;      // heap offset of the synthetic-int table: the tile's first persist allocation, the same for
                         // every tile of the launch (its word in the lane's Ctx went to the prefix memo's valid bits)
};
__shared__ WaveConst g_wave;
#define C_HEAP(c) g_wave.heap
#define C_DN(c) (g_wave.nodes + (c).dbase)
#define C_KL(c) (g_wave.klen + (c).dbase)
#define C_DB(c) g_wave.db
#define C_FCAP(c) g_wave.fcap
#define C_RCAP(c) g_wave.rcap
#define C_TYPE_KEY(c) g_wave.type_key
#define C_TIX(c) ((c).tix_off != NONE ? g_wave.tix + (c).tix_off : nullptr)
#define C_SGUARD(c) g_wave.sguard
#define C_SYN(c) g_wave.syn_off
#else
#define C_HEAP(c) (c).heap
#define C_DN(c) (c).dn
#define C_KL(c) (c).kl
#define C_DB(c) (c).db
#define C_FCAP(c) (c).fcap
#define C_RCAP(c) (c).rcap
#define C_TYPE_KEY(c) (c).type_key
#define C_TIX(c) (c).tix
#define C_SGUARD(c) (c).sguard
#define C_SYN(c) (c).syn_off
#endif

#if GG_CTX_PACK
struct __attribute__((packed, aligned(4))) Ctx {
#else
struct Ctx {
#endif
#if GG_LANE
  uint32_t dbase;        // this document's first node (global node index; the host keeps it < 2^32)
  uint32_t tix_off;      // this document's first resource-type column entry, NONE without a column
  uint32_t rbase;        // record slot 0 of this lane's chunk in the global arena (slot i at rbase + 64 i),
                         // NONE when the batch's reservation did not fit the arena
#else
  ProgRef P;             // the rules program
  const DNodeP* dn;      // this document's packed nodes
  const uint32_t* kl;    // this document's key-length column
  const char* db;
  uint8_t* heap;
  uint32_t fcap;         // bytes of the frame region at the heap start (then record staging)
  uint32_t rcap;         // bytes of the record staging region
  const uint32_t* tix;   // this document's resource-type column (DevBatch), or null
  uint32_t type_key;     // string id of "Type"
  uint32_t sguard;       // LaunchArgs::stack_guard
#endif
  uint32_t tmp;          // grows up from tmp_base
  uint32_t pers;         // grows down from cap
  uint32_t nframes;
  uint32_t nrec;
  uint32_t err, err_a, err_b;
  uint32_t suppress;
  uint32_t rec_created;
  uint32_t memo;         // persist offset: u32 per name slot (3 = unknown)
  uint32_t split;        // lane groups: 1 + the walker level whose entries the group's lanes share out (0: none)
  uint32_t nsyn;         // synthetic ints (count()) in this tile
#if !GG_LANE
  uint32_t syn_off;      // persist offset of synthetic table (16 B each: src, lo, hi, pad); lane mode: g_wave.syn_off
#endif
  uint32_t resmap;       // document-relative node of root.Resources, or NONE
  uint32_t ffok;         // node whose fast-filter test the enclosing fan-out already passed
  uint32_t wbase;        // persist offset of the query walker's level stack
  uint32_t wdepth;       // levels in use
  uint32_t naux;         // side records staged at the top of the record region (R4 / R5 key lists)
  uint32_t vtab;         // persist offset of the root scope's resolved variables (16 B per var id:
                         // state, off, n, cap) -- query / function lets and key captures
#if GG_LANE
  // Lane l's Ctx starts at word 24 l + ... without this word: a stride sharing a factor 8 with the 64 LDS
  // banks puts the 64 lanes' copies of a field in 8 banks, an 8-way conflict on every interpreter-state
  // access (SQ_LDS_BANK_CONFLICT 4.7 cycles per LDS instruction at cfg5, profiles/r05za_lds_cfg5.csv).
  // An odd stride in words spreads them over all 64 banks (static_assert below).  The word is the lane's
  // output flag: with several lanes per document (LaunchArgs::lane_group) only the first writes records.
  uint32_t mute;
  // prefix memo (walk_run_body<false>, one lane per tile): valid bit of entry (slot, j) at slot * PM_CAP + j,
  // cleared with the tile.  It took syn_off's place, so the stride (and the kernel's LDS) is what it was.
  uint32_t pm;
#endif
#ifdef GG_STATS
  uint32_t st[8];        // diagnostic counters (build variant "stats" only)
  uint32_t tdep[8];      // timed-region nesting per category (outermost entry is timed)
  unsigned long long tst[9];   // shader-clock cycles inside each category; [8] = whole tile
  uint32_t fc[14];       // entries of the noinline evaluator functions (FCALL), for scratch-traffic estimates
#endif
#if GG_CTX_PAD
  uint32_t pad_[GG_CTX_PAD];  // LDS lane stride (bank spread of the per-lane Ctx array)
#endif
};
#if GG_LANE && !GG_CTX_PACK && !defined(GG_STATS)
static_assert((sizeof(Ctx) / 4) % 2 == 1, "lane-mode Ctx stride must be an odd number of LDS words");
#endif
// The interpreter state lives in LDS (one Ctx per lane) and is passed by reference through the
// noinline evaluator functions: the reference is typed as an LDS reference so its fields are
// read with ds_read/ds_write, and the heap and document arena are typed as global memory, so
// no access goes through flat instructions (a flat access waits for every outstanding memory
// operation of the wave, vmcnt(0) and lgkmcnt(0), which serialises the interpreter's loads).
// (The host compilation pass of this translation unit only parses the device functions: the
// address-space qualifiers are applied in the device pass.)
#if defined(__HIP_DEVICE_COMPILE__)
#define GG_AS(n) __attribute__((address_space(n)))
#else
#define GG_AS(n)
#endif
typedef GG_AS(3) Ctx LCtx;
// A clause is read in place from the LDS-staged program (lane mode) rather than copied into
// registers: a copy live across the interpreter's calls costs callee-saved VGPRs that every call
// saves to scratch; LDS re-reads after a call are cheap.
#if GG_LANE
typedef GG_AS(3) const PClause& PCRef;
#else
typedef const PClause& PCRef;
#endif
typedef GG_AS(1) const DNode gDNode;
typedef GG_AS(1) const DNodeP gDNodeP;
typedef GG_AS(1) const uint32_t gU32c;
typedef GG_AS(1) uint8_t gU8;
typedef GG_AS(1) uint32_t gU32;
typedef GG_AS(1) uint4 gU4;
typedef GG_AS(1) QR gQR;
#ifdef GG_STATS
// Inclusive wave time per category (stats build only): the outermost entry of a category reads the
// shader clock (s_memtime, a counter read) on entry and exit.  Lanes of a wave run in lock-step, so
// a lane's time includes the cycles it sits masked off while other lanes take another path.
struct TScope {
  GG_AS(3) Ctx* c; uint32_t k; unsigned long long t0;
  __device__ TScope(GG_AS(3) Ctx& cc, uint32_t kk) : c(&cc), k(kk), t0(0) { if (c->tdep[k]++ == 0) t0 = __builtin_amdgcn_s_memtime(); }
  __device__ ~TScope() { if (--c->tdep[k] == 0) c->tst[k] += __builtin_amdgcn_s_memtime() - t0; }
};
#define TSCOPE(c, k) TScope _tscope_##k(const_cast<LCtx&>(c), k)
#define STAT(c, i) ((const_cast<LCtx&>(c)).st[i]++)
#define FCALL(c, i) ((const_cast<LCtx&>(c)).fc[i]++)
#else
#define FCALL(c, i) ((void)0)
#define STAT(c, i) ((void)0)
#define TSCOPE(c, k) ((void)0)
#endif

// The recursion's lane stack in use: the AMDGPU ABI's stack pointer s32 (bytes per lane under flat
// scratch, which gfx950 code uses: eval_conj's prologue is `s_addk_i32 s32, 0x190` for its 400-byte
// frame).  Every recursion of the evaluator passes a check of it (eval_clause, the query driver,
// resolve_function), so a rules file nesting deeper than the device's lane stack ends its tile with
// E_STACK -- an explicit error -- instead of running the next call's frame past its scratch.  The guard
// leaves room for the deepest chain of frames between two checks (capi.cpp kStackMargin, derived from the
// product ISA's per-function ScratchSize by tools/stack_budget.py).
DEV bool stack_low(const LCtx& c) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t sp;
  asm volatile("s_mov_b32 %0, s32  ; gg_stack_check" : "=s"(sp));
  return sp > C_SGUARD(c);
#else
  (void)c;
  return false;
#endif
}

#define CHK(c) do { if ((c).err) return; } while (0)
#define CHKV(c, v) do { if ((c).err) return (v); } while (0)

DEV void fail(LCtx& c, uint32_t e, uint32_t a = 0, uint32_t b = 0) {
  if (!c.err) { c.err = e; c.err_a = a; c.err_b = b; }
}

// ------------------------------------------------------------------ memory ---
DEV uint32_t alloc_tmp(LCtx& c, uint32_t bytes) {
  bytes = (bytes + 15u) & ~15u;
  uint32_t o = c.tmp;
  if (c.tmp + bytes > c.pers) { fail(c, E_HEAP); return C_FCAP(c) + C_RCAP(c); }
  c.tmp += bytes;
  return o;
}
DEV uint32_t alloc_pers(LCtx& c, uint32_t bytes) {
  bytes = (bytes + 15u) & ~15u;
  if (c.pers < c.tmp + bytes) { fail(c, E_HEAP); return C_FCAP(c) + C_RCAP(c); }
  c.pers -= bytes;
  return c.pers;
}
// Heap addressing.  Offsets are per-tile logical bytes.  In lane mode the 64 lanes of a wave
// share one region interleaved at 16-byte granularity: logical chunk k of lane l lives at
// heap + k * 1024 + l * 16, so lanes touching the same logical offset (the common case: one
// program, similar documents) hit one contiguous 1 KB span instead of 64 cache lines.  A
// 16-byte-aligned chunk stays contiguous per lane, so QRs are addressed in place; wider structs
// go through hload/hstore chunk by chunk.  Wave mode: plain contiguous layout.
#ifndef GG_HEAP_GRAIN
#define GG_HEAP_GRAIN 4   // log2 of the interleave grain (bytes per lane per heap row)
#endif
DEV gU8* haddr(const LCtx& c, uint32_t off) {
  STAT(c, 1);
#if GG_LANE
  constexpr uint32_t G = GG_HEAP_GRAIN;
  return (gU8*)C_HEAP(c) + (size_t)(off >> G) * (64u << G) + (__lane_id() << G) + (off & ((1u << G) - 1u));
#else
  return (gU8*)C_HEAP(c) + off;
#endif
}
template <typename T>
DEV T hload(const LCtx& c, uint32_t off) {
  static_assert(sizeof(T) % 16 == 0, "chunked heap struct");
  T v;
  for (uint32_t k = 0; k < sizeof(T) / 16; k++) ((uint4*)&v)[k] = *(gU4*)haddr(c, off + 16 * k);
  return v;
}
template <typename T>
DEV void hstore(LCtx& c, uint32_t off, const T& v) {
  static_assert(sizeof(T) % 16 == 0, "chunked heap struct");
  for (uint32_t k = 0; k < sizeof(T) / 16; k++) *(gU4*)haddr(c, off + 16 * k) = ((const uint4*)&v)[k];
}
DEV gQR* qra(LCtx& c, uint32_t off) { return (gQR*)haddr(c, off); }
struct U32View {
  const LCtx* c;
  uint32_t off;
  DEV gU32& operator[](uint32_t i) const { return *(gU32*)haddr(*c, off + 4u * i); }
};
DEV U32View u32a(LCtx& c, uint32_t off) { return U32View{&c, off}; }
DEV uint32_t frame_off(uint32_t idx) { return idx * (uint32_t)sizeof(Frame); }
DEV Frame fget(const LCtx& c, uint32_t idx) { return hload<Frame>(c, frame_off(idx)); }
// the frame's first 16 bytes (kind, parent, root, block): all that scope walks need, so they read
// one chunk; value frames (the common kind) store only this half
DEV uint4 fhot(const LCtx& c, uint32_t idx) { return *(gU4*)haddr(c, frame_off(idx)); }
DEV void fput(LCtx& c, uint32_t idx, const Frame& f) { hstore(c, frame_off(idx), f); }

DEV void qr_push(LCtx& c, QR q) {
  uint32_t o = alloc_tmp(c, 16);
  CHK(c);
  *qra(c, o) = q;
}
DEV QR mk_qr(uint32_t node, uint32_t kind) { QR q; q.node = node; q.meta = kind; q.uref = 0; q.aux = 0; return q; }
DEV QR mk_unres(uint32_t node, uint32_t reason, uint32_t qid, uint32_t step, uint32_t aux) {
  QR q; q.node = node; q.meta = QR_UNRESOLVED | (reason << 8); q.uref = (qid << 12) | step; q.aux = aux; return q;
}
DEV uint32_t qkind(const QR& q) { return q.meta & 3u; }

// ------------------------------------------------------------------- nodes ---
DEV DNode node(const LCtx& c, uint32_t ref) {
  STAT(c, 0);
  if (ref & SYN_BIT) {
    const gU32* s = (const gU32*)haddr(c, C_SYN(c) + 16u * (ref & 0xFFFFu));
    DNode d; d.kind = K_INT; d.count = 0; d.a = s[1]; d.b = s[2]; d.key_off = NONE; d.key_len = 0; d.key_hash = 0; d.parent = NONE;
    return d;
  }
  if (ref & KEY_BIT) {
    // the key of a map entry as a String value (MapValue.keys, path_value.rs:459-466)
    uint32_t e = ref & ~KEY_BIT;
    DNode en;
    if (e & LIT_BIT) {
      en = PG(c, lit_nodes)[e & ~LIT_BIT];
    } else {
      // document nodes: key id == pool offset of the key (checked by pack_nodes_kernel)
      const DNodeP p = ((gDNodeP*)C_DN(c))[e];
      en.key_off = p.key_hash; en.key_hash = p.key_hash; en.key_len = ((gU32c*)C_KL(c))[e];
    }
    DNode d; d.kind = K_STRING; d.count = en.key_len; d.a = en.key_off; d.b = en.key_hash;
    d.key_off = NONE; d.key_len = 0; d.key_hash = 0; d.parent = NONE;
    return d;
  }
  if (ref & LIT_BIT) return PG(c, lit_nodes)[ref & ~LIT_BIT];
  const DNodeP p = ((gDNodeP*)C_DN(c))[ref];
  DNode d; d.kind = p.kc & 15u; d.count = p.kc >> 4; d.a = p.a; d.b = p.b;
  d.key_off = p.key_hash; d.key_len = 0; d.key_hash = p.key_hash; d.parent = NONE;
  return d;
}
DEV const char* bytes_of(const LCtx& c, uint32_t ref) { return (ref & LIT_BIT) ? PROG(c).bytes : C_DB(c); }
DEV uint32_t child(uint32_t ref, const DNode& n, uint32_t j) { return (ref & LIT_BIT) | (n.a + j); }
// slot j of map `ref`'s MapValue.keys (a key ref is KEY_BIT | slot): the entry itself, or -- for a
// document map with a repeated key (doc_loader.cpp Emitter) -- slot j of its key block, the keys
// list in document order with duplicates, while the entries keep one value per key
DEV uint32_t key_slot(uint32_t ref, const DNode& m, uint32_t j) {
  return (m.b && !(ref & LIT_BIT)) ? m.b + j : (ref & LIT_BIT) | (m.a + j);
}
DEV int64_t ival(const DNode& n) { return (int64_t)(((uint64_t)n.b << 32) | n.a); }
DEV double fval(const DNode& n) { return __longlong_as_double((long long)(((uint64_t)n.b << 32) | n.a)); }
DEV bool is_scalar_k(uint32_t k) { return k != K_LIST && k != K_MAP; }

DEV bool bytes_eq(const char* a, const char* b, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) if (a[i] != b[i]) return false;
  return true;
}

// Pool strings (document pool and rule literals) start 16-byte aligned and are zero-padded to
// a 16-byte multiple, so equal-length strings compare in 16-byte chunks.
DEV uint4 chunk16(const char* p, uint32_t i) { return ((const uint4*)p)[i]; }
DEV bool str_eq(const char* a, const char* b, uint32_t n) {
  for (uint32_t i = 0; i < (n + 15u) / 16u; i++) {
    uint4 p = chunk16(a, i), q = chunk16(b, i);
    if ((p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z) | (p.w ^ q.w)) return false;
  }
  return true;
}

#if GG_LANE
// Lane-mode key scans read only the entries' key ids, KSCAN at a time: the loads of one batch are
// independent, so a scan waits for one memory latency per batch instead of one per entry (each
// lane walks its own document; the arena reads are latency-, not bandwidth-bound).  Indices past
// the map's end are clamped to its last entry and masked in the compare.
static const uint32_t KSCAN = 8;
#ifndef GG_KSCAN_PRED
#define GG_KSCAN_PRED 1
#endif
template <typename NP>
DEV void key_batch(NP e, uint32_t i, uint32_t n, uint32_t (&h)[KSCAN]) {
#if GG_KSCAN_PRED
  // entries past the map's end are not loaded: a wave issues load k only if some lane's map has an
  // entry k, so small maps (a resource's Type / Properties / Metadata) cost 2-4 loads, not 8 (the
  // vector-memory address path is the kernel's busiest unit, profiles/pmc_r02_ta.json)
#pragma unroll
  for (uint32_t k = 0; k < KSCAN; k++) h[k] = i + k < n ? e[i + k].key_hash : NONE;
#else
#pragma unroll
  for (uint32_t k = 0; k < KSCAN; k++) h[k] = e[i + k < n ? i + k : n - 1].key_hash;
#endif
}
template <typename NP>
DEV uint32_t map_scan(uint32_t ref, const DNode& m, NP e, uint32_t khash) {
  for (uint32_t i = 0; i < m.count; i += KSCAN) {
    uint32_t h[KSCAN];
    key_batch(e, i, m.count, h);
#pragma unroll
    for (uint32_t k = 0; k < KSCAN; k++)
      if (i + k < m.count && h[k] == khash) return child(ref, m, i + k);   // key ids: equal ids <=> equal keys
  }
  return NONE;
}
// child of map `ref` whose key == (kp, klen, khash); NONE if absent (this lane's document)
DEV uint32_t map_get(const LCtx& c, uint32_t ref, const char* kp, uint32_t klen, uint32_t khash) {
  DNode m = node(c, ref);
  if (ref & LIT_BIT) return map_scan(ref, m, PG(c, lit_nodes) + m.a, khash);
  return map_scan(ref, m, (gDNodeP*)C_DN(c) + m.a, khash);
}
#else
// wave-cooperative: child of map `ref` whose key == (kp, klen, khash); NONE if absent
DEVN uint32_t map_get(const LCtx& c, uint32_t ref, const char* kp, uint32_t klen, uint32_t khash) {
  DNode m = node(c, ref);
  const char* base = bytes_of(c, ref);
  const uint32_t lane = __lane_id();
  for (uint32_t start = 0; start < m.count; start += 64) {
    uint32_t i = start + lane;
    bool hit = false;
    if (i < m.count) {
      DNode ch = node(c, child(ref, m, i));
      hit = ch.key_hash == khash;
    }
    unsigned long long mask = __ballot(hit);
    if (mask) return child(ref, m, start + (uint32_t)__ffsll((long long)mask) - 1u);
  }
  return NONE;
}
#endif

DEV uint32_t map_get_pstr(const LCtx& c, uint32_t ref, uint32_t sid) {
  PStr s = PG(c, strs)[sid];
  return map_get(c, ref, PROG(c).bytes + s.off, s.len, s.hash);
}

#ifndef GG_FULLKEY
#define GG_FULLKEY 4
#endif
#if GG_LANE && GG_FULLKEY
// Document maps in lane mode: the walker's key step loads whole 16-B entries, GG_FULLKEY at a time
// (0: key ids only, as map_get_key), so the matching entry's node comes with the scan and the next
// step needs no dependent reload of it (-1 %, profiles/r02_ab_fullkey.log; walk_run stays at 120
// VGPRs).
static const uint32_t KFULL = GG_FULLKEY;
DEV DNode unpack_node(const DNodeP& p) {
  DNode d; d.kind = p.kc & 15u; d.count = p.kc >> 4; d.a = p.a; d.b = p.b;
  d.key_off = p.key_hash; d.key_len = 0; d.key_hash = p.key_hash; d.parent = NONE;
  return d;
}
DEV uint32_t map_get_key_full(const LCtx& c, uint32_t ref, const DNode& m, const PPart& part, uint32_t& conv, DNode& hn) {
  const PStr key = PG(c, strs)[part.a];
  uint32_t ahash[7];
  uint32_t k0 = conv ? conv - 1 : 0, k1 = conv ? conv : 7;
  for (uint32_t k = 0; k < 7; k++) {
    if (k < k0 || k >= k1) { ahash[k] = NONE; continue; }
    ahash[k] = PG(c, strs)[PG(c, alts)[part.b + k]].hash;
  }
  const gDNodeP* e = (const gDNodeP*)C_DN(c) + m.a;
  uint32_t best = NONE, bestk = 7;
  DNodeP bn; bn.kc = 0; bn.a = 0; bn.b = 0; bn.key_hash = 0;   // the best converter match's entry
  for (uint32_t i = 0; i < m.count; i += KFULL) {
    DNodeP h[KFULL];
#pragma unroll
    for (uint32_t k = 0; k < KFULL; k++) {
      if (i + k < m.count) h[k] = e[i + k];
      else { h[k].kc = 0; h[k].a = 0; h[k].b = 0; h[k].key_hash = NONE; }
    }
#pragma unroll
    for (uint32_t q = 0; q < KFULL; q++) {
      if (i + q < m.count) {
        const uint32_t r = child(ref, m, i + q);
        STAT(c, 6);
        if (h[q].key_hash == key.hash) { hn = unpack_node(h[q]); return r; }
        uint32_t kk = 7;
        for (uint32_t k = k0; k < bestk; k++)
          if (h[q].key_hash == ahash[k]) { kk = k; break; }
        if (kk < bestk) { best = r; bestk = kk; bn = h[q]; }
      }
    }
  }
  // hn is written only once the scan is over (it may be the very node `m` the caller passed)
  if (best != NONE) { if (!conv) conv = bestk + 1; hn = unpack_node(bn); }
  return best;
}
#endif

// QueryPart::Key lookup with the reference's case-converter fallback (eval_context.rs:528-568):
// the exact key wins; otherwise the first converter (in CONVERTERS order) whose converted key is
// present, or only converter `conv` once one has been chosen for this path.  Lane mode does it in
// one pass over the map's entries (the exact-then-7-alternates sequence of lookups gives the same
// child); wave mode keeps the cooperative per-key lookups.
DEV uint32_t map_get_key(const LCtx& c, uint32_t ref, const DNode& m, const PPart& part, uint32_t& conv) {
#if GG_LANE
  const PStr key = PG(c, strs)[part.a];
  uint32_t ahash[7];
  uint32_t k0 = conv ? conv - 1 : 0, k1 = conv ? conv : 7;
  for (uint32_t k = 0; k < 7; k++) {
    if (k < k0 || k >= k1) { ahash[k] = NONE; continue; }
    ahash[k] = PG(c, strs)[PG(c, alts)[part.b + k]].hash;
  }
  uint32_t best = NONE, bestk = 7;
  for (uint32_t i = 0; i < m.count; i += KSCAN) {
    uint32_t h[KSCAN];
    if (ref & LIT_BIT) key_batch(PG(c, lit_nodes) + m.a, i, m.count, h);
    else key_batch((gDNodeP*)C_DN(c) + m.a, i, m.count, h);
    for (uint32_t q = 0; q < KSCAN && i + q < m.count; q++) {
      const uint32_t r = child(ref, m, i + q);
      STAT(c, 6);
      if (h[q] == key.hash) return r;   // key ids (doc_loader.h): no byte compare
      for (uint32_t k = k0; k < bestk; k++)
        if (h[q] == ahash[k]) { best = r; bestk = k; break; }
    }
  }
  if (best != NONE && !conv) conv = bestk + 1;
  return best;
#else
  uint32_t hit = map_get_pstr(c, ref, part.a);
  if (hit != NONE) return hit;
  if (conv) return map_get_pstr(c, ref, PG(c, alts)[part.b + conv - 1]);
  for (uint32_t k = 0; k < 7; k++) {
    hit = map_get_pstr(c, ref, PG(c, alts)[part.b + k]);
    if (hit != NONE) { conv = k + 1; return hit; }
  }
  return NONE;
#endif
}

// ---------------------------------------------------------------- records ---
// Record staging addresses.  Lane mode interleaves the record region per RECORD, not per 16-B chunk:
// slot i of lane l lives at region + i * 64 * 48 + l * 48, the same physical span as the chunk
// interleave (RECS_BYTES / 16 rows of 1 KB), so one lane's 48-B record is one or two lines instead of
// three rows (lanes push records at different times), and lanes pushing slot i together still write
// one contiguous 3 KB span.  Wave mode: the contiguous heap.
#ifndef GG_REC_INTERLEAVE
#define GG_REC_INTERLEAVE 1
#endif
#if GG_LANE && GG_REC_INTERLEAVE
// staging slot `slot` of lane `lane` of the wave (a lane group's members write their leader's slots when they
// merge a split block's records)
DEV gU4* stage_ptr(uint32_t lane, uint32_t slot) {
  static_assert(RECS_BYTES % sizeof(Rec) == 0, "record region holds whole records");
  return (gU4*)((gU8*)g_wave.heap + (size_t)(FRAMES_BYTES >> GG_HEAP_GRAIN) * (64u << GG_HEAP_GRAIN) +
                (size_t)slot * (64u * sizeof(Rec)) + lane * sizeof(Rec));
}
#endif
DEV void stage_store(LCtx& c, uint32_t slot, const Rec& r) {
#if GG_LANE && GG_REC_INTERLEAVE
  gU4* d = stage_ptr(__lane_id(), slot);
  for (uint32_t k = 0; k < sizeof(Rec) / 16; k++) d[k] = ((const uint4*)&r)[k];
#else
  hstore(c, C_FCAP(c) + slot * (uint32_t)sizeof(Rec), r);
#endif
}
DEV Rec stage_load(const LCtx& c, uint32_t slot) {
#if GG_LANE && GG_REC_INTERLEAVE
  const gU4* q = stage_ptr(__lane_id(), slot);
  Rec v;
  for (uint32_t k = 0; k < sizeof(Rec) / 16; k++) ((uint4*)&v)[k] = q[k];
  return v;
#else
  return hload<Rec>(c, C_FCAP(c) + slot * (uint32_t)sizeof(Rec));
#endif
}
// Direct record writes (lane mode): every batch reserves g_wave.rchunk record slots per lane in the global
// record arena, interleaved by slot (slot i of lane l at the wave's base + 64 i + l: lanes writing their
// i-th record together write one contiguous 3 KB row).  A tile's first rchunk records go straight to their
// output -- no staging store, no read-back, no copy-out at tile end; records past the chunk are staged in
// the lane heap and the tile is copied out contiguously at its end, as before.  Rolled-back records are
// overwritten like staged ones.  session_fetch compacts the chunks into the dense record array.
DEV uint32_t rec_chunk_slots() {
#if GG_LANE
  return g_wave.rchunk;
#else
  return 0;
#endif
}
// Ctx::mute: 0 -- the lane writes its tile's records; 1 -- a lane that shares its document's tile with a
// leader lane computes the same records but writes none; 2 | R0 << 2 -- inside a split block (eval_recursive.inc
// split_block) every lane of the group keeps the records of the values it evaluates in its own staging, record
// R0 + k at slot rec_slots - 1 - naux - k (downward, below the side records), until the group merges them
DEV uint32_t private_slot(const LCtx& c, uint32_t slot) {
#if GG_LANE
  return C_RCAP(c) / (uint32_t)sizeof(Rec) - 1u - c.naux - (slot - (c.mute >> 2));
#else
  (void)c;
  return slot;
#endif
}
DEV void rec_store(LCtx& c, uint32_t slot, const Rec& r) {
#if GG_LANE
  if (c.mute & 2u) { stage_store(c, private_slot(c, slot), r); return; }
  if (slot < g_wave.rchunk) {
    if (c.rbase != NONE && !c.mute) {
      gU4* d = (gU4*)(g_wave.recs + c.rbase + (size_t)slot * g_wave.rstride);
      for (uint32_t k = 0; k < sizeof(Rec) / 16; k++) d[k] = ((const uint4*)&r)[k];
    }
    return;
  }
  slot -= g_wave.rchunk;
  if (c.mute) return;
#endif
  stage_store(c, slot, r);
}
DEV Rec rec_load(const LCtx& c, uint32_t slot) {
#if GG_LANE
  if (slot < g_wave.rchunk) {
    Rec v;
    const gU4* q = (const gU4*)(g_wave.recs + c.rbase + (size_t)slot * g_wave.rstride);
    for (uint32_t k = 0; k < sizeof(Rec) / 16; k++) ((uint4*)&v)[k] = q[k];
    return v;
  }
  slot -= g_wave.rchunk;
#endif
  return stage_load(c, slot);
}
DEV uint32_t rec_slots(const LCtx& c) { return C_RCAP(c) / (uint32_t)sizeof(Rec); }
// room in the staging region for nmain records and naux side records (records inside the direct chunk
// take no staging space)
DEV bool rec_room(const LCtx& c, uint32_t nmain, uint32_t naux) {
  const uint32_t ch = rec_chunk_slots();
#if GG_LANE
  if (c.mute & 2u) {
    // a split block's private records sit above the leader's staged ones (R0 - ch of them) and below the side records
    const uint32_t r0 = c.mute >> 2, staged0 = r0 > ch ? r0 - ch : 0u;
    return (staged0 + (nmain - r0) + naux) * (uint32_t)sizeof(Rec) <= C_RCAP(c);
  }
#endif
  const uint32_t staged = nmain > ch ? nmain - ch : 0u;
  return (staged + naux) * (uint32_t)sizeof(Rec) <= C_RCAP(c);
}
// stores side record `w` (already publishable) below the previous ones; returns its index
DEV uint32_t aux_store(LCtx& c, const Rec& w) {
  if (!rec_room(c, c.nrec, c.naux + 1)) { fail(c, E_RECORDS); return 0; }
#if GG_LANE && GG_REC_INTERLEAVE
  if (!c.mute) stage_store(c, rec_slots(c) - 1 - c.naux, w);   // RECS_BYTES is a whole number of records
#else
  // wave mode: the region's top byte is the anchor (its size need not be a multiple of 48; the wave
  // loop publishes side records from heap + fcap + rcap downward)
  hstore(c, C_FCAP(c) + C_RCAP(c) - (c.naux + 1) * (uint32_t)sizeof(Rec), w);
#endif
  return c.naux++;
}
// A count() result referenced by a record travels as QR_SYNTH_INT (source node + value).  An
// unresolved result whose traversed_to is a count() value (a key / index / filter step on the Int,
// eval_context.rs:573-581, 587-607, 820-822, 913-919) keeps its reason and remaining query in the QR,
// so the value goes to a side record instead: node = SYN_BIT | that record's index (reporter R::N).
DEV QR publishable(LCtx& c, QR q) {
  if (q.meta != 0xFFFFFFFFu && (q.node & SYN_BIT) && q.node != NONE) {
    const gU32* s = (const gU32*)haddr(c, C_SYN(c) + 16u * (q.node & 0xFFFFu));
    QR o; o.node = s[0]; o.meta = QR_SYNTH_INT; o.uref = s[1]; o.aux = s[2];
    if (qkind(q) != QR_UNRESOLVED) return o;
    Rec a; a.kind = REC_AUX; a.clause = NONE; a.x = 0; a.y = 0; a.from = o;
    a.to.node = NONE; a.to.meta = 0xFFFFFFFFu; a.to.uref = 0; a.to.aux = 0;
    q.node = SYN_BIT | aux_store(c, a);
  }
  return q;
}
DEV void rec_push(LCtx& c, const Rec& r) {
  if (c.suppress && !VB) return;
  TSCOPE(c, 4);
  STAT(c, 5);
  Rec w = r;
  w.from = publishable(c, r.from);   // (may add a side record)
  w.to = publishable(c, r.to);
  if (!rec_room(c, c.nrec + 1, c.naux)) { fail(c, E_RECORDS); return; }
#if GG_AB_NOREC == 1 || GG_AB_NOREC == 2   // diagnostic upper bound only (records not kept: parity fails)
  (void)w;
#else
  rec_store(c, c.nrec, w);
#endif
  c.nrec++;
}
DEV Rec mk_rec(uint32_t kind, uint32_t clause) {
  Rec r; r.kind = kind; r.clause = clause; r.x = 0; r.y = 0;
  r.from = mk_qr(NONE, 0); r.to = mk_qr(NONE, 0); r.to.meta = 0xFFFFFFFFu;
  return r;
}
// verbose kernel: container open / close events and ClauseCheck::Success leaves (no-ops elsewhere)
DEV void ev_open(LCtx& c, uint32_t type, uint32_t id, uint32_t aux = 0) {
  if (!VB) return;
  Rec r = mk_rec(REC_EV_OPEN, id); r.x = type; r.y = aux; rec_push(c, r);
}
DEV void ev_close(LCtx& c, uint32_t type, uint32_t id, uint32_t st, bool alo = false, uint32_t msg = NONE) {
  if (!VB) return;
  Rec r = mk_rec(REC_EV_CLOSE, id); r.x = type; r.y = st | (alo ? 256u : 0u); r.from.uref = msg; rec_push(c, r);
}
DEV void rec_success(LCtx& c, uint32_t clause) {
  if (VB) rec_push(c, mk_rec(REC_SUCCESS, clause));
}
// drops the records a passing / skipped container made (the reference's report keeps FAILs only)
DEV void rec_rollback(LCtx& c, uint32_t mark) { if (!VB && !c.suppress) c.nrec = mark; }
// An opening record (rule, disjunction) is kept only when its container FAILs, which most do not:
// its slot is reserved (nrec advanced, nothing written) and written when the container closes as a
// failure.  Returns false when nothing was reserved (suppressed context).
DEV bool rec_reserve(LCtx& c) {
  if (c.suppress || VB) return false;
  if (!rec_room(c, c.nrec + 1, c.naux)) { fail(c, E_RECORDS); return false; }
  c.nrec++;
  return true;
}
DEV void rec_fill(LCtx& c, uint32_t slot, const Rec& r) {
  rec_store(c, slot, r);
}
// Side records: staged downward from the top of the record region and published after the tile's
// records.  They hold what an unresolved reason's text needs beyond its QR (the join keys of R4 /
// R5).  The QR carrying such a reason can outlive the clause that made it (let caches), so side
// records are never suppressed or rolled back.  Returns the side-record index.
DEV uint32_t aux_push(LCtx& c, const Rec& r) {
  Rec w = r;
  w.from = publishable(c, r.from);
  w.to = publishable(c, r.to);
  return aux_store(c, w);
}

// Key capture into the root scope (RootScope::add_variable_capture_key, eval_context.rs:1165-1176):
// appends the map entry's key (as a String value) to variable `var`'s resolved list.
DEV void capture_key(LCtx& c, uint32_t var, uint32_t entry) {
  const uint32_t slot = c.vtab + var * 16u;
  uint32_t st = u32a(c, slot)[0], off = u32a(c, slot)[1], n = u32a(c, slot)[2], cap = u32a(c, slot)[3];
  if (!st) { n = 0; cap = 0; }
  if (n == cap) {
    const uint32_t ncap = cap ? cap * 2u : 4u;
    const uint32_t noff = alloc_pers(c, ncap * 16u);
    if (c.err) return;
    for (uint32_t i = 0; i < n; i++) *qra(c, noff + i * 16u) = *qra(c, off + i * 16u);
    off = noff; cap = ncap;
  }
  *qra(c, off + n * 16u) = mk_qr(KEY_BIT | entry, QR_RESOLVED);
  U32View v = u32a(c, slot);
  v[0] = 1u; v[1] = off; v[2] = n + 1u; v[3] = cap;
}

// ---------------------------------------------------------------- frames ---
DEV uint32_t push_frame(LCtx& c, uint32_t kind, uint32_t parent, uint32_t root, uint32_t block) {
  TSCOPE(c, 7);
  STAT(c, 4);
  if ((c.nframes + 1) * (uint32_t)sizeof(Frame) > C_FCAP(c)) { fail(c, E_DEPTH); return 0; }
  uint32_t idx = c.nframes++;
  Frame f;
  f.kind = kind; f.parent = parent; f.root = root; f.block = block;
  f.cache = NONE; f.call = NONE; f.params = NONE; f.prule = NONE;
  if (kind == F_VALUE) {
    uint4 h; h.x = kind; h.y = parent; h.z = root; h.w = block;
    *(gU4*)haddr(c, frame_off(idx)) = h;
    return idx;
  }
  if ((kind == F_ROOT || kind == F_BLOCK) && block != NONE) {
    uint32_t nl = PG(c, blocks)[block].nlets;
    if (nl) {
      uint32_t o = alloc_pers(c, nl * 16);
      if (c.err) { fput(c, idx, f); return idx; }
      for (uint32_t i = 0; i < nl; i++) u32a(c, o)[i * 4] = 0;
      f.cache = o;
    }
  }
  fput(c, idx, f);
  return idx;
}
DEV void pop_frame(LCtx& c) { c.nframes--; }

DEV uint32_t frame_root(LCtx& c, uint32_t f) {
  uint4 F = fhot(c, f);
  while (F.x == F_PARAM) F = fhot(c, F.y);
  return F.z;
}

// ---------------------------------------------------------- comparisons ---
// compare_values (path_value.rs:1047-1068): 0 ok (ord in *ord), 1 NotComparable(types), 2 NotComparable(float)
struct Cmp { int32_t status; int32_t ord; uint32_t ka, kb; };

// byte-wise Ord of two pool strings (Rust String cmp), 16 bytes per step
DEV int32_t bytes_cmp(const char* a, uint32_t na, const char* b, uint32_t nb) {
  uint32_t n = na < nb ? na : nb;
  for (uint32_t i = 0; i * 16u < n; i++) {
    uint4 p = chunk16(a, i), q = chunk16(b, i);
    uint32_t w[4] = {p.x ^ q.x, p.y ^ q.y, p.z ^ q.z, p.w ^ q.w};
    uint32_t pa[4] = {p.x, p.y, p.z, p.w}, qa[4] = {q.x, q.y, q.z, q.w};
    for (uint32_t k = 0; k < 4; k++) {
      if (!w[k]) continue;
      uint32_t byte = (uint32_t)(__ffs((int)w[k]) - 1) >> 3;
      uint32_t pos = i * 16u + k * 4u + byte;
      if (pos >= n) break;   // difference lies past the shorter string: lengths decide
      uint32_t x = (pa[k] >> (byte * 8)) & 0xFFu, y = (qa[k] >> (byte * 8)) & 0xFFu;
      return x < y ? -1 : 1;
    }
  }
  return na == nb ? 0 : (na < nb ? -1 : 1);
}

DEV Cmp compare_values(const LCtx& c, uint32_t ra, const DNode& a, uint32_t rb, const DNode& b) {
  Cmp r; r.status = 0; r.ord = 0; r.ka = a.kind; r.kb = b.kind;
  if (a.kind == K_NULL && b.kind == K_NULL) return r;
  if (a.kind == K_INT && b.kind == K_INT) { int64_t x = ival(a), y = ival(b); r.ord = x < y ? -1 : (x > y ? 1 : 0); return r; }
  if (a.kind == K_STRING && b.kind == K_STRING) { r.ord = bytes_cmp(bytes_of(c, ra) + a.a, a.count, bytes_of(c, rb) + b.a, b.count); return r; }
  if (a.kind == K_FLOAT && b.kind == K_FLOAT) {
    double x = fval(a), y = fval(b);
    if (x != x || y != y) { r.status = 2; return r; }
    r.ord = x < y ? -1 : (x > y ? 1 : 0); return r;
  }
  if (a.kind == K_CHAR && b.kind == K_CHAR) { r.ord = a.a < b.a ? -1 : (a.a > b.a ? 1 : 0); return r; }
  r.status = 1;
  return r;
}

// regex is_match (path_value.rs:255,263,1074-1077) over a UTF-8 haystack by the rule's DFA over
// code-point classes (regex_dfa.h): per ASCII byte one class read and one dependent transition
// read, T[state * ncls + class]; a multi-byte character is decoded and its class found by a binary
// search over the class boundaries.  The tables are read from the LDS-staged program when they fit
// the staging window (stage_program), from HBM otherwise.  -1 = unsupported regex.
template <typename U16P, typename U8P, typename U32P>
DEV int dfa_run(U16P T, U16P A, U8P ascii, U32P bounds, uint32_t nb, uint32_t ncls, uint32_t st, const char* s, uint32_t n) {
  // A: 1 = a match ends here (decided), 2 = a match ends here if the haystack ends here (`$`)
  if (A[st] & 1u) return 1;
  uint32_t cp = 0, need = 0;
  for (uint32_t i = 0; i < n; i += 16) {
    uint4 ch = chunk16(s, i / 16u);
    uint32_t w[4] = {ch.x, ch.y, ch.z, ch.w};
    uint32_t m = n - i < 16u ? n - i : 16u;
    for (uint32_t j = 0; j < m; j++) {
      const uint32_t by = (w[j >> 2] >> ((j & 3u) * 8)) & 0xFFu;
      uint32_t cls;
      if (by < 0x80u) {
        cls = ascii[by];
      } else {
        if (by >= 0xC0u) { need = by >= 0xF0u ? 3u : by >= 0xE0u ? 2u : 1u; cp = by & (0x3Fu >> need); continue; }
        cp = (cp << 6) | (by & 0x3Fu);
        if (--need) continue;
        uint32_t lo = 0, hi = nb;   // last boundary with first code point <= cp (bounds[0] starts at U+0080)
        while (hi - lo > 1u) { const uint32_t md = (lo + hi) >> 1; if ((bounds[md] >> 8) <= cp) lo = md; else hi = md; }
        cls = bounds[lo] & 0xFFu;
      }
      st = T[st * ncls + cls];
      if (st == 0) return 0;
      if (A[st] & 1u) return 1;
    }
  }
  return A[st] ? 1 : 0;
}
#if GG_NFA
// The NFA simulation of a regex whose DFA exceeds the compile limits (regex_dfa.cpp nfa_fallback; layout
// guard_types.h kNfa*): per character the live-state bitset is intersected with the class's member set and
// the follow sets of the survivors are or-ed onto the restart set Z.  O(W + live x W) per character
// against the DFA's one lookup, so it runs only where no DFA fits; the memo still answers each distinct
// (regex, document string) pair once per launch.  Compiled only into the GG_NFA kernel variant
// (eval_kernel_nfa.hip), launched for programs holding such a regex: inlined at the evaluator's regex
// sites it grows their stack frames, which the common path should not pay.  The two live-state bitsets sit in the lane heap's free
// span above c.tmp (nothing allocates while the regex runs), not in private arrays: a 256-B private
// frame inside the recursive evaluator would outgrow its dynamic stack.
template <typename U32P>
DEV int nfa_run(const LCtx& c, U32P T, const char* s, uint32_t n) {
  const uint32_t m = T[kNfaM], W = T[kNfaW], ncls = T[kNfaCls], nb = T[kNfaNb];
  const U32P S0 = T + kNfaHdr;
  const U32P Z = S0 + W;
  const U32P FL = Z + W;
  const U32P F = FL + m;
  const U32P M = F + (size_t)m * W;
  const U32P A = M + (size_t)ncls * W;
  const U32P B = A + 128;
  if (c.pers < c.tmp + 8u * W) return -1;
  const U32View cur{&c, c.tmp}, nx{&c, c.tmp + 4u * W};
  for (uint32_t w = 0; w < W; w++) cur[w] = S0[w];
  uint32_t cf = T[kNfaStartFlags];
  if (cf & 1u) return 1;
  uint32_t cp = 0, need = 0;
  for (uint32_t i = 0; i < n; i += 16) {
    uint4 ch = chunk16(s, i / 16u);
    uint32_t wd[4] = {ch.x, ch.y, ch.z, ch.w};
    uint32_t mm = n - i < 16u ? n - i : 16u;
    for (uint32_t j = 0; j < mm; j++) {
      const uint32_t by = (wd[j >> 2] >> ((j & 3u) * 8)) & 0xFFu;
      uint32_t cls;
      if (by < 0x80u) {
        cls = A[by];
      } else {
        if (by >= 0xC0u) { need = by >= 0xF0u ? 3u : by >= 0xE0u ? 2u : 1u; cp = by & (0x3Fu >> need); continue; }
        cp = (cp << 6) | (by & 0x3Fu);
        if (--need) continue;
        uint32_t lo = 0, hi = nb;
        while (hi - lo > 1u) { const uint32_t md = (lo + hi) >> 1; if (B[2 * md] <= cp) lo = md; else hi = md; }
        cls = B[2 * lo + 1];
      }
      uint32_t nf = T[kNfaAgainFlags];
      for (uint32_t w = 0; w < W; w++) nx[w] = Z[w];
      for (uint32_t w = 0; w < W; w++) {
        uint32_t x = cur[w] & M[(size_t)cls * W + w];
        while (x) {
          const uint32_t st = w * 32u + (uint32_t)__builtin_ctz(x);
          x &= x - 1u;
          nf |= FL[st];
          const U32P f = F + (size_t)st * W;
          for (uint32_t v = 0; v < W; v++) nx[v] |= f[v];
        }
      }
      if (nf & 1u) return 1;
      for (uint32_t w = 0; w < W; w++) cur[w] = nx[w];
      cf = nf;
    }
  }
  return (cf & 2u) ? 1 : 0;
}

// The simulation is a leaf call, not inlined: the evaluator's own frames stay exactly the default
// variant's, so this variant runs in the same lane stack (no device-wide stack limit is raised for it).
#if GG_LANE
DEVN int nfa_match_lds(const LCtx& c, uint32_t table, const char* s, uint32_t n) {
  return nfa_run(c, (GG_AS(3) const uint32_t*)((GG_AS(3) const uint16_t*)PROG(c).dfa + table), s, n);
}
DEVN int nfa_match_hbm(const LCtx& c, uint32_t table, const char* s, uint32_t n) {
  return nfa_run(c, (GG_AS(1) const uint32_t*)((GG_AS(1) const uint16_t*)PROG(c).dfa + table), s, n);
}
#else
DEVN int nfa_match_any(const LCtx& c, uint32_t table, const char* s, uint32_t n) {
  return nfa_run(c, (const uint32_t*)(PROG(c).dfa + table), s, n);
}
#endif
#endif
DEV int regex_match(const LCtx& c, uint32_t rid, const char* s, uint32_t n) {
  PRegex rx = PG(c, regex)[rid];
  if (rx.flags & 1u) return -1;
  const uint32_t nb = rx.flags >> 8;
#if GG_NFA
  if (rx.flags & 2u) {
#if GG_LANE
    if (PROG(c).dfa_lds) return nfa_match_lds(c, rx.table, s, n);
    return nfa_match_hbm(c, rx.table, s, n);
#else
    return nfa_match_any(c, rx.table, s, n);
#endif
  }
#endif
#if GG_LANE
  if (PROG(c).dfa_lds) {
    typedef GG_AS(3) const uint16_t* L16;
    L16 D = (L16)PROG(c).dfa;
    return dfa_run(D + rx.table, D + rx.accept, (GG_AS(3) const uint8_t*)(D + rx.ascii),
                   (GG_AS(3) const uint32_t*)(D + rx.bounds), nb, rx.ncls, rx.start, s, n);
  }
  typedef GG_AS(1) const uint16_t* G16;
  G16 D = (G16)PROG(c).dfa;
  return dfa_run(D + rx.table, D + rx.accept, (GG_AS(1) const uint8_t*)(D + rx.ascii),
                 (GG_AS(1) const uint32_t*)(D + rx.bounds), nb, rx.ncls, rx.start, s, n);
#else
  // wave mode: the program copy may point into the workgroup's LDS window or into HBM (generic)
  const uint16_t* D = PROG(c).dfa;
  return dfa_run(D + rx.table, D + rx.accept, (const uint8_t*)(D + rx.ascii), (const uint32_t*)(D + rx.bounds), nb,
                 rx.ncls, rx.start, s, n);
#endif
}

// is_match of regex `rid` on string node `s` reached through `ref`: a document string (interned,
// 16-B aligned in the pool) is looked up in the program's memo (DevProg::rx_memo) first, and a
// computed answer is or-ed in; concurrent lanes computing the same slot store the same bits.
DEV int regex_match_ref(const LCtx& c, uint32_t rid, uint32_t ref, const DNode& s) {
  uint32_t* memo = (ref & LIT_BIT) ? nullptr : PROG(c).rx_memo;
  if (!memo) return regex_match(c, rid, bytes_of(c, ref) + s.a, s.count);
  const uint32_t slot = s.a >> 4, sh = (slot & 15u) * 2u;
  uint32_t* w = memo + (size_t)rid * PROG(c).memo_words + (slot >> 4);
  const uint32_t v = (*w >> sh) & 3u;
  if (v) return (int)v - 1;
  const int m = regex_match(c, rid, C_DB(c) + s.a, s.count);
  if (m >= 0) atomicOr(w, (uint32_t)(m + 1) << sh);
  return m;
}

DEV bool within(const DRange& r, uint32_t kind, const DNode& v) {
  if (kind == K_RANGE_INT) {
    int64_t x = ival(v), lo = (int64_t)r.lo, hi = (int64_t)r.hi;
    bool l = (r.incl & 1) ? lo <= x : lo < x;
    bool u = (r.incl & 2) ? hi >= x : hi > x;
    return l && u;
  }
  if (kind == K_RANGE_FLOAT) {
    double x = fval(v), lo = __longlong_as_double((long long)r.lo), hi = __longlong_as_double((long long)r.hi);
    bool l = (r.incl & 1) ? lo <= x : lo < x;
    bool u = (r.incl & 2) ? hi >= x : hi > x;
    return l && u;
  }
  uint32_t x = v.a, lo = (uint32_t)r.lo, hi = (uint32_t)r.hi;
  bool l = (r.incl & 1) ? lo <= x : lo < x;
  bool u = (r.incl & 2) ? hi >= x : hi > x;
  return l && u;
}

// compare_eq (path_value.rs:1070-1152) for a pair that is not (map, map) or (list, list).
// Returns Cmp with status 0 and ord 0 (equal) / 1 (not equal), status 1/2 for NotComparable,
// status 3 for an unsupported regex (raises E_REGEX_UNSUPPORTED).
DEV Cmp compare_eq_leaf(LCtx& c, uint32_t ra, const DNode& a, uint32_t rb, const DNode& b) {
  Cmp r; r.status = 0; r.ord = 1; r.ka = a.kind; r.kb = b.kind;
  if ((a.kind == K_STRING && b.kind == K_REGEX) || (a.kind == K_REGEX && b.kind == K_STRING)) {
    uint32_t rs = a.kind == K_STRING ? ra : rb;
    DNode s = a.kind == K_STRING ? a : b, x = a.kind == K_STRING ? b : a;
    int m = regex_match_ref(c, x.b, rs, s);
    if (m < 0) { fail(c, E_REGEX_UNSUPPORTED, x.b); r.status = 3; return r; }
    r.ord = m ? 0 : 1; return r;
  }
  if (a.kind == K_STRING && b.kind == K_STRING) {
    r.ord = a.b == b.b ? 0 : 1;   // string ids
    return r;
  }
  if (a.kind == K_BOOL && b.kind == K_BOOL) { r.ord = a.a == b.a ? 0 : 1; return r; }
  if (a.kind == K_REGEX && b.kind == K_REGEX) {
    r.ord = (a.count == b.count && str_eq(bytes_of(c, ra) + a.a, bytes_of(c, rb) + b.a, a.count)) ? 0 : 1;
    return r;
  }
  if ((a.kind == K_INT && b.kind == K_RANGE_INT) || (a.kind == K_FLOAT && b.kind == K_RANGE_FLOAT) ||
      (a.kind == K_CHAR && b.kind == K_RANGE_CHAR)) {
    r.ord = within(PG(c, lit_ranges)[b.a], b.kind, a) ? 0 : 1; return r;
  }
  Cmp v = compare_values(c, ra, a, rb, b);
  if (v.status) return v;
  r.ord = v.ord == 0 ? 0 : 1;
  return r;
}

// PartialEq (path_value.rs:245-291) for a pair that is not (map, map) or (list, list): errors => false
DEV bool pv_eq_leaf(LCtx& c, uint32_t ra, const DNode& a, uint32_t rb, const DNode& b) {
  if (a.kind == K_BOOL && b.kind == K_BOOL) return a.a == b.a;
  if (a.kind == K_STRING && b.kind == K_STRING) return a.b == b.b;
  if ((a.kind == K_STRING && b.kind == K_REGEX) || (a.kind == K_REGEX && b.kind == K_STRING)) {
    uint32_t rs = a.kind == K_STRING ? ra : rb;
    DNode s = a.kind == K_STRING ? a : b, x = a.kind == K_STRING ? b : a;
    int m = regex_match_ref(c, x.b, rs, s);
    if (m < 0) { fail(c, E_REGEX_UNSUPPORTED, x.b); return false; }
    return m == 1;
  }
  if (a.kind == K_REGEX && b.kind == K_REGEX)
    return a.count == b.count && str_eq(bytes_of(c, ra) + a.a, bytes_of(c, rb) + b.a, a.count);
  if ((a.kind == K_INT && b.kind == K_RANGE_INT) || (a.kind == K_FLOAT && b.kind == K_RANGE_FLOAT) ||
      (a.kind == K_CHAR && b.kind == K_RANGE_CHAR))
    return within(PG(c, lit_ranges)[b.a], b.kind, a);
  Cmp v = compare_values(c, ra, a, rb, b);
  return v.status == 0 && v.ord == 0;
}

// The structural recursion of compare_eq / PartialEq over (map, map) and (list, list) pairs runs
// iteratively with an explicit stack of pair levels on the tmp heap (16 B each: first child of
// each side -- or the map itself on the right, whose entries are looked up by key -- the next
// entry and the entry count | map flag), so neither comparison makes a device call.  Entries are
// visited in the recursion's order and the first unequal pair's result is the answer.
static const uint32_t EQ_DEPTH = 64;
DEV bool eq_containers(const DNode& a, const DNode& b) {
  return (a.kind == K_MAP && b.kind == K_MAP) || (a.kind == K_LIST && b.kind == K_LIST);
}
// next child pair of the innermost level; false when the map lookup on the right misses
DEV bool eq_next_pair(LCtx& c, uint4& L, uint32_t& ca, uint32_t& cb) {
  const uint32_t i = L.z++;
  ca = L.x + i;
  if (L.w >> 31) {
    DNode cn = node(c, ca);
    cb = map_get(c, L.y, bytes_of(c, ca) + cn.key_off, cn.key_len, cn.key_hash);
    return cb != NONE;
  }
  cb = L.y + i;
  return true;
}
DEV uint4 eq_level(uint32_t ra, const DNode& a, uint32_t rb, const DNode& b) {
  uint4 L;
  L.x = child(ra, a, 0);
  L.y = a.kind == K_MAP ? rb : child(rb, b, 0);
  L.z = 0;
  L.w = a.count | (a.kind == K_MAP ? 0x80000000u : 0u);
  return L;
}

DEVN Cmp compare_eq(LCtx& c, uint32_t ra, uint32_t rb) {
  DNode a = node(c, ra), b = node(c, rb);
  if (!eq_containers(a, b)) return compare_eq_leaf(c, ra, a, rb, b);
  Cmp r; r.status = 0; r.ord = 1; r.ka = a.kind; r.kb = b.kind;
  if (a.count != b.count) return r;
  const uint32_t mark = c.tmp;
  const uint32_t stk = alloc_tmp(c, EQ_DEPTH * 16);
  if (c.err) return r;
  uint32_t d = 0;
  uint4 L = eq_level(ra, a, rb, b);
  for (;;) {
    if (L.z >= (L.w & 0x7FFFFFFFu)) {
      if (d == 0) { r.ord = 0; break; }   // every entry equal
      d--;
      L = *(gU4*)haddr(c, stk + d * 16u);
      continue;
    }
    const bool is_map = L.w >> 31;
    uint32_t ca, cb;
    if (!eq_next_pair(c, L, ca, cb)) { r.ka = r.kb = K_MAP; break; }   // key missing on the right
    DNode an = node(c, ca), bn = node(c, cb);
    if (eq_containers(an, bn)) {
      if (an.count != bn.count) { r.ka = an.kind; r.kb = bn.kind; break; }
      if (d + 1 >= EQ_DEPTH) { fail(c, E_DEPTH); break; }
      *(gU4*)haddr(c, stk + d * 16u) = L;
      d++;
      L = eq_level(ca, an, cb, bn);
      continue;
    }
    Cmp x = compare_eq_leaf(c, ca, an, cb, bn);
    if (x.status || x.ord) { r = x; break; }
    (void)is_map;
  }
  c.tmp = mark;
  return r;
}

DEVN bool pv_eq(LCtx& c, uint32_t ra, uint32_t rb) {
  DNode a = node(c, ra), b = node(c, rb);
  if (!eq_containers(a, b)) return pv_eq_leaf(c, ra, a, rb, b);
  if (a.count != b.count) return false;
  const uint32_t mark = c.tmp;
  const uint32_t stk = alloc_tmp(c, EQ_DEPTH * 16);
  if (c.err) return false;
  uint32_t d = 0;
  bool eq = false;
  uint4 L = eq_level(ra, a, rb, b);
  for (;;) {
    if (L.z >= (L.w & 0x7FFFFFFFu)) {
      if (d == 0) { eq = true; break; }
      d--;
      L = *(gU4*)haddr(c, stk + d * 16u);
      continue;
    }
    uint32_t ca, cb;
    if (!eq_next_pair(c, L, ca, cb)) break;
    DNode an = node(c, ca), bn = node(c, cb);
    if (eq_containers(an, bn)) {
      if (an.count != bn.count) break;
      if (d + 1 >= EQ_DEPTH) { fail(c, E_DEPTH); break; }
      *(gU4*)haddr(c, stk + d * 16u) = L;
      d++;
      L = eq_level(ca, an, cb, bn);
      continue;
    }
    if (!pv_eq_leaf(c, ca, an, cb, bn)) break;
  }
  c.tmp = mark;
  return eq;
}

// ---------------------------------------------------------- query engine ---
DEV uint32_t qpart_index(const LCtx& c, uint32_t qid, uint32_t qi) { return PG(c, queries)[qid].first + qi; }

DEV Rec mk_rec(uint32_t kind, uint32_t clause);
DEV void rec_push(LCtx& c, const Rec& r);

// in_cmp(not_in) (eval.rs:540-566): 1 true, 0 false, -1 NotComparable
DEVN int in_cmp(LCtx& c, uint32_t l, uint32_t r, bool not_in) {
  DNode a = node(c, l), b = node(c, r);
  if (a.kind == K_STRING && b.kind == K_STRING) {
    const char* hay = bytes_of(c, r) + b.a;
    const char* nd = bytes_of(c, l) + a.a;
    bool found = a.count == 0;
    for (uint32_t i = 0; !found && i + a.count <= b.count; i++) found = bytes_eq(hay + i, nd, a.count);
    return (found != not_in) ? 1 : 0;
  }
  if (b.kind == K_LIST) {
    bool found = false;
    for (uint32_t i = 0; i < b.count; i++) {
      Cmp x = compare_eq(c, l, child(r, b, i));
      if (x.status) return -1;
      if (x.ord == 0) found = true;
    }
    return (found != not_in) ? 1 : 0;
  }
  Cmp x = compare_eq(c, l, r);
  if (x.status) return -1;
  return ((x.ord == 0) != not_in) ? 1 : 0;
}

// MapKeyFilter step (eval_context.rs:830-922): real_binary_operation over the map's keys with
// context "" (records leak into the enclosing clause, exactly as in the reference).  The RHS values are
// in `rhs` (a literal, the RHS query walked from `cur`, or a function); this leaf compares every key of
// map `cur` and returns the selected entries (u32 each, at *sel_off) -- map_key_filter then continues the
// query at qi + 1 from each of them.
DEV uint32_t map_key_select(LCtx& c, uint32_t cur, const DNode& cn, const PPart& part, View rhs, uint32_t& sel_off) {
  uint32_t op = part.c & 15u;
  bool neg = (part.c >> 4) & 1u;
  if (op == OP_EQ && rhs.n > 1) op = OP_IN;
  uint32_t yop = op | (neg ? 16u : 0u) | 0x100u;
  // the keys compared are MapValue.keys (eval_context.rs:850-856): with a repeated key, every
  // occurrence, and each passing one selects values.get(key) -- the key's single entry -- again
  const bool kblock = cn.b && !(cur & LIT_BIT);
  const uint32_t nkeys = kblock ? node(c, cn.b).count : cn.count;
  sel_off = alloc_tmp(c, (nkeys ? nkeys : 1) * 4);
  uint32_t items_off = alloc_tmp(c, (rhs.n ? rhs.n : 1) * 16);
  if (c.err) return 0;
  uint32_t nsel = 0;
  for (uint32_t j = 0; j < nkeys && !c.err; j++) {
    const uint32_t kslot = key_slot(cur, cn, j);
    uint32_t entry = kslot;
    if (kblock) {
      const uint32_t kid = node(c, kslot).key_hash;
      for (uint32_t i = 0; i < cn.count; i++)
        if (node(c, child(cur, cn, i)).key_hash == kid) { entry = child(cur, cn, i); break; }
    }
    uint32_t kref = KEY_BIT | kslot;
    if (op == OP_IN) {
      bool found = false;
      for (uint32_t i = 0; i < rhs.n && !c.err; i++) {
        QR r = *qra(c, rhs.off + i * 16);
        if (qkind(r) == QR_UNRESOLVED) { *qra(c, items_off + i * 16) = r; continue; }
        uint32_t rr = r.node;
        int res = in_cmp(c, kref, rr, neg);
        if (res < 0 && qkind(r) == QR_LITERAL) {
          DNode rn = node(c, rr);
          if (rn.kind == K_LIST && rn.count == 1) { rr = child(rr, rn, 0); res = in_cmp(c, kref, rr, neg); }
        }
        *qra(c, items_off + i * 16) = mk_qr(rr, QR_RESOLVED);
        if (res == 1) found = true;
      }
      if (c.err) break;
      c.rec_created++;
      if (found) { rec_success(c, NONE); u32a(c, sel_off)[nsel++] = entry; continue; }
      if (!c.suppress || VB) {
        Rec rc = mk_rec(REC_IN, NONE);
        rc.from = mk_qr(kref, QR_RESOLVED); rc.x = rhs.n; rc.y = yop;
        rec_push(c, rc);
        for (uint32_t i = 0; i < rhs.n; i += 2) {
          Rec l = mk_rec(REC_LIST, NONE);
          l.from = *qra(c, items_off + i * 16);
          if (i + 1 < rhs.n) l.to = *qra(c, items_off + (i + 1) * 16);
          rec_push(c, l);
        }
      }
    } else {
      for (uint32_t i = 0; i < rhs.n && !c.err; i++) {
        QR r = *qra(c, rhs.off + i * 16);
        c.rec_created++;
        Rec rc = mk_rec(REC_CMP, NONE);
        rc.from = mk_qr(kref, QR_RESOLVED); rc.y = yop;
        if (qkind(r) == QR_UNRESOLVED) { rc.to = r; rec_push(c, rc); continue; }
        uint32_t rr = r.node;
        Cmp x = compare_eq(c, kref, rr);
        if (x.status && qkind(r) == QR_LITERAL) {
          DNode rn = node(c, rr);
          if (rn.kind == K_LIST && rn.count == 1) { rr = child(rr, rn, 0); x = compare_eq(c, kref, rr); }
        }
        if (c.err) break;
        bool ok = x.status == 0 && ((x.ord == 0) != neg);
        if (ok) { rec_success(c, NONE); u32a(c, sel_off)[nsel++] = entry; continue; }
        rc.to = mk_qr(rr, QR_RESOLVED);
        rec_push(c, rc);
      }
    }
  }
  return nsel;
}

// Fast filter test (compiler-marked `[ key == 'string' ]`, see compiler.cpp fast_filter_clause):
// 1 = the clause PASSes for value `v`, 0 = it FAILs, -1 = not decidable here (non-map value, key
// absent -- the generic path then tries the case-converted keys -- or a list, whose Eq has
// unwrapping/flattening rules): the caller runs the generic conjunction evaluation.  Records the
// generic path would create are suppressed inside filters, so only the status matters.
DEV int fast_filter(LCtx& c, uint32_t fc, uint32_t v) {
  STAT(c, 7);
  DNode vn = node(c, v);
  if (vn.kind != K_MAP) return -1;
  const PClause pc = PG(c, clauses)[fc];
  const PPart kp = PG(c, parts)[PG(c, queries)[pc.a].first];
  uint32_t ch = map_get_pstr(c, v, kp.a);
  if (ch == NONE) return -1;
  DNode cn = node(c, ch);
  if (cn.kind == K_LIST) return -1;
  if (cn.kind != K_STRING) return 0;   // NotComparable: the clause FAILs (records suppressed in filters)
  DNode ln = PG(c, lit_nodes)[pc.b & ~LIT_BIT];
  if (ln.kind == K_REGEX) {
    // `<key> == /re/` (compiler: DFA-compilable regexes only): is_match over the value's bytes
    const int m = regex_match_ref(c, ln.b, ch, cn);
    return m < 0 ? -1 : m;
  }
  return cn.b == ln.b ? 1 : 0;
}

// ------------------------------------------------------- iterative walker ---
// query_retrieval (eval_context.rs:337-924) is depth-first recursion over the query's steps; here
// it is one loop with an explicit stack of fan-out levels in the tile heap (48 B per level), so a
// fan-out costs a level push instead of a device call (a call saves ~100 callee-saved VGPRs to
// scratch on entry: ~25 KB of traffic per wave per call).  Results keep the reference's
// depth-first order: a level hands out its children in order and each child is walked to the
// end before the next one.
enum WKind : uint32_t { WK_VAR = 0, WK_LIST = 1, WK_MAP = 2, WK_ACCMAP = 3, WK_FLIST = 4 };
struct WLevel {
  uint32_t kind, qi, cur, n;        // fan-out step, node (VAR: view offset), entry count
  uint32_t j0, resolver, conv, fpushed;   // VAR: next entry; others: current chunk base
  uint32_t keep_lo, keep_hi, pass_lo, pass_hi;   // chunk masks: entries left / shortcut PASS
};
#if GG_LANE
static const uint32_t WLEVELS = 32;
#else
static const uint32_t WLEVELS = 256;
#endif

// PPart.c of a filter (compiler.cpp): clause id + 1 of its fast-filter clause (bits 0-29), bit 31 "the rest of
// the conjunction decides", bit 30 COOP_FILTER: the conjunction reads only the value it tests (no variables,
// rule references, functions or captures), so several lanes may test the values of one list at once
static const uint32_t COOP_FILTER = 1u << 30;
// bit 29 QUICK_FILTER: the conjunction's clauses are key paths (an unnamed `[*]` last) against one literal or a
// unary check, none of which can raise (compiler.cpp quick_conj): quick_conj tests a value without the evaluator
static const uint32_t QUICK_FILTER = 1u << 29;
#ifndef GG_QUICK
#define GG_QUICK 1
#endif
// one-lane walkers hand quick-filter chunks to the driver (coop_level); not in the NFA kernel variant, where the
// added return path changes the walker's code generation and the lane kernel's results on a program with three or
// more NFA-simulated regexes differed from the oracle (tests/test_gpu_parity.py test_nfa_regex_pack_vs_oracle;
// cause not found -- the one-lane path there keeps the per-value filter requests)
#ifndef GG_QUICK_WALK
#define GG_QUICK_WALK (!GG_NFA)
#endif
DEV uint32_t fast_ff(const LCtx& c, uint32_t pc) { return pc & 0x1FFFFFFFu; }
// shortcut masks for the chunk of entries [j0, j0 + 64) of a fan-out level (see the comment at
// WK_MAP in query_retrieval): keep = entries that still need the full path, pass = entries whose
// shortcut test said PASS
DEV void walk_chunk(LCtx& c, const PQuery& Q, uint32_t kind, uint32_t qi, uint32_t cur, const DNode& cn, uint32_t j0,
                    uint64_t& keep, uint64_t& pass) {
  const uint32_t jn = cn.count - j0 < 64 ? cn.count - j0 : 64;
  keep = jn == 64 ? ~0ull : ((1ull << jn) - 1ull);
  pass = 0;
  if (kind == WK_LIST || VB) return;
  if (kind == WK_MAP) {
    uint32_t ffc = 0;
    if (PG(c, parts)[Q.first + qi].a != NONE) return;   // named: every entry is captured
    if (qi + 1 < Q.n) {
      const PPart nx = PG(c, parts)[Q.first + qi + 1];
      if (nx.kind == P_FILTER && nx.b == NONE) ffc = fast_ff(c, nx.c);
    }
    if (!ffc) return;
    // `Resources.*[ Type == '...' ]`: the test reads the resource-type column
    uint32_t tlit = NONE;
    const gU32c* tixp = (const gU32c*)C_TIX(c);
    if (tixp && cur == c.resmap) {
      const PClause fpc = PG(c, clauses)[ffc - 1];
      const DNode fl = PG(c, lit_nodes)[fpc.b & ~LIT_BIT];
      if (fl.kind == K_STRING && PG(c, strs)[PG(c, parts)[PG(c, queries)[fpc.a].first].a].hash == C_TYPE_KEY(c)) tlit = fl.b;
    }
    for (uint32_t j = 0; j < jn; j++) {
      int ff;
      if (tlit != NONE) {
        const uint32_t t = tixp[j0 + j];
        ff = t == TIX_UNDECIDED ? fast_filter(c, ffc - 1, child(cur, cn, j0 + j)) : (t == tlit ? 1 : 0);
      } else {
        ff = fast_filter(c, ffc - 1, child(cur, cn, j0 + j));
      }
      if (ff == 0) { c.rec_created++; keep &= ~(1ull << j); }
      else if (ff == 1) pass |= 1ull << j;
    }
    return;
  }
  const PPart part = PG(c, parts)[Q.first + qi];
  if (kind == WK_FLIST) c.rec_created += jn;
  if (!fast_ff(c, part.c)) return;
  for (uint32_t j = 0; j < jn; j++) {
    int ff = fast_filter(c, fast_ff(c, part.c) - 1, child(cur, cn, j0 + j));
    if (ff == 0) { if (kind == WK_ACCMAP) c.rec_created++; keep &= ~(1ull << j); }
    else if (ff == 1 && !(part.c >> 31)) pass |= 1ull << j;   // bit 31: the rest of the conjunction decides
  }
}

DEV uint32_t walk_off(const LCtx& c, uint32_t d) { return c.wbase + d * (uint32_t)sizeof(WLevel); }
#if GG_LANE
// A filtered list (or map-values) fan-out whose chunks go to the driver (coop_chunk): 1 -- the document's lane
// group tests them together (or, one lane per document, a quick filter's chunk: one call per 64 values instead of
// a filter request per value); 2 -- a quick filter's chunk this lane tests alone (below a split walk's split level,
// where the group's lanes walk different entries); 0 -- the walker's own chunk pass
// one lane per document: a quick filter's chunk (the one-lane walker's own test, kept apart from coop_level so
// that walker's code is the same as without lane groups)
DEV bool coop_level_one(const LCtx& c, const PQuery& Q, const WLevel& L) {
  if (L.kind != WK_FLIST && L.kind != WK_ACCMAP) return false;
  if (g_wave.group < 2) return GG_QUICK && (PG(c, parts)[Q.first + L.qi].c & QUICK_FILTER) != 0;
  if (c.split && c.split != c.wdepth) return false;
  const uint32_t pc = PG(c, parts)[Q.first + L.qi].c;
  return fast_ff(c, pc) != 0 || (pc & COOP_FILTER) != 0;
}
DEV uint32_t coop_level(const LCtx& c, const PQuery& Q, const WLevel& L) {
  if (L.kind != WK_FLIST && L.kind != WK_ACCMAP) return 0;
  const uint32_t pc = PG(c, parts)[Q.first + L.qi].c;
  const bool quick = GG_QUICK && (pc & QUICK_FILTER) != 0;
  if (g_wave.group < 2) return quick ? 1u : 0u;
  if (c.split && c.split != c.wdepth) return quick ? 2u : 0u;
  return (fast_ff(c, pc) != 0 || (pc & COOP_FILTER) != 0) ? 1u : 0u;
}
#endif
// Walker level d.  Lane mode interleaves the level stack per 48-B level (level d of lane l at the
// region's first row + d * 64 * 48 + l * 48: the same physical span as the chunk interleave), as
// the record staging does, so one lane's level is one or two lines instead of three rows.
#ifndef GG_WALK_INTERLEAVE
#define GG_WALK_INTERLEAVE 0
#endif
#if GG_LANE && GG_WALK_INTERLEAVE
DEV gU4* walk_ptr(const LCtx& c, uint32_t d) {
  return (gU4*)((gU8*)C_HEAP(c) + (size_t)(c.wbase >> GG_HEAP_GRAIN) * (64u << GG_HEAP_GRAIN) +
                (size_t)d * (64u * sizeof(WLevel)) + __lane_id() * sizeof(WLevel));
}
DEV WLevel walk_load(const LCtx& c, uint32_t d) {
  const gU4* q = walk_ptr(c, d);
  WLevel v;
  for (uint32_t k = 0; k < sizeof(WLevel) / 16; k++) ((uint4*)&v)[k] = q[k];
  return v;
}
DEV void walk_store(LCtx& c, uint32_t d, const WLevel& L) {
  gU4* q = walk_ptr(c, d);
  for (uint32_t k = 0; k < sizeof(WLevel) / 16; k++) q[k] = ((const uint4*)&L)[k];
}
#else
DEV WLevel walk_load(const LCtx& c, uint32_t d) { return hload<WLevel>(c, walk_off(c, d)); }
DEV void walk_store(LCtx& c, uint32_t d, const WLevel& L) { hstore(c, walk_off(c, d), L); }
#endif

// a filter's conjunction for one value: records suppressed, temporaries dropped.  Verbose: `conj`
// carries the record kind in its top bits -- Filter/Map#n (check_and_delegate, eval_context.rs:280)
// or Filter/List#n (:758); a scalar under `[*]` (:790-815) makes no record
// FK_SCALAR: a scalar under `[*]` (eval_context.rs:790-815) -- its conjunction is evaluated under the
// enclosing clause's record with no Filter container around it, so its failing clauses are reported
// with that clause (extraction skips only the children of Filter records): records are kept, and
// roll back with the enclosing clause like any nested clause's
static const uint32_t FK_MAP = 1u << 30, FK_LIST = 2u << 30, FK_SCALAR = 1u << 29;
// Split walks (lane groups, eval_recursive.inc query_retrieval_body): the lanes of a document's group share out
// the entries of the walk's first fan-out level -- entry i to lane i mod G -- and each lane's results follow a
// marker QR naming the entry, so the driver can merge the lanes' lists in entry order.
static const uint32_t QR_MARK = 0xFFFFFFFEu;
DEV bool split_skip(LCtx& c, uint32_t level, uint32_t idx) {
#if GG_LANE
  if (c.split != level + 1u) return false;
  const uint32_t m = g_wave.group - 1u;
  if ((idx & m) != (__lane_id() & m)) return true;
  QR k; k.node = idx; k.meta = QR_MARK; k.uref = 0; k.aux = 0;
  qr_push(c, k);
#else
  (void)c; (void)level; (void)idx;
#endif
  return false;
}
// The walker proper (walk_run) is a leaf: it makes no device calls, so it runs in caller-saved
// registers with no prologue saves.  Steps that need the evaluator (a `%var` head, `%var` keys, a
// filter's conjunction, a map-key filter) make it return a request with its registers parked in
// the WState record; query_retrieval (a small driver whose only live state is that record) serves
// the request and re-enters the walker at the recorded site.  A device call costs the callee's
// prologue saves, so the expensive frame is taken only by the requests, not by every walk.
enum WReq : uint32_t { RQ_DONE = 0, RQ_VAR = 1, RQ_KEYVAR = 2, RQ_FILTER = 3, RQ_MAPKEY = 4, RQ_CHUNK = 5, RQ_QCHUNK = 6 };
enum WSite : uint32_t { WS_START = 0, WS_VAR = 1, WS_DEAD = 2, WS_FILTER_MAP = 3, WS_FILTER_SCALAR = 4, WS_FILTER_LEVEL = 5,
                        WS_CHUNK = 6 };
struct WState {
  uint32_t qi, qid, cur, resolver, conv, wbase, site, ra;   // walker registers; request argument
  uint32_t rb, st, voff, vn;                                  // frame argument; served results
};

// Prefix memo (one lane per tile).  Rules repeat a walk: consecutive clauses over `%buckets.Properties.
// PublicAccessBlockConfiguration.<leaf>` redo the two key steps for every bucket.  The compiler gives the access
// clauses' queries that share a run of plain key steps right after the same root-only `%var` head a slot (PQuery.pad
// bits 8-15: slot + 1, bits 16-23: steps in the run; compiler.cpp mark_prefix_slots).  The first walk of value j
// that passes the run's end stores the node it reached in entry (slot, j); later walks of value j descend from
// there.  A plain key step on a map writes no record, captures nothing and leaves rec_created alone, so both walks
// give the same results.  Only a run resolved by exact keys from converter state 0 is stored or reused (the
// state at the run's end is then 0 again); a failed prefix is never stored, so it is walked again and yields
// today's unresolved result.  The marked variables are root query / function lets nothing captures into: their
// value list is fixed for the tile once resolved, so (slot, j) names one value.  Entries live in the lane heap
// below the walker's level stack (PM_BYTES, allocated with the tile), one node reference each: a hit is one heap
// read against one node read and one dependent entry scan per key step.  The valid bits are Ctx.pm, cleared with
// the tile, so nothing of a previous tile is read.  Values at or past PM_CAP are walked as before.  The walker's
// code generation decides whether this pays (DESIGN.md 4.1, round 7): the miss is one register kept across the
// descent and a compare per step -- entries that carried the node's words, a second inlined key scan, a call or a
// request to the driver for the miss all cost the other rules files more than the memo saved.
// GG_PREFIX_MEMO=0 builds without it (A/B).
#ifndef GG_PREFIX_MEMO
#define GG_PREFIX_MEMO 1
#endif
static const uint32_t PM_CAP = kPrefixCap, PM_BYTES = kPrefixSlots * kPrefixCap * 4;   // guard_types.h
static const uint32_t SYN_BYTES = 256 * 16;   // the synthetic-int table (256 of 16 B), a tile's first persist allocation
#define GG_PM (GG_LANE && GG_PREFIX_MEMO)
#if GG_PM
DEV gU32* pm_entry(const LCtx& c, uint32_t bit) { return (gU32*)haddr(c, c.wbase - PM_BYTES + 4u * bit); }
#endif

// GROUP: the walker of lane groups (LaunchArgs::lane_group > 1), with the split-walk and shared-chunk hooks; a
// separate instantiation, so the walker the one-lane-per-tile launches inline carries none of their registers
// (walk_run's frame: 124 B without them, 188 B with)
template <bool GROUP>
DEV uint32_t walk_run_body(LCtx& c, WState& w) { FCALL(c, 7);
  const PQuery Q = PG(c, queries)[w.qid];
  const uint32_t qid = w.qid, wbase = w.wbase;
  uint32_t qi = w.qi, cur = w.cur, resolver = w.resolver, conv = w.conv;
  bool descend = true, resume_level = false;
  uint32_t rst = w.st;
  // The innermost level lives in registers while this invocation works on it (a child walked to
  // its end comes straight back to it): it is written to the heap stack only when a deeper level
  // is pushed over it or the walker returns a request, instead of a store and a dependent reload
  // per child.
  WLevel T;
  DNode Tcn;             // T's container node (map / list levels): children come from it without a reload
  int32_t tdepth = -1;   // level index cached in T, -1 = none
  auto flush = [&]() {
    if (tdepth >= 0) walk_store(c, (uint32_t)tdepth, T);
    tdepth = -1;
  };
  auto set_top = [&](const WLevel& L, uint32_t d, const DNode& lcn) {
    if (tdepth >= 0 && tdepth != (int32_t)d) walk_store(c, (uint32_t)tdepth, T);
    T = L;
    Tcn = lcn;
    tdepth = (int32_t)d;
  };
#if GG_PM
  uint32_t pm = 0;       // a memo miss under way: (entry bit + 1) << 16 | the step after the run; 0 = none
#endif
  switch (w.site) {
    case WS_START: break;
    case WS_VAR:
      if (!c.err) {
        if (c.wdepth >= WLEVELS) { fail(c, E_DEPTH); }
        else {
          WLevel L;
          L.kind = WK_VAR; L.qi = qi; L.cur = w.voff; L.n = w.vn; L.j0 = 0; L.resolver = resolver; L.conv = conv;
          L.fpushed = 0; L.keep_lo = L.keep_hi = L.pass_lo = L.pass_hi = 0;
          set_top(L, c.wdepth, Tcn);
          c.wdepth++;
        }
      }
      descend = false;
      break;
    case WS_DEAD: descend = false; break;
    case WS_CHUNK: descend = false; break;   // the parked level's chunk masks were filled in (coop_chunk)
    case WS_FILTER_MAP:
      if (!c.err && rst == ST_PASS) qi++;
      else descend = false;
      break;
    case WS_FILTER_SCALAR:
      pop_frame(c);
      if (!c.err && rst == ST_PASS) qi++;
      else descend = false;
      break;
    default:   // WS_FILTER_LEVEL
      if (c.err) pop_frame(c);   // the entry's value frame (the level itself unwinds below)
      descend = false;
      resume_level = true;
      break;
  }
  w.site = WS_START;
  for (;;) {
#if GG_LANE && GG_FULLKEY
    bool have_next = false;   // ncn holds node(cur), from the key scan that found cur
    DNode ncn;
#endif
    // ---- descend from (qi, cur) through single-successor steps, to a result, a dead end or a fan-out
    while (descend) {
      descend = false;
      if (c.err) break;
#if GG_PM
      if constexpr (!GROUP) {
        // the run's end is reached only through its resolved key steps (a failed step ends the descent)
        if (pm && qi == (pm & 0xFFFFu)) {
          const uint32_t bit = (pm >> 16) - 1u;
          if (!conv) { *pm_entry(c, bit) = cur; c.pm |= 1u << bit; }
          pm = 0;
        }
      }
#endif
      if (qi >= Q.n) { qr_push(c, mk_qr(cur, QR_RESOLVED)); break; }
      const PPart part = PG(c, parts)[Q.first + qi];
      uint32_t lkind = NONE, ln = 0;
      if (qi == 0 && part.kind == P_VAR_HEAD) {
        if (part.c) {
          // a root-only variable already resolved (compiler mark_root_vars): its values come straight
          // from the root table, no request to the scope chain
          const uint4 vs = *(gU4*)haddr(c, c.vtab + part.a * 16u);
          if (vs.x) {
            if (c.wdepth >= WLEVELS) { fail(c, E_DEPTH); break; }
            WLevel L;
            L.kind = WK_VAR; L.qi = qi; L.cur = vs.y; L.n = vs.z; L.j0 = 0; L.resolver = resolver; L.conv = conv;
            L.fpushed = 0; L.keep_lo = L.keep_hi = L.pass_lo = L.pass_hi = 0;
            set_top(L, c.wdepth, Tcn);
            c.wdepth++;
            break;
          }
        }
        w.qi = qi; w.cur = cur; w.resolver = resolver; w.conv = conv; w.site = WS_VAR; w.ra = part.a;
        flush(); return RQ_VAR;
      }
#if GG_LANE && GG_FULLKEY
      DNode cn = have_next ? ncn : node(c, cur);
      have_next = false;
#else
      DNode cn = node(c, cur);
#endif
      switch (part.kind) {
        case P_THIS:
          qi++;
          descend = true;
          continue;
        case P_KEY_INDEX:
        case P_INDEX: {
          int32_t idx = (int32_t)part.a;
          if (cn.kind == K_LIST) {
            uint32_t check = (uint32_t)(idx >= 0 ? idx : -idx);
            if (check < cn.count) { cur = child(cur, cn, check); qi++; descend = true; continue; }
            qr_push(c, mk_unres(cur, R_INDEX_OOB, qid, 0, (uint32_t)idx));
          } else if (part.kind == P_KEY_INDEX) {
            qr_push(c, mk_unres(cur, R_KEY_INDEX_NOT_ARRAY, qid, 0, (uint32_t)idx));
          } else {
            qr_push(c, mk_unres(cur, R_INDEX_NOT_ARRAY, qid, qi, (uint32_t)idx));
          }
          break;
        }
        case P_KEY: {
          if (cn.kind != K_MAP) { qr_push(c, mk_unres(cur, R_NOT_STRUCT, qid, qi, 0)); break; }
#if GG_LANE && GG_FULLKEY
          if (!(cur & LIT_BIT)) {
            uint32_t hit = map_get_key_full(c, cur, cn, part, conv, ncn);
            if (hit != NONE) {
              cur = hit; qi++; descend = true; have_next = true; continue;
            }
            qr_push(c, mk_unres(cur, R_KEY_NOT_FOUND, qid, qi, 0));
            break;
          }
#endif
          uint32_t hit = map_get_key(c, cur, cn, part, conv);
          if (hit != NONE) { cur = hit; qi++; descend = true; continue; }
          qr_push(c, mk_unres(cur, R_KEY_NOT_FOUND, qid, qi, 0));
          break;
        }
        case P_KEY_VAR:
          if (cn.kind != K_MAP) { qr_push(c, mk_unres(cur, R_NOT_STRUCT, qid, qi, 0)); break; }
          w.qi = qi; w.cur = cur; w.resolver = resolver; w.conv = conv; w.site = WS_DEAD;
          flush(); return RQ_KEYVAR;
        case P_ALL_INDICES:
        case P_ALL_VALUES: {
          bool named = part.a != NONE;
          if (cn.kind == K_LIST) {
            if (cn.count == 0) { qr_push(c, mk_unres(cur, R_NO_MORE_ENTRIES, qid, qi, 0)); break; }
            lkind = WK_LIST; ln = cn.count;
          } else if (cn.kind == K_MAP) {
            if (part.kind == P_ALL_INDICES && !named) { qi++; descend = true; continue; }
            // named (`[*] name` / `* name`): every entry's key is captured as it is visited
            if (cn.count == 0) { qr_push(c, mk_unres(cur, R_NO_MORE_ENTRIES, qid, qi, 0)); break; }
            // Filtered fan-out runs in two passes per chunk of 64 entries: the shortcut test over
            // the chunk, then the full path for the survivors only (in entry order).  In lane mode
            // the wave then iterates max(survivors) times with most lanes active, instead of once
            // per entry with the few lanes whose entry matched.
            lkind = WK_MAP; ln = cn.count;
          } else {
            qi++;
            descend = true;
            continue;
          }
          break;
        }
        case P_FILTER: {
          if (cn.kind == K_MAP) {
            uint32_t prev = qi > 0 ? PG(c, parts)[Q.first + qi - 1].kind : P_THIS;
            if (prev == P_ALL_VALUES || prev == P_ALL_INDICES) {
              // check_and_delegate(...)(resolver)  eval_context.rs:268-313
              c.rec_created++;
              if (fast_ff(c, part.c) && !VB) {
                const bool passed = c.ffok == cur;
                c.ffok = NONE;
                const uint4 F = fhot(c, resolver);
                if (F.x == F_VALUE && F.z == cur) {
                  int ff = passed ? 1 : fast_filter(c, fast_ff(c, part.c) - 1, cur);
                  if (ff == 0) break;
                  if (ff == 1 && !(part.c >> 31)) { qi++; descend = true; continue; }
                }
              }
              w.qi = qi; w.cur = cur; w.resolver = resolver; w.conv = conv; w.site = WS_FILTER_MAP;
              w.ra = part.a | (VB ? FK_MAP : 0u); w.rb = resolver;
              flush(); return RQ_FILTER;
            } else if (prev == P_KEY || prev == P_KEY_VAR || prev == P_KEY_INDEX) {
              // accumulate_map(check_and_delegate(..)) over the map's values
              lkind = WK_ACCMAP; ln = cn.count;
            } else {
              fail(c, E_UNSUPPORTED, 2);
            }
          } else if (cn.kind == K_LIST) {
            lkind = WK_FLIST; ln = cn.count;
          } else {
            uint32_t prev = qi > 0 ? PG(c, parts)[Q.first + qi - 1].kind : P_THIS;
            if (prev == P_ALL_INDICES) {
              uint32_t f = push_frame(c, F_VALUE, resolver, cur, NONE);
              if (c.err) break;
              w.qi = qi; w.cur = cur; w.resolver = resolver; w.conv = conv; w.site = WS_FILTER_SCALAR;
              w.ra = part.a | FK_SCALAR; w.rb = f;
              flush(); return RQ_FILTER;
            } else {
              qr_push(c, mk_unres(cur, R_FILTER_NOT_STRUCT, qid, qi, 0));
            }
          }
          break;
        }
        case P_MAP_KEY_FILTER:
          if (cn.kind != K_MAP) { qr_push(c, mk_unres(cur, R_MAPFILTER_NOT_STRUCT, qid, qi, 0)); break; }
          w.qi = qi; w.cur = cur; w.resolver = resolver; w.conv = conv; w.site = WS_DEAD;
          flush(); return RQ_MAPKEY;
        default:
          fail(c, E_UNSUPPORTED, 6);
          break;
      }
      if (lkind != NONE && !c.err) {
        if (c.wdepth >= WLEVELS) { fail(c, E_DEPTH); break; }
        WLevel L;
        L.kind = lkind; L.qi = qi; L.cur = cur; L.n = ln; L.j0 = 0xFFFFFFC0u; L.resolver = resolver; L.conv = conv;
        L.fpushed = 0; L.keep_lo = L.keep_hi = L.pass_lo = L.pass_hi = 0;
        set_top(L, c.wdepth, cn);
        c.wdepth++;
      }
    }
    // ---- next child of the innermost level that has one
    bool got = false;
    while (!c.err && c.wdepth > wbase) {
      WLevel L;
      const bool cached = tdepth == (int32_t)(c.wdepth - 1);
      if (cached) L = T;
      else L = walk_load(c, c.wdepth - 1);
      DNode cn_keep = Tcn;   // the level's container node (map / list levels), kept with the level in T
      if (L.kind == WK_VAR) {
        if (L.fpushed) { pop_frame(c); L.fpushed = 0; }
        while (L.j0 < L.n && !c.err) {
          if (GROUP && split_skip(c, c.wdepth - 1, L.j0)) { L.j0++; continue; }   // another lane of the group walks it
          QR e = *qra(c, L.cur + L.j0 * 16);
          L.j0++;
          if (qkind(e) == QR_UNRESOLVED) { qr_push(c, e); continue; }
          uint32_t index = L.qi + 1;
          if (L.qi + 1 < Q.n && PG(c, parts)[Q.first + L.qi + 1].kind == P_ALL_INDICES) index = L.qi + 2;
          if (index < Q.n) {
            // the ValueScope of each variable value (eval_context.rs:366-377) is observable only by a
            // later filter / map-key filter / %var key (compiler: PPart.b of the head)
            uint32_t f = L.resolver;
            if (PG(c, parts)[Q.first + L.qi].b) {
              f = push_frame(c, F_VALUE, L.resolver, e.node, NONE);
              if (c.err) break;
              L.fpushed = 1;
            }
            qi = index; cur = e.node; resolver = f; conv = L.conv;
#if GG_PM
            if constexpr (!GROUP) {
              // the mark is read here, not kept with Q: a query without one pays an LDS read and a branch
              pm = 0;
              const uint32_t mark = PG(c, queries)[qid].pad >> 8, j = L.j0 - 1u;
              if (mark && j < PM_CAP && !L.conv) {
                const uint32_t bit = ((mark & 0xFFu) - 1u) * PM_CAP + j, end = index + (mark >> 8);
                if ((c.pm >> bit) & 1u) { cur = *pm_entry(c, bit); qi = end; }
                else pm = ((bit + 1u) << 16) | end;
              }
            }
#endif
            got = true;
            break;
          }
          qr_push(c, e);
        }
      } else {
        const DNode cn = cached ? Tcn : node(c, L.cur);
        cn_keep = cn;
        uint64_t keep = ((uint64_t)L.keep_hi << 32) | L.keep_lo, pass = ((uint64_t)L.pass_hi << 32) | L.pass_lo;
        if (resume_level) {
          // back from a filter test of entry j (WS_FILTER_LEVEL): its value frame is the innermost
          resume_level = false;
          const uint32_t j = L.fpushed >> 8;
          L.fpushed = 0;
          const uint32_t v = child(L.cur, cn, L.j0 + j);
          if (L.kind == WK_ACCMAP) {
            if (rst == ST_PASS) {
              const uint32_t cv = PG(c, parts)[Q.first + L.qi].b;
              if (cv != NONE) capture_key(c, cv, key_slot(L.cur, cn, L.j0 + j));   // check_and_delegate (eval_context.rs:290-293)
              L.fpushed = 1;
              qi = L.qi + 1; cur = v; resolver = c.nframes - 1; conv = L.conv;
              got = true;
            } else {
              pop_frame(c);
            }
          } else {
            pop_frame(c);   // WK_FLIST: the value frame only scopes the filter test
            if (rst == ST_PASS) { qi = L.qi + 1; cur = v; resolver = L.resolver; conv = L.conv; got = true; }
          }
        } else if (L.fpushed) {
          pop_frame(c);
          L.fpushed = 0;
        }
        while (!c.err && !got) {
          if (!keep) {
            L.j0 += 64;
            if (L.j0 >= L.n) break;
#if GG_LANE
            if constexpr (GROUP) {
              const uint32_t cl = coop_level(c, Q, L);
              if (cl) {
                // the chunk's filter tests split over the document's lane group (or quick, by this lane): the
                // driver runs them (coop_chunk) and writes the chunk's masks into the parked level
                L.keep_lo = L.keep_hi = L.pass_lo = L.pass_hi = 0;
                L.fpushed = 0;
                set_top(L, c.wdepth - 1, cn);
                flush();
                w.site = WS_CHUNK;
                return cl == 2u ? RQ_QCHUNK : RQ_CHUNK;
              }
            } else if (GG_QUICK_WALK && coop_level_one(c, Q, L)) {
              // a quick filter's chunk: the driver tests it (coop_chunk) and writes the masks into the parked level
              L.keep_lo = L.keep_hi = L.pass_lo = L.pass_hi = 0;
              L.fpushed = 0;
              set_top(L, c.wdepth - 1, cn);
              flush();
              w.site = WS_CHUNK;
              return RQ_CHUNK;
            }
#endif
            walk_chunk(c, Q, L.kind, L.qi, L.cur, cn, L.j0, keep, pass);
            continue;
          }
          const uint32_t j = (uint32_t)__ffsll((long long)keep) - 1u;
          keep &= keep - 1ull;
          if (GROUP && split_skip(c, c.wdepth - 1, L.j0 + j)) continue;   // another lane of the group walks it
          const uint32_t v = child(L.cur, cn, L.j0 + j);
          const bool jpass = (pass >> j) & 1ull;
          if (L.kind == WK_LIST || (L.kind == WK_FLIST && jpass)) {
            qi = L.qi + 1; cur = v; resolver = L.resolver; conv = L.conv;
            got = true;
            break;
          }
          if (L.kind == WK_MAP) {
            const PPart fp = PG(c, parts)[Q.first + L.qi];
            // accumulate_map's allv (eval_context.rs:692-696): the key is the zip's keys[j] (:216)
            if (fp.a != NONE) { capture_key(c, fp.a, key_slot(L.cur, cn, L.j0 + j)); if (c.err) break; }
            // survivors passed the shortcut test (unless undecided): the filter step need not redo it
            c.ffok = jpass ? v : NONE;
            // an entry's value frame is the scope a later filter / map-key filter / %var key step
            // reads (compiler: PPart.b); a plain key path below the fan-out runs in the level's scope
            uint32_t f = L.resolver;
            if (fp.b) {
              f = push_frame(c, F_VALUE, L.resolver, v, NONE);
              if (c.err) break;
              L.fpushed = 1;
            }
            qi = L.qi + 1; cur = v; resolver = f; conv = L.conv;
            got = true;
            break;
          }
          const uint32_t f = push_frame(c, F_VALUE, L.resolver, v, NONE);
          if (c.err) break;
          if (L.kind == WK_ACCMAP) c.rec_created++;
          if (L.kind == WK_ACCMAP && jpass) {
            const uint32_t cv = PG(c, parts)[Q.first + L.qi].b;
            if (cv != NONE) { capture_key(c, cv, key_slot(L.cur, cn, L.j0 + j)); if (c.err) break; }   // check_and_delegate (eval_context.rs:290-293)
            L.fpushed = 1;
            qi = L.qi + 1; cur = v; resolver = f; conv = L.conv;
            got = true;
            break;
          }
          // the filter's conjunction for entry j: park the level (masks + j) and ask the driver
          L.keep_lo = (uint32_t)keep; L.keep_hi = (uint32_t)(keep >> 32);
          L.pass_lo = (uint32_t)pass; L.pass_hi = (uint32_t)(pass >> 32);
          L.fpushed = j << 8;
          set_top(L, c.wdepth - 1, cn);
          flush();
          w.site = WS_FILTER_LEVEL; w.ra = PG(c, parts)[Q.first + L.qi].a; w.rb = f;
          if (VB) w.ra |= L.kind == WK_FLIST ? FK_LIST : FK_MAP;
          flush(); return RQ_FILTER;
        }
        L.keep_lo = (uint32_t)keep; L.keep_hi = (uint32_t)(keep >> 32);
        L.pass_lo = (uint32_t)pass; L.pass_hi = (uint32_t)(pass >> 32);
      }
      if (got) { set_top(L, c.wdepth - 1, cn_keep); break; }
      if (tdepth == (int32_t)(c.wdepth - 1)) tdepth = -1;   // popped: its state is dead
      c.wdepth--;
    }
    if (!got) break;
    descend = true;
  }
  // an error unwinds this walk's levels (their value frames are the innermost ones)
  while (c.wdepth > wbase) {
    WLevel L;
    if (tdepth == (int32_t)(c.wdepth - 1)) { L = T; tdepth = -1; }
    else L = walk_load(c, c.wdepth - 1);
    if (L.fpushed & 0xFFu) pop_frame(c);
    c.wdepth--;
  }
  flush();
  return RQ_DONE;
}

// a walk's registers at its start (query_retrieval from step qi of query qid at node cur)
DEV void walk_init(const LCtx& c, WState& w, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv) {
  w.qi = qi; w.qid = qid; w.cur = cur; w.resolver = resolver; w.conv = conv; w.wbase = c.wdepth;
  w.site = WS_START; w.ra = 0; w.rb = 0; w.st = 0; w.voff = 0; w.vn = 0;
}

// copies a tmp view into the persist region
DEV View persist_view(LCtx& c, View v) {
  View p; p.n = v.n; p.off = alloc_pers(c, v.n ? v.n * 16 : 16);
  if (c.err) return p;
  for (uint32_t i = 0; i < v.n; i++) *qra(c, p.off + i * 16) = *qra(c, v.off + i * 16);
  return p;
}

// ----------------------------------------------------------------- unary ---
DEV uint32_t cl_op(PCRef pc) { return pc.flags & 15u; }
DEV bool cl_not(PCRef pc) { return (pc.flags >> 4) & 1u; }
DEV bool cl_neg(PCRef pc) { return (pc.flags >> 5) & 1u; }
DEV uint32_t cl_rhs(PCRef pc) { return (pc.flags >> 8) & 15u; }
DEV bool cl_empty_expr(PCRef pc) { return (pc.flags >> 12) & 1u; }

DEV void rec_unary(LCtx& c, uint32_t clause, QR from) {
  Rec r = mk_rec(REC_UNARY, clause); r.from = from; rec_push(c, r);
}

// returns: 0 = empty/skip, fills pass/fail counts
struct Agg { uint32_t pass, fail; bool empty; uint32_t empty_status; };

DEV Agg unary_operation(LCtx& c, uint32_t clause, PCRef pc, uint32_t frame, View lhs) {
  TSCOPE(c, 3);
  Agg g; g.pass = 0; g.fail = 0; g.empty = false; g.empty_status = ST_SKIP;
  uint32_t op = cl_op(pc);
  bool neg = cl_not(pc), inverse = cl_neg(pc);
  if (cl_empty_expr(pc) && op == OP_EMPTY) {
    if (lhs.n) {
      for (uint32_t i = 0; i < lhs.n; i++) {
        QR e = *qra(c, lhs.off + i * 16);
        bool pass;
        QR res = e;
        if (qkind(e) != QR_UNRESOLVED) {
          DNode n = node(c, e.node);
          bool isnull = n.kind == K_NULL;
          pass = neg ? !isnull : isnull;
          res = mk_qr(e.node, QR_RESOLVED);
        } else {
          pass = !neg;
        }
        if (inverse) pass = !pass;
        if (pass) { g.pass++; rec_success(c, clause); } else { g.fail++; rec_unary(c, clause, res); }
      }
      return g;
    }
    bool result = !neg;
    if (inverse) result = !result;
    g.empty = true;
    if (result) { g.empty_status = ST_PASS; rec_success(c, clause); }
    else { g.empty_status = ST_FAIL; rec_push(c, mk_rec(REC_NOVALUE_EMPTY, clause)); }
    return g;
  }
  if (lhs.n == 0) { g.empty = true; g.empty_status = ST_SKIP; return g; }
  for (uint32_t i = 0; i < lhs.n; i++) {
    QR e = *qra(c, lhs.off + i * 16);
    bool r;
    if (qkind(e) == QR_UNRESOLVED) {
      r = op == OP_EMPTY;   // !EXISTS == EMPTY; IS_* false
    } else {
      DNode n = node(c, e.node);
      switch (op) {
        case OP_EXISTS: r = true; break;
        case OP_EMPTY:
          if (n.kind == K_LIST || n.kind == K_MAP || n.kind == K_STRING) r = n.count == 0;
          else if (n.kind == K_BOOL) r = false;
          else { fail(c, E_EMPTY_INCOMPATIBLE, e.node, n.kind); return g; }
          break;
        case OP_IS_STRING: r = n.kind == K_STRING; break;
        case OP_IS_LIST: r = n.kind == K_LIST; break;
        case OP_IS_MAP: r = n.kind == K_MAP; break;
        case OP_IS_BOOL: r = n.kind == K_BOOL; break;
        case OP_IS_INT: r = n.kind == K_INT; break;
        case OP_IS_FLOAT: r = n.kind == K_FLOAT; break;
        default: r = n.kind == K_NULL; break;
      }
    }
    if (neg) r = !r;
    if (inverse) r = !r;
    if (r) { g.pass++; rec_success(c, clause); } else { g.fail++; rec_unary(c, clause, e); }
  }
  return g;
}

// ---------------------------------------------------------------- binary ---
// ValueEvalResult (operators.rs:62-96) staged on the tmp stack
enum VerKind : uint32_t { V_LHS_UNRES = 0, V_RHS_UNRES = 1, V_NOTCMP = 2, V_SUCCESS = 3, V_FAIL = 4 };
enum CmpKind : uint32_t { CK_VALUE = 0, CK_VALUEIN = 1, CK_LISTIN = 2, CK_QUERYIN = 3 };

struct Ver {
  uint32_t kind, ck;
  uint32_t a, b;         // lhs / rhs node refs (or list nodes)
  QR u;                  // unresolved (LHS/RHS_UNRES)
  uint32_t diff_off, diff_n, l_off, l_n, r_off, r_n, nc, nct;
};

DEV Ver vget(const LCtx& c, uint32_t off) { return hload<Ver>(c, off); }

DEV void ver_push(LCtx& c, const Ver& v) {
  uint32_t o = alloc_tmp(c, sizeof(Ver));
  CHK(c);
  hstore(c, o, v);
}
DEV Ver mk_ver(uint32_t kind, uint32_t ck, uint32_t a, uint32_t b) {
  Ver v; v.kind = kind; v.ck = ck; v.a = a; v.b = b; v.u = mk_qr(NONE, 0);
  v.diff_off = 0; v.diff_n = 0; v.l_off = 0; v.l_n = 0; v.r_off = 0; v.r_n = 0; v.nc = 0; v.nct = 0;
  return v;
}

// node-ref arrays on the tmp stack
struct Arr { uint32_t off, n; };
DEV Arr arr_new(LCtx& c, uint32_t cap) { Arr a; a.off = alloc_tmp(c, (cap ? cap : 1) * 4); a.n = 0; return a; }
DEV void arr_put(LCtx& c, Arr& a, uint32_t v) { u32a(c, a.off)[a.n++] = v; }
DEV uint32_t arr_at(LCtx& c, const Arr& a, uint32_t i) { return u32a(c, a.off)[i]; }

DEV bool arr_contains(LCtx& c, const Arr& a, uint32_t ref) {
  for (uint32_t i = 0; i < a.n; i++) if (pv_eq(c, arr_at(c, a, i), ref)) return true;
  return false;
}
DEV bool list_contains(LCtx& c, uint32_t list_ref, uint32_t ref) {
  DNode l = node(c, list_ref);
  for (uint32_t i = 0; i < l.count; i++) if (pv_eq(c, child(list_ref, l, i), ref)) return true;
  return false;
}

// match_value with compare_eq / Common comparator
// compare_eq for the scalar kinds, inline (containers, regexes and ranges take the call)
DEV Cmp compare_eq_scalar(LCtx& c, uint32_t ra, const DNode& a, uint32_t rb) {
  if (((ra | rb) & (SYN_BIT | KEY_BIT)) == 0) {
    DNode b = node(c, rb);
    if (a.kind == b.kind && (a.kind == K_STRING || a.kind == K_BOOL || a.kind == K_INT || a.kind == K_NULL)) {
      Cmp r; r.status = 0; r.ka = a.kind; r.kb = b.kind;
      if (a.kind == K_STRING) r.ord = a.b == b.b ? 0 : 1;
      else if (a.kind == K_NULL) r.ord = 0;
      else r.ord = (a.a == b.a && (a.kind == K_BOOL || a.b == b.b)) ? 0 : 1;
      return r;
    }
  }
  return compare_eq(c, ra, rb);
}

// `a` = node(c, l), which the caller has already read
DEV Ver match_value(LCtx& c, uint32_t l, const DNode& a, uint32_t r, uint32_t op) {
  Cmp x;
  if (op == OP_EQ) x = compare_eq_scalar(c, l, a, r);
  else { DNode b = node(c, r); x = compare_values(c, l, a, r, b); }
  if (x.status == 3) return mk_ver(V_FAIL, CK_VALUE, l, r);  // error already raised
  if (x.status) { Ver v = mk_ver(V_NOTCMP, CK_VALUE, l, r); v.nc = x.status == 1 ? NC_TYPES : NC_FLOAT; v.nct = (x.ka << 8) | x.kb; return v; }
  bool ok;
  if (op == OP_EQ) ok = x.ord == 0;
  else if (op == OP_LT) ok = x.ord < 0;
  else if (op == OP_LE) ok = x.ord <= 0;
  else if (op == OP_GT) ok = x.ord > 0;
  else ok = x.ord >= 0;
  return mk_ver(ok ? V_SUCCESS : V_FAIL, CK_VALUE, l, r);
}
DEV Ver match_value(LCtx& c, uint32_t l, uint32_t r, uint32_t op) { const DNode a = node(c, l); return match_value(c, l, a, r, op); }

DEV Ver string_in(LCtx& c, uint32_t l, uint32_t r) {
  DNode a = node(c, l), b = node(c, r);
  if (a.kind == K_STRING && b.kind == K_STRING) {
    const char* hay = bytes_of(c, r) + b.a;
    const char* nd = bytes_of(c, l) + a.a;
    bool found = a.count == 0;
    for (uint32_t i = 0; !found && i + a.count <= b.count; i++) found = bytes_eq(hay + i, nd, a.count);
    return mk_ver(found ? V_SUCCESS : V_FAIL, CK_VALUE, l, r);
  }
  Ver v = mk_ver(V_NOTCMP, CK_VALUE, l, r); v.nc = NC_STRING_IN; return v;
}

DEV Ver contained_in(LCtx& c, uint32_t l, uint32_t r) {
  DNode a = node(c, l), b = node(c, r);
  if (a.kind == K_LIST) {
    if (b.kind == K_LIST) {
      if (b.count && node(c, child(r, b, 0)).kind == K_LIST) {
        bool in = list_contains(c, r, l);
        Ver v = mk_ver(in ? V_SUCCESS : V_FAIL, CK_LISTIN, l, r);
        if (!in) { Arr d = arr_new(c, 1); if (!c.err) arr_put(c, d, l); v.diff_off = d.off; v.diff_n = d.n; }
        return v;
      }
      Arr d = arr_new(c, a.count);
      if (c.err) return mk_ver(V_FAIL, CK_LISTIN, l, r);
      for (uint32_t i = 0; i < a.count; i++) {
        uint32_t e = child(l, a, i);
        if (!list_contains(c, r, e)) arr_put(c, d, e);
      }
      Ver v = mk_ver(d.n == 0 ? V_SUCCESS : V_FAIL, CK_LISTIN, l, r);
      v.diff_off = d.off; v.diff_n = d.n;
      return v;
    }
    Ver v = mk_ver(V_NOTCMP, CK_VALUE, l, r); v.nc = NC_CONTAINED_IN; return v;
  }
  if (b.kind == K_LIST) return mk_ver(list_contains(c, r, l) ? V_SUCCESS : V_FAIL, CK_VALUEIN, l, r);
  return match_value(c, l, r, OP_EQ);
}

DEV bool is_literal_view(LCtx& c, View v, uint32_t& node_out) {
  if (v.n == 1) { QR q = *qra(c, v.off); if (qkind(q) == QR_LITERAL) { node_out = q.node; return true; } }
  return false;
}

// resolved/literal selection (operators.rs:116-130); unresolved go through on_unres
DEV Arr selected(LCtx& c, View v) {
  Arr a = arr_new(c, v.n);
  if (c.err) return a;
  for (uint32_t i = 0; i < v.n; i++) { QR q = *qra(c, v.off + i * 16); if (qkind(q) != QR_UNRESOLVED) arr_put(c, a, q.node); }
  return a;
}
DEV Arr flattened(LCtx& c, View v) {
  uint32_t cap = 0;
  for (uint32_t i = 0; i < v.n; i++) {
    QR q = *qra(c, v.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) continue;
    DNode n = node(c, q.node);
    cap += n.kind == K_LIST ? n.count : 1;
  }
  Arr a = arr_new(c, cap);
  if (c.err) return a;
  for (uint32_t i = 0; i < v.n; i++) {
    QR q = *qra(c, v.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) continue;
    DNode n = node(c, q.node);
    if (n.kind == K_LIST) for (uint32_t j = 0; j < n.count; j++) arr_put(c, a, child(q.node, n, j));
    else arr_put(c, a, q.node);
  }
  return a;
}
DEV void push_lhs_unres(LCtx& c, View v) {
  for (uint32_t i = 0; i < v.n; i++) {
    QR q = *qra(c, v.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; ver_push(c, e); }
  }
}
DEV void push_rhs_unres(LCtx& c, View rhs, const Arr& lhs_sel) {
  for (uint32_t i = 0; i < rhs.n; i++) {
    QR q = *qra(c, rhs.off + i * 16);
    if (qkind(q) != QR_UNRESOLVED) continue;
    for (uint32_t j = 0; j < lhs_sel.n; j++) { Ver e = mk_ver(V_RHS_UNRES, 0, arr_at(c, lhs_sel, j), NONE); e.u = q; ver_push(c, e); }
  }
}
DEV void push_rhs_unres_single(LCtx& c, View rhs, uint32_t l) {
  for (uint32_t i = 0; i < rhs.n; i++) {
    QR q = *qra(c, rhs.off + i * 16);
    if (qkind(q) != QR_UNRESOLVED) continue;
    Ver e = mk_ver(V_RHS_UNRES, 0, l, NONE); e.u = q; ver_push(c, e);
  }
}

// QueryIn over selected lhs/rhs with a diff built by `contained_in` (InOperation) or PartialEq (Eq)
DEV void push_queryin(LCtx& c, Arr diff, Arr ls, Arr rs) {
  Ver v = mk_ver(diff.n == 0 ? V_SUCCESS : V_FAIL, CK_QUERYIN, NONE, NONE);
  v.diff_off = diff.off; v.diff_n = diff.n; v.l_off = ls.off; v.l_n = ls.n; v.r_off = rs.off; v.r_n = rs.n;
  ver_push(c, v);
}

// operators.rs: EqOperation / InOperation / CommonOperator then (op, not) reverse diffs.
// Returns number of Ver entries written starting at *start; returns false for Skip.
DEVN bool compare_op(LCtx& c, uint32_t op, bool neg, View lhs, View rhs, uint32_t& start, uint32_t& count) { FCALL(c, 8);
  if (lhs.n == 0 || rhs.n == 0) return false;
  uint32_t aux_mark = c.tmp;
  // all auxiliary arrays are allocated before the Ver list so the list stays contiguous:
  // collect Vers into a separate region by first computing into the tmp stack, then compacting.
  uint32_t vstart = c.tmp;
  uint32_t lnode, rnode;
  bool ll = is_literal_view(c, lhs, lnode), rl = is_literal_view(c, rhs, rnode);
  // Ver entries and arrays interleave on the tmp stack; we record Ver offsets in an index array.
  // (simple approach: push Vers into a linked list via a side index)
  const uint32_t MAXV = 4096;
  uint32_t idx_off = alloc_tmp(c, MAXV * 4);
  if (c.err) return false;
  uint32_t nv = 0;
  auto add = [&](const Ver& v) {
    if (nv >= MAXV) { fail(c, E_HEAP); return; }
    uint32_t o = alloc_tmp(c, sizeof(Ver));
    if (c.err) return;
    hstore(c, o, v);
    u32a(c, idx_off)[nv++] = o;
  };
  if (op == OP_EQ) {
    if (ll && rl) add(match_value(c, lnode, rnode, OP_EQ));
    else if (ll) {
      for (uint32_t i = 0; i < rhs.n; i++) { QR q = *qra(c, rhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_RHS_UNRES, 0, lnode, NONE); e.u = q; add(e); } }
      DNode ln = node(c, lnode);
      for (uint32_t i = 0; i < rhs.n && !c.err; i++) {
        QR q = *qra(c, rhs.off + i * 16);
        if (qkind(q) == QR_UNRESOLVED) continue;
        if (ln.kind == K_LIST) add(match_value(c, lnode, q.node, OP_EQ));
        else {
          DNode rn = node(c, q.node);
          if (rn.kind == K_LIST) for (uint32_t j = 0; j < rn.count && !c.err; j++) add(match_value(c, lnode, child(q.node, rn, j), OP_EQ));
          else add(match_value(c, lnode, q.node, OP_EQ));
        }
      }
    } else if (rl) {
      for (uint32_t i = 0; i < lhs.n; i++) { QR q = *qra(c, lhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; add(e); } }
      DNode rn = node(c, rnode);
      for (uint32_t i = 0; i < lhs.n && !c.err; i++) {
        QR q = *qra(c, lhs.off + i * 16);
        if (qkind(q) == QR_UNRESOLVED) continue;
        DNode en = node(c, q.node);
        if (rn.kind == K_LIST) {
          if (is_scalar_k(en.kind) && rn.count == 1) add(match_value(c, q.node, child(rnode, rn, 0), OP_EQ));
          else add(match_value(c, q.node, rnode, OP_EQ));
        } else {
          if (en.kind == K_LIST) for (uint32_t j = 0; j < en.count && !c.err; j++) add(match_value(c, child(q.node, en, j), rnode, OP_EQ));
          else add(match_value(c, q.node, rnode, OP_EQ));
        }
      }
    } else {
      for (uint32_t i = 0; i < lhs.n; i++) { QR q = *qra(c, lhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; add(e); } }
      Arr ls = selected(c, lhs);
      Arr rs = selected(c, rhs);
      if (c.err) return false;
      for (uint32_t i = 0; i < rhs.n; i++) {
        QR q = *qra(c, rhs.off + i * 16);
        if (qkind(q) != QR_UNRESOLVED) continue;
        for (uint32_t j = 0; j < ls.n; j++) { Ver e = mk_ver(V_RHS_UNRES, 0, arr_at(c, ls, j), NONE); e.u = q; add(e); }
      }
      Arr diff;
      if (ls.n > rs.n) { diff = arr_new(c, ls.n); for (uint32_t i = 0; i < ls.n && !c.err; i++) { uint32_t e = arr_at(c, ls, i); if (!arr_contains(c, rs, e)) arr_put(c, diff, e); } }
      else { diff = arr_new(c, rs.n); for (uint32_t i = 0; i < rs.n && !c.err; i++) { uint32_t e = arr_at(c, rs, i); if (!arr_contains(c, ls, e)) arr_put(c, diff, e); } }
      Ver v = mk_ver(diff.n == 0 ? V_SUCCESS : V_FAIL, CK_QUERYIN, NONE, NONE);
      v.diff_off = diff.off; v.diff_n = diff.n; v.l_off = ls.off; v.l_n = ls.n; v.r_off = rs.off; v.r_n = rs.n;
      add(v);
    }
  } else if (op == OP_IN) {
    if (ll && rl) {
      Ver v = string_in(c, lnode, rnode);
      if (v.kind != V_SUCCESS) v = contained_in(c, lnode, rnode);
      add(v);
    } else if (ll) {
      for (uint32_t i = 0; i < rhs.n; i++) { QR q = *qra(c, rhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_RHS_UNRES, 0, lnode, NONE); e.u = q; add(e); } }
      Arr rs = selected(c, rhs);
      if (c.err) return false;
      bool any_list = false;
      for (uint32_t i = 0; i < rs.n; i++) if (node(c, arr_at(c, rs, i)).kind == K_LIST) any_list = true;
      DNode ln = node(c, lnode);
      if (any_list) { for (uint32_t i = 0; i < rs.n && !c.err; i++) add(contained_in(c, lnode, arr_at(c, rs, i))); }
      else if (ln.kind == K_LIST) {
        Arr diff = arr_new(c, ln.count);
        for (uint32_t i = 0; i < ln.count && !c.err; i++) { uint32_t e = child(lnode, ln, i); if (!arr_contains(c, rs, e)) arr_put(c, diff, e); }
        Arr ls = arr_new(c, 1); if (!c.err) arr_put(c, ls, lnode);
        Ver v = mk_ver(diff.n == 0 ? V_SUCCESS : V_FAIL, CK_QUERYIN, NONE, NONE);
        v.diff_off = diff.off; v.diff_n = diff.n; v.l_off = ls.off; v.l_n = ls.n; v.r_off = rs.off; v.r_n = rs.n;
        add(v);
      } else {
        for (uint32_t i = 0; i < rs.n && !c.err; i++) add(contained_in(c, lnode, arr_at(c, rs, i)));
      }
    } else if (rl) {
      DNode rn = node(c, rnode);
      for (uint32_t i = 0; i < lhs.n && !c.err; i++) {
        QR q = *qra(c, lhs.off + i * 16);
        if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; add(e); continue; }
      }
      for (uint32_t i = 0; i < lhs.n && !c.err; i++) {
        QR q = *qra(c, lhs.off + i * 16);
        if (qkind(q) == QR_UNRESOLVED) continue;
        DNode en = node(c, q.node);
        if (rn.kind == K_STRING) {
          if (en.kind == K_LIST) for (uint32_t j = 0; j < en.count && !c.err; j++) add(string_in(c, child(q.node, en, j), rnode));
          else add(string_in(c, q.node, rnode));
        } else add(contained_in(c, q.node, rnode));
      }
    } else {
      for (uint32_t i = 0; i < lhs.n; i++) { QR q = *qra(c, lhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; add(e); } }
      Arr ls = selected(c, lhs);
      Arr rs = selected(c, rhs);
      if (c.err) return false;
      for (uint32_t i = 0; i < rhs.n; i++) {
        QR q = *qra(c, rhs.off + i * 16);
        if (qkind(q) != QR_UNRESOLVED) continue;
        for (uint32_t j = 0; j < ls.n; j++) { Ver e = mk_ver(V_RHS_UNRES, 0, arr_at(c, ls, j), NONE); e.u = q; add(e); }
      }
      Arr diff = arr_new(c, ls.n);
      for (uint32_t i = 0; i < ls.n && !c.err; i++) {
        uint32_t el = arr_at(c, ls, i);
        bool found = false;
        for (uint32_t j = 0; j < rs.n && !c.err && !found; j++) {
          uint32_t mark = c.tmp;
          found = contained_in(c, el, arr_at(c, rs, j)).kind == V_SUCCESS;
          c.tmp = mark;
        }
        if (!found) arr_put(c, diff, el);
      }
      Ver v = mk_ver(diff.n == 0 ? V_SUCCESS : V_FAIL, CK_QUERYIN, NONE, NONE);
      v.diff_off = diff.off; v.diff_n = diff.n; v.l_off = ls.off; v.l_n = ls.n; v.r_off = rs.off; v.r_n = rs.n;
      add(v);
    }
  } else {
    // CommonOperator (Lt/Gt/Le/Ge): flattened cross product
    for (uint32_t i = 0; i < lhs.n; i++) { QR q = *qra(c, lhs.off + i * 16); if (qkind(q) == QR_UNRESOLVED) { Ver e = mk_ver(V_LHS_UNRES, 0, NONE, NONE); e.u = q; add(e); } }
    Arr lf = flattened(c, lhs);
    if (c.err) return false;
    for (uint32_t i = 0; i < rhs.n; i++) {
      QR q = *qra(c, rhs.off + i * 16);
      if (qkind(q) != QR_UNRESOLVED) continue;
      for (uint32_t j = 0; j < lf.n; j++) { Ver e = mk_ver(V_RHS_UNRES, 0, arr_at(c, lf, j), NONE); e.u = q; add(e); }
    }
    Arr rf = flattened(c, rhs);
    if (c.err) return false;
    for (uint32_t i = 0; i < lf.n && !c.err; i++)
      for (uint32_t j = 0; j < rf.n && !c.err; j++) add(match_value(c, arr_at(c, lf, i), arr_at(c, rf, j), op));
  }
  if (c.err) return false;
  (void)aux_mark; (void)vstart;
  if (neg) {
    for (uint32_t k = 0; k < nv && !c.err; k++) {
      const uint32_t voff = u32a(c, idx_off)[k];
      Ver v = vget(c, voff);
      if (v.kind == V_FAIL) {
        if (v.ck == CK_QUERYIN) {
          bool use_r = rhs.n >= lhs.n && op == OP_EQ;
          Arr other; other.off = use_r ? v.r_off : v.l_off; other.n = use_r ? v.r_n : v.l_n;
          Arr d; d.off = v.diff_off; d.n = v.diff_n;
          Arr rd = arr_new(c, other.n);
          for (uint32_t i = 0; i < other.n && !c.err; i++) { uint32_t e = arr_at(c, other, i); if (!arr_contains(c, d, e)) arr_put(c, rd, e); }
          v.kind = rd.n == 0 ? V_SUCCESS : V_FAIL; v.diff_off = rd.off; v.diff_n = rd.n;
        } else if (v.ck == CK_LISTIN) {
          DNode ln = node(c, v.a);
          Arr d; d.off = v.diff_off; d.n = v.diff_n;
          Arr rd = arr_new(c, ln.count);
          for (uint32_t i = 0; i < ln.count && !c.err; i++) { uint32_t e = child(v.a, ln, i); if (!arr_contains(c, d, e)) arr_put(c, rd, e); }
          v.kind = rd.n == 0 ? V_SUCCESS : V_FAIL; v.diff_off = rd.off; v.diff_n = rd.n;
        } else {
          v.kind = V_SUCCESS;
        }
      } else if (v.kind == V_SUCCESS) {
        if (v.ck == CK_QUERYIN) { v.kind = V_FAIL; v.diff_off = v.l_off; v.diff_n = v.l_n; }
        else if (v.ck == CK_LISTIN) {
          DNode ln = node(c, v.a);
          Arr rd = arr_new(c, ln.count);
          for (uint32_t i = 0; i < ln.count && !c.err; i++) arr_put(c, rd, child(v.a, ln, i));
          v.kind = V_FAIL; v.diff_off = rd.off; v.diff_n = rd.n;
        } else v.kind = V_FAIL;
      }
      hstore(c, voff, v);
    }
  }
  start = idx_off;
  count = nv;
  return !c.err;
}

DEV void rec_cmp(LCtx& c, uint32_t clause, QR from, QR to, bool has_to, uint32_t nc, uint32_t nct) {
  Rec r = mk_rec(REC_CMP, clause);
  r.from = from;
  if (has_to) r.to = to;
  r.x = nc; r.y = nct;
  rec_push(c, r);
}
DEV void rec_in(LCtx& c, uint32_t clause, uint32_t from, uint32_t to_off, uint32_t to_n, bool to_is_single, uint32_t single) {
  if (c.suppress && !VB) return;
  Rec r = mk_rec(REC_IN, clause);
  r.from = mk_qr(from, QR_RESOLVED);
  r.x = to_is_single ? 1 : to_n;
  rec_push(c, r);
  uint32_t n = to_is_single ? 1 : to_n;
  for (uint32_t i = 0; i < n; i += 2) {
    Rec l = mk_rec(REC_LIST, clause);
    l.from = mk_qr(to_is_single ? single : u32a(c, to_off)[i], QR_RESOLVED);
    if (i + 1 < n) l.to = mk_qr(u32a(c, to_off)[i + 1], QR_RESOLVED);
    rec_push(c, l);
  }
}

// A query compared with a single rule literal (`q == 'x'`, `q != 5`, `q <= 256`, `q IN [...]` over
// scalars) -- the common clause shape: the same records, in the same order, as compare_op
// followed by the record loop below (unresolved LHS values first, then one comparison per LHS value
// or list element), produced while comparing instead of through staged ValueEvalResults.  Returns
// false (nothing done) for the shapes it does not cover; compare_op handles those.
DEV bool binary_literal_stream(LCtx& c, uint32_t clause, uint32_t op, bool neg, View lhs, uint32_t rnode, Agg& g) {
  const DNode rn = node(c, rnode);
  if (op == OP_IN) {
    // contained_in(value, list) per scalar LHS value (operators.rs InOperation, literal RHS list)
    if (rn.kind != K_LIST) return false;
    for (uint32_t i = 0; i < lhs.n; i++) {
      const QR q = *qra(c, lhs.off + i * 16);
      if (qkind(q) != QR_UNRESOLVED && !is_scalar_k(node(c, q.node).kind)) return false;
    }
  } else if (op == OP_EQ) {
    if (rn.kind == K_LIST && rn.count != 1) return false;
  } else {
    if (rn.kind == K_LIST) return false;   // CommonOperator flattens both sides: plain scalar RHS only
  }
  for (uint32_t i = 0; i < lhs.n; i++) {
    const QR q = *qra(c, lhs.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) { rec_cmp(c, clause, q, q, false, 0, 0); g.fail++; }
  }
  for (uint32_t i = 0; i < lhs.n && !c.err; i++) {
    const QR q = *qra(c, lhs.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) continue;
    const DNode en = node(c, q.node);
    if (op == OP_IN) {
      const bool in = list_contains(c, rnode, q.node);
      if (c.err) return true;
      if (in != neg) { g.pass++; rec_success(c, clause); }
      else { rec_in(c, clause, q.node, 0, 0, true, rnode); g.fail++; }
      continue;
    }
    // EQ: a one-element literal list unwraps against a scalar value; a list value compares each
    // element; CommonOperator flattens list values too
    uint32_t r = rnode;
    if (op == OP_EQ && rn.kind == K_LIST) {
      if (is_scalar_k(en.kind)) r = child(rnode, rn, 0);
    }
    const bool each = en.kind == K_LIST && !(op == OP_EQ && rn.kind == K_LIST);
    const uint32_t n = each ? en.count : 1;
    for (uint32_t j = 0; j < n && !c.err; j++) {
      const uint32_t l = each ? child(q.node, en, j) : q.node;
      Ver v = each ? match_value(c, l, r, op) : match_value(c, l, en, r, op);
      if (c.err) return true;
      if (v.kind == V_NOTCMP) { rec_cmp(c, clause, mk_qr(v.a, QR_RESOLVED), mk_qr(v.b, QR_RESOLVED), true, v.nc, v.nct); g.fail++; continue; }
      const bool ok = (v.kind == V_SUCCESS) != neg;
      if (ok) { g.pass++; rec_success(c, clause); }
      else { rec_cmp(c, clause, mk_qr(v.a, QR_RESOLVED), mk_qr(v.b, QR_RESOLVED), true, 0, 0); g.fail++; }
    }
  }
  return true;
}

// `query in query` over string values (the join filters of the network pack: `Properties.SubnetId.Ref
// in %local_subnet_refs`): compare_op's InOperation verdict for two non-literal sides (operators.rs
// QueryIn: unresolved LHS values, then unresolved RHS values against every selected LHS value, then
// the LHS values no RHS value equals), with the same records and counts, computed in place -- no
// compare_op call (45 callee-saved VGPRs) and no staged Ver list.  false: a value is not a plain
// string (or a synthesized / key value), and compare_op decides.
#ifndef GG_IN_FAST
#define GG_IN_FAST 1
#endif
DEV bool in_strings_fast(LCtx& c, uint32_t clause, View lhs, View rhs, Agg& g) {
  uint32_t nl = 0, nr = 0;
  for (uint32_t i = 0; i < lhs.n; i++) {
    const QR q = *qra(c, lhs.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) continue;
    if ((q.node & (SYN_BIT | KEY_BIT)) || node(c, q.node).kind != K_STRING) return false;
    nl++;
  }
  for (uint32_t i = 0; i < rhs.n; i++) {
    const QR q = *qra(c, rhs.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) continue;
    if ((q.node & (SYN_BIT | KEY_BIT)) || node(c, q.node).kind != K_STRING) return false;
    nr++;
  }
  for (uint32_t i = 0; i < lhs.n && !c.err; i++) {
    const QR q = *qra(c, lhs.off + i * 16);
    if (qkind(q) == QR_UNRESOLVED) { rec_cmp(c, clause, q, q, false, 0, 0); g.fail++; }
  }
  for (uint32_t i = 0; i < rhs.n && !c.err; i++) {
    const QR q = *qra(c, rhs.off + i * 16);
    if (qkind(q) != QR_UNRESOLVED) continue;
    for (uint32_t j = 0; j < lhs.n && !c.err; j++) {
      const QR l = *qra(c, lhs.off + j * 16);
      if (qkind(l) != QR_UNRESOLVED) { rec_cmp(c, clause, mk_qr(l.node, QR_RESOLVED), q, true, 0, 0); g.fail++; }
    }
  }
  if (c.err) return true;
  // the LHS values no RHS value equals (string ids: one pool entry per distinct string)
  uint32_t missing = 0;
  for (uint32_t j = 0; j < lhs.n; j++) {
    const QR l = *qra(c, lhs.off + j * 16);
    if (qkind(l) == QR_UNRESOLVED) continue;
    const uint32_t id = node(c, l.node).b;
    bool found = false;
    for (uint32_t i = 0; i < rhs.n && !found; i++) {
      const QR r = *qra(c, rhs.off + i * 16);
      found = qkind(r) != QR_UNRESOLVED && node(c, r.node).b == id;
    }
    if (!found) missing++;
  }
  if (!missing) {
    g.pass += nl;
    if (VB) for (uint32_t i = 0; i < nl; i++) rec_success(c, clause);
    return true;
  }
  // failure records list the RHS values (selected, in order) after each missing LHS value
  Arr rs = selected(c, rhs);
  if (c.err) return true;
  for (uint32_t j = 0; j < lhs.n && !c.err; j++) {
    const QR l = *qra(c, lhs.off + j * 16);
    if (qkind(l) == QR_UNRESOLVED) continue;
    const uint32_t id = node(c, l.node).b;
    bool found = false;
    for (uint32_t i = 0; i < rs.n && !found; i++) found = node(c, arr_at(c, rs, i)).b == id;
    if (!found) { rec_in(c, clause, l.node, rs.off, rs.n, false, 0); g.fail++; }
  }
  (void)nr;
  return true;
}

// the literal-RHS fast path of binary_operation: true when it decided the clause (g filled)
DEV bool binary_fast(LCtx& c, uint32_t clause, PCRef pc, View rhs, View lhs, Agg& g) {
  g.pass = 0; g.fail = 0; g.empty = false; g.empty_status = ST_SKIP;
  uint32_t rlit, llit;
  // any RHS that is one literal value streams: an inline literal, or a `%var` bound to one (compare_op
  // reads only the views, so the records are the same either way)
  if (lhs.n && is_literal_view(c, rhs, rlit) && !is_literal_view(c, lhs, llit)) {
    const uint32_t tmark = c.tmp;
    const bool done = binary_literal_stream(c, clause, cl_op(pc), cl_not(pc), lhs, rlit, g);
    c.tmp = tmark;
    if (done || c.err) return true;
  }
  return false;
}
// binary_operation past the literal fast path
DEV Agg binary_rest(LCtx& c, uint32_t clause, PCRef pc, View rhs, uint32_t frame, View lhs, Agg g) {
  uint32_t rlit, llit;
  if (GG_IN_FAST && cl_op(pc) == OP_IN && !cl_not(pc) && lhs.n && rhs.n && !is_literal_view(c, lhs, llit) &&
      !is_literal_view(c, rhs, rlit)) {
    const uint32_t tmark = c.tmp;
    const bool done = in_strings_fast(c, clause, lhs, rhs, g);
    c.tmp = tmark;
    if (done) return g;
  }
  uint32_t start = 0, nv = 0;
  if (!compare_op(c, cl_op(pc), cl_not(pc), lhs, rhs, start, nv)) {
    if (!c.err) { g.empty = true; g.empty_status = ST_SKIP; }
    return g;
  }
  for (uint32_t k = 0; k < nv && !c.err; k++) {
    Ver v = vget(c, u32a(c, start)[k]);
    switch (v.kind) {
      case V_LHS_UNRES: rec_cmp(c, clause, v.u, v.u, false, 0, 0); g.fail++; break;
      case V_RHS_UNRES: rec_cmp(c, clause, mk_qr(v.a, QR_RESOLVED), v.u, true, 0, 0); g.fail++; break;
      case V_NOTCMP: rec_cmp(c, clause, mk_qr(v.a, QR_RESOLVED), mk_qr(v.b, QR_RESOLVED), true, v.nc, v.nct); g.fail++; break;
      case V_SUCCESS: {
        const uint32_t np = v.ck == CK_QUERYIN ? v.l_n : 1u;
        g.pass += np;
        if (VB) for (uint32_t i = 0; i < np; i++) rec_success(c, clause);
        break;
      }
      default:
        if (v.ck == CK_VALUE) { rec_cmp(c, clause, mk_qr(v.a, QR_RESOLVED), mk_qr(v.b, QR_RESOLVED), true, 0, 0); g.fail++; }
        else if (v.ck == CK_VALUEIN) { rec_in(c, clause, v.a, 0, 0, true, v.b); g.fail++; }
        else if (v.ck == CK_LISTIN) { rec_in(c, clause, v.a, 0, 0, true, v.b); g.fail++; }
        else {
          for (uint32_t i = 0; i < v.diff_n && !c.err; i++) { rec_in(c, clause, u32a(c, v.diff_off)[i], v.r_off, v.r_n, false, 0); g.fail++; }
        }
        break;
    }
  }
  return g;
}

#if GG_LANE
// Quick filters (QUICK_FILTER): one clause of the conjunction for value `v` -- the values its key path selects
// (eval_context.rs query_retrieval over Key steps, then an unnamed AllValues / AllIndices fan-out) listed on
// the tmp stack as the walker would list them, then eval_access's comparison and status (eval.rs:1040-1225)
// through the same unary_operation / binary_literal_stream.  Records are suppressed by the caller.  Returns a
// status, or QUICK_UNDECIDED when binary_literal_stream does not cover the values (the generic test decides).
static const uint32_t QUICK_UNDECIDED = 0xFFu;
DEV uint32_t quick_clause(LCtx& c, uint32_t cid, uint32_t v) {
  const PCRef pc = PG(c, clauses)[cid];
  const PQuery Q = PG(c, queries)[pc.a];
  const uint32_t t0 = c.tmp;
  uint32_t cur = v, conv = 0;
  bool listed = false;
  for (uint32_t qi = 0; qi < Q.n && !listed; qi++) {
    const PPart part = PG(c, parts)[Q.first + qi];
    if (part.kind == P_THIS) continue;
    const DNode cn = node(c, cur);
    if (part.kind == P_KEY) {
      uint32_t hit = NONE;
      if (cn.kind == K_MAP) hit = map_get_key(c, cur, cn, part, conv);
      if (hit == NONE) { qr_push(c, mk_unres(cur, cn.kind == K_MAP ? R_KEY_NOT_FOUND : R_NOT_STRUCT, pc.a, qi, 0)); listed = true; }
      cur = hit;
      continue;
    }
    // the last step, an unnamed `[*]` / `*`: a list's elements, a map's values (AllValues); a scalar -- or a map
    // under AllIndices -- stands for itself
    if (cn.kind == K_LIST || (cn.kind == K_MAP && part.kind == P_ALL_VALUES)) {
      if (cn.count == 0) qr_push(c, mk_unres(cur, R_NO_MORE_ENTRIES, pc.a, qi, 0));
      for (uint32_t j = 0; j < cn.count; j++) qr_push(c, mk_qr(child(cur, cn, j), QR_RESOLVED));
      listed = true;
    }
  }
  if (!listed) qr_push(c, mk_qr(cur, QR_RESOLVED));
  View lhs; lhs.off = t0; lhs.n = (c.tmp - t0) / 16u;
  Agg g; g.pass = 0; g.fail = 0; g.empty = false; g.empty_status = ST_SKIP;
  const uint32_t op = cl_op(pc);
  uint32_t st = QUICK_UNDECIDED;
  if (!c.err) {
    bool done = true;
    if (op >= OP_EXISTS) g = unary_operation(c, cid, pc, NONE, lhs);
    else done = binary_literal_stream(c, cid, op, cl_not(pc), lhs, pc.b, g);
    if (done && !c.err) {
      if (g.empty) st = g.empty_status;
      else if (Q.match_all) st = g.fail ? ST_FAIL : ST_PASS;
      else st = g.pass ? ST_PASS : ST_FAIL;
    }
  }
  c.tmp = t0;
  return st;
}
// eval_conjunction_clauses (eval.rs:1970-2065) over quick clauses: the filter's status for value `v`, or
// QUICK_UNDECIDED.  No clause can raise, so a failing disjunction decides at once.
DEV uint32_t quick_conj(LCtx& c, uint32_t conj, uint32_t v) {
  const PRange2 cj = PG(c, conjs)[conj];
  uint32_t num_pass = 0, res = NONE;
  c.suppress++;
  for (uint32_t i = 0; i < cj.n && res == NONE; i++) {
    const PRange2 d = PG(c, disjs)[PG(c, disj_refs)[cj.first + i]];
    uint32_t dfails = 0;
    bool passed = false;
    for (uint32_t j = 0; j < d.n; j++) {
      const uint32_t st = quick_clause(c, PG(c, clause_refs)[d.first + j], v);
      if (st == QUICK_UNDECIDED) { res = QUICK_UNDECIDED; break; }
      if (st == ST_PASS) { passed = true; break; }
      if (st == ST_FAIL) dfails++;
    }
    if (res != NONE) break;
    if (passed) num_pass++;
    else if (dfails) res = ST_FAIL;
  }
  c.suppress--;
  if (res != NONE) return res;
  return num_pass ? ST_PASS : ST_SKIP;
}
#endif

DEV Agg binary_operation(LCtx& c, uint32_t clause, PCRef pc, View rhs, uint32_t frame, View lhs) {
  TSCOPE(c, 2);
  Agg g;
  if (binary_fast(c, clause, pc, rhs, lhs, g)) return g;
  return binary_rest(c, clause, pc, rhs, frame, lhs, g);
}

// the control layer: the recursive evaluator
#include "eval_recursive.inc"
