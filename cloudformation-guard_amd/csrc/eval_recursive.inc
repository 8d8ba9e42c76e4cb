// The recursive evaluator: eval_rule -> eval_conj -> clause evaluators -> blocks -> eval_conj ..., with
// query filters, variable resolution and count() re-entering it from the query driver -- a
// function-for-function restatement of guard/src/rules/eval.rs:1837-2065, 1077-1822 and
// eval_context.rs:268-313, 337-924, 1117-1163, functions/collections.rs:6-23 (included at the end of
// eval_core.inc).  Calls save the callee's callee-saved VGPRs to scratch and the kernels need a dynamic
// lane stack (capi.cpp sets 16 KB); stack_guard below keeps the recursion inside it.  An explicit
// continuation-stack variant was built in round 5 and measured 10-15 % slower on cfg2 / cfg4 / cfg5 with
// more write traffic (DESIGN.md 4.1, profiles/r05_machine_ab.log); it was removed in round 6.

// call structure of the clause interpreter (each AMDGPU call saves the callee's callee-saved VGPRs
// to scratch): eval_clause is a dispatcher folded into eval_conj, so a clause costs one call --
// eval_access_call, eval_type_block, eval_block_clause, ... -- not two (GG_CALL_CLAUSE restores the
// separate eval_clause call for A/B); GG_INLINE_CONJ folds eval_conj into its callers
#if GG_CALL_CLAUSE
#define CLAUSE_FN DEVN
#else
#define CLAUSE_FN DEV
#endif
#if GG_INLINE_CONJ
#define CONJ_FN DEV
#else
#define CONJ_FN DEVN
#endif

// forward decls
DEVN void query_retrieval(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv);
DEV View scope_query(LCtx& c, uint32_t frame, uint32_t qid);
DEVN View resolve_variable(LCtx& c, uint32_t frame, uint32_t var);
#ifndef GG_SPLIT_LET
#define GG_SPLIT_LET 1
#endif
#if GG_SPLIT_LET
#define LET_FN DEVN
#else
#define LET_FN DEV
#endif
LET_FN View resolve_let(LCtx& c, uint32_t f, uint32_t fkind, uint32_t var, uint32_t let_idx, uint32_t slot_off);
CONJ_FN uint32_t eval_conj(LCtx& c, uint32_t conj, uint32_t frame);
// GG_FLAT_CONJ: a conjunction whose clauses are all access clauses runs inline at block / condition
// sites (no recursive call, so no callee-saved register traffic per block value); 0 = always call
// the query walker inlined at the access clause's query site (GG_INLINE_WALK), at let resolution
// (GG_INLINE_WALK_LET) and in the nested query driver (GG_INLINE_WALK_NESTED); elsewhere it is a call
#ifndef GG_INLINE_WALK
#define GG_INLINE_WALK 1
#endif
#ifndef GG_INLINE_WALK_LET
#define GG_INLINE_WALK_LET 1
#endif
#ifndef GG_INLINE_WALK_NESTED
#define GG_INLINE_WALK_NESTED 1
#endif
#ifndef GG_FLAT_CONJ
#define GG_FLAT_CONJ 0
#endif
DEV uint32_t eval_conj_site(LCtx& c, uint32_t conj, uint32_t frame);
#if GG_FLAT_CONJ >= 2
#define GG_COND_CONJ eval_conj_site
#else
#define GG_COND_CONJ eval_conj
#endif
DEVN uint32_t eval_rule(LCtx& c, uint32_t rule, uint32_t frame, uint32_t custom_msg);
DEVN View resolve_function(LCtx& c, uint32_t fid, uint32_t frame);
DEVN void map_key_filter(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, const DNode& cn, uint32_t resolver,
                         uint32_t conv, const PPart& part);
DEVN void key_var_step(LCtx& c, const PQuery& Q, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv,
                       const PPart& part);


// a filter's conjunction for one value: records suppressed, temporaries dropped.  Verbose: `conj`
// carries the record kind in its top bits -- Filter/Map#n (check_and_delegate, eval_context.rs:280)
// or Filter/List#n (:758); a scalar under `[*]` (:790-815) makes no record
// FK_SCALAR: a scalar under `[*]` (eval_context.rs:790-815) -- its conjunction is evaluated under the
// enclosing clause's record with no Filter container around it, so its failing clauses are reported
// with that clause (extraction skips only the children of Filter records): records are kept, and
// roll back with the enclosing clause like any nested clause's
DEVN uint32_t filter_test(LCtx& c, uint32_t conj, uint32_t frame) { FCALL(c, 13);
  TSCOPE(c, 5);
  uint32_t mark = c.tmp;
  const uint32_t fk = VB ? conj >> 30 : 0u;
  const bool scalar = (conj & FK_SCALAR) != 0;
  conj &= FK_SCALAR - 1u;
  const uint32_t et = fk == 2u ? EV_FILTER_LIST : EV_FILTER_MAP;
  if (fk) ev_open(c, et, NONE, PG(c, conjs)[conj].n);
  if (!scalar) c.suppress++;
  uint32_t st = eval_conj(c, conj, frame);
  if (!scalar) c.suppress--;
  if (fk) ev_close(c, et, NONE, c.err ? ST_FAIL : st);
  c.tmp = mark;
  return st;
}

#if GG_LANE
// The filter tests of one chunk (64 entries) of a list fan-out, split over the lanes of the document's group
// (LaunchArgs::lane_group > 1: every lane of the group runs the document's tile in step, with a private copy of
// its state).  Lane g of a group of G tests entries g, g + G, ...: the fast-filter shortcut, then -- for a
// COOP_FILTER conjunction, which reads only the value it tests -- the conjunction itself (filter_test in a value
// frame of its own).  The lanes' verdicts are or-ed across the group with xor shuffles, so every lane leaves
// with the chunk's keep / pass masks and the same rec_created count the sequential path would have given
// (walk_chunk, then one RQ_FILTER per undecided entry: eval_context.rs:723-828 Filter over a list, 268-313
// check_and_delegate for map values).  A test that raises an error, or a group that is not all present,
// leaves the chunk to that sequential path unchanged (keep = every entry, pass = none): errors surface at the
// entry and in the order the reference raises them.  The walker parked the level (WS_CHUNK) with its masks
// cleared; they are written back into it here.
DEVN void coop_chunk(LCtx& c, const WState& w, bool alone) {
  WLevel L = walk_load(c, c.wdepth - 1);
  const PQuery Q = PG(c, queries)[w.qid];
  const PPart part = PG(c, parts)[Q.first + L.qi];
  const DNode cn = node(c, L.cur);
  const uint32_t jn = cn.count - L.j0 < 64 ? cn.count - L.j0 : 64;
  const uint64_t full = jn == 64 ? ~0ull : ((1ull << jn) - 1ull);
  if (L.kind == WK_FLIST) c.rec_created += jn;
  const uint32_t rc0 = c.rec_created;
  // the group: G aligned lanes; all must be here (they run one tile in step), else this lane does it alone
  const uint32_t G = g_wave.group, lane = __lane_id();
  const uint64_t present = __ballot(1);
  const uint32_t gbase = lane & ~(G - 1u);
  const uint64_t gmask = (G >= 64u ? ~0ull : ((1ull << G) - 1ull)) << gbase;
  const bool together = !alone && (present & gmask) == gmask;
  const uint32_t step = together ? G : 1u, first = together ? lane - gbase : 0u;
  const uint32_t ffc = fast_ff(c, part.c);
  const bool full_test = (part.c & COOP_FILTER) != 0, rest = (part.c >> 31) != 0, quick = GG_QUICK && (part.c & QUICK_FILTER) != 0;
  const uint32_t tmp0 = c.tmp, nf0 = c.nframes, wd0 = c.wdepth, sup0 = c.suppress, pers0 = c.pers;
  uint64_t rem = 0, pas = 0;
  uint32_t bad = 0;
  // the lanes test different values now: no query inside may split, no chunk below may be shared
  const uint32_t split0 = c.split;
  c.split = 0xFFFFFFFFu;
  for (uint32_t j = first; j < jn; j += step) {
    const uint32_t v = child(L.cur, cn, L.j0 + j);
    const uint64_t bit = 1ull << j;
    const int ff = ffc ? fast_filter(c, ffc - 1, v) : -1;
    if (ff == 0) { rem |= bit; if (L.kind == WK_ACCMAP) c.rec_created++; continue; }
    if (ff == 1 && !rest) { pas |= bit; continue; }
    if (quick) {
      const uint32_t st = quick_conj(c, part.a, v);
      if (c.err) { c.err = 0; c.err_a = 0; c.err_b = 0; c.tmp = tmp0; bad = 1; break; }
      if (st != QUICK_UNDECIDED) {
        if (st == ST_PASS) pas |= bit;
        else { rem |= bit; if (L.kind == WK_ACCMAP) c.rec_created++; }
        continue;
      }
    }
    if (!full_test) continue;   // undecided: the sequential path tests it
    uint32_t st = ST_SKIP;
    const uint32_t f = push_frame(c, F_VALUE, L.resolver, v, NONE);
    if (!c.err) st = filter_test(c, part.a, f);
    c.tmp = tmp0; c.nframes = nf0; c.wdepth = wd0; c.suppress = sup0; c.pers = pers0;
    if (c.err) { c.err = 0; c.err_a = 0; c.err_b = 0; bad = 1; break; }
    if (st == ST_PASS) pas |= bit;
    else { rem |= bit; if (L.kind == WK_ACCMAP) c.rec_created++; }
  }
  c.split = split0;
  uint32_t d = c.rec_created - rc0;
  if (together) {
    for (uint32_t m = 1; m < G; m <<= 1) {
      rem |= ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(rem >> 32), (int)m, (int)G) << 32) |
             (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)rem, (int)m, (int)G);
      pas |= ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(pas >> 32), (int)m, (int)G) << 32) |
             (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)pas, (int)m, (int)G);
      bad |= (uint32_t)__shfl_xor((int)bad, (int)m, (int)G);
      d += (uint32_t)__shfl_xor((int)d, (int)m, (int)G);
    }
  }
  uint64_t keep = full & ~rem, pass = pas;
  if (bad) { keep = full; pass = 0; d = 0; }
  c.rec_created = rc0 + d;
  L.keep_lo = (uint32_t)keep; L.keep_hi = (uint32_t)(keep >> 32);
  L.pass_lo = (uint32_t)pass; L.pass_hi = (uint32_t)(pass >> 32);
  L.fpushed = 0;
  walk_store(c, c.wdepth - 1, L);
}
#endif

DEVN uint32_t walk_run(LCtx& c, WState& w) { return walk_run_body<false>(c, w); }
#if GG_LANE
DEVN uint32_t walk_run_group(LCtx& c, WState& w) { return walk_run_body<true>(c, w); }
#endif

#if GG_LANE
// Split walks: the lanes of a document's group (LaunchArgs::lane_group) walk the entries of a top-level query's
// first fan-out level round robin (eval_core.inc split_skip) and merge their result lists in entry order, so each
// lane leaves with the list the sequential walk gives.  Only a query the compiler marked (PQuery.pad bit 0: no
// captures, `%var` keys or map-key filters -- nothing a walk does besides producing results) and a group that is
// all here; a walk whose entries recorded anything (a filter over a scalar), raised an error or counted ran out
// of room is redone in full by every lane, so records and errors come in the reference's order.
DEV bool split_start(const LCtx& c, uint32_t qid) {
  if (g_wave.group < 2u || !g_wave.split_on || c.split || !(PG(c, queries)[qid].pad & 1u)) return false;
  const uint32_t G = g_wave.group, gbase = __lane_id() & ~(G - 1u);
  const uint64_t gmask = (G >= 64u ? ~0ull : ((1ull << G) - 1ull)) << gbase;
  return (__ballot(1) & gmask) == gmask;
}
DEV uint32_t group_or(uint32_t v, uint32_t G) {
  for (uint32_t m = 1; m < G; m <<= 1) v |= (uint32_t)__shfl_xor((int)v, (int)m, (int)G);
  return v;
}
DEV uint32_t group_sum(uint32_t v, uint32_t G) {
  for (uint32_t m = 1; m < G; m <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)m, (int)G);
  return v;
}
DEV uint32_t group_min(uint32_t v, uint32_t G) {
  for (uint32_t m = 1; m < G; m <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)m, (int)G); v = o < v ? o : v; }
  return v;
}
// the lanes' marked lists [tmp0, c.tmp) merged in entry order into [tmp0, ...); false: redo the walk unsplit
DEVN bool split_merge(LCtx& c, uint32_t tmp0, uint32_t nrec0, uint32_t naux0, uint32_t nsyn0, uint32_t rc0) {
  const uint32_t G = g_wave.group, lane = __lane_id(), gbase = lane & ~(G - 1u);
  const uint32_t tend = c.tmp;
  uint32_t bad = (c.err || c.nrec != nrec0 || c.naux != naux0 || c.nsyn != nsyn0) ? 1u : 0u;
  // a walk that never reached a fan-out level has no markers: every lane holds the same list
  const uint32_t marked = group_or(!bad && tend > tmp0 && qra(c, tmp0)->meta == QR_MARK ? 1u : 0u, G);
  bad = group_or(bad, G);
  if (bad) return false;
  if (!marked) return true;
  uint32_t mine = 0;
  for (uint32_t o = tmp0; o < tend; o += 16) mine += qra(c, o)->meta != QR_MARK ? 1u : 0u;
  const uint32_t total = group_sum(mine, G);
  if (group_or(tend + 16u * total > c.pers ? 1u : 0u, G)) return false;
  uint32_t cur = tmp0, out = tend;
  for (;;) {
    // round r: entries rG .. rG + G - 1, entry rG + g walked by lane g (if it was handed out at all)
    const uint32_t mi = cur < tend ? qra(c, cur)->node : NONE;
    const uint32_t r = group_min(mi == NONE ? NONE : mi / G, G);
    if (r == NONE) break;
    const bool has = mi != NONE && mi / G == r;
    const uint32_t s = cur + 16u;
    uint32_t n = 0;
    if (has) {
      while (s + 16u * n < tend && qra(c, s + 16u * n)->meta != QR_MARK) n++;
      cur = s + 16u * n;
    }
    uint32_t mx = n;
    for (uint32_t m = 1; m < G; m <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)mx, (int)m, (int)G); mx = o > mx ? o : mx; }
    uint32_t rt = 0;
    for (uint32_t i = 0; i < mx; i++) {
      QR q; q.node = 0; q.meta = 0; q.uref = 0; q.aux = 0;
      if (i < n) q = *qra(c, s + 16u * i);
      uint32_t acc = 0;
      for (uint32_t o = 0; o < G; o++) {
        const int src = (int)(gbase + o);
        const uint32_t no = (uint32_t)__shfl((int)n, src);
        QR x;
        x.node = (uint32_t)__shfl((int)q.node, src); x.meta = (uint32_t)__shfl((int)q.meta, src);
        x.uref = (uint32_t)__shfl((int)q.uref, src); x.aux = (uint32_t)__shfl((int)q.aux, src);
        if (i < no) *qra(c, out + 16u * (acc + i)) = x;
        acc += no;
      }
      rt = acc;
    }
    out += 16u * rt;
  }
  for (uint32_t i = 0; i < total; i++) *qra(c, tmp0 + 16u * i) = *qra(c, tend + 16u * i);
  c.tmp = tmp0 + 16u * total;
  c.rec_created = rc0 + group_sum(c.rec_created - rc0, G);
  return true;
}
#endif

// one walk of query qid from step qi at node cur to the end: the walker and the requests it parks on
template <bool IW>
DEV void walk_all(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv) {
  WState w;
  w.qi = qi; w.qid = qid; w.cur = cur; w.resolver = resolver; w.conv = conv; w.wbase = c.wdepth;
  w.site = WS_START; w.ra = 0; w.rb = 0; w.st = 0; w.voff = 0; w.vn = 0;
#if GG_LANE
  bool parked = false;   // at a shared chunk, waiting for the rest of the group
#endif
  for (;;) {
#if GG_LANE
    const uint32_t rq = parked ? (uint32_t)RQ_CHUNK
                               : (g_wave.group > 1u ? walk_run_group(c, w) : (IW ? walk_run_body<false>(c, w) : walk_run(c, w)));
#else
    const uint32_t rq = IW ? walk_run_body<false>(c, w) : walk_run(c, w);
#endif
    if (rq == RQ_DONE) break;
#if GG_LANE
    if (g_wave.group > 1u) {
      // In a split walk the lanes reach the split level's chunks after different numbers of requests (each
      // serves the filters of its own entries): a lane at a chunk waits until no lane of its group is still
      // walking, so the group tests the chunk together instead of each lane testing it alone
      const uint32_t G = g_wave.group, gbase = __lane_id() & ~(G - 1u);
      const uint64_t gmask = (G >= 64u ? ~0ull : ((1ull << G) - 1ull)) << gbase;
      const uint64_t walking = __ballot(rq != RQ_CHUNK) & gmask;
      if (rq == RQ_CHUNK) {
        parked = walking != 0;
        if (!parked) coop_chunk(c, w, false);
        continue;
      }
      // a quick filter's chunk below the split level: this lane's own (it counted as walking above)
      if (rq == RQ_QCHUNK) { coop_chunk(c, w, true); continue; }
    } else if (rq == RQ_CHUNK) {
      coop_chunk(c, w, false);
      continue;
    }
    // inside a split walk the group's lanes serve requests for different entries: the walks those requests
    // start (filters, lets) neither split nor share chunks, and cannot mistake their levels for the split level
    const uint32_t sp = c.split;
    if (sp) c.split = 0xFFFFFFFFu;
#endif
    if (rq == RQ_FILTER) {
      w.st = filter_test(c, w.ra, w.rb);
    } else if (rq == RQ_VAR) {
      View v = resolve_variable(c, w.resolver, w.ra);
      w.voff = v.off; w.vn = v.n;
    } else {
      const PQuery Q = PG(c, queries)[w.qid];
      const PPart part = PG(c, parts)[Q.first + w.qi];
      if (rq == RQ_KEYVAR) {
        key_var_step(c, Q, w.qi, w.qid, w.cur, w.resolver, w.conv, part);
      } else {
        const DNode cn = node(c, w.cur);
        map_key_filter(c, w.qi, w.qid, w.cur, cn, w.resolver, w.conv, part);
      }
    }
#if GG_LANE
    if (sp) c.split = sp;
#endif
  }
}

#if GG_LANE
// a split walk (split_start said yes): the group shares out the first fan-out's entries, then merges; redone
// in full by every lane when split_merge refuses.  A call of its own, so the common walks carry none of it.
DEVN void split_walk(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv) {
  // a `%var` head first (the walk's first request, its let evaluated lazily): resolved here, with the whole
  // group still in step, its own walk may split too; the split walk then finds it cached
  if (qi == 0) {
    const PPart p0 = PG(c, parts)[PG(c, queries)[qid].first];
    if (p0.kind == P_VAR_HEAD) (void)resolve_variable(c, resolver, p0.a);
  }
  const uint32_t tmp0 = c.tmp, nrec0 = c.nrec, naux0 = c.naux, nsyn0 = c.nsyn, rc0 = c.rec_created;
  const uint32_t nf0 = c.nframes, wd0 = c.wdepth, sup0 = c.suppress;
  c.split = c.wdepth + 1u;
  walk_all<false>(c, qi, qid, cur, resolver, conv);
  c.split = 0;
  if (split_merge(c, tmp0, nrec0, naux0, nsyn0, rc0)) return;
  // redo: every lane walks every entry (the reference's order of records and errors)
  c.tmp = tmp0; c.err = 0; c.err_a = 0; c.err_b = 0; c.nrec = nrec0; c.naux = naux0; c.nsyn = nsyn0;
  c.rec_created = rc0; c.nframes = nf0; c.wdepth = wd0; c.suppress = sup0;
  walk_all<false>(c, qi, qid, cur, resolver, conv);
}
#endif

DEV uint32_t eval_block(LCtx& c, uint32_t block, uint32_t frame);
#if GG_LANE && GG_REC_INTERLEAVE
// Split blocks: a block clause over a document's values (eval_general_block_clause's per-value loop, eval.rs
// 1303-1426) whose block the compiler marked (PClause.c = 1: access clauses reading only the value) is shared
// out by the document's lane group -- lane g evaluates values g, g + G, ... with its records kept privately
// (Ctx::mute private mode), then the group writes every value's records to the leader's record slots in value
// order (prefix sums per round of G values).  Returns 0 with the state restored when the sequential loop has to
// run instead (a value raised an error or made side records / count() values, or the private records would meet
// the leader's); else 1 | 2 (some value FAILed) | 4 (some value PASSed).
// The group's private records (Ctx::mute private mode) written to the leader's record slots in value order: round
// r holds values rG .. rG + G - 1, value rG + g from lane g, whose record count is u32 r of `cnt` (tmp); its records
// land after those of every earlier value, from slot `base` on.  Each lane reads its own private records from
// private index `src0` on (private record k at staging slot rec_slots - 1 - A0 - k).  Returns the records written.
DEV uint32_t group_merge(LCtx& c, uint32_t R0, uint32_t A0, uint32_t base, uint32_t src0, uint32_t rounds,
                         uint32_t nvals, uint32_t cnt) {
  (void)R0;
  const uint32_t G = g_wave.group, lane = __lane_id(), gbase = lane & ~(G - 1u), g = lane - gbase;
  const uint32_t slots = C_RCAP(c) / (uint32_t)sizeof(Rec), ch = rec_chunk_slots();
  uint32_t at0 = base, src = src0;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t n = r * G + g < nvals ? u32a(c, cnt)[r] : 0u;
    uint32_t incl = n;
    for (uint32_t d = 1; d < G; d <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, d, (int)G);
      if (g >= d) incl += v;
    }
    const uint32_t tot = (uint32_t)__shfl((int)incl, (int)(G - 1u), (int)G);
    const uint32_t at = at0 + incl - n;
    for (uint32_t k = 0; k < n; k++) {
      Rec x;
      const gU4* q = stage_ptr(lane, slots - 1u - A0 - (src + k));
      for (uint32_t w = 0; w < sizeof(Rec) / 16; w++) ((uint4*)&x)[w] = q[w];
      const uint32_t dst = at + k;
      gU4* d;
      if (dst < ch) d = c.rbase != NONE ? (gU4*)(g_wave.recs + c.rbase + (size_t)dst * g_wave.rstride) : nullptr;
      else d = stage_ptr(gbase, dst - ch);
      if (d) for (uint32_t w = 0; w < sizeof(Rec) / 16; w++) d[w] = ((const uint4*)&x)[w];
    }
    src += n;
    at0 += tot;
  }
  return at0 - base;
}
DEV bool split_block_start(const LCtx& c, uint32_t nvals) {
  if (g_wave.group < 2u || !g_wave.split_on || c.split || nvals < 2u) return false;
  const uint32_t G = g_wave.group, gbase = __lane_id() & ~(G - 1u);
  const uint64_t gmask = (G >= 64u ? ~0ull : ((1ull << G) - 1ull)) << gbase;
  return (__ballot(1) & gmask) == gmask;
}
DEVN uint32_t split_block(LCtx& c, uint32_t cid, uint32_t block, uint32_t frame, View vals) {
  const uint32_t G = g_wave.group, lane = __lane_id(), gbase = lane & ~(G - 1u), g = lane - gbase;
  const uint32_t R0 = c.nrec, A0 = c.naux, S0 = c.nsyn, rc0 = c.rec_created, tmp0 = c.tmp, nf0 = c.nframes;
  const uint32_t wd0 = c.wdepth, sup0 = c.suppress, pers0 = c.pers, ff0 = c.ffok, mute0 = c.mute, split0 = c.split;
  const uint32_t rounds = (vals.n + G - 1u) / G;
  const uint32_t cnt = alloc_tmp(c, 4u * rounds);   // records of each owned value
  uint32_t fails = 0, passes = 0;
  if (!c.err) {
    c.mute = 2u | (R0 << 2);
    c.split = 0xFFFFFFFFu;   // the lanes evaluate different values: nothing inside splits or shares chunks
    for (uint32_t r = 0; r < rounds && !c.err; r++) {
      const uint32_t i = r * G + g, n0 = c.nrec;
      if (i < vals.n) {
        const QR e = *qra(c, vals.off + i * 16);
        if (qkind(e) == QR_UNRESOLVED) {
          fails++;
          c.rec_created++;
          Rec x = mk_rec(REC_MISSING_BLOCK_VALUE, cid); x.from = e; rec_push(c, x);
        } else {
          const uint32_t t = c.tmp;
          const uint32_t f = push_frame(c, F_VALUE, frame, e.node, NONE);
          if (c.err) break;
          const uint32_t st = eval_block(c, block, f);
          pop_frame(c);
          c.tmp = t;
          if (st == ST_PASS) passes++; else if (st == ST_FAIL) fails++;
        }
      }
      u32a(c, cnt)[r] = c.nrec - n0;
    }
    c.mute = mute0; c.split = split0;
  }
  uint32_t bad = (c.err || c.naux != A0 || c.nsyn != S0) ? 1u : 0u;
  bad = group_or(bad, G);
  const uint32_t mine = c.nrec - R0;
  const uint32_t total = bad ? 0u : group_sum(mine, G);
  const uint32_t slots = C_RCAP(c) / (uint32_t)sizeof(Rec), ch = rec_chunk_slots();
  const uint32_t staged0 = R0 > ch ? R0 - ch : 0u;
  const uint32_t end = R0 + total, staged = end > ch ? end - ch : 0u;
  if (!bad && staged + A0 > slots) {
    // the sequential loop runs out of record room too: the tile goes to the wave kernel (E_RECORDS)
    c.tmp = tmp0; c.nframes = nf0; c.wdepth = wd0; c.suppress = sup0; c.pers = pers0; c.ffok = ff0;
    c.nrec = R0;
    fail(c, E_RECORDS);
    return 1u;
  }
  // the leader's private records must stay clear of the slots the merge writes below them
  const uint32_t lead = (uint32_t)__shfl((int)mine, (int)gbase);
  if (bad || staged + A0 + lead > slots) {
    c.tmp = tmp0; c.err = 0; c.err_a = 0; c.err_b = 0; c.nrec = R0; c.naux = A0; c.nsyn = S0; c.rec_created = rc0;
    c.nframes = nf0; c.wdepth = wd0; c.suppress = sup0; c.pers = pers0; c.ffok = ff0;
    return 0u;
  }
  (void)staged0;
  group_merge(c, R0, A0, R0, 0u, rounds, vals.n, cnt);
  __threadfence_block();
  c.nrec = end;
  c.rec_created = rc0 + group_sum(c.rec_created - rc0, G);
  fails = group_sum(fails, G);
  passes = group_sum(passes, G);
  c.tmp = tmp0; c.nframes = nf0; c.wdepth = wd0; c.suppress = sup0; c.pers = pers0; c.ffok = ff0;
  return 1u | (fails ? 2u : 0u) | (passes ? 4u : 0u);
}

// Split comparisons: an access clause's comparison over a long value list -- unary_operation, or
// binary_literal_stream against one literal (eval.rs:1040-1225; operators.rs per-value compare) -- shared out by the
// document's lane group like a split block: lane g compares values g, g + G, ... with its records kept privately,
// then the group writes them to the leader's slots in the reference's order (a literal comparison's unresolved
// values first, then every value's comparison, each in value order) and sums the counts.  false (state unchanged):
// the sequential comparison runs -- a shape binary_literal_stream leaves to compare_op, an error, side records or
// count() values, or private records that would meet the leader's.  Else 1 << 63 | fails << 32 | passes.
DEVN uint64_t split_compare(LCtx& c, uint32_t cid, PCRef pc, View rhs, View lhs) {
  const uint32_t op = cl_op(pc);
  const bool unary = op >= OP_EXISTS;
  uint32_t rlit = NONE, llit;
  if (unary) {
    if (cl_empty_expr(pc) && op == OP_EMPTY) return 0;
  } else {
    if (!is_literal_view(c, rhs, rlit) || is_literal_view(c, lhs, llit)) return 0;
    const DNode rn = node(c, rlit);
    if (op == OP_IN ? rn.kind != K_LIST : (rn.kind == K_LIST && (op != OP_EQ || rn.count != 1))) return 0;
  }
  const uint32_t G = g_wave.group, lane = __lane_id(), gbase = lane & ~(G - 1u), g = lane - gbase;
  const uint32_t rounds = (lhs.n + G - 1u) / G;
  // IN over a literal list takes scalar values only (binary_literal_stream): any other value -> compare_op for all
  if (op == OP_IN) {
    uint32_t other = 0;
    for (uint32_t r = 0; r < rounds; r++) {
      const uint32_t i = r * G + g;
      if (i >= lhs.n) break;
      const QR q = *qra(c, lhs.off + i * 16);
      if (qkind(q) != QR_UNRESOLVED && !is_scalar_k(node(c, q.node).kind)) other = 1;
    }
    if (group_or(other, G)) return 0;
  }
  const uint32_t R0 = c.nrec, A0 = c.naux, S0 = c.nsyn, rc0 = c.rec_created, tmp0 = c.tmp, mute0 = c.mute, split0 = c.split;
  const uint32_t cnt1 = alloc_tmp(c, 4u * rounds), cnt2 = alloc_tmp(c, 4u * rounds);
  uint32_t pass = 0, fail_n = 0, mine1 = 0;
  if (!c.err) {
    c.mute = 2u | (R0 << 2);
    c.split = 0xFFFFFFFFu;
    // a literal comparison's unresolved values first (their records precede every comparison's)
    for (uint32_t r = 0; r < rounds && !c.err; r++) {
      const uint32_t i = r * G + g, n0 = c.nrec;
      if (!unary && i < lhs.n) {
        const QR q = *qra(c, lhs.off + i * 16);
        if (qkind(q) == QR_UNRESOLVED) { rec_cmp(c, cid, q, q, false, 0, 0); fail_n++; }
      }
      u32a(c, cnt1)[r] = c.nrec - n0;
    }
    mine1 = c.nrec - R0;
    for (uint32_t r = 0; r < rounds && !c.err; r++) {
      const uint32_t i = r * G + g, n0 = c.nrec;
      if (i < lhs.n) {
        View one; one.off = lhs.off + i * 16; one.n = 1;
        const uint32_t t = c.tmp;
        if (unary) {
          const Agg a = unary_operation(c, cid, pc, NONE, one);
          pass += a.pass; fail_n += a.fail;
        } else if (qkind(*qra(c, one.off)) != QR_UNRESOLVED) {
          Agg a; a.pass = 0; a.fail = 0; a.empty = false; a.empty_status = ST_SKIP;
          (void)binary_literal_stream(c, cid, op, cl_not(pc), one, rlit, a);
          pass += a.pass; fail_n += a.fail;
        }
        c.tmp = t;
      }
      u32a(c, cnt2)[r] = c.nrec - n0;
    }
    c.mute = mute0; c.split = split0;
  }
  uint32_t bad = (c.err || c.naux != A0 || c.nsyn != S0) ? 1u : 0u;
  bad = group_or(bad, G);
  const uint32_t mine = c.nrec - R0;
  const uint32_t total1 = bad ? 0u : group_sum(mine1, G), total = bad ? 0u : group_sum(mine, G);
  const uint32_t slots = C_RCAP(c) / (uint32_t)sizeof(Rec), ch = rec_chunk_slots();
  const uint32_t end = R0 + total, staged = end > ch ? end - ch : 0u;
  const uint32_t lead = (uint32_t)__shfl((int)mine, (int)gbase);
  if (bad || staged + A0 + lead > slots) {
    c.tmp = tmp0; c.err = 0; c.err_a = 0; c.err_b = 0; c.nrec = R0; c.naux = A0; c.nsyn = S0; c.rec_created = rc0;
    return 0;
  }
  group_merge(c, R0, A0, R0, 0u, rounds, lhs.n, cnt1);
  group_merge(c, R0, A0, R0 + total1, mine1, rounds, lhs.n, cnt2);
  __threadfence_block();
  c.nrec = end;
  c.rec_created = rc0 + group_sum(c.rec_created - rc0, G);
  pass = group_sum(pass, G);
  fail_n = group_sum(fail_n, G);
  c.tmp = tmp0;
  return (1ull << 63) | ((uint64_t)(fail_n & 0x7FFFFFFFu) << 32) | pass;
}
#endif

// IW: the walker runs inline (its registers belong to the caller's frame, whose callee-saved set
// is already saved) instead of as a call that saves and restores the callee-saved VGPRs it uses
// (26 + 2 per entry) -- the access clause's queries, one site per conjunction dispatcher.  TOP: a clause's,
// block's or let's own query, which a lane group may split (nested queries never are)
template <bool IW, bool TOP = false>
DEV void query_retrieval_body(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv) {
  CHK(c);
  TSCOPE(c, 1);
  STAT(c, 2);
  if (stack_low(c)) { fail(c, E_STACK); return; }
#if GG_LANE
  if (TOP && g_wave.group > 1u && split_start(c, qid)) { split_walk(c, qi, qid, cur, resolver, conv); return; }
#endif
  walk_all<IW>(c, qi, qid, cur, resolver, conv);
}
DEVN void query_retrieval(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv) { FCALL(c, 6);
  query_retrieval_body<(GG_INLINE_WALK_NESTED != 0)>(c, qi, qid, cur, resolver, conv);
}
// scope_query (a clause's / block's / let's top-level query) runs the query driver inline; nested
// queries (filters, %var keys, key captures) call it.  GG_INLINE_QR=0 restores the call.
#ifndef GG_INLINE_QR
#define GG_INLINE_QR 1
#endif
#if GG_INLINE_QR
#define QR_TOP query_retrieval_body<IW, true>
#else
#define QR_TOP query_retrieval
#endif

// `%var` key interpolation step (eval_context.rs:420-526): rare, kept as plain recursion
DEVN void key_var_step(LCtx& c, const PQuery& Q, uint32_t qi, uint32_t qid, uint32_t cur, uint32_t resolver, uint32_t conv,
                       const PPart& part) { FCALL(c, 12);
  View keys = resolve_variable(c, resolver, part.a);
  if (c.err) return;
  uint32_t first = 0, last = keys.n;
  if (qi + 1 < Q.n) {
    PPart nx = PG(c, parts)[Q.first + qi + 1];
    if (nx.kind == P_ALL_INDICES || nx.kind == P_KEY || nx.kind == P_KEY_INDEX || nx.kind == P_KEY_VAR) {
    } else if (nx.kind == P_INDEX) {
      int32_t ix = (int32_t)nx.a;
      uint32_t check = (uint32_t)(ix >= 0 ? ix : -ix);
      if (check < keys.n) { first = check; last = check + 1; }
      else {
        // R4 (eval_context.rs:430-437): the text lists every key (Debug), kept in side records
        Rec h = mk_rec(REC_AUX, part.a); h.x = keys.n; h.y = check;
        const uint32_t ai = aux_push(c, h);
        for (uint32_t i = 0; i < keys.n && !c.err; i += 2) {
          Rec pr = mk_rec(REC_AUX, part.a);
          pr.from = *qra(c, keys.off + i * 16);
          if (i + 1 < keys.n) pr.to = *qra(c, keys.off + (i + 1) * 16);
          aux_push(c, pr);
        }
        if (!c.err) qr_push(c, mk_unres(cur, R_VAR_INDEX_OOB, qid, qi, ai));
        return;
      }
    } else {
      fail(c, E_INTERP_QUERY, qid, qi); return;
    }
  }
  for (uint32_t i = first; i < last && !c.err; i++) {
    QR k = *qra(c, keys.off + i * 16);
    if (qkind(k) == QR_UNRESOLVED) {
      // R5 (eval_context.rs:448-458): the text needs the unresolved key's own path and reason
      Rec h = mk_rec(REC_AUX, part.a); h.from = k;
      const uint32_t ai = aux_push(c, h);
      if (!c.err) qr_push(c, mk_unres(cur, R_VAR_KEYS_UNRESOLVED, qid, qi, ai));
      continue;
    }
    DNode kn = node(c, k.node);
    if (kn.kind == K_STRING) {
      uint32_t hit = map_get(c, cur, bytes_of(c, k.node) + kn.a, kn.count, kn.b);
      if (hit != NONE) query_retrieval(c, qi + 1, qid, hit, resolver, conv);
      else qr_push(c, mk_unres(cur, R_LOCATE_KEY, qid, qi, k.node));
    } else if (kn.kind == K_LIST) {
      for (uint32_t j = 0; j < kn.count && !c.err; j++) {
        uint32_t inner = child(k.node, kn, j);
        DNode in = node(c, inner);
        if (in.kind != K_STRING) { fail(c, E_INTERP_NON_STRING, k.node, qid); break; }
        uint32_t hit = map_get(c, cur, bytes_of(c, inner) + in.a, in.count, in.b);
        if (hit != NONE) query_retrieval(c, qi + 1, qid, hit, resolver, conv);
        else qr_push(c, mk_unres(cur, R_LOCATE_KEY_LIST, qid, qi, inner));
      }
    } else {
      fail(c, E_INTERP_NON_STRING, k.node, qid);
    }
  }
}

// EvalContext::query for a frame
template <bool IW>
DEV View scope_query_t(LCtx& c, uint32_t frame, uint32_t qid) {
  View v; v.off = c.tmp; v.n = 0;
  uint32_t f = frame;
  uint4 F = fhot(c, f);
  while (F.x == F_PARAM) { f = F.y; F = fhot(c, f); }
  uint32_t start = c.tmp;
  QR_TOP(c, 0, qid, F.z, F.x == F_VALUE ? F.y : f, 0);
  v.off = start;
  v.n = (c.tmp - start) / 16;
  return v;
}

DEV View scope_query(LCtx& c, uint32_t frame, uint32_t qid) { return scope_query_t<false>(c, frame, qid); }


// scope variable resolution (RootScope/BlockScope/ValueScope/ResolvedParameterContext)
// a query or function let's first evaluation, cached in its frame (slot_off) or, at the root, in
// the resolved-variable table: a call of its own, so resolve_variable's cache hits -- most of its
// calls -- run in a small frame while this one holds the inlined walker (GG_INLINE_WALK_LET)
LET_FN View resolve_let(LCtx& c, uint32_t f, uint32_t fkind, uint32_t var, uint32_t let_idx, uint32_t slot_off) {
  View none; none.off = 0; none.n = 0;
  PLet L = PG(c, lets)[let_idx];
  uint32_t mark = c.tmp;
  View r;
  if (L.kind == L_FUNC) {
    r = resolve_function(c, L.id, f);
  } else {
    r = scope_query_t<(GG_INLINE_WALK_LET != 0)>(c, f, L.id);
    if (!c.err && !PG(c, queries)[L.id].match_all) {
      // `some` lets keep only Resolved results (eval_context.rs:1148-1158)
      uint32_t k = 0;
      for (uint32_t i = 0; i < r.n; i++) {
        QR q = *qra(c, r.off + i * 16);
        if (qkind(q) == QR_RESOLVED) *qra(c, r.off + (k++) * 16) = q;
      }
      r.n = k;
    }
  }
  if (c.err) return none;
  View p = persist_view(c, r);
  c.tmp = mark;
  if (c.err) return none;
  if (fkind == F_ROOT) {
    // resolved_variables.insert: replaces any key captured into this name while the query ran
    U32View vs = u32a(c, c.vtab + var * 16u);
    vs[0] = 1; vs[1] = p.off; vs[2] = p.n; vs[3] = p.n;
    return p;
  }
  U32View slot = u32a(c, slot_off);
  slot[0] = 1; slot[1] = p.off; slot[2] = p.n;
  return p;
}

DEVN View resolve_variable(LCtx& c, uint32_t frame, uint32_t var) { FCALL(c, 9);
  TSCOPE(c, 6);
  View none; none.off = 0; none.n = 0;
  uint32_t f = frame;
  for (uint32_t guard = 0; guard < 4096; guard++) {
    const uint4 H = fhot(c, f);
    if (H.x == F_VALUE) { f = H.y; continue; }
    Frame F = fget(c, f);
    if (F.kind == F_PARAM) {
      PParamRule pr = PG(c, params)[F.prule];
      for (uint32_t i = 0; i < pr.nparams; i++) {
        if (PG(c, param_vars)[pr.first_param + i] == var) {
          View v; v.off = u32a(c, F.params)[i * 2]; v.n = u32a(c, F.params)[i * 2 + 1];
          return v;
        }
      }
      f = F.parent; continue;
    }
    // ROOT / BLOCK: literal (last) > cached > function (last) > query (last)  (extract_variables)
    PBlock B = PG(c, blocks)[F.block];
    uint32_t lit_i = NONE, fn_i = NONE, q_i = NONE;
    for (uint32_t i = 0; i < B.nlets; i++) {
      PLet L = PG(c, lets)[B.first_let + i];
      if (L.var != var) continue;
      if (L.kind == L_LITERAL) lit_i = i; else if (L.kind == L_FUNC) fn_i = i; else q_i = i;
    }
    if (F.kind == F_ROOT && lit_i == NONE) {
      // RootScope::resolve_variable (eval_context.rs:1117-1163): resolved_variables (query / function
      // lets already resolved, and key captures) before evaluating a let
      U32View vs = u32a(c, c.vtab + var * 16u);
      if (vs[0]) { View v; v.off = vs[1]; v.n = vs[2]; return v; }
    }
    if (lit_i != NONE) {
      U32View slot = u32a(c, F.cache + lit_i * 16);
      if (slot[0] == 0) {
        uint32_t o = alloc_pers(c, 16);
        if (c.err) return none;
        *qra(c, o) = mk_qr(PG(c, lets)[B.first_let + lit_i].id, QR_LITERAL);
        slot = u32a(c, F.cache + lit_i * 16);
        slot[0] = 1; slot[1] = o; slot[2] = 1;
      }
      View v; v.off = slot[1]; v.n = slot[2]; return v;
    }
    uint32_t use = fn_i != NONE ? fn_i : q_i;
    if (use == NONE) {
      if (F.kind == F_ROOT) { fail(c, E_VAR_MISSING, var); return none; }
      f = F.parent; continue;
    }
    U32View slot = u32a(c, F.cache + use * 16);
    if (slot[0] == 1) { View v; v.off = slot[1]; v.n = slot[2]; return v; }
    return resolve_let(c, f, F.kind, var, B.first_let + use, F.cache + use * 16);
  }
  fail(c, E_DEPTH);
  return none;
}

// count() (functions/collections.rs:6-23); other functions are outside the MI355X path
DEVN View resolve_function(LCtx& c, uint32_t fid, uint32_t frame) { FCALL(c, 10);
  PFunc F = PG(c, funcs)[fid];
  View out; out.off = c.tmp; out.n = 0;
  if (stack_low(c)) { fail(c, E_STACK); return out; }   // count(count(...)) nests without a clause
  if (F.fname != F_COUNT || F.nargs != 1) { fail(c, E_UNSUPPORTED, 7); return out; }
  PLet A = PG(c, lets)[F.first_arg];
  View arg;
  if (A.kind == L_LITERAL) {
    arg.off = alloc_tmp(c, 16); arg.n = 1;
    if (c.err) return out;
    *qra(c, arg.off) = mk_qr(A.id, QR_LITERAL);
  } else if (A.kind == L_QUERY) {
    arg = scope_query(c, frame, A.id);
  } else {
    arg = resolve_function(c, A.id, frame);
  }
  if (c.err) return out;
  uint32_t cnt = 0;
  for (uint32_t i = 0; i < arg.n; i++) if (qkind(*qra(c, arg.off + i * 16)) != QR_UNRESOLVED) cnt++;
  uint32_t src = NONE;
  if (arg.n) src = qra(c, arg.off)->node;
  if (c.nsyn >= 256) { fail(c, E_HEAP); return out; }
  gU32* s = (gU32*)haddr(c, C_SYN(c) + 16u * c.nsyn);
  s[0] = src; s[1] = cnt; s[2] = 0; s[3] = 0;
  uint32_t ref = SYN_BIT | c.nsyn++;
  out.off = alloc_tmp(c, 16); out.n = 1;
  if (c.err) return out;
  QR q = mk_qr(ref, QR_RESOLVED);
  *qra(c, out.off) = q;
  return out;
}

// MapKeyFilter step (eval_context.rs:830-922): the RHS, the keys compared (map_key_select), then the query
// continued at qi + 1 from each selected entry; results slid down over the temporaries
DEVN void map_key_filter(LCtx& c, uint32_t qi, uint32_t qid, uint32_t cur, const DNode& cn, uint32_t resolver,
                         uint32_t conv, const PPart& part) { FCALL(c, 11);
  const uint32_t m0 = c.tmp;
  View rhs;
  if (part.a == RHS_LITERAL) {
    rhs.off = alloc_tmp(c, 16); rhs.n = 1;
    if (c.err) return;
    *qra(c, rhs.off) = mk_qr(part.b, QR_LITERAL);
  } else if (part.a == RHS_QUERY) {
    uint32_t start = c.tmp;
    query_retrieval(c, 0, part.b, cur, resolver, conv);
    rhs.off = start; rhs.n = (c.tmp - start) / 16;
  } else {
    rhs = resolve_function(c, part.b, resolver);
  }
  if (c.err) return;
  uint32_t sel_off = 0;
  const uint32_t nsel = map_key_select(c, cur, cn, part, rhs, sel_off);
  if (c.err) return;
  uint32_t res0 = c.tmp;
  for (uint32_t k = 0; k < nsel && !c.err; k++) query_retrieval(c, qi + 1, qid, u32a(c, sel_off)[k], resolver, conv);
  if (c.err) return;
  // results must stay contiguous for the caller: slide them over the temporaries
  uint32_t n = (c.tmp - res0) / 4;
  U32View dst = u32a(c, m0);
  U32View src = u32a(c, res0);
  for (uint32_t i = 0; i < n; i++) dst[i] = src[i];
  c.tmp = m0 + n * 4;
}

// ----------------------------------------------------------------- clauses ---
CLAUSE_FN uint32_t eval_clause(LCtx& c, uint32_t cid, uint32_t frame);

// container that is "flattened" into its parent when FAIL and dropped otherwise
DEV void flat_close(LCtx& c, uint32_t mark, uint32_t status) { if (status != ST_FAIL) rec_rollback(c, mark); }

DEV uint32_t eval_access(LCtx& c, uint32_t cid, PCRef pc, uint32_t frame) {
  uint32_t mark = c.nrec;
  uint32_t tmark = c.tmp;
  bool all = PG(c, queries)[pc.a].match_all != 0;
  ev_open(c, EV_GAC, cid);
  Agg g;
  const uint32_t op = cl_op(pc);
  const bool unary = op >= OP_EXISTS;
  const uint32_t rk = unary ? RHS_LITERAL : cl_rhs(pc);
  View rhs; rhs.off = 0; rhs.n = 0;
  if (!unary) {
    if (rk == RHS_LITERAL) {
      rhs.off = alloc_tmp(c, 16); rhs.n = 1;
      if (c.err) return ST_FAIL;
      *qra(c, rhs.off) = mk_qr(pc.b, QR_LITERAL);
    } else if (rk == RHS_FUNC) {
      rhs = resolve_function(c, pc.b, frame);
    } else if (rk != RHS_QUERY) {
      fail(c, E_NO_RHS, cid);
      return ST_FAIL;
    }
    if (c.err) return ST_FAIL;
  }
  // the clause's queries -- a query RHS first, then the LHS (eval.rs:1096-1101, binary_operation) -- through one
  // query-driver site, so the inlined walker (GG_INLINE_WALK) is instantiated once per dispatcher
  View lhs;
  for (uint32_t k = rk == RHS_QUERY ? 0u : 1u; k < 2; k++) {
    const View v = scope_query_t<GG_INLINE_WALK != 0>(c, frame, k ? pc.a : pc.b);
    if (c.err) return ST_FAIL;
    if (k) lhs = v; else rhs = v;
  }
#if GG_LANE && GG_REC_INTERLEAVE
  // a long value list in a lane group: the group shares the comparisons out (split_compare)
  uint64_t sc = 0;
  if (g_wave.group > 1u && lhs.n >= 2u * g_wave.group && split_block_start(c, lhs.n)) sc = split_compare(c, cid, pc, rhs, lhs);
  if (sc) { g.pass = (uint32_t)sc; g.fail = (uint32_t)(sc >> 32) & 0x7FFFFFFFu; g.empty = false; g.empty_status = ST_SKIP; }
  else
#endif
  g = unary ? unary_operation(c, cid, pc, frame, lhs) : binary_operation(c, cid, pc, rhs, frame, lhs);
  c.tmp = tmark;
  if (c.err) return ST_FAIL;
  uint32_t st;
  if (g.empty) st = g.empty_status;
  else if (all) st = g.fail ? ST_FAIL : ST_PASS;
  else st = g.pass ? ST_PASS : ST_FAIL;
  flat_close(c, mark, st);   // GuardClauseBlockCheck
  ev_close(c, EV_GAC, cid, st, g.empty ? all : !all);   // eval.rs:1160-1210
  return st;
}

DEVN uint32_t rule_status(LCtx& c, uint32_t slot) {
  U32View memo = u32a(c, c.memo);
  if (memo[slot] != 3u) return memo[slot];
  PRange2 nr = PG(c, name_rules)[slot];
  uint32_t st = ST_SKIP;
  c.suppress++;
  for (uint32_t i = 0; i < nr.n && !c.err; i++) {
    uint32_t s = eval_rule(c, PG(c, name_rule_ids)[nr.first + i], 0, NONE);
    if (s != ST_SKIP) { st = s; break; }
  }
  c.suppress--;
  if (c.err) return ST_FAIL;
  u32a(c, c.memo)[slot] = st;
  return st;
}

DEV uint32_t eval_named(LCtx& c, uint32_t cid, PCRef pc) {
  if (pc.a == NONE) { fail(c, E_RULE_MISSING, cid); return ST_FAIL; }
  ev_open(c, EV_NAMED, cid);   // the rule's own events (first evaluation) nest inside
  uint32_t st = rule_status(c, pc.a);
  if (c.err) return ST_FAIL;
  bool neg = pc.flags & 1u;
  uint32_t out = st == ST_PASS ? (neg ? ST_FAIL : ST_PASS) : (neg ? ST_PASS : ST_FAIL);
  if (out == ST_FAIL && !VB) rec_push(c, mk_rec(REC_DEPENDENT_RULE, cid));
  ev_close(c, EV_NAMED, cid, out);   // ClauseCheck::Success / DependentRule
  return out;
}

// eval_general_block_clause: BlockScope(block, resolver.root(), resolver)
DEV uint32_t eval_block(LCtx& c, uint32_t block, uint32_t frame) {
  uint32_t root = frame_root(c, frame);
  uint32_t f = push_frame(c, F_BLOCK, frame, root, block);
  if (c.err) return ST_FAIL;
  uint32_t st = eval_conj_site(c, PG(c, blocks)[block].conj, f);
  pop_frame(c);
  return st;
}

// block and type-block clauses: folded into eval_conj's dispatcher (GG_INLINE_BLOCKS), whose
// prologue already saves the whole callee-saved set, instead of calls that save 31-44 more
#ifndef GG_INLINE_BLOCKS
#define GG_INLINE_BLOCKS 1
#endif
#if GG_INLINE_BLOCKS
#define BLOCK_FN DEV
#else
#define BLOCK_FN DEVN
#endif
BLOCK_FN uint32_t eval_block_clause(LCtx& c, uint32_t cid, PCRef pc, uint32_t frame) { FCALL(c, 2);
  uint32_t mark = c.nrec;
  uint32_t created0 = c.rec_created;
  uint32_t tmark = c.tmp;
  bool match_all = PG(c, queries)[pc.a].match_all != 0;
  ev_open(c, EV_BLOCK, cid);
  View vals = scope_query(c, frame, pc.a);
  if (c.err) return ST_FAIL;
  if (vals.n == 0) {
    uint32_t st = (pc.flags & 1u) ? ST_FAIL : ST_SKIP;
    if (st == ST_FAIL && c.rec_created == created0 && !VB) rec_push(c, mk_rec(REC_BLOCK_EMPTY, cid));
    c.tmp = tmark;
    if (st != ST_FAIL) rec_rollback(c, mark);
    ev_close(c, EV_BLOCK, cid, st, !match_all);
    return st;
  }
  uint32_t fails = 0, passes = 0;
#if GG_LANE && GG_REC_INTERLEAVE
  uint32_t sb = 0;
  if (pc.c == 1u && split_block_start(c, vals.n)) sb = split_block(c, cid, pc.b, frame, vals);
  if (sb) { fails = (sb >> 1) & 1u; passes = (sb >> 2) & 1u; }
  for (uint32_t i = sb ? vals.n : 0u; i < vals.n && !c.err; i++) {
#else
  for (uint32_t i = 0; i < vals.n && !c.err; i++) {
#endif
    QR e = *qra(c, vals.off + i * 16);
    if (qkind(e) == QR_UNRESOLVED) {
      fails++;
      c.rec_created++;
      Rec r = mk_rec(REC_MISSING_BLOCK_VALUE, cid); r.from = e; rec_push(c, r);
      continue;
    }
    uint32_t f = push_frame(c, F_VALUE, frame, e.node, NONE);
    if (c.err) break;
    uint32_t st = eval_block(c, pc.b, f);
    pop_frame(c);
    if (st == ST_PASS) passes++; else if (st == ST_FAIL) fails++;
  }
  c.tmp = tmark;
  if (c.err) return ST_FAIL;
  uint32_t st;
  if (match_all) st = fails ? ST_FAIL : (passes ? ST_PASS : ST_SKIP);
  else st = passes ? ST_PASS : (fails ? ST_FAIL : ST_SKIP);
  flat_close(c, mark, st);
  ev_close(c, EV_BLOCK, cid, st, !match_all);   // BlockGuardCheck (eval.rs:1417-1424)
  return st;
}

// eval_when_condition_block (eval.rs:1428-1502)
DEV uint32_t eval_when_block(LCtx& c, uint32_t cid, PCRef pc, uint32_t frame) {
  uint32_t mark = c.nrec;
  ev_open(c, EV_WHEN, cid);
  ev_open(c, EV_WHEN_COND, cid);
  c.suppress++;
  uint32_t cond = GG_COND_CONJ(c, pc.a, frame);
  c.suppress--;
  if (c.err) return ST_FAIL;
  ev_close(c, EV_WHEN_COND, cid, cond);
  if (cond != ST_PASS) { rec_rollback(c, mark); ev_close(c, EV_WHEN, cid, ST_SKIP); return ST_SKIP; }
  uint32_t st = eval_block(c, pc.b, frame);
  if (c.err) return ST_FAIL;
  flat_close(c, mark, st);   // WhenCheck
  ev_close(c, EV_WHEN, cid, st);
  return st;
}

// eval_type_block_clause (eval.rs:1649-1822)
BLOCK_FN uint32_t eval_type_block(LCtx& c, uint32_t cid, PCRef pc, uint32_t frame) { FCALL(c, 3);
  uint32_t mark = c.nrec;
  ev_open(c, EV_TYPE, cid);
  if (pc.c != NONE) {
    ev_open(c, EV_TYPE_COND, cid);
    c.suppress++;
    uint32_t cond = GG_COND_CONJ(c, pc.c, frame);
    c.suppress--;
    if (c.err) return ST_FAIL;
    ev_close(c, EV_TYPE_COND, cid, cond);
    if (cond != ST_PASS) { ev_close(c, EV_TYPE, cid, ST_SKIP); return ST_SKIP; }
  }
  uint32_t tmark = c.tmp;
  View vals = scope_query(c, frame, pc.a);
  if (c.err) return ST_FAIL;
  if (vals.n == 0) { c.tmp = tmark; ev_close(c, EV_TYPE, cid, ST_SKIP); return ST_SKIP; }
  uint32_t fails = 0, passes = 0;
  for (uint32_t i = 0; i < vals.n && !c.err; i++) {
    QR e = *qra(c, vals.off + i * 16);
    if (qkind(e) == QR_UNRESOLVED) { fail(c, E_TYPEBLOCK_UNRESOLVED, cid); break; }
    uint32_t vmark = c.nrec;
    ev_open(c, EV_TYPE_VAL, cid, i);
    uint32_t f = push_frame(c, F_VALUE, frame, e.node, NONE);
    if (c.err) break;
    uint32_t st = eval_block(c, pc.b, f);
    pop_frame(c);
    if (st == ST_PASS) passes++; else if (st == ST_FAIL) fails++;
    flat_close(c, vmark, st);   // TypeBlock(status) per value
    ev_close(c, EV_TYPE_VAL, cid, st);
  }
  c.tmp = tmark;
  if (c.err) return ST_FAIL;
  uint32_t st = fails ? ST_FAIL : (passes ? ST_PASS : ST_SKIP);
  flat_close(c, mark, st);       // TypeCheck
  ev_close(c, EV_TYPE, cid, st);
  return st;
}

DEVN uint32_t eval_param_call(LCtx& c, uint32_t cid, PCRef pc, uint32_t frame) { FCALL(c, 4);
  if (pc.a == NONE) { fail(c, E_PARAM_MISSING, cid); return ST_FAIL; }
  PParamRule pr = PG(c, params)[pc.a];
  if (pr.nparams != pc.c) { fail(c, E_PARAM_ARITY, cid, pr.nparams); return ST_FAIL; }
  uint32_t po = alloc_pers(c, (pr.nparams ? pr.nparams : 1) * 8);
  if (c.err) return ST_FAIL;
  for (uint32_t i = 0; i < pc.c && !c.err; i++) {
    PLet a = PG(c, lets)[pc.b + i];
    View v;
    uint32_t tmark = c.tmp;
    if (a.kind == L_LITERAL) {
      v.off = alloc_tmp(c, 16); v.n = 1;
      if (c.err) break;
      *qra(c, v.off) = mk_qr(a.id, QR_RESOLVED);
    } else if (a.kind == L_QUERY) {
      v = scope_query(c, frame, a.id);
    } else {
      v = resolve_function(c, a.id, frame);
    }
    if (c.err) break;
    View p = persist_view(c, v);
    c.tmp = tmark;
    u32a(c, po)[i * 2] = p.off;
    u32a(c, po)[i * 2 + 1] = p.n;
  }
  if (c.err) return ST_FAIL;
  uint32_t f = push_frame(c, F_PARAM, frame, NONE, NONE);
  if (c.err) return ST_FAIL;
  { Frame F = fget(c, f); F.call = cid; F.params = po; F.prule = pc.a; fput(c, f, F); }
  uint32_t st = eval_rule(c, pr.rule, f, pc.e);
  pop_frame(c);
  return st;
}

// an access clause: inlined into eval_conj's dispatcher (GG_INLINE_ACCESS, default).  Its callee-saved
// registers are then saved once per conjunction instead of once per access clause (a conjunction of
// k access clauses: 48 saves, not 22 + 41 k; cfg-2 lane kernel 61.9 -> 60.5 ms, profiles/r02_ab_inline.log);
// GG_INLINE_ACCESS=0 restores the separate call
#ifndef GG_INLINE_ACCESS
#define GG_INLINE_ACCESS 1
#endif
#if GG_INLINE_ACCESS
DEV
#else
DEVN
#endif
uint32_t eval_access_call(LCtx& c, uint32_t cid, uint32_t frame) {
  PCRef pc = PG(c, clauses)[cid];
  return eval_access(c, cid, pc, frame);
}

// rule references and `when` blocks in their own frame too (keeps the dispatcher in eval_conj lean)
DEVN uint32_t eval_misc_call(LCtx& c, uint32_t cid, uint32_t frame) { FCALL(c, 5);
  PCRef pc = PG(c, clauses)[cid];
  return pc.kind == C_NAMED ? eval_named(c, cid, pc) : eval_when_block(c, cid, pc, frame);
}

#if GG_AB_BURN
// Diagnostic A/B only (never in the product build): a call that clobbers 32 callee-saved VGPRs, so its
// prologue saves 32 callee-saved VGPRs to scratch and its epilogue restores them -- the same traffic
// shape as the interpreter's own calls.  Measures what one clause's worth of save/restore costs.
DEVN uint32_t ab_burn(LCtx& c, uint32_t seed) {
#if GG_AB_BURN_NOCLOB
  asm volatile("" :::);
#else
  asm volatile("" ::: "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95");
#endif
  return seed + c.tmp;
}
#endif
// eval_clause for a clause known to be an access clause (flat conjunctions)
DEV uint32_t eval_clause_access(LCtx& c, uint32_t cid, uint32_t frame) {
  STAT(c, 3);
  if (stack_low(c)) { fail(c, E_STACK); return ST_FAIL; }
  return eval_access_call(c, cid, frame);
}
CLAUSE_FN uint32_t eval_clause(LCtx& c, uint32_t cid, uint32_t frame) {
  STAT(c, 3);
#if GG_AB_BURN
  for (int b = 0; b < GG_AB_BURN; b++)
    if (ab_burn(c, cid + (uint32_t)b) == 0x9E3779B9u) c.nsyn += 0;
#endif
  if (stack_low(c)) { fail(c, E_STACK); return ST_FAIL; }
  PCRef pc = PG(c, clauses)[cid];
  uint32_t st;
  switch (pc.kind) {
    case C_ACCESS: st = eval_access_call(c, cid, frame); break;
    case C_NAMED:
    case C_WHEN: st = eval_misc_call(c, cid, frame); break;
    case C_BLOCK: st = eval_block_clause(c, cid, pc, frame); break;
    case C_TYPEBLOCK: st = eval_type_block(c, cid, pc, frame); break;
    case C_PARAM: st = eval_param_call(c, cid, pc, frame); break;
    default: fail(c, E_UNSUPPORTED, 8); st = ST_FAIL; break;
  }
  return st;
}

// eval_conjunction_clauses (eval.rs:1970-2065).  FLAT: every clause is an access clause (the caller
// checked), dispatched straight to the inlined access evaluation
template <bool FLAT>
DEV uint32_t eval_conj_body(LCtx& c, uint32_t conj, uint32_t frame) {
  PRange2 cj = PG(c, conjs)[conj];
  uint32_t num_pass = 0, num_fail = 0;
  for (uint32_t i = 0; i < cj.n && !c.err; i++) {
    PRange2 d = PG(c, disjs)[PG(c, disj_refs)[cj.first + i]];
    bool multi = d.n > 1;
    uint32_t mark = c.nrec;
    const bool open = multi && rec_reserve(c);
    if (multi) ev_open(c, EV_DISJ, NONE);
    uint32_t dfails = 0;
    bool passed = false;
    for (uint32_t j = 0; j < d.n && !c.err; j++) {
      uint32_t st;
      if constexpr (FLAT) st = eval_clause_access(c, PG(c, clause_refs)[d.first + j], frame);
      else st = eval_clause(c, PG(c, clause_refs)[d.first + j], frame);
      if (c.err) break;
      if (st == ST_PASS) { num_pass++; passed = true; break; }
      if (st == ST_FAIL) dfails++;
    }
    if (c.err) break;
    if (passed) {
      if (multi) { rec_rollback(c, mark); ev_close(c, EV_DISJ, NONE, ST_PASS, true); }
      continue;
    }
    if (dfails) num_fail++;
    if (multi) {
      if (dfails) {
        if (open) rec_fill(c, mark, mk_rec(REC_DISJ_OPEN, 0));
        if (!VB) rec_push(c, mk_rec(REC_DISJ_CLOSE, 0));
      } else rec_rollback(c, mark);
      ev_close(c, EV_DISJ, NONE, dfails ? ST_FAIL : ST_SKIP, true);
    }
  }
  if (c.err) return ST_FAIL;
  if (num_fail) return ST_FAIL;
  if (num_pass) return ST_PASS;
  return ST_SKIP;
}
CONJ_FN uint32_t eval_conj(LCtx& c, uint32_t conj, uint32_t frame) { FCALL(c, 0); return eval_conj_body<false>(c, conj, frame); }
DEV bool conj_flat(LCtx& c, uint32_t conj) {
  const PRange2 cj = PG(c, conjs)[conj];
  for (uint32_t i = 0; i < cj.n; i++) {
    const PRange2 d = PG(c, disjs)[PG(c, disj_refs)[cj.first + i]];
    for (uint32_t j = 0; j < d.n; j++)
      if (PG(c, clauses)[PG(c, clause_refs)[d.first + j]].kind != C_ACCESS) return false;
  }
  return true;
}
DEV uint32_t eval_conj_site(LCtx& c, uint32_t conj, uint32_t frame) {
#if GG_FLAT_CONJ
  if (conj_flat(c, conj)) return eval_conj_body<true>(c, conj, frame);
#endif
  return eval_conj(c, conj, frame);
}

// eval_rule (eval.rs:1837-1906).  frame: 0 = root frame
DEVN uint32_t eval_rule(LCtx& c, uint32_t rid, uint32_t frame, uint32_t custom_msg) { FCALL(c, 1);
  TSCOPE(c, 0);
  PRule R = PG(c, rules)[rid];
  uint32_t mark = c.nrec;
  const bool open = rec_reserve(c);
  ev_open(c, EV_RULE, rid);
  if (R.cond != NONE) {
    ev_open(c, EV_RULE_COND, rid);
    c.suppress++;
    uint32_t cond = GG_COND_CONJ(c, R.cond, frame);
    c.suppress--;
    if (c.err) return ST_FAIL;
    ev_close(c, EV_RULE_COND, rid, cond);
    if (cond != ST_PASS) { rec_rollback(c, mark); ev_close(c, EV_RULE, rid, ST_SKIP, false, custom_msg); return ST_SKIP; }
  }
  uint32_t st = eval_block(c, R.block, frame);
  if (c.err) return ST_FAIL;
  if (st == ST_FAIL) {
    if (open) { Rec o = mk_rec(REC_RULE_OPEN, rid); o.x = custom_msg; rec_fill(c, mark, o); }
    if (!VB) rec_push(c, mk_rec(REC_RULE_CLOSE, rid));
  } else rec_rollback(c, mark);
  ev_close(c, EV_RULE, rid, st, false, custom_msg);
  return st;
}


// the kernels' entry: a top-level rule of the file (eval_rules_file, eval.rs:1915-1968)
DEV uint32_t run_rule(LCtx& c, uint32_t rid) { return eval_rule(c, rid, 0, NONE); }
