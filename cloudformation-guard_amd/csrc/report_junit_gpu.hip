// The device JUnit report writer (`validate --structured -o junit`): report_junit_kernel.  Device restatement
// of ReportWriter::add's OUT_JUNIT case (reporter.cpp; JunitReporter::report, xml.rs:14-80, and get_test_case,
// reporters/mod.rs:108-168): one <testsuite> per document, one <testcase> per rules file, a FAILed file's
// <failure> holding every message of its ClauseReports -- custom message, then error message, nothing between.
//
// report_gpu.hip is included for the record layout and the message text producers (paths, value displays,
// remaining queries, reasons), which are templates over the writer; GG_REPORT_JUNIT leaves its JSON / SARIF /
// YAML writers and kernels out and makes the producers real calls, so this unit compiles in seconds and the
// other kernels keep their code.  The writer here is rg::X: XML escaping and nothing else.
#define GG_REPORT_JUNIT 1
#include "report_gpu.hip"

namespace gg {
namespace rg {

// ------------------------------------------------------------------------------ XML writer ---
// p == null: the size pass.  Text goes through the dot filter (REC_IN's message: '.' dropped before '['),
// then quick_xml's escape of & < > ' "; every other byte, UTF-8 included, passes.  The value displays
// already are the JSON text of a value: no second escaping layer.
struct X {
  char* p;
  uint64_t n;
  uint32_t fb;
  bool dotf, held;
};
RD void raw(X& x, char c) {
  if (x.p) x.p[x.n] = c;
  x.n++;
}
RD void raws(X& x, const char* s) { for (; *s; s++) raw(x, *s); }
RD void emit(X& x, char c) {
  switch (c) {
    case '&': raws(x, "&amp;"); return;
    case '<': raws(x, "&lt;"); return;
    case '>': raws(x, "&gt;"); return;
    case '\'': raws(x, "&apos;"); return;
    case '"': raws(x, "&quot;"); return;
    default: raw(x, c);
  }
}
RD void tput(X& x, char c) {
  if (x.dotf) {
    if (x.held) { x.held = false; if (c != '[') emit(x, '.'); }
    if (c == '.') { x.held = true; return; }
  }
  emit(x, c);
}
// 8 bytes none of which XML escapes: '&' / '\'' (0x26, 0x27) and '<' / '>' (0x3C, 0x3E) differ in one bit
// each, so three zero-byte tests cover the five
RD bool xplain8(uint64_t v) {
  const uint64_t ones = 0x0101010101010101ull, highs = 0x8080808080808080ull;
  const uint64_t a = (v | ones) ^ (ones * 0x27u), l = (v | (ones * 2u)) ^ (ones * 0x3Eu), q = v ^ (ones * 0x22u);
  return !((((a - ones) & ~a) | ((l - ones) & ~l) | ((q - ones) & ~q)) & highs);
}
// n bytes at s; a 16-byte aligned source (the pool and the reporter tables' zero-padded strings) is read 16
// bytes at a time and a chunk without a special character is copied as it is
RD void xbulk(X& x, const char* s, uint32_t n) {
  uint32_t i = 0;
  if ((((uintptr_t)s) & 15u) == 0) {
    for (; i < n; i += 16) {
      const uint4 q = *(const uint4*)(s + i);
      const uint64_t lo = (uint64_t)q.x | ((uint64_t)q.y << 32), hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
      const uint32_t m = n - i < 16 ? n - i : 16;
      const bool plain = xplain8(lo) && xplain8(hi);
#pragma unroll 1
      for (uint32_t k = 0; k < m; k++) {
        const char c = (char)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF);
        if (plain) raw(x, c); else emit(x, c);
      }
    }
    return;
  }
#pragma unroll 1
  for (; i < n; i++) emit(x, s[i]);
}
RD void tstr(X& x, const char* s, uint32_t n) {
  if (!x.dotf) { xbulk(x, s, n); return; }
  for (uint32_t i = 0; i < n; i++) tput(x, s[i]);
}
// COMPOSE(x) { producer }: one message text; its end flushes a held '.' and ends the dot filter
RD uint32_t sbeg(X&) { return 1; }
RD uint32_t send(X& x) {
  if (x.held) { x.held = false; emit(x, '.'); }
  x.dotf = false;
  return 0;
}

// ---------------------------------------------------------------------------------- records ---
// What the <failure> opening needs and only the end of the records gives: the number of messages (each has an
// error message, so "no texts" is "no messages": `<failure ../>`) and the last top-level Rule that held one.
struct JScan { uint32_t nmsg, rule; };

// One FAILed tile's records, the open / close stack of tile_sarif.  scan != null: the pre-scan (counts, writes
// nothing, reads records only).  Else every message's texts in record order -- the (custom_message,
// error_message) pairs of the host's Messages (reporter.cpp Walker::items), Some("") and None both empty.
RN void tile_junit(X& w, const Ctx& c, const RecSeq recs, uint32_t nrec, JScan* scan) {
  uint32_t closes[kMaxDepth];
  uint32_t sp = 0;
  uint32_t rule = NONE;   // the enclosing top-level Rule (its name index), NONE outside one
  uint32_t i = 0;
  while (i < nrec && !w.fb) {
    const Rec rc = recs[i];
    if (sp && rc.kind == closes[sp - 1]) {
      i++;
      if (--sp == 0) rule = NONE;
      continue;
    }
    i++;
    if (rc.kind == REC_RULE_OPEN || rc.kind == REC_DISJ_OPEN) {
      if (sp == kMaxDepth) { w.fb = FB_DEPTH; return; }
      if (sp == 0 && rc.kind == REC_RULE_OPEN) rule = rc.clause;
      closes[sp++] = rc.kind == REC_RULE_OPEN ? REC_RULE_CLOSE : REC_DISJ_CLOSE;
      continue;
    }
    const bool mk = rc.clause == NONE;   // a map-key-filter comparison (REC_CMP / REC_IN): no clause, no custom message
    const bool from_unres = qkind(rc.from) == QR_UNRESOLVED;
    switch (rc.kind) {
      case REC_BLOCK_EMPTY: case REC_MISSING_BLOCK_VALUE: case REC_UNARY: case REC_NOVALUE_EMPTY: case REC_DEPENDENT_RULE:
        if (!clause_ok(w, c, rc.clause)) return;
        break;
      case REC_CMP:
        if (!from_unres && rc.to.meta == 0xFFFFFFFFu) continue;   // `to` absent: nothing reported (eval_context.rs:2283)
        if (!mk && !clause_ok(w, c, rc.clause)) return;
        break;
      case REC_IN:
        if (!mk && !clause_ok(w, c, rc.clause)) return;
        break;
      default:
        continue;
    }
    if (scan) {
      scan->nmsg++;
      if (rule != NONE) scan->rule = rule;
      continue;
    }
    const PClause pc = mk ? PClause{} : c.P->clauses[rc.clause];
    const uint32_t op = mk ? (rc.y & 15u) : (pc.flags & 15u);
    const bool neg = mk ? ((rc.y >> 4) & 1u) : ((pc.flags >> 4) & 1u);
    switch (rc.kind) {
      case REC_BLOCK_EMPTY:
        tlit(w, "query for block clause did not retrieve any value");
        break;
      case REC_MISSING_BLOCK_VALUE:
        tlit(w, "Check was not compliant as property ["); remaining(w, c, rc.from);
        tlit(w, "] is missing. Value traversed to ["); unresolved_display(w, c, rc.from); tput(w, ']');
        break;
      case REC_UNARY:
        custom_text(w, c, pc);
        if (from_unres) {
          tlit(w, "Check was not compliant as property ["); remaining(w, c, rc.from);
          tlit(w, "] is missing. Value traversed to ["); unresolved_display(w, c, rc.from); tlit(w, "].");
        } else {
          tlit(w, "Check was not compliant as property ["); q_path_display(w, c, rc.from); tlit(w, "] ");
          tlit(w, unary_msg(op, neg)); tput(w, '.');
        }
        break;
      case REC_NOVALUE_EMPTY:
        if (pc.e != NONE) {   // the custom message's newlines become ';' (for every format: Walker::items)
          if (pc.e >= c.P->n_msgs) { w.fb = FB_REF; return; }
          const RStr r = c.P->msgs[pc.e];
          for (uint32_t k = 0; k < r.len; k++) { const char ch = c.P->text[r.off + k]; tput(w, ch == '\n' ? ';' : ch); }
        }
        tlit(w, "Check was not compliant as variable in context ["); tstr_tab(w, c, c.P->ctx, pc.d); tlit(w, "] was not empty");
        break;
      case REC_DEPENDENT_RULE:
        custom_text(w, c, pc);
        tlit(w, "Check was not compliant as dependent rule ["); tstr_tab(w, c, c.P->ctx, pc.f);
        tlit(w, "] did not PASS. Context ["); tstr_tab(w, c, c.P->ctx, pc.d); tput(w, ']');
        break;
      case REC_CMP: {
        const bool to_unres = !from_unres && qkind(rc.to) == QR_UNRESOLVED;
        if (!mk) custom_text(w, c, pc);
        if (from_unres || to_unres) {
          const QR& u = from_unres ? rc.from : rc.to;
          tlit(w, "Check was not compliant as property ["); remaining(w, c, u);
          tlit(w, from_unres ? "] to compare from is missing. Value traversed to [" : "] to compare to is missing. Value traversed to [");
          unresolved_display(w, c, u); tlit(w, "].");
        } else {
          tlit(w, "Check was not compliant as property value ["); pav_display(w, c, rc.from); tlit(w, "] ");
          tlit(w, op_msg(op, neg)); tlit(w, " value ["); pav_display(w, c, rc.to); tlit(w, "].");
        }
        if (rc.x) { tlit(w, " Error = ["); nc_reason(w, c, rc); tput(w, ']'); }
        break;
      }
      default: {   // REC_IN; the `to` values: the REC_LIST records that follow, two per record
        const uint32_t nto = rc.x;
        const uint32_t l0 = i;
        uint32_t have = 0;
        while (have < nto && i < nrec && recs[i].kind == REC_LIST) { have += (have + 1 < nto) ? 2u : 1u; i++; }
        if (!mk) custom_text(w, c, pc);
        COMPOSE(w) {
        tlit(w, "Check was not compliant as property ["); q_path_display(w, c, rc.from); tlit(w, "] was not present in [");
        w.dotf = true;   // the items joined by '.', then every '.' before a '[' dropped (reporter.cpp "fixed")
        for (uint32_t k = 0; k < have; k++) {
          const Rec& lr = recs[l0 + k / 2];
          const QR t = (k & 1u) ? lr.to : lr.from;
          if (k) tput(w, '.');
          if (qkind(t) == QR_UNRESOLVED) { tlit(w, "(unresolved, "); unresolved_display(w, c, t); }
          else { tlit(w, "(resolved, "); pav_display(w, c, t); }
          tput(w, ')');
        }
        if (w.held) { w.held = false; emit(w, '.'); }
        w.dotf = false;
        tput(w, ']');
        }
        break;
      }
    }
  }
}

// a reporter-table string, XML-escaped; from `skip` on
RD void xstr(X& w, const char* text, RStr r, uint32_t skip) { xbulk(w, text + r.off + skip, r.len - skip); }

// one document's <testsuite> (ReportWriter::add, OUT_JUNIT)
RN void file_junit(X& w, const RenderArgs& A, uint32_t doc) {
  const uint32_t k = doc - A.doc0;
  const uint32_t nf = A.nfiles;
  uint32_t nfail = 0;
  for (uint32_t f = 0; f < nf; f++) nfail += A.tiles[(size_t)doc * nf + f].status == ST_FAIL;
  raws(w, "    <testsuite name=\"");
  xbulk(w, A.names + A.name_off[k], (uint32_t)(A.name_off[k + 1] - A.name_off[k]));
  raws(w, "\" errors=\"0\" failures=\""); tu64(w, nfail); raws(w, "\" time=\"0\">\n");
  for (uint32_t f = 0; f < nf && !w.fb; f++) {
    const TileOut to = A.tiles[(size_t)doc * nf + f];
    const RProg& P = A.progs[f];
    raws(w, "        <testcase name=\""); xstr(w, P.text, P.file_name, 0);
    if (to.status != ST_FAIL) {
      raws(w, to.status == ST_PASS ? "\" time=\"0\" status=\"pass\"/>\n" : "\" time=\"0\" status=\"skip\"/>\n");
      continue;
    }
    raws(w, "\" time=\"0\">\n            <failure");
    const Ctx c{&A, &P, A.base[doc]};
    const RecSeq recs{A.recs + to.rec_off, to.pad1 > 1u ? to.pad1 : 1u};
    JScan sc{0, NONE};
    tile_junit(w, c, recs, to.rec_n, &sc);
    if (w.fb) return;
    if (sc.rule != NONE) {
      // get_test_case (reporters/mod.rs:108-168): the last rule failure names it, after the first ".guard/"
      if (sc.rule >= P.n_rule_names) { w.fb = FB_REF; return; }
      const RStr r = P.rule_names[sc.rule];
      const char* s = P.text + r.off;
      uint32_t skip = 0;
      for (uint32_t g = 0; g + 7 <= r.len && !skip; g++) {
        bool hit = true;
        for (uint32_t j = 0; j < 7 && hit; j++) hit = s[g + j] == ".guard/"[j];
        if (hit) skip = g + 7;
      }
      raws(w, " message=\""); xstr(w, P.text, r, skip); raw(w, '"');
    }
    if (sc.nmsg) {
      raw(w, '>');
      tile_junit(w, c, recs, to.rec_n, nullptr);
      raws(w, "</failure>\n");
    } else {
      raws(w, "/>\n");
    }
    raws(w, "        </testcase>\n");
  }
  raws(w, "    </testsuite>\n");
}

}  // namespace rg

// The JUnit report's test suites (rg::file_junit), one lane per document, in the size / write passes and the
// launch shape of report_kernel: the lanes wait on scattered record and arena loads, so resident waves
// (4 per SIMD) matter more than registers.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) report_junit_kernel(RenderArgs A, uint32_t write) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < A.ndocs; k += gridDim.x * blockDim.x) {
    rg::X x{};
    if (write) {
      if (A.sizes[k] & kHostDoc) continue;
      x.p = A.out + A.offsets[k];
    }
    rg::file_junit(x, A, A.doc0 + k);
    if (!write) A.sizes[k] = x.fb ? (kHostDoc | x.fb) : x.n;
  }
}

}  // namespace gg
