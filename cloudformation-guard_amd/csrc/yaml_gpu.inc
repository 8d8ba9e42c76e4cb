// Block-style YAML documents on the device loader (json_gpu.hip, included after the JSON passes).
//
// The subset CloudFormation templates are written in, parsed one lane per document into exactly the
// arena the host loader builds from libyaml's events (doc_loader.cpp libyaml_load + scalar_node +
// Emitter; reference Loader::load and its scalar typing, libyaml/loader.rs:31-244):
//   * block mappings and block sequences (indented, indentless as a mapping value, compact `- k: v`
//     and `- - x` entries), single-line flow sequences and mappings inside them;
//   * plain, single-quoted and double-quoted scalars on one line, literal and folded block scalars
//     (| >, with - / + chomping); comments; a leading `---`;
//   * CloudFormation short-form tags: `!Ref x` / `!GetAtt a.b` ... become {"Ref": "x"} (a string,
//     untyped), `!Join [..]` / `!If` + a block sequence become {"Fn::Join": [..]} (loader.rs:197-244),
//     other `!` tags leave scalars as untyped strings and sequences as they are.
// Marks are libyaml's event start marks: a block mapping at its first key, a block sequence at its first
// `-`, a tagged node at its tag, an empty value one column after its `:`; a root list keeps (0,0).
// Everything else -- block-scalar indentation indicators, folded scalars with more-indented lines,
// multi-line plain or quoted scalars, anchors and aliases,
// complex keys, `!!` tags, flow collections over several lines, tabs, CR, a second document, a number
// the host would type outside the JSON number grammar (`.5`, `+1.5`, `inf`, beyond i64) -- refuses the
// document, which the host loader then builds at its position: results never depend on which ran.
// Count and emit run this same code (M_COUNT / M_EMIT), as the JSON passes do.

static const uint32_t kConstPos = 0x80000000u;   // a string "position" naming kYFn[idx].lng, not text

struct YFn { char shrt[20]; char lng[24]; uint32_t single, seq; };
// doc_loader.cpp kShort / kSingle / kSeq (loader.rs:197-244)
__constant__ YFn kYFn[21] = {
    {"Ref", "Ref", 1, 0}, {"GetAtt", "Fn::GetAtt", 1, 1}, {"Base64", "Fn::Base64", 1, 0}, {"Sub", "Fn::Sub", 1, 1},
    {"GetAZs", "Fn::GetAZs", 1, 0}, {"ImportValue", "Fn::ImportValue", 1, 0}, {"Condition", "Condition", 1, 0},
    {"RefAll", "Fn::RefAll", 1, 0}, {"Select", "Fn::Select", 0, 1}, {"Split", "Fn::Split", 0, 1},
    {"Join", "Fn::Join", 0, 1}, {"FindInMap", "Fn::FindInMap", 0, 1}, {"And", "Fn::And", 0, 1},
    {"Equals", "Fn::Equals", 0, 1}, {"Contains", "Fn::Contains", 0, 1}, {"EachMemberIn", "Fn::EachMemberIn", 0, 1},
    {"EachMemberEquals", "Fn::EachMemberEquals", 0, 1}, {"ValueOf", "Fn::ValueOf", 0, 1}, {"If", "Fn::If", 0, 1},
    {"Not", "Fn::Not", 0, 1}, {"Or", "Fn::Or", 0, 1}};
__device__ inline uint32_t yfn_len(uint32_t f) {
  uint32_t n = 0;
  while (n < 24 && kYFn[f].lng[n]) n++;
  return n;
}

__device__ inline bool yblank(uint32_t c) { return c == ' ' || c == '\n' || c == 256u; }

// one UTF-8 sequence at i (lead byte c >= 0x80) as decode_string accepts it; its continuation-byte count
// in *n, false when outside the subset
__device__ __attribute__((always_inline)) inline bool utf8_seq(Text& T, uint64_t i, uint32_t c, uint32_t* n_out) {
  const uint32_t n = c >= 0xF0u ? 3u : (c >= 0xE0u ? 2u : (c >= 0xC2u ? 1u : 0u));
  if (!n || c > 0xF4u) return false;
  uint32_t cp = c & (0x3Fu >> n);
  for (uint32_t k = 1; k <= n; k++) {
    const uint32_t b = T.at(i + k);
    if ((b & 0xC0u) != 0x80u) return false;
    cp = (cp << 6) | (b & 0x3Fu);
  }
  if ((n == 2 && cp < 0x800u) || (n == 3 && (cp < 0x10000u || cp > 0x10FFFFu))) return false;
  if (cp >= 0xD800u && cp <= 0xDFFFu) return false;
  if (cp < 0xA0u || cp == 0x2028u || cp == 0x2029u || cp == 0xFFFEu || cp == 0xFFFFu || cp == 0xFEFFu) return false;
  *n_out = n;
  return true;
}

// a single-quoted scalar at q ('' is a quote); same return convention as decode_string
template <typename Sink>
__device__ __attribute__((always_inline)) inline uint64_t decode_single(Text& T, uint64_t q, Sink&& sink, uint32_t& cont) {
  uint64_t i = q + 1;
  for (;;) {
    const uint32_t c = T.at(i);
    if (c == '\'') {
      if (T.at(i + 1) != '\'') return i + 1;
      sink.byte('\'');
      i += 2;
      continue;
    }
    if (c >= 0x80u && c < 0x100u) {
      uint32_t n = 0;
      if (!utf8_seq(T, i, c, &n)) return 0;
      for (uint32_t k = 0; k <= n; k++) sink.byte(T.at(i + k));
      cont += n;
      i += n + 1;
      continue;
    }
    if (c < 0x20u || c > 0x7Eu) return 0;
    sink.byte(c);
    i++;
  }
}

// A literal (|) or folded (>) block scalar whose indicator is at q, as libyaml's scan_block_scalar reads it:
// chomping - / + / clip, the indentation of its first content line (no indentation indicator; leading
// empty lines may not be wider), content lines at that indentation (literal: more-indented lines keep
// their extra spaces; folded: refused), line breaks kept (literal) or folded into a space between two
// content lines with no empty line between (folded), empty lines as breaks, then the chomped final breaks.
// parent: the enclosing block collection's indentation (a first content line at or left of it leaves the
// scalar empty: refused); -2 trusts the text (the own / verify passes).  Returns the start of the line
// that ends the scalar (or the end of the text), *lines the line breaks consumed; 0 = refused.
template <typename Sink>
__device__ __attribute__((always_inline)) inline uint64_t decode_block(Text& T, uint64_t q, Sink&& sink, int32_t parent,
                                                                       uint32_t* lines) {
  const bool folded = T.at(q) == '>';
  uint64_t i = q + 1;
  int chomp = 0;   // -1 strip, 0 clip, +1 keep
  if (T.at(i) == '-') { chomp = -1; i++; }
  else if (T.at(i) == '+') { chomp = 1; i++; }
  if (!yblank(T.at(i)) && T.at(i) != '#') return 0;   // an indentation indicator, or text after the indicator
  uint32_t nl = 0;
  {
    const uint64_t s0 = i;
    while (T.at(i) == ' ') i++;
    if (T.at(i) == '#') {
      if (i == s0) return 0;
      while (T.at(i) != '\n' && T.at(i) != 256u) i++;
    }
    if (T.at(i) != '\n') return 0;
    i++;
    nl++;
  }
  // leading empty lines and the first content line's indentation
  uint32_t lead = 0, maxsp = 0, indent = 0;
  for (;;) {
    uint64_t j = i;
    while (T.at(j) == ' ') j++;
    const uint32_t sp = (uint32_t)(j - i), c = T.at(j);
    if (c == '\n') { if (sp > maxsp) maxsp = sp; lead++; nl++; i = j + 1; continue; }
    if (c == 256u || c == '\t' || c == '\r') return 0;
    indent = sp;
    break;
  }
  if ((parent != -2 && (int32_t)indent <= parent) || maxsp > indent || indent == 0) return 0;
  for (uint32_t k = 0; k < lead; k++) sink.byte('\n');
  bool first = true, pending = false, prev_blank = false;
  uint32_t trailing = 0;
  for (;;) {
    // at a content line: `indent` spaces, then its content
    i += indent;
    const uint32_t c0 = T.at(i);
    const bool blank = c0 == ' ' || c0 == '\t';
    if (folded && blank) return 0;
    if (!first) {
      if (folded && pending && !prev_blank && !blank) { if (!trailing) sink.byte(' '); }
      else if (pending) sink.byte('\n');
      for (uint32_t k = 0; k < trailing; k++) sink.byte('\n');
    }
    first = false;
    trailing = 0;
    for (;;) {
      const uint32_t c = T.at(i);
      if (c == '\n' || c == 256u) break;
      if (c >= 0x80u && c < 0x100u) {
        uint32_t n = 0;
        if (!utf8_seq(T, i, c, &n)) return 0;
        for (uint32_t k = 0; k <= n; k++) sink.byte(T.at(i + k));
        i += n + 1;
        continue;
      }
      if ((c < 0x20u && c != '\t') || c == 0x7Fu) return 0;
      sink.byte(c);
      i++;
    }
    prev_blank = blank;
    if (T.at(i) == 256u) { pending = false; break; }
    pending = true;
    i++;
    nl++;
    // empty lines, then either the next content line or the line that ends the scalar
    bool more = false;
    for (;;) {
      uint64_t j = i;
      while (T.at(j) == ' ') j++;
      const uint32_t sp = (uint32_t)(j - i), c = T.at(j);
      if (c == '\n') { if (sp > indent) return 0; trailing++; nl++; i = j + 1; continue; }
      if (c == 256u) break;
      if (sp >= indent) more = true;
      break;
    }
    if (!more) break;
  }
  if (chomp != -1 && pending) sink.byte('\n');
  if (chomp == 1) for (uint32_t k = 0; k < trailing; k++) sink.byte('\n');
  if (lines) *lines = nl;
  return i;
}

// The decoded bytes of the string occurrence at q (the own and verify passes): a JSON / YAML
// double-quoted string, a single-quoted one, a constant (kConstPos), or `len` raw bytes of a plain
// scalar.  0 on failure.
template <typename Sink>
__device__ uint64_t decode_at(Text& T, uint64_t q, uint32_t len, Sink&& sink, uint32_t& cont) {
  if (q & kConstPos) {
    const uint32_t f = (uint32_t)(q & 0xFFu);
    if (f >= 21 || len != yfn_len(f)) return 0;
    for (uint32_t k = 0; k < len; k++) sink.byte((uint8_t)kYFn[f].lng[k]);
    return 1;
  }
  const uint32_t c = T.at(q);
  if (c == '"') return decode_string(T, q, sink, cont);
  if (c == '\'') return decode_single(T, q, sink, cont);
  if (c == '|' || c == '>') return decode_block(T, q, sink, -2, nullptr);
  for (uint32_t k = 0; k < len; k++) sink.byte(T.at(q + k));
  return q + len + 1;
}


// Plain scalar typing (doc_loader.cpp scalar_node, loader.rs:62-119): Rust i64::from_str, then
// f64::from_str, then the bool words, then ~ / null.  1: nd typed; 0: a string; -1: refuse (a float
// outside the JSON number grammar, an i64 overflow, inf / nan words: the host types those).
__device__ __attribute__((always_inline)) inline int yaml_plain_type(Text& T, uint64_t s, uint32_t L, DNode& nd) {
  if (!L) return 0;
  const uint32_t c0 = T.at(s);
  // only a digit, a sign, '.', '~' or the first letter of inf / nan / null / a bool word can type
  if (!is_digit(c0) && c0 != '+' && c0 != '-' && c0 != '.' && c0 != '~' && c0 != 'i' && c0 != 'I' && c0 != 'n' &&
      c0 != 'N' && c0 != 't' && c0 != 'y' && c0 != 'o' && c0 != 'f')
    return 0;
  // [+-]?[0-9]+
  {
    uint32_t j = (c0 == '+' || c0 == '-') ? 1u : 0u;
    bool digits = j < L;
    for (uint32_t k = j; k < L && digits; k++) digits = is_digit(T.at(s + k));
    if (digits) {
      uint64_t v = 0;
      for (uint32_t k = j; k < L; k++) {
        const uint32_t dg = T.at(s + k) - '0';
        if (v > (0x7FFFFFFFFFFFFFFFull + 1ull - dg) / 10ull) return -1;   // beyond i64 (a float to Rust)
        v = v * 10ull + dg;
      }
      const bool neg = c0 == '-';
      if (!neg && v > 0x7FFFFFFFFFFFFFFFull) return -1;
      const uint64_t u = neg ? (uint64_t)0 - v : v;
      nd.kind = K_INT; nd.a = (uint32_t)u; nd.b = (uint32_t)(u >> 32);
      return 1;
    }
  }
  // Rust f64 grammar: [+-]? (inf | infinity | nan | digits? (. digits?)? ([eE][+-]?digits)?) with a digit
  {
    uint32_t k = (c0 == '+' || c0 == '-') ? 1u : 0u;
    const uint32_t c1 = T.at(s + k) | 0x20u;
    if (c1 == 'i' || c1 == 'n') {
      // inf / infinity / nan (any case): floats to Rust
      const char* w[3] = {"inf", "infinity", "nan"};
      for (int x = 0; x < 3; x++) {
        uint32_t n = 0;
        while (w[x][n]) n++;
        if (L - k != n) continue;
        bool eq = true;
        for (uint32_t q = 0; q < n && eq; q++) eq = (T.at(s + k + q) | 0x20u) == (uint32_t)w[x][q];
        if (eq) return -1;
      }
    } else {
      uint32_t nd0 = 0;
      while (k < L && is_digit(T.at(s + k))) { k++; nd0++; }
      if (k < L && T.at(s + k) == '.') { k++; while (k < L && is_digit(T.at(s + k))) { k++; nd0++; } }
      bool fl = nd0 > 0;
      if (fl && k < L && (T.at(s + k) | 0x20u) == 'e') {
        k++;
        if (k < L && (T.at(s + k) == '+' || T.at(s + k) == '-')) k++;
        uint32_t ne = 0;
        while (k < L && is_digit(T.at(s + k))) { k++; ne++; }
        fl = ne > 0;
      }
      if (fl && k == L) {
        // a Rust float: typed here only inside the JSON number grammar
        uint32_t j = 0;
        if (T.at(s) == '-') j++;
        if (j < L && T.at(s + j) == '0') j++;
        else if (j < L && T.at(s + j) >= '1' && T.at(s + j) <= '9') { while (j < L && is_digit(T.at(s + j))) j++; }
        else return -1;
        if (j < L && T.at(s + j) == '.') { j++; const uint32_t d0 = j; while (j < L && is_digit(T.at(s + j))) j++; if (j == d0) return -1; }
        if (j < L && (T.at(s + j) | 0x20u) == 'e') {
          j++;
          if (j < L && (T.at(s + j) == '+' || T.at(s + j) == '-')) j++;
          const uint32_t d0 = j;
          while (j < L && is_digit(T.at(s + j))) j++;
          if (j == d0) return -1;
        }
        if (j != L) return -1;
        uint64_t u = 0;
        if (!parse_json_f64([&](uint64_t q) { return T.at(s + q); }, L, kPow5_128, u)) return -1;
        nd.kind = K_FLOAT; nd.a = (uint32_t)u; nd.b = (uint32_t)(u >> 32);
        return 1;
      }
    }
  }
  auto word = [&](const char* w) __attribute__((always_inline)) {
    uint32_t n = 0;
    while (w[n]) n++;
    if (n != L) return false;
    for (uint32_t q = 0; q < n; q++) if (T.at(s + q) != (uint32_t)(uint8_t)w[q]) return false;
    return true;
  };
  if (word("true") || word("yes") || word("on") || word("y")) { nd.kind = K_BOOL; nd.a = 1; return 1; }
  if (word("false") || word("no") || word("off") || word("n")) { nd.kind = K_BOOL; nd.a = 0; return 1; }
  if (L == 1 && c0 == '~') { nd.kind = K_NULL; return 1; }
  if (L == 4 && (T.at(s) | 0x20u) == 'n' && (T.at(s + 1) | 0x20u) == 'u' && (T.at(s + 2) | 0x20u) == 'l' && (T.at(s + 3) | 0x20u) == 'l') {
    nd.kind = K_NULL;
    return 1;
  }
  return 0;
}

enum : uint32_t { Y_BMAP = 0, Y_BSEQ = 1, Y_FMAP = 2, Y_FSEQ = 3, Y_FN = 4 };
// node contexts: the root, a node on its own line(s) under a block collection, a mapping value after
// `key: ` on the key's line, a sequence entry after `- ` (compact mappings and sequences allowed), an
// element of a flow collection
enum : uint32_t { C_ROOT = 0, C_BLOCK = 1, C_MAPVAL = 2, C_SEQVAL = 3 };
static const uint32_t kYMaxDepth = 64;

struct YF {
  uint32_t kind;
  int32_t indent;    // block collections: their column; BSEQ: bit 30 = indentless (a mapping value's)
  uint32_t slot, k, first, j, cnt;
};

// A segment of a document for the cooperative path (yaml_coop.inc): one entry of a block collection with
// everything under it, parsed by parse_yaml_doc<MODE, true> started from this descriptor instead of the
// document's first byte.  The first segment (YS_FIRST) starts as a document does and leaves the root
// collection open; every other one starts at a line start inside the open frame `f` (f.j: the entry's
// ordinal).  A segment whose entry is a split `key:` header leaves that key's collection open too: the
// collections a segment leaves open are its spine (`nspine`, the first it opens; kind, indentation and
// child count as the segmentation kernel predicts them).
enum : uint32_t { YS_FIRST = 1, YS_WHOLE = 2 };
struct YSeg {
  uint32_t doc, start, end, line;   // the text range (document offsets; start is a line start) and its first line
  uint32_t flags, hdr, hu;          // the frame it starts in: spine container hu of this document's segment hdr
  uint32_t nspine, skind[2], scnt[2];
  int32_t sindent[2];
  YF f;                             // the open frame (fix kernel; f.j by the segmentation kernel)
  uint32_t nn, nc, ns;              // count pass: nodes, containers, strings
  uint32_t cbase, next;             // fix kernel: the first container ordinal and children-block slot
};

template <uint32_t MODE, bool SEG = false>
__device__ __attribute__((always_inline)) inline void parse_yaml_doc(const JArgs& A, uint32_t d, YSeg* seg = nullptr) {
  const uint64_t b0 = A.off[d], b1 = A.off[d + 1];
  Text T(A.text, b0, SEG ? (uint64_t)seg->end : b1 - b0);
  uint64_t i = 0, ls = 0;
  uint32_t line = 0, cont = 0;
  bool ok = true;
  auto column = [&]() __attribute__((always_inline)) { return (uint32_t)(i - ls) - cont; };
  auto bad = [&](uint32_t why) __attribute__((always_inline)) {
    if (SEG) {
      // a document's segments refuse it concurrently: the first reason stands, with its position (which
      // segment is first may differ from run to run when several refuse)
      if (atomicCAS(&A.doc_bad[d], 0u, why) == 0u && A.bad_at) A.bad_at[d] = (uint32_t)i;
    } else if (!A.doc_bad[d]) { A.doc_bad[d] = why; if (A.bad_at) A.bad_at[d] = (uint32_t)i; }
    ok = false;
  };
  const uint64_t nb = (MODE >= M_EMIT) ? A.node_base[d] : 0;
  const uint32_t nlimit = (MODE >= M_EMIT) ? A.n_nodes[d] : 0xFFFFFFFFu;
  // a segment's count pass numbers its containers from 0 and leaves their child counts at its own half
  // text offset in A.ycnt; the fix kernel moves them to the document's container order
  const bool seg_count = SEG && MODE == M_COUNT;
  uint16_t* const cnts = seg_count ? A.ycnt : A.counts;
  const uint64_t cb = (b0 >> 1) + (seg_count ? seg->start >> 1 : 0u);
  const uint64_t kcap = seg_count ? (seg->end - seg->start) >> 1 : (b1 - b0) >> 1;
  uint32_t nn = 1, nc = 0, ns = 0, ci = 0, next = 1;
  if (SEG && MODE >= M_EMIT) { ci = seg->cbase; next = seg->next; }
  // the open collections: the innermost in registers (`top`), the ones around it in st[0, sp - 1) (scratch)
  YF st[kYMaxDepth];
  YF top{};
  uint32_t sp = 0;

  // ---- text
  // spaces a 16-byte window at a time (indentation, the blank after `:` / `-`)
  auto sp_skip = [&]() __attribute__((always_inline)) {
    for (;;) {
      const uint32_t r = T.run_of(i, [](uint32_t x) { return Text::not_space(x); });
      if (!r) break;
      i += r;
    }
  };
  auto newline = [&]() __attribute__((always_inline)) { i++; line++; ls = i; cont = 0; };
  // a comment at i to the end of its line: libyaml's reader accepts only printable characters, tabs
  // and (refused here) CR / NEL, in comments too
  auto skip_comment = [&]() __attribute__((always_inline)) -> bool {
    for (;;) {
      const uint32_t r = T.run_of(i, [](uint32_t x) { return Text::not_printable(x); });
      if (r) { i += r; continue; }
      const uint32_t c = T.at(i);
      if (c == '\n' || c == 256u) return true;
      if (c >= 0x80u && c < 0x100u) {
        uint32_t n = 0;
        if (!utf8_seq(T, i, c, &n)) { bad(BAD_YAML); return false; }
        i += n + 1;
        continue;
      }
      if ((c < 0x20u && c != '\t') || c == 0x7Fu) { bad(BAD_YAML); return false; }
      i++;
    }
  };
  // the rest of a line after a value: spaces, a comment after a space, the break (or the end)
  auto end_line = [&]() __attribute__((always_inline)) -> bool {
    sp_skip();
    uint32_t c = T.at(i);
    if (c == '#') {
      if (i != ls && T.at(i - 1) != ' ') { bad(BAD_YAML); return false; }   // a comment follows a space
      if (!skip_comment()) return false;
      c = T.at(i);
    }
    if (c == '\n') { newline(); return true; }
    if (c == 256u) return true;
    bad(BAD_YAML);
    return false;
  };
  // from a line start: skip blank and comment lines; false at the end of the text.  A document marker,
  // a directive or a tab / CR refuses.
  auto next_line = [&]() __attribute__((always_inline)) -> bool {
    for (;;) {
      sp_skip();
      uint32_t c = T.at(i);
      if (c == 256u) return false;
      if (c == '\n') { newline(); continue; }
      if (c == '#') { if (!skip_comment()) return false; continue; }
      if (c == '\t' || c == '\r') { bad(BAD_YAML); return false; }
      if (i == ls && (c == '%' || ((c == '-' || c == '.') && T.at(i + 1) == c && T.at(i + 2) == c && yblank(T.at(i + 3))))) {
        bad(BAD_YAML);
        return false;
      }
      return true;
    }
  };

  // ---- emission (the JSON passes' layout and records)
  uint32_t ekey = NONE, elen = 0, ekpos = 0, ekl = 0, ekc = 0;
  auto put = [&](uint32_t rel, DNode nd, uint32_t parent, uint32_t vpos, uint32_t ml, uint32_t mc) __attribute__((always_inline)) {
    if (rel >= nlimit) { bad(BAD_YAML); return; }
    nd.key_off = ekey; nd.key_len = elen; nd.key_hash = ekey == NONE ? 0u : ekey; nd.parent = parent;
    NodeRec r;
    r.n = nd; r.line = ml; r.col = mc; r.kline = ekl; r.kcol = ekc; r.kpos = ekpos; r.vpos = vpos;
    r.pad0 = 0; r.pad1 = 0;
    A.recs[nb + rel] = r;
  };
  struct HashSink {
    WordStream ws;
    uint64_t h;
    __device__ void byte(uint32_t c) { ws.byte(c, [&](uint32_t w, uint32_t) { h = (h ^ w) * 0x100000001b3ull; }); }
    __device__ void run(const Text& T, uint32_t k, uint32_t r) {
      ws.run(T, k, r, [&](uint32_t w, uint32_t) { h = (h ^ w) * 0x100000001b3ull; });
    }
  };
  auto fp_slot = [&](HashSink& hs, uint32_t q, uint32_t* len_out) __attribute__((always_inline)) -> uint32_t {
    const uint64_t h = (hs.h ^ hs.ws.word) * 0x100000001b3ull;
    const uint32_t len = hs.ws.len;
    *len_out = len;
    const uint64_t key64 = intern_key64(h, len, A.fp_mask);
    const uint32_t s = intern_slot(A, key64, len, d, q);
    if (s == ~0u) { refuse(A, BAD_TABLE); bad(BAD_TABLE); }
    return s;
  };
  // a scalar's bytes: its table slot and decoded length (EMIT); false on refusal.  style: '"', '\'' or 0
  // (plain: L raw bytes at s), 1 (constant kYFn[s].lng)
  auto scalar_slot = [&](uint64_t s, uint32_t L, uint32_t style, uint32_t* slot, uint32_t* len) __attribute__((always_inline)) -> bool {
    if (MODE != M_EMIT) return true;
    HashSink hs{WordStream(), 0xcbf29ce484222325ull};
    uint32_t c2 = 0;
    if (style == 1) {
      for (uint32_t k = 0; k < L; k++) hs.byte((uint8_t)kYFn[s].lng[k]);
      *slot = fp_slot(hs, kConstPos | (uint32_t)s, len);
    } else if (style == '"') {
      if (!decode_string(T, s, hs, c2)) { bad(BAD_YAML); return false; }
      *slot = fp_slot(hs, (uint32_t)s, len);
    } else if (style == '\'') {
      if (!decode_single(T, s, hs, c2)) { bad(BAD_YAML); return false; }
      *slot = fp_slot(hs, (uint32_t)s, len);
    } else if (style == '|' || style == '>') {
      if (!decode_block(T, s, hs, -2, nullptr)) { bad(BAD_YAML); return false; }
      *slot = fp_slot(hs, (uint32_t)s, len);
    } else {
      // the raw bytes a window at a time (the same words as byte by byte)
      for (uint32_t k = 0; k < L;) {
        (void)T.at(s + k);   // loads the window holding byte s + k
        const uint32_t o = T.woff(s + k), r = min(16u - o, L - k);
        hs.run(T, o, r);
        k += r;
      }
      *slot = fp_slot(hs, (uint32_t)s, len);
    }
    return ok;
  };
  auto open = [&](uint32_t rel, uint32_t parent, uint32_t kind, int32_t indent, uint32_t ml, uint32_t mc) __attribute__((always_inline)) -> bool {
    if (sp >= kYMaxDepth) { bad(BAD_DEPTH); return false; }
    const uint32_t k = ci++;
    if (k >= kcap) { bad(BAD_YAML); return false; }
    nc++;
    uint32_t cnt = 0, first = 0;
    if (MODE >= M_EMIT) {
      cnt = cnts[cb + k];
      first = next;
      next += cnt;
      if (next > nlimit || (kind == Y_FN && cnt != 1)) { bad(BAD_YAML); return false; }
    }
    if (MODE == M_EMIT) {
      DNode nd; nd.kind = (kind == Y_BSEQ || kind == Y_FSEQ) ? K_LIST : K_MAP; nd.count = cnt; nd.a = first; nd.b = 0;
      put(rel, nd, parent, 0, ml, mc);
    }
    YF f; f.kind = kind; f.indent = indent; f.slot = rel; f.k = k; f.first = first; f.j = 0; f.cnt = cnt;
    if (sp) st[sp - 1] = top;
    top = f;
    sp++;
    return ok;
  };
  auto close_top = [&]() __attribute__((always_inline)) -> bool {
    YF& f = top;
    if (MODE == M_COUNT) {
      if (f.j > 0xFFFFu) { bad(BAD_WIDE); return false; }
      cnts[cb + f.k] = (uint16_t)f.j;
    } else if (f.j != f.cnt) { bad(BAD_YAML); return false; }
    sp--;
    if (sp) top = st[sp - 1];
    return true;
  };
  // the next child of the top frame: its node index (the caller sets the key fields first)
  auto child = [&]() __attribute__((always_inline)) -> uint32_t {
    YF& f = top;
    const uint32_t rel = f.first + f.j;
    f.j++;
    nn++;
    return rel;
  };
  auto no_key = [&]() __attribute__((always_inline)) { ekey = NONE; elen = 0; ekpos = 0; ekl = 0; ekc = 0; };
  // a string node (quoted, plain or constant)
  auto string_node = [&](uint32_t rel, uint32_t parent, uint64_t s, uint32_t L, uint32_t style, uint32_t ml, uint32_t mc) __attribute__((always_inline)) {
    ns++;
    uint32_t slot = 0, len = 0;
    if (!scalar_slot(s, L, style, &slot, &len)) return;
    if (MODE == M_EMIT) {
      DNode nd; nd.kind = K_STRING; nd.count = len; nd.a = slot; nd.b = slot;
      put(rel, nd, parent, style == 1 ? (kConstPos | (uint32_t)s) : (uint32_t)s, ml, mc);
    }
  };
  // a CloudFormation function wrapper {long form: child}: opened with its one child's key set
  auto open_fn = [&](uint32_t rel, uint32_t parent, uint32_t f, uint32_t ml, uint32_t mc) __attribute__((always_inline)) -> bool {
    if (!open(rel, parent, Y_FN, -1, ml, mc)) return false;
    ns++;
    uint32_t slot = 0, len = 0;
    if (!scalar_slot(f, yfn_len(f), 1, &slot, &len)) return false;
    ekey = slot; elen = len; ekpos = kConstPos | f; ekl = ml; ekc = mc;
    return true;
  };
  // frames completed by their one child
  auto close_fns = [&]() __attribute__((always_inline)) {
    while (ok && sp && top.kind == Y_FN && top.j == 1) close_top();
  };

  // ---- scalars
  // a plain scalar at i: its end (trailing spaces trimmed); flow: stops at , [ ] { } and refuses ':'
  auto scan_plain = [&](bool flow, uint64_t* e_out) __attribute__((always_inline)) -> bool {
    const uint64_t s = i;
    const uint32_t c0 = T.at(i);
    if (c0 == ',' || c0 == '[' || c0 == ']' || c0 == '{' || c0 == '}' || c0 == '#' || c0 == '&' || c0 == '*' ||
        c0 == '!' || c0 == '|' || c0 == '>' || c0 == '\'' || c0 == '"' || c0 == '%' || c0 == '@' || c0 == '`' ||
        ((c0 == '-' || c0 == '?' || c0 == ':') && (yblank(T.at(i + 1)) || (flow && (T.at(i + 1) == ',' || T.at(i + 1) == ']' || T.at(i + 1) == '}'))))) {
      bad(BAD_YAML);
      return false;
    }
    uint64_t last = i;
    for (;;) {
      // ordinary bytes (printable ASCII other than space : # and the flow indicators) a window at a time:
      // each only moves `last` past itself, as the byte loop below does
      const uint32_t run = flow ? T.run_of(i, [](uint32_t x) { return Text::yplain_special<true>(x); })
                                : T.run_of(i, [](uint32_t x) { return Text::yplain_special<false>(x); });
      if (run) { i += run; last = i; continue; }
      const uint32_t c = T.at(i);
      if (c == '\n' || c == 256u) { if (flow) { bad(BAD_YAML); return false; } break; }
      if (c == ':' && (yblank(T.at(i + 1)) || flow)) { if (flow && !yblank(T.at(i + 1))) { bad(BAD_YAML); return false; } break; }
      if (c == '#' && i > s && T.at(i - 1) == ' ') { if (flow) { bad(BAD_YAML); return false; } break; }
      if (flow && (c == ',' || c == '[' || c == ']' || c == '{' || c == '}')) break;
      if (c >= 0x80u && c < 0x100u) {
        uint32_t n = 0;
        if (!utf8_seq(T, i, c, &n)) { bad(BAD_YAML); return false; }
        i += n + 1;
        cont += n;
        last = i;
        continue;
      }
      if (c < 0x20u || c == 0x7Fu) { bad(BAD_YAML); return false; }
      i++;
      if (c != ' ') last = i;
    }
    if (last - s > 1024) { bad(BAD_YAML); return false; }
    *e_out = last;
    return true;
  };
  // a quoted scalar at i (one line): i moves past it
  auto scan_quoted = [&]() __attribute__((always_inline)) -> bool {
    struct Skip {
      __device__ void byte(uint32_t) {}
      __device__ void run(const Text&, uint32_t, uint32_t) {}
    } sk;
    const uint32_t q = T.at(i);
    const uint64_t e = q == '"' ? decode_string<false>(T, i, sk, cont) : decode_single(T, i, sk, cont);
    if (!e) { bad(BAD_YAML); return false; }
    i = e;
    return true;
  };
  // a scalar value node at s (style '"' / '\'' / 0 plain of L bytes) with an optional tag f (~0u none,
  // 0xFFFF an unknown `!` tag)
  auto scalar_value = [&](uint32_t rel, uint32_t parent, uint64_t s, uint32_t L, uint32_t style, uint32_t tag,
                          uint32_t ml, uint32_t mc) __attribute__((always_inline)) {
    if (tag != ~0u) {
      if (tag < 21 && kYFn[tag].single) {
        if (!open_fn(rel, parent, tag, ml, mc)) return;
        const uint32_t fr = top.slot;
        string_node(child(), fr, s, L, style, ml, mc);
        close_fns();
        return;
      }
      string_node(rel, parent, s, L, style, ml, mc);
      return;
    }
    if (style) { string_node(rel, parent, s, L, style, ml, mc); return; }
    DNode nd; nd.kind = K_NULL; nd.count = 0; nd.a = 0; nd.b = 0;
    const int ty = yaml_plain_type(T, s, L, nd);
    if (ty < 0) { bad(BAD_NUMBER); return; }
    if (ty == 0) { string_node(rel, parent, s, L, 0, ml, mc); return; }
    if (MODE == M_EMIT) put(rel, nd, parent, 0, ml, mc);
  };
  // a `!` tag at i: the index of its short form in kYFn, 0xFFFF another `!name`; ~0u refused
  auto scan_tag = [&]() __attribute__((always_inline)) -> uint32_t {
    uint64_t j = i + 1;
    while (true) {
      const uint32_t c = T.at(j);
      if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9')) j++;
      else break;
    }
    const uint32_t n = (uint32_t)(j - i - 1);
    if (!n || !yblank(T.at(j))) { bad(BAD_YAML); return ~0u; }
    uint32_t f = 0xFFFFu;
    for (uint32_t x = 0; x < 21 && f == 0xFFFFu; x++) {
      uint32_t m = 0;
      while (kYFn[x].shrt[m]) m++;
      if (m != n) continue;
      bool eq = true;
      for (uint32_t q = 0; q < n && eq; q++) eq = T.at(i + 1 + q) == (uint32_t)(uint8_t)kYFn[x].shrt[q];
      if (eq) f = x;
    }
    i = j;
    return f;
  };

  // ---- flow collections: [ ... ] / { ... } on one line, at i; the node `rel` of parent `parent`
  auto flow = [&](uint32_t rel, uint32_t parent, uint32_t tag, uint32_t ml, uint32_t mc) __attribute__((always_inline)) {
    const uint32_t base_sp = sp;
    auto open_flow = [&](uint32_t r, uint32_t p, uint32_t tg, uint32_t l, uint32_t c) __attribute__((always_inline)) -> bool {
      const bool seq = T.at(i) == '[';
      if (seq && tg < 21 && kYFn[tg].seq) {
        if (!open_fn(r, p, tg, l, c)) return false;
        p = top.slot;
        r = child();
      }
      if (!open(r, p, seq ? Y_FSEQ : Y_FMAP, -1, l, c)) return false;
      i++;
      return true;
    };
    if (!open_flow(rel, parent, tag, ml, mc)) return;
    while (ok && sp > base_sp) {
      YF& F = top;
      if (F.kind == Y_FN) { close_fns(); continue; }
      const uint32_t closer = F.kind == Y_FSEQ ? ']' : '}';
      sp_skip();
      uint32_t c = T.at(i);
      if (F.j > 0) {
        if (c == closer) { i++; close_top(); close_fns(); continue; }
        if (c != ',') { bad(BAD_YAML); return; }
        i++;
        sp_skip();
        c = T.at(i);
        if (c == closer) { bad(BAD_YAML); return; }   // a trailing comma
      } else if (c == closer) {
        i++; close_top(); close_fns(); continue;
      }
      if (c == '\n' || c == 256u || c == '#') { bad(BAD_YAML); return; }
      const uint32_t fslot = F.slot;
      if (F.kind == Y_FMAP) {
        if (F.j >= kMaxPairwiseKeys) { bad(BAD_WIDEMAP); return; }
        const uint64_t ks = i;
        const uint32_t kl = line, kc = column();
        uint32_t L = 0, style = 0;
        if (c == '"' || c == '\'') {
          style = c;
          if (!scan_quoted()) return;
          sp_skip();
          if (T.at(i) != ':') { bad(BAD_YAML); return; }
        } else {
          uint64_t e = 0;
          if (!scan_plain(true, &e)) return;
          L = (uint32_t)(e - ks);
          DNode kt;
          if (yaml_plain_type(T, ks, L, kt) != 0) { bad(BAD_YAML); return; }
          sp_skip();
          if (T.at(i) != ':' || !yblank(T.at(i + 1))) { bad(BAD_YAML); return; }
        }
        i++;
        ns++;
        uint32_t slot = 0, len = 0;
        if (!scalar_slot(ks, L, style, &slot, &len)) return;
        ekey = slot; elen = len; ekpos = (uint32_t)ks; ekl = kl; ekc = kc;
        sp_skip();
        c = T.at(i);
      } else {
        no_key();
      }
      const uint32_t r = child();
      uint32_t l = line, cc = column();
      uint32_t tg = ~0u;
      if (c == '!') {
        tg = scan_tag();
        if (tg == ~0u) return;
        sp_skip();
        c = T.at(i);
      }
      if (c == '[' || c == '{') {
        if (!open_flow(r, fslot, tg, l, cc)) return;
        continue;
      }
      if (c == '"' || c == '\'') {
        const uint64_t s = i;
        if (!scan_quoted()) return;
        scalar_value(r, fslot, s, 0, c, tg, l, cc);
      } else {
        const uint64_t s = i;
        uint64_t e = 0;
        if (!scan_plain(true, &e)) return;
        scalar_value(r, fslot, s, (uint32_t)(e - s), 0, tg, l, cc);
      }
    }
  };

  // ---- the document: leading blank and comment lines, an optional `---` line, the root at column 0
  const bool at_start = !SEG || (seg->flags & YS_FIRST);   // (a later segment starts at a line inside its frame)
  if (at_start) {
    for (;;) {
      sp_skip();
      const uint32_t c = T.at(i);
      if (c == '\n') { newline(); continue; }
      if (c == '#') { if (!skip_comment()) return; continue; }
      break;
    }
    if (i == ls && T.at(i) == '-' && T.at(i + 1) == '-' && T.at(i + 2) == '-' && yblank(T.at(i + 3))) {
      i += 3;
      if (!end_line()) return;
    }
    if (!next_line()) { if (ok) bad(BAD_YAML); return; }
  }
  // state: S_NODE (a node for n_rel at i), S_LINE (at the first content byte of a line, column ccol, or
  // the end), S_AFTER (an inline value just ended mid-line)
  enum : uint32_t { S_NODE = 0, S_LINE = 1, S_AFTER = 2 };
  uint32_t state = S_NODE, n_rel = 0, n_parent = NONE, n_ctx = C_ROOT;
  int32_t n_pn = -1;
  bool eof = false;
  uint32_t ccol = 0;
  if (at_start && column() != 0) { bad(BAD_YAML); return; }
  no_key();
  // the frames a segment leaves open: the one it starts in and its spine
  const uint32_t prot = SEG ? seg->nspine + (at_start ? 0u : 1u) : 0u;
  if (!at_start) {
    i = seg->start; ls = i; line = seg->line;
    nn = 0;
    top = seg->f;
    sp = 1;
    eof = !next_line();
    if (!ok) return;
    ccol = eof ? 0 : column();
    state = S_LINE;
  }
  while (ok) {
    if (state == S_AFTER) {
      close_fns();
      if (!ok || !end_line()) return;
      eof = !next_line();
      if (!ok) return;
      ccol = eof ? 0 : column();
      state = S_LINE;
      continue;
    }
    if (state == S_LINE) {
      if (SEG && sp <= prot) {
        // at a frame this segment leaves open.  The end of the segment: exactly those frames are open, each
        // one entry further, the spine as predicted.  Another line: it opens the frame's one entry here, at
        // the frame's column -- a shallower line would close the frame, a second entry is the next
        // segment's: the document was split where no entry starts, and is refused
        if (eof) {
          bool fine = sp == prot;
          for (uint32_t t = 1; fine && t <= prot; t++) {
            const YF& fr = t == sp ? top : st[t - 1];
            if (t == 1 && !at_start) { fine = fr.j == seg->f.j + 1; continue; }
            const uint32_t u = t - (at_start ? 1u : 2u);
            fine = fr.kind == seg->skind[u] && fr.indent == seg->sindent[u] && fr.j == 1;
          }
          if (!fine) bad(BAD_YAML);
          break;
        }
        if (sp && (top.j != (sp == 1 && !at_start ? seg->f.j : 0u) || ccol != (uint32_t)(top.indent & 0xFFFF))) {
          bad(BAD_YAML);
          return;
        }
      }
      if (!sp) { if (!eof) bad(BAD_YAML); break; }
      YF& F = top;
      const int32_t ind = F.indent & 0xFFFF;
      if (F.kind == Y_BMAP) {
        if (eof || (int32_t)ccol < ind) { close_top(); close_fns(); continue; }
        if ((int32_t)ccol > ind) { bad(BAD_YAML); return; }
        if (F.j >= kMaxPairwiseKeys) { bad(BAD_WIDEMAP); return; }
        uint32_t c = T.at(i);
        if (c == '-' && yblank(T.at(i + 1))) { bad(BAD_YAML); return; }
        if (c == '?' || c == '!' || c == '&' || c == '*' || c == '[' || c == '{') { bad(BAD_YAML); return; }
        const uint64_t ks = i;
        const uint32_t kl = line, kc = ccol;
        uint32_t L = 0, style = 0;
        if (c == '"' || c == '\'') {
          style = c;
          if (!scan_quoted()) return;
          if (line != kl || i - ks > 1024) { bad(BAD_YAML); return; }
        } else {
          uint64_t e = 0;
          if (!scan_plain(false, &e)) return;
          L = (uint32_t)(e - ks);
          // a plain key the host types (a number, a bool word, null) is its error to report
          DNode kt;
          if (yaml_plain_type(T, ks, L, kt) != 0) { bad(BAD_YAML); return; }
        }
        sp_skip();
        if (T.at(i) != ':' || !yblank(T.at(i + 1))) { bad(BAD_YAML); return; }
        const uint64_t colon = i;
        const uint32_t ccolon = column();
        i++;
        ns++;
        uint32_t slot = 0, len = 0;
        if (!scalar_slot(ks, L, style, &slot, &len)) return;
        ekey = slot; elen = len; ekpos = (uint32_t)ks; ekl = kl; ekc = kc;
        const uint32_t fslot = F.slot;
        const uint32_t r = child();
        sp_skip();
        c = T.at(i);
        if (c == '\n' || c == 256u || c == '#') {
          if (!end_line()) return;
          const bool e2 = !next_line();
          if (!ok) return;
          const int32_t c2 = e2 ? -1 : (int32_t)column();
          if (!e2 && (c2 > ind || (c2 == ind && T.at(i) == '-' && yblank(T.at(i + 1))))) {
            n_rel = r; n_parent = fslot; n_ctx = C_BLOCK; n_pn = ind; state = S_NODE;
            continue;
          }
          // an empty value: a plain empty scalar one column after the ':' (libyaml process_empty_scalar)
          string_node(r, fslot, colon, 0, 0, kl, ccolon + 1);
          eof = e2; ccol = e2 ? 0 : (uint32_t)c2;
          continue;
        }
        n_rel = r; n_parent = fslot; n_ctx = C_MAPVAL; n_pn = ind; state = S_NODE;
        continue;
      }
      if (F.kind == Y_BSEQ) {
        const bool indentless = (F.indent >> 30) & 1;
        if (eof || (int32_t)ccol < ind) { close_top(); close_fns(); continue; }
        if ((int32_t)ccol > ind) { bad(BAD_YAML); return; }
        if (!(T.at(i) == '-' && yblank(T.at(i + 1)))) {
          if (indentless) { close_top(); close_fns(); continue; }
          bad(BAD_YAML);
          return;
        }
        i++;
        no_key();
        const uint32_t fslot = F.slot;
        const uint32_t r = child();
        sp_skip();
        const uint32_t c = T.at(i);
        if (c == '\n' || c == 256u || c == '#') {
          if (!end_line()) return;
          const bool e2 = !next_line();
          if (!ok) return;
          if (e2 || (int32_t)column() <= ind) { bad(BAD_YAML); return; }   // an empty entry
          n_rel = r; n_parent = fslot; n_ctx = C_BLOCK; n_pn = ind; state = S_NODE;
          continue;
        }
        n_rel = r; n_parent = fslot; n_ctx = C_SEQVAL; n_pn = ind; state = S_NODE;
        continue;
      }
      bad(BAD_YAML);
      return;
    }
    // S_NODE: node n_rel at i
    uint32_t ml = line, mc = column();
    uint32_t tag = ~0u;
    uint32_t c = T.at(i);
    if (c == '!') {
      tag = scan_tag();
      if (tag == ~0u) return;
      sp_skip();
      c = T.at(i);
      if (c == '\n' || c == 256u || c == '#') {
        // a tagged node on the following lines: a block sequence only
        if (n_ctx == C_ROOT || n_ctx == C_BLOCK) { bad(BAD_YAML); return; }
        if (!end_line()) return;
        if (!next_line()) { if (ok) bad(BAD_YAML); return; }
        const int32_t c2 = (int32_t)column();
        if (!(T.at(i) == '-' && yblank(T.at(i + 1)))) { bad(BAD_YAML); return; }
        if (!(c2 > n_pn || (c2 == n_pn && n_ctx == C_MAPVAL))) { bad(BAD_YAML); return; }
        uint32_t r = n_rel, p = n_parent;
        if (tag < 21 && kYFn[tag].seq) {
          if (!open_fn(r, p, tag, ml, mc)) return;
          p = top.slot;
          r = child();
        }
        if (!open(r, p, Y_BSEQ, c2 | (c2 == n_pn ? (1 << 30) : 0), ml, mc)) return;
        ccol = (uint32_t)c2; eof = false; state = S_LINE;
        continue;
      }
    }
    const uint32_t cc = column();
    if (c == '-' && yblank(T.at(i + 1))) {
      if (n_ctx == C_MAPVAL || tag != ~0u) { bad(BAD_YAML); return; }
      uint32_t r = n_rel, p = n_parent;
      if (tag != ~0u && tag < 21 && kYFn[tag].seq) {
        if (!open_fn(r, p, tag, ml, mc)) return;
        p = top.slot;
        r = child();
      }
      const uint32_t lm = (r == 0 && p == NONE) ? 0u : ml, cm = (r == 0 && p == NONE) ? 0u : mc;   // a root list: (0,0)
      if (!open(r, p, Y_BSEQ, (int32_t)cc | ((int32_t)cc == n_pn ? (1 << 30) : 0), lm, cm)) return;
      ccol = cc; eof = false; state = S_LINE;
      continue;
    }
    if (c == '[' || c == '{') {
      const bool root = n_rel == 0 && n_parent == NONE;
      flow(n_rel, n_parent, tag, root && c == '[' ? 0u : ml, root && c == '[' ? 0u : mc);
      if (!ok) return;
      state = S_AFTER;
      continue;
    }
    if ((c == '|' || c == '>') && n_ctx != C_ROOT) {
      // a block scalar: its lines are consumed here; the line that ends it is the next content line
      struct Skip {
        __device__ void byte(uint32_t) {}
        __device__ void run(const Text&, uint32_t, uint32_t) {}
      } sk;
      uint32_t nl = 0;
      const uint64_t e = decode_block(T, i, sk, n_pn, &nl);
      if (!e) { bad(BAD_YAML); return; }
      scalar_value(n_rel, n_parent, i, 0, c, tag, ml, mc);
      if (!ok) return;
      i = e; ls = e; line += nl; cont = 0;
      eof = !next_line();
      if (!ok) return;
      ccol = eof ? 0 : column();
      close_fns();
      state = S_LINE;
      continue;
    }
    if (c == '\n' || c == 256u || c == '#' || c == '|' || c == '>' || c == '&' || c == '*' || c == '?' || c == '%' ||
        c == '@' || c == '`' || c == ',' || c == ']' || c == '}' || c == '\t' || c == '\r') {
      bad(BAD_YAML);
      return;
    }
    const uint64_t s = i;
    const uint32_t cont_s = cont, line_s = line;
    uint32_t L = 0, style = 0;
    if (c == '"' || c == '\'') {
      style = c;
      if (!scan_quoted()) return;
    } else {
      uint64_t e = 0;
      if (!scan_plain(false, &e)) return;
      L = (uint32_t)(e - s);
      i = e;
    }
    const uint64_t after = i;
    sp_skip();
    if (T.at(i) == ':' && yblank(T.at(i + 1)) && line == line_s) {
      // a key: a block mapping at this column (the mapping loop reads the key again)
      if (n_ctx == C_MAPVAL || tag != ~0u) { bad(BAD_YAML); return; }
      if (!open(n_rel, n_parent, Y_BMAP, (int32_t)cc, ml, mc)) return;
      i = s; cont = cont_s;
      ccol = cc; eof = false; state = S_LINE;
      continue;
    }
    i = after;
    if (n_ctx == C_ROOT) { bad(BAD_YAML); return; }   // a scalar document: the host loads it
    scalar_value(n_rel, n_parent, s, L, style, tag, ml, mc);
    if (!ok) return;
    state = S_AFTER;
  }
  if (!ok) return;
  if (SEG) {
    if (MODE == M_COUNT) { seg->nn = nn; seg->nc = nc; seg->ns = ns; }
    return;
  }
  if (sp) { bad(BAD_YAML); return; }
  if (MODE == M_COUNT) { A.n_nodes[d] = nn; A.n_cont[d] = nc; A.n_str[d] = ns; }
}

// the YAML passes: documents the JSON count pass found not to start with { or [ (BAD_NOTJSON)
template <uint32_t MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) yaml_pass_kernel(JArgs A) {
  for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < A.ndocs; d += gridDim.x * blockDim.x) {
    if (*A.bad) return;
    if (MODE == M_COUNT) {
      if (A.doc_bad[d] != BAD_NOTJSON) continue;
      A.doc_bad[d] = 0;
      A.is_yaml[d] = 1;
      parse_yaml_doc<M_COUNT>(A, d);
      if (A.doc_bad[d]) { A.is_yaml[d] = 0; A.n_nodes[d] = 0; A.n_cont[d] = 0; A.n_str[d] = 0; }
    } else {
      if (!A.is_yaml[d] || A.doc_bad[d]) continue;
      parse_yaml_doc<MODE>(A, d);
    }
  }
}
