// Cooperative parse of large block-style YAML documents: a workgroup of 256 lanes per document for the
// line index and the segmentation, then a lane per segment (included by json_gpu.hip after yaml_gpu.inc
// and json_coop.inc).  The lane passes give a CloudFormation template of 64 KB to 1 MB to one lane; here the
// document is cut at the entries of its root collection and, below a root `key:` that holds nothing else
// on its line, at the entries of that key's collection (a template's Resources), and every piece is parsed
// by the lane parser itself (parse_yaml_doc<MODE, true>), started from a descriptor.  The kernels leave
// exactly what the lane passes leave (n_nodes / n_cont / n_str, the 16-bit child counts in container
// pre-order, one NodeRec per node), so the own, fix / verify and merge passes run on their output unchanged:
//   index    the text in 4 KB tiles, 16 bytes a lane: newline, space and CR masks; a line's record is written
//            where its indentation ends (offset, indentation, class: blank, comment, `- ` entry, `---`,
//            other).  Whether a lane's first byte still lies in a line's indentation is carried lane ->
//            wave -> workgroup -> tile as that line's start (a lane of 16 spaces passes on what it receives);
//            the records are compacted by a prefix sum over the same levels.  A count instantiation sizes
//            the buffer exactly.
//   segment  over the line records: the root collection's kind and entries, the split headers (one lane per
//            root entry reads its header line), the entries below them; a prefix sum numbers the segments.
//            A count instantiation sizes the descriptors.
//   parse    count, then emit, one lane per segment.
//   fix      between them, per document: prefix sums of the segments' node, container and string totals
//            give every segment its first container ordinal and children-block slot and its open frame;
//            the child counts move from segment order to the document's container order.
// The index cannot know that a line continues a multi-line scalar or flow collection, which the lane
// parser refuses anyway: a segment that does not end exactly where the next one starts, with exactly the
// predicted frames open, refuses its document (yaml_gpu.inc, S_LINE), and the host loader builds it.

enum : uint32_t { YL_BLANK = 0, YL_COMMENT = 1, YL_DASH = 2, YL_DOC = 3, YL_OTHER = 4 };
struct YLine { uint32_t off, meta; };   // the first byte past the indentation; indentation | class << 16

__device__ inline uint32_t ytext(const JArgs& A, uint64_t b0, uint32_t len, uint32_t p) { return p < len ? A.text[b0 + p] : 256u; }

template <bool EMIT>
__global__ void __launch_bounds__(256) yaml_coop_index_kernel(JArgs A) {
  __shared__ uint32_t s_pend[4], s_known[4], s_cnt[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  for (uint32_t ci = blockIdx.x; ci < A.nycoop; ci += gridDim.x) {
    const uint32_t d = A.ycoop_list[ci];
    if (EMIT && A.doc_bad[d]) continue;
    const uint64_t b0 = A.off[d], b1 = A.off[d + 1];
    const uint32_t len = (uint32_t)(b1 - b0);
    YLine* out = EMIT ? A.ylines + A.tok_base[d] : nullptr;
    // what the tiles before this one leave: 1 + the start of the line whose indentation the tile begins
    // in (0: it begins past it), and the lines so far
    uint32_t pend_c = 1, nline_c = 0, why = 0;
    for (uint64_t tile = b0 & ~15ull; tile < b1; tile += kCoopTile) {
      const uint64_t g = tile + (uint64_t)tid * 16u;
      uint4 w = make_uint4(0, 0, 0, 0);
      uint32_t valid = 0;
      if (g < b1) {
        w = *(const uint4*)(A.text + g);   // aligned; the text ends in 16 bytes of padding
        const uint32_t lo = g < b0 ? (uint32_t)(b0 - g) : 0u, hi = b1 - g < 16 ? (uint32_t)(b1 - g) : 16u;
        valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
      }
      const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
      uint32_t nl = 0, ns = 0;   // line breaks; bytes that end an indentation (anything but a space)
#pragma unroll
      for (uint32_t k = 0; k < 16; k++) {
        const uint32_t bit = 1u << k, c = (wd[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
        if (!(valid & bit)) continue;   // outside the document: a space
        if (c == '\n') nl |= bit;
        if (c != ' ') ns |= bit;
        if (c == '\r') why = BAD_YAML;
      }
      const uint32_t rel = (uint32_t)(g - b0);   // (wraps in the one lane that starts before the document)
      // a lane with a byte other than a space knows what it passes on: the start of its last line when only
      // spaces follow that line's break, else nothing
      uint32_t mine = 0;
      if (nl) {
        const uint32_t jl = 32u - (uint32_t)__clz(nl);   // the byte after the last break (16: the next lane's first)
        if (!(ns >> jl)) mine = rel + jl + 1u;
      }
      const uint64_t kn = __ballot(ns != 0);
      const uint32_t last = __shfl(mine, kn ? 63 - __clzll((long long)kn) : 0);
      const uint32_t prev = __shfl(mine, (kn & lt) ? 63 - __clzll((long long)(kn & lt)) : 0);
      if (lane == 0) { s_known[wave] = kn != 0; s_pend[wave] = last; }
      __syncthreads();
      uint32_t pend = pend_c, pend_n = pend_c;
      for (uint32_t v = 0; v < 4; v++) {
        if (s_known[v]) { pend_n = s_pend[v]; if (v < wave) pend = pend_n; }
      }
      if (kn & lt) pend = prev;
      // line starts in this window (bit 0: the line carried in), and for each the byte that ends its indentation
      const uint32_t lsm = ((nl << 1) & 0xFFFFu) | (pend ? 1u : 0u);
      uint32_t ev = 0;
      for (uint32_t m = lsm; m; m &= m - 1u) {
        const uint32_t r = ns & (0xFFFFu << __builtin_ctz(m));
        ev |= r & (0u - r);
      }
      const uint32_t n = (uint32_t)__popc(ev), in = wave_incl_sum(n, lane);
      if (lane == 63) s_cnt[wave] = in;
      __syncthreads();
      uint32_t at = nline_c + in - n, tot = 0;
      for (uint32_t v = 0; v < 4; v++) { tot += s_cnt[v]; if (v < wave) at += s_cnt[v]; }
      for (uint32_t e = ev; e; e &= e - 1u, at++) {
        const uint32_t k = (uint32_t)__builtin_ctz(e);
        const uint32_t j = 31u - (uint32_t)__clz(lsm & ((2u << k) - 1u));
        const uint32_t p = rel + k, start = (j == 0 && pend) ? pend - 1u : rel + j, indent = p - start;
        const uint32_t c0 = ytext(A, b0, len, p), c1 = ytext(A, b0, len, p + 1);
        uint32_t cls = YL_OTHER;
        if (c0 == '\n') cls = YL_BLANK;
        else if (c0 == '#') cls = YL_COMMENT;
        else if (c0 == '\t') why = BAD_YAML;   // a tab in the indentation
        else if (c0 == '-' && yblank(c1)) cls = YL_DASH;
        else if ((c0 == '-' || c0 == '.') && indent == 0 && c1 == c0 && ytext(A, b0, len, p + 2) == c0 && yblank(ytext(A, b0, len, p + 3))) {
          if (c0 == '.') why = BAD_YAML;   // a document end marker
          cls = YL_DOC;
        }
        if (indent > 0xFFFFu) why = BAD_YAML;
        if (EMIT) { YLine o; o.off = p; o.meta = (indent & 0xFFFFu) | (cls << 16); out[at] = o; }
      }
      pend_c = pend_n; nline_c += tot;
    }
    // the text ends inside an indentation: a last line of spaces only
    if (pend_c && pend_c - 1u < len) {
      if (EMIT && tid == 0) { YLine o; o.off = len; o.meta = ((len - (pend_c - 1u)) & 0xFFFFu) | (YL_BLANK << 16); out[nline_c] = o; }
      nline_c++;
    }
    if (!EMIT) {
      if (why) coop_refuse(A, d, why);
      if (tid == 0) A.n_tok[d] = nline_c;
    }
  }
}

// line records -> segments.  Root entries: the content lines at column 0 from the root's first line on (a
// root mapping: not `- ` lines, which belong to an indentless sequence under the key before them; a root
// sequence: `- ` lines).  A root mapping entry whose line is `key:` and nothing else (a plain key; blanks
// or a comment may follow) and whose next content line is indented, or a `- ` line at column 0, is a split
// header: its segment ends after its collection's first entry, and every further content line at that
// line's indentation (of its kind: `- ` lines in a sequence, others in a mapping) starts a segment.
template <bool EMIT>
__global__ void __launch_bounds__(256) yaml_coop_segment_kernel(JArgs A) {
  __shared__ uint32_t s_first[2], s_bad, s_p[4];
  // a root mapping's entries (at most kMaxPairwiseKeys): line; split << 31 | sequence << 30 | indentation;
  // its collection's first entry line; its segment
  __shared__ uint32_t s_rline[kMaxPairwiseKeys + 1], s_rmeta[kMaxPairwiseKeys], s_rfc[kMaxPairwiseKeys], s_rseg[kMaxPairwiseKeys + 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t ci = blockIdx.x; ci < A.nycoop; ci += gridDim.x) {
    const uint32_t d = A.ycoop_list[ci];
    __syncthreads();   // the previous document's shared state is read no more
    if (A.doc_bad[d]) continue;
    const uint64_t b0 = A.off[d];
    const uint32_t len = (uint32_t)(A.off[d + 1] - b0), nl = A.n_tok[d];
    const YLine* L = A.ylines + A.tok_base[d];
    YSeg* S = EMIT ? A.ysegs + A.seg_base[d] : nullptr;
    if (tid < 2) s_first[tid] = NONE;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    // the first content line; with a `---` there, the first one after it (no other line may be a marker)
    for (uint32_t l = tid; l < nl; l += 256) if ((L[l].meta >> 16) >= YL_DASH) atomicMin(&s_first[0], l);
    __syncthreads();
    const uint32_t f0 = s_first[0];
    const bool marker = f0 != NONE && (L[f0].meta >> 16) == YL_DOC;
    for (uint32_t l = tid; l < nl; l += 256) {
      const uint32_t cls = L[l].meta >> 16;
      if (cls == YL_DOC && l != f0) s_bad = BAD_YAML;
      if (marker && l > f0 && cls >= YL_DASH) atomicMin(&s_first[1], l);
    }
    __syncthreads();
    const uint32_t fr = marker ? s_first[1] : f0;
    if (s_bad || fr == NONE || (L[fr].meta & 0xFFFFu)) {   // a second document, no content, an indented root
      if (tid == 0) coop_refuse(A, d, BAD_YAML);
      continue;
    }
    const bool rseq = (L[fr].meta >> 16) == YL_DASH;
    const uint32_t rc0 = ytext(A, b0, len, L[fr].off);
    if (rc0 == '[' || rc0 == '{') {
      // a flow collection as the root: one segment, the whole document
      if (tid == 0) {
        if (EMIT) {
          YSeg o{};
          o.doc = d; o.start = 0; o.end = len; o.line = 0; o.flags = YS_FIRST | YS_WHOLE; o.hdr = NONE;
          S[0] = o;
        } else A.n_seg[d] = 1;
      }
      continue;
    }
    auto is_root = [&](uint32_t l) {
      if (l < fr || l >= nl) return false;
      const uint32_t m = L[l].meta;
      return (m & 0xFFFFu) == 0 && (m >> 16) == (rseq ? YL_DASH : YL_OTHER);
    };
    uint32_t R = 0;
    if (!rseq) {
      // the root mapping's entry lines, in order
      for (uint32_t l0 = fr; l0 < nl; l0 += 256) {
        const bool r = is_root(l0 + tid);
        const uint64_t rb = __ballot(r);
        if (lane == 0) s_p[wave] = (uint32_t)__popcll(rb);
        __syncthreads();
        uint32_t at = R + (uint32_t)__popcll(rb & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < 4; v++) { if (v < wave) at += s_p[v]; R += s_p[v]; }
        if (r && at < kMaxPairwiseKeys) s_rline[at] = l0 + tid;
        __syncthreads();
      }
      if (R > kMaxPairwiseKeys) {   // more keys than the verify pass's duplicate-key scan takes
        if (tid == 0) coop_refuse(A, d, BAD_WIDEMAP);
        continue;
      }
      if (tid == 0) s_rline[R] = nl;
      __syncthreads();
      if (tid < R) {
        // the header line: a key, its `:` (a plain key: the first one before a blank, as scan_plain ends the
        // key), then blanks and a comment at most
        uint32_t meta = 0, fc = 0, p = L[s_rline[tid]].off, c = ytext(A, b0, len, p);
        bool head = true;
        if (c == '"' || c == '\'') {
          // a quoted key: to its closing quote on this line (\x escapes, '' in single quotes), then blanks
          const uint32_t q = c;
          for (p++; head; p++) {
            c = ytext(A, b0, len, p);
            if (c == '\n' || c == 256u) head = false;
            else if (q == '"' && c == '\\') p++;
            else if (c == q) { if (q == '\'' && ytext(A, b0, len, p + 1) == q) p++; else break; }
          }
          if (head) {
            p++;
            while (ytext(A, b0, len, p) == ' ') p++;
            head = ytext(A, b0, len, p) == ':' && yblank(ytext(A, b0, len, p + 1));
          }
        }
        else for (; head; p++) {
          c = ytext(A, b0, len, p);
          if (c == '\n' || c == 256u || (c == '#' && ytext(A, b0, len, p - 1) == ' ')) head = false;
          else if (c == ':' && yblank(ytext(A, b0, len, p + 1))) break;
        }
        if (head) {
          p++;
          while (ytext(A, b0, len, p) == ' ') p++;
          c = ytext(A, b0, len, p);
          head = c == '\n' || c == 256u || c == '#';
        }
        if (head) {
          uint32_t l = s_rline[tid] + 1;
          while (l < s_rline[tid + 1] && (L[l].meta >> 16) < YL_DASH) l++;
          if (l < s_rline[tid + 1]) {   // (indented, or a `- ` line at column 0: a root entry line is neither)
            const uint32_t m = L[l].meta;
            meta = 0x80000000u | ((m >> 16) == YL_DASH ? 0x40000000u : 0u) | (m & 0xFFFFu);
            fc = l;
          }
        }
        s_rmeta[tid] = meta; s_rfc[tid] = fc;
      }
      __syncthreads();
    }
    // segment starts, numbered in document order
    uint32_t rcount = 0, nseg = 0;   // root entries and segments before this tile
    for (uint32_t l0 = fr; l0 < nl; l0 += 256) {
      const uint32_t l = l0 + tid;
      const bool root = is_root(l);
      const uint64_t rb = __ballot(root);
      if (lane == 0) s_p[wave] = (uint32_t)__popcll(rb);
      __syncthreads();
      uint32_t e = rcount + (uint32_t)__popcll(rb & ((2ull << lane) - 1ull));   // root entries up to and with this line
      uint32_t rtot = 0;
      for (uint32_t v = 0; v < 4; v++) { if (v < wave) e += s_p[v]; rtot += s_p[v]; }
      e--;   // the root entry this line lies under (from fr on there is one)
      bool sub = false;
      uint32_t hm = 0;
      if (!rseq && l < nl && !root) {
        hm = s_rmeta[e];
        const uint32_t m = L[l].meta, cls = m >> 16;
        sub = (hm >> 31) && cls >= YL_DASH && (m & 0xFFFFu) == (hm & 0xFFFFu) && (cls == YL_DASH) == ((hm >> 30) & 1u) &&
              l != s_rfc[e];
      }
      __syncthreads();
      const bool startsg = root || sub;
      const uint64_t sb = __ballot(startsg);
      if (lane == 0) s_p[wave] = (uint32_t)__popcll(sb);
      __syncthreads();
      uint32_t s = nseg + (uint32_t)__popcll(sb & ((1ull << lane) - 1ull)), stot = 0;
      for (uint32_t v = 0; v < 4; v++) { if (v < wave) s += s_p[v]; stot += s_p[v]; }
      if (root && !rseq) s_rseg[e] = s;
      __syncthreads();
      if (EMIT && startsg) {
        // every field but `end` (the next segment's lane writes it), the spine's child counts and the rest
        // of the frame (below, and the fix kernel)
        YSeg& o = S[s];
        o.doc = d; o.hdr = NONE; o.hu = 0; o.nspine = 0; o.flags = 0;
        o.nn = 0; o.nc = 0; o.ns = 0; o.cbase = 0; o.next = 0;
        o.f.kind = 0; o.f.indent = 0; o.f.slot = 0; o.f.k = 0; o.f.first = 0; o.f.cnt = 0;
        for (uint32_t u = 0; u < 2; u++) { o.skind[u] = 0; o.sindent[u] = 0; o.scnt[u] = 0; }
        if (s == 0) { o.start = 0; o.line = 0; o.flags = YS_FIRST; }
        else { o.start = L[l].off - (L[l].meta & 0xFFFFu); o.line = l; S[s - 1].end = o.start; }
        // a split header's collection: its kind and its column (an indentless sequence: at the key's)
        const uint32_t hd = rseq ? 0u : s_rmeta[e], hseq = (hd >> 30) & 1u;
        const uint32_t hkind = hseq ? Y_BSEQ : Y_BMAP;
        const int32_t hind = (int32_t)((hd & 0xFFFFu) | (hseq && !(hd & 0xFFFFu) ? 1u << 30 : 0u));
        if (root) {
          o.f.j = e;
          o.f.kind = rseq ? Y_BSEQ : Y_BMAP;
          if (s == 0) { o.skind[0] = o.f.kind; o.nspine = 1; }
          else o.hdr = 0;
          if (hd >> 31) { o.skind[o.nspine] = hkind; o.sindent[o.nspine] = hind; o.nspine++; }
        } else {
          o.hdr = s_rseg[e];
          o.hu = o.hdr == 0 ? 1u : 0u;   // segment 0 opens the root before its header's collection
          o.f.j = s - o.hdr;
          o.f.kind = hkind; o.f.indent = hind;
        }
      }
      rcount += rtot; nseg += stot;
      __syncthreads();
    }
    if (rseq) R = rcount;
    // the spine's child counts: the root's entries, a split header's segments
    if (R > 0xFFFFu) { if (tid == 0) coop_refuse(A, d, BAD_WIDE); continue; }
    if (!rseq) {
      if (tid == 0) s_rseg[R] = nseg;
      __syncthreads();
      if (tid < R && (s_rmeta[tid] >> 31)) {
        const uint32_t h = s_rseg[tid], c = s_rseg[tid + 1] - h;
        if (c > 0xFFFFu) coop_refuse(A, d, BAD_WIDE);
        else if (EMIT) S[h].scnt[S[h].nspine - 1] = c;
      }
    }
    if (tid == 0) {
      if (EMIT) { S[0].scnt[0] = R; S[nseg - 1].end = len; }
      else A.n_seg[d] = nseg;
    }
  }
}

// one lane per segment: the lane parser, started from the segment's descriptor
template <uint32_t MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) yaml_coop_parse_kernel(JArgs A) {
  for (uint64_t s = blockIdx.x * blockDim.x + threadIdx.x; s < A.nsegs; s += (uint64_t)gridDim.x * blockDim.x) {
    if (*A.bad) return;
    YSeg* sg = A.ysegs + s;
    const uint32_t d = sg->doc;
    if (d >= A.ndocs || A.doc_bad[d]) continue;
    parse_yaml_doc<MODE, true>(A, d, sg);
  }
}

// after the count pass, per document: every segment's first container ordinal and children-block slot
// (prefix sums over the segments in document order), its open frame, the document's totals, and the
// child counts in the document's container order
__global__ void __launch_bounds__(256) yaml_coop_fix_kernel(JArgs A) {
  __shared__ uint32_t s_a[4], s_b[4], s_tot[3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t ci = blockIdx.x; ci < A.nycoop; ci += gridDim.x) {
    const uint32_t d = A.ycoop_list[ci];
    __syncthreads();
    if (A.doc_bad[d]) continue;
    const uint32_t nseg = A.n_seg[d];
    YSeg* S = A.ysegs + A.seg_base[d];
    const uint64_t cb = A.off[d] >> 1;
    if (tid < 3) s_tot[tid] = 0;
    // a segment opens its containers in order, the spine first; the blocks it lays out are the children of
    // the containers it closes (all its nodes but its entry and the spine's first entries) and the spine's
    uint32_t cbase = 0, next = 1, tn = 0, ts = 0;
    for (uint32_t t0 = 0; t0 < nseg; t0 += 256) {
      const uint32_t t = t0 + tid;
      uint32_t nc = 0, al = 0;
      if (t < nseg) {
        const YSeg& g = S[t];
        nc = g.nc;
        al = g.nn - 1u - g.nspine;
        for (uint32_t u = 0; u < g.nspine; u++) al += g.scnt[u];
        tn += g.nn; ts += g.ns;
      }
      const uint32_t ic = wave_incl_sum(nc, lane), ia = wave_incl_sum(al, lane);
      if (lane == 63) { s_a[wave] = ic; s_b[wave] = ia; }
      __syncthreads();
      uint32_t c = cbase + ic - nc, x = next + ia - al;
      for (uint32_t v = 0; v < 4; v++) {
        if (v < wave) { c += s_a[v]; x += s_b[v]; }
        cbase += s_a[v]; next += s_b[v];
      }
      if (t < nseg) { S[t].cbase = c; S[t].next = x; }
      __syncthreads();
    }
    atomicAdd(&s_tot[0], tn); atomicAdd(&s_tot[1], ts);
    __syncthreads();
    // every node is some container's child, or the root; the containers fit the document's count slots
    if (next != s_tot[0] || cbase > ((A.off[d + 1] - A.off[d]) >> 1)) {
      if (tid == 0) coop_refuse(A, d, BAD_YAML);
      continue;
    }
    if (tid == 0) { A.n_nodes[d] = s_tot[0]; A.n_cont[d] = cbase; A.n_str[d] = s_tot[1]; }
    for (uint32_t t = tid; t < nseg; t += 256) {
      YSeg& g = S[t];
      if (g.hdr != NONE) {
        // the frame it starts in: spine container hu of segment hdr -- the root (node 0, its children from
        // node 1), or a split header's collection (the root's child of the header's ordinal)
        const YSeg& h = S[g.hdr];
        const uint32_t u = g.hu;
        g.f.kind = h.skind[u]; g.f.indent = h.sindent[u]; g.f.cnt = h.scnt[u];
        g.f.k = h.cbase + u;
        g.f.first = h.next + (u ? h.scnt[0] : 0u);
        g.f.slot = (u == 0 && (h.flags & YS_FIRST)) ? 0u : 1u + h.f.j;
      }
      const uint64_t from = cb + (g.start >> 1), to = cb + g.cbase;
      for (uint32_t u = 0; u < g.nspine; u++) A.counts[to + u] = (uint16_t)g.scnt[u];
      for (uint32_t k = g.nspine; k < g.nc; k++) A.counts[to + k] = A.ycnt[from + k];
    }
  }
}
