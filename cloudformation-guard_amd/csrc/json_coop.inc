// Cooperative parse of large JSON documents: a workgroup of 256 lanes per document (included by
// json_gpu.hip).  The lane passes give a document to one lane, which leaves the device idle on a batch
// of a few thousand Terraform plans of a megabyte each; here no lane walks a document.  Three kernels
// produce exactly what the lane passes produce (n_nodes / n_cont / n_str, the 16-bit child counts, one
// NodeRec per node), so the own, fix / verify and merge passes run on their output unchanged:
//   index   the text in 4 KB tiles, 16 bytes a lane: byte-class masks, escapes (ends of odd backslash
//           runs), the in-string mask (prefix XOR of the unescaped quotes), depth, line and column as
//           prefix scans over lane -> wave -> workgroup -> tile, and the tokens outside strings (value
//           starts, closers, colons, commas) compacted into the document's token buffer.  A count
//           instantiation sizes that buffer exactly.
//   tree    the tokens in tiles of 256: each token finds its enclosing container (the nearest earlier
//           open token one level up: a backward walk over the tile in LDS, then a per-level carry) and
//           the commas of that container before it (its sibling ordinal); the grammar is checked
//           against the predecessor token and the container's kind; closers record child counts; a
//           second sweep turns the counts into block bases (host layout: JsonFast::v2).
//   emit    one lane per value token writes the node's NodeRec through the lane parser's own string,
//           number and intern functions.
// Anything these kernels cannot prove to be inside the lane parser's subset refuses the document: the
// host loader builds it then (json_gpu.hip header).  No recursion, no per-lane stack.

enum : uint32_t { TK_OMAP = 0, TK_OLIST = 1, TK_CMAP = 2, TK_CLIST = 3, TK_COLON = 4, TK_COMMA = 5, TK_STR = 6, TK_SCALAR = 7, TK_NONE = 0xFF };

// depth: open tokens -- the depth outside; closers -- the depth after; the others -- the depth they sit at
struct Tok { uint32_t off, line, col, meta; };   // meta: kind | depth << 8
// tree kernel -> emit: the enclosing container's open token, the ordinal among its elements, and for an
// open token its child count and the document-relative node of its first child
struct TokAux { uint32_t ptok, ord, cnt, base; };

static const uint32_t kCoopTile = 4096;   // bytes a workgroup takes per step: 256 lanes x one uint4

__device__ inline uint32_t wave_incl_sum(uint32_t v, uint32_t lane) {
  for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(v, o); if (lane >= o) v += u; }
  return v;
}
__device__ inline uint32_t wave_incl_max(uint32_t v, uint32_t lane) {
  for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(v, o); if (lane >= o && u > v) v = u; }
  return v;
}
__device__ inline void coop_refuse(const JArgs& A, uint32_t d, uint32_t why) { atomicCAS(&A.doc_bad[d], 0u, why); }

template <bool EMIT>
__global__ void __launch_bounds__(256) json_coop_index_kernel(JArgs A) {
  __shared__ uint32_t s_esc[4], s_par[4], s_sum1[4], s_sum2[4], s_max[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  for (uint32_t ci = blockIdx.x; ci < A.ncoop; ci += gridDim.x) {
    const uint32_t d = A.coop_list[ci];
    if (EMIT && A.doc_bad[d]) continue;
    const uint64_t b0 = A.off[d], b1 = A.off[d + 1];
    const uint64_t tb = EMIT ? A.tok_base[d] : 0;
    // what the tiles before this one leave, the same in every lane
    uint32_t esc_c = 0, par_c = 0, line_c = 0, P_c = 0, ls_c = 0, ntok_c = 0, why = 0;
    int32_t depth_c = 0;
    for (uint64_t tile = b0 & ~15ull; tile < b1; tile += kCoopTile) {
      const uint64_t g = tile + (uint64_t)tid * 16u;
      uint4 w = make_uint4(0, 0, 0, 0);
      uint32_t valid = 0;   // the bytes of this lane's window inside the document
      if (g < b1) {
        w = *(const uint4*)(A.text + g);   // aligned; the text ends in 16 bytes of padding
        const uint32_t lo = g < b0 ? (uint32_t)(b0 - g) : 0u, hi = b1 - g < 16 ? (uint32_t)(b1 - g) : 16u;
        valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
      }
      const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
      uint32_t bs = 0, qt = 0, om = 0, ol = 0, cm = 0, cl = 0, co = 0, cma = 0, wsm = 0, nl = 0, ctl = 0, ncm = 0;
#pragma unroll
      for (uint32_t k = 0; k < 16; k++) {
        const uint32_t bit = 1u << k;
        uint32_t c = (wd[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
        if (!(valid & bit)) c = ' ';   // outside the document: whitespace that counts for no column
        else if ((c & 0xC0u) != 0x80u) ncm |= bit;   // marks count characters: not a UTF-8 continuation byte
        if (c == '\\') bs |= bit;
        if (c == '"') qt |= bit;
        if (c == '{') om |= bit;
        if (c == '[') ol |= bit;
        if (c == '}') cm |= bit;
        if (c == ']') cl |= bit;
        if (c == ':') co |= bit;
        if (c == ',') cma |= bit;
        if (c == ' ' || c == '\n') wsm |= bit;
        if (c == '\n') nl |= bit;
        if (c < 0x20u || c == 0x7Fu) ctl |= bit;
      }
      // escapes: a byte after an odd run of backslashes.  Whether this lane's last byte escapes the next
      // lane's first: a lane whose backslashes do not fill it knows (its trailing run's parity), a lane
      // of 16 backslashes passes on what it receives.
      const uint32_t nbs = ~bs & 0xFFFFu;
      const uint32_t run = nbs ? (uint32_t)__clz(nbs) - 16u : 16u;
      const uint64_t kn = __ballot(run < 16u), od = __ballot(run < 16u && (run & 1u));
      if (lane == 0) s_esc[wave] = kn ? 2u | (uint32_t)((od >> (63 - __clzll((long long)kn))) & 1ull) : 0u;
      __syncthreads();
      uint32_t ec = esc_c, esc_n = esc_c;
      for (uint32_t v = 0; v < 4; v++) {
        if (s_esc[v] & 2u) { esc_n = s_esc[v] & 1u; if (v < wave) ec = esc_n; }
      }
      if (kn & lt) ec = (uint32_t)((od >> (63 - __clzll((long long)(kn & lt)))) & 1ull);
      uint32_t escaped = 0;
#pragma unroll
      for (uint32_t k = 0; k < 16; k++) {
        const uint32_t bit = 1u << k;
        if (ec) { escaped |= bit; ec = 0; }
        else if (bs & bit) ec = 1;
      }
      // in-string mask: prefix XOR of the unescaped quotes (set from an opening quote to the byte before
      // the closing one), flipped by the parity of the quotes in the lanes, waves and tiles before
      const uint32_t uq = qt & ~escaped;
      uint32_t px = uq;
      px ^= px << 1; px ^= px << 2; px ^= px << 4; px ^= px << 8;
      px &= 0xFFFFu;
      const uint64_t ob = __ballot(__popc(uq) & 1u);
      if (lane == 0) s_par[wave] = (uint32_t)__popcll(ob) & 1u;
      __syncthreads();
      uint32_t pc = par_c, par_n = par_c;
      for (uint32_t v = 0; v < 4; v++) { par_n ^= s_par[v]; if (v < wave) pc ^= s_par[v]; }
      pc ^= (uint32_t)__popcll(ob & lt) & 1u;
      const uint32_t in = pc ? (~px & 0xFFFFu) : px;
      const uint32_t out = ~in & ~uq & 0xFFFFu;   // outside strings and not a closing quote
      const uint32_t sopen = uq & in;
      if (ctl & in) why = BAD_SYNTAX;   // a bare control byte (a line break included) or DEL in a string
      const uint32_t omk = (om | ol) & out, clk = (cm | cl) & out, cok = co & out, cmk = cma & out;
      // a number or literal: a run of other bytes outside strings; it starts after a separator (the byte
      // before this window read again: a lane's first byte outside a string follows no string content)
      const uint32_t sc = out & ~(om | ol | cm | cl | co | cma | wsm);
      uint32_t pb = ' ';
      if ((sc & 1u) && g > b0) pb = A.text[g - 1];
      const bool psep = pb == ' ' || pb == '\n' || pb == '{' || pb == '}' || pb == '[' || pb == ']' || pb == ':' || pb == ',' || pb == '"';
      const uint32_t scs = sc & ~((sc << 1) | (psep ? 0u : 1u));
      const uint32_t tk = omk | clk | cok | cmk | sopen | scs;
      const uint32_t nlm = nl & out;
      // exclusive prefixes over the workgroup: newlines and characters, tokens and depth (+16 a lane, so
      // the packed sums stay unsigned)
      const uint32_t v1 = (uint32_t)__popc(nlm) | ((uint32_t)__popc(ncm) << 16);
      const uint32_t v2 = (uint32_t)__popc(tk) | (((uint32_t)__popc(omk) + 16u - (uint32_t)__popc(clk)) << 16);
      const uint32_t i1 = wave_incl_sum(v1, lane), i2 = wave_incl_sum(v2, lane);
      if (lane == 63) { s_sum1[wave] = i1; s_sum2[wave] = i2; }
      __syncthreads();
      uint32_t e1 = i1 - v1, e2 = i2 - v2, t1 = 0, t2 = 0;
      for (uint32_t v = 0; v < 4; v++) {
        t1 += s_sum1[v]; t2 += s_sum2[v];
        if (v < wave) { e1 += s_sum1[v]; e2 += s_sum2[v]; }
      }
      const uint32_t line0 = line_c + (e1 & 0xFFFFu), P0 = P_c + (e1 >> 16);
      const uint32_t tok0 = ntok_c + (e2 & 0xFFFFu);
      const int32_t depth0 = depth_c + (int32_t)(e2 >> 16) - 16 * (int32_t)tid;
      // the character count at the latest line start: the count is monotone, so a prefix maximum carries it
      uint32_t lsv = 0;
      if (nlm) lsv = P0 + (uint32_t)__popc(ncm & ((2u << (31 - __clz(nlm))) - 1u));
      const uint32_t im = wave_incl_max(lsv, lane);
      uint32_t ex = __shfl_up(im, 1);
      if (lane == 0) ex = 0;
      if (lane == 63) s_max[wave] = im;
      __syncthreads();
      uint32_t ls = ls_c > ex ? ls_c : ex, ls_n = ls_c;
      for (uint32_t v = 0; v < 4; v++) {
        if (s_max[v] > ls_n) ls_n = s_max[v];
        if (v < wave && s_max[v] > ls) ls = s_max[v];
      }
      // this lane's tokens, in order
      int32_t dep = depth0;
      uint32_t ln = line0, t = tok0, ev = tk | nlm;
      while (ev) {
        const uint32_t k = (uint32_t)__builtin_ctz(ev), bit = 1u << k;
        ev &= ev - 1u;
        if (nlm & bit) { ln++; ls = P0 + (uint32_t)__popc(ncm & ((2u << k) - 1u)); continue; }
        uint32_t kind, dd;
        if (omk & bit) {
          kind = (om & bit) ? TK_OMAP : TK_OLIST;
          if (dep >= (int32_t)kMaxDepth && !why) why = BAD_DEPTH;
          dd = (uint32_t)dep;
          dep++;
        } else if (clk & bit) {
          kind = (cm & bit) ? TK_CMAP : TK_CLIST;
          dep--;
          if (dep < 0) why = BAD_SYNTAX;
          dd = (uint32_t)dep;
        } else {
          kind = (cok & bit) ? TK_COLON : ((cmk & bit) ? TK_COMMA : ((sopen & bit) ? TK_STR : TK_SCALAR));
          dd = (uint32_t)dep;
        }
        if (EMIT) {   // a refused document's tokens are never written: its depths are in [0, 64]
          Tok o;
          o.off = (uint32_t)(g + k - b0); o.line = ln; o.col = P0 + (uint32_t)__popc(ncm & (bit - 1u)) - ls;
          o.meta = kind | (dd << 8);
          A.toks[tb + t] = o;
        }
        t++;
      }
      esc_c = esc_n; par_c = par_n; ls_c = ls_n;
      line_c += t1 & 0xFFFFu; P_c += t1 >> 16; ntok_c += t2 & 0xFFFFu;
      depth_c += (int32_t)(t2 >> 16) - 16 * 256;
    }
    if (!EMIT) {
      // an unterminated string, an unclosed container, no token at all
      if (par_c || depth_c != 0 || ntok_c == 0) { if (!why) why = BAD_SYNTAX; }
      if (why) coop_refuse(A, d, why);
      if (tid == 0) A.n_tok[d] = ntok_c;
    }
  }
}

// tokens -> tree.  `lvl` is the depth of the container contents a token sits in: a value's, colon's or
// comma's own depth, a closer's depth after + 1; the enclosing container is the nearest earlier open
// token of depth lvl - 1 (depth moves by one per open / close, so it exists whenever lvl > 0).
__global__ void __launch_bounds__(256) json_coop_tree_kernel(JArgs A) {
  __shared__ uint32_t s_meta[256 + 2];   // this tile's tokens and the two before it
  // per level, what the tiles so far leave: the open token of the latest container whose contents are at
  // that level and the commas seen in it; s_last: the tile's last lane with news for the level (+1)
  __shared__ uint32_t s_cptok[kMaxDepth + 2], s_cord[kMaxDepth + 2], s_last[kMaxDepth + 2];
  __shared__ uint32_t s_p1[4], s_p2[4], s_tot[3], s_bad;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t ci = blockIdx.x; ci < A.ncoop; ci += gridDim.x) {
    const uint32_t d = A.coop_list[ci];
    __syncthreads();   // the previous document's shared state is read no more
    if (A.doc_bad[d]) continue;
    const uint32_t nt = A.n_tok[d];
    const Tok* tk = A.toks + A.tok_base[d];
    TokAux* ax = A.aux + A.tok_base[d];
    if (tid < kMaxDepth + 2) { s_cptok[tid] = NONE; s_cord[tid] = 0; s_last[tid] = 0; }
    if (tid < 3) s_tot[tid] = 0;
    if (tid == 0) s_bad = 0;
    uint32_t nval = 0, nstr = 0, ncont = 0;
    for (uint32_t t0 = 0; t0 < nt; t0 += 256) {
      const uint32_t t = t0 + tid;
      const bool have = t < nt;
      const uint32_t meta = have ? tk[t].meta : TK_NONE;
      s_meta[tid + 2] = meta;
      if (tid < 2) s_meta[tid] = t0 + tid >= 2 ? tk[t0 + tid - 2].meta : TK_NONE;
      __syncthreads();
      const uint32_t kind = meta & 0xFFu, dep = meta >> 8;
      const bool open = kind <= TK_OLIST, close = kind == TK_CMAP || kind == TK_CLIST;
      const uint32_t lvl = close ? dep + 1 : dep;
      uint32_t ptok = NONE, c = 0;
      if (have) {
        uint32_t pk = TK_NONE;   // the enclosing container's kind
        if (lvl > 0) {
          for (int32_t j = (int32_t)tid - 1; j >= 0; j--) {
            const uint32_t x = s_meta[j + 2], xk = x & 0xFFu, xd = x >> 8;
            if (xk <= TK_OLIST && xd == lvl - 1) { ptok = t0 + (uint32_t)j; pk = xk; break; }
            if (xk == TK_COMMA && xd == lvl) c++;
          }
          if (ptok == NONE) {
            ptok = s_cptok[lvl]; c += s_cord[lvl];
            if (ptok != NONE) pk = tk[ptok].meta & 0xFFu;
          }
        }
        const uint32_t p1k = t ? s_meta[tid + 1] & 0xFFu : TK_NONE, p2k = t > 1 ? s_meta[tid] & 0xFFu : TK_NONE;
        const bool pmap = pk == TK_OMAP;
        const bool first = p1k <= TK_OLIST || p1k == TK_COMMA;   // an element starts here
        // the predecessor completes a value (a string that is a map key does not)
        const bool p1key = p1k == TK_STR && pmap && (p2k == TK_COMMA || p2k <= TK_OLIST);
        const bool p1val = p1k == TK_SCALAR || p1k == TK_CMAP || p1k == TK_CLIST || (p1k == TK_STR && !p1key);
        bool ok, key = false;
        if (t == 0) ok = open && dep == 0;
        else if (lvl == 0 || pk > TK_OLIST) ok = false;   // after the root closed
        else if (kind == TK_STR && pmap) { key = first; ok = key || p1k == TK_COLON; }
        else if (open || kind == TK_SCALAR || kind == TK_STR) ok = pmap ? p1k == TK_COLON : first;
        else if (kind == TK_COLON) {
          // as the lane parser: the colon on the key's line, within 1000 bytes of its opening quote
          ok = pmap && p1key && tk[t].line == tk[t - 1].line && tk[t].off - tk[t - 1].off <= 1000u;
        } else if (kind == TK_COMMA) ok = p1val;
        else ok = pmap == (kind == TK_CMAP) && (p1k <= TK_OLIST || p1val);   // a closer: no trailing comma
        if (!ok) s_bad = BAD_SYNTAX;
        if (close) {
          const uint32_t cnt = p1k <= TK_OLIST ? 0u : c + 1u;
          if (cnt > 0xFFFFu) s_bad = BAD_WIDE;
          if (ok) ax[ptok].cnt = cnt;
        } else if (kind != TK_COLON && kind != TK_COMMA) {
          ax[t].ptok = ptok; ax[t].ord = c;
          if (kind == TK_STR) nstr++;
          if (!key) nval++;
          if (open) ncont++;
        }
        if (open) atomicMax(&s_last[dep + 1], tid + 1);
        if (kind == TK_COMMA) atomicMax(&s_last[lvl], tid + 1);
      }
      __syncthreads();
      if (have && open && s_last[dep + 1] == tid + 1) { s_cptok[dep + 1] = t; s_cord[dep + 1] = 0; }
      if (have && kind == TK_COMMA && s_last[lvl] == tid + 1) { s_cptok[lvl] = ptok; s_cord[lvl] = c + 1; }
      __syncthreads();
      if (tid < kMaxDepth + 2) s_last[tid] = 0;
    }
    atomicAdd(&s_tot[0], nval); atomicAdd(&s_tot[1], ncont); atomicAdd(&s_tot[2], nstr);
    __syncthreads();
    // child counts -> block bases: a container's children follow those of the containers opened before it
    // (pre-order = the text order of the open tokens); the counts go to the lane pass's place
    uint32_t kc = 0, bc = 1;
    const uint64_t cb = A.off[d] >> 1;
    if (!s_bad) {
      for (uint32_t t0 = 0; t0 < nt; t0 += 256) {
        const uint32_t t = t0 + tid;
        const bool open = t < nt && (tk[t].meta & 0xFFu) <= TK_OLIST;
        const uint32_t cnt = open ? ax[t].cnt : 0u;
        const uint64_t ob = __ballot(open);
        const uint32_t ic = wave_incl_sum(cnt, lane);
        if (lane == 63) { s_p1[wave] = (uint32_t)__popcll(ob); s_p2[wave] = ic; }
        __syncthreads();
        uint32_t k = kc + (uint32_t)__popcll(ob & ((1ull << lane) - 1ull)), base = bc + ic - cnt;
        for (uint32_t v = 0; v < 4; v++) {
          if (v < wave) { k += s_p1[v]; base += s_p2[v]; }
          kc += s_p1[v]; bc += s_p2[v];
        }
        if (open) { ax[t].base = base; A.counts[cb + k] = (uint16_t)cnt; }
        __syncthreads();
      }
      // every node is some container's child, or the root
      if (tid == 0 && bc != s_tot[0]) s_bad = BAD_SYNTAX;
    }
    __syncthreads();
    if (tid == 0) {
      if (s_bad) coop_refuse(A, d, s_bad);
      else { A.n_nodes[d] = s_tot[0]; A.n_cont[d] = s_tot[1]; A.n_str[d] = s_tot[2]; }
    }
  }
}

// one lane per value token: its node, whole, as the lane emit pass writes it
__global__ void __launch_bounds__(256) json_coop_emit_kernel(JArgs A) {
  for (uint32_t ci = blockIdx.x; ci < A.ncoop; ci += gridDim.x) {
    const uint32_t d = A.coop_list[ci];
    if (*A.bad) return;
    if (A.doc_bad[d]) continue;
    const uint32_t nt = A.n_tok[d];
    const Tok* tk = A.toks + A.tok_base[d];
    const TokAux* ax = A.aux + A.tok_base[d];
    const uint64_t nb = A.node_base[d];
    Text T(A.text, A.off[d], A.off[d + 1] - A.off[d]);
    auto bad = [&](uint32_t why) { if (!A.doc_bad[d]) A.doc_bad[d] = why; };
    for (uint32_t t = threadIdx.x; t < nt; t += blockDim.x) {
      const Tok o = tk[t];
      const uint32_t kind = o.meta & 0xFFu;
      if (kind >= TK_CMAP && kind <= TK_COMMA) continue;
      const TokAux a = ax[t];
      uint32_t rel = 0, parent = NONE, cont = 0;
      NodeRec r;
      r.n.key_off = NONE; r.n.key_len = 0; r.n.key_hash = 0;
      r.line = o.line; r.col = o.col; r.kline = 0; r.kcol = 0; r.kpos = 0; r.vpos = 0; r.pad0 = 0; r.pad1 = 0;
      if (t == 0) {
        if (kind == TK_OLIST) { r.line = 0; r.col = 0; }   // emit_root: lists keep (0,0)
      } else {
        const TokAux pa = ax[a.ptok];
        const bool pmap = (tk[a.ptok].meta & 0xFFu) == TK_OMAP;
        if (pmap && (tk[t - 1].meta & 0xFFu) != TK_COLON) continue;   // a key: its value's lane takes it
        rel = pa.base + a.ord;
        parent = a.ptok ? ax[pa.ptok].base + pa.ord : 0u;
        if (pmap) {
          const Tok ko = tk[t - 2];   // key, colon, value (tree kernel)
          uint32_t slot = 0, len = 0;
          const uint64_t e = string_occurrence<true>(A, T, ko.off, d, cont, &slot, &len);
          if (!e || e > tk[t - 1].off) { bad(BAD_SYNTAX); continue; }
          // duplicate keys are found by the fix / verify pass; maps past its scan bound are refused
          if (a.ord >= kMaxPairwiseKeys) { bad(BAD_WIDEMAP); continue; }
          r.n.key_off = slot; r.n.key_len = len; r.n.key_hash = slot;
          r.kpos = ko.off; r.kline = ko.line; r.kcol = ko.col;
        }
      }
      r.n.parent = parent;
      if (kind == TK_STR) {
        uint32_t slot = 0, len = 0;
        const uint64_t e = string_occurrence<true>(A, T, o.off, d, cont, &slot, &len);
        if (!e || e > tk[t + 1].off) { bad(BAD_SYNTAX); continue; }   // (a string is never the last token)
        r.n.kind = K_STRING; r.n.count = len; r.n.a = slot; r.n.b = slot;
        r.vpos = o.off;
      } else if (kind <= TK_OLIST) {
        r.n.kind = kind == TK_OMAP ? K_MAP : K_LIST; r.n.count = a.cnt; r.n.a = a.base; r.n.b = 0;
      } else {
        const uint64_t L = plain_len(T, o.off);
        if (!L || !after_plain_ok(T.at(o.off + L))) { bad(BAD_SYNTAX); continue; }
        r.n.kind = K_NULL; r.n.count = 0; r.n.a = 0; r.n.b = 0;
        if (!scalar(T, o.off, L, r.n)) { bad(BAD_NUMBER); continue; }
      }
      A.recs[nb + rel] = r;
    }
  }
}
