// One YAML scalar as serde_yaml 0.9 over libyaml 0.2.5 writes it (width unlimited, unicode on), as a
// streaming state machine shared by the device YAML report writer (report_gpu.hip) and a host
// diagnostic (gg_yaml_scalar).  A scalar's style has to be known before its first byte is written and
// depends on the whole string, so a string runs through the machine twice: scan() every byte, decide(),
// then emit() every byte in the chosen style.
//
// serde_yaml asks for literal when the string holds '\n', for single quotes when the plain form would
// resolve to null / bool / int / float (reporter.cpp yaml_resolves_to_non_string), else for "any"; the
// emitter (emitter.c yaml_emitter_analyze_scalar / select_scalar_style) then refuses plain, single
// quotes or literal by what the string holds.  The state is the emitter's flag bits plus a one-character
// hold: "followed by whitespace" is a one-character look-ahead, and a UTF-8 sequence may span the pieces
// a message is composed from.  HOST: cases left to libyaml itself (keep chomping, which ends the stream
// with "...", complex keys, U+2028 / U+2029 outside double quotes, a float whose finiteness the digit
// counts do not settle, invalid UTF-8).
#pragma once
#include <stdint.h>

#ifndef GG_HD
#define GG_HD
#endif

namespace gg {
namespace ys {

enum Style : uint32_t { PLAIN = 0, SINGLE = 1, DOUBLE = 2, LITERAL = 3, HOST = 4 };

enum : uint32_t {
  F_BLOCK = 1u << 0,      // block indicators: plain refused
  F_SPECIAL = 1u << 1,    // a character libyaml does not call printable
  F_NL = 1u << 2,         // '\n' (serde_yaml: literal)
  F_BRK = 1u << 3,        // any break: \r \n U+0085 U+2028 U+2029
  F_UBRK = 1u << 4,       // U+2028 / U+2029 (printable breaks: written raw with the emitter's indent)
  F_LEAD = 1u << 5,       // leading space or break
  F_BRK_SP = 1u << 6,     // a space after a break
  F_SP_BRK = 1u << 7,     // a space before a break
  F_PP_NL = 1u << 8,      // the character before the previous one was '\n'
  F_BAD = 1u << 9,        // invalid UTF-8
  F_LEAD_HINT = 1u << 10  // the first character is a space or a break (literal header digit)
};

// the number spellings of yaml_resolves_to_non_string as a DFA over ASCII bytes
enum : uint32_t {
  N_START = 0, N_SIGN, N_ZERO, N_INT, N_X0, N_X, N_O0, N_O, N_B0, N_B, N_DOT0, N_FRAC, N_E, N_ES, N_ED, N_FAIL
};

struct Sc {
  uint32_t f;        // F_*
  uint32_t n;        // characters seen: 0, 1, 2, 3 = more
  uint32_t bytes;    // bytes seen
  uint32_t prev;     // the previous character (the hold)
  uint32_t first;    // the first character
  uint32_t cp, need, lo; // UTF-8 sequence in flight (either phase); lo: its smallest non-overlong value
  uint32_t num;      // N_* state
  uint32_t nint, eabs;  // integer digits / exponent magnitude (saturating): settle finiteness
  uint64_t head;     // the first 8 bytes (null / bool / .inf / .nan spellings)
  // emit phase
  uint32_t style, indent;
  bool bol, eneg;
};

GG_HD inline bool is_break(uint32_t c) { return c == '\n' || c == '\r' || c == 0x85u || c == 0x2028u || c == 0x2029u; }
GG_HD inline bool is_blankz(uint32_t c) { return c == ' ' || c == '\t' || c == 0 || is_break(c); }
GG_HD inline bool is_printable(uint32_t c) {
  return c == 0x0A || (c >= 0x20 && c <= 0x7E) || (c >= 0xA0 && c <= 0xD7FF) || (c >= 0xE000 && c <= 0xFFFD && c != 0xFEFF);
}
GG_HD inline bool is_indicator(uint32_t c) {
  switch (c) {
    case '#': case ',': case '[': case ']': case '{': case '}': case '&': case '*': case '!': case '|':
    case '>': case '\'': case '"': case '%': case '@': case '`': return true;
    default: return false;
  }
}

GG_HD inline void begin(Sc& s) {
  s.f = 0; s.n = 0; s.bytes = 0; s.prev = 0; s.first = 0; s.cp = 0; s.need = 0; s.lo = 0;
  s.num = N_START; s.nint = 0; s.eabs = 0; s.head = 0; s.eneg = false;
}

GG_HD inline uint32_t num_step(uint32_t st, uint32_t c, Sc& s) {
  const bool dig = c >= '0' && c <= '9';
  switch (st) {
    case N_START:
      if (c == '+' || c == '-') return N_SIGN;
      [[fallthrough]];
    case N_SIGN:
      if (c == '0') { s.nint = 1; return N_ZERO; }
      if (dig) { s.nint = 1; return N_INT; }
      return c == '.' ? N_DOT0 : N_FAIL;
    case N_ZERO:
      if (c == 'x') return N_X0;
      if (c == 'o') return N_O0;
      if (c == 'b') return N_B0;
      [[fallthrough]];
    case N_INT:
      if (dig) { if (s.nint < 4096) s.nint++; return N_INT; }
      if (c == '.') return N_FRAC;
      return (c == 'e' || c == 'E') ? N_E : N_FAIL;
    case N_X0: case N_X:
      return (dig || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F')) ? N_X : N_FAIL;
    case N_O0: case N_O: return (c >= '0' && c <= '7') ? N_O : N_FAIL;
    case N_B0: case N_B: return (c == '0' || c == '1') ? N_B : N_FAIL;
    case N_DOT0: return dig ? N_FRAC : N_FAIL;
    case N_FRAC:
      if (dig) return N_FRAC;
      return (c == 'e' || c == 'E') ? N_E : N_FAIL;
    case N_E:
      if (c == '+' || c == '-') { s.eneg = c == '-'; return N_ES; }
      [[fallthrough]];
    case N_ES: case N_ED:
      if (!dig) return N_FAIL;
      if (s.eabs < 100000) s.eabs = s.eabs * 10 + (c - '0');
      return N_ED;
    default: return N_FAIL;
  }
}

// one whole character
GG_HD inline void scan_cp(Sc& s, uint32_t c) {
  const bool brk = is_break(c);
  if (s.n == 0) {
    s.first = c;
    if (is_indicator(c)) s.f |= F_BLOCK;
    if (c == ' ' || brk) s.f |= F_LEAD | F_LEAD_HINT;
  } else {
    const uint32_t p = s.prev;
    const bool blank = brk || c == ' ' || c == '\t' || c == 0;
    if (blank && (p == ':' || (s.n == 1 && (p == '-' || p == '?')))) s.f |= F_BLOCK;
    if (c == '#' && is_blankz(p)) s.f |= F_BLOCK;
    if (s.n == 2 && c == p && c == s.first && (c == '-' || c == '.')) s.f |= F_BLOCK;   // "---" / "..."
    if (c == ' ' && is_break(p)) s.f |= F_BRK_SP;
    if (brk && p == ' ') s.f |= F_SP_BRK;
    s.f = p == '\n' ? (s.f | F_PP_NL) : (s.f & ~F_PP_NL);
  }
  if (!is_printable(c)) s.f |= F_SPECIAL;
  if (brk) s.f |= c == '\n' ? (F_NL | F_BRK) : (c >= 0x2028u ? (F_UBRK | F_BRK) : F_BRK);
  s.num = (c < 0x80 && s.num != N_FAIL) ? num_step(s.num, c, s) : N_FAIL;
  s.prev = c;
  if (s.n < 3) s.n++;
}

// assembles UTF-8 into s.cp; true when a character is complete (overlong forms, surrogates and values
// past U+10FFFF set F_BAD)
GG_HD inline bool utf8_byte(Sc& s, unsigned char b) {
  if (s.need) {
    if ((b & 0xC0) != 0x80) { s.f |= F_BAD; s.need = 0; return false; }
    s.cp = (s.cp << 6) | (b & 0x3Fu);
    if (--s.need) return false;
    if (s.cp < s.lo || (s.cp >= 0xD800 && s.cp <= 0xDFFF) || s.cp > 0x10FFFF) s.f |= F_BAD;
    return true;
  }
  if (b < 0x80) { s.cp = b; return true; }
  if (b >= 0xC2 && b <= 0xDF) { s.cp = b & 0x1Fu; s.need = 1; s.lo = 0x80; }
  else if (b >= 0xE0 && b <= 0xEF) { s.cp = b & 0x0Fu; s.need = 2; s.lo = 0x800; }
  else if (b >= 0xF0 && b <= 0xF4) { s.cp = b & 0x07u; s.need = 3; s.lo = 0x10000; }
  else s.f |= F_BAD;
  return false;
}

GG_HD inline void scan_slow(Sc& s, unsigned char b) {
  if (s.bytes < 8) s.head |= (uint64_t)b << (8 * s.bytes);
  s.bytes++;
  if (utf8_byte(s, b)) scan_cp(s, s.cp);
}
// the common byte, small enough to inline wherever text is produced: past the first two characters, with
// the number spellings ruled out, a printable ASCII byte other than ':' and '#', or a space after one,
// changes only the hold.  false: scan_slow takes the byte.
GG_HD inline bool scan_fast(Sc& s, unsigned char b) {
  if (s.n < 3 || s.num != N_FAIL || s.need) return false;
  const uint32_t p = s.prev;
  const bool inert = b > 0x20 && b < 0x7F && b != ':' && b != '#';
  if (!inert && !(b == ' ' && p > 0x20 && p < 0x7F && p != ':')) return false;
  if (s.bytes < 8) s.head |= (uint64_t)b << (8 * s.bytes);
  s.bytes++;
  s.f = p == '\n' ? (s.f | F_PP_NL) : (s.f & ~F_PP_NL);
  s.prev = b;
  return true;
}
GG_HD inline void scan(Sc& s, unsigned char b) { if (!scan_fast(s, b)) scan_slow(s, b); }

// 16 bytes that change nothing but the hold: printable ASCII, no space, ':' or '#', once the first two
// characters are past and the number spellings are ruled out
GG_HD inline bool inert8(uint64_t x) {
  const uint64_t ones = 0x0101010101010101ull, highs = 0x8080808080808080ull;
  const uint64_t lt = (x - ones * 0x21u) & ~x & highs;           // a byte < 0x21
  const uint64_t hi = ((x | highs) - ones * 0x7Fu) & highs;      // a byte >= 0x7F (bit 7 clear: tested by x & highs)
  const uint64_t c = x ^ (ones * (uint64_t)':'), h = x ^ (ones * (uint64_t)'#');
  return !(lt | hi | (x & highs) | ((c - ones) & ~c & highs) | ((h - ones) & ~h & highs));
}
GG_HD inline bool scan16(Sc& s, uint64_t lo, uint64_t hi) {
  if (s.n < 3 || s.num != N_FAIL || s.need || !inert8(lo) || !inert8(hi)) return false;
  s.bytes += 16;
  s.prev = (uint32_t)(hi >> 56);
  s.f &= ~F_PP_NL;
  return true;
}

GG_HD inline bool head_is(const Sc& s, const char* w, uint32_t off) {
  uint32_t i = 0;
  for (; w[i]; i++) if ((char)(s.head >> (8 * (i + off))) != w[i]) return false;
  return s.bytes == i + off;
}
// yaml_resolves_to_non_string: 1 yes, 0 no, 2 = a float spelling whose finiteness is not settled here
GG_HD inline uint32_t resolves(const Sc& s) {
  if (s.bytes == 0) return 1;
  if (s.bytes <= 5) {
    if (head_is(s, "~", 0) || head_is(s, "null", 0) || head_is(s, "Null", 0) || head_is(s, "NULL", 0) ||
        head_is(s, "true", 0) || head_is(s, "True", 0) || head_is(s, "TRUE", 0) || head_is(s, "false", 0) ||
        head_is(s, "False", 0) || head_is(s, "FALSE", 0) || head_is(s, ".nan", 0) || head_is(s, ".NaN", 0) ||
        head_is(s, ".NAN", 0))
      return 1;
    const uint32_t o = (s.first == '+' || s.first == '-') ? 1 : 0;
    if (head_is(s, ".inf", o) || head_is(s, ".Inf", o) || head_is(s, ".INF", o)) return 1;
  }
  switch (s.num) {
    case N_X: case N_O: case N_B: return 1;
    case N_ZERO: case N_INT: case N_FRAC: case N_ED:
      // below 10^308 every decimal is finite; past it strtod decides (the host)
      return s.nint + (s.eneg ? 0 : s.eabs) <= 308 ? 1 : 2;
    default: return 0;
  }
}

// the style libyaml writes after the scan; sets up the emit phase.  indent: the column of the
// enclosing collection's entries (a literal's lines go two further in)
GG_HD inline uint32_t decide(Sc& s, bool is_key, uint32_t indent) {
  uint32_t f = s.f;
  if (s.need || (f & F_BAD)) return s.style = HOST;
  const uint32_t p = s.prev;
  const bool trail_sp = s.n && p == ' ', trail_brk = s.n && is_break(p);
  if (s.n && (p == ':' || (s.n == 1 && (p == '-' || p == '?')))) f |= F_BLOCK;
  if (is_key && (s.bytes > 128 || (f & F_BRK))) return s.style = HOST;   // "? key": not a simple key
  const bool special = f & F_SPECIAL;
  const bool plain_ok = !(f & (F_BLOCK | F_LEAD | F_BRK | F_BRK_SP | F_SP_BRK)) && !special && !trail_sp && !trail_brk;
  const bool single_ok = !(f & (F_BRK_SP | F_SP_BRK)) && !special;
  const bool block_ok = !(f & F_SP_BRK) && !special && !trail_sp;
  uint32_t st;
  if (f & F_NL) st = block_ok ? LITERAL : DOUBLE;
  else {
    const uint32_t r = resolves(s);
    if (r == 2) return s.style = HOST;
    st = (r == 0 && plain_ok) ? PLAIN : single_ok ? SINGLE : DOUBLE;
  }
  if (st != DOUBLE && (f & F_UBRK)) st = HOST;
  if (st == LITERAL && p == '\n' && (s.n == 1 || (f & F_PP_NL))) st = HOST;   // "|+": the stream ends in "..."
  s.style = st; s.indent = indent + 2; s.bol = true; s.cp = 0; s.need = 0;
  return st;
}

template <class Out>
GG_HD inline void emit_open(Sc& s, Out& o) {
  switch (s.style) {
    case SINGLE: o.put('\''); break;
    case DOUBLE: o.put('"'); break;
    case LITERAL:
      o.put('|');
      if (s.f & F_LEAD_HINT) o.put('2');
      if (s.prev != '\n') o.put('-');
      break;
    default: break;
  }
}
template <class Out>
GG_HD inline void emit_close(Sc& s, Out& o) {
  if (s.style == SINGLE) o.put('\'');
  else if (s.style == DOUBLE) o.put('"');
}
template <class Out>
GG_HD inline void hex(Out& o, uint32_t v, int digits) {
  for (int i = digits - 1; i >= 0; i--) o.put("0123456789ABCDEF"[(v >> (4 * i)) & 15u]);
}
// one character inside double quotes (emitter.c yaml_emitter_write_double_quoted_scalar)
template <class Out>
GG_HD inline void emit_dq(Out& o, uint32_t c) {
  if (is_printable(c) && !is_break(c) && c != '"' && c != '\\') {
    if (c < 0x80) o.put((char)c);
    else if (c < 0x800) { o.put((char)(0xC0 | (c >> 6))); o.put((char)(0x80 | (c & 0x3F))); }
    else { o.put((char)(0xE0 | (c >> 12))); o.put((char)(0x80 | ((c >> 6) & 0x3F))); o.put((char)(0x80 | (c & 0x3F))); }
    return;
  }
  o.put('\\');
  switch (c) {
    case 0x00: o.put('0'); return;
    case 0x07: o.put('a'); return;
    case 0x08: o.put('b'); return;
    case 0x09: o.put('t'); return;
    case 0x0A: o.put('n'); return;
    case 0x0B: o.put('v'); return;
    case 0x0C: o.put('f'); return;
    case 0x0D: o.put('r'); return;
    case 0x1B: o.put('e'); return;
    case 0x22: o.put('"'); return;
    case 0x5C: o.put('\\'); return;
    case 0x85: o.put('N'); return;
    case 0xA0: o.put('_'); return;
    case 0x2028: o.put('L'); return;
    case 0x2029: o.put('P'); return;
    default:
      if (c <= 0xFF) { o.put('x'); hex(o, c, 2); }
      else if (c <= 0xFFFF) { o.put('u'); hex(o, c, 4); }
      else { o.put('U'); hex(o, c, 8); }
  }
}
// every byte but a double-quoted escape or UTF-8 sequence (false: emit_slow takes the byte)
template <class Out>
GG_HD inline bool emit_fast(Sc& s, Out& o, unsigned char b) {
  switch (s.style) {
    case SINGLE:
      if (b == '\'') o.put('\'');
      o.put((char)b);
      return true;
    case DOUBLE:
      if (s.need || b < 0x20 || b > 0x7E || b == '"' || b == '\\') return false;
      o.put((char)b);
      return true;
    case LITERAL:
      // every line is preceded by its break: a bare one for an empty line, break + indent otherwise;
      // the text's last break is left to whatever follows the scalar
      if (b == '\n') {
        if (s.bol) o.put('\n');
        s.bol = true;
        return true;
      }
      if (s.bol) { o.put('\n'); for (uint32_t i = 0; i < s.indent; i++) o.put(' '); s.bol = false; }
      o.put((char)b);
      return true;
    default:
      o.put((char)b);
      return true;
  }
}
template <class Out>
GG_HD inline void emit_slow(Sc& s, Out& o, unsigned char b) { if (utf8_byte(s, b)) emit_dq(o, s.cp); }
template <class Out>
GG_HD inline void emit(Sc& s, Out& o, unsigned char b) { if (!emit_fast(s, o, b)) emit_slow(s, o, b); }

// the whole scalar at once: scan, decide, emit; the style, HOST with nothing written
template <class Out>
GG_HD inline uint32_t render(Out& o, const char* s, uint32_t n, bool is_key, uint32_t indent) {
  Sc sc;
  begin(sc);
  for (uint32_t i = 0; i < n; i++) scan(sc, (unsigned char)s[i]);
  if (decide(sc, is_key, indent) == HOST) return HOST;
  emit_open(sc, o);
  for (uint32_t i = 0; i < n; i++) emit(sc, o, (unsigned char)s[i]);
  emit_close(sc, o);
  return sc.style;
}

}  // namespace ys
}  // namespace gg
