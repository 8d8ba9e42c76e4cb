// Shortest round-trip binary64 -> decimal (Schubfach: R. Giulietti, "The Schubfach way to render doubles"),
// shared by the device report writers and a host diagnostic.  The digits are the ones ryu::Buffer::
// format_finite and Rust's `impl Display for f64` print: the shortest decimal inside the double's rounding
// interval, the closest to the true value among the shortest, ties to even.  Exact integer arithmetic: three
// 64 x 128-bit products by one entry of pow10_table.h (its rounding is the one the proof asks for, see
// tools/gen_pow10_table.py), high halves by a multiply-high; no floating point, no 128-bit division, and no
// loop over the digits -- trailing zeros leave in 10^8, 10^4, 10^2 and 10 steps, characters come from two
// 8-digit SWAR conversions held in registers.
//
// Two layouts over the digits (host_format.h pins the same forms): ryu_layout (serde_json / serde_yaml
// numbers) and display_layout (Rust Display: never an exponent).  Both write through a put(char) callable.
#pragma once
#include <stdint.h>

#include "pow10_table.h"

#ifndef GG_HD
#define GG_HD
#endif

namespace gg {
namespace sf {

struct Dec64 {
  uint64_t digits;   // <= 17 decimal digits, no trailing zero; 0 for +-0.0
  int32_t exp;       // |x| = digits * 10^exp
  uint32_t neg;
};

// the high half of a 64 x 64-bit product (on the device the compiler lowers it as it lowers __umul64hi: four
// 32-bit multiply-high / multiply-add pairs; written this way the host sees the same line)
GG_HD inline uint64_t mulhi64(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

// floor(g * cp / 2^128), its lowest bit made sticky (round to odd); cp < 2^60, so nothing overflows.  g is at
// most one unit above 10^k 2^-r, which moves the 128-bit product by less than cp / 2^64 < 1 unit of its low
// word: a low word of 0 or 1 is an exact product
GG_HD inline uint64_t round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
  const uint64_t xhi = mulhi64(cp, glo);
  const uint64_t ylo = cp * ghi + xhi;
  const uint64_t yhi = mulhi64(cp, ghi) + (ylo < xhi ? 1u : 0u);
  return yhi | (ylo > 1 ? 1u : 0u);
}

// the shortest digits of the finite double with these IEEE bits; tab = kPow10_128
template <typename Tab>
GG_HD inline Dec64 shortest_f64(uint64_t bits, const Tab& tab) {
  Dec64 r;
  r.neg = (uint32_t)(bits >> 63);
  const uint64_t frac = bits & 0x000FFFFFFFFFFFFFull;
  const uint32_t bexp = (uint32_t)(bits >> 52) & 0x7FFu;
  uint64_t d;
  int32_t e;
  if (bexp == 0 && frac == 0) { r.digits = 0; r.exp = 0; return r; }
  const uint64_t c = bexp ? (frac | (1ull << 52)) : frac;
  const int32_t q = bexp ? (int32_t)bexp - 1075 : -1074;
  if (q <= 0 && q > -53 && (c & ((1ull << -q) - 1)) == 0) {
    d = c >> -q; e = 0;   // an integer below 2^53: its own digits are the shortest
  } else {
    // the rounding interval [cbl, cbr] around cb = 4c in units of 2^(q-2); the lower half is half as wide
    // just above a power of two
    const bool even = (c & 1) == 0;
    const bool closer = frac == 0 && bexp > 1;
    const uint64_t cbl = 4 * c - 2 + (closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    const int32_t k = (q * 1262611 - (closer ? 524031 : 0)) >> 22;   // floor(log10 2^q), or of 3/4 2^q
    const int32_t h = q + ((-k * 1741647) >> 19) + 1;                // in [1, 4]
    const Pow10_128 g = tab[-k - kPow10Min];                          // one 16-byte load, index per lane
    const uint64_t vbl = round_to_odd(g.hi, g.lo, cbl << h);
    const uint64_t vb = round_to_odd(g.hi, g.lo, cb << h);
    const uint64_t vbr = round_to_odd(g.hi, g.lo, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb >> 2;
    bool done = false;
    if (s >= 10) {   // one digit fewer: the multiple of 10^(k+1) below or above, when exactly one is inside
      const uint64_t sp = s / 10;
      const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
      if (up_in != wp_in) { d = sp + (wp_in ? 1 : 0); e = k + 1; done = true; }
    }
    if (!done) {
      const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
      if (u_in != w_in) d = s + (w_in ? 1 : 0);
      else {           // both inside: the closer one, ties to even
        const uint64_t mid = 4 * s + 2;
        d = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
      }
      e = k;
    }
  }
  // at most 15 trailing zeros (a 17-digit result has none: the shorter candidate would have been inside)
  if (d % 100000000u == 0) { d /= 100000000u; e += 8; }
  if (d % 10000u == 0) { d /= 10000u; e += 4; }
  if (d % 100u == 0) { d /= 100u; e += 2; }
  if (d % 10u == 0) { d /= 10u; e += 1; }
  r.digits = d; r.exp = e;
  return r;
}

// x < 10^8 as eight ASCII digits, the most significant in the lowest byte
GG_HD inline uint64_t ascii8(uint32_t x) {
  const uint64_t m4 = (uint64_t)(x / 10000u) | ((uint64_t)(x % 10000u) << 32);       // 2 x 4 digits
  const uint64_t t2 = ((m4 * 10486u) >> 20) & 0x0000007F0000007Full;                 // / 100 per 32-bit lane
  const uint64_t m2 = t2 | ((m4 - 100u * t2) << 16);                                 // 4 x 2 digits
  const uint64_t t1 = ((m2 * 103u) >> 10) & 0x000F000F000F000Full;                   // / 10 per 16-bit lane
  return (t1 | ((m2 - 10u * t1) << 8)) + 0x3030303030303030ull;
}

// the digits of a Dec64 as characters, in registers: digit j of n, counted from the most significant
struct Digits {
  uint64_t a, b;   // digits 1..8 and 9..16 of the 17-digit zero-padded form
  uint32_t top;    // its digit 0
  uint32_t n;      // significant digits
  GG_HD char at(uint32_t j) const {
    const uint32_t i = 17u - n + j;
    if (i == 0) return (char)('0' + top);
    return (char)(((i <= 8 ? a >> (8 * (i - 1)) : b >> (8 * (i - 9)))) & 0xFF);
  }
};
GG_HD inline Digits digits_of(uint64_t d) {
  Digits g;
  g.top = (uint32_t)(d / 10000000000000000ull);
  const uint64_t rest = d % 10000000000000000ull;
  const uint32_t hi = (uint32_t)(rest / 100000000u), lo = (uint32_t)(rest % 100000000u);
  g.a = ascii8(hi); g.b = ascii8(lo);
  // leading zeros of the padded form: whole zero parts, then zero bytes ('0' ^ '0') from the low end
  uint32_t z;
  if (g.top) z = 0;
  else if (hi) z = 1u + (uint32_t)__builtin_ctzll(g.a ^ 0x3030303030303030ull) / 8u;
  else z = 9u + (lo ? (uint32_t)__builtin_ctzll(g.b ^ 0x3030303030303030ull) / 8u : 7u);
  g.n = 17u - z;
  return g;
}

// One layout routine for both styles, with a single put site (the device writers inline their whole
// character path into it).  The text is [-] body [suffix]: body = z1 zeros, the n digits, z2 zeros, with a '.'
// after its first `dot` characters; suffix = the exponent, packed eight characters to a register.
//   ryu::Buffer::format_finite (ryu pretty.rs): 1234.0, 12.34, 0.001234 (kk > -5), else 1.234e21, 1e-7; -0.0
//   Rust `impl Display for f64`: the digits at their place, zero-padded in either direction, no exponent
//   (up to 309 integer digits or 324 fraction digits, written as they come); -0
template <class Put> GG_HD inline void layout(const Dec64& x, bool display, Put&& put) {
  const Digits g = digits_of(x.digits);   // +-0.0: the one digit 0
  const int32_t n = (int32_t)g.n, kk = n + x.exp;   // the decimal point belongs after digit kk
  const uint32_t none = 0xFFFFFFFFu;
  uint32_t z1 = 0, z2 = 0, dot = none, sl = 0;
  uint64_t suf = 0;
  if (kk <= 0 && (display || kk > -5)) { z1 = (uint32_t)(1 - kk); dot = 1; }             // 0.00ddd
  else if (x.exp < 0 && kk > 0 && (display || kk <= 16)) dot = (uint32_t)kk;             // dd.ddd
  else if (display) z2 = (uint32_t)x.exp;                                                // dd000
  else if (x.exp >= 0 && kk <= 16) { z2 = (uint32_t)x.exp + 1; dot = (uint32_t)kk; }     // dd00.0
  else {                                                                                 // d.ddde-x
    if (n > 1) dot = 1;
    const int32_t ex = kk - 1;
    const uint32_t a = (uint32_t)(ex < 0 ? -ex : ex);
    suf = 'e'; sl = 1;
    if (ex < 0) { suf |= (uint64_t)'-' << 8; sl = 2; }
    if (a >= 100) { suf |= (uint64_t)('0' + a / 100) << (8 * sl); sl++; }
    if (a >= 10) { suf |= (uint64_t)('0' + a / 10 % 10) << (8 * sl); sl++; }
    suf |= (uint64_t)('0' + a % 10) << (8 * sl); sl++;
  }
  const uint32_t len = z1 + (uint32_t)n + z2 + (dot != none ? 1u : 0u), total = x.neg + len + sl;
#pragma unroll 1
  for (uint32_t i = 0; i < total; i++) {
    char c = '-';
    if (i >= x.neg) {
      const uint32_t p = i - x.neg;
      if (p >= len) c = (char)((suf >> (8 * (p - len))) & 0xFF);
      else if (p == dot) c = '.';
      else {
        const uint32_t j = p - (p > dot ? 1u : 0u);
        c = (j < z1 || j >= z1 + (uint32_t)n) ? '0' : g.at(j - z1);
      }
    }
    put(c);
  }
}
template <class Put> GG_HD inline void ryu_layout(const Dec64& x, Put&& put) { layout(x, false, put); }
template <class Put> GG_HD inline void display_layout(const Dec64& x, Put&& put) { layout(x, true, put); }

}  // namespace sf
}  // namespace gg
