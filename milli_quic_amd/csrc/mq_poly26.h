// mq_poly26.h — Poly1305 arithmetic mod 2^130 - 5 in radix 2^26 (5 limbs), general multiplier
// (r, r^2 .. r^8), as plain integer code that compiles for the device and for the host (tests/csrc/
// test_poly_pair.cpp checks it without a GPU). Included by mq_device.h.
#pragma once
#include <stdint.h>

#include "mq_poly_sched.h"  // MQ_HD

// full unrolling where hipcc compiles this; a host compiler takes the plain loop
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MQ_UNROLL _Pragma("unroll")
#else
#define MQ_UNROLL
#endif

namespace mq {

struct P26 { uint32_t l[5]; };
struct P26m { uint32_t r[5], s[4]; };  // multiplier with s[i] = 5 * r[i+1]

MQ_HD P26m p26_mult(const P26& r) {
  P26m m;
MQ_UNROLL
  for (int i = 0; i < 5; ++i) m.r[i] = r.l[i];
MQ_UNROLL
  for (int i = 0; i < 4; ++i) m.s[i] = r.l[i + 1] * 5u;
  return m;
}

MQ_HD P26 p26_from_words(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t hibit) {
  P26 h;
  h.l[0] = t0 & 0x3ffffff;
  h.l[1] = ((t0 >> 26) | (t1 << 6)) & 0x3ffffff;
  h.l[2] = ((t1 >> 20) | (t2 << 12)) & 0x3ffffff;
  h.l[3] = ((t2 >> 14) | (t3 << 18)) & 0x3ffffff;
  h.l[4] = (t3 >> 8) | (hibit << 24);
  return h;
}

// h = h * m (mod 2^130 - 5), partially reduced (limbs < 2^26, l[1] < 2^26 + 2^9). Inputs: limbs
// < 2^27 (a product plus one absorbed block), multiplier limbs < 2^26 (s < 2^28.4), so every
// column sum stays below 2^58 and each carry (d >> 26) below 2^32, so the top carry is a 32-bit
// operand of the x5 fold.
MQ_HD void p26_mul(P26& h, const P26m& m) {
  const uint32_t h0 = h.l[0], h1 = h.l[1], h2 = h.l[2], h3 = h.l[3], h4 = h.l[4];
  const uint64_t d0 = (uint64_t)h0 * m.r[0] + (uint64_t)h1 * m.s[3] + (uint64_t)h2 * m.s[2] + (uint64_t)h3 * m.s[1] + (uint64_t)h4 * m.s[0];
  const uint64_t d1 = (d0 >> 26) + (uint64_t)h0 * m.r[1] + (uint64_t)h1 * m.r[0] + (uint64_t)h2 * m.s[3] + (uint64_t)h3 * m.s[2] + (uint64_t)h4 * m.s[1];
  const uint64_t d2 = (d1 >> 26) + (uint64_t)h0 * m.r[2] + (uint64_t)h1 * m.r[1] + (uint64_t)h2 * m.r[0] + (uint64_t)h3 * m.s[3] + (uint64_t)h4 * m.s[2];
  const uint64_t d3 = (d2 >> 26) + (uint64_t)h0 * m.r[3] + (uint64_t)h1 * m.r[2] + (uint64_t)h2 * m.r[1] + (uint64_t)h3 * m.r[0] + (uint64_t)h4 * m.s[3];
  const uint64_t d4 = (d3 >> 26) + (uint64_t)h0 * m.r[4] + (uint64_t)h1 * m.r[3] + (uint64_t)h2 * m.r[2] + (uint64_t)h3 * m.r[1] + (uint64_t)h4 * m.r[0];
  const uint32_t c4 = (uint32_t)(d4 >> 26);
  const uint64_t t = (uint64_t)((uint32_t)d0 & 0x3ffffff) + (uint64_t)c4 * 5u;
  h.l[0] = (uint32_t)t & 0x3ffffff;
  h.l[1] = ((uint32_t)d1 & 0x3ffffff) + (uint32_t)(t >> 26);
  h.l[2] = (uint32_t)d2 & 0x3ffffff;
  h.l[3] = (uint32_t)d3 & 0x3ffffff;
  h.l[4] = (uint32_t)d4 & 0x3ffffff;
}

// h = h * m2 + y * m1 (mod 2^130 - 5): two products into the same five column sums and one carry
// chain, partially reduced exactly as p26_mul leaves it (limbs < 2^26, l[1] < 2^26 + 2^9). Two Horner
// steps ((h + x) m + y) m are p26_mul2(h + x, m^2, y, m).
// Bound: h limbs < 2^27 + 2^9 (a p26_mul output plus one absorbed block), y limbs < 2^26 (a raw
// block), both multipliers p26_mul outputs: limbs < 2^26 + 2^9, s < 5 (2^26 + 2^9). A column with
// s terms is then below (2^27 + 2^9 + 2^26)(2^26 + 2^9)(1 + 4 * 5) ~ 31.5 * 2^53 < 2^58, the carry
// into the next one below 2^32: p26_mul's invariant. Column 4 holds no s term (< 7.6 * 2^53), so
// c4 < 2^31 stays a 32-bit operand of the x5 fold and l[1] gains less than 2^9. The bound does not
// hold for a third product in the same sums.
MQ_HD void p26_mul2(P26& h, const P26m& m2, const P26& y, const P26m& m1) {
  const uint32_t h0 = h.l[0], h1 = h.l[1], h2 = h.l[2], h3 = h.l[3], h4 = h.l[4];
  const uint32_t y0 = y.l[0], y1 = y.l[1], y2 = y.l[2], y3 = y.l[3], y4 = y.l[4];
  const uint64_t d0 = (uint64_t)y0 * m1.r[0] + (uint64_t)y1 * m1.s[3] + (uint64_t)y2 * m1.s[2] + (uint64_t)y3 * m1.s[1] + (uint64_t)y4 * m1.s[0] +
                      (uint64_t)h0 * m2.r[0] + (uint64_t)h1 * m2.s[3] + (uint64_t)h2 * m2.s[2] + (uint64_t)h3 * m2.s[1] + (uint64_t)h4 * m2.s[0];
  const uint64_t d1 = (d0 >> 26) + (uint64_t)y0 * m1.r[1] + (uint64_t)y1 * m1.r[0] + (uint64_t)y2 * m1.s[3] + (uint64_t)y3 * m1.s[2] + (uint64_t)y4 * m1.s[1] +
                      (uint64_t)h0 * m2.r[1] + (uint64_t)h1 * m2.r[0] + (uint64_t)h2 * m2.s[3] + (uint64_t)h3 * m2.s[2] + (uint64_t)h4 * m2.s[1];
  const uint64_t d2 = (d1 >> 26) + (uint64_t)y0 * m1.r[2] + (uint64_t)y1 * m1.r[1] + (uint64_t)y2 * m1.r[0] + (uint64_t)y3 * m1.s[3] + (uint64_t)y4 * m1.s[2] +
                      (uint64_t)h0 * m2.r[2] + (uint64_t)h1 * m2.r[1] + (uint64_t)h2 * m2.r[0] + (uint64_t)h3 * m2.s[3] + (uint64_t)h4 * m2.s[2];
  const uint64_t d3 = (d2 >> 26) + (uint64_t)y0 * m1.r[3] + (uint64_t)y1 * m1.r[2] + (uint64_t)y2 * m1.r[1] + (uint64_t)y3 * m1.r[0] + (uint64_t)y4 * m1.s[3] +
                      (uint64_t)h0 * m2.r[3] + (uint64_t)h1 * m2.r[2] + (uint64_t)h2 * m2.r[1] + (uint64_t)h3 * m2.r[0] + (uint64_t)h4 * m2.s[3];
  const uint64_t d4 = (d3 >> 26) + (uint64_t)y0 * m1.r[4] + (uint64_t)y1 * m1.r[3] + (uint64_t)y2 * m1.r[2] + (uint64_t)y3 * m1.r[1] + (uint64_t)y4 * m1.r[0] +
                      (uint64_t)h0 * m2.r[4] + (uint64_t)h1 * m2.r[3] + (uint64_t)h2 * m2.r[2] + (uint64_t)h3 * m2.r[1] + (uint64_t)h4 * m2.r[0];
  const uint32_t c4 = (uint32_t)(d4 >> 26);
  const uint64_t t = (uint64_t)((uint32_t)d0 & 0x3ffffff) + (uint64_t)c4 * 5u;
  h.l[0] = (uint32_t)t & 0x3ffffff;
  h.l[1] = ((uint32_t)d1 & 0x3ffffff) + (uint32_t)(t >> 26);
  h.l[2] = (uint32_t)d2 & 0x3ffffff;
  h.l[3] = (uint32_t)d3 & 0x3ffffff;
  h.l[4] = (uint32_t)d4 & 0x3ffffff;
}

// Full reduction mod p and tag = (h + s) mod 2^128, as 4 LE words.
MQ_HD void p26_finish(P26 h, const uint32_t (&s)[4], uint32_t (&tag)[4]) {
  uint32_t c;
  c = h.l[0] >> 26; h.l[0] &= 0x3ffffff; h.l[1] += c;
  c = h.l[1] >> 26; h.l[1] &= 0x3ffffff; h.l[2] += c;
  c = h.l[2] >> 26; h.l[2] &= 0x3ffffff; h.l[3] += c;
  c = h.l[3] >> 26; h.l[3] &= 0x3ffffff; h.l[4] += c;
  c = h.l[4] >> 26; h.l[4] &= 0x3ffffff; h.l[0] += c * 5;
  // h < 2 p now, limbs 1 .. 4 below 2^26 and limb 0 a few fives above it at most. g = h + 5 in
  // normalised limbs (g4 may reach 2^26) carries whatever the fold left; h itself is not carried on:
  // a lane sum c 2^130 + (2^128 - 5 c) has limbs 1 .. 3 all ones, its fold ripples up to limb 4, and
  // a chain on h that stops early packs a limb of 2^26 into the words. Both results come from g:
  // h >= p: (h - p) = g - 2^130, which is g mod 2^128; h < p: h = g - 5, taken off in the tag's sum
  // as + (2^128 - 5).
  uint32_t g0, g1, g2, g3, g4;
  g0 = h.l[0] + 5; c = g0 >> 26; g0 &= 0x3ffffff;
  g1 = h.l[1] + c; c = g1 >> 26; g1 &= 0x3ffffff;
  g2 = h.l[2] + c; c = g2 >> 26; g2 &= 0x3ffffff;
  g3 = h.l[3] + c; c = g3 >> 26; g3 &= 0x3ffffff;
  g4 = h.l[4] + c;
  bool use_g = (g4 >> 26) != 0;
  const uint32_t k = use_g ? 0u : 0xffffffffu;  // the words of 2^128 - 5: k - 4, k, k, k
  uint32_t w0 = g0 | (g1 << 26), w1 = (g1 >> 6) | (g2 << 20), w2 = (g2 >> 12) | (g3 << 14),
           w3 = (g3 >> 18) | (g4 << 8);
  uint64_t t = (uint64_t)w0 + s[0] + (k & 0xfffffffbu);
  tag[0] = (uint32_t)t;
  t = (uint64_t)w1 + s[1] + k + (t >> 32);
  tag[1] = (uint32_t)t;
  t = (uint64_t)w2 + s[2] + k + (t >> 32);
  tag[2] = (uint32_t)t;
  t = (uint64_t)w3 + s[3] + k + (t >> 32);
  tag[3] = (uint32_t)t;
}

}  // namespace mq
