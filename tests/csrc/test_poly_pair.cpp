// Host check of the paired Poly1305 reduction (milli_quic_amd/csrc/mq_poly26.h p26_mul2) and of the
// step loop of mq_chacha.hip's poly_tag with its pair loop, on real bytes:
//   1. p26_mul2(h, m2, y, m1) against plain arithmetic mod 2^130 - 5 (unsigned __int128 columns), on
//      random operands and on the corner operands of its documented bound: every column sum (with the
//      carry that enters it) below 2^58, the result congruent and inside p26_mul's output bounds.
//   2. poly_tag's whole step loop replayed lane by lane over mq_poly_sched.h and mq_poly26.h — the
//      set-up powers by the group prefix, the general steps, the lean stretch as pair loop plus odd
//      single step, the final multiply, the group sum, p26_finish — for G = 4 and 8, EDGE both ways,
//      over waves of packets of different geometry with some inactive. Every tag is compared with a
//      straightforward serial Poly1305 of the RFC 8439 §2.8 MAC input under the same key, and the
//      addresses loaded with those of the same replay without the pair loop (the same sequence).
//      Lean stretches of 0, 1, 2, 3, 4, 5, 16 and 17 steps must all have occurred.
// The replay, the reference arithmetic and the serial Poly1305 live in poly_replay.h, which
// test_poly_states.cpp runs on crafted packets.
// Built with -fsanitize=address,undefined by tests/test_poly_pair.py.
#include "poly_replay.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd(uint32_t n) { return (uint32_t)((rnd64() >> 20) % n); }

// ---- 1. p26_mul2 ---------------------------------------------------------------------------------
static uint64_t g_mul2_cases;
static uint64_t g_col_max;
static void check_mul2(const P26& h, const P26& r2, const P26& y, const P26& r1) {
  const P26m m2 = p26_mult(r2), m1 = p26_mult(r1);
  // the column sums as p26_mul2 forms them (s[i] = 5 r[i + 1]), each with the carry that enters it
  u128 carry = 0;
  for (int c = 0; c < 5; ++c) {
    u128 d = carry;
    for (int i = 0; i < 5; ++i) {
      const int k = c - i;
      d += (u128)h.l[i] * (k >= 0 ? m2.r[k] : m2.s[k + 4]);
      d += (u128)y.l[i] * (k >= 0 ? m1.r[k] : m1.s[k + 4]);
    }
    CHECK(d < ((u128)1 << 58));
    if ((uint64_t)d > g_col_max) g_col_max = (uint64_t)d;
    carry = d >> 26;
    CHECK(carry < ((u128)1 << 32));
  }
  const Ref want = ref_add(ref_mul(ref_of(h), ref_of(r2)), ref_mul(ref_of(y), ref_of(r1)));
  P26 got = h;
  p26_mul2(got, m2, y, m1);
  CHECK(ref_eq(ref_of(got), want));
  CHECK(got.l[0] < (1u << 26) && got.l[2] < (1u << 26) && got.l[3] < (1u << 26) && got.l[4] < (1u << 26));
  CHECK(got.l[1] < (1u << 26) + (1u << 9));
  // and the two single reductions it replaces: ((h r1) + y) r1 when r2 = r1^2 is checked in part 2
  ++g_mul2_cases;
}
static void test_mul2() {
  std::snprintf(g_what, sizeof g_what, "p26_mul2");
  const uint32_t HMAX = (1u << 27) - 1, YMAX = (1u << 26) - 1, MMAX = (1u << 26) + (1u << 9) - 1;
  P26 h, y, r2, r1;
  // every operand at its corner, then each limb of each operand at its corner or at zero
  for (int i = 0; i < 5; ++i) h.l[i] = HMAX, y.l[i] = YMAX, r2.l[i] = MMAX, r1.l[i] = MMAX;
  check_mul2(h, r2, y, r1);
  for (uint32_t mask = 0; mask < (1u << 20); mask += 1 + rnd(37)) {
    for (int i = 0; i < 5; ++i) {
      h.l[i] = (mask >> i & 1) ? HMAX : 0;
      y.l[i] = (mask >> (5 + i) & 1) ? YMAX : 0;
      r2.l[i] = (mask >> (10 + i) & 1) ? MMAX : 0;
      r1.l[i] = (mask >> (15 + i) & 1) ? MMAX : 0;
    }
    check_mul2(h, r2, y, r1);
  }
  for (int t = 0; t < 200000; ++t) {
    for (int i = 0; i < 5; ++i) {
      h.l[i] = (uint32_t)rnd64() & HMAX;
      y.l[i] = (uint32_t)rnd64() & YMAX;
      r2.l[i] = (uint32_t)(rnd64() % (MMAX + 1ull));
      r1.l[i] = (uint32_t)(rnd64() % (MMAX + 1ull));
    }
    // operands near the corner in a random subset of limbs
    if (t % 4 == 0)
      for (int i = 0; i < 5; ++i) {
        if (rnd(2)) h.l[i] = HMAX - rnd(3);
        if (rnd(2)) y.l[i] = YMAX - rnd(3);
        if (rnd(2)) r2.l[i] = MMAX - rnd(3);
        if (rnd(2)) r1.l[i] = MMAX - rnd(3);
      }
    check_mul2(h, r2, y, r1);
  }
  // two Horner steps: ((h + x) m + y) m by p26_mul twice equals p26_mul2(h + x, m^2, y, m) mod p
  for (int t = 0; t < 20000; ++t) {
    P26 x;
    for (int i = 0; i < 5; ++i) {
      h.l[i] = (uint32_t)rnd64() & YMAX;
      x.l[i] = (uint32_t)rnd64() & YMAX;
      y.l[i] = (uint32_t)rnd64() & YMAX;
      r1.l[i] = (uint32_t)rnd64() & YMAX;
    }
    const P26m m1 = p26_mult(r1);
    P26 sq = r1;
    p26_mul(sq, m1);
    P26 a = h, b = h;
    for (int i = 0; i < 5; ++i) a.l[i] += x.l[i], b.l[i] += x.l[i];
    p26_mul(a, m1);
    for (int i = 0; i < 5; ++i) a.l[i] += y.l[i];
    p26_mul(a, m1);
    p26_mul2(b, p26_mult(sq), y, m1);
    CHECK(ref_eq(ref_of(a), ref_of(b)));
  }
}

// ---- 2. the step loop of poly_tag ------------------------------------------------------------------
// Lays the packets out back to back from `at0` on (16 bytes of tag behind each), fills the memory
// with random bytes up to the furthest byte a load may touch, runs the replay with and without the
// pair loop and compares tags and load sequences.
template <int G, bool EDGE>
static void run_case(std::vector<Pkt> w, int64_t at0) {
  int64_t at = at0, end = 0;
  uint32_t Kmax = 0;
  for (auto& p : w) {
    p.pkt = at;
    at += p.aad_len + p.ct_len + 16;
    for (int k = 0; k < 4; ++k) p.rk[k] = (uint32_t)rnd64(), p.sk[k] = (uint32_t)rnd64();
    if (rnd(16) == 0)
      for (int k = 0; k < 4; ++k) p.rk[k] = 0xffffffffu;  // the largest clamped r
    if (!p.act) continue;
    const PolyGeom g = poly_geom<G>(p.aad_len, p.ct_len);
    if (g.K > Kmax) Kmax = g.K;
    const int64_t lim = p.pkt + p.aad_len + 16 * (int64_t)g.T + 20;  // the look-ahead bound
    if (lim > end) end = lim;
  }
  if (Kmax == 0) return;
  const int64_t idle = 16 * (int64_t)G * (Kmax - 1) + 20;  // an inactive group strides from address 0
  if (idle > end) end = idle;
  std::vector<uint8_t> mem((size_t)end);
  for (auto& b : mem) b = (uint8_t)rnd64();
  if (rnd(8) == 0)
    for (auto& b : mem) b = 0xff;  // every message limb at its maximum
  std::snprintf(g_what, sizeof g_what, "G %d EDGE %d: %zu packets, first aad %u ct %u at %lld", G, (int)EDGE, w.size(),
                w[0].aad_len, w[0].ct_len, (long long)at0);
  std::vector<std::vector<int64_t>> la, lb;
  const std::vector<Tag> ta = run_wave<G, EDGE, true>(w, mem, la);
  const std::vector<Tag> tb = run_wave<G, EDGE, false>(w, mem, lb);
  CHECK(la == lb);
  for (size_t p = 0; p < w.size(); ++p) {
    if (!w[p].act) continue;
    const Tag want = serial_tag(w[p], mem);
    CHECK(std::memcmp(ta[p].w, want.w, 16) == 0);
    CHECK(std::memcmp(tb[p].w, want.w, 16) == 0);
  }
}

template <int G, bool EDGE>
static void run_all() {
  Pkt z{};
  z.act = true;
  // one geometry for the whole wave (as config B's tiles): every ciphertext length up to 20 steps and
  // a few, every payload alignment in turn; two packets so that a second lane group runs beside it
  for (uint32_t ct = 0; ct <= 16u * G * 20 + 80; ++ct) {
    Pkt a = z, b = z;
    a.aad_len = b.aad_len = ct % 5 == 0 ? 1 + ct % 32 : 13;
    a.ct_len = b.ct_len = ct;
    run_case<G, EDGE>({a, b}, ct & 3);
  }
  // config B itself
  {
    Pkt a = z;
    a.aad_len = 13, a.ct_len = 1171;
    run_case<G, EDGE>(std::vector<Pkt>(16, a), 3);
  }
  // packets of different geometry, some inactive: klo, khi and Kmax come from the reductions
  for (int t = 0; t < 1500; ++t) {
    const int n = 2 + (int)rnd(7);
    std::vector<Pkt> w;
    const uint32_t span = t % 3 == 0 ? 1280 : (t % 3 == 1 ? 2400 : 200);
    for (int p = 0; p < n; ++p) {
      Pkt q = z;
      q.aad_len = 1 + rnd(48);
      q.ct_len = rnd(span);
      q.act = rnd(5) != 0;
      if (t % 5 == 0 && p > 0 && rnd(2)) q.ct_len = w[0].ct_len, q.aad_len = w[0].aad_len;
      if (t % 7 == 0 && p == 0) q.ct_len = 1171, q.aad_len = 13, q.act = true;
      w.push_back(q);
    }
    run_case<G, EDGE>(w, rnd(4));
  }
  for (int len : {0, 1, 2, 3, 4, 5, 16, 17}) {
    std::snprintf(g_what, sizeof g_what, "G %d EDGE %d: no lean stretch of %d steps", G, (int)EDGE, len);
    CHECK(g_stretch_seen[G == 8][EDGE][len]);
  }
}

int main() {
  test_mul2();
  run_all<4, true>();
  run_all<4, false>();
  run_all<8, true>();
  run_all<8, false>();
  // the figures the design document quotes for the workgroup MAC at config B (G = 4, AAD 13 B,
  // ciphertext 1171 B, 19 steps): 16 lean steps with the former edge steps, 17 with the edge steps
  {
    std::snprintf(g_what, sizeof g_what, "config B geometry");
    const PolyGeom g = poly_geom<4>(13, 1171);
    const PolyLean e = poly_lean<4, true>(g.A, g.nb, 1171, g.K, true), f = poly_lean<4, false>(g.A, g.nb, 1171, g.K, true);
    CHECK(g.A == 1 && g.T == 74 && g.nb == 76 && g.K == 19);
    CHECK(f.k_lo == 1 && f.k_hi == 17 && e.k_lo == 1 && e.k_hi == 18);
  }
  std::printf("poly pair ok: %llu p26_mul2 cases (largest column %.3f * 2^53), %llu waves, %llu pair steps, %llu single lean steps\n",
              (unsigned long long)g_mul2_cases, (double)g_col_max / 9007199254740992.0, (unsigned long long)g_waves,
              (unsigned long long)g_pairs, (unsigned long long)g_singles);
  return 0;
}
