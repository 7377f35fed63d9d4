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
// Built with -fsanitize=address,undefined by tests/test_poly_pair.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../milli_quic_amd/csrc/mq_poly26.h"
#include "../../milli_quic_amd/csrc/mq_poly_sched.h"

using namespace mq;
typedef unsigned __int128 u128;

#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_what); \
      std::abort();                                                                           \
    }                                                                                         \
  } while (0)
static char g_what[160] = "";

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd(uint32_t n) { return (uint32_t)((rnd64() >> 20) % n); }

// ---- reference arithmetic mod p = 2^130 - 5: five limbs of 26 bits, always fully reduced ----------
struct Ref { uint64_t l[5]; };
static Ref ref_norm(const u128 (&in)[5]) {
  u128 c[5];
  for (int i = 0; i < 5; ++i) c[i] = in[i];
  for (int pass = 0; pass < 6; ++pass) {
    for (int i = 0; i < 4; ++i) {
      c[i + 1] += c[i] >> 26;
      c[i] &= 0x3ffffff;
    }
    c[0] += (c[4] >> 26) * 5;
    c[4] &= 0x3ffffff;
  }
  Ref r;
  for (int i = 0; i < 5; ++i) {
    if (c[i] >> 26) std::abort();  // the passes above leave a number below 2^130
    r.l[i] = (uint64_t)c[i];
  }
  // r < 2^130: subtract p once if r >= p
  uint64_t g[5], carry = 5;
  for (int i = 0; i < 5; ++i) {
    g[i] = r.l[i] + carry;
    carry = g[i] >> 26;
    g[i] &= 0x3ffffff;
  }
  if (carry)
    for (int i = 0; i < 5; ++i) r.l[i] = g[i];
  return r;
}
static Ref ref_of(const P26& h) {
  u128 c[5];
  for (int i = 0; i < 5; ++i) c[i] = h.l[i];
  return ref_norm(c);
}
static Ref ref_add(const Ref& a, const Ref& b) {
  u128 c[5];
  for (int i = 0; i < 5; ++i) c[i] = (u128)a.l[i] + b.l[i];
  return ref_norm(c);
}
static Ref ref_mul(const Ref& a, const Ref& b) {
  u128 c[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 5; ++i)
    for (int k = 0; k < 5; ++k) {
      const u128 p = (u128)a.l[i] * b.l[k];
      if (i + k < 5) c[i + k] += p;
      else c[i + k - 5] += p * 5;  // 2^130 = 5
    }
  return ref_norm(c);
}
static bool ref_eq(const Ref& a, const Ref& b) {
  for (int i = 0; i < 5; ++i)
    if (a.l[i] != b.l[i]) return false;
  return true;
}
static Ref ref_block(const uint8_t* p, uint32_t hibit) {
  uint32_t w[4];
  std::memcpy(w, p, 16);
  return ref_of(p26_from_words(w[0], w[1], w[2], w[3], hibit));
}

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
struct Pkt {
  uint32_t aad_len, ct_len;
  int64_t pkt;  // byte address of the packet in the wave's memory (any alignment)
  bool act;
  uint32_t rk[4], sk[4];  // the one-time key as the keystream gives it (r unclamped)
};
struct Blk { int64_t src; int rem; bool pre, lens; };
struct Lane {
  int i;
  Blk b;
  int64_t a;
  uint32_t m[4];
  P26 acc;
};
struct Tag { uint32_t w[4]; };

static uint64_t g_waves, g_pairs, g_singles;
static bool g_stretch_seen[2][2][32];  // [G == 8][EDGE][steps]

static void keep_bytes(uint32_t (&m)[4], int n) {  // zero the bytes from n on
  uint8_t b[16];
  std::memcpy(b, m, 16);
  for (int k = n; k < 16; ++k) b[k] = 0;
  std::memcpy(m, b, 16);
}

// poly_tag<G, PAIR, EDGE> over the lanes of the packets `in` (one lane group each); mem: the bytes
// the loads see. Returns the tags; loads: per lane, every address read, in order.
template <int G, bool EDGE, bool PAIR>
static std::vector<Tag> run_wave(const std::vector<Pkt>& in, const std::vector<uint8_t>& mem, std::vector<std::vector<int64_t>>& loads) {
  const int n = (int)in.size();
  std::vector<Pkt> pk = in;
  for (auto& p : pk)
    if (!p.act) p.aad_len = p.ct_len = 0, p.pkt = 0;  // what cc_wg_mac hands an inactive packet
  auto pay_of = [&](int p) { return pk[p].pkt + pk[p].aad_len; };
  loads.assign((size_t)n * G, std::vector<int64_t>());
  auto rd = [&](size_t lane, int64_t at, uint32_t (&m)[4]) {  // four little-endian words from byte address at
    CHECK(at >= 0 && at + 16 <= (int64_t)mem.size());
    std::memcpy(m, mem.data() + at, 16);
    loads[lane].push_back(at);
  };
  // a dword-aligned load with the payload's selector: the bytes from al + (pay & 3) on; the kernel
  // reads the five dwords from al
  auto rd_sel = [&](int p, int j, int64_t al, uint32_t (&m)[4]) {
    CHECK((al & 3) == 0 && al + 20 <= (int64_t)mem.size());
    rd((size_t)p * G + j, al + (pay_of(p) & 3), m);
  };

  // set-up: powers by the group prefix, exactly poly_tag's multiplies
  std::vector<P26> v((size_t)n * G), rG(n);
  std::vector<P26m> mG(n), mG2(n);
  std::vector<std::vector<P26m>> mlast(n, std::vector<P26m>(G));
  for (int p = 0; p < n; ++p) {
    const uint32_t* rk = pk[p].rk;
    const P26 r = p26_from_words(rk[0] & 0x0fffffffu, rk[1] & 0x0ffffffcu, rk[2] & 0x0ffffffcu, rk[3] & 0x0ffffffcu, 0);
    P26 t = r;
    p26_mul(t, p26_mult(r));
    for (int j = 0; j < G; ++j) v[(size_t)p * G + j] = (j & 1) ? t : r;
    for (int j = 0; j < G; ++j) {
      P26 u = v[(size_t)p * G + j];
      p26_mul(u, p26_mult(t));
      if (j & 2) v[(size_t)p * G + j] = u;
    }
    if (G == 8) {
      const P26 r4 = v[(size_t)p * G + 3];
      for (int j = 0; j < G; ++j) {
        P26 u = v[(size_t)p * G + j];
        p26_mul(u, p26_mult(r4));
        if (j & 4) v[(size_t)p * G + j] = u;
      }
    }
    rG[p] = v[(size_t)p * G + G - 1];
    mG[p] = p26_mult(rG[p]);
    for (int j = 0; j < G; ++j) mlast[p][j] = p26_mult(v[(size_t)p * G + G - 1 - j]);
    // the prefix really holds r^(j+1)
    Ref want = ref_of(r);
    for (int j = 0; j < G; ++j) {
      CHECK(ref_eq(ref_of(v[(size_t)p * G + j]), want));
      want = ref_mul(want, ref_of(r));
    }
  }

  std::vector<PolyGeom> geo(n);
  uint32_t Kmax = 0;
  for (int p = 0; p < n; ++p) {
    geo[p] = poly_geom<G>(pk[p].aad_len, pk[p].ct_len);
    if (pk[p].act && geo[p].K > Kmax) Kmax = geo[p].K;
  }
  std::vector<PolyLean> ln(n);
  uint32_t klo = 0, khi = 0xFFFFFFFFu;
  for (int p = 0; p < n; ++p) {
    ln[p] = poly_lean<G, EDGE>(geo[p].A, geo[p].nb, pk[p].ct_len, Kmax, pk[p].act);
    if (ln[p].k_lo > klo) klo = ln[p].k_lo;
    if (ln[p].k_hi < khi) khi = ln[p].k_hi;
  }
  if (khi > Kmax - 1) khi = Kmax - 1;  // as the kernel: never read when Kmax == 0

  std::vector<Lane> L((size_t)n * G);
  for (auto& l : L)
    for (int q = 0; q < 5; ++q) l.acc.l[q] = 0;
  auto where = [&](int p, int i) {
    const PolyBlk pb = poly_blk(geo[p].A, geo[p].T, pk[p].aad_len, pk[p].ct_len, i);
    Blk b;
    b.pre = pb.pre;
    b.lens = pb.lens;
    b.src = pb.aad ? pk[p].pkt + pb.off : pay_of(p) + pb.off;
    b.rem = pb.rem;
    if (b.pre || b.lens) b.src = pk[p].pkt;
    return b;
  };
  auto absorb = [&](int p, Lane& l) {
    const Blk& b = l.b;
    uint32_t m[4] = {l.m[0], l.m[1], l.m[2], l.m[3]};
    const int rem = b.rem < 0 ? 0 : (b.rem > 16 ? 16 : b.rem);
    if (!EDGE) {
      keep_bytes(m, b.pre ? 0 : rem);
      if (b.lens) { m[0] = pk[p].aad_len; m[1] = 0; m[2] = pk[p].ct_len; m[3] = 0; }
    } else {
      keep_bytes(m, b.pre || b.lens ? 0 : rem);
      m[0] = b.lens ? pk[p].aad_len : m[0];
      m[2] = b.lens ? pk[p].ct_len : m[2];
    }
    const P26 x = p26_from_words(m[0], m[1], m[2], m[3], b.pre ? 0u : 1u);
    for (int q = 0; q < 5; ++q) l.acc.l[q] += x.l[q];
  };
  auto add_whole = [&](Lane& l) {
    const P26 x = p26_from_words(l.m[0], l.m[1], l.m[2], l.m[3], 1u);
    for (int q = 0; q < 5; ++q) l.acc.l[q] += x.l[q];
  };

  uint32_t stretch = 0;
  if (Kmax > 0) {
    for (int p = 0; p < n; ++p)
      for (int j = 0; j < G; ++j) {
        Lane& l = L[(size_t)p * G + j];
        l.i = j - ln[p].z;
        l.b = where(p, l.i);
        rd((size_t)p * G + j, l.b.src, l.m);
      }
    for (uint32_t k = 0; k + 1 < Kmax; ++k) {
      if (k == klo && k < khi) {
        stretch = khi - klo;
        for (auto& l : L) l.a = l.b.src & ~(int64_t)3;
        if (PAIR && khi - k >= 2) {
          for (int p = 0; p < n; ++p) {
            P26 r2G = rG[p];
            p26_mul(r2G, mG[p]);
            mG2[p] = p26_mult(r2G);
          }
          for (; k + 1 < khi; k += 2) {
            ++g_pairs;
            for (int p = 0; p < n; ++p)
              for (int j = 0; j < G; ++j) {
                Lane& l = L[(size_t)p * G + j];
                add_whole(l);
                l.a += 16 * G;
                rd_sel(p, j, l.a, l.m);
                const P26 y = p26_from_words(l.m[0], l.m[1], l.m[2], l.m[3], 1u);
                l.a += 16 * G;
                rd_sel(p, j, l.a, l.m);
                for (int q = 0; q < 5; ++q) CHECK(l.acc.l[q] < (1u << 27) + (1u << 9) && y.l[q] < (1u << 26));
                p26_mul2(l.acc, mG2[p], y, mG[p]);
              }
          }
        }
        uint32_t singles = 0;
        for (; k < khi; ++k) {
          ++g_singles;
          ++singles;
          for (int p = 0; p < n; ++p)
            for (int j = 0; j < G; ++j) {
              Lane& l = L[(size_t)p * G + j];
              add_whole(l);
              l.a += 16 * G;
              rd_sel(p, j, l.a, l.m);
              p26_mul(l.acc, mG[p]);
            }
        }
        CHECK(!PAIR || singles <= 1);
        const uint32_t nl = khi - klo;
        for (auto& l : L) {
          l.i += (int)(G * nl);
          l.b.src += 16 * (int64_t)G * nl;
          l.b.rem -= (int)(16 * G * nl);
          if (EDGE) l.b.lens = l.b.rem <= 0;
        }
        if (k + 1 >= Kmax) break;
      }
      bool all_steady = true;
      for (int p = 0; p < n; ++p)
        for (int j = 0; j < G; ++j) {
          Lane& l = L[(size_t)p * G + j];
          absorb(p, l);
          const bool steady = !pk[p].act || (l.i >= (int)geo[p].A && l.i + G < ln[p].ct_full_end);
          all_steady = all_steady && steady;
          l.i += G;
        }
      for (int p = 0; p < n; ++p)
        for (int j = 0; j < G; ++j) {
          Lane& l = L[(size_t)p * G + j];
          if (all_steady) {
            l.b.src += 16 * G;
            l.b.rem -= 16 * G;
            rd_sel(p, j, l.b.src & ~(int64_t)3, l.m);
          } else {
            l.b = where(p, l.i);
            rd((size_t)p * G + j, l.b.src, l.m);
          }
          p26_mul(l.acc, mG[p]);
        }
    }
    for (int p = 0; p < n; ++p)
      for (int j = 0; j < G; ++j) {
        Lane& l = L[(size_t)p * G + j];
        absorb(p, l);
        p26_mul(l.acc, mlast[p][j]);
      }
    if (stretch < 32) g_stretch_seen[G == 8][EDGE][stretch] = true;
  }
  std::vector<Tag> tags(n);
  for (int p = 0; p < n; ++p) {
    P26 sum;
    for (int q = 0; q < 5; ++q) {
      sum.l[q] = 0;
      for (int j = 0; j < G; ++j) sum.l[q] += L[(size_t)p * G + j].acc.l[q];
    }
    p26_finish(sum, pk[p].sk, tags[p].w);
  }
  ++g_waves;
  return tags;
}

// RFC 8439 §2.8 / §2.5: the MAC input block by block, h = (h + block) r, tag = (h + s) mod 2^128
static Tag serial_tag(const Pkt& p, const std::vector<uint8_t>& mem) {
  std::vector<uint8_t> in;
  auto pad16 = [&] { while (in.size() % 16) in.push_back(0); };
  in.insert(in.end(), mem.begin() + p.pkt, mem.begin() + p.pkt + p.aad_len);
  pad16();
  in.insert(in.end(), mem.begin() + p.pkt + p.aad_len, mem.begin() + p.pkt + p.aad_len + p.ct_len);
  pad16();
  for (uint64_t v : {(uint64_t)p.aad_len, (uint64_t)p.ct_len})
    for (int b = 0; b < 8; ++b) in.push_back((uint8_t)(v >> (8 * b)));
  const Ref r = ref_of(p26_from_words(p.rk[0] & 0x0fffffffu, p.rk[1] & 0x0ffffffcu, p.rk[2] & 0x0ffffffcu, p.rk[3] & 0x0ffffffcu, 0));
  Ref h = {{0, 0, 0, 0, 0}};
  for (size_t o = 0; o < in.size(); o += 16) h = ref_mul(ref_add(h, ref_block(in.data() + o, 1)), r);
  u128 acc = 0;
  for (int i = 4; i >= 0; --i) acc = (acc << 26) | h.l[i];  // mod 2^128 by truncation
  const u128 s = (u128)p.sk[0] | (u128)p.sk[1] << 32 | (u128)p.sk[2] << 64 | (u128)p.sk[3] << 96;
  acc += s;
  Tag t;
  for (int w = 0; w < 4; ++w) t.w[w] = (uint32_t)(acc >> (32 * w));
  return t;
}

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
