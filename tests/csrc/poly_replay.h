// Host replay of mq_chacha.hip's poly_tag step loop over mq_poly_sched.h and mq_poly26.h (the
// schedule and the arithmetic the kernel itself calls), lane by lane, with the reference arithmetic
// mod 2^130 - 5 and the serial Poly1305 it is compared with. Shared by test_poly_pair.cpp (geometry:
// every stretch length, alignment and mixed wave) and test_poly_states.cpp (values: crafted packets
// whose accumulator ends on the boundaries of p26_finish).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// found through -I milli_quic_amd/csrc, so that a build may put another mq_poly26.h in front of it
#include "mq_poly26.h"
#include "mq_poly_sched.h"

using namespace mq;
typedef unsigned __int128 u128;

#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_what); \
      std::abort();                                                                           \
    }                                                                                         \
  } while (0)
inline char g_what[160] = "";

// ---- reference arithmetic mod p = 2^130 - 5: five limbs of 26 bits, always fully reduced ----------
struct Ref { uint64_t l[5]; };
inline Ref ref_norm(const u128 (&in)[5]) {
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
inline Ref ref_of(const P26& h) {
  u128 c[5];
  for (int i = 0; i < 5; ++i) c[i] = h.l[i];
  return ref_norm(c);
}
inline Ref ref_add(const Ref& a, const Ref& b) {
  u128 c[5];
  for (int i = 0; i < 5; ++i) c[i] = (u128)a.l[i] + b.l[i];
  return ref_norm(c);
}
inline Ref ref_mul(const Ref& a, const Ref& b) {
  u128 c[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 5; ++i)
    for (int k = 0; k < 5; ++k) {
      const u128 p = (u128)a.l[i] * b.l[k];
      if (i + k < 5) c[i + k] += p;
      else c[i + k - 5] += p * 5;  // 2^130 = 5
    }
  return ref_norm(c);
}
inline bool ref_eq(const Ref& a, const Ref& b) {
  for (int i = 0; i < 5; ++i)
    if (a.l[i] != b.l[i]) return false;
  return true;
}
inline Ref ref_block(const uint8_t* p, uint32_t hibit) {
  uint32_t w[4];
  std::memcpy(w, p, 16);
  return ref_of(p26_from_words(w[0], w[1], w[2], w[3], hibit));
}

// ---- the step loop of poly_tag ---------------------------------------------------------------------
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

inline uint64_t g_waves, g_pairs, g_singles;
inline bool g_stretch_seen[2][2][32];  // [G == 8][EDGE][steps]

inline void keep_bytes(uint32_t (&m)[4], int n) {  // zero the bytes from n on
  uint8_t b[16];
  std::memcpy(b, m, 16);
  for (int k = n; k < 16; ++k) b[k] = 0;
  std::memcpy(m, b, 16);
}

// poly_tag<G, PAIR, EDGE> over the lanes of the packets `in` (one lane group each); mem: the bytes
// the loads see. Returns the tags; loads: per lane, every address read, in order; sums (when given):
// per packet the group sum as p26_finish receives it.
template <int G, bool EDGE, bool PAIR>
static std::vector<Tag> run_wave(const std::vector<Pkt>& in, const std::vector<uint8_t>& mem, std::vector<std::vector<int64_t>>& loads,
                                 std::vector<P26>* sums = nullptr) {
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
  if (sums) sums->assign(n, P26{});
  for (int p = 0; p < n; ++p) {
    P26 sum;
    for (int q = 0; q < 5; ++q) {
      sum.l[q] = 0;
      for (int j = 0; j < G; ++j) sum.l[q] += L[(size_t)p * G + j].acc.l[q];
    }
    if (sums) (*sums)[p] = sum;
    p26_finish(sum, pk[p].sk, tags[p].w);
  }
  ++g_waves;
  return tags;
}

// RFC 8439 §2.8 / §2.5: the MAC input block by block, h = (h + block) r, tag = (h + s) mod 2^128
inline Tag serial_tag(const Pkt& p, const std::vector<uint8_t>& mem) {
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
