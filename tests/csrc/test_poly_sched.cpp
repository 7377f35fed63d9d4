// Host check of the interleaved Poly1305 schedule (milli_quic_amd/csrc/mq_poly_sched.h) that
// mq_chacha.hip's poly_tag runs: the step loop of poly_tag is replayed here lane by lane — the
// general steps, the lean stretch with its fixed-stride look-ahead load and the catch-up behind it,
// the final absorb — with the wave's min / max reductions taken over the emulated packets, and
// every absorb and every load is compared with what RFC 8439 §2.8 asks of it:
//   * every MAC block 0 .. nb-1 of an active packet is absorbed exactly once, on group lane
//     (i + z) % G in step (i + z) / G, from the right address and with the right count of real bytes;
//   * prepended zero blocks are absorbed only at indices < 0, the lengths block only at nb - 1;
//   * every step of the lean stretch [klo, khi) has only whole ciphertext blocks on active lanes;
//   * every load of an active lane stays inside [pkt & ~3, pay + 16 T + 20): at most the tag and
//     19 bytes behind it; an inactive lane strides no further than 16 G (Kmax - 1) + 20 from its base.
// Built with -fsanitize=address,undefined by tests/test_poly_sched.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../milli_quic_amd/csrc/mq_poly_sched.h"

using namespace mq;

#define CHECK(c)                                                                                   \
  do {                                                                                             \
    if (!(c)) {                                                                                    \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed: G %d packet %d lane %d step %u (aad %u ct %u)\n", \
                   __FILE__, __LINE__, #c, g_G, g_p, g_j, g_k, g_aad, g_ct);                         \
      std::abort();                                                                                \
    }                                                                                              \
  } while (0)

static int g_G, g_p, g_j;
static uint32_t g_k, g_aad, g_ct;

struct Pkt {
  uint32_t aad_len, ct_len;
  int64_t pkt;  // byte address of the packet (any alignment)
  bool act;
};

struct Blk { int64_t src; int rem; bool pre, lens; };

struct Lane {
  int i;
  Blk b;
  int64_t a;       // the lean stretch's dword-aligned address
  int64_t loaded;  // byte address the four message words in flight were read from
};

static uint64_t g_cases, g_lean_steps, g_lean_to_last;

template <int G, bool EDGE>
static void run_wave(const std::vector<Pkt>& in) {
  const int n = (int)in.size();
  g_G = G;
  // what the kernel hands an inactive packet: no AAD, no payload
  std::vector<Pkt> pk = in;
  for (auto& p : pk)
    if (!p.act) p.aad_len = p.ct_len = 0;
  std::vector<PolyGeom> geo(n);
  uint32_t Kmax = 0;
  for (int p = 0; p < n; ++p) {
    geo[p] = poly_geom<G>(pk[p].aad_len, pk[p].ct_len);
    if (pk[p].act && geo[p].K > Kmax) Kmax = geo[p].K;
  }
  if (Kmax == 0) return;  // no active packet: poly_tag absorbs nothing
  std::vector<PolyLean> ln(n);
  uint32_t klo = 0, khi = 0xFFFFFFFFu;
  for (int p = 0; p < n; ++p) {
    ln[p] = poly_lean<G, EDGE>(geo[p].A, geo[p].nb, pk[p].ct_len, Kmax, pk[p].act);
    if (ln[p].k_lo > klo) klo = ln[p].k_lo;
    if (ln[p].k_hi < khi) khi = ln[p].k_hi;
  }
  if (khi > Kmax - 1) khi = Kmax - 1;

  std::vector<std::vector<int>> seen(n);
  for (int p = 0; p < n; ++p) seen[p].assign(geo[p].nb, 0);
  std::vector<Lane> L((size_t)n * G);

  auto pay_of = [&](int p) { return pk[p].pkt + pk[p].aad_len; };
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
  // a load of five dwords from the dword-aligned address `al`
  auto check_load = [&](int p, int64_t al) {
    CHECK((al & 3) == 0);
    if (pk[p].act) {
      CHECK(al >= (pk[p].pkt & ~(int64_t)3));
      CHECK(al + 20 <= pay_of(p) + 16 * (int64_t)geo[p].T + 20);
    } else {
      CHECK(al >= (pk[p].pkt & ~(int64_t)3));
      CHECK(al + 20 <= pk[p].pkt + 16 * (int64_t)G * (Kmax - 1) + 20);
    }
  };
  auto load_words = [&](int p, Lane& l) {  // load_words(sp, b.src, m)
    check_load(p, l.b.src & ~(int64_t)3);
    l.loaded = l.b.src;
  };
  auto load_sel_pay = [&](int p, Lane& l, int64_t al) {  // load_words_sel(sp, al, sel_pay, m)
    check_load(p, al);
    l.loaded = al + (pay_of(p) & 3);
  };
  // the absorb of step k: b (or, in the lean stretch, a whole block with the 2^128 bit) and the
  // words in flight
  auto absorb = [&](int p, int j, uint32_t k, const Lane& l, bool lean) {
    g_p = p; g_j = j; g_k = k; g_aad = pk[p].aad_len; g_ct = pk[p].ct_len;
    if (!pk[p].act) return;
    const int A = (int)geo[p].A, T = (int)geo[p].T;
    const int i = (int)(G * k) + j - ln[p].z;  // the block this lane owes this step
    CHECK(i <= A + T);
    if (lean) {
      CHECK(k >= klo && k < khi);
      CHECK(i >= A && i < ln[p].ct_full_end);
      CHECK(l.loaded == pay_of(p) + 16 * (int64_t)(i - A));
      ++seen[p][i];
      return;
    }
    CHECK(l.i == i);
    if (i < 0) {
      CHECK(l.b.pre);
      return;
    }
    CHECK(!l.b.pre);
    ++seen[p][i];
    if (i == A + T) {
      CHECK(l.b.lens);  // the words are replaced by the lengths
      return;
    }
    CHECK(!l.b.lens);
    const int64_t at = i < A ? pk[p].pkt + 16 * (int64_t)i : pay_of(p) + 16 * (int64_t)(i - A);
    const int real = i < A ? (int)pk[p].aad_len - 16 * i : (int)pk[p].ct_len - 16 * (i - A);
    CHECK(l.loaded == at);
    CHECK(real > 0);
    CHECK((l.b.rem < 16 ? l.b.rem : 16) == (real < 16 ? real : 16));  // bytes the mask keeps
  };

  for (int p = 0; p < n; ++p)
    for (int j = 0; j < G; ++j) {
      Lane& l = L[(size_t)p * G + j];
      l.i = j - ln[p].z;
      l.b = where(p, l.i);
      load_words(p, l);
    }
  uint32_t k = 0;
  for (; k + 1 < Kmax; ++k) {
    if (k == klo && k < khi) {
      for (int p = 0; p < n; ++p)
        for (int j = 0; j < G; ++j) L[(size_t)p * G + j].a = L[(size_t)p * G + j].b.src & ~(int64_t)3;
      for (; k < khi; ++k) {
        ++g_lean_steps;
        for (int p = 0; p < n; ++p)
          for (int j = 0; j < G; ++j) {
            Lane& l = L[(size_t)p * G + j];
            absorb(p, j, k, l, true);
            l.a += 16 * G;
            load_sel_pay(p, l, l.a);
          }
      }
      const uint32_t nl = khi - klo;
      for (int p = 0; p < n; ++p)
        for (int j = 0; j < G; ++j) {
          Lane& l = L[(size_t)p * G + j];
          l.i += (int)(G * nl);
          l.b.src += 16 * (int64_t)G * nl;
          l.b.rem -= (int)(16 * G * nl);
          if (EDGE) l.b.lens = l.b.rem <= 0;
        }
      if (k + 1 >= Kmax) {
        ++g_lean_to_last;
        break;
      }
    }
    bool all_steady = true;
    for (int p = 0; p < n; ++p)
      for (int j = 0; j < G; ++j) {
        Lane& l = L[(size_t)p * G + j];
        absorb(p, j, k, l, false);
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
          load_sel_pay(p, l, l.b.src & ~(int64_t)3);
        } else {
          l.b = where(p, l.i);
          load_words(p, l);
        }
      }
  }
  k = Kmax - 1;
  for (int p = 0; p < n; ++p)
    for (int j = 0; j < G; ++j) absorb(p, j, k, L[(size_t)p * G + j], false);
  for (int p = 0; p < n; ++p) {
    if (!pk[p].act) continue;
    g_p = p; g_j = -1; g_aad = pk[p].aad_len; g_ct = pk[p].ct_len;
    for (uint32_t i = 0; i < geo[p].nb; ++i) {
      g_k = i;
      CHECK(seen[p][i] == 1);
    }
  }
  ++g_cases;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 20) % n);
}

template <int G, bool EDGE>
static void run_all() {
  // one geometry for the whole wave (as config B's tiles), every payload alignment in turn
  for (uint32_t aad = 1; aad <= 48; ++aad)
    for (uint32_t ct = 0; ct <= 640; ++ct) {
      std::vector<Pkt> w{Pkt{aad, ct, (int64_t)(4096 + ((aad * 7 + ct) & 3)), true}};
      run_wave<G, EDGE>(w);
    }
  // config B itself and a long packet
  run_wave<G, EDGE>({Pkt{13, 1171, 4096, true}});
  run_wave<G, EDGE>({Pkt{13, 2371, 4099, true}});
  // groups of 2..8 packets of different geometry, some inactive: klo, khi and Kmax come from the
  // reductions; every few waves one packet of one step (Kmax = 1 alone) beside a long one
  for (int t = 0; t < 10000; ++t) {
    const int n = 2 + (int)rnd(7);
    std::vector<Pkt> w;
    int64_t at = 4096 + rnd(4);
    const uint32_t span = t % 3 == 0 ? 1280 : (t % 3 == 1 ? 200 : 48);
    for (int p = 0; p < n; ++p) {
      Pkt q{1 + rnd(48), rnd(span), at, rnd(5) != 0};
      if (t % 7 == 0 && p == 0) q = Pkt{1 + rnd(16), rnd(16 * (G > 2 ? G - 2 : 1) - 15), at, true};
      if (t % 7 == 0 && p == 1) q = Pkt{13, 1171, at, true};
      if (t % 11 == 0 && p >= 2) q.ct_len = w[1].ct_len, q.aad_len = w[1].aad_len;
      w.push_back(q);
      at += q.aad_len + q.ct_len + 16;
    }
    run_wave<G, EDGE>(w);
  }
}

int main() {
  run_all<1, true>();
  run_all<2, true>();
  run_all<4, true>();
  run_all<8, true>();
  CHECK(g_lean_to_last > 0);
  // the former bound (EDGE = false, what poly_tag's narrow lane groups run): the stretch's last load
  // is a whole block too, so it never reaches the final absorb
  const uint64_t to_last = g_lean_to_last;
  run_all<1, false>();
  run_all<2, false>();
  run_all<4, false>();
  run_all<8, false>();
  CHECK(g_lean_to_last == to_last);
  // the figures the design document quotes for config B (G = 8, AAD 13 B, ciphertext 1171 B):
  // steps 1..8 of 10 are lean, the final absorb follows the stretch
  {
    const PolyGeom g = poly_geom<8>(13, 1171);
    const PolyLean l = poly_lean<8>(g.A, g.nb, 1171, g.K, true);
    g_G = 8; g_p = g_j = 0; g_k = 0; g_aad = 13; g_ct = 1171;
    CHECK(g.A == 1 && g.T == 74 && g.nb == 76 && g.K == 10 && l.z == 4 && l.ct_full_end == 74);
    CHECK(l.k_lo == 1 && l.k_hi == 9);
  }
  std::printf("poly sched ok: %llu waves, %llu lean steps, %llu stretches ending at the final absorb\n",
              (unsigned long long)g_cases, (unsigned long long)g_lean_steps, (unsigned long long)g_lean_to_last);
  return 0;
}
