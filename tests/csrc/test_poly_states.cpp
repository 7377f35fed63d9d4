// Host replay of crafted ChaCha20-Poly1305 packets (tests/poly_states.py: the Poly1305 accumulator
// ends on a chosen residue mod 2^130 - 5) through every reduction that stands before p26_finish
// (milli_quic_amd/csrc/mq_poly26.h), with the arithmetic and the schedule the kernels call:
//   serial     Horner over p26_mul, one lane (the narrow tiles' G = 1)
//   g4, g4p    poly_tag's step loop, four lanes per packet, without and with the pair loop (p26_mul2)
//   g8, g8p    the same with eight lanes and the edge steps (kEdge = G == 8, as the kernel)
//   resident   mq_resident.hip's schedule: the 64 powers by the prefix scan, 64-way Horner with
//              p26_mul standing in for p26_mul_lat (the same column sums and carries), 64-bit limb
//              sums, p26_from_sums
// The lane-group replays (poly_replay.h) run every vector in two waves: beside a random packet of its
// own geometry, and behind a longer one (prepended zero blocks, a shorter common lean stretch).
// Reads the vector file named by argv[1], one vector per line:
//   name  small  otk(hex 32 B)  aad_len  ct_len  padded MAC input (hex)  tag (hex 16 B)
// (small: 1 when the target residue is in 0 .. 4) and prints per vector and schedule
//   vec <name> <ct_len> <small> <schedule> match=<0|1> ge_p=<0|1> limb26=<0|1>
// ge_p: the value entering p26_finish was >= p; limb26: one of its limbs was >= 2^26. Then one line
// per schedule with the count of vectors that entered >= p, and the count of random neighbours in the
// lane-group waves whose tag differed from the reference arithmetic. Exit status 1 when a tag differs.
// Built with -fsanitize=address,undefined by tests/test_poly_states.py.
#include <string>

#include "poly_replay.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

struct Vec {
  std::string name;
  int small;
  uint32_t aad_len, ct_len;
  uint32_t otk[8];
  std::vector<uint8_t> aad_ct;  // AAD || ciphertext, unpadded
  Tag want;
};
struct Entered { bool ge_p, limb26; };
static size_t g_neighbours_wrong;  // random packets beside the vectors whose tag differed

static std::vector<uint8_t> unhex(const std::string& s) {
  CHECK(s.size() % 2 == 0);
  std::vector<uint8_t> out(s.size() / 2);
  auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)(nib(s[2 * i]) << 4 | nib(s[2 * i + 1]));
  return out;
}

// the number the limbs stand for against p, without folding: carries into a sixth limb
static Entered entered(const P26& h) {
  uint64_t l[6] = {h.l[0], h.l[1], h.l[2], h.l[3], h.l[4], 0};
  Entered e{false, false};
  for (int i = 0; i < 5; ++i) e.limb26 = e.limb26 || h.l[i] >= (1u << 26);
  for (int i = 0; i < 5; ++i) {
    l[i + 1] += l[i] >> 26;
    l[i] &= 0x3ffffff;
  }
  e.ge_p = l[5] != 0 || (l[4] == 0x3ffffff && l[3] == 0x3ffffff && l[2] == 0x3ffffff && l[1] == 0x3ffffff && l[0] >= 0x3fffffb);
  return e;
}

static P26 clamped_r(const uint32_t* rk) {
  return p26_from_words(rk[0] & 0x0fffffffu, rk[1] & 0x0ffffffcu, rk[2] & 0x0ffffffcu, rk[3] & 0x0ffffffcu, 0);
}

// the padded MAC input again, from AAD || ciphertext and the lengths
static std::vector<uint8_t> mac_input(const Vec& v) {
  std::vector<uint8_t> in(v.aad_ct.begin(), v.aad_ct.begin() + v.aad_len);
  while (in.size() % 16) in.push_back(0);
  in.insert(in.end(), v.aad_ct.begin() + v.aad_len, v.aad_ct.end());
  while (in.size() % 16) in.push_back(0);
  for (uint64_t n : {(uint64_t)v.aad_len, (uint64_t)v.ct_len})
    for (int b = 0; b < 8; ++b) in.push_back((uint8_t)(n >> (8 * b)));
  return in;
}

static Tag serial_p26(const Vec& v, Entered& e) {
  const std::vector<uint8_t> in = mac_input(v);
  const P26m m = p26_mult(clamped_r(v.otk));
  P26 acc{};
  for (size_t o = 0; o < in.size(); o += 16) {
    uint32_t w[4];
    std::memcpy(w, in.data() + o, 16);
    const P26 x = p26_from_words(w[0], w[1], w[2], w[3], 1u);
    for (int q = 0; q < 5; ++q) acc.l[q] += x.l[q];
    p26_mul(acc, m);
  }
  e = entered(acc);
  const uint32_t sk[4] = {v.otk[4], v.otk[5], v.otk[6], v.otk[7]};
  Tag t;
  p26_finish(acc, sk, t.w);
  return t;
}

// mq_resident.hip poly_powers + poly_tag (open form: the packet holds the ciphertext) + p26_from_sums
static Tag resident(const Vec& v, Entered& e) {
  const P26 r = clamped_r(v.otk);
  P26 one{};
  one.l[0] = 1;
  std::vector<P26> pw(64, r);
  auto step = [&](auto src) {  // src(j): the lane whose value lane j multiplies by, or -1 for one
    std::vector<P26> nv = pw;
    for (int j = 0; j < 64; ++j) {
      const int s = src(j);
      p26_mul(nv[j], p26_mult(s < 0 ? one : pw[s]));
    }
    pw = nv;
  };
  for (int sh : {1, 2, 4, 8}) step([&](int j) { return j % 16 >= sh ? j - sh : -1; });  // row_shr
  step([&](int j) { return (j / 16) & 1 ? 16 * (j / 16) - 1 : -1; });                   // row_bcast:15, rows 1, 3
  step([&](int j) { return j >= 32 ? 31 : -1; });                                       // row_bcast:31, rows 2, 3
  Ref want = ref_of(r);
  for (int j = 0; j < 64; ++j) {
    CHECK(ref_eq(ref_of(pw[j]), want));
    want = ref_mul(want, ref_of(r));
  }
  const P26m m64 = p26_mult(pw[63]);
  const uint32_t A = (v.aad_len + 15) >> 4, T = (v.ct_len + 15) >> 4, nb = A + T + 1, K = (nb + 63) / 64;
  const int z = (int)(64 * K) - (int)nb;
  const uint8_t* aad = v.aad_ct.data();
  const uint8_t* ct = aad + v.aad_len;
  uint64_t s[5] = {0, 0, 0, 0, 0};
  for (int lane = 0; lane < 64; ++lane) {
    P26 acc{};
    for (uint32_t k = 0; k < K; ++k) {
      const int i = (int)(64 * k) + 63 - lane - z;
      uint8_t b[16] = {0};
      uint32_t hib = 1;
      if (i < 0) {
        hib = 0;
      } else if (i < (int)A) {
        const int rem = (int)v.aad_len - 16 * i;
        std::memcpy(b, aad + 16 * i, rem < 16 ? rem : 16);
      } else if (i < (int)(A + T)) {
        const uint32_t o = 16u * (uint32_t)(i - (int)A);
        const uint32_t rem = v.ct_len - o;
        std::memcpy(b, ct + o, rem < 16 ? rem : 16);
      } else {
        uint32_t w[4] = {v.aad_len, 0, v.ct_len, 0};
        std::memcpy(b, w, 16);
      }
      uint32_t w[4];
      std::memcpy(w, b, 16);
      const P26 x = p26_from_words(w[0], w[1], w[2], w[3], hib);
      for (int q = 0; q < 5; ++q) acc.l[q] += x.l[q];
      p26_mul(acc, k + 1 < K ? m64 : p26_mult(pw[lane]));
    }
    for (int q = 0; q < 5; ++q) s[q] += acc.l[q];
  }
  for (int pass = 0; pass < 2; ++pass) {  // p26_from_sums
    for (int l = 0; l < 4; ++l) {
      s[l + 1] += s[l] >> 26;
      s[l] &= 0x3ffffff;
    }
    s[0] += (s[4] >> 26) * 5;
    s[4] &= 0x3ffffff;
  }
  P26 h;
  for (int l = 0; l < 5; ++l) h.l[l] = (uint32_t)s[l];
  e = entered(h);
  const uint32_t sk[4] = {v.otk[4], v.otk[5], v.otk[6], v.otk[7]};
  Tag t;
  p26_finish(h, sk, t.w);
  return t;
}

// the vector in a wave of two lane groups: beside a random packet of its geometry (first = true) or
// behind a random packet 200 B longer
template <int G, bool PAIR>
static Tag lane_groups(const Vec& v, bool first, Entered& e) {
  Pkt a{}, b{};
  a.act = b.act = true;
  a.aad_len = b.aad_len = v.aad_len;
  a.ct_len = b.ct_len = v.ct_len;
  (first ? b : a).ct_len += first ? 0 : 200;
  Pkt& mine = first ? a : b;
  Pkt& other = first ? b : a;
  for (int k = 0; k < 4; ++k) {
    mine.rk[k] = v.otk[k], mine.sk[k] = v.otk[4 + k];
    other.rk[k] = (uint32_t)rnd64(), other.sk[k] = (uint32_t)rnd64();
  }
  a.pkt = 3;  // the payload's alignment follows from the AAD length
  b.pkt = a.pkt + a.aad_len + a.ct_len + 16;
  int64_t end = 0;
  uint32_t Kmax = 0;
  for (const Pkt* p : {&a, &b}) {
    const PolyGeom g = poly_geom<G>(p->aad_len, p->ct_len);
    if (g.K > Kmax) Kmax = g.K;
    const int64_t lim = p->pkt + p->aad_len + 16 * (int64_t)g.T + 20;  // the look-ahead bound
    if (lim > end) end = lim;
  }
  std::vector<uint8_t> mem((size_t)end);
  for (auto& x : mem) x = (uint8_t)rnd64();
  std::memcpy(mem.data() + mine.pkt, v.aad_ct.data(), v.aad_ct.size());
  std::vector<std::vector<int64_t>> loads;
  std::vector<P26> sums;
  const std::vector<Pkt> w = {a, b};
  const std::vector<Tag> tags = run_wave<G, G == 8, PAIR>(w, mem, loads, &sums);
  const int at = first ? 0 : 1;
  const Tag ref = serial_tag(w[1 - at], mem);  // the random neighbour against the reference arithmetic
  if (std::memcmp(tags[1 - at].w, ref.w, 16) != 0) ++g_neighbours_wrong;
  e = entered(sums[at]);
  return tags[at];
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  std::FILE* f = std::fopen(argv[1], "r");
  CHECK(f != nullptr);
  std::vector<Vec> vecs;
  {
    std::vector<char> line(1 << 17);
    while (std::fgets(line.data(), (int)line.size(), f)) {
      std::vector<std::string> tok;
      for (char* t = std::strtok(line.data(), " \n"); t; t = std::strtok(nullptr, " \n")) tok.push_back(t);
      if (tok.empty()) continue;
      CHECK(tok.size() == 7);
      Vec v;
      v.name = tok[0];
      v.small = std::atoi(tok[1].c_str());
      const std::vector<uint8_t> otk = unhex(tok[2]), in = unhex(tok[5]), tag = unhex(tok[6]);
      v.aad_len = (uint32_t)std::strtoul(tok[3].c_str(), nullptr, 10);
      v.ct_len = (uint32_t)std::strtoul(tok[4].c_str(), nullptr, 10);
      const size_t apad = (v.aad_len + 15u) / 16 * 16, cpad = (v.ct_len + 15u) / 16 * 16;
      CHECK(otk.size() == 32 && tag.size() == 16 && in.size() == apad + cpad + 16);
      std::memcpy(v.otk, otk.data(), 32);
      std::memcpy(v.want.w, tag.data(), 16);
      v.aad_ct.assign(in.begin(), in.begin() + v.aad_len);
      v.aad_ct.insert(v.aad_ct.end(), in.begin() + apad, in.begin() + apad + v.ct_len);
      vecs.push_back(v);
    }
    std::fclose(f);
  }
  const char* names[6] = {"serial", "g4", "g4p", "g8", "g8p", "resident"};
  size_t ge[6] = {0, 0, 0, 0, 0, 0};
  bool ok = true;
  for (const Vec& v : vecs) {
    std::snprintf(g_what, sizeof g_what, "%s ct %u aad %u", v.name.c_str(), v.ct_len, v.aad_len);
    for (int s = 0; s < 6; ++s) {
      bool match = true, ge_p = false, limb26 = false;
      auto take = [&](const Tag& t, const Entered& e) {
        match = match && std::memcmp(t.w, v.want.w, 16) == 0;
        ge_p = ge_p || e.ge_p;
        limb26 = limb26 || e.limb26;
      };
      Entered e;
      if (s == 0) {
        const Tag t = serial_p26(v, e);
        take(t, e);
      } else if (s == 5) {
        const Tag t = resident(v, e);
        take(t, e);
      } else {
        for (bool first : {true, false}) {
          const Tag t = s == 1   ? lane_groups<4, false>(v, first, e)
                        : s == 2 ? lane_groups<4, true>(v, first, e)
                        : s == 3 ? lane_groups<8, false>(v, first, e)
                                 : lane_groups<8, true>(v, first, e);
          take(t, e);
        }
      }
      ok = ok && match;
      ge[s] += ge_p;
      std::printf("vec %s %u %d %s match=%d ge_p=%d limb26=%d\n", v.name.c_str(), v.ct_len, v.small, names[s], (int)match, (int)ge_p,
                  (int)limb26);
    }
  }
  for (int s = 0; s < 6; ++s) std::printf("schedule %s: %zu of %zu vectors entered p26_finish >= p\n", names[s], ge[s], vecs.size());
  std::printf("random neighbours with a wrong tag: %zu\n", g_neighbours_wrong);
  ok = ok && g_neighbours_wrong == 0;
  std::printf("poly states %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
