// Host check of the two-lane ChaCha20 block (milli_quic_amd/csrc/mq_chacha_pair.h
// chacha20_block_pair), the code seal's keystream pool runs for its header-protection blocks: the
// word type holds both lanes' words side by side and the exchange swaps the two slots, so the very
// template the kernel instantiates with a DPP move runs here in lockstep. Compared with a plain
// RFC 8439 §2.3 block function written out below:
//   1. the RFC 8439 §2.3.2 test vector (also against the RFC's printed words);
//   2. the ChaCha20 header-protection vectors given on the command line (one "key sample mask" line of
//      hex each, from tests/golden/hp_vectors.json: counters 0 and 0xffffffff are among them): the mask
//      is keystream bytes 0..4, counter and nonce are the sample's four little-endian words;
//   3. random keys, counters and nonces.
// Half 0 must return keystream words 0 and 1 (what the kernel uses), half 1 words 2 and 3.
// Built with -fsanitize=address,undefined by tests/test_chacha_pair.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mq_chacha_pair.h"

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "FAILED %s:%d %s [%s]\n", __FILE__, __LINE__, #c, g_what); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)
static char g_what[128] = "";

// both lanes of a pair: slot h is the word on half h
struct Lanes {
  uint32_t v[2];
};
static Lanes operator+(Lanes a, Lanes b) { return Lanes{{a.v[0] + b.v[0], a.v[1] + b.v[1]}}; }
static Lanes operator^(Lanes a, Lanes b) { return Lanes{{a.v[0] ^ b.v[0], a.v[1] ^ b.v[1]}}; }
static Lanes operator|(Lanes a, Lanes b) { return Lanes{{a.v[0] | b.v[0], a.v[1] | b.v[1]}}; }
static Lanes operator<<(Lanes a, int r) { return Lanes{{a.v[0] << r, a.v[1] << r}}; }
static Lanes operator>>(Lanes a, int r) { return Lanes{{a.v[0] >> r, a.v[1] >> r}}; }
struct SwapSlots {
  Lanes operator()(Lanes x) const { return Lanes{{x.v[1], x.v[0]}}; }
};

// RFC 8439 §2.3, as written there
static uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static void qr(uint32_t (&x)[16], int a, int b, int c, int d) {
  x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 16);
  x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 12);
  x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 8);
  x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 7);
}
static void plain_block(const uint32_t (&key)[8], const uint32_t (&in)[4], uint32_t (&out)[16]) {
  uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  for (int i = 0; i < 8; ++i) s[4 + i] = key[i];
  for (int i = 0; i < 4; ++i) s[12 + i] = in[i];
  uint32_t x[16];
  std::memcpy(x, s, sizeof x);
  for (int i = 0; i < 10; ++i) {
    qr(x, 0, 4, 8, 12); qr(x, 1, 5, 9, 13); qr(x, 2, 6, 10, 14); qr(x, 3, 7, 11, 15);
    qr(x, 0, 5, 10, 15); qr(x, 1, 6, 11, 12); qr(x, 2, 7, 8, 13); qr(x, 3, 4, 9, 14);
  }
  for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

// the pair block as the kernel sets it up (mq_chacha.hip cc_pool_seal): half h takes the constants
// 2h, 2h + 1, key words 2h, 2h + 1 and 4 + 2h, 5 + 2h, input words 2h, 2h + 1
static void pair_block(const uint32_t (&key)[8], const uint32_t (&in)[4], uint32_t (&w)[4]) {
  Lanes a[2], b[2], c[2], d[2];
  for (int i = 0; i < 2; ++i)
    for (uint32_t h = 0; h < 2; ++h) {
      a[i].v[h] = mq::cc_pair_const(h, i);
      b[i].v[h] = key[2 * h + i];
      c[i].v[h] = key[4 + 2 * h + i];
      d[i].v[h] = in[2 * h + i];
    }
  Lanes k0, k1;
  mq::chacha20_block_pair(a, b, c, d, SwapSlots{}, k0, k1);
  w[0] = k0.v[0]; w[1] = k1.v[0]; w[2] = k0.v[1]; w[3] = k1.v[1];
}

static uint64_t g_cases;
static void check(const uint32_t (&key)[8], const uint32_t (&in)[4]) {
  uint32_t want[16], got[4];
  plain_block(key, in, want);
  pair_block(key, in, got);
  CHECK(got[0] == want[0] && got[1] == want[1]);  // half 0: what the kernel stores
  CHECK(got[2] == want[2] && got[3] == want[3]);  // half 1
  ++g_cases;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
  out.clear();
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v;
    if (std::sscanf(s.substr(i, 2).c_str(), "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}
static uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

int main(int argc, char** argv) {
  // 1. RFC 8439 §2.3.2: key 00..1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
  {
    std::snprintf(g_what, sizeof g_what, "RFC 8439 2.3.2");
    uint8_t kb[32];
    for (int i = 0; i < 32; ++i) kb[i] = (uint8_t)i;
    uint32_t key[8];
    for (int i = 0; i < 8; ++i) key[i] = le32(kb + 4 * i);
    const uint32_t in[4] = {1u, 0x09000000u, 0x4a000000u, 0u};
    uint32_t got[4];
    pair_block(key, in, got);
    CHECK(got[0] == 0xe4e7f110u && got[1] == 0x15593bd1u && got[2] == 0x1fdd0f50u && got[3] == 0xc47120a3u);
    check(key, in);
  }
  // 2. header-protection vectors
  uint32_t n_hp = 0;
  bool ctr_zero = false, ctr_ones = false;
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "r");
    CHECK(f != nullptr);
    char k[80], s[40], m[16];
    while (std::fscanf(f, "%79s %39s %15s", k, s, m) == 3) {
      std::snprintf(g_what, sizeof g_what, "hp vector %u", n_hp);
      std::vector<uint8_t> kb, sb, mb;
      CHECK(unhex(k, kb) && kb.size() == 32 && unhex(s, sb) && sb.size() == 16 && unhex(m, mb) && mb.size() == 5);
      uint32_t key[8], in[4], got[4];
      for (int i = 0; i < 8; ++i) key[i] = le32(kb.data() + 4 * i);
      for (int i = 0; i < 4; ++i) in[i] = le32(sb.data() + 4 * i);
      pair_block(key, in, got);
      CHECK(got[0] == le32(mb.data()) && (got[1] & 0xffu) == mb[4]);
      check(key, in);
      ctr_zero |= in[0] == 0u;
      ctr_ones |= in[0] == 0xffffffffu;
      ++n_hp;
    }
    std::fclose(f);
    CHECK(n_hp > 0 && ctr_zero && ctr_ones);
  }
  // 3. random keys, counters and nonces; a few words forced to the carry corners
  for (int t = 0; t < 4096; ++t) {
    std::snprintf(g_what, sizeof g_what, "random %d", t);
    uint32_t key[8], in[4];
    for (auto& x : key) x = rnd32();
    for (auto& x : in) x = rnd32();
    if (t % 16 == 1) in[0] = 0xffffffffu;
    if (t % 16 == 2) in[0] = 0u;
    if (t % 16 == 3) key[t / 16 % 8] = 0xffffffffu;
    check(key, in);
  }
  std::printf("chacha pair ok: %llu blocks, %u hp vectors\n", (unsigned long long)g_cases, n_hp);
  return 0;
}
