// Host replay of milli_quic_amd/csrc/mq_route.h — the classification, CID extraction, admission rule
// and hash that the routing kernels (mq_route.hip) call — against a table of expected outcomes
// written by tests/test_route.py from its Python model. Built with AddressSanitizer and UBSan: every
// datagram sits in a heap buffer of exactly its length, and the header words are gathered the way the
// kernel gathers them (16 bytes at once where the datagram has them, else byte by byte), so a load
// at or past the datagram's end is reported.
//
// Input lines:
//   D <datagram hex | -> <short_dcid_len> <min_initial_len> <M | cid hex | -> <admissible 0|1>
//   H <seed hex (32 digits)> <cid hex | ->      -> prints "H <cid> <siphash hex>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../milli_quic_amd/csrc/mq_route.h"

using namespace mq;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}

// the kernel's load_hdr16: bytes [lo, hi) of the datagram into four words
static void load_hdr16(const uint8_t* p, uint32_t len, uint32_t lo, uint32_t hi, uint32_t* h) {
  uint8_t b[16] = {0};
  if (len >= lo + 16) std::memcpy(b, p + lo, 16);
  else
    for (uint32_t j = lo; j < hi; ++j) b[j - lo] = p[j];
  for (int q = 0; q < 4; ++q) h[q] = b[4 * q] | b[4 * q + 1] << 8 | b[4 * q + 2] << 16 | (uint32_t)b[4 * q + 3] << 24;
}

static CidKey key_of(const std::vector<uint8_t>& cid) {
  uint8_t b[20] = {0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA,
                   0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA, 0xAA};  // padding must not matter
  if (!cid.empty()) std::memcpy(b, cid.data(), cid.size());
  uint32_t o[5];
  for (int q = 0; q < 5; ++q) o[q] = b[4 * q] | b[4 * q + 1] << 8 | b[4 * q + 2] << 16 | (uint32_t)b[4 * q + 3] << 24;
  return route_key_words(o, (uint32_t)cid.size());
}

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "line %d: %s failed (input line %zu)\n", __LINE__, #c, lineno); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  size_t lineno = 0, n_d = 0;
  while (std::getline(in, line)) {
    ++lineno;
    std::istringstream ss(line);
    std::string kind;
    ss >> kind;
    if (kind == "D") {
      std::string dg_hex, want;
      uint32_t sdl, min_len, adm;
      ss >> dg_hex >> sdl >> min_len >> want >> adm;
      const std::vector<uint8_t> v = unhex(dg_hex);
      const uint32_t len = (uint32_t)v.size();
      uint8_t* p = (uint8_t*)std::malloc(len ? len : 1);  // exactly the datagram (ASan watches its end)
      if (len) std::memcpy(p, v.data(), len);
      uint32_t hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool malformed = len == 0;
      DgClass c = {kDgMalformed, 0, 0};
      CidKey k = {};
      if (len) {
        load_hdr16(p, len, 0, len < 16 ? len : 16, hdr);
        c = route_classify(len, hdr[0], hdr[1], sdl);
        malformed = c.kind == kDgMalformed;
      }
      if (!malformed) {
        const uint32_t need = c.cid_off + c.cid_len;
        CHECK(need <= len && need <= 26);
        if (need > 16) load_hdr16(p, len, 16, need, hdr + 4);
        k = route_key(hdr, c.kind == kDgLong, c.cid_len);
      }
      if (want == "M") {
        CHECK(malformed);
      } else {
        CHECK(!malformed);
        const std::vector<uint8_t> cid = unhex(want);
        CHECK(c.cid_len == cid.size());
        CHECK(route_key_equal(k, key_of(cid)));
        CHECK(cid.empty() || std::memcmp(p + c.cid_off, cid.data(), cid.size()) == 0);
        CHECK(route_admissible(c.kind, hdr[0], hdr[1], len, min_len) == (adm != 0));
      }
      std::free(p);
      ++n_d;
    } else if (kind == "H") {
      std::string seed_hex, cid_hex;
      ss >> seed_hex >> cid_hex;
      const std::vector<uint8_t> seed = unhex(seed_hex), cid = unhex(cid_hex);
      CHECK(seed.size() == 16);
      uint64_t k0, k1;
      std::memcpy(&k0, seed.data(), 8);
      std::memcpy(&k1, seed.data() + 8, 8);
      std::printf("H %s %016llx\n", cid_hex.c_str(), (unsigned long long)route_sip13(k0, k1, key_of(cid)));
    }
  }

  // hash and tag properties
  lineno = 0;
  const uint64_t k0 = 0x0706050403020100ull, k1 = 0x0f0e0d0c0b0a0908ull, all = (1ull << kCidHashBits) - 1;
  for (uint32_t len = 0; len <= 20; ++len) {
    std::vector<uint8_t> a(len, 0), b(len, 0);
    for (uint32_t j = 0; j < len; ++j) a[j] = b[j] = (uint8_t)(17 * j + len);
    CHECK(route_sip13(k0, k1, key_of(a)) == route_sip13(k0, k1, key_of(b)));  // equal CIDs, equal hash
    CHECK(route_tag(k0, k1, all, key_of(a)) == route_tag(k0, k1, all, key_of(b)));
    // the same bytes under another length (zero padding): 00..00 of length len vs len + 1, and the
    // empty CID vs 00
    if (len < 20) {
      const std::vector<uint8_t> z0(len, 0), z1(len + 1, 0);
      CHECK(!route_key_equal(key_of(z0), key_of(z1)));
      CHECK(route_sip13(k0, k1, key_of(z0)) != route_sip13(k0, k1, key_of(z1)));
      for (uint32_t bits = 1; bits <= 59; bits += 29)  // tags differ whatever the hash mask keeps
        CHECK(route_tag(k0, k1, (1ull << bits) - 1, key_of(z0)) != route_tag(k0, k1, (1ull << bits) - 1, key_of(z1)));
    }
    const uint64_t tag = route_tag(k0, k1, all, key_of(a));
    CHECK(tag != kCidEmpty && tag != kCidTomb && (tag & 31) == len);
    CHECK(route_sip13(k0 ^ 1, k1, key_of(a)) != route_sip13(k0, k1, key_of(a)));  // the seed keys it
  }
  CHECK((kCidEmpty & 31) > 20 && (kCidTomb & 31) > 20);
  std::printf("route host ok %zu\n", n_d);
  return 0;
}
