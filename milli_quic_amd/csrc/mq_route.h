// mq_route.h — the per-datagram arithmetic of mq_batch_route (mq_route.hip) as plain integer code that
// compiles for the device and for the host (tests/csrc/test_route_host.cpp replays it without a GPU):
// datagram classification and CID extraction as decode_dcid does them (reference
// src/packet/decode_dcid.rs:9-37), the first-Initial admission rule (src/connection/recv.rs:275-278,
// RFC 9000 §14.1, §17.2) and the keyed hash of the connection-ID table.
//
// A lane holds the first header bytes of its datagram as little-endian 32-bit words hdr[0..7]
// (byte j of the datagram = bits 8 (j & 3).. of hdr[j >> 2]); bytes it did not load are zero.
#pragma once
#include <stdint.h>

#ifndef MQ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MQ_HD __host__ __device__ __forceinline__
#else
#define MQ_HD inline
#endif
#endif

namespace mq {

constexpr uint32_t kRouteMaxCid = 20;  // RFC 9000 §17.2: a connection ID has at most 20 bytes

// ---- classification (decode_dcid.rs:9-37) ---------------------------------------------------------
enum : uint32_t { kDgMalformed = 0, kDgShort = 1, kDgLong = 2 };
struct DgClass {
  uint32_t kind;     // kDg*
  uint32_t cid_off;  // 1 (short header) or 6 (long header)
  uint32_t cid_len;  // <= 20
};

// len: the datagram's length; w0, w1: its bytes 0..7 (those below len). decode_dcid -> None, and a
// long-header DCID length over 20 (no table key is longer), are kDgMalformed.
MQ_HD DgClass route_classify(uint32_t len, uint32_t w0, uint32_t w1, uint32_t short_dcid_len) {
  DgClass c = {kDgMalformed, 0, 0};
  if (len == 0) return c;  // datagram.is_empty()
  if (w0 & 0x80) {         // long header: the DCID length is byte 5, the DCID starts at byte 6
    if (len < 6) return c;
    const uint32_t L = (w1 >> 8) & 0xFF;
    if (len < 6 + L) return c;
    if (L > kRouteMaxCid) return c;
    c.kind = kDgLong, c.cid_off = 6, c.cid_len = L;
  } else {  // short header: the DCID starts at byte 1, its length comes from the server's configuration
    if (len < 1 + short_dcid_len) return c;
    c.kind = kDgShort, c.cid_off = 1, c.cid_len = short_dcid_len;
  }
  return c;
}

// A datagram whose CID is in no table may open a new connection when it starts with an Initial
// packet (long header, type bits 0) of a non-zero version (0 is Version Negotiation, §17.2.1) and is
// at least min_initial_len bytes long (§14.1: 1200; 0 = no check).
MQ_HD bool route_admissible(uint32_t kind, uint32_t w0, uint32_t w1, uint32_t len, uint32_t min_initial_len) {
  const uint32_t version = (w0 >> 8) | (w1 << 24);  // bytes 1..4 (any byte order: only zero matters)
  return kind == kDgLong && (w0 & 0x30) == 0 && version != 0 && len >= min_initial_len;
}

// ---- table key: the CID zero-padded to 20 bytes, and its length ------------------------------------
struct CidKey {
  uint64_t w0, w1;  // CID bytes 0..7, 8..15
  uint32_t w2;      // CID bytes 16..19
  uint32_t len;
};

// o[q] = CID bytes 4q..4q+3, whatever follows the CID still in them: zero the bytes from len on
MQ_HD CidKey route_key_words(const uint32_t (&o)[5], uint32_t len) {
  uint32_t m[5];
  for (int q = 0; q < 5; ++q) {
    const int keep = (int)len - 4 * q;
    m[q] = keep >= 4 ? o[q] : (keep <= 0 ? 0u : o[q] & ((1u << (8 * keep)) - 1u));
  }
  CidKey k;
  k.w0 = m[0] | (uint64_t)m[1] << 32;
  k.w1 = m[2] | (uint64_t)m[3] << 32;
  k.w2 = m[4];
  k.len = len;
  return k;
}

// From the header words: the CID starts at byte 6 (long_hdr) or byte 1.
MQ_HD CidKey route_key(const uint32_t (&hdr)[8], bool long_hdr, uint32_t cid_len) {
  uint32_t o[5];
  for (int q = 0; q < 5; ++q) {
    const uint32_t lo = long_hdr ? hdr[q + 1] : hdr[q], hi = long_hdr ? hdr[q + 2] : hdr[q + 1];
    o[q] = long_hdr ? (lo >> 16) | (hi << 16) : (lo >> 8) | (hi << 24);
  }
  return route_key_words(o, cid_len);
}

MQ_HD bool route_key_equal(const CidKey& a, const CidKey& b) {
  return a.len == b.len && a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2;
}

// ---- hash: SipHash-1-3 under the table's seed ------------------------------------------------------
// The DCID of an Initial is chosen by the peer, so an unkeyed hash would let it build long probe
// chains. Message: the three 64-bit words of the padded CID, the length in the top byte of the last
// one (as SipHash places the message length), so the padding never aliases 00 with the empty CID.
MQ_HD uint64_t route_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
struct SipState { uint64_t v0, v1, v2, v3; };
MQ_HD void sip_round(SipState& s) {
  s.v0 += s.v1; s.v1 = route_rotl(s.v1, 13); s.v1 ^= s.v0; s.v0 = route_rotl(s.v0, 32);
  s.v2 += s.v3; s.v3 = route_rotl(s.v3, 16); s.v3 ^= s.v2;
  s.v0 += s.v3; s.v3 = route_rotl(s.v3, 21); s.v3 ^= s.v0;
  s.v2 += s.v1; s.v1 = route_rotl(s.v1, 17); s.v1 ^= s.v2; s.v2 = route_rotl(s.v2, 32);
}
MQ_HD uint64_t route_sip13(uint64_t k0, uint64_t k1, const CidKey& k) {
  SipState s = {k0 ^ 0x736f6d6570736575ull, k1 ^ 0x646f72616e646f6dull, k0 ^ 0x6c7967656e657261ull,
                k1 ^ 0x7465646279746573ull};
  const uint64_t m[3] = {k.w0, k.w1, (uint64_t)k.w2 | (uint64_t)k.len << 56};
  for (int q = 0; q < 3; ++q) {
    s.v3 ^= m[q];
    sip_round(s);
    s.v0 ^= m[q];
  }
  s.v2 ^= 0xff;
  sip_round(s);
  sip_round(s);
  sip_round(s);
  return s.v0 ^ s.v1 ^ s.v2 ^ s.v3;
}

// The 64-bit word a slot is claimed with: 59 hash bits above the CID length. A length is at most 20,
// so the two values with length bits 31 and 30 are free for "empty" and "tombstone", and words of
// different lengths never compare equal. hash_mask keeps the low bits of the hash
// (mq_debug_cid_table_hash_bits; all 59 in the product).
constexpr uint32_t kCidHashBits = 59;
constexpr uint64_t kCidEmpty = ~0ull, kCidTomb = ~0ull - 1;
MQ_HD uint64_t route_tag(uint64_t k0, uint64_t k1, uint64_t hash_mask, const CidKey& k) {
  return ((route_sip13(k0, k1, k) & hash_mask) << 5) | k.len;
}
MQ_HD uint32_t route_tag_pos(uint64_t tag, uint32_t slot_mask) { return (uint32_t)(tag >> 5) & slot_mask; }

// ---- table layout (mq_route.hip; the host side passes CidTableDev to the launches) -----------------
struct alignas(16) CidSlot {
  uint64_t tag;
  uint64_t w0, w1;
  uint32_t w2;
  uint32_t conn;
};
static_assert(sizeof(CidSlot) == 32, "CidSlot layout");

struct CidTableDev {
  CidSlot* slots;
  uint32_t* ctr;  // [0] live entries, [1] tombstones
  uint32_t slot_mask, capacity;
  uint64_t k0, k1, hash_mask;
};

}  // namespace mq
