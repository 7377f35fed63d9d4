// mq_frames.h — the per-frame arithmetic of mq_batch_frames (mq_frames.hip) as plain integer code that
// compiles for the device and for the host (tests/csrc/test_frames_host.cpp replays it without a GPU):
// read_varint (reference src/frame/mod.rs:183-190 over src/varint.rs:31-67), read_bytes (:200-207) and
// frame::decode (:228-461), item by item and in its order of checks.
//
// The payload is seen through a byte-fetch functor: fetch(p) returns byte p of the payload, and is only
// ever called with p < len. Positions are relative to the payload start; the reference's
// decode(&payload[pos..]) sees the same bytes with its own zero at `start`, so "the rest of the buffer"
// is len - pos here. Frame data (CRYPTO, STREAM, NEW_TOKEN, reason, CID, token, PATH_* bytes) is
// skipped by its length and never fetched.
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

constexpr uint64_t kFrameMaxType = 0x1e;  // HANDSHAKE_DONE: every value above is FrameEncodingError
constexpr uint32_t kFrameMaxCid = 20;     // NEW_CONNECTION_ID (mod.rs:396-398)
// the payload lengths the records can describe (uint16 positions and counts)
constexpr uint32_t kFrameMaxPayload = 0xFFFF;

struct FrameFields {  // one decoded frame: what mq_frame holds beside pkt, pos and level
  uint32_t type;      // the decoded type value, 0x00..0x1e
  uint32_t data_pos, data_len, aux;
  uint64_t v0, v1, v2, v3;
};

// read_varint: false = FrameEncodingError (pos >= len, or the encoding runs past len)
template <class Fetch>
MQ_HD bool frame_varint(Fetch& fetch, uint32_t len, uint32_t& pos, uint64_t& out) {
  if (pos >= len) return false;
  const uint32_t b0 = fetch(pos);
  const uint32_t n = 1u << (b0 >> 6);
  if (len - pos < n) return false;
  uint64_t v = b0 & 0x3f;
  for (uint32_t k = 1; k < n; ++k) v = v << 8 | (uint64_t)fetch(pos + k);
  pos += n;
  out = v;
  return true;
}

// read_bytes: the 64-bit length against the bytes left (pos <= len always holds here)
MQ_HD bool frame_bytes(uint32_t len, uint32_t& pos, uint64_t n, uint32_t& at, uint32_t& got) {
  if ((uint64_t)(len - pos) < n) return false;
  at = pos;
  got = (uint32_t)n;
  pos += (uint32_t)n;
  return true;
}

// frame::decode on payload[start, len): true with the fields and the position behind the frame, or
// false = Err(FrameEncodingError). start < len (dispatch_frames' loop condition).
template <class Fetch>
MQ_HD bool frame_decode(Fetch& fetch, uint32_t start, uint32_t len, FrameFields& f, uint32_t& next) {
  uint32_t pos = start;
  uint64_t type;
  f.type = 0, f.data_pos = 0, f.data_len = 0, f.aux = 0;
  f.v0 = 0, f.v1 = 0, f.v2 = 0, f.v3 = 0;
  if (!frame_varint(fetch, len, pos, type)) return false;
  if (type > kFrameMaxType) return false;
  const uint32_t t = (uint32_t)type;
  f.type = t;
  if (t == 0x02 || t == 0x03) {  // ACK: four fields, ack_range_count (gap, range) pairs, ECN counts
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if (!frame_varint(fetch, len, pos, f.v1)) return false;
    if (!frame_varint(fetch, len, pos, f.v2)) return false;
    if (!frame_varint(fetch, len, pos, f.v3)) return false;
    f.data_pos = pos;
    uint64_t skip;
    for (uint64_t k = 0; k < f.v2; ++k) {  // each pair takes >= 2 bytes: at most (len - pos) / 2 rounds
      if (!frame_varint(fetch, len, pos, skip)) return false;
      if (!frame_varint(fetch, len, pos, skip)) return false;
    }
    f.data_len = pos - f.data_pos;
    if (t == 0x03) {
      f.aux = pos;
      for (int k = 0; k < 3; ++k)
        if (!frame_varint(fetch, len, pos, skip)) return false;
    }
  } else if (t == 0x04) {  // RESET_STREAM
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if (!frame_varint(fetch, len, pos, f.v1)) return false;
    if (!frame_varint(fetch, len, pos, f.v2)) return false;
  } else if (t == 0x05 || t == 0x11 || t == 0x15) {  // STOP_SENDING, MAX_STREAM_DATA, STREAM_DATA_BLOCKED
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if (!frame_varint(fetch, len, pos, f.v1)) return false;
  } else if (t == 0x06) {  // CRYPTO
    uint64_t n;
    if (!frame_varint(fetch, len, pos, f.v1)) return false;
    if (!frame_varint(fetch, len, pos, n)) return false;
    if (!frame_bytes(len, pos, n, f.data_pos, f.data_len)) return false;
  } else if (t == 0x07) {  // NEW_TOKEN
    uint64_t n;
    if (!frame_varint(fetch, len, pos, n)) return false;
    if (!frame_bytes(len, pos, n, f.data_pos, f.data_len)) return false;
  } else if (t >= 0x08 && t <= 0x0f) {  // STREAM: OFF 0x04, LEN 0x02, FIN 0x01
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if ((t & 0x04) && !frame_varint(fetch, len, pos, f.v1)) return false;
    if (t & 0x02) {
      uint64_t n;
      if (!frame_varint(fetch, len, pos, n)) return false;
      if (!frame_bytes(len, pos, n, f.data_pos, f.data_len)) return false;
    } else {  // the data extends to the end of the packet
      f.data_pos = pos, f.data_len = len - pos;
      pos = len;
    }
  } else if (t == 0x10 || t == 0x12 || t == 0x13 || t == 0x14 || t == 0x16 || t == 0x17 || t == 0x19) {
    if (!frame_varint(fetch, len, pos, f.v0)) return false;  // one value
  } else if (t == 0x18) {  // NEW_CONNECTION_ID
    uint64_t n;
    uint32_t tok_len;
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if (!frame_varint(fetch, len, pos, f.v1)) return false;
    if (!frame_varint(fetch, len, pos, n)) return false;
    if (n > kFrameMaxCid) return false;
    if (!frame_bytes(len, pos, n, f.data_pos, f.data_len)) return false;
    if (!frame_bytes(len, pos, 16, f.aux, tok_len)) return false;
  } else if (t == 0x1a || t == 0x1b) {  // PATH_CHALLENGE, PATH_RESPONSE
    if (!frame_bytes(len, pos, 8, f.data_pos, f.data_len)) return false;
  } else if (t == 0x1c || t == 0x1d) {  // CONNECTION_CLOSE (0x1d: no frame_type field)
    uint64_t n;
    if (!frame_varint(fetch, len, pos, f.v0)) return false;
    if (t == 0x1c && !frame_varint(fetch, len, pos, f.v1)) return false;
    if (!frame_varint(fetch, len, pos, n)) return false;
    if (!frame_bytes(len, pos, n, f.data_pos, f.data_len)) return false;
  }  // 0x00 PADDING, 0x01 PING, 0x1e HANDSHAKE_DONE: the type alone
  next = pos;
  return true;
}

// dispatch_frames' classification (recv.rs:533-539): everything but PADDING and ACK elicits an ACK
MQ_HD bool frame_ack_eliciting(uint32_t type) { return type != 0x00 && type != 0x02 && type != 0x03; }
MQ_HD bool frame_is_close(uint32_t type) { return type == 0x1c || type == 0x1d; }

}  // namespace mq
