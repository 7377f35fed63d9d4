// mq_acks.h — the per-tracker arithmetic of mq_batch_acks (mq_acks.hip) as plain integer code that
// compiles for the device and for the host (tests/csrc/test_acks_host.cpp replays it without a GPU):
// RecvPnTracker::record and insert_range (reference src/connection/mod.rs:224-296), the run operation
// that stands for recording an ascending run of packet numbers, the fields of build_ack_frame
// (src/connection/transmit.rs:321-380) and the ACK encoding (src/frame/mod.rs:482-508).
//
// A tracker is the reference's heapless::Vec<(u64, u64), 32>: at most 32 inclusive ranges, ascending,
// non-overlapping and non-adjacent. The functions below state every operation on the array form
// (AckRanges). mq_acks.hip keeps one range per lane instead; it takes the predicates, the field and
// varint arithmetic and the frame layout from here and replaces the loops over the array by ballots
// and lane shifts. Both forms assume a tracker that satisfies the invariant and packet numbers below
// 2^62; with other content they stay inside the 32 ranges and the frame slot, and nothing more is said.
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

constexpr uint32_t kAckRanges = 32;        // MQ_PN_TRACKER_RANGES
constexpr uint32_t kAckFrameMax = 528;     // MQ_ACK_FRAME_MAX: the largest frame has 515 bytes
constexpr uint32_t kAckFrameLongest = 515;  // 1 + 8 + 1 + 1 + 8 + 31 * 16

struct AckRanges {  // mq_pn_tracker without its reserved words
  uint32_t n;
  uint64_t r[kAckRanges][2];  // (start, end)
};

// ---- the three questions record() asks of every range (mod.rs:233-246) -----------------------------
MQ_HD bool ack_contains(uint64_t start, uint64_t end, uint64_t pn) { return pn >= start && pn <= end; }
MQ_HD bool ack_extends_up(uint64_t end, uint64_t pn) { return pn == end + 1; }
MQ_HD bool ack_extends_down(uint64_t start, uint64_t pn) { return pn + 1 == start; }

MQ_HD void ack_remove(AckRanges& t, uint32_t at) {  // at < t.n
  for (uint32_t i = at; i + 1 < t.n; ++i) t.r[i][0] = t.r[i + 1][0], t.r[i][1] = t.r[i + 1][1];
  --t.n;
}

// insert_range (mod.rs:281-295): in front of the first range whose start is above `start`. t.n < 32.
MQ_HD uint32_t ack_insert(AckRanges& t, uint64_t start, uint64_t end) {
  uint32_t pos = t.n;
  for (uint32_t i = 0; i < t.n; ++i) {
    if (t.r[i][0] > start) {
      pos = i;
      break;
    }
  }
  for (uint32_t i = t.n; i > pos; --i) t.r[i][0] = t.r[i - 1][0], t.r[i][1] = t.r[i - 1][1];
  t.r[pos][0] = start, t.r[pos][1] = end;
  ++t.n;
  return pos;
}

// RecvPnTracker::record (mod.rs:224-278). Returns the index of the range that holds pn afterwards.
MQ_HD uint32_t ack_record(AckRanges& t, uint64_t pn) {
  uint32_t left = kAckRanges, right = kAckRanges;
  for (uint32_t i = 0; i < t.n; ++i) {
    if (ack_contains(t.r[i][0], t.r[i][1], pn)) return i;  // already tracked
    if (ack_extends_up(t.r[i][1], pn)) left = i;
    if (ack_extends_down(t.r[i][0], pn)) right = i;
  }
  if (left < kAckRanges && right < kAckRanges) {  // pn bridges two ranges
    const uint64_t s = t.r[left][0], e = t.r[right][1];
    const uint32_t hi = left < right ? right : left, lo = left < right ? left : right;
    ack_remove(t, hi);
    ack_remove(t, lo);
    return ack_insert(t, s, e);
  }
  if (left < kAckRanges) {
    t.r[left][1] = pn;
    return left;
  }
  if (right < kAckRanges) {
    t.r[right][0] = pn;
    return right;
  }
  if (t.n == kAckRanges) ack_remove(t, 0);  // full: the lowest range goes first, wherever pn lies
  return ack_insert(t, pn, pn);
}

// Recording first, first + 1, ..., last in turn: record(first), then the range that holds `first` rises
// to max(end, last) and takes in every following range that starts at or below its end + 1. After the
// first packet number none of the run can stand alone, so nothing is dropped inside a run.
MQ_HD void ack_record_run(AckRanges& t, uint64_t first, uint64_t last) {
  const uint32_t at = ack_record(t, first);
  if (last > t.r[at][1]) t.r[at][1] = last;
  while (at + 1 < t.n && t.r[at + 1][0] <= t.r[at][1] + 1) {
    if (t.r[at + 1][1] > t.r[at][1]) t.r[at][1] = t.r[at + 1][1];
    ack_remove(t, at + 1);
  }
}

// ---- ACK frame --------------------------------------------------------------------------------------
// shortest-form varint (src/varint.rs encode_varint); v < 2^62 (larger values keep their low 62 bits)
MQ_HD uint32_t ack_varint_len(uint64_t v) { return v < 64 ? 1u : v < 16384 ? 2u : v < (1ull << 30) ? 4u : 8u; }
template <class Put>
MQ_HD uint32_t ack_varint_put(Put& put, uint32_t pos, uint64_t v) {
  const uint32_t n = ack_varint_len(v);
  const uint32_t tag = n == 1 ? 0u : n == 2 ? 0x40u : n == 4 ? 0x80u : 0xC0u;
  for (uint32_t k = 0; k < n; ++k) {
    uint32_t b = (uint32_t)(v >> (8 * (n - 1 - k))) & 0xFFu;
    if (k == 0) b = (b & 0x3Fu) | tag;
    put(pos + k, b);
  }
  return n;
}

// the (gap, range) pair of a range below the top one (transmit.rs:347-352): next_start is the start of
// the range above it
MQ_HD uint64_t ack_gap(uint64_t next_start, uint64_t end) { return next_start - end - 2; }
MQ_HD uint64_t ack_len(uint64_t start, uint64_t end) { return end - start; }
MQ_HD uint32_t ack_pair_bytes(uint64_t start, uint64_t end, uint64_t next_start) {
  return ack_varint_len(ack_gap(next_start, end)) + ack_varint_len(ack_len(start, end));
}
template <class Put>
MQ_HD uint32_t ack_pair_put(Put& put, uint32_t pos, uint64_t start, uint64_t end, uint64_t next_start) {
  const uint32_t a = ack_varint_put(put, pos, ack_gap(next_start, end));
  return a + ack_varint_put(put, pos + a, ack_len(start, end));
}

// type 0x02, largest_ack, ack_delay = 0, ack_range_count = n - 1, first_ack_range (mod.rs:482-501)
MQ_HD uint32_t ack_head_bytes(uint32_t n, uint64_t top_start, uint64_t top_end) {
  return 1u + ack_varint_len(top_end) + 1u + ack_varint_len(n - 1) + ack_varint_len(ack_len(top_start, top_end));
}
template <class Put>
MQ_HD uint32_t ack_head_put(Put& put, uint32_t n, uint64_t top_start, uint64_t top_end) {
  uint32_t pos = 0;
  put(pos++, 0x02u);
  pos += ack_varint_put(put, pos, top_end);
  put(pos++, 0x00u);
  pos += ack_varint_put(put, pos, n - 1);
  pos += ack_varint_put(put, pos, ack_len(top_start, top_end));
  return pos;
}

// build_ack_frame over the array form: the frame's length (at most kAckFrameLongest), 0 for an empty
// tracker (None)
template <class Put>
MQ_HD uint32_t ack_frame_put(Put& put, const AckRanges& t) {
  if (t.n == 0) return 0;
  uint32_t pos = ack_head_put(put, t.n, t.r[t.n - 1][0], t.r[t.n - 1][1]);
  for (uint32_t i = t.n - 1; i-- > 0;) pos += ack_pair_put(put, pos, t.r[i][0], t.r[i][1], t.r[i + 1][0]);
  return pos;
}

}  // namespace mq
