// mq_recovery.h — the arithmetic of mq_batch_sent and mq_batch_recovery (mq_recovery.hip) as plain
// integer code that compiles for the device and for the host (tests/csrc/test_recovery_host.cpp replays
// it without a GPU): SentPacketTracker (reference src/transport/recovery.rs:49-171), LossDetector
// (src/transport/loss.rs:53-288) and CongestionController (src/transport/congestion.rs:23-137) as they
// are driven by build_*_packet (src/connection/transmit.rs:610-619, 743-752) and by Frame::Ack and
// Frame::HandshakeDone in dispatch_frame (src/connection/recv.rs:563-612, 692-704).
//
// The scalar state of a connection is RecState; everything that touches it alone (update_rtt, the two
// congestion steps, the loss delay, next_timeout, drop_space) is stated once and used by both forms. The
// tracker's 128 entries are an array here (RecConn, the functions rec_apply_*): the literal loops of the
// reference. mq_recovery.hip keeps two entries per lane of a wave instead; it takes the per-entry
// predicates and the walk over the ACK ranges from here and replaces the loops over the array by
// ballots and ranks. Times below 2^56 and windows below 2^48 keep every intermediate value inside 64
// bits; with other content both forms stay inside the 128 entries and nothing more is said.
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

constexpr uint32_t kSentSlots = 128;      // MQ_SENT_SLOTS
constexpr uint32_t kRecPairs = 16;        // heapless::Vec<(u64, u64), 16> in dispatch_frame
constexpr uint32_t kRecNewlyAcked = 32;   // AckResult::newly_acked
constexpr uint32_t kRecLostMax = 64;      // lost_pns of detect_lost_packets
constexpr uint64_t kRecNone = ~0ull;      // a timeout that is None; min_rtt before the first sample
constexpr uint32_t kSentUsed = 0x01, kSentAckEliciting = 0x02, kSentInFlight = 0x04;  // MQ_SENT_*
constexpr uint32_t kRecConfirmed = 0x01;  // MQ_RECOVERY_CONFIRMED
constexpr uint32_t kEvtRtt = 0x01, kEvtRangesCut = 0x02, kEvtRangesBroke = 0x04, kEvtLostCut = 0x08;  // MQ_ACKEVT_*
// mq_conn_recovery.have: bit l of each group of three is level l
constexpr uint32_t kHaveLargest = 1u << 0, kHaveLastSent = 1u << 3, kHaveLossTime = 1u << 6;
constexpr uint32_t kHaveSrtt = 1u << 9, kHaveRecoveryStart = 1u << 10;
constexpr uint64_t kRecInitialRtt = 333000, kRecGranularity = 1000, kRecPacketThreshold = 3;

struct RecState {  // mq_conn_recovery without its entries
  uint64_t largest_acked[3], last_sent[3], loss_time[3];
  uint64_t srtt, rttvar, min_rtt, latest_rtt, max_ack_delay;
  uint64_t cwnd, ssthresh, in_flight, recovery_start, persistent_threshold, mds, min_window;
  uint32_t have, pto_count, count, flags;
};

// a[i] for i < 3 without an indexed access: the device form keeps the state in registers
MQ_HD uint64_t rec_get3(const uint64_t (&a)[3], uint32_t i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; }
MQ_HD void rec_set3(uint64_t (&a)[3], uint32_t i, uint64_t v) {
  a[0] = i == 0 ? v : a[0];
  a[1] = i == 1 ? v : a[1];
  a[2] = i == 2 ? v : a[2];
}
MQ_HD uint64_t rec_sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }

// ---- an entry: pn, time_sent and the word size | level << 16 | flags << 24 ----------------------------
MQ_HD uint32_t sent_meta(uint32_t size, uint32_t level, uint32_t flags) {
  return (size & 0xFFFFu) | (level & 0xFFu) << 16 | (flags & 0xFFu) << 24;
}
MQ_HD uint32_t sent_size(uint32_t meta) { return meta & 0xFFFFu; }
MQ_HD uint32_t sent_level(uint32_t meta) { return (meta >> 16) & 0xFFu; }
MQ_HD bool sent_used(uint32_t meta) { return (meta >> 24 & kSentUsed) != 0; }
MQ_HD bool sent_is(uint32_t meta, uint32_t level) { return sent_used(meta) && sent_level(meta) == level; }
// has_ack_eliciting_in_flight (recovery.rs:179-184), for any level
MQ_HD bool sent_counts_for_pto(uint32_t meta) {
  const uint32_t all = kSentUsed | kSentAckEliciting | kSentInFlight;
  return (meta >> 24 & all) == all;
}
MQ_HD uint32_t sent_new_meta(uint32_t pkt_len, uint32_t level) {  // transmit.rs:610-617: `total_pkt_len as u16`
  return sent_meta(pkt_len, level, kSentUsed | kSentAckEliciting | kSentInFlight);
}

// What a row holds for an Option that is None: 0. Applied when a connection is written back.
MQ_HD void rec_normalise(RecState& s) {
  for (uint32_t l = 0; l < 3; ++l) {
    if (!(s.have & (kHaveLargest << l))) s.largest_acked[l] = 0;
    if (!(s.have & (kHaveLastSent << l))) s.last_sent[l] = 0;
    if (!(s.have & (kHaveLossTime << l))) s.loss_time[l] = 0;
  }
  if (!(s.have & kHaveSrtt)) s.srtt = 0;
  if (!(s.have & kHaveRecoveryStart)) s.recovery_start = 0;
}

// ---- LossDetector -----------------------------------------------------------------------------------------
// drop_space (loss.rs:283-288)
MQ_HD void rec_drop_space(RecState& s, uint32_t level) {
  s.have &= ~((kHaveLargest | kHaveLastSent | kHaveLossTime) << level);
  rec_set3(s.largest_acked, level, 0);
  rec_set3(s.last_sent, level, 0);
  rec_set3(s.loss_time, level, 0);
}
// on_ack_eliciting_sent (loss.rs:278-280) and CongestionController::on_packet_sent (congestion.rs:48-50)
MQ_HD void rec_on_sent(RecState& s, uint32_t level, uint64_t now, uint32_t pkt_len) {
  rec_set3(s.last_sent, level, now);
  s.have |= kHaveLastSent << level;
  s.in_flight += pkt_len;
}
// update_rtt (loss.rs:68-101)
MQ_HD void rec_update_rtt(RecState& s, uint64_t latest, uint64_t ack_delay, bool confirmed) {
  s.latest_rtt = latest;
  if (s.min_rtt == kRecNone || latest < s.min_rtt) s.min_rtt = latest;
  if (!(s.have & kHaveSrtt)) {
    s.have |= kHaveSrtt;
    s.srtt = latest;
    s.rttvar = latest / 2;
    return;
  }
  uint64_t adjusted = latest;
  if (confirmed) {
    const uint64_t capped = ack_delay < s.max_ack_delay ? ack_delay : s.max_ack_delay;
    if (latest > s.min_rtt + capped) adjusted = latest - capped;
  }
  const uint64_t sample = s.srtt > adjusted ? s.srtt - adjusted : adjusted - s.srtt;
  s.rttvar = (3 * s.rttvar + sample) / 4;
  s.srtt = (7 * s.srtt + adjusted) / 8;
}
// on_ack_received (loss.rs:104-113); returns largest_acked[level] afterwards
MQ_HD uint64_t rec_on_largest_acked(RecState& s, uint32_t level, uint64_t largest) {
  const uint64_t prev = rec_get3(s.largest_acked, level);
  const uint64_t now = (s.have & (kHaveLargest << level)) && prev >= largest ? prev : largest;
  rec_set3(s.largest_acked, level, now);
  s.have |= kHaveLargest << level;
  return now;
}
MQ_HD uint64_t rec_smoothed_rtt(const RecState& s) { return (s.have & kHaveSrtt) ? s.srtt : kRecInitialRtt; }
// the loss delay of detect_lost_packets (loss.rs:130-131)
MQ_HD uint64_t rec_loss_delay(const RecState& s) {
  const uint64_t srtt = rec_smoothed_rtt(s);
  const uint64_t base = srtt > s.latest_rtt ? srtt : s.latest_rtt;
  const uint64_t d = base * 9 / 8;
  return d > kRecGranularity ? d : kRecGranularity;
}
// what the scan of detect_lost_packets does with an entry of the level (loss.rs:139-167)
constexpr uint32_t kLossSkip = 0, kLossLost = 1, kLossWait = 2;
MQ_HD uint32_t rec_loss_class(uint64_t pn, uint64_t time_sent, uint64_t largest_acked, uint64_t lost_send_time) {
  if (pn > largest_acked) return kLossSkip;
  if (largest_acked >= pn + kRecPacketThreshold) return kLossLost;
  return time_sent <= lost_send_time ? kLossLost : kLossWait;
}
// the end of detect_lost_packets (loss.rs:170): kRecNone = None
MQ_HD void rec_set_loss_time(RecState& s, uint32_t level, uint64_t t) {
  rec_set3(s.loss_time, level, t == kRecNone ? 0 : t);
  s.have = t == kRecNone ? s.have & ~(kHaveLossTime << level) : s.have | kHaveLossTime << level;
}
// pto_duration (loss.rs:176-185)
MQ_HD uint64_t rec_pto_duration(const RecState& s) {
  const uint64_t rttvar = (s.have & kHaveSrtt) ? s.rttvar : kRecInitialRtt / 2;
  const uint64_t v = 4 * rttvar > kRecGranularity ? 4 * rttvar : kRecGranularity;
  return rec_smoothed_rtt(s) + v + s.max_ack_delay;
}
// next_timeout (loss.rs:241-260) over pto_timeout (:188-228); kRecNone = None
MQ_HD uint64_t rec_next_timeout(const RecState& s, bool ack_eliciting_in_flight) {
  uint64_t t = kRecNone;
  for (uint32_t l = 0; l < 3; ++l) {
    if ((s.have & (kHaveLossTime << l)) && s.loss_time[l] < t) t = s.loss_time[l];
  }
  if (!ack_eliciting_in_flight || !(s.have & (7u * kHaveLastSent))) return t;
  uint64_t recent = 0;
  for (uint32_t l = 0; l < 3; ++l) {
    if ((s.have & (kHaveLastSent << l)) && s.last_sent[l] > recent) recent = s.last_sent[l];
  }
  const uint32_t shift = s.pto_count < 62 ? s.pto_count : 62;
  const uint64_t pto = recent + rec_pto_duration(s) * (1ull << shift);
  return pto < t ? pto : t;
}

// ---- CongestionController ---------------------------------------------------------------------------------
// on_packet_acked (congestion.rs:54-72)
MQ_HD void rec_on_packet_acked(RecState& s, uint64_t bytes, uint64_t sent_time) {
  s.in_flight = rec_sat_sub(s.in_flight, bytes);
  if ((s.have & kHaveRecoveryStart) && sent_time <= s.recovery_start) return;
  if (s.cwnd < s.ssthresh) s.cwnd += bytes;
  else if (s.cwnd) s.cwnd += s.mds * bytes / s.cwnd;  // (a zero window panics in the reference)
}
// on_packet_lost (congestion.rs:75-87)
MQ_HD void rec_on_packet_lost(RecState& s, uint64_t bytes, uint64_t sent_time, uint64_t now) {
  s.in_flight = rec_sat_sub(s.in_flight, bytes);
  if ((s.have & kHaveRecoveryStart) && sent_time <= s.recovery_start) return;
  s.recovery_start = now;
  s.have |= kHaveRecoveryStart;
  const uint64_t half = s.cwnd / 2;
  s.ssthresh = half > s.min_window ? half : s.min_window;
  s.cwnd = s.ssthresh;
}

// ---- the ACK's ranges ---------------------------------------------------------------------------------------
// decode_varint on bytes [pos, len) seen through fetch(p), p < len; false when it does not fit
template <class Fetch>
MQ_HD bool rec_varint(Fetch& fetch, uint32_t len, uint32_t& pos, uint64_t& out) {
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
// The pairs of dispatch_frame (recv.rs:565-570: the first 16 are kept) and the ranges that on_ack_received
// builds from them (recovery.rs:79-96). visit(lo, hi) is called for every acked range, the first one
// included, in the reference's order. Returns kEvtRangesCut | kEvtRangesBroke. At most 17 pairs are decoded.
template <class Fetch, class Visit>
MQ_HD uint32_t rec_walk_ranges(Fetch& fetch, uint32_t len, uint64_t largest, uint64_t first_range, Visit& visit) {
  uint64_t smallest = rec_sat_sub(largest, first_range);
  visit(smallest, largest);
  uint32_t flags = 0, pos = 0;
  for (uint32_t i = 0; i <= kRecPairs; ++i) {
    uint64_t gap, range;
    if (!rec_varint(fetch, len, pos, gap) || !rec_varint(fetch, len, pos, range)) break;
    if (i == kRecPairs) {
      flags |= kEvtRangesCut;
      break;
    }
    if (flags & kEvtRangesBroke) continue;  // only the count matters behind the break
    if (smallest < gap + 2) {
      flags |= kEvtRangesBroke;
      continue;
    }
    const uint64_t hi = smallest - gap - 2;
    smallest = rec_sat_sub(hi, range);
    visit(smallest, hi);
  }
  return flags;
}

// ---- the array form -------------------------------------------------------------------------------------------
struct RecSent {
  uint64_t pn, time_sent;
  uint32_t meta;
};
struct RecConn {
  RecState s;
  RecSent sent[kSentSlots];
};
struct RecLost {
  uint64_t pn;
  uint32_t size, level;
};
struct RecAckOut {  // what an mq_ack_evt and its mq_lost_pkt say
  uint32_t n_acked, n_acked_cc, n_lost, flags;
  uint64_t largest_newly_acked;
  RecLost lost[kRecLostMax];
};

MQ_HD void rec_clear(RecSent& e) { e.pn = 0, e.time_sent = 0, e.meta = 0; }

// transmit.rs:610-619
MQ_HD void rec_apply_sent(RecConn& c, uint64_t pn, uint32_t level, uint64_t now, uint32_t pkt_len) {
  for (uint32_t i = 0; i < kSentSlots; ++i) {
    if (!sent_used(c.sent[i].meta)) {
      c.sent[i].pn = pn, c.sent[i].time_sent = now, c.sent[i].meta = sent_new_meta(pkt_len, level);
      ++c.s.count;
      break;
    }
  }
  rec_on_sent(c.s, level, now, pkt_len);
}
// drop_space on both structures (recovery.rs:162-171, loss.rs:283-288)
MQ_HD void rec_apply_drop(RecConn& c, uint32_t level) {
  for (uint32_t i = 0; i < kSentSlots; ++i) {
    if (sent_is(c.sent[i].meta, level)) {
      rec_clear(c.sent[i]);
      --c.s.count;
    }
  }
  rec_drop_space(c.s, level);
}
// Frame::HandshakeDone on a client (recv.rs:694-703)
MQ_HD void rec_apply_handshake_done(RecConn& c) {
  c.s.flags |= kRecConfirmed;
  rec_apply_drop(c, 1);
}
MQ_HD uint64_t rec_conn_timeout(const RecConn& c) {
  bool any = false;
  for (uint32_t i = 0; i < kSentSlots; ++i) any = any || sent_counts_for_pto(c.sent[i].meta);
  return rec_next_timeout(c.s, any);
}
struct RecMark {  // which entries of the level an ACK's ranges cover
  const RecConn* c;
  uint32_t level;
  bool acked[kSentSlots];
  MQ_HD void operator()(uint64_t lo, uint64_t hi) {
    for (uint32_t i = 0; i < kSentSlots; ++i) {
      if (sent_is(c->sent[i].meta, level) && c->sent[i].pn >= lo && c->sent[i].pn <= hi) acked[i] = true;
    }
  }
};
// Frame::Ack (recv.rs:563-612)
template <class Fetch>
MQ_HD void rec_apply_ack(RecConn& c, Fetch& fetch, uint32_t len, uint32_t level, uint64_t largest, uint64_t ack_delay,
                         uint64_t first_range, uint64_t now, RecAckOut& out) {
  RecMark mark;
  mark.c = &c, mark.level = level;
  for (uint32_t i = 0; i < kSentSlots; ++i) mark.acked[i] = false;
  out.flags = rec_walk_ranges(fetch, len, largest, first_range, mark);
  out.n_acked = 0, out.n_acked_cc = 0, out.n_lost = 0, out.largest_newly_acked = 0;
  RecSent newly[kRecNewlyAcked];
  RecSent top = {0, 0, 0};
  for (uint32_t i = 0; i < kSentSlots; ++i) {
    if (!mark.acked[i]) continue;
    if (out.n_acked_cc < kRecNewlyAcked) newly[out.n_acked_cc++] = c.sent[i];
    if (out.n_acked == 0 || c.sent[i].pn > top.pn) top = c.sent[i];
    ++out.n_acked;
    rec_clear(c.sent[i]);
    --c.s.count;
  }
  const uint64_t la = rec_on_largest_acked(c.s, level, largest);
  if (out.n_acked) {
    out.largest_newly_acked = top.pn;
    if (top.time_sent > 0 && now >= top.time_sent) {
      rec_update_rtt(c.s, now - top.time_sent, ack_delay, (c.s.flags & kRecConfirmed) != 0);
      out.flags |= kEvtRtt;
    }
    c.s.pto_count = 0;
  }
  for (uint32_t k = 0; k < out.n_acked_cc; ++k) rec_on_packet_acked(c.s, sent_size(newly[k].meta), newly[k].time_sent);
  // detect_lost_packets
  const uint64_t delay = rec_loss_delay(c.s), lost_send_time = rec_sat_sub(now, delay);
  uint64_t lost_pns[kRecLostMax];
  uint64_t loss_time = kRecNone;
  for (uint32_t i = 0; i < kSentSlots; ++i) {
    if (!sent_is(c.sent[i].meta, level)) continue;
    const uint32_t cls = rec_loss_class(c.sent[i].pn, c.sent[i].time_sent, la, lost_send_time);
    if (cls == kLossLost) {
      if (out.n_lost == kRecLostMax) {
        out.flags |= kEvtLostCut;
        break;
      }
      lost_pns[out.n_lost++] = c.sent[i].pn;
    } else if (cls == kLossWait) {
      const uint64_t deadline = c.sent[i].time_sent + delay;
      if (deadline < loss_time) loss_time = deadline;
    }
  }
  rec_set_loss_time(c.s, level, loss_time);
  uint32_t removed = 0;
  for (uint32_t k = 0; k < out.n_lost; ++k) {
    for (uint32_t i = 0; i < kSentSlots; ++i) {
      if (sent_is(c.sent[i].meta, level) && c.sent[i].pn == lost_pns[k]) {
        const RecSent e = c.sent[i];
        rec_clear(c.sent[i]);
        --c.s.count;
        rec_on_packet_lost(c.s, sent_size(e.meta), e.time_sent, now);
        out.lost[removed].pn = e.pn, out.lost[removed].size = sent_size(e.meta), out.lost[removed].level = level;
        ++removed;
        break;
      }
    }
  }
  out.n_lost = removed;  // every lost pn names an entry that is still there: removed == lost_pns.len()
}

}  // namespace mq
