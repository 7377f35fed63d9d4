// mq_recovery.hip — mq_batch_sent and mq_batch_recovery: sent-packet tracking, received ACK frames, RTT,
// congestion window and timers on the device (SentPacketTracker, LossDetector and CongestionController,
// reference src/transport/{recovery,loss,congestion}.rs, as driven by src/connection/transmit.rs:610-619,
// 743-752 and by Frame::Ack / Frame::HandshakeDone in dispatch_frame, src/connection/recv.rs:563-612,
// 692-704). The arithmetic is mq_recovery.h, shared with the host test.
//
// Which slot a packet gets, which 32 acked packets reach the congestion controller, which 64 are lost and
// what the window is afterwards all depend on the order of the requests and records of a connection, so it
// is the sequential replay per connection that has to come out:
//   select   one thread per request / record: key = conn, or n_conns where it is not selected; for an ACK
//            record a flag, the arena offset of its range bytes and its datagram's time
//   scan     exclusive sum of the flags (hipcub): an ACK record's event index, so events come out in
//            record order
//   sort     stable radix sort of (key, index) over the bits of n_conns (hipcub): each connection's
//            requests / records become contiguous, still in order
//   replay   ONE WAVE per connection, lane l holding slots l and l + 64 of the tracker; the scalar state
//            is the same in every lane. The wave finds its run by binary search over the sorted keys and
//            loads it 64 at a time (lane i item i of the chunk).
//            sent: the free slots' ranks (mbcnt over two ballots) pair them with the chunk's requests, so
//            a chunk is stored in one step; the last send time per level is a ballot and a broadcast.
//            recovery: the records are applied in turn from lane broadcasts. The ACK's range bytes are
//            loaded once (lane i bytes i, i + 64, ..) and the walk over the ranges marks each lane's two
//            entries; "acked", "lost" and "first entry with this pn" are two ballots each, the rank of a
//            slot inside its mask gives the 32-cap, the 64-cap and its break point; the congestion
//            updates, which depend on order through cwnd, run as a wave-uniform loop over broadcasts of
//            at most 32 + 64 packets. Lost packets go to the connection's own 128 staging entries (a call
//            cannot lose more than the tracker holds).
//   scan     exclusive sum of the events' loss counts: lost_first
//   finish   one thread per event: lost_first, and its staged mq_lost_pkt to their place below max_lost
// Every output is a function of the inputs: no atomics.
#include "mq_launch.h"
#include "mq_recovery.h"
#include "mq_replay.h"

namespace mq {

constexpr uint32_t kRcBlock = 256;
constexpr uint32_t kRcWavesPerBlock = kRcBlock / kWave;
constexpr uint32_t kRcBytes = 5;  // range bytes per lane: 17 pairs are at most 272 bytes
static_assert(kSentSlots == 2 * kWave, "two slots per lane");
static_assert(kRcBytes * kWave >= (kRecPairs + 1) * 16, "the decoded pairs fit the lanes' bytes");
static_assert(sizeof(mq_sent_pkt) == 24 && sizeof(mq_conn_recovery) == 3264 && sizeof(mq_ack_evt) == 32 &&
                  sizeof(mq_lost_pkt) == 16 && sizeof(mq_frame) == 48 && sizeof(mq_send_req) == 48 &&
                  sizeof(mq_recv_pkt) == 32 && sizeof(mq_dgram) == 16,
              "ABI");
static_assert(offsetof(mq_conn_recovery, cwnd) == 112 && offsetof(mq_conn_recovery, have) == 168 &&
                  offsetof(mq_conn_recovery, sent) == 192,
              "ABI");
static_assert(MQ_SENT_SLOTS == kSentSlots && MQ_SENT_USED == kSentUsed && MQ_SENT_ACK_ELICITING == kSentAckEliciting &&
                  MQ_SENT_IN_FLIGHT == kSentInFlight && MQ_RECOVERY_CONFIRMED == kRecConfirmed &&
                  MQ_ACKEVT_RTT == kEvtRtt && MQ_ACKEVT_RANGES_CUT == kEvtRangesCut &&
                  MQ_ACKEVT_RANGES_BROKE == kEvtRangesBroke && MQ_ACKEVT_LOST_CUT == kEvtLostCut,
              "ABI constants");

struct SentWs : SortWs {  // n each
  void* cub;
  size_t cub_bytes;
};
struct RecoveryWs : SortWs {                // max_frames each
  uint32_t *flags, *pos;                    // max_frames + 1: selected ACK records, their exclusive scan
  uint64_t *src, *now;                      // max_frames: arena offset of the range bytes, the datagram's time
  uint32_t *n_lost, *lost_base;             // max_frames + 1: losses per event, their exclusive scan
  uint32_t* lost_at;                        // max_frames: an event's first staging entry
  mq_lost_pkt* staged;                      // 128 n_conns
  void* cub;
  size_t cub_bytes;
};

// ---- the wave: the group's ballot, get, below and count, and what only this file needs -------------------
using RcLanes = LaneGroup<kWave>;
// the value of lane `src`, which is the same in all lanes
__device__ __forceinline__ uint32_t rc_bcast32(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(src & 63u));
}
__device__ __forceinline__ uint64_t rc_bcast64(uint64_t v, uint32_t src) {
  return rc_bcast32((uint32_t)v, src) | (uint64_t)rc_bcast32((uint32_t)(v >> 32), src) << 32;
}
__device__ __forceinline__ uint64_t rc_xor64(uint64_t v, uint32_t d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)d, kWave);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)d, kWave);
  return lo | (uint64_t)hi << 32;
}
__device__ __forceinline__ uint64_t rc_max64(uint64_t v) {
#pragma unroll
  for (uint32_t d = kWave / 2; d; d >>= 1) {
    const uint64_t o = rc_xor64(v, d);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t rc_min64(uint64_t v) { return ~rc_max64(~v); }
__device__ __forceinline__ uint64_t rc_sum64(uint64_t v) {
#pragma unroll
  for (uint32_t d = kWave / 2; d; d >>= 1) v += rc_xor64(v, d);
  return v;
}
// the lowest slot of a mask pair (low half, high half); one of them is not empty
__device__ __forceinline__ uint32_t rc_first(uint64_t lo, uint64_t hi) {
  return lo ? (uint32_t)__builtin_ctzll(lo) : kWave + (uint32_t)__builtin_ctzll(hi);
}

// A connection over the wave: lane l holds entries l and l + 64; s is the same in all lanes.
struct LaneConn {
  RecState s;
  uint64_t pn[2], ts[2];
  uint32_t meta[2];
  uint32_t lane;

  __device__ __forceinline__ void load(const mq_conn_recovery* p) {
    for (uint32_t l = 0; l < 3; ++l) {
      s.largest_acked[l] = p->largest_acked[l];
      s.last_sent[l] = p->time_of_last_ack_eliciting[l];
      s.loss_time[l] = p->loss_time[l];
    }
    s.srtt = p->smoothed_rtt, s.rttvar = p->rttvar, s.min_rtt = p->min_rtt, s.latest_rtt = p->latest_rtt;
    s.max_ack_delay = p->max_ack_delay;
    s.cwnd = p->cwnd, s.ssthresh = p->ssthresh, s.in_flight = p->bytes_in_flight;
    s.recovery_start = p->recovery_start_time, s.persistent_threshold = p->persistent_congestion_threshold;
    s.mds = p->max_datagram_size, s.min_window = p->minimum_window;
    s.have = p->have, s.pto_count = p->pto_count, s.count = p->count, s.flags = p->flags;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint64_t* e = reinterpret_cast<const uint64_t*>(&p->sent[lane + kWave * h]);
      pn[h] = e[0], ts[h] = e[1], meta[h] = (uint32_t)e[2];
      if (!sent_used(meta[h])) clear(h);  // an unused entry goes back all-zero
    }
  }
  // every field but `reserved`, every entry
  __device__ __forceinline__ void store(mq_conn_recovery* p) {
    rec_normalise(s);
    if (lane == 0) {
      for (uint32_t l = 0; l < 3; ++l) {
        p->largest_acked[l] = s.largest_acked[l];
        p->time_of_last_ack_eliciting[l] = s.last_sent[l];
        p->loss_time[l] = s.loss_time[l];
      }
      p->smoothed_rtt = s.srtt, p->rttvar = s.rttvar, p->min_rtt = s.min_rtt, p->latest_rtt = s.latest_rtt;
      p->max_ack_delay = s.max_ack_delay;
      p->cwnd = s.cwnd, p->ssthresh = s.ssthresh, p->bytes_in_flight = s.in_flight;
      p->recovery_start_time = s.recovery_start, p->persistent_congestion_threshold = s.persistent_threshold;
      p->max_datagram_size = s.mds, p->minimum_window = s.min_window;
      p->have = s.have, p->pto_count = s.pto_count, p->count = s.count, p->flags = s.flags;
    }
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      uint64_t* e = reinterpret_cast<uint64_t*>(&p->sent[lane + kWave * h]);
      e[0] = pn[h], e[1] = ts[h], e[2] = meta[h];
    }
  }
  __device__ __forceinline__ void clear(uint32_t h) { pn[h] = 0, ts[h] = 0, meta[h] = 0; }
  // entry `slot` (< 128, the same in all lanes)
  __device__ __forceinline__ uint64_t pn_of(uint32_t slot) const { return rc_bcast64(slot < kWave ? pn[0] : pn[1], slot); }
  __device__ __forceinline__ uint64_t ts_of(uint32_t slot) const { return rc_bcast64(slot < kWave ? ts[0] : ts[1], slot); }
  __device__ __forceinline__ uint32_t meta_of(uint32_t slot) const {
    return rc_bcast32(slot < kWave ? meta[0] : meta[1], slot);
  }
  __device__ __forceinline__ void clear_slot(uint32_t slot) {
    if (lane == (slot & (kWave - 1))) {
      if (slot < kWave) clear(0);
      else clear(1);
    }
  }
  // drop_space on both structures (recovery.rs:162-171, loss.rs:283-288)
  __device__ __forceinline__ void drop(uint32_t level) {
    const bool d0 = sent_is(meta[0], level), d1 = sent_is(meta[1], level);
    s.count -= RcLanes::count(RcLanes::ballot(d0)) + RcLanes::count(RcLanes::ballot(d1));
    if (d0) clear(0);
    if (d1) clear(1);
    rec_drop_space(s, level);
  }
  __device__ __forceinline__ uint64_t timeout() const {
    const bool any = RcLanes::ballot(sent_counts_for_pto(meta[0]) || sent_counts_for_pto(meta[1])) != 0;
    return rec_next_timeout(s, any);
  }
};

// an ACK's range bytes over the wave: lane i holds bytes i, i + 64, ..
struct LaneBytes {
  uint32_t b[kRcBytes];
  __device__ __forceinline__ uint32_t operator()(uint32_t p) const {  // p < 272, the same in all lanes
    const uint32_t q = p >> 6;
    const uint32_t v = q == 0 ? b[0] : q == 1 ? b[1] : q == 2 ? b[2] : q == 3 ? b[3] : b[4];
    return rc_bcast32(v, p);
  }
};
// the walk's visitor: which of the lane's two entries the ranges cover
struct LaneMark {
  uint64_t pn0, pn1;
  bool in0, in1, a0, a1;
  __device__ __forceinline__ void operator()(uint64_t lo, uint64_t hi) {
    a0 = a0 || (in0 && pn0 >= lo && pn0 <= hi);
    a1 = a1 || (in1 && pn1 >= lo && pn1 <= hi);
  }
};

// key_run for a key that the whole wave shares: the run's ends are scalars
__device__ __forceinline__ void rc_run(const uint32_t* __restrict__ keys, uint32_t n, uint32_t c, uint32_t& r,
                                       uint32_t& r_end) {
  key_run(keys, n, c, r, r_end);
  r = __builtin_amdgcn_readfirstlane(r), r_end = __builtin_amdgcn_readfirstlane(r_end);
}

}  // namespace mq

using namespace mq;

// ---- mq_batch_sent -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRcBlock) void mq_sent_key_kernel(const mq_send_req* __restrict__ reqs,
                                                               const uint8_t* __restrict__ status, uint32_t n,
                                                               uint32_t n_conns, SentWs ws) {
  const uint32_t i = blockIdx.x * kRcBlock + threadIdx.x;
  if (i >= n) return;
  const uint4 q = reinterpret_cast<const uint4*>(reqs + i)[2];  // frame_len, out_cap, conn, level + flags
  const bool on = status[i] == MQ_OK && q.z < n_conns && (q.w & 0xFFu) < 3;
  ws.keys_in[i] = on ? q.z : n_conns;
  ws.idx_in[i] = i;
}

__global__ __launch_bounds__(kRcBlock) void mq_sent_replay_kernel(const mq_send_req* __restrict__ reqs,
                                                                  const uint32_t* __restrict__ pkt_len,
                                                                  const uint64_t* __restrict__ now, uint32_t n,
                                                                  mq_conn_recovery* __restrict__ rec, uint32_t n_conns,
                                                                  uint64_t* __restrict__ timeouts, SentWs ws) {
  const uint32_t c = blockIdx.x * kRcWavesPerBlock + wave_id();
  if (c >= n_conns) return;  // the whole wave
  uint32_t r, r_end;
  rc_run(ws.keys, n, c, r, r_end);
  if (r == r_end) return;  // a connection that records nothing is left as it is
  LaneConn t;
  t.lane = threadIdx.x & (kWave - 1);
  t.load(rec + c);
  while (r < r_end) {
    const uint32_t cnt = r_end - r < (uint32_t)kWave ? r_end - r : (uint32_t)kWave;
    uint64_t my_pn = 0, my_now = 0;
    uint32_t my_level = 3, my_len = 0;
    if (t.lane < cnt) {  // lane i takes request i of the chunk
      const uint32_t i = ws.idx[r + t.lane];  // < n: the sort permutes 0 .. n - 1
      my_pn = reqs[i].pn, my_level = reqs[i].level, my_len = pkt_len[i], my_now = now[i];
    }
    // the k-th free slot takes the chunk's k-th request
    const uint64_t f_lo = RcLanes::ballot(!sent_used(t.meta[0])), f_hi = RcLanes::ballot(!sent_used(t.meta[1]));
    const uint32_t n_free = RcLanes::count(f_lo) + RcLanes::count(f_hi);
    const uint32_t rank[2] = {RcLanes::below(f_lo), RcLanes::count(f_lo) + RcLanes::below(f_hi)};
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint64_t q_pn = RcLanes::get64(my_pn, rank[h]), q_now = RcLanes::get64(my_now, rank[h]);
      const uint32_t q_level = RcLanes::get32(my_level, rank[h]), q_len = RcLanes::get32(my_len, rank[h]);
      if (!sent_used(t.meta[h]) && rank[h] < cnt) t.pn[h] = q_pn, t.ts[h] = q_now, t.meta[h] = sent_new_meta(q_len, q_level);
    }
    t.s.count += n_free < cnt ? n_free : cnt;
    t.s.in_flight += rc_sum64(my_len);
    for (uint32_t l = 0; l < 3; ++l) {  // on_ack_eliciting_sent: the level's last request of the chunk
      const uint64_t m = RcLanes::ballot(my_level == l);
      if (m) {
        t.s.last_sent[l] = rc_bcast64(my_now, 63u - (uint32_t)__builtin_clzll(m));
        t.s.have |= kHaveLastSent << l;
      }
    }
    r += cnt;
  }
  t.store(rec + c);
  const uint64_t to = t.timeout();
  if (timeouts && t.lane == 0) timeouts[c] = to;
}

// ---- mq_batch_recovery ---------------------------------------------------------------------------------------
// select: which records are processed, for which connection; an ACK's range bytes and time
__global__ __launch_bounds__(kRcBlock) void mq_recovery_select_kernel(RecoveryArgs a, RecoveryWs ws) {
  const uint32_t k = blockIdx.x * kRcBlock + threadIdx.x;
  if (k > a.max_frames) return;
  ws.n_lost[k] = 0;
  if (k == a.max_frames) {
    ws.flags[k] = 0;
    return;
  }
  const uint32_t nf = *a.n_frames_dev, np = *a.n_pkts_dev;
  const uint32_t n_frames = nf < a.max_frames ? nf : a.max_frames, n_pkts = np < a.max_pkts ? np : a.max_pkts;
  uint32_t key = a.n_conns, flag = 0;
  uint64_t src = 0, now = 0;
  if (k < n_frames) {
    const uint4 f = reinterpret_cast<const uint4*>(a.frames + k)[0];  // pkt; pos, len; type, level, data_pos; data_len, aux
    const uint32_t type = f.z & 0xFFu, level = (f.z >> 8) & 0xFFu, data_pos = f.z >> 16, data_len = f.w & 0xFFFFu;
    const bool ack = type == 0x02 || type == 0x03;
    if ((ack || (type == 0x1e && (a.flags & MQ_RECOVERY_CLIENT))) && level < 3) {
      const FrameSite site = frame_site(a.pkts, n_pkts, a.dgrams, a.n_dgrams, a.arena_len, f.x, data_pos, data_len, ack);
      if (site.conn < a.n_conns && site.inside) {
        key = site.conn, flag = ack;
        src = site.src;
        if (ack) now = a.dgram_now[site.dgram];
      }
    }
  }
  ws.keys_in[k] = key;
  ws.idx_in[k] = k;
  ws.flags[k] = flag;
  ws.src[k] = src;
  ws.now[k] = now;
}

// replay: every connection's drop bits, then its selected records in record order
__global__ __launch_bounds__(kRcBlock) void mq_recovery_replay_kernel(RecoveryArgs a, RecoveryWs ws) {
  const uint32_t c = blockIdx.x * kRcWavesPerBlock + wave_id();
  if (c >= a.n_conns) return;  // the whole wave
  uint32_t r = 0, r_end = 0;
  if (a.max_frames) rc_run(ws.keys, a.max_frames, c, r, r_end);
  const uint32_t drop_bits = a.drop_mask ? a.drop_mask[c] & 7u : 0u;
  if (r == r_end && !drop_bits) return;  // an untouched connection is left as it is
  LaneConn t;
  t.lane = threadIdx.x & (kWave - 1);
  t.load(a.rec + c);
  for (uint32_t l = 0; l < 3; ++l) {
    if (drop_bits >> l & 1u) t.drop(l);
  }
  mq_lost_pkt* staged = ws.staged + (size_t)c * kSentSlots;
  uint32_t staged_n = 0;  // <= 128: every staged packet left a slot, and this call fills none
  while (r < r_end) {
    const uint32_t cnt = r_end - r < (uint32_t)kWave ? r_end - r : (uint32_t)kWave;
    uint32_t my_k = 0, my_head = 0, my_pos = 0;
    uint64_t my_largest = 0, my_delay = 0, my_first = 0, my_src = 0, my_now = 0;
    if (t.lane < cnt) {  // lane i takes record i of the chunk
      my_k = ws.idx[r + t.lane];  // < max_frames: the sort permutes 0 .. max_frames - 1
      const uint4* f = reinterpret_cast<const uint4*>(a.frames + my_k);
      const uint4 h = f[0], v01 = f[1], v23 = f[2];
      my_head = (h.z & 0xFFFFu) | (h.w & 0xFFFFu) << 16;  // type, level, data_len
      my_largest = v01.x | (uint64_t)v01.y << 32, my_delay = v01.z | (uint64_t)v01.w << 32;
      my_first = v23.z | (uint64_t)v23.w << 32;
      my_src = ws.src[my_k], my_now = ws.now[my_k];
      my_pos = ws.pos[my_k];  // the event index: < the number of selected ACK records <= max_frames
    }
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t head = rc_bcast32(my_head, j);
      const uint32_t type = head & 0xFFu, level = (head >> 8) & 0xFFu, len = head >> 16;
      if (type == 0x1e) {  // HANDSHAKE_DONE on a client (recv.rs:694-703)
        t.s.flags |= kRecConfirmed;
        t.drop(1);
        continue;
      }
      const uint32_t k = rc_bcast32(my_k, j), pos = rc_bcast32(my_pos, j);
      const uint64_t largest = rc_bcast64(my_largest, j), ack_delay = rc_bcast64(my_delay, j);
      const uint64_t first_range = rc_bcast64(my_first, j), src = rc_bcast64(my_src, j), now = rc_bcast64(my_now, j);
      // 1. the ranges: which entries they cover
      LaneBytes bytes;
#pragma unroll
      for (uint32_t q = 0; q < kRcBytes; ++q) {
        const uint32_t at = t.lane + kWave * q;
        bytes.b[q] = at < len ? a.arena[src + at] : 0u;  // [src, src + len) lies inside the arena (select)
      }
      LaneMark mark = {t.pn[0], t.pn[1], sent_is(t.meta[0], level), sent_is(t.meta[1], level), false, false};
      uint32_t ev_flags = rec_walk_ranges(bytes, len, largest, first_range, mark);
      // 2. remove them; the first 32 in slot order are newly_acked
      const uint64_t a_lo = RcLanes::ballot(mark.a0), a_hi = RcLanes::ballot(mark.a1);
      const uint32_t n_acked = RcLanes::count(a_lo) + RcLanes::count(a_hi);
      uint64_t top_pn = 0, top_ts = 0;
      if (n_acked) {
        const uint64_t v0 = mark.a0 ? t.pn[0] : 0, v1 = mark.a1 ? t.pn[1] : 0;
        top_pn = rc_max64(v0 > v1 ? v0 : v1);
        const uint32_t top = rc_first(RcLanes::ballot(mark.a0 && t.pn[0] == top_pn), RcLanes::ballot(mark.a1 && t.pn[1] == top_pn));
        top_ts = t.ts_of(top);
      }
      // 3. largest acked
      const uint64_t la = rec_on_largest_acked(t.s, level, largest);
      // 4. RTT
      if (n_acked) {
        if (top_ts > 0 && now >= top_ts) {
          rec_update_rtt(t.s, now - top_ts, ack_delay, (t.s.flags & kRecConfirmed) != 0);
          ev_flags |= kEvtRtt;
        }
        t.s.pto_count = 0;
      }
      // 5. on_packet_acked for the first 32, in slot order
      uint32_t n_cc = 0;
      {
        uint64_t m_lo = a_lo, m_hi = a_hi;
        while (n_cc < kRecNewlyAcked && (m_lo | m_hi)) {
          const uint32_t slot = rc_first(m_lo, m_hi);
          if (m_lo) m_lo &= m_lo - 1;
          else m_hi &= m_hi - 1;
          rec_on_packet_acked(t.s, sent_size(t.meta_of(slot)), t.ts_of(slot));
          ++n_cc;
        }
      }
      if (mark.a0) t.clear(0);
      if (mark.a1) t.clear(1);
      t.s.count -= n_acked;
      // 6. detect_lost_packets
      const uint64_t delay = rec_loss_delay(t.s), lost_send_time = rec_sat_sub(now, delay);
      const uint32_t cls0 = sent_is(t.meta[0], level) ? rec_loss_class(t.pn[0], t.ts[0], la, lost_send_time) : kLossSkip;
      const uint32_t cls1 = sent_is(t.meta[1], level) ? rec_loss_class(t.pn[1], t.ts[1], la, lost_send_time) : kLossSkip;
      uint64_t l_lo = RcLanes::ballot(cls0 == kLossLost), l_hi = RcLanes::ballot(cls1 == kLossLost);
      uint32_t stop = kSentSlots;  // the slot of the 65th loss: the scan ends there
      if (RcLanes::count(l_lo) + RcLanes::count(l_hi) > kRecLostMax) {
        const uint32_t rank0 = RcLanes::below(l_lo), rank1 = RcLanes::count(l_lo) + RcLanes::below(l_hi);
        stop = rc_first(RcLanes::ballot(cls0 == kLossLost && rank0 == kRecLostMax),
                        RcLanes::ballot(cls1 == kLossLost && rank1 == kRecLostMax));
        l_lo = RcLanes::ballot(cls0 == kLossLost && rank0 < kRecLostMax);
        l_hi = RcLanes::ballot(cls1 == kLossLost && rank1 < kRecLostMax);
        ev_flags |= kEvtLostCut;
      }
      const bool w0 = cls0 == kLossWait && t.lane < stop, w1 = cls1 == kLossWait && t.lane + kWave < stop;
      uint64_t loss_time = kRecNone;
      if (RcLanes::ballot(w0 || w1)) {
        const uint64_t d0 = w0 ? t.ts[0] + delay : kRecNone, d1 = w1 ? t.ts[1] + delay : kRecNone;
        loss_time = rc_min64(d0 < d1 ? d0 : d1);
      }
      rec_set_loss_time(t.s, level, loss_time);
      // 7. remove(level, pn) for each lost pn in push order, then on_packet_lost
      const uint32_t staged_first = staged_n;
      uint32_t n_lost = 0;
      while (l_lo | l_hi) {
        const uint32_t from = rc_first(l_lo, l_hi);
        if (l_lo) l_lo &= l_lo - 1;
        else l_hi &= l_hi - 1;
        const uint64_t pn = t.pn_of(from);
        const uint64_t m_lo = RcLanes::ballot(sent_is(t.meta[0], level) && t.pn[0] == pn);
        const uint64_t m_hi = RcLanes::ballot(sent_is(t.meta[1], level) && t.pn[1] == pn);
        if (!(m_lo | m_hi)) continue;  // remove() found nothing
        const uint32_t slot = rc_first(m_lo, m_hi);  // the first entry with this pn, not always `from`
        const uint32_t size = sent_size(t.meta_of(slot));
        const uint64_t sent_time = t.ts_of(slot);
        t.clear_slot(slot);
        --t.s.count;
        rec_on_packet_lost(t.s, size, sent_time, now);
        if (t.lane == 0 && staged_n < kSentSlots) {
          uint4* q = reinterpret_cast<uint4*>(staged + staged_n);
          *q = make_uint4((uint32_t)pn, (uint32_t)(pn >> 32), c, size | level << 16);
        }
        if (staged_n < kSentSlots) ++staged_n, ++n_lost;
      }
      if (t.lane == 0) {  // pos < max_frames
        uint4* q = reinterpret_cast<uint4*>(a.evts + pos);
        q[0] = make_uint4(k, c, n_acked | n_cc << 16, n_lost | ev_flags << 16);
        q[1] = make_uint4(0, 0, (uint32_t)top_pn, (uint32_t)(top_pn >> 32));
        ws.n_lost[pos] = n_lost;
        ws.lost_at[pos] = staged_first;
      }
    }
    r += cnt;
  }
  t.store(a.rec + c);
  const uint64_t to = t.timeout();
  if (a.timeouts && t.lane == 0) a.timeouts[c] = to;
}

// finish: the counts, every event's lost_first, and its lost packets to their place
__global__ __launch_bounds__(kRcBlock) void mq_recovery_finish_kernel(RecoveryArgs a, RecoveryWs ws) {
  const uint32_t i = blockIdx.x * kRcBlock + threadIdx.x;
  const uint32_t n_evts = ws.pos[a.max_frames];  // <= max_frames
  if (i == 0) *a.n_evts = n_evts, *a.n_lost = ws.lost_base[a.max_frames];
  if (i >= n_evts) return;
  const uint32_t base = ws.lost_base[i], n = ws.n_lost[i], at = ws.lost_at[i];
  a.evts[i].lost_first = base;
  const uint32_t c = a.evts[i].conn;  // < n_conns, written by the replay
  if (c >= a.n_conns) return;
  for (uint32_t j = 0; j < n && at + j < kSentSlots; ++j) {  // at + n <= 128 by the replay
    if ((uint64_t)base + j < a.max_lost) {
      reinterpret_cast<uint4*>(a.lost)[base + j] = reinterpret_cast<const uint4*>(ws.staged)[(size_t)c * kSentSlots + at + j];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------
namespace {
// Both layouts end with 256 bytes that no kernel touches. Nobody knows why they are there; callers size
// by these figures.
size_t sent_layout(uint32_t n, uint32_t n_conns, void* base, SentWs& w) {
  Carve c(base);
  w.keys_in = c.take<uint32_t>(n);
  w.keys = c.take<uint32_t>(n);
  w.idx_in = c.take<uint32_t>(n);
  w.idx = c.take<uint32_t>(n);
  w.cub_bytes = cub_temp_bytes<true>(n, key_bits(n_conns), {});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes() + 256;
}
size_t recovery_layout(uint32_t n, uint32_t n_conns, void* base, RecoveryWs& w) {
  Carve c(base);
  w.keys_in = c.take<uint32_t>(n);
  w.keys = c.take<uint32_t>(n);
  w.idx_in = c.take<uint32_t>(n);
  w.idx = c.take<uint32_t>(n);
  w.flags = c.take<uint32_t>((size_t)n + 1);
  w.pos = c.take<uint32_t>((size_t)n + 1);
  w.src = c.take<uint64_t>(n);
  w.now = c.take<uint64_t>(n);
  w.n_lost = c.take<uint32_t>((size_t)n + 1);
  w.lost_base = c.take<uint32_t>((size_t)n + 1);
  w.lost_at = c.take<uint32_t>(n);
  w.staged = c.take<mq_lost_pkt>((size_t)kSentSlots * n_conns);
  w.cub_bytes = cub_temp_bytes<true>(n, key_bits(n_conns), {n + 1});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes() + 256;
}
dim3 rc_blocks(uint64_t threads) { return dim3((uint32_t)((threads + kRcBlock - 1) / kRcBlock)); }
}  // namespace

size_t mq_sent_workspace(uint32_t n, uint32_t n_conns) {
  SentWs w = {};
  return sent_layout(n, n_conns, nullptr, w);
}
size_t mq_recovery_workspace(uint32_t max_frames, uint32_t n_conns) {
  RecoveryWs w = {};
  return recovery_layout(max_frames, n_conns, nullptr, w);
}

// n > 0 and n_conns > 0
hipError_t mq_launch_sent(const SentArgs& a, void* workspace, hipStream_t s) {
  SentWs w = {};
  sent_layout(a.n, a.n_conns, workspace, w);
  hipError_t e;
  const dim3 block(kRcBlock);
  hipLaunchKernelGGL(mq_sent_key_kernel, rc_blocks(a.n), block, 0, s, a.reqs, a.status, a.n, a.n_conns, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = sort_by_key(w, a.n, key_bits(a.n_conns), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_sent_replay_kernel, rc_blocks((uint64_t)a.n_conns * kWave), block, 0, s, a.reqs, a.pkt_len, a.now,
                     a.n, a.rec, a.n_conns, a.timeouts, w);
  return hipGetLastError();
}

// n_conns > 0; max_frames == 0 applies the drop mask alone
hipError_t mq_launch_recovery(const RecoveryArgs& a, void* workspace, hipStream_t s) {
  RecoveryWs w = {};
  recovery_layout(a.max_frames, a.n_conns, workspace, w);
  hipError_t e;
  const dim3 block(kRcBlock);
  if (a.max_frames) {
    hipLaunchKernelGGL(mq_recovery_select_kernel, rc_blocks((uint64_t)a.max_frames + 1), block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_sum(w, w.flags, w.pos, a.max_frames + 1, s)) != hipSuccess) return e;
    if ((e = sort_by_key(w, a.max_frames, key_bits(a.n_conns), s)) != hipSuccess) return e;
  } else {
    if ((e = hipMemsetAsync(a.n_evts, 0, 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.n_lost, 0, 4, s)) != hipSuccess) return e;
    if (!a.drop_mask) return hipSuccess;
  }
  hipLaunchKernelGGL(mq_recovery_replay_kernel, rc_blocks((uint64_t)a.n_conns * kWave), block, 0, s, a, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (!a.max_frames) return hipSuccess;
  if ((e = exclusive_sum(w, w.n_lost, w.lost_base, a.max_frames + 1, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_recovery_finish_kernel, rc_blocks(a.max_frames), block, 0, s, a, w);
  return hipGetLastError();
}
