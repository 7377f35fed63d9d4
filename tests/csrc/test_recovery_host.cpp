// test_recovery_host.cpp — the kernels' shared recovery arithmetic (milli_quic_amd/csrc/mq_recovery.h)
// replayed on the host against a table that tests/test_recovery.py writes from the Python model. Built
// with -fsanitize=address,undefined: the connection and an ACK's range bytes sit in heap buffers of
// exactly their size, so an access outside the 128 entries or the range bytes is an ASan error.
//
// Every case is one connection: its sends in request order (mq_batch_sent), then its drop bits and its
// selected records in record order (mq_batch_recovery). A phase that touches the connection loads the
// row, applies the array form and writes the row back whole, as the device does.
//
// Table (little-endian): uint32 case count; per case the row before (3264 bytes); uint32 n_sends and per
// send uint64 pn, now, uint32 pkt_len, level; the row after the sends and uint64 its timeout; uint32 drop
// bits; uint32 n_recs and per record uint32 type, level, uint64 largest, ack_delay, first_range, now,
// uint32 data_len, the range bytes, and for an ACK the expected uint32 n_acked, n_acked_cc, n_lost, flags,
// uint64 largest_newly_acked and n_lost times (uint64 pn, uint32 size, level); the row after and uint64
// its timeout.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mq_aead.h"
#include "../../milli_quic_amd/csrc/mq_recovery.h"

namespace {
struct Bytes {
  const uint8_t* p;
  uint32_t operator()(uint32_t at) const { return p[at]; }
};

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || std::fread(to, 1, n, f) == n; }
template <class T>
bool rd(FILE* f, T& v) {
  return read_exact(f, &v, sizeof v);
}

void load(const mq_conn_recovery& r, mq::RecConn& c) {
  mq::RecState& s = c.s;
  for (int l = 0; l < 3; ++l) {
    s.largest_acked[l] = r.largest_acked[l], s.last_sent[l] = r.time_of_last_ack_eliciting[l];
    s.loss_time[l] = r.loss_time[l];
  }
  s.srtt = r.smoothed_rtt, s.rttvar = r.rttvar, s.min_rtt = r.min_rtt, s.latest_rtt = r.latest_rtt;
  s.max_ack_delay = r.max_ack_delay, s.cwnd = r.cwnd, s.ssthresh = r.ssthresh, s.in_flight = r.bytes_in_flight;
  s.recovery_start = r.recovery_start_time, s.persistent_threshold = r.persistent_congestion_threshold;
  s.mds = r.max_datagram_size, s.min_window = r.minimum_window;
  s.have = r.have, s.pto_count = r.pto_count, s.count = r.count, s.flags = r.flags;
  for (uint32_t i = 0; i < mq::kSentSlots; ++i) {
    const mq_sent_pkt& e = r.sent[i];
    c.sent[i].pn = e.pn, c.sent[i].time_sent = e.time_sent;
    c.sent[i].meta = mq::sent_meta(e.size, e.level, e.flags);
    if (!mq::sent_used(c.sent[i].meta)) mq::rec_clear(c.sent[i]);
  }
}

void store(mq::RecConn& c, mq_conn_recovery& r) {  // every field but `reserved`
  mq::rec_normalise(c.s);
  const mq::RecState& s = c.s;
  for (int l = 0; l < 3; ++l) {
    r.largest_acked[l] = s.largest_acked[l], r.time_of_last_ack_eliciting[l] = s.last_sent[l];
    r.loss_time[l] = s.loss_time[l];
  }
  r.smoothed_rtt = s.srtt, r.rttvar = s.rttvar, r.min_rtt = s.min_rtt, r.latest_rtt = s.latest_rtt;
  r.max_ack_delay = s.max_ack_delay, r.cwnd = s.cwnd, r.ssthresh = s.ssthresh, r.bytes_in_flight = s.in_flight;
  r.recovery_start_time = s.recovery_start, r.persistent_congestion_threshold = s.persistent_threshold;
  r.max_datagram_size = s.mds, r.minimum_window = s.min_window;
  r.have = s.have, r.pto_count = s.pto_count, r.count = s.count, r.flags = s.flags;
  for (uint32_t i = 0; i < mq::kSentSlots; ++i) {
    mq_sent_pkt& e = r.sent[i];
    std::memset(&e, 0, sizeof e);
    e.pn = c.sent[i].pn, e.time_sent = c.sent[i].time_sent;
    e.size = (uint16_t)mq::sent_size(c.sent[i].meta), e.level = (uint8_t)mq::sent_level(c.sent[i].meta);
    e.flags = (uint8_t)(c.sent[i].meta >> 24);
  }
}

int fail(uint32_t k, const char* what, uint32_t at = 0) {
  std::printf("case %u: %s (%u)\n", k, what, at);
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(mq_sent_pkt) == 24 && sizeof(mq_conn_recovery) == 3264 && sizeof(mq_ack_evt) == 32 &&
                    sizeof(mq_lost_pkt) == 16,
                "ABI layout");
  static_assert(MQ_SENT_SLOTS == mq::kSentSlots && MQ_SENT_USED == mq::kSentUsed &&
                    MQ_RECOVERY_CONFIRMED == mq::kRecConfirmed && MQ_ACKEVT_LOST_CUT == mq::kEvtLostCut,
                "ABI constants");
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_cases = 0;
  if (!rd(f, n_cases)) return 2;
  uint64_t n_sends_all = 0, n_acks_all = 0, n_lost_all = 0;
  for (uint32_t k = 0; k < n_cases; ++k) {
    std::unique_ptr<mq_conn_recovery> row(new mq_conn_recovery), want(new mq_conn_recovery);
    std::unique_ptr<mq::RecConn> c(new mq::RecConn);  // exactly sized
    uint64_t want_timeout = 0;
    uint32_t n_sends = 0, drop = 0, n_recs = 0;
    if (!rd(f, *row) || !rd(f, n_sends)) return 2;
    if (n_sends) load(*row, *c);
    for (uint32_t i = 0; i < n_sends; ++i) {
      uint64_t pn, now;
      uint32_t len, level;
      if (!rd(f, pn) || !rd(f, now) || !rd(f, len) || !rd(f, level)) return 2;
      mq::rec_apply_sent(*c, pn, level, now, len);
    }
    if (!rd(f, *want) || !rd(f, want_timeout)) return 2;
    if (n_sends) {
      store(*c, *row);
      if (mq::rec_conn_timeout(*c) != want_timeout) return fail(k, "timeout after the sends");
    }
    if (std::memcmp(row.get(), want.get(), sizeof *row) != 0) return fail(k, "row after the sends");
    n_sends_all += n_sends;
    if (!rd(f, drop) || !rd(f, n_recs)) return 2;
    const bool touched = (drop & 7u) != 0 || n_recs != 0;
    if (touched) load(*row, *c);
    for (uint32_t l = 0; l < 3; ++l) {
      if (drop >> l & 1u) mq::rec_apply_drop(*c, l);
    }
    for (uint32_t i = 0; i < n_recs; ++i) {
      uint32_t type, level, data_len;
      uint64_t largest, delay, first, now;
      if (!rd(f, type) || !rd(f, level) || !rd(f, largest) || !rd(f, delay) || !rd(f, first) || !rd(f, now) ||
          !rd(f, data_len))
        return 2;
      std::vector<uint8_t> data(data_len);  // exactly sized: a fetch beyond data_len is an ASan error
      if (!read_exact(f, data.data(), data_len)) return 2;
      if (type == 0x1e) {
        mq::rec_apply_handshake_done(*c);
        continue;
      }
      uint32_t w[4];
      uint64_t top;
      if (!read_exact(f, w, sizeof w) || !rd(f, top)) return 2;
      std::unique_ptr<mq::RecAckOut> out(new mq::RecAckOut);
      Bytes fetch = {data.data()};
      mq::rec_apply_ack(*c, fetch, data_len, level, largest, delay, first, now, *out);
      if (out->n_acked != w[0] || out->n_acked_cc != w[1] || out->n_lost != w[2] || out->flags != w[3] ||
          out->largest_newly_acked != top)
        return fail(k, "event of record", i);
      for (uint32_t j = 0; j < w[2]; ++j) {
        uint64_t pn;
        uint32_t size, lvl;
        if (!rd(f, pn) || !rd(f, size) || !rd(f, lvl)) return 2;
        if (out->lost[j].pn != pn || out->lost[j].size != size || out->lost[j].level != lvl)
          return fail(k, "lost packet of record", i);
      }
      ++n_acks_all;
      n_lost_all += w[2];
    }
    if (!rd(f, *want) || !rd(f, want_timeout)) return 2;
    if (touched) {
      store(*c, *row);
      if (mq::rec_conn_timeout(*c) != want_timeout) return fail(k, "timeout after the records");
    }
    if (std::memcmp(row.get(), want.get(), sizeof *row) != 0) return fail(k, "row after the records");
  }
  uint8_t extra;
  if (std::fread(&extra, 1, 1, f) != 0) return 2;  // the whole table was read
  std::fclose(f);
  std::printf("recovery host ok %u cases %llu sends %llu acks %llu lost\n", n_cases, (unsigned long long)n_sends_all,
              (unsigned long long)n_acks_all, (unsigned long long)n_lost_all);
  return 0;
}
