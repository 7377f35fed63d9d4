// test_stream_data_host.cpp — the kernels' shared stream arithmetic (milli_quic_amd/csrc/mq_stream_data.h)
// replayed on the host against a table that tests/test_stream_data.py writes from the Python model. Built
// with -fsanitize=address,undefined: every connection sits in a heap object of exactly its size, so an
// access outside the 32 slots is an ASan error.
//
// Table (little-endian): uint32 case count; per case uint32 stream_buf, uint64 initial_max, uint32
// is_client, the connection's mq_conn_streams before (2592 bytes), uint32 n_records and per record
// { uint32 type, len; uint64 id, a; uint32 dst; uint16 copy_len, skip; uint8 map_slot, buf_slot, mark,
// store, flags, pad[3] } (the expected outcome behind the inputs), the expected mq_conn_streams after the
// replay, uint32 n_reads and per read { uint32 slot, cap, copied; uint8 status, fin, pad[2] }, and the
// expected mq_conn_streams after the reads.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mq_aead.h"
#include "../../milli_quic_amd/csrc/mq_stream_data.h"

namespace {
struct Rec {
  uint32_t type, len;
  uint64_t id, a;
  uint32_t dst;
  uint16_t copy_len, skip;
  uint8_t map_slot, buf_slot, mark, store, flags, pad[3];
};
struct Read {
  uint32_t slot, cap, copied;
  uint8_t status, fin, pad[2];
};
static_assert(sizeof(Rec) == 40 && sizeof(Read) == 16, "table layout");

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || std::fread(to, 1, n, f) == n; }

void load_buf(const mq_stream_buf& p, mq::StreamBuf& b, uint32_t stream_buf) {
  b.stream_id = p.stream_id, b.next_offset = p.next_offset, b.len = p.len, b.read_offset = p.read_offset;
  b.used = p.used, b.fin_received = p.fin_received;
  mq::stream_buf_clamp(b, stream_buf);
}
mq::StreamConn* load(const mq_conn_streams& s, uint32_t stream_buf) {
  mq::StreamConn* c = new mq::StreamConn;  // exactly sized
  for (uint32_t i = 0; i < mq::kStreamSlots; ++i) {
    const mq_stream_entry& e = s.map[i];
    c->map[i] = {e.id, e.recv_offset, e.recv_max_data, e.recv_max_data_next, e.fin_offset, e.flags, e.recv_state};
    load_buf(s.buf[i], c->buf[i], stream_buf);
  }
  c->max_bidi_remote = s.max_bidi_remote, c->max_uni_remote = s.max_uni_remote;
  return c;
}
void store(mq_conn_streams& s, const mq::StreamConn& c) {  // whole, but never the reserved bytes
  for (uint32_t i = 0; i < mq::kStreamSlots; ++i) {
    mq_stream_entry& e = s.map[i];
    const mq::StreamEntry& m = c.map[i];
    e.id = m.id, e.recv_offset = m.recv_offset, e.recv_max_data = m.recv_max_data;
    e.recv_max_data_next = m.recv_max_data_next, e.fin_offset = m.fin_offset, e.flags = m.flags, e.recv_state = m.recv_state;
    mq_stream_buf& p = s.buf[i];
    const mq::StreamBuf& b = c.buf[i];
    p.stream_id = b.stream_id, p.next_offset = b.next_offset, p.len = b.len, p.read_offset = b.read_offset;
    p.used = b.used, p.fin_received = b.fin_received;
  }
  s.max_bidi_remote = c.max_bidi_remote, s.max_uni_remote = c.max_uni_remote;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(mq_stream_entry) == 48 && sizeof(mq_stream_buf) == 32 && sizeof(mq_conn_streams) == 2592 &&
                    sizeof(mq_stream_evt) == 32 && sizeof(mq_stream_read_req) == 32 && sizeof(mq_stream_read_res) == 8,
                "ABI layout");
  static_assert(MQ_STREAM_SLOTS == mq::kStreamSlots && MQ_STREAM_WOULD_BLOCK == mq::kStreamWouldBlock &&
                    MQ_STREAMS_CLIENT == 1,
                "ABI constants");
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_cases = 0;
  if (!read_exact(f, &n_cases, 4)) return 2;
  int bad = 0;
  uint64_t n_recs_all = 0, n_reads_all = 0;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t stream_buf = 0, is_client = 0, n_recs = 0, n_reads = 0;
    uint64_t initial_max = 0;
    mq_conn_streams* state = new mq_conn_streams;
    mq_conn_streams* want = new mq_conn_streams;
    if (!read_exact(f, &stream_buf, 4) || !read_exact(f, &initial_max, 8) || !read_exact(f, &is_client, 4) ||
        !read_exact(f, state, sizeof *state) || !read_exact(f, &n_recs, 4))
      return 2;
    std::vector<Rec> recs(n_recs);
    if (!read_exact(f, recs.data(), sizeof(Rec) * (size_t)n_recs) || !read_exact(f, want, sizeof *want)) return 2;
    mq::StreamConn* conn = load(*state, stream_buf);
    for (uint32_t i = 0; i < n_recs; ++i) {
      const Rec& r = recs[i];
      const mq::StreamOutcome o =
          mq::stream_apply(*conn, r.type, r.id, r.a, r.len, is_client != 0, initial_max, stream_buf);
      if (o.map_slot != r.map_slot || o.buf_slot != r.buf_slot || o.mark != r.mark || o.store != r.store ||
          o.flags != r.flags || o.skip != r.skip || o.copy_len != r.copy_len || o.dst != r.dst) {
        std::printf("case %u record %u: slots %u/%u mark %u store %u flags %02x skip %u copy %u dst %u, expected "
                    "%u/%u %u %u %02x %u %u %u\n",
                    c, i, o.map_slot, o.buf_slot, o.mark, o.store, o.flags, o.skip, o.copy_len, o.dst, r.map_slot,
                    r.buf_slot, r.mark, r.store, r.flags, r.skip, r.copy_len, r.dst);
        ++bad;
        break;
      }
      if (o.store == mq::kStoreCopied && (uint64_t)o.dst + o.copy_len > stream_buf) {
        std::printf("case %u record %u: the copy leaves the buffer\n", c, i);
        ++bad;
      }
    }
    if (n_recs) store(*state, *conn);  // a connection without records is left as it is
    if (std::memcmp(state, want, sizeof *want) != 0) {
      std::printf("case %u: state after the replay differs\n", c);
      ++bad;
    }
    delete conn;
    n_recs_all += n_recs;

    if (!read_exact(f, &n_reads, 4)) return 2;
    std::vector<Read> reads(n_reads);
    if (!read_exact(f, reads.data(), sizeof(Read) * (size_t)n_reads) || !read_exact(f, want, sizeof *want)) return 2;
    for (uint32_t i = 0; i < n_reads; ++i) {
      const Read& q = reads[i];
      if (q.slot >= mq::kStreamSlots) return 2;
      mq_stream_buf& p = state->buf[q.slot];
      mq::StreamBuf* b = new mq::StreamBuf;
      load_buf(p, *b, stream_buf);
      const mq::StreamRead r = mq::stream_read(*b, q.cap);
      if (r.copied != q.copied || r.status != q.status || r.fin != q.fin || (uint64_t)r.from + r.copied > stream_buf) {
        std::printf("case %u read %u: copied %u status %u fin %u, expected %u %u %u\n", c, i, r.copied, r.status, r.fin,
                    q.copied, q.status, q.fin);
        ++bad;
      }
      if (r.status == MQ_OK) p.len = b->len, p.read_offset = b->read_offset, p.used = b->used;
      delete b;
    }
    if (std::memcmp(state, want, sizeof *want) != 0) {
      std::printf("case %u: state after the reads differs\n", c);
      ++bad;
    }
    n_reads_all += n_reads;
    delete state;
    delete want;
  }
  std::fclose(f);
  if (bad) {
    std::printf("FAILED %d of %u cases\n", bad, n_cases);
    return 1;
  }
  std::printf("stream data host ok %u cases %llu records %llu reads\n", n_cases, (unsigned long long)n_recs_all,
              (unsigned long long)n_reads_all);
  return 0;
}
