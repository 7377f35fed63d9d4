// mq_stream_data.h — the per-stream and per-buffer arithmetic of mq_batch_stream_data and
// mq_batch_stream_read (mq_stream_data.hip) as plain integer code that compiles for the device and for
// the host (tests/csrc/test_stream_data_host.cpp replays it without a GPU): StreamMap::get_or_create,
// mark_recv and handle_reset (reference src/transport/stream.rs:227-280, 325-388, 405-424), the decision
// of store_stream_data (src/connection/mod.rs:769-842) and of stream_recv (mod.rs:660-687).
//
// A connection is the reference's default form (no `alloc`): 32 Option<StreamState> and 32
// Option<StreamRecvBuf>. The functions on one entry and one buffer are what both forms share. The array
// form (StreamConn, stream_apply) states a whole record on the tables with loops; mq_stream_data.hip
// keeps one map slot and one buffer slot per lane and replaces the loops by ballots.
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

constexpr uint32_t kStreamSlots = 32;  // MQ_STREAM_SLOTS
constexpr uint32_t kStreamNone = 0xFF;

// mq_stream_entry.flags
constexpr uint8_t kSeUsed = 0x01, kSeHasRecv = 0x02, kSeHasSend = 0x04, kSeHasFin = 0x08;
// mq_stream_entry.recv_state (RecvStreamState, stream.rs)
constexpr uint8_t kRsRecv = 0, kRsSizeKnown = 1, kRsDataRecvd = 2, kRsResetRecvd = 3;
// mq_stream_evt.mark
constexpr uint8_t kMarkOk = 0, kMarkInvalidState = 1, kMarkStreamState = 2, kMarkFinalSize = 3, kMarkFlowControl = 4;
// mq_stream_evt.store
constexpr uint8_t kStoreNone = 0, kStoreNoBuffer = 1, kStoreGap = 2, kStoreDuplicate = 3, kStoreCopied = 4;
// mq_stream_evt.flags
constexpr uint8_t kEvNewStream = 0x01, kEvNewBuf = 0x02, kEvFinSet = 0x04, kEvTruncated = 0x08, kEvReadable = 0x10,
                  kEvReset = 0x20;
// mq_stream_read_res.status beside MQ_OK / MQ_ERR_INVALID_ARG / MQ_ERR_DEFERRED
constexpr uint8_t kStreamWouldBlock = 11;  // MQ_STREAM_WOULD_BLOCK

struct StreamEntry {  // mq_stream_entry without its reserved bytes
  uint64_t id, recv_offset, recv_max_data, recv_max_data_next, fin_offset;
  uint8_t flags, recv_state;
};
struct StreamBuf {  // mq_stream_buf without its reserved bytes
  uint64_t stream_id, next_offset;
  uint32_t len, read_offset;
  uint8_t used, fin_received;
};

// get_or_create's first question (stream.rs:235-243): as the client, the peer's ids are the odd ones
MQ_HD bool stream_peer_initiated(uint64_t id, bool is_client) { return (id & 1) == (is_client ? 1u : 0u); }
MQ_HD bool stream_bidirectional(uint64_t id) { return (id & 2) == 0; }

// the entry get_or_create makes (stream.rs:253-276, RecvState::new :129-137)
MQ_HD void stream_entry_create(StreamEntry& e, uint64_t id, uint64_t initial_max) {
  e.id = id;
  e.recv_offset = 0;
  e.recv_max_data = e.recv_max_data_next = initial_max;
  e.fin_offset = 0;
  e.flags = (uint8_t)(kSeUsed | kSeHasRecv | (stream_bidirectional(id) ? kSeHasSend : 0));
  e.recv_state = kRsRecv;
}
// max_bidi_remote / max_uni_remote after a new stream (stream.rs:256-259, 267-270)
MQ_HD uint64_t stream_raise_remote(uint64_t cur, uint64_t id) { return id / 4 >= cur ? id / 4 + 1 : cur; }

// mark_recv (stream.rs:325-388) on a found entry, with its partial effects before an error. offset is a
// varint (< 2^62) and len < 2^16, so `end` cannot wrap; the auto-tune's add is 64-bit wrapping where the
// reference would overflow (a seeded window near 2^64).
MQ_HD uint8_t stream_mark_recv(StreamEntry& e, uint64_t offset, uint64_t len, bool fin) {
  if (!(e.flags & kSeHasRecv)) return kMarkInvalidState;
  if (e.recv_state != kRsRecv && e.recv_state != kRsSizeKnown) return kMarkStreamState;
  const uint64_t end = offset + len;
  if (e.flags & kSeHasFin) {
    if (end > e.fin_offset) return kMarkFinalSize;
    if (fin && end != e.fin_offset) return kMarkFinalSize;
  }
  if (fin) {
    e.fin_offset = end;
    e.flags |= kSeHasFin;
    e.recv_state = kRsSizeKnown;
  }
  if (end > e.recv_max_data) return kMarkFlowControl;
  if (end > e.recv_offset) e.recv_offset = end;
  if ((e.flags & kSeHasFin) && e.recv_offset >= e.fin_offset) e.recv_state = kRsDataRecvd;
  const uint64_t remaining = e.recv_max_data > e.recv_offset ? e.recv_max_data - e.recv_offset : 0;
  const uint64_t window = e.recv_max_data_next;
  if (remaining < window / 2) e.recv_max_data_next = e.recv_offset + window;
  return kMarkOk;
}

// handle_reset (stream.rs:405-424) on a found entry
MQ_HD uint8_t stream_handle_reset(StreamEntry& e, uint64_t final_size) {
  if (!(e.flags & kSeHasRecv)) return kMarkInvalidState;
  if (e.recv_state != kRsRecv && e.recv_state != kRsSizeKnown && e.recv_state != kRsDataRecvd) return kMarkStreamState;
  if ((e.flags & kSeHasFin) && e.fin_offset != final_size) return kMarkFinalSize;
  e.fin_offset = final_size;
  e.flags |= kSeHasFin;
  e.recv_state = kRsResetRecvd;
  return kMarkOk;
}

// a loaded buffer header: flags become 0 / 1, len <= stream_buf, read_offset <= len
MQ_HD void stream_buf_clamp(StreamBuf& b, uint32_t stream_buf) {
  b.used = b.used != 0;
  b.fin_received = b.fin_received != 0;
  if (b.len > stream_buf) b.len = stream_buf;
  if (b.read_offset > b.len) b.read_offset = b.len;
}
MQ_HD void stream_buf_init(StreamBuf& b, uint64_t id) {  // mod.rs:808-815
  b.stream_id = id, b.next_offset = 0, b.len = 0, b.read_offset = 0, b.used = 1, b.fin_received = 0;
}

struct StreamStore {
  uint32_t dst;  // buf.len before the frame (store == 4)
  uint16_t skip, copy_len;
  uint8_t store, flags;  // kStore*, kEvFinSet | kEvTruncated
};
// store_stream_data on its buffer (mod.rs:817-840): what to copy, and the header's new counters
MQ_HD StreamStore stream_store(StreamBuf& b, uint64_t offset, uint32_t len, bool fin, uint32_t stream_buf) {
  StreamStore s = {0, 0, 0, kStoreGap, 0};
  if (offset > b.next_offset) return s;
  if (offset + len <= b.next_offset) {
    s.store = kStoreDuplicate;
    if (fin) b.fin_received = 1, s.flags = kEvFinSet;
    return s;
  }
  const uint32_t skip = (uint32_t)(b.next_offset - offset);  // < len
  const uint32_t fresh = len - skip, room = stream_buf - b.len;
  const uint32_t n = fresh < room ? fresh : room;
  s.store = kStoreCopied;
  s.dst = b.len, s.skip = (uint16_t)skip, s.copy_len = (uint16_t)n;
  if (n < fresh) s.flags |= kEvTruncated;
  b.len += n;
  b.next_offset += n;
  if (fin) b.fin_received = 1, s.flags |= kEvFinSet;
  return s;
}

struct StreamRead {
  uint32_t copied, from;  // bytes to copy, from data[from..]
  uint8_t status, fin;
};
// stream_recv on its buffer (mod.rs:664-682); the slot is released by used = 0
MQ_HD StreamRead stream_read(StreamBuf& b, uint32_t cap) {
  StreamRead r = {0, b.read_offset, 0, 0};
  const uint32_t available = b.len - b.read_offset;
  if (available == 0) {
    if (b.fin_received) b.used = 0, r.fin = 1;
    else r.status = kStreamWouldBlock;
    return r;
  }
  r.copied = available < cap ? available : cap;
  b.read_offset += r.copied;
  r.fin = b.fin_received && b.read_offset >= b.len;
  if (r.fin) b.used = 0;
  return r;
}

// ---- the array form: one record on a connection's tables -------------------------------------------
struct StreamConn {
  StreamEntry map[kStreamSlots];
  StreamBuf buf[kStreamSlots];
  uint64_t max_bidi_remote, max_uni_remote;
};
struct StreamOutcome {  // the fields of mq_stream_evt that the replay decides
  uint32_t dst;
  uint16_t copy_len, skip;
  uint8_t map_slot, buf_slot, mark, store, flags;
};

MQ_HD uint32_t stream_find(const StreamConn& c, uint64_t id) {
  for (uint32_t s = 0; s < kStreamSlots; ++s) {
    if ((c.map[s].flags & kSeUsed) && c.map[s].id == id) return s;
  }
  return kStreamNone;
}

// type 0x04: RESET_STREAM(id, final_size = a). type 0x08..0x0f: STREAM(id, offset = a, len), FIN = type & 1.
// recv.rs:620-644, 661-669.
MQ_HD StreamOutcome stream_apply(StreamConn& c, uint32_t type, uint64_t id, uint64_t a, uint32_t len, bool is_client,
                                 uint64_t initial_max, uint32_t stream_buf) {
  StreamOutcome o = {0, 0, 0, (uint8_t)kStreamNone, (uint8_t)kStreamNone, 0xFF, kStoreNone, 0};
  const bool is_stream = type >= 0x08;
  uint32_t m = stream_find(c, id);
  if (m == kStreamNone && is_stream && stream_peer_initiated(id, is_client)) {
    for (uint32_t s = 0; s < kStreamSlots; ++s) {
      if (!(c.map[s].flags & kSeUsed)) {
        m = s;
        break;
      }
    }
    if (m != kStreamNone) {
      stream_entry_create(c.map[m], id, initial_max);
      uint64_t& remote = stream_bidirectional(id) ? c.max_bidi_remote : c.max_uni_remote;
      remote = stream_raise_remote(remote, id);
      o.flags |= kEvNewStream;
    }
  }
  if (m == kStreamNone) return o;
  o.map_slot = (uint8_t)m;
  if (!is_stream) {
    o.mark = stream_handle_reset(c.map[m], a);
    o.flags |= kEvReset;
    return o;
  }
  const bool fin = type & 1;
  o.mark = stream_mark_recv(c.map[m], a, len, fin);
  o.flags |= kEvReadable;
  uint32_t b = kStreamNone;
  for (uint32_t s = 0; s < kStreamSlots && b == kStreamNone; ++s) {
    if (c.buf[s].used && c.buf[s].stream_id == id) b = s;
  }
  if (b == kStreamNone) {
    for (uint32_t s = 0; s < kStreamSlots && b == kStreamNone; ++s) {
      if (!c.buf[s].used) b = s;
    }
    if (b == kStreamNone) {
      o.store = kStoreNoBuffer;
      return o;
    }
    stream_buf_init(c.buf[b], id);
    o.flags |= kEvNewBuf;
  }
  o.buf_slot = (uint8_t)b;
  const StreamStore s = stream_store(c.buf[b], a, len, fin, stream_buf);
  o.store = s.store, o.flags |= s.flags;
  if (s.store == kStoreCopied) o.dst = s.dst, o.skip = s.skip, o.copy_len = s.copy_len;
  return o;
}

}  // namespace mq
