// mq_stream_data.hip — mq_batch_stream_data and mq_batch_stream_read: per-stream bookkeeping and the
// payload gather on the device, behind mq_batch_frames (Frame::Stream / Frame::ResetStream in
// dispatch_frame, reference src/connection/recv.rs:620-644, 661-669; StreamMap, src/transport/stream.rs:
// 227-388, 405-424; store_stream_data and stream_recv, src/connection/mod.rs:769-842, 660-687). The
// per-entry and per-buffer arithmetic is mq_stream_data.h, shared with the host test.
//
// Which map slot and which buffer a stream gets depends on the order in which ids first appear, and
// what a frame copies on what the frames before it left, so it is the sequential replay per connection
// that has to come out:
//   select   one thread per record: key = conn, or n_conns where the record is not selected; a flag;
//            the arena offset of the record's data
//   scan     exclusive sum of the flags (hipcub): a selected record's event index, so events come out
//            in record order; the last entry is *n_evts
//   sort     stable radix sort of (key, record index) over the bits of n_conns (hipcub): each
//            connection's records become contiguous, still in arrival order
//   replay   32 lanes per connection, lane s holding map slot s and buffer slot s. The group finds its
//            run by binary search over the sorted keys, loads it 32 records at a time (lane i record i
//            of the chunk) and applies the records in turn from lane broadcasts: "find id" and "first
//            free" are one ballot each over map and buffers, the updates are lane-local on the owning
//            lane, lane 0 writes the event at its scanned index.
//   copy     the events with copy_len > 0 have disjoint destinations: kCopyLanes lanes per event move
//            16-byte chunks at any alignment, four loads in flight per lane before their stores, and a
//            byte-exact tail.
// mq_batch_stream_read: mark (a request's claim word becomes "free"), claim (atomicMin of the request
// index on the claim word of its buffer), serve (the winner answers and copies with the same routine).
// The claim's minimum does not depend on arrival order, so every output is a function of the inputs.
#include "mq_launch.h"
#include "mq_replay.h"
#include "mq_stream_data.h"

#ifndef MQ_STREAM_COPY_LANES
#define MQ_STREAM_COPY_LANES 32  // lanes per copied event: 16, 32 or 64 (DESIGN.md §4.4 has the comparison)
#endif

namespace mq {

constexpr uint32_t kSdBlock = 256;
constexpr uint32_t kSdGroup = 32;  // lanes per connection: one map slot and one buffer slot each
constexpr uint32_t kSdGroupsPerBlock = kSdBlock / kSdGroup;
constexpr uint32_t kCopyLanes = MQ_STREAM_COPY_LANES;
constexpr uint32_t kCopyDepth = 4;  // 16-byte loads in flight per lane
static_assert(kSdGroup == kStreamSlots, "one lane per slot");
static_assert(kCopyLanes == 16 || kCopyLanes == 32 || kCopyLanes == 64, "a power of two inside the wave");
static_assert(sizeof(mq_stream_entry) == 48 && sizeof(mq_stream_buf) == 32 && sizeof(mq_conn_streams) == 2592 &&
                  sizeof(mq_stream_evt) == 32 && sizeof(mq_stream_read_req) == 32 && sizeof(mq_stream_read_res) == 8 &&
                  sizeof(mq_frame) == 48,
              "ABI");
static_assert(MQ_STREAM_SLOTS == kStreamSlots && MQ_STREAM_WOULD_BLOCK == kStreamWouldBlock, "ABI constants");

struct StreamDataWs : SortWs {              // max_frames each
  uint32_t *flags, *pos;                    // max_frames + 1: selected, their exclusive scan
  uint64_t* src;                            // max_frames: arena offset of a selected STREAM record's data
  void* cub;
  size_t cub_bytes;
};
struct StreamReadWs {
  uint32_t* claim;  // 32 n_conns: lowest request index per (connection, buffer slot)
  uint32_t* slot;   // n_reqs: 0..31, kStreamNone, or kReadInvalid
};
constexpr uint32_t kReadInvalid = 0xFE;
using SdLanes = LaneGroup<kSdGroup>;

// ---- the copy routine: n bytes, any alignment on both sides, nothing outside [dst, dst + n) written ----
template <uint32_t kLanes>
__device__ __forceinline__ void sd_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n,
                                        uint32_t lane) {
  const uint32_t chunks = n >> 4;
  for (uint32_t c = lane; c < chunks; c += kCopyDepth * kLanes) {
    uint4 v[kCopyDepth];
#pragma unroll
    for (uint32_t q = 0; q < kCopyDepth; ++q) {
      if (c + q * kLanes < chunks) v[q] = ld16(src + 16ull * (c + q * kLanes));
    }
#pragma unroll
    for (uint32_t q = 0; q < kCopyDepth; ++q) {
      if (c + q * kLanes < chunks) *(uint4_u*)(dst + 16ull * (c + q * kLanes)) = v[q];
    }
  }
  const uint32_t t = (chunks << 4) + lane;  // the tail: fewer than 16 bytes, one per lane
  if (lane < 16 && t < n) dst[t] = src[t];
}

__device__ __forceinline__ void sd_load_entry(const mq_stream_entry* p, StreamEntry& e) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1], c = q[2];
  e.id = a.x | (uint64_t)a.y << 32, e.recv_offset = a.z | (uint64_t)a.w << 32;
  e.recv_max_data = b.x | (uint64_t)b.y << 32, e.recv_max_data_next = b.z | (uint64_t)b.w << 32;
  e.fin_offset = c.x | (uint64_t)c.y << 32;
  e.flags = (uint8_t)c.z, e.recv_state = (uint8_t)(c.z >> 8);
}
__device__ __forceinline__ void sd_store_entry(mq_stream_entry* p, const StreamEntry& e) {  // not the reserved bytes
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4((uint32_t)e.id, (uint32_t)(e.id >> 32), (uint32_t)e.recv_offset, (uint32_t)(e.recv_offset >> 32));
  q[1] = make_uint4((uint32_t)e.recv_max_data, (uint32_t)(e.recv_max_data >> 32), (uint32_t)e.recv_max_data_next,
                    (uint32_t)(e.recv_max_data_next >> 32));
  p->fin_offset = e.fin_offset;
  p->flags = e.flags, p->recv_state = e.recv_state;
}
__device__ __forceinline__ void sd_load_buf(const mq_stream_buf* p, StreamBuf& b, uint32_t stream_buf) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], c = q[1];
  b.stream_id = a.x | (uint64_t)a.y << 32, b.next_offset = a.z | (uint64_t)a.w << 32;
  b.len = c.x, b.read_offset = c.y;
  b.used = (uint8_t)c.z, b.fin_received = (uint8_t)(c.z >> 8);
  stream_buf_clamp(b, stream_buf);
}
__device__ __forceinline__ void sd_store_buf(mq_stream_buf* p, const StreamBuf& b) {  // not the reserved bytes
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4((uint32_t)b.stream_id, (uint32_t)(b.stream_id >> 32), (uint32_t)b.next_offset,
                    (uint32_t)(b.next_offset >> 32));
  p->len = b.len, p->read_offset = b.read_offset;
  p->used = b.used, p->fin_received = b.fin_received;
}

}  // namespace mq

using namespace mq;

// select: which records are processed, for which connection, and where their data starts
__global__ __launch_bounds__(kSdBlock) void mq_stream_select_kernel(StreamDataArgs a, StreamDataWs ws) {
  const uint32_t k = blockIdx.x * kSdBlock + threadIdx.x;
  if (k > a.max_frames) return;
  if (k == a.max_frames) {
    ws.flags[k] = 0;
    return;
  }
  const uint32_t nf = *a.n_frames_dev, np = *a.n_pkts_dev;
  const uint32_t n_frames = nf < a.max_frames ? nf : a.max_frames, n_pkts = np < a.max_pkts ? np : a.max_pkts;
  uint32_t key = a.n_conns;
  uint64_t src = 0;
  if (k < n_frames) {
    const uint4 f = reinterpret_cast<const uint4*>(a.frames + k)[0];  // pkt; pos, len; type, level, data_pos; data_len, aux
    const uint32_t type = f.z & 0xFFu, data_pos = f.z >> 16, data_len = f.w & 0xFFFFu;
    if (type == 0x04 || (type >= 0x08 && type <= 0x0f)) {
      const FrameSite site =
          frame_site(a.pkts, n_pkts, a.dgrams, a.n_dgrams, a.arena_len, f.x, data_pos, data_len, type != 0x04);
      src = site.src;
      if (site.conn < a.n_conns && site.inside) key = site.conn;
    }
  }
  ws.keys_in[k] = key;
  ws.idx_in[k] = k;
  ws.flags[k] = key < a.n_conns;
  ws.src[k] = src;
}

// replay: every connection's selected records, in record order. Its arguments stay a flat __restrict__ list:
// with the argument struct the replay over 64 long connections measured 1.3 % slower
__global__ __launch_bounds__(kSdBlock) void mq_stream_replay_kernel(
    const mq_frame* __restrict__ frames, uint32_t max_frames, mq_conn_streams* __restrict__ streams, uint32_t n_conns,
    uint32_t stream_buf, uint64_t initial_max, uint32_t call_flags, mq_stream_evt* __restrict__ evts,
    uint32_t* __restrict__ n_evts, StreamDataWs ws) {
  const uint32_t c = blockIdx.x * kSdGroupsPerBlock + threadIdx.x / kSdGroup;
  const uint32_t lane = SdLanes::lane();
  const uint32_t group_first = SdLanes::first();
  const bool is_client = (call_flags & MQ_STREAMS_CLIENT) != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_evts = ws.pos[max_frames];
  uint32_t r = 0, r_end = 0;
  if (c < n_conns) key_run(ws.keys, max_frames, c, r, r_end);  // the connection's run
  const bool touched = r < r_end;
  StreamEntry e = {};
  StreamBuf b = {};
  uint64_t max_bidi = 0, max_uni = 0;
  if (touched) {
    sd_load_entry(&streams[c].map[lane], e);
    sd_load_buf(&streams[c].buf[lane], b, stream_buf);
    max_bidi = streams[c].max_bidi_remote, max_uni = streams[c].max_uni_remote;
  }
  // `on` is the same in all lanes of a group, so every branch on it is uniform inside the group, and a
  // cross-lane step reads lanes of its own group only; both groups of the wave take every step
  while (__builtin_amdgcn_ballot_w64(r < r_end) != 0) {
    const uint32_t cnt = r < r_end ? (r_end - r < kSdGroup ? r_end - r : kSdGroup) : 0u;
    uint32_t my_k = 0, my_type = 0, my_len = 0, my_pos = 0;
    uint64_t my_id = 0, my_a = 0, my_src = 0;
    if (lane < cnt) {  // lane i takes record i of the chunk
      my_k = ws.idx[r + lane];
      const uint4* f = reinterpret_cast<const uint4*>(frames + my_k);
      const uint4 h = f[0], v01 = f[1];
      my_type = h.z & 0xFFu, my_len = h.w & 0xFFFFu;
      my_id = v01.x | (uint64_t)v01.y << 32;
      if (my_type == 0x04) my_a = frames[my_k].v[2], my_len = 0;
      else my_a = v01.z | (uint64_t)v01.w << 32;
      my_src = ws.src[my_k];
      my_pos = ws.pos[my_k];  // the event index: < the number selected <= max_frames
    }
    for (uint32_t j = 0; j < kSdGroup; ++j) {
      const bool on = j < cnt;
      if (__builtin_amdgcn_ballot_w64(on) == 0) break;  // the longer chunk of the wave's two groups
      const uint32_t k = SdLanes::get32(my_k, j), type = SdLanes::get32(my_type, j), len = SdLanes::get32(my_len, j);
      const uint32_t pos = SdLanes::get32(my_pos, j);
      const uint64_t id = SdLanes::get64(my_id, j), a = SdLanes::get64(my_a, j), src = SdLanes::get64(my_src, j);
      const bool is_stream = type >= 0x08, fin = (type & 1u) != 0;
      const bool m_used = (e.flags & kSeUsed) != 0;
      const uint32_t m_found = SdLanes::ballot(on && m_used && e.id == id, group_first);
      const uint32_t m_free = SdLanes::ballot(on && !m_used, group_first);
      const uint32_t b_found = SdLanes::ballot(on && b.used && b.stream_id == id, group_first);
      uint32_t mslot = kStreamNone, bslot = kStreamNone, ev_flags = 0;
      if (m_found) {
        mslot = (uint32_t)__builtin_ctz(m_found);
      } else if (on && is_stream && stream_peer_initiated(id, is_client) && m_free) {
        mslot = (uint32_t)__builtin_ctz(m_free);
        if (lane == mslot) stream_entry_create(e, id, initial_max);
        if (stream_bidirectional(id)) max_bidi = stream_raise_remote(max_bidi, id);
        else max_uni = stream_raise_remote(max_uni, id);
        ev_flags |= kEvNewStream;
      }
      const bool have = on && mslot != kStreamNone;
      uint32_t mark_l = 0xFF;
      if (have && lane == mslot) mark_l = is_stream ? stream_mark_recv(e, a, len, fin) : stream_handle_reset(e, a);
      const uint32_t mark_got = SdLanes::get32(mark_l, mslot);
      const uint32_t mark = have ? mark_got : 0xFFu;
      if (have) ev_flags |= is_stream ? kEvReadable : kEvReset;
      // store_stream_data
      const bool storing = have && is_stream;
      const uint32_t b_free = SdLanes::ballot(on && !b.used, group_first);
      uint32_t store = kStoreNone;
      if (storing) {
        if (b_found) {
          bslot = (uint32_t)__builtin_ctz(b_found);
        } else if (b_free) {
          bslot = (uint32_t)__builtin_ctz(b_free);
          if (lane == bslot) stream_buf_init(b, id);
          ev_flags |= kEvNewBuf;
        } else {
          store = kStoreNoBuffer;
        }
      }
      uint32_t pack_l = 0, dst_l = 0;  // store | flags << 8 | skip << 16; copy_len; dst
      uint32_t n_l = 0;
      if (storing && lane == bslot) {
        const StreamStore s = stream_store(b, a, len, fin, stream_buf);
        pack_l = s.store | (uint32_t)s.flags << 8 | (uint32_t)s.skip << 16;
        n_l = s.copy_len, dst_l = s.dst;
      }
      const uint32_t pack = SdLanes::get32(pack_l, bslot), n = SdLanes::get32(n_l, bslot), dst = SdLanes::get32(dst_l, bslot);
      if (on && lane == 0) {
        uint32_t skip = 0, copy_len = 0, at = 0;
        uint64_t from = 0;
        if (storing && bslot != kStreamNone) {
          store = pack & 0xFFu, ev_flags |= (pack >> 8) & 0xFFu;
          if (store == kStoreCopied) skip = pack >> 16, copy_len = n, at = dst, from = src + skip;
        }
        uint4* q = reinterpret_cast<uint4*>(evts + pos);
        q[0] = make_uint4(k, c, (uint32_t)from, (uint32_t)(from >> 32));
        q[1] = make_uint4(at, copy_len | skip << 16, mslot | bslot << 8 | mark << 16 | store << 24, ev_flags | type << 8);
      }
    }
    r += cnt;
  }
  if (!touched) return;  // a connection without records is left as it is
  sd_store_entry(&streams[c].map[lane], e);
  sd_store_buf(&streams[c].buf[lane], b);
  if (lane == 0) streams[c].max_bidi_remote = max_bidi, streams[c].max_uni_remote = max_uni;
}

// copy: kCopyLanes lanes per event
__global__ __launch_bounds__(kSdBlock) void mq_stream_copy_kernel(const uint8_t* __restrict__ arena,
                                                                  const mq_stream_evt* __restrict__ evts,
                                                                  uint32_t max_frames, uint8_t* __restrict__ bufs,
                                                                  uint32_t stream_buf, StreamDataWs ws) {
  const uint64_t i = ((uint64_t)blockIdx.x * kSdBlock + threadIdx.x) / kCopyLanes;
  if (i >= ws.pos[max_frames]) return;
  const uint4* q = reinterpret_cast<const uint4*>(evts + i);
  const uint4 a = q[0], b = q[1];
  const uint32_t copy_len = b.y & 0xFFFFu, bslot = (b.z >> 8) & 0xFFu;
  if (copy_len == 0 || (b.z >> 24) != kStoreCopied) return;
  const uint64_t src = a.z | (uint64_t)a.w << 32;
  // dst + copy_len <= stream_buf by stream_store; conn < n_conns and bslot < 32 by the replay
  uint8_t* to = bufs + ((uint64_t)a.y * kStreamSlots + bslot) * stream_buf + b.x;
  sd_copy<kCopyLanes>(to, arena + src, copy_len, threadIdx.x & (kCopyLanes - 1));
}

// ---- mq_batch_stream_read -----------------------------------------------------------------------------
// mark: which buffer a request names; its claim word becomes "free"
__global__ __launch_bounds__(kSdBlock) void mq_stream_read_mark_kernel(StreamReadArgs args, StreamReadWs ws) {
  const uint32_t k = blockIdx.x * kSdBlock + threadIdx.x;
  if (k >= args.n_reqs) return;
  const uint4 a = reinterpret_cast<const uint4*>(args.reqs + k)[0];  // conn, cap, stream_id
  const uint64_t id = a.z | (uint64_t)a.w << 32, out_offset = args.reqs[k].out_offset;
  uint32_t slot = kReadInvalid;
  if (a.x < args.n_conns && out_offset <= args.out_len && a.y <= args.out_len - out_offset) {
    slot = kStreamNone;
    for (uint32_t s = 0; s < kStreamSlots; ++s) {
      const mq_stream_buf* p = &args.streams[a.x].buf[s];
      if (p->used && p->stream_id == id) {
        slot = s;
        break;
      }
    }
    if (slot != kStreamNone) ws.claim[(uint64_t)a.x * kStreamSlots + slot] = 0xFFFFFFFFu;
  }
  ws.slot[k] = slot;
}

// claim: the lowest request index per buffer
__global__ __launch_bounds__(kSdBlock) void mq_stream_read_claim_kernel(const mq_stream_read_req* __restrict__ reqs,
                                                                        uint32_t n_reqs, StreamReadWs ws) {
  const uint32_t k = blockIdx.x * kSdBlock + threadIdx.x;
  if (k >= n_reqs) return;
  const uint32_t slot = ws.slot[k];
  if (slot < kStreamSlots) atomicMin(&ws.claim[(uint64_t)reqs[k].conn * kStreamSlots + slot], k);
}

// serve: kCopyLanes lanes per request
__global__ __launch_bounds__(kSdBlock) void mq_stream_read_serve_kernel(StreamReadArgs args, StreamReadWs ws) {
  const uint64_t k = ((uint64_t)blockIdx.x * kSdBlock + threadIdx.x) / kCopyLanes;
  if (k >= args.n_reqs) return;
  const uint32_t lane = threadIdx.x & (kCopyLanes - 1);
  const uint32_t slot = ws.slot[k];
  const uint4 a = reinterpret_cast<const uint4*>(args.reqs + k)[0];
  uint32_t status = MQ_OK, copied = 0, fin = 0;
  if (slot == kReadInvalid) {
    status = MQ_ERR_INVALID_ARG;
  } else if (slot == kStreamNone) {
    status = kStreamWouldBlock;
  } else if (ws.claim[(uint64_t)a.x * kStreamSlots + slot] != (uint32_t)k) {
    status = MQ_ERR_DEFERRED;
  } else {
    mq_stream_buf* p = &args.streams[a.x].buf[slot];
    StreamBuf b;
    sd_load_buf(p, b, args.stream_buf);  // every lane of the request holds the header before lane 0 writes it
    const StreamRead r = stream_read(b, a.y);
    status = r.status, copied = r.copied, fin = r.fin;
    if (copied) {
      sd_copy<kCopyLanes>(args.out + args.reqs[k].out_offset,
                          args.bufs + ((uint64_t)a.x * kStreamSlots + slot) * args.stream_buf + r.from, copied, lane);
    }
    if (lane == 0 && status == MQ_OK) p->len = b.len, p->read_offset = b.read_offset, p->used = b.used;
  }
  if (lane == 0) {
    const uint32_t s = slot < kStreamSlots ? slot : kStreamNone;
    *reinterpret_cast<uint2*>(args.res + k) = make_uint2(copied, status | fin << 8 | s << 16);
  }
}

// ---- host side -----------------------------------------------------------------------------------------
namespace {
size_t stream_data_layout(uint32_t n, uint32_t n_conns, void* base, StreamDataWs& w) {
  Carve c(base);
  w.keys_in = c.take<uint32_t>(n);
  w.keys = c.take<uint32_t>(n);
  w.idx_in = c.take<uint32_t>(n);
  w.idx = c.take<uint32_t>(n);
  w.flags = c.take<uint32_t>((size_t)n + 1);
  w.pos = c.take<uint32_t>((size_t)n + 1);
  w.src = c.take<uint64_t>(n);
  w.cub_bytes = cub_temp_bytes<true>(n, key_bits(n_conns), {n + 1});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes();  // no slack behind the last piece, unlike stream read
}
size_t stream_read_layout(uint32_t n_reqs, uint32_t n_conns, void* base, StreamReadWs& w) {
  Carve c(base);
  w.claim = c.take<uint32_t>((size_t)kStreamSlots * n_conns);
  w.slot = c.take<uint32_t>(n_reqs);
  // 256 bytes that no kernel touches. Nobody knows why they are there; callers size by this figure
  return c.bytes() + 256;
}
dim3 sd_blocks(uint64_t threads) { return dim3((uint32_t)((threads + kSdBlock - 1) / kSdBlock)); }
}  // namespace

size_t mq_stream_data_workspace(uint32_t max_frames, uint32_t n_conns) {
  StreamDataWs w = {};
  return stream_data_layout(max_frames, n_conns, nullptr, w);
}
size_t mq_stream_read_workspace(uint32_t n_reqs, uint32_t n_conns) {
  StreamReadWs w = {};
  return stream_read_layout(n_reqs, n_conns, nullptr, w);
}

// max_frames > 0 and n_conns > 0
hipError_t mq_launch_stream_data(const StreamDataArgs& a, void* workspace, hipStream_t s) {
  StreamDataWs w = {};
  stream_data_layout(a.max_frames, a.n_conns, workspace, w);
  hipError_t e;
  const dim3 block(kSdBlock);
  hipLaunchKernelGGL(mq_stream_select_kernel, sd_blocks((uint64_t)a.max_frames + 1), block, 0, s, a, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(w, w.flags, w.pos, a.max_frames + 1, s)) != hipSuccess) return e;
  if ((e = sort_by_key(w, a.max_frames, key_bits(a.n_conns), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_stream_replay_kernel, sd_blocks((uint64_t)a.n_conns * kSdGroup), block, 0, s, a.frames,
                     a.max_frames, a.streams, a.n_conns, a.stream_buf, a.initial_max_stream_data, a.flags, a.evts, a.n_evts,
                     w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_stream_copy_kernel, sd_blocks((uint64_t)a.max_frames * kCopyLanes), block, 0, s, a.arena, a.evts,
                     a.max_frames, a.bufs, a.stream_buf, w);
  return hipGetLastError();
}

// n_reqs > 0
hipError_t mq_launch_stream_read(const StreamReadArgs& a, void* workspace, hipStream_t s) {
  StreamReadWs w = {};
  stream_read_layout(a.n_reqs, a.n_conns, workspace, w);
  hipError_t e;
  const dim3 block(kSdBlock);
  hipLaunchKernelGGL(mq_stream_read_mark_kernel, sd_blocks(a.n_reqs), block, 0, s, a, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_stream_read_claim_kernel, sd_blocks(a.n_reqs), block, 0, s, a.reqs, a.n_reqs, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_stream_read_serve_kernel, sd_blocks((uint64_t)a.n_reqs * kCopyLanes), block, 0, s, a, w);
  return hipGetLastError();
}
