// mq_replay.h — the "replay per connection" recipe that the stages behind mq_batch_frames share
// (mq_acks.hip, mq_stream_data.hip, mq_recovery.hip; DESIGN.md has the recipe once):
//   select   key every item by its connection, "none" = the first key above the range
//   scan     exclusive sum of a flag array (exclusive_sum)
//   sort     stable radix sort of (key, index) over key_bits of the range (sort_by_key): a
//            connection's items become one run, still in arrival order
//   replay   a lane group per connection finds its run (key_run), loads it one chunk at a time
//            (lane i item i) and applies the items in turn from lane broadcasts (LaneGroup)
// HIP only: mq_acks.h, mq_stream_data.h and mq_recovery.h stay free of it for their host tests.
#ifndef MQ_REPLAY_H
#define MQ_REPLAY_H

#include <hipcub/hipcub.hpp>

#include <initializer_list>
#include <type_traits>

#include "mq_device.h"
#include "mq_workspace.h"

namespace mq {

// ---- device side -------------------------------------------------------------------------------------------
// W consecutive lanes of a wave, W = 32 or 64. group_first is the wave lane the group starts at
// (first()); a whole wave has none to pass.
template <uint32_t W>
struct LaneGroup {
  static_assert(W == 32 || W == 64, "half a wave or a whole one");
  using Mask = std::conditional_t<W == 64, uint64_t, uint32_t>;

  static __device__ __forceinline__ uint32_t lane() { return threadIdx.x & (W - 1); }
  static __device__ __forceinline__ uint32_t first() { return threadIdx.x & (kWave - 1) & ~(W - 1); }
  // bit i: the predicate of the group's lane i. Every lane of the wave must call it.
  static __device__ __forceinline__ Mask ballot(bool p, uint32_t group_first = 0) {
    return (Mask)(__builtin_amdgcn_ballot_w64(p) >> group_first);
  }
  // the value of the group's lane `src` (any value is taken modulo W)
  static __device__ __forceinline__ uint32_t get32(uint32_t v, uint32_t src) {
    return (uint32_t)__shfl((int)v, (int)(src & (W - 1)), (int)W);
  }
  static __device__ __forceinline__ uint64_t get64(uint64_t v, uint32_t src) {
    return get32((uint32_t)v, src) | (uint64_t)get32((uint32_t)(v >> 32), src) << 32;
  }
  // set bits of a group mask below this lane, and in all of it
  static __device__ __forceinline__ uint32_t below(Mask m) {
    if constexpr (W == 64) return lanes_below(m);
    else return (uint32_t)__builtin_popcount(m & ((1u << lane()) - 1u));
  }
  static __device__ __forceinline__ uint32_t count(Mask m) { return (uint32_t)__builtin_popcountll(m); }
};

// the run of `key` in the ascending keys[0, n): [lower bound of key, lower bound of key + 1)
__device__ __forceinline__ void key_run(const uint32_t* __restrict__ keys, uint32_t n, uint32_t key, uint32_t& r,
                                        uint32_t& r_end) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  r = lo, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  r_end = lo;
}

// Where a frame record's data lies: record -> packet -> datagram -> connection.
struct FrameSite {
  uint32_t dgram, conn;  // conn is the datagram's, not yet compared with n_conns
  uint64_t src;          // arena offset of the data
  bool inside;           // [src, src + data_len) lies inside the arena, or the data is not read
};
// conn = MQ_CONN_NONE (above every n_conns) and src = 0 where the record names no packet below n_pkts
// or the packet no datagram below n_dgrams. has_data: the stage reads the record's data bytes.
__device__ __forceinline__ FrameSite frame_site(const mq_recv_pkt* __restrict__ pkts, uint32_t n_pkts,
                                                const mq_dgram* __restrict__ dgrams, uint32_t n_dgrams,
                                                uint64_t arena_len, uint32_t pkt, uint32_t data_pos,
                                                uint32_t data_len, bool has_data) {
  FrameSite s = {0, MQ_CONN_NONE, 0, false};
  if (pkt < n_pkts) {
    const uint4 a = reinterpret_cast<const uint4*>(pkts + pkt)[0];  // offset, pn
    const uint4 b = reinterpret_cast<const uint4*>(pkts + pkt)[1];  // len, dgram, payload_offset + level + status, ..
    if (b.y < n_dgrams) {
      s.dgram = b.y, s.conn = dgrams[b.y].conn;
      const uint64_t off = a.x | (uint64_t)a.y << 32;
      const uint32_t rel = (b.z & 0xFFFFu) + data_pos;
      s.src = off + rel;
      // no wrap: the sum is compared piece by piece
      s.inside = !has_data || (off <= arena_len && rel <= arena_len - off && data_len <= arena_len - off - rel);
    }
  }
  return s;
}

// ---- host side ---------------------------------------------------------------------------------------------
// The sort's four arrays, n each. A stage's workspace struct starts with them and ends with
// `void* cub; size_t cub_bytes;`, the hipcub temporary storage that sort_by_key and exclusive_sum take.
struct SortWs {
  uint32_t *keys_in, *keys, *idx_in, *idx;
};

// hipcub temporary storage for the largest of: one sort of sort_n pairs over sort_bits bits (kSort),
// and one exclusive sum per entry of scan_ns. A template, so that a file without a sort (frames,
// route) does not get the sort's kernels
template <bool kSort>
size_t cub_temp_bytes(uint32_t sort_n, uint32_t sort_bits, std::initializer_list<uint32_t> scan_ns) {
  size_t most = 0, b = 0;
  if constexpr (kSort) {
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, most, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)sort_n, 0, (int)sort_bits);
  }
  for (const uint32_t n : scan_ns) {
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    if (b > most) most = b;
  }
  return most;
}

// (keys_in, idx_in) -> (keys, idx), stable, over the low `bits` bits
template <class Ws>
hipError_t sort_by_key(const Ws& w, uint32_t n, uint32_t bits, hipStream_t s) {
  size_t cb = w.cub_bytes;
  return hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.keys_in, w.keys, w.idx_in, w.idx, (int)n, 0, (int)bits, s);
}
template <class Ws>
hipError_t exclusive_sum(const Ws& w, uint32_t* in, uint32_t* out, uint32_t n, hipStream_t s) {
  size_t cb = w.cub_bytes;
  return hipcub::DeviceScan::ExclusiveSum(w.cub, cb, in, out, (int)n, s);
}

}  // namespace mq

#endif
