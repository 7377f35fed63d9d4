// mq_acks.hip — mq_batch_acks: received-PN trackers and ACK frames on the device, behind
// mq_batch_frames (track_received_pn -> RecvPnTracker::record, reference src/connection/recv.rs:248-249,
// mod.rs:224-296; build_ack_frame, transmit.rs:321-380). The per-tracker arithmetic is mq_acks.h,
// shared with the host test.
//
// The tracker's result depends on arrival order once its 32 ranges are in use, so it is the
// sequential replay that has to come out — but not in 2^20 dependent steps:
//   key      a packet's key is 3 conn + level, or "none" (= 3 n_conns) where it is not recorded
//   sort     stable radix sort of (key, index) over the bits of 3 n_conns (hipcub): each tracker's
//            packets become contiguous, still in arrival order
//   flag     position j starts a run unless j - 1 has the same key and the packet number before it
//   scan     exclusive sum of the flags (hipcub); the last entry is the number of runs
//   runs     (key, first PN, last PN) per run, in sorted order
//   replay   32 lanes per tracker, one range per lane. The lanes find their tracker's runs with a
//            binary search over the run keys and apply them in turn: record(first) is three ballots
//            and a lane shift, the rest of the run one more ballot and shift (mq_acks.h,
//            ack_record_run). A connection in order is one run, whatever its length.
//   due      one thread per connection: pending |= conn_flags & 7; which levels are due
//   scan     exclusive sum of the due counts: ACK k, in (conn, level) order
//   build    32 lanes per connection, level by level: lane r sizes the (gap, range) pair of range r, a
//            prefix sum over the lanes places it, each lane stores its own bytes; lane 0 writes the
//            request. The same grid writes the null requests behind the last ACK.
// Every output is a function of the inputs: no atomics.
#include "mq_replay.h"  // first: mq_acks.h needs the HIP runtime's qualifiers

#include "mq_acks.h"
#include "mq_launch.h"

namespace mq {

constexpr uint32_t kAckBlock = 256;
constexpr uint32_t kAckGroup = 32;  // lanes per tracker: one range each
constexpr uint32_t kAckGroupsPerBlock = kAckBlock / kAckGroup;
static_assert(kAckGroup == kAckRanges, "one lane per range");
static_assert(sizeof(mq_pn_tracker) == 528 && sizeof(mq_send_req) == 48 && sizeof(mq_recv_pkt) == 32, "ABI");

struct AcksWs : SortWs {                    // max_pkts each
  uint32_t *flags, *pos;                    // max_pkts + 1: run starts, their exclusive scan
  uint32_t* run_key;                        // max_pkts
  uint64_t *run_first, *run_last;           // max_pkts
  uint32_t *due, *base;                     // n_conns + 1: due levels per connection, their exclusive scan
  void* cub;
  size_t cub_bytes;
};

using AckLanes = LaneGroup<kAckGroup>;

// One tracker over the group: lane r holds range r; n is the same in all lanes.
struct LaneTracker {
  uint64_t s, e;
  uint32_t n;
  uint32_t lane, group_first;

  __device__ __forceinline__ bool valid() const { return lane < n; }
  // lanes >= from take the range of lane + k
  __device__ __forceinline__ void close_up(uint32_t from, uint32_t k) {
    const uint64_t ns = AckLanes::get64(s, lane + k), ne = AckLanes::get64(e, lane + k);
    if (lane >= from) s = ns, e = ne;
    n -= k;
  }
  // ack_record_run of mq_acks.h. `on` is the same in all lanes of the group, so every branch is uniform
  // inside the group, and a cross-lane step reads lanes of its own group only: the wave's other group
  // may be in another branch
  __device__ __forceinline__ void record_run(bool on, uint64_t first, uint64_t last) {
    const uint32_t in = AckLanes::ballot(on && valid() && ack_contains(s, e, first), group_first);
    const uint32_t up = AckLanes::ballot(on && valid() && ack_extends_up(e, first), group_first);
    const uint32_t down = AckLanes::ballot(on && valid() && ack_extends_down(s, first), group_first);
    uint32_t at;
    if (in) {
      at = (uint32_t)__builtin_ctz(in);
    } else if (up && down) {  // first bridges range `at` and the one above it
      at = (uint32_t)__builtin_ctz(up);
      const uint32_t ri = (uint32_t)__builtin_ctz(down);
      const uint64_t re = AckLanes::get64(e, ri);
      if (lane == at) e = re;
      close_up(ri, 1);
    } else if (up) {
      at = (uint32_t)__builtin_ctz(up);
      if (lane == at) e = first;
    } else if (down) {
      at = (uint32_t)__builtin_ctz(down);
      if (lane == at) s = first;
    } else {  // a new stand-alone range; a full tracker loses its lowest range first
      if (on && n == kAckRanges) close_up(0, 1);
      const uint32_t above = AckLanes::ballot(on && valid() && s > first, group_first);
      at = above ? (uint32_t)__builtin_ctz(above) : n;
      const uint64_t ps = AckLanes::get64(s, lane - 1), pe = AckLanes::get64(e, lane - 1);
      if (on) {
        if (lane > at) s = ps, e = pe;
        if (lane == at) s = e = first;
        ++n;
      }
    }
    // the rest of the run: range `at` rises to `last` and takes in the ranges it now reaches
    uint64_t end = AckLanes::get64(e, at);
    if (last > end) end = last;
    const uint32_t reach = AckLanes::ballot(on && valid() && lane > at && s <= end + 1, group_first);
    const uint32_t k = (uint32_t)__builtin_popcount(reach);
    const uint64_t top = AckLanes::get64(e, at + k);  // the last range taken in holds the largest end
    if (k && top > end) end = top;
    if (on && lane == at) e = end;
    if (k) close_up(at + 1, k);
  }
};

}  // namespace mq

using namespace mq;

// key: which tracker a packet is recorded in
__global__ __launch_bounds__(kAckBlock) void mq_acks_key_kernel(AcksArgs a, AcksWs ws) {
  const uint32_t i = blockIdx.x * kAckBlock + threadIdx.x;
  if (i >= a.max_pkts) return;
  const uint32_t n_dev = *a.n_pkts_dev;
  const uint32_t n_pkts = n_dev < a.max_pkts ? n_dev : a.max_pkts;
  uint32_t key = 3u * a.n_conns;
  if (i < n_pkts) {
    const uint4 b = reinterpret_cast<const uint4*>(a.pkts + i)[1];  // len, dgram, payload_offset + level + status, ..
    const uint32_t level = (b.z >> 16) & 0xFFu, status = b.z >> 24;
    bool ok = status == MQ_OK && level < 3 && b.y < a.n_dgrams;
    if (ok && a.summary) ok = a.summary[i].status == MQ_OK;
    if (ok) {
      const uint32_t c = a.dgrams[b.y].conn;
      if (c < a.n_conns) key = 3u * c + level;
    }
  }
  ws.keys_in[i] = key;
  ws.idx_in[i] = i;
}

// flag: run starts over the sorted order
__global__ __launch_bounds__(kAckBlock) void mq_acks_flag_kernel(const mq_recv_pkt* __restrict__ pkts, uint32_t max_pkts,
                                                                 uint32_t n_conns, AcksWs ws) {
  const uint32_t j = blockIdx.x * kAckBlock + threadIdx.x;
  if (j > max_pkts) return;
  uint32_t f = 0;
  if (j < max_pkts) {
    const uint32_t key = ws.keys[j];
    if (key < 3u * n_conns) {
      f = 1;
      if (j > 0 && ws.keys[j - 1] == key && pkts[ws.idx[j]].pn == pkts[ws.idx[j - 1]].pn + 1) f = 0;
    }
  }
  ws.flags[j] = f;
}

// runs: (key, first PN, last PN) per run
__global__ __launch_bounds__(kAckBlock) void mq_acks_runs_kernel(const mq_recv_pkt* __restrict__ pkts, uint32_t max_pkts,
                                                                 uint32_t n_conns, AcksWs ws) {
  const uint32_t j = blockIdx.x * kAckBlock + threadIdx.x;
  if (j >= max_pkts) return;
  const uint32_t key = ws.keys[j];
  if (key >= 3u * n_conns) return;
  const uint64_t pn = pkts[ws.idx[j]].pn;
  if (ws.flags[j]) {  // pos[j] < max_pkts: at most one run per packet
    ws.run_key[ws.pos[j]] = key;
    ws.run_first[ws.pos[j]] = pn;
  }
  if (j + 1 == max_pkts || ws.flags[j + 1] || ws.keys[j + 1] >= 3u * n_conns) ws.run_last[ws.pos[j + 1] - 1] = pn;
}

// replay: the runs of every tracker, in arrival order
__global__ __launch_bounds__(kAckBlock) void mq_acks_replay_kernel(mq_pn_tracker* __restrict__ trackers, uint32_t max_pkts,
                                                                   uint32_t n_conns, AcksWs ws) {
  const uint32_t t = blockIdx.x * kAckGroupsPerBlock + threadIdx.x / kAckGroup;
  LaneTracker tr;
  tr.lane = AckLanes::lane();
  tr.group_first = AckLanes::first();
  tr.s = tr.e = 0, tr.n = 0;
  const uint32_t n_runs = ws.pos[max_pkts];  // <= max_pkts
  // the tracker's first run. The walk below compares every run's key, which costs no more than the
  // search for the run's end would, so that end goes unused
  uint32_t r = n_runs, r_end;
  if (t < 3u * n_conns) key_run(ws.run_key, n_runs, t, r, r_end);
  bool on = r < n_runs && ws.run_key[r] == t;
  const bool touched = on;
  if (touched) {
    const uint32_t n = trackers[t].n;
    tr.n = n < kAckRanges ? n : kAckRanges;
    if (tr.valid()) tr.s = trackers[t].range[tr.lane][0], tr.e = trackers[t].range[tr.lane][1];
  }
  while (__builtin_amdgcn_ballot_w64(on) != 0) {  // both groups of the wave stay in step
    uint64_t first = 0, last = 0;
    if (on) first = ws.run_first[r], last = ws.run_last[r];
    tr.record_run(on, first, last);
    if (on) {
      ++r;
      on = r < n_runs && ws.run_key[r] == t;
    }
  }
  if (!touched) return;  // a tracker without packets is left as it is
  if (tr.lane == 0) trackers[t].n = tr.n;
  trackers[t].range[tr.lane][0] = tr.valid() ? tr.s : 0;
  trackers[t].range[tr.lane][1] = tr.valid() ? tr.e : 0;
}

// due: the pending bits, and which levels get an ACK
__global__ __launch_bounds__(kAckBlock) void mq_acks_due_kernel(const uint32_t* __restrict__ conn_flags,
                                                                const mq_pn_tracker* __restrict__ trackers,
                                                                uint32_t* __restrict__ ack_pending, uint32_t n_conns,
                                                                bool build, AcksWs ws) {
  const uint32_t c = blockIdx.x * kAckBlock + threadIdx.x;
  if (c > n_conns) return;
  if (c == n_conns) {
    if (build) ws.due[c] = 0;
    return;
  }
  uint32_t p = ack_pending[c];
  if (conn_flags) p |= conn_flags[c] & 7u;
  ack_pending[c] = p;
  if (!build) return;
  uint32_t due = 0;
  for (uint32_t l = 0; l < 3; ++l) {
    if ((p >> l & 1u) && trackers[3u * c + l].n != 0) ++due;
  }
  ws.due[c] = due;
}

struct AckSlot {
  uint8_t* p;
  __device__ __forceinline__ void operator()(uint32_t at, uint32_t b) const {
    if (at < kAckFrameMax) p[at] = (uint8_t)b;
  }
};

// build: the due ACK frames and their requests, in (conn, level) order; null requests behind them
__global__ __launch_bounds__(kAckBlock) void mq_acks_build_kernel(const mq_pn_tracker* __restrict__ trackers,
                                                                  uint32_t* __restrict__ ack_pending, uint32_t n_conns,
                                                                  mq_ack_build b, AcksWs ws) {
  const uint64_t gid = (uint64_t)blockIdx.x * kAckBlock + threadIdx.x;
  const uint32_t total = ws.base[n_conns];
  if (gid == 0) *b.n_acks = total;
  if (gid >= total && gid < b.max_acks) {  // a null request: mq_batch_protect answers it with INVALID_ARG
    uint4* q = reinterpret_cast<uint4*>(b.reqs + gid);
    q[0] = make_uint4(0, 0, 0, 0);
    q[1] = make_uint4(0, 0, 0, 0);
    q[2] = make_uint4(0, 0, MQ_CONN_NONE, 0);
  }
  const uint32_t lane = threadIdx.x & (kAckGroup - 1);
  const bool live = gid / kAckGroup < n_conns;
  const uint32_t c = live ? (uint32_t)(gid / kAckGroup) : 0u;
  uint32_t pending = live ? ack_pending[c] : 0u;
  uint32_t k = live ? ws.base[c] : 0u;
  for (uint32_t l = 0; l < 3; ++l) {
    const uint32_t t = 3u * c + l;
    uint32_t n = 0;
    if (live && (pending >> l & 1u)) {
      n = trackers[t].n;
      n = n < kAckRanges ? n : kAckRanges;
    }
    const bool due = n != 0;
    const bool on = due && k < b.max_acks;
    // lane r: range r and the start of the range above it
    uint64_t s = 0, e = 0;
    if (on && lane < n) s = trackers[t].range[lane][0], e = trackers[t].range[lane][1];
    const uint64_t next_start = AckLanes::get64(s, lane + 1);
    const uint32_t w = on && lane + 1 < n ? ack_pair_bytes(s, e, next_start) : 0u;
    // the pairs go out from range n - 2 down: lane r's pair lies behind those of the lanes above it
    uint32_t incl = w;
#pragma unroll
    for (uint32_t d = 1; d < kAckGroup; d <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, d, (int)kAckGroup);
      if (lane >= d) incl += v;
    }
    const uint32_t all = (uint32_t)__shfl((int)incl, (int)(kAckGroup - 1), (int)kAckGroup);
    if (on) {
      const uint64_t top_s = AckLanes::get64(s, n - 1), top_e = AckLanes::get64(e, n - 1);
      const uint32_t head = ack_head_bytes(n, top_s, top_e);
      AckSlot put = {b.ack_frames + (size_t)kAckFrameMax * k};
      if (lane + 1 == n) ack_head_put(put, n, s, e);
      else if (lane + 1 < n) ack_pair_put(put, head + (all - incl), s, e, next_start);
      if (lane == 0) {
        const uint64_t pn = b.next_pn[t];
        b.next_pn[t] = pn + 1;
        const uint64_t la = b.conns[c].largest_pn[l];
        const uint32_t flags = (l == MQ_LEVEL_INITIAL && (b.flags & MQ_ACKS_CLIENT)) ? MQ_SEND_PAD_TO_MIN : 0u;
        const uint64_t fo = (uint64_t)kAckFrameMax * k, oo = (uint64_t)b.out_stride * k;
        uint4* q = reinterpret_cast<uint4*>(b.reqs + k);
        q[0] = make_uint4((uint32_t)fo, (uint32_t)(fo >> 32), (uint32_t)oo, (uint32_t)(oo >> 32));
        q[1] = make_uint4((uint32_t)pn, (uint32_t)(pn >> 32), (uint32_t)la, (uint32_t)(la >> 32));
        q[2] = make_uint4(head + all, b.out_stride, c, l | flags << 8);
      }
      pending &= ~(1u << l);
    }
    if (due) ++k;
  }
  if (live && lane == 0) ack_pending[c] = pending;
}

// ---- host side -----------------------------------------------------------------------------------------
namespace {
size_t acks_layout(uint32_t n, uint32_t n_conns, void* base, AcksWs& w) {
  Carve c(base);
  w.keys_in = c.take<uint32_t>(n);
  w.keys = c.take<uint32_t>(n);
  w.idx_in = c.take<uint32_t>(n);
  w.idx = c.take<uint32_t>(n);
  w.flags = c.take<uint32_t>((size_t)n + 1);
  w.pos = c.take<uint32_t>((size_t)n + 1);
  w.run_key = c.take<uint32_t>(n);
  w.run_first = c.take<uint64_t>(n);
  w.run_last = c.take<uint64_t>(n);
  w.due = c.take<uint32_t>((size_t)n_conns + 1);
  w.base = c.take<uint32_t>((size_t)n_conns + 1);
  w.cub_bytes = cub_temp_bytes<true>(n, key_bits(3ull * n_conns), {n + 1, n_conns + 1});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes();  // no slack behind the last piece, unlike sent, recovery and stream read
}
}  // namespace

size_t mq_acks_workspace(uint32_t max_pkts, uint32_t n_conns) {
  AcksWs w = {};
  return acks_layout(max_pkts, n_conns, nullptr, w);
}

hipError_t mq_launch_acks(const AcksArgs& a, void* workspace, hipStream_t s) {
  AcksWs w = {};
  acks_layout(a.max_pkts, a.n_conns, workspace, w);
  hipError_t e;
  const dim3 block(kAckBlock);
  auto blocks = [](uint64_t threads) { return dim3((uint32_t)((threads + kAckBlock - 1) / kAckBlock)); };
  if (a.max_pkts && a.n_conns) {
    hipLaunchKernelGGL(mq_acks_key_kernel, blocks(a.max_pkts), block, 0, s, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_by_key(w, a.max_pkts, key_bits(3ull * a.n_conns), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(mq_acks_flag_kernel, blocks((uint64_t)a.max_pkts + 1), block, 0, s, a.pkts, a.max_pkts, a.n_conns, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_sum(w, w.flags, w.pos, a.max_pkts + 1, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(mq_acks_runs_kernel, blocks(a.max_pkts), block, 0, s, a.pkts, a.max_pkts, a.n_conns, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mq_acks_replay_kernel, blocks(3ull * a.n_conns * kAckGroup), block, 0, s, a.trackers, a.max_pkts,
                       a.n_conns, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(mq_acks_due_kernel, blocks((uint64_t)a.n_conns + 1), block, 0, s, a.conn_flags, a.trackers,
                     a.ack_pending, a.n_conns, a.build != nullptr, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (!a.build) return hipSuccess;
  if ((e = exclusive_sum(w, w.due, w.base, a.n_conns + 1, s)) != hipSuccess) return e;
  const uint64_t threads =
      (uint64_t)a.n_conns * kAckGroup > a.build->max_acks ? (uint64_t)a.n_conns * kAckGroup : a.build->max_acks;
  hipLaunchKernelGGL(mq_acks_build_kernel, blocks(threads ? threads : 1), block, 0, s, a.trackers, a.ack_pending,
                     a.n_conns, *a.build, w);
  return hipGetLastError();
}
