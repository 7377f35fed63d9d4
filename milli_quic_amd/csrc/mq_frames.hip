// mq_frames.hip — mq_batch_frames: the frames of every opened packet as fixed-size records, on the
// device (dispatch_frames, reference src/connection/recv.rs:518-545, over frame::decode,
// src/frame/mod.rs:228-461). The per-frame arithmetic is mq_frames.h, shared with the host test.
//
// A group of kFrameLanes lanes takes one packet. The group looks at the payload through a window of
// 16 bytes per lane: lane j loads payload bytes [base + 16 j, base + 16 j + 16) with one unaligned
// 16-B load where all of them lie inside the payload, else byte by byte up to the payload's end, and
// puts them into the group's slice of LDS. Every lane of the group then runs the same decode over the
// window (a byte is one LDS read); the window moves when a position outside it is asked for. So the
// control flow is uniform inside a group, and the group's lanes are always active together.
//   padding  a zero type byte starts a run: every lane has the mask of its non-zero bytes, a ballot
//            finds the first lane with one at or behind the position, and the run ends there or at
//            the window's end. A 900-byte run of an Initial costs 900 / (16 x lanes) windows.
//   data     CRYPTO / STREAM / NEW_TOKEN / reason bytes are skipped by their length and never loaded.
// Nothing outside [payload start, payload end) is loaded, and nothing but the outputs is written.
//
// Arrival order with a count the host never sees:
//   count    walks every packet, writes its summary (all but `first`) and its record count, ORs the
//            connection flags.
//   scan     exclusive sum of the counts over max_pkts + 1 entries (hipcub); the last one is the total.
//   emit     writes summary.first; a packet with records is walked again up to its last record, and the
//            records whose index is below max_frames are stored, three 16-B stores spread over the lanes.
// Every output is a function of the inputs: no atomics but the OR into conn_flags.
#include "mq_replay.h"  // first: mq_frames.h needs the HIP runtime's qualifiers

#include "mq_frames.h"
#include "mq_launch.h"

#ifndef MQ_FRAMES_LANES
#define MQ_FRAMES_LANES 4  // 1, 2, 4, 8, 16 and 32 were measured
#endif

namespace mq {

constexpr uint32_t kFrameLanes = MQ_FRAMES_LANES;
constexpr uint32_t kFrameWin = 16 * kFrameLanes;  // window bytes
constexpr uint32_t kFrameBlock = 256;
constexpr uint32_t kFramePktsPerBlock = kFrameBlock / kFrameLanes;
static_assert(kFrameLanes >= 1 && kFrameLanes <= 32 && (kFrameLanes & (kFrameLanes - 1)) == 0, "group width");

struct FramesWs {
  uint32_t* counts;  // max_pkts + 1: records per packet; [max_pkts] = 0
  uint32_t* first;   // max_pkts + 1: exclusive scan; [max_pkts] = the total
  void* cub;
  size_t cub_bytes;
};

// orders the wave's own LDS accesses for the compiler; the hardware runs one wave's LDS
// instructions in order
__device__ __forceinline__ void frames_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bit k set: byte k of the 16 is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(const uint4& w) {
  const uint32_t x[4] = {w.x, w.y, w.z, w.w};
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= ((x[q] >> (8 * k)) & 0xFFu) ? 1u << (4 * q + k) : 0u;
  }
  return m;
}

// The group's view of one payload. Every member but `lane` and `nz` is the same in all its lanes.
struct FrameWindow {
  const uint8_t* p;  // payload start
  uint32_t len;      // payload length
  uint32_t base, n;  // the window holds payload bytes [base, base + n), n <= kFrameWin
  uint8_t* lds;      // the group's kFrameWin bytes
  uint32_t lane;     // lane in the group
  uint32_t nz;       // non-zero mask of this lane's 16 window bytes (bytes past n are zero)

  __device__ __forceinline__ void fill(uint32_t at) {  // at < len
    base = at;
    n = len - at < kFrameWin ? len - at : kFrameWin;
    const uint32_t lo = 16 * lane;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (lo + 16 <= n) {
      w = ld16(p + at + lo);
    } else if (lo < n) {  // the payload's last, partial 16 bytes
      uint64_t a = 0, b = 0;
      for (uint32_t k = 0; lo + k < n; ++k) {
        const uint64_t v = p[at + lo + k];
        if (k < 8) a |= v << (8 * k);
        else b |= v << (8 * (k - 8));
      }
      w = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
    nz = nonzero_bytes(w);
    frames_sync();  // the reads of the old window are done
    *reinterpret_cast<uint4*>(lds + lo) = w;
    frames_sync();
  }
  __device__ __forceinline__ uint32_t operator()(uint32_t pos) {  // pos < len
    if (pos - base >= n) fill(pos);
    return lds[pos - base];
  }
  // pos is inside the window and holds a zero byte: the length of the zero run from pos, cut at the
  // window's end
  __device__ __forceinline__ uint32_t zero_run(uint32_t pos, uint32_t group_first) const {
    const uint32_t rel = pos - base, lo = 16 * lane;
    uint32_t m = nz;
    if (rel > lo) m = rel - lo >= 16 ? 0u : m & ~((1u << (rel - lo)) - 1u);
    const uint64_t ball = __builtin_amdgcn_ballot_w64(m != 0);
    const uint32_t gb = (uint32_t)(ball >> group_first) & (uint32_t)((1ull << kFrameLanes) - 1);
    if (gb == 0) return n - rel;
    const uint32_t j = (uint32_t)__builtin_ctz(gb);
    const uint32_t mj = (uint32_t)__shfl((int)m, (int)(group_first + j), kWave);
    return 16 * j + (uint32_t)__builtin_ctz(mj) - rel;
  }
};

struct PktRange {
  const uint8_t* p;
  uint32_t len;
  uint32_t status;  // MQ_OK, MQ_FRAMES_SKIPPED or MQ_ERR_INVALID_ARG
  uint32_t level, dgram;
};

// The packet's payload: arena[offset + payload_offset, offset + len - 16), when the packet opened and
// all of it lies inside the arena and the records can describe it.
__device__ __forceinline__ PktRange pkt_range(const uint8_t* arena, uint64_t arena_len, const mq_recv_pkt* pk) {
  const uint4* q = reinterpret_cast<const uint4*>(pk);
  const uint4 a = q[0], b = q[1];  // offset, pn | len, dgram, payload_offset + level + status, key_gen
  const uint64_t off = a.x | (uint64_t)a.y << 32;
  const uint32_t len = b.x, po = b.z & 0xFFFFu;
  PktRange r;
  r.p = nullptr, r.len = 0;
  r.dgram = b.y;
  r.level = (b.z >> 16) & 0xFFu;
  r.status = MQ_FRAMES_SKIPPED;
  if ((b.z >> 24) != MQ_OK) return r;
  r.status = MQ_ERR_INVALID_ARG;
  if (off > arena_len || len > arena_len - off || po + 16u > len || len - po - 16u > kFrameMaxPayload) return r;
  r.status = MQ_OK;
  r.p = arena + off + po;
  r.len = len - po - 16u;
  return r;
}

}  // namespace mq

using namespace mq;

// Emit = false: the count pass. Emit = true: the emit pass (walks up to the packet's last record).
template <bool Emit>
__global__ __launch_bounds__(kFrameBlock) void mq_frames_kernel(FramesArgs a, FramesWs ws) {
  __shared__ uint4 win[kFrameBlock];
  const uint32_t lane = threadIdx.x & (kFrameLanes - 1);
  const uint32_t group_first = threadIdx.x & (kWave - 1) & ~(kFrameLanes - 1);
  const uint32_t i = blockIdx.x * kFramePktsPerBlock + threadIdx.x / kFrameLanes;
  if (i >= a.max_pkts) return;
  const uint32_t n_dev = *a.n_pkts_dev;
  const uint32_t n_pkts = n_dev < a.max_pkts ? n_dev : a.max_pkts;
  uint32_t want = 0, first = 0;
  if (Emit) {
    if (i == 0 && lane == 0) *a.n_frames = ws.first[a.max_pkts];
    if (i >= n_pkts) return;
    first = ws.first[i];
    want = ws.counts[i];
    if (lane == 0) a.summary[i].first = first;
    if (want == 0) return;
  } else if (i >= n_pkts) {
    if (lane == 0) {
      ws.counts[i] = 0;
      if (i + 1 == a.max_pkts) ws.counts[a.max_pkts] = 0;
    }
    return;
  }
  const PktRange r = pkt_range(a.arena, a.arena_len, a.pkts + i);
  uint32_t status = r.status, recs = 0, pads = 0, err_pos = 0, flags = 0, close = 0;
  if (status == MQ_OK && r.len) {
    FrameWindow w;
    w.p = r.p, w.len = r.len, w.lane = lane;
    w.lds = reinterpret_cast<uint8_t*>(win + (threadIdx.x - lane));
    w.fill(0);
    uint32_t pos = 0;
    while (pos < r.len) {
      if (w(pos) == 0) {  // PADDING: a one-byte type 0, and so is every zero byte behind it
        const uint32_t run = w.zero_run(pos, group_first);
        pads += run;
        pos += run;
        continue;
      }
      FrameFields f;
      uint32_t next;
      if (!frame_decode(w, pos, r.len, f, next)) {
        status = MQ_ERR_FRAME;
        err_pos = pos;
        break;
      }
      if (f.type == 0) {  // PADDING in a longer encoding of its type
        ++pads;
        pos = next;
        continue;
      }
      if (frame_ack_eliciting(f.type)) flags |= 1u;
      if (frame_is_close(f.type)) close = 1;
      if (Emit) {
        const uint64_t at = (uint64_t)first + recs;
        if (at < a.max_frames) {
          uint4* dst = reinterpret_cast<uint4*>(a.frames + at);
#pragma unroll
          for (uint32_t q = 0; q < 3; ++q) {  // the record's three 16-B parts, spread over the group's lanes
            if (lane != q % kFrameLanes) continue;
            uint4 v;
            if (q == 0)
              v = make_uint4(i, pos | (next - pos) << 16, f.type | r.level << 8 | f.data_pos << 16,
                             f.data_len | f.aux << 16);
            else if (q == 1)
              v = make_uint4((uint32_t)f.v0, (uint32_t)(f.v0 >> 32), (uint32_t)f.v1, (uint32_t)(f.v1 >> 32));
            else
              v = make_uint4((uint32_t)f.v2, (uint32_t)(f.v2 >> 32), (uint32_t)f.v3, (uint32_t)(f.v3 >> 32));
            dst[q] = v;
          }
        }
      }
      ++recs;
      pos = next;
      if (Emit && recs == want) break;
    }
  }
  if (Emit || lane != 0) return;
  ws.counts[i] = recs;
  if (i + 1 == a.max_pkts) ws.counts[a.max_pkts] = 0;
  // first is written by the emit pass
  const uint4 s = make_uint4(0u, recs | err_pos << 16, pads | status << 16 | flags << 24, 0u);
  *reinterpret_cast<uint4*>(a.summary + i) = s;
  if (a.conn_flags && status != MQ_FRAMES_SKIPPED && status != MQ_ERR_INVALID_ARG && r.dgram < a.n_dgrams) {
    const uint32_t c = a.dgrams[r.dgram].conn;
    uint32_t bits = 0;
    if (status == MQ_OK && flags && r.level < 3) bits |= 1u << r.level;
    if (close) bits |= 1u << 3;
    if (status == MQ_ERR_FRAME) bits |= 1u << 4;
    if (bits && c < a.n_conns) atomicOr(a.conn_flags + c, bits);
  }
}

// ---- host side -----------------------------------------------------------------------------------------
namespace {
size_t frames_layout(uint32_t n, void* base, FramesWs& w) {
  Carve c(base);
  w.counts = c.take<uint32_t>((size_t)n + 1);
  w.first = c.take<uint32_t>((size_t)n + 1);
  w.cub_bytes = cub_temp_bytes<false>(0, 0, {n + 1});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes();
}
}  // namespace

size_t mq_frames_workspace(uint32_t max_pkts) {
  FramesWs w = {};
  return frames_layout(max_pkts, nullptr, w);
}

// max_pkts > 0
hipError_t mq_launch_frames(const FramesArgs& a, void* workspace, hipStream_t s) {
  FramesWs w = {};
  frames_layout(a.max_pkts, workspace, w);
  hipError_t e;
  if (a.conn_flags && a.n_conns && (e = hipMemsetAsync(a.conn_flags, 0, 4 * (size_t)a.n_conns, s)) != hipSuccess) return e;
  const dim3 grid((a.max_pkts + kFramePktsPerBlock - 1) / kFramePktsPerBlock), block(kFrameBlock);
  hipLaunchKernelGGL(mq_frames_kernel<false>, grid, block, 0, s, a, w);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(w, w.counts, w.first, a.max_pkts + 1, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_frames_kernel<true>, grid, block, 0, s, a, w);
  return hipGetLastError();
}
