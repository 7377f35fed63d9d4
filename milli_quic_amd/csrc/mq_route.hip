// mq_route.hip — datagram routing on the device: the connection-ID table (mq_cid_table_*) and
// mq_batch_route, which fills mq_dgram.conn and admits the connections of first Initial packets
// (decode_dcid, reference src/packet/decode_dcid.rs:9-37; first-Initial rule,
// src/connection/recv.rs:275-278; RFC 9000 §5.2, §14.1, §17.2). The per-datagram arithmetic is
// mq_route.h, shared with the host test.
//
// Table: open addressing, linear probing, a power of two >= 2 x capacity slots of 32 bytes:
//   [tag 8 B][CID bytes 0..15][CID bytes 16..19][conn 4 B]
// tag = 59 bits of a SipHash-1-3 of the CID under the table's seed, above the CID's length; the
// all-ones word is an empty slot, all-ones - 1 a tombstone (mq_route.h). A slot is claimed with one
// 64-bit compare-and-swap of its tag and filled afterwards; nothing reads a slot in the kernel that
// fills it. Two counters (live entries, tombstones) sit beside the slots.
//
// No lane ever waits for another: every probe loop is bounded by the slot count and takes "somebody
// else's slot" as "probe on"; phases that need each other's results are separate kernels on the
// caller's stream. Counters are summed per wave before one atomic.
//
// mq_batch_route with admission, one lane per datagram:
//   lookup   classify, extract the CID, look it up (the table is read-only here). An admissible miss
//            stores its key in the workspace and claims its tag in a batch-local set of 64-bit words
//            (>= 2 x n_dgrams slots, cleared per call): compare-and-swap empty -> tag, finding its own
//            tag counts as success; then atomicMin(first[slot], i).
//   groups   a miss whose key equals datagram first[slot]'s belongs to that group, and is the group's
//            representative if it is that datagram; an unequal key is a real collision of the whole
//            slot word: MQ_ROUTE_DEFERRED.
//   rank     exclusive scan of the representative flags in datagram order (hipcub).
//   admit    groups with rank below the limit: every datagram takes conn_base + rank of its
//            representative; the representative writes new_dcids / new_dcid_lens, the connection row
//            and the table entry.
// Determinism: a tag owns exactly one slot of the batch set whatever the claim order (set words are
// written once), so first[slot] is the lowest datagram index of that tag; flags, ranks and with them
// every output follow from the inputs. Only the positions of the new table entries depend on timing,
// and no result depends on those.
#include "mq_launch.h"
#include "mq_replay.h"
#include "mq_route.h"

namespace mq {

struct RouteHead {  // first 256 bytes of the workspace
  uint32_t limit;   // groups this call may admit: min(max_new, capacity - live at the start)
};

struct RouteWs {
  RouteHead* head;
  CidSlot* keys;                  // n: the key of each admissible miss (conn unused)
  uint32_t* sidx;                 // n: its slot of the batch set
  uint32_t* flags;                // n + 1: 1 = group representative; [n] = 0
  uint32_t* rank;                 // n + 1: exclusive scan of flags; [n] = number of groups
  unsigned long long* set;        // set_mask + 1 tags
  uint32_t* first;                // set_mask + 1: lowest datagram index per tag
  uint32_t set_mask;
  void* cub;
  size_t cub_bytes;
};

constexpr uint8_t kRoutePending = 0x80;  // status of an admissible miss between the kernels of one call

// ---- wave helpers ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {  // every lane of the wave must call it
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
// counter += / -= the wave's sum of x: one atomic per wave (every lane of the wave must call it)
__device__ __forceinline__ void wave_counter_add(uint32_t* ctr, uint32_t x) {
  const uint32_t s = wave_sum(x);
  if (s && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(ctr, s);
}
__device__ __forceinline__ void wave_counter_sub(uint32_t* ctr, uint32_t x) {
  const uint32_t s = wave_sum(x);
  if (s && (threadIdx.x & (kWave - 1)) == 0) atomicSub(ctr, s);
}

// ---- slots -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return lo | (uint64_t)hi << 32; }

__device__ __forceinline__ CidSlot slot_of(const CidTableDev& t, const CidKey& k) {
  CidSlot s;
  s.tag = route_tag(t.k0, t.k1, t.hash_mask, k);
  s.w0 = k.w0, s.w1 = k.w1, s.w2 = k.w2, s.conn = 0;
  return s;
}

// The first slot on key's probe chain that holds it: its index, or -1. Two 16-B loads per slot, the
// second only behind a matching first half.
__device__ __forceinline__ int64_t slot_find(const CidTableDev& t, const CidSlot& key, uint32_t start, uint32_t* conn) {
  const uint32_t pos = route_tag_pos(key.tag, t.slot_mask);
  for (uint32_t p = start; p <= t.slot_mask; ++p) {
    const uint32_t s = (pos + p) & t.slot_mask;
    const uint4* q = reinterpret_cast<const uint4*>(t.slots + s);
    const uint4 a = q[0];
    const uint64_t tag = u64_of(a.x, a.y);
    if (tag == kCidEmpty) return -1;
    if (tag == key.tag && u64_of(a.z, a.w) == key.w0) {
      const uint4 b = q[1];
      if (u64_of(b.x, b.y) == key.w1 && b.z == key.w2) {
        *conn = b.w;
        return (int64_t)p;
      }
    }
  }
  return -1;
}

// Claims a free slot on key's chain and fills it. The caller knows that the key is not in the table,
// so any taken slot — one with the same tag included — is another entry: probe on. Returns whether
// the slot was a tombstone. With live entries <= capacity <= slots / 2 a free slot always turns up.
__device__ __forceinline__ bool slot_insert(CidSlot* slots, uint32_t slot_mask, const CidSlot& key, uint32_t conn) {
  const uint32_t pos = route_tag_pos(key.tag, slot_mask);
  for (uint32_t p = 0; p <= slot_mask; ++p) {
    CidSlot* d = slots + ((pos + p) & slot_mask);
    unsigned long long* tw = reinterpret_cast<unsigned long long*>(&d->tag);
    const unsigned long long cur = *reinterpret_cast<volatile unsigned long long*>(tw);
    if (cur != kCidEmpty && cur != kCidTomb) continue;
    if (atomicCAS(tw, cur, (unsigned long long)key.tag) != cur) continue;  // somebody else's now
    d->w0 = key.w0, d->w1 = key.w1, d->w2 = key.w2, d->conn = conn;
    return cur == kCidTomb;
  }
  return false;
}

// ---- header bytes ------------------------------------------------------------------------------------
// Bytes [lo, hi) of the datagram at p (lo = 0 or 16, hi <= lo + 16, hi <= len) as four words: one
// unaligned 16-B load where the datagram has all of [lo, lo + 16), else byte loads.
__device__ __forceinline__ void load_hdr16(const uint8_t* p, uint32_t len, uint32_t lo, uint32_t hi,
                                           uint32_t& h0, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
  if (len >= lo + 16) {
    const uint4 v = ld16(p + lo);
    h0 = v.x, h1 = v.y, h2 = v.z, h3 = v.w;
    return;
  }
  uint64_t a = 0, b = 0;
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t k = j - lo;
    const uint64_t v = p[j];
    if (k < 8) a |= v << (8 * k);
    else b |= v << (8 * (k - 8));
  }
  h0 = (uint32_t)a, h1 = (uint32_t)(a >> 32), h2 = (uint32_t)b, h3 = (uint32_t)(b >> 32);
}

// A table key from a 20-byte-stride array (insert / remove); false for a length over 20.
__device__ __forceinline__ bool key_from_row(const uint8_t* cids, const uint8_t* lens, uint32_t i, CidKey* k) {
  const uint32_t len = lens[i];
  if (len > kRouteMaxCid) return false;
  const u32_u* c = reinterpret_cast<const u32_u*>(cids + (size_t)kRouteMaxCid * i);
  uint32_t o[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) o[q] = c[q];
  *k = route_key_words(o, len);
  return true;
}

}  // namespace mq

using namespace mq;

// ---- route -------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void mq_route_lookup_kernel(
    CidTableDev t, const uint8_t* __restrict__ arena, uint64_t arena_len, mq_dgram* dg, uint32_t n, uint32_t sdl,
    uint32_t admit_on, uint32_t min_initial_len, uint8_t* __restrict__ status, RouteWs ws) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 d = *reinterpret_cast<const uint4*>(dg + i);  // offset, len, conn
  const uint64_t off = u64_of(d.x, d.y);
  const uint32_t len = d.z;
  uint32_t st = MQ_ROUTE_MALFORMED, conn = MQ_CONN_NONE;
  CidSlot key;
  if (off <= arena_len && len <= arena_len - off && len != 0) {
    const uint8_t* p = arena + off;
    uint32_t hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    load_hdr16(p, len, 0, len < 16 ? len : 16, hdr[0], hdr[1], hdr[2], hdr[3]);
    const DgClass c = route_classify(len, hdr[0], hdr[1], sdl);
    if (c.kind != kDgMalformed) {
      const uint32_t need = c.cid_off + c.cid_len;  // <= 26 and <= len
      if (need > 16) load_hdr16(p, len, 16, need, hdr[4], hdr[5], hdr[6], hdr[7]);
      key = slot_of(t, route_key(hdr, c.kind == kDgLong, c.cid_len));
      if (slot_find(t, key, 0, &conn) >= 0) st = MQ_ROUTE_HIT;
      else if (admit_on && route_admissible(c.kind, hdr[0], hdr[1], len, min_initial_len)) st = kRoutePending;
      else st = MQ_ROUTE_UNKNOWN;
    }
  }
  if (st == kRoutePending) {
    uint4* kq = reinterpret_cast<uint4*>(ws.keys + i);
    kq[0] = make_uint4((uint32_t)key.tag, (uint32_t)(key.tag >> 32), (uint32_t)key.w0, (uint32_t)(key.w0 >> 32));
    kq[1] = make_uint4((uint32_t)key.w1, (uint32_t)(key.w1 >> 32), key.w2, 0u);
    const uint32_t pos = route_tag_pos(key.tag, ws.set_mask);
    uint32_t s = pos;
    for (uint32_t q = 0; q <= ws.set_mask; ++q) {  // the set has >= 2n slots: a free one always turns up
      s = (pos + q) & ws.set_mask;
      const unsigned long long old = atomicCAS(ws.set + s, (unsigned long long)kCidEmpty, (unsigned long long)key.tag);
      if (old == kCidEmpty || old == key.tag) break;
    }
    atomicMin(ws.first + s, i);
    ws.sidx[i] = s;
  }
  status[i] = (uint8_t)st;
  dg[i].conn = conn;
}

extern "C" __global__ __launch_bounds__(256) void mq_route_groups_kernel(CidTableDev t, uint32_t n, uint32_t max_new,
                                                                        uint8_t* __restrict__ status, RouteWs ws) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    const uint32_t live = t.ctr[0], room = live < t.capacity ? t.capacity - live : 0u;
    ws.head->limit = max_new < room ? max_new : room;
    ws.flags[n] = 0;
  }
  if (i >= n) return;
  uint32_t flag = 0;
  if (status[i] == kRoutePending) {
    const uint32_t f = ws.first[ws.sidx[i]];  // <= i
    if (f == i) {
      flag = 1;
    } else {  // same tag (length included): the same CID, or a collision of all 64 bits
      const uint4* a = reinterpret_cast<const uint4*>(ws.keys + i);
      const uint4* b = reinterpret_cast<const uint4*>(ws.keys + f);
      const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
      const bool same = a0.z == b0.z && a0.w == b0.w && a1.x == b1.x && a1.y == b1.y && a1.z == b1.z;
      if (!same) status[i] = MQ_ROUTE_DEFERRED;
    }
  }
  ws.flags[i] = flag;
}

// Lanes [0, max(n, max_new)). rank == nullptr: a call without datagrams (n = 0).
extern "C" __global__ __launch_bounds__(256) void mq_route_admit_kernel(
    CidTableDev t, mq_dgram* dg, uint32_t n, uint32_t sdl, mq_conn_recv* conns, uint32_t conn_base, uint32_t max_new,
    uint32_t row_first, uint8_t* __restrict__ new_dcids, uint8_t* __restrict__ new_dcid_lens, uint32_t* n_new,
    uint8_t* __restrict__ status, RouteWs ws) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t groups = n ? ws.rank[n] : 0u, limit = n ? ws.head->limit : 0u;
  const uint32_t admitted = groups < limit ? groups : limit;
  if (i == 0) {
    *n_new = admitted;
    if (admitted) atomicAdd(t.ctr, admitted);  // live entries
  }
  if (i < max_new && i >= admitted) new_dcid_lens[i] = 0xFF;
  uint32_t reused = 0;
  if (i < n && status[i] == kRoutePending) {
    const uint32_t f = ws.first[ws.sidx[i]];
    const uint32_t k = ws.rank[f];
    if (k < limit) {
      const uint32_t conn = conn_base + k;
      status[i] = MQ_ROUTE_NEW;
      dg[i].conn = conn;
      if (f == i) {  // the group's representative
        const CidSlot key = ws.keys[i];
        const uint32_t len = (uint32_t)key.tag & 31u;
        u32_u* c = reinterpret_cast<u32_u*>(new_dcids + (size_t)kRouteMaxCid * k);
        c[0] = (uint32_t)key.w0, c[1] = (uint32_t)(key.w0 >> 32), c[2] = (uint32_t)key.w1;
        c[3] = (uint32_t)(key.w1 >> 32), c[4] = key.w2;
        new_dcid_lens[k] = (uint8_t)len;
        mq_conn_recv row = {};
        row.initial_row = row_first + 2 * k;
        row.flags = MQ_RECV_HAS_INITIAL;
        row.dcid_len = (uint8_t)sdl;
        conns[conn] = row;
        reused = slot_insert(t.slots, t.slot_mask, key, conn) ? 1u : 0u;
      }
    } else {
      status[i] = MQ_ROUTE_FULL;
    }
  }
  wave_counter_sub(t.ctr + 1, reused);  // tombstones taken over
}

// ---- table operations --------------------------------------------------------------------------------
// insert, first kernel: MALFORMED / HIT / pending against the table as it is (read-only here)
extern "C" __global__ __launch_bounds__(256) void mq_cid_present_kernel(CidTableDev t, const uint8_t* __restrict__ cids,
                                                                       const uint8_t* __restrict__ lens, uint32_t n,
                                                                       uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  CidKey k;
  if (!key_from_row(cids, lens, i, &k)) {
    status[i] = MQ_ROUTE_MALFORMED;
    return;
  }
  uint32_t conn;
  status[i] = slot_find(t, slot_of(t, k), 0, &conn) >= 0 ? (uint8_t)MQ_ROUTE_HIT : kRoutePending;
}

// insert, second kernel: the pending entries take a place below the capacity, then a slot
extern "C" __global__ __launch_bounds__(256) void mq_cid_insert_kernel(CidTableDev t, const uint8_t* __restrict__ cids,
                                                                      const uint8_t* __restrict__ lens,
                                                                      const uint32_t* __restrict__ conn, uint32_t n,
                                                                      uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool want = i < n && status[i] == kRoutePending;
  // places: one atomicAdd per wave on the live counter; what overshoots the capacity is given back
  const uint64_t m = __builtin_amdgcn_ballot_w64(want);
  uint32_t reused = 0;
  if (m) {
    const uint32_t cnt = (uint32_t)__builtin_popcountll(m), r = lanes_below(m);
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0;
    if (want && r == 0) {
      base = atomicAdd(t.ctr, cnt);
      const uint32_t fit = base >= t.capacity ? 0u : (cnt < t.capacity - base ? cnt : t.capacity - base);
      if (fit < cnt) atomicSub(t.ctr, cnt - fit);
    }
    base = __shfl(base, leader);
    if (want) {
      if (base + r >= t.capacity) {
        status[i] = MQ_ROUTE_FULL;
      } else {
        CidKey k;
        (void)key_from_row(cids, lens, i, &k);
        reused = slot_insert(t.slots, t.slot_mask, slot_of(t, k), conn[i]) ? 1u : 0u;
        status[i] = MQ_OK;
      }
    }
  }
  wave_counter_sub(t.ctr + 1, reused);
}

// remove: every entry of the CID on its chain (two of them after an insert call that named it twice)
extern "C" __global__ __launch_bounds__(256) void mq_cid_remove_kernel(CidTableDev t, const uint8_t* __restrict__ cids,
                                                                      const uint8_t* __restrict__ lens, uint32_t n,
                                                                      uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t freed = 0;
  if (i < n) {
    CidKey k;
    uint32_t st = MQ_ROUTE_UNKNOWN;
    if (key_from_row(cids, lens, i, &k)) {
      const CidSlot key = slot_of(t, k);
      const uint32_t pos = route_tag_pos(key.tag, t.slot_mask);
      uint32_t conn;
      int64_t p = -1;
      while ((p = slot_find(t, key, (uint32_t)(p + 1), &conn)) >= 0) {  // p grows: at most slot-count steps
        st = MQ_OK;
        unsigned long long* tw = reinterpret_cast<unsigned long long*>(&t.slots[(pos + (uint32_t)p) & t.slot_mask].tag);
        if (atomicCAS(tw, (unsigned long long)key.tag, (unsigned long long)kCidTomb) == key.tag) ++freed;
      }
    }
    status[i] = (uint8_t)st;
  }
  wave_counter_sub(t.ctr, freed);
  wave_counter_add(t.ctr + 1, freed);
}

// compact: every live slot of the old buffer into the cleared new one (same slot count: the tag
// gives the position; the keys are unique there)
extern "C" __global__ __launch_bounds__(256) void mq_cid_rehash_kernel(const CidSlot* __restrict__ from, CidSlot* to,
                                                                      uint32_t slot_mask) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > slot_mask) return;
  const uint4* q = reinterpret_cast<const uint4*>(from + i);
  const uint4 a = q[0];
  const uint64_t tag = u64_of(a.x, a.y);
  if (tag == kCidEmpty || tag == kCidTomb) return;
  const uint4 b = q[1];
  CidSlot key;
  key.tag = tag, key.w0 = u64_of(a.z, a.w), key.w1 = u64_of(b.x, b.y), key.w2 = b.z;
  (void)slot_insert(to, slot_mask, key, b.w);
}

// ---- host side -----------------------------------------------------------------------------------------
namespace {
uint32_t route_set_slots(uint32_t n) {  // a power of two >= 2n (n <= 2^31 - 1 gives at most 2^32: see below)
  uint64_t s = 16;
  while (s < 2ull * n) s <<= 1;
  return (uint32_t)(s - 1);  // as a mask
}
size_t route_layout(uint32_t n, void* base, RouteWs& w) {
  Carve c(base);
  w.set_mask = route_set_slots(n);
  w.head = c.take<RouteHead>(1);
  w.keys = c.take<CidSlot>(n);
  w.sidx = c.take<uint32_t>(n);
  w.flags = c.take<uint32_t>((size_t)n + 1);
  w.rank = c.take<uint32_t>((size_t)n + 1);
  w.set = c.take<unsigned long long>((size_t)w.set_mask + 1);
  w.first = c.take<uint32_t>((size_t)w.set_mask + 1);
  w.cub_bytes = cub_temp_bytes<false>(0, 0, {n + 1});
  w.cub = c.take<uint8_t>(w.cub_bytes);
  return c.bytes();
}
dim3 grid_for(uint64_t lanes) { return dim3((uint32_t)((lanes + 255) / 256)); }
}  // namespace

size_t mq_route_workspace(uint32_t n) {
  RouteWs w = {};
  return route_layout(n, nullptr, w);
}

hipError_t mq_launch_route(const CidTableDev& t, const uint8_t* arena, uint64_t arena_len, mq_dgram* dg, uint32_t n,
                           uint32_t sdl, const mq_route_admit* admit, uint8_t* status, void* workspace,
                           hipStream_t s) {
  RouteWs w = {};
  hipError_t e;
  if (!admit) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mq_route_lookup_kernel, grid_for(n), dim3(256), 0, s, t, arena, arena_len, dg, n, sdl, 0u, 0u,
                       status, w);
    return hipGetLastError();
  }
  if (n) {
    route_layout(n, workspace, w);
    // the batch set: all-ones = empty; first[]: all-ones = no datagram yet
    if ((e = hipMemsetAsync(w.set, 0xFF, 8 * ((size_t)w.set_mask + 1), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.first, 0xFF, 4 * ((size_t)w.set_mask + 1), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(mq_route_lookup_kernel, grid_for(n), dim3(256), 0, s, t, arena, arena_len, dg, n, sdl, 1u,
                       admit->min_initial_len, status, w);
    hipLaunchKernelGGL(mq_route_groups_kernel, grid_for(n), dim3(256), 0, s, t, n, admit->max_new, status, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = exclusive_sum(w, w.flags, w.rank, n + 1, s)) != hipSuccess) return e;
  }
  const uint64_t lanes = n > admit->max_new ? n : admit->max_new;
  hipLaunchKernelGGL(mq_route_admit_kernel, grid_for(lanes ? lanes : 1), dim3(256), 0, s, t, dg, n, sdl, admit->conns,
                     admit->conn_base, admit->max_new, admit->row_first, admit->new_dcids, admit->new_dcid_lens,
                     admit->n_new, status, w);
  return hipGetLastError();
}

hipError_t mq_launch_cid_insert(const CidTableDev& t, const uint8_t* cids, const uint8_t* lens, const uint32_t* conn,
                                uint32_t n, uint8_t* status, hipStream_t s) {
  hipLaunchKernelGGL(mq_cid_present_kernel, grid_for(n), dim3(256), 0, s, t, cids, lens, n, status);
  hipLaunchKernelGGL(mq_cid_insert_kernel, grid_for(n), dim3(256), 0, s, t, cids, lens, conn, n, status);
  return hipGetLastError();
}

hipError_t mq_launch_cid_remove(const CidTableDev& t, const uint8_t* cids, const uint8_t* lens, uint32_t n,
                                uint8_t* status, hipStream_t s) {
  hipLaunchKernelGGL(mq_cid_remove_kernel, grid_for(n), dim3(256), 0, s, t, cids, lens, n, status);
  return hipGetLastError();
}

// `to` (as large as t.slots) is cleared to all-ones — every slot empty — and receives the live entries
// of t.slots; the tombstone counter goes to zero
hipError_t mq_launch_cid_compact(const CidTableDev& t, void* to, hipStream_t s) {
  const size_t bytes = sizeof(CidSlot) * ((size_t)t.slot_mask + 1);
  hipError_t e;
  if ((e = hipMemsetAsync(to, 0xFF, bytes, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mq_cid_rehash_kernel, grid_for((uint64_t)t.slot_mask + 1), dim3(256), 0, s, t.slots,
                     (CidSlot*)to, t.slot_mask);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipMemsetAsync(t.ctr + 1, 0, 4, s);
}
