// mq_chacha.hip — AEAD_CHACHA20_POLY1305 packet protection (RFC 8439 / RFC 9001 §5) on gfx950.
//
// Replaces, per packet of a batch, the reference's ChaCha20Poly1305Aead::seal_in_place /
// open_in_place (src/crypto/rustcrypto.rs:111-165) plus ChaChaHeaderProtection::mask
// (:197-220), composed the way src/connection/transmit.rs:625-755 (send) and
// src/connection/recv.rs:340-421,953-1025 (receive) compose them.
//
// Per tile (8 packets, one octet of lanes per packet; see mq_tile.h):
//   seal: keystream block ctr on lane ctr % 8 (ctr 0 = Poly1305 one-time key) XORed into LDS
//         (blocks >= 16 and the header-protection block through the workgroup's keystream pool)
//         -> interleaved Poly1305 over AAD||pad||CT||pad||lens (per wave, 8 lanes per packet; in
//         the flat 10-KiB kernels as a workgroup phase, 4 lanes per packet) -> tag -> header mask applied
//   open: HP mask -> unmask byte 0 / PN -> decode_pn -> nonce -> first keystream block (lane 0:
//         one-time key) -> Poly1305 over the untouched ciphertext -> tag check -> only then the
//         keystream XOR (held first block + the rest); failed packets are never stored.
#include "mq_tile.h"
#include "mq_build.h"
#include "mq_launch.h"

#include <cstdlib>
#include <type_traits>

namespace mq {

// Byte stride between the LDS images of a packet's consecutive keystream blocks: 64. The
// MQ_PROF_SKIP & 128 diagnostic build (never the product) uses 68 — a 17-dword stride, so the
// eight lanes of a packet hit eight distinct LDS banks — computing garbage with the same
// instructions: its time minus the product's is what the keystream XOR's bank conflicts cost.
#if MQ_PROF_SKIP & 128
constexpr uint32_t kKsStride = 68;
#else
constexpr uint32_t kKsStride = 64;
#endif

// The Poly1305 one-time key r || s (words 0..7 of keystream block 0) as poly_tag takes it. Octet
// tiles: in the packet's 32-B LDS scratch, written by octet lane 0; s is read only once the Horner
// loop is done. Narrow tiles: in registers, already broadcast over the lane group.
struct OtkLds {
  const uint32_t* p;
  __device__ __forceinline__ void r(uint32_t (&w)[4]) const { u4w(*(const uint4*)p, w); }
  __device__ __forceinline__ void s(uint32_t (&w)[4]) const { u4w(*(const uint4*)(p + 4), w); }
};
struct OtkRegs {
  uint32_t rk[4], sk[4];
  __device__ __forceinline__ void r(uint32_t (&w)[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = rk[k];
  }
  __device__ __forceinline__ void s(uint32_t (&w)[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = sk[k];
  }
};

// Interleaved Poly1305 of the AEAD MAC input for the lane group's packet (RFC 8439 §2.8: AAD||pad16||
// CT||pad16||LE64(len AAD)||LE64(len CT)), G lanes per packet (8: an octet tile, 1 / 2 / 4: narrow
// tiles): group lane j takes MAC blocks G k + j - z, Horner with r^G, one final multiply by
// r^(G-j), then the group sum. Every lane of the group returns the same tag.
// The edge steps of the octet form (kEdge below: the lean stretch up to the last whole block, the
// general absorb's single byte count) are not taken by the narrow lane groups G < 8: their batches
// (64- and 256-B packets) measured 0.6 % slower with them (profiles/r09_ab_len_sweep_all_groups.txt),
// and at G = 4 in the workgroup MAC phase they gained nothing beyond the spread (profiles/r12_ab_b_variants.txt).
// PAIR: the lean stretch takes its steps two at a time, ((acc + m_k) R + m_k+1) R as
// (acc + m_k) R^2 + m_k+1 R with one reduction (p26_mul2), then at most one single step. On for
// cc_wg_mac only: the other instantiations have no registers to spare for R^2.
template <int G, bool PAIR = false, class S, class K>
__device__ __forceinline__ void poly_tag(const S& sp, typename S::off_t pkt, typename S::off_t pay, uint32_t aad_len,
                                         uint32_t ct_len, const K& otk, int j, bool act, uint32_t (&tag)[4]) {
  typedef Grp<G> Gp;
  constexpr bool kEdge = G == 8;
  uint32_t rk[4], s[4];
#if MQ_PROF_SKIP & 2
  otk.s(s);
  for (int w = 0; w < 4; ++w) tag[w] = s[w] ^ aad_len ^ ct_len;
  return;
#endif
  otk.r(rk);
  const P26 r = p26_from_words(rk[0] & 0x0fffffffu, rk[1] & 0x0ffffffcu, rk[2] & 0x0ffffffcu, rk[3] & 0x0ffffffcu, 0);
  // powers by a group prefix: v = r^(j+1) after up to three multiplies (r^2, then x r^2 on lanes
  // with bit 1 of j, then x r^4 — taken from octet lane 3 — on lanes with bit 2); r^G is the last
  // group lane's v, and the final multiplier r^(G-j) is lane G-1-j's v (the group mirror)
  P26 v = r, rG = r, rj = r;
  if (G >= 2) {
    P26 t = r;
    p26_mul(t, p26_mult(r));  // r^2
#pragma unroll
    for (int l = 0; l < 5; ++l) v.l[l] = (j & 1) ? t.l[l] : v.l[l];
    if (G >= 4) {
      P26 u = v;
      p26_mul(u, p26_mult(t));
#pragma unroll
      for (int l = 0; l < 5; ++l) v.l[l] = (j & 2) ? u.l[l] : v.l[l];
    }
    if (G == 8) {
      P26 r4, u = v;
#pragma unroll
      for (int l = 0; l < 5; ++l) r4.l[l] = oct_lane3(v.l[l]);
      p26_mul(u, p26_mult(r4));
#pragma unroll
      for (int l = 0; l < 5; ++l) v.l[l] = (j & 4) ? u.l[l] : v.l[l];
    }
#pragma unroll
    for (int l = 0; l < 5; ++l) {
      rG.l[l] = Gp::last(v.l[l]);
      rj.l[l] = Gp::mirror(v.l[l]);
    }
  }
  const P26m mG = p26_mult(rG), mlast = p26_mult(rj);

  const PolyGeom geo = poly_geom<G>(aad_len, ct_len);  // the schedule: mq_poly_sched.h
  const uint32_t A = geo.A, T = geo.T;
  // per-packet values are group-uniform: the group reductions
  const uint32_t Kmax = Gp::wave_max(act ? geo.K : 0u);
  // prepend zero blocks (no 2^128 bit) so every packet of the wave runs exactly Kmax steps
  const PolyLean ln = poly_lean<G, kEdge>(A, geo.nb, ct_len, Kmax, act);
  const int z = ln.z;
  P26 acc;
#pragma unroll
  for (int l = 0; l < 5; ++l) acc.l[l] = 0;

  // MAC block i = G k + j - z of this lane: where it lives, how many of its bytes are real
  struct Blk { typename S::off_t src; int rem; bool pre, lens; };
  auto where = [&](int i) {
    const PolyBlk pb = poly_blk(A, T, aad_len, ct_len, i);
    Blk b;
    b.pre = pb.pre;
    b.lens = pb.lens;
    b.src = pb.aad ? pkt + pb.off : pay + pb.off;
    b.rem = pb.rem;
    if (b.pre || b.lens) b.src = pkt;
    return b;
  };
  auto absorb = [&](const Blk& b, uint32_t (&m)[4]) {
    // wave-uniform fast path: every active lane holds a whole AAD / ciphertext block
    if (!kEdge) {
      if (wave_any(act && (b.pre || b.lens || b.rem < 16))) {
#pragma unroll
        for (int w = 0; w < 4; ++w) m[w] &= byte_mask(b.pre ? 0 : b.rem, w);
        if (b.lens) { m[0] = aad_len; m[1] = 0; m[2] = ct_len; m[3] = 0; }
      }
    } else if (wave_any(act && (b.pre || b.lens || b.rem < 16))) {
      // one byte count per lane: nothing of a prepended block or of the lengths block's slot, whose
      // two non-zero words then go in
      keep_bytes<4>(m, b.pre || b.lens ? 0 : min(max(b.rem, 0), 16));
      m[0] = b.lens ? aad_len : m[0];
      m[2] = b.lens ? ct_len : m[2];
    }
    const P26 x = p26_from_words(m[0], m[1], m[2], m[3], b.pre ? 0u : 1u);
#pragma unroll
    for (int l = 0; l < 5; ++l) acc.l[l] += x.l[l];
  };
  if (Kmax > 0) {
    int i = j - z;
    Blk b = where(i);
    uint32_t m[4];
    load_words<4>(sp, b.src, m);
    // steady state: every active lane moves from one whole ciphertext block to the next one G
    // blocks on (src + 16 G, payload alignment fixed), so the address and realignment selector
    // need no per-step recomputation
    const uint32_t sel_pay = sel_load((uint32_t)(pay & 3));
    const int ct_full_end = ln.ct_full_end;  // first index past the whole CT blocks
    // lean steps k in [klo, khi): every active lane absorbs a whole ciphertext block (G k + j - z in
    // [A, ct_full_end)), so no masks, 2^128 bit selects or address recomputation. The block such a
    // step loads for the next one may be a partial ciphertext block or lie behind the ciphertext
    // (the lengths block's slot): the same address arithmetic fetches a partial block's bytes, and
    // the general absorb that follows masks by rem or replaces the words. The stretch may so end at
    // Kmax - 2, with the final absorb next (kEdge). The look-ahead reads below pay + 16 T + 20: the tag and
    // up to 19 B behind it (a staged image: the next packet or the wave's scratch; the arena:
    // bounds-checked loads).
    const uint32_t klo = Gp::wave_max(ln.k_lo), khi = min(Gp::wave_min(ln.k_hi), Kmax - 1);
    for (uint32_t k = 0; k + 1 < Kmax; ++k) {
      if (k == klo && k < khi) {  // wave-uniform: the lean stretch, steps klo .. khi - 1
        // only the block address advances; i, src and rem catch up once at the end
        typename S::off_t a = b.src & ~(typename S::off_t)3;
        uint32_t sel = sel_pay;
        pin(sel);  // keep the selector in a register (hipcc rematerialised it every step)
        if (PAIR && khi - k >= 2) {  // wave-uniform, so r^(2G) is paid only where a pair runs
          // two steps per reduction. The loads are the single steps' very sequence (each step fetches
          // the next one's block at a += 16 G), so the look-ahead bound does not move: below
          // pay + 16 T + 20, inside the workgroup's allocation (cc_wg_mac). klo and khi are
          // wave-uniform, so this loop is too.
          P26 r2G = rG;
          p26_mul(r2G, mG);
          const P26m mG2 = p26_mult(r2G);
          for (; k + 1 < khi; k += 2) {
            const P26 x = p26_from_words(m[0], m[1], m[2], m[3], 1u);
#pragma unroll
            for (int l = 0; l < 5; ++l) acc.l[l] += x.l[l];
            a += 16 * G;
            load_words_sel<4>(sp, a, sel, m);
            const P26 y = p26_from_words(m[0], m[1], m[2], m[3], 1u);
            a += 16 * G;
            load_words_sel<4>(sp, a, sel, m);
            p26_mul2(acc, mG2, y, mG);
          }
        }
        for (; k < khi; ++k) {
          const P26 x = p26_from_words(m[0], m[1], m[2], m[3], 1u);
#pragma unroll
          for (int l = 0; l < 5; ++l) acc.l[l] += x.l[l];
          a += 16 * G;
          load_words_sel<4>(sp, a, sel, m);
          p26_mul(acc, mG);
        }
        const uint32_t nl = khi - klo;
        i += (int)(G * nl);
        b.src += 16 * G * nl;
        b.rem -= (int)(16 * G * nl);
        // the block in flight lies in or just behind the ciphertext (i <= A + T): nothing of it is
        // real exactly when it is the lengths block. b.pre stays false.
        if (kEdge) b.lens = b.rem <= 0;
        if (k + 1 >= Kmax) break;
      }
      absorb(b, m);
      const bool steady = !act || (i >= (int)A && i + G < ct_full_end);
      i += G;
      if (!wave_any(!steady)) {
        b.src += 16 * G;
        b.rem -= 16 * G;
        load_words_sel<4>(sp, b.src & ~(typename S::off_t)3, sel_pay, m);
      } else {
        b = where(i);
        load_words<4>(sp, b.src, m);  // next block's LDS reads overlap this multiply
      }
      p26_mul(acc, mG);
    }
    absorb(b, m);
    p26_mul(acc, mlast);
  }
#pragma unroll
  for (int l = 0; l < 5; ++l) acc.l[l] = Gp::sum(acc.l[l]);
  otk.s(s);
  p26_finish(acc, s, tag);
}

__device__ __forceinline__ void load_key8(const uint32_t* src, uint32_t (&k)[8]) {
  const uint4 a = *(const uint4*)src, b = *(const uint4*)(src + 4);
  k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
}

// ---- keystream pool of a workgroup (kCcWaves waves, one staged tile each) ---------------------
// A 1200-B packet takes 20 ChaCha20 blocks (one-time key and 19 keystream; open's header-protection
// block runs in the one-packet-per-lane pre-pass, seal's in this pool, below), but an octet runs 24
// slots in three iterations, so 1/6 of the rounds went idle. Each wave runs
// iterations 0 and 1 of its own packets; every later keystream block (slot >= 16) goes to the
// workgroup's pool, which all its lanes work off together between two barriers (open: once the
// MACs have read the ciphertext; seal: before the MACs): 4 waves x 8 packets x 4 blocks = 128
// blocks, two wave-iterations for the four instead of a 4/8-full third one each. (Measured at 2,
// 4 and 8 waves: 8 in lockstep lose most of the gain to staging waits that no longer overlap.
// Seal with the HP block kept in the tile measured no gain: 21 blocks = 2.625 iterations per
// tile leave a 3-iteration wave in every workgroup, profiles/r02_ab_chacha_seal_pool_b_rejected.txt.)
#ifndef MQ_CC_WAVES
#define MQ_CC_WAVES 4
#endif
constexpr int kCcWaves = MQ_CC_WAVES;
#ifndef MQ_CC_POOL_ITERS
#define MQ_CC_POOL_ITERS 2
#endif
constexpr uint32_t kCcOwnIters = MQ_CC_POOL_ITERS;  // a wave's own iterations before the pool
constexpr uint32_t kCcPoolSlot = kCcOwnIters * kLanesPerPkt;  // first pooled slot

// Seal also pools every packet's header-protection block (RFC 9001 §5.4.4: ChaCha20 under the HP
// key, counter and nonce from the 16-B ciphertext sample at pn_offset + 4): the sample is
// ciphertext of keystream block 1, in place after iteration 0, and roles 2-3 of a 1200-B workgroup
// have no keystream iteration of the pool to run, so the mask costs no pass over the batch (r02 ran
// it as a post-pass kernel: 63 us and 0.23 GB per 2^20 packets). The mask waits in the record until
// the MAC has read the unprotected header; octet lane 0 then applies it.
// The pool's entries (cc_pool_seal): every packet's pooled keystream blocks first, in packet order,
// padded to whole wave-iterations, then the HP blocks, two lanes each (chacha20_block_pair: lane l
// takes HP entry l >> 1, half l & 1), 32 to a wave-iteration. A 1200-B workgroup: 128 keystream
// blocks on roles 0 and 1, 32 HP blocks on role 2. No iteration holds both kinds, so the keystream
// iterations run open's form of the block (the content key alone, round one hoisted where the key
// is wave-uniform, no sample load) and the HP iteration half a block function per lane.
// -DMQ_CC_HP_INTERLEAVED builds the former pool (cc_pool_run for seal too: each packet's HP block
// as one lane's whole block behind its keystream entries) for A/B libraries, and the kernels in
// which the new one costs scratch keep it (the kernels over partition lists: chacha_tile).
//
// this packet's 32-B pool record in its wave's scratch: [0] pooled keystream blocks (bits 0-7) | the
// PN length << 8 (3 bits) when the header-protection block is pooled too | for the workgroup MAC
// (cc_wg_mac) the AAD length << 11 (14 bits: a staged packet is under 16 KiB) and kCcRecMac,
// [1] payload LDS offset (workgroup) | P << 17, [2] / [7] mask words 0 / 1 (written by the pool;
// open pools no mask: [2] is the MAC's verdict, tag XOR received tag), [3] key row, [4..6] nonce words
constexpr uint32_t kCcRecMac = 0x80000000u;  // the packet waits for the workgroup MAC
constexpr uint32_t kCcRecAadShift = 11, kCcRecAadMask = 0x3fffu;
struct CcPool {
  bool on;              // wave-uniform: staged tile whose slots >= 16 go to the pool
  uint8_t* wg;          // the workgroup's LDS
  uint32_t base;        // this wave's region in it
  uint32_t* rec;        // this packet's record
  const KeyRow* kt;
  uint32_t role;        // this wave's role in the pool and the MAC phase: its index, or rotated (chacha_tile)
  bool mac;             // workgroup-uniform: the MAC runs as a workgroup phase (cc_wg_mac)
};

// What both pools (cc_pool_run, cc_pool_seal) share. Packet q of the workgroup (tile q / 8, octet
// q % 8) has its record in its wave's scratch behind the image (IMG: bytes of LDS per wave).
template <uint32_t IMG>
__device__ __forceinline__ uint32_t* cc_rec(uint8_t* wg, uint32_t q) {
  return (uint32_t*)(wg + (q >> 3) * IMG + (IMG - kScratchBytes) + 32u * (q & 7));
}
// The packet of pool entry e, given on lane q the entries ex[q] of the packets before packet q (an
// exclusive prefix sum over the KQ packets): the last q with ex[q] <= e, by a binary search whose
// probes are wave shuffles. A packet without entries is never the answer for an entry that exists.
template <uint32_t KQ>
__device__ __forceinline__ uint32_t cc_packet_of(uint32_t ex, uint32_t e) {
  uint32_t q = 0;
#pragma unroll
  for (uint32_t step = KQ / 2; step >= 1; step >>= 1) {
    const uint32_t v = (uint32_t)__shfl((int)ex, (int)(q + step), kWave);
    if (v <= e) q += step;
  }
  return q;
}

// IMG: bytes of LDS per wave (kLdsBytes; the long-packet kernels' larger images, chacha_tile);
// W: waves of the workgroup sharing the pool
// R1 (open's pool of a single-key kernel: keystream blocks only, no header-protection entries):
// the block function takes round one's constant part, computed once per wave (chacha20_round1)
// Sp: the LDS space of the workgroup's staged tiles (LdsSpace, or LdsSpaceRaw: the raw-dword XOR)
template <bool SINGLE, uint32_t IMG = kLdsBytes, uint32_t W = kCcWaves, bool R1 = false, class Sp = LdsSpace>
__device__ __forceinline__ void cc_pool_run(const CcPool& pool, uint32_t tid = threadIdx.x) {
  // role r takes the pool's wave-iterations r, r + W, ...
  static_assert(SINGLE || !R1, "round one is hoisted for wave-uniform keys only");
  constexpr uint32_t kQ = kPktsPerTile * W;  // packets of the workgroup
  static_assert(kQ <= kWave, "one packet per lane in the pool scan");
  const int lane = tid & (kWave - 1);
  const uint32_t w = pool.role;
  auto rec = [&](uint32_t q) -> uint32_t* { return cc_rec<IMG>(pool.wg, q); };
  const uint32_t r0l = (uint32_t)lane < kQ ? rec((uint32_t)lane)[0] : 0u;  // lane q: packet q
  const uint32_t nq = (r0l & 0xffu) + ((r0l >> 8 & 7u) ? 1u : 0u);
  const uint32_t incl = wave_incl_scan(nq), excl = incl - nq;
  const uint32_t T = lane_u32(incl, kWave - 1);
  Sp sp{};
  sp.base = pool.wg;
  for (uint32_t e0 = kWave * w; e0 < T; e0 += kWave * W) {  // wave-uniform
    const uint32_t e = e0 + (uint32_t)lane;
    const uint32_t q = cc_packet_of<kQ>(excl, e);
    const uint32_t eq = (uint32_t)__shfl((int)excl, (int)q, kWave);
    const bool act = e < T;
    uint32_t* r = rec(q);
    const uint32_t r0 = r[0], r1 = r[1], pay = r1 & 0x1ffffu, P = r1 >> 17;
    const uint32_t idx = e - eq, pn_len = r0 >> 8 & 7u;
    const bool hp = !R1 && act && idx == (r0 & 0xffu);  // the packet's last entry: its HP block
    const uint32_t cb = kCcPoolSlot + idx, o = kKsStride * (cb - 1);
    const KeyRow* row = SINGLE || !act ? pool.kt : pool.kt + r[3];  // an idle lane's record may be stale
    uint32_t key[8];
    if (R1) {
      load_key8(row->key, key);
    } else if (SINGLE) {  // both keys wave-uniform (SGPRs); pick per lane
      uint32_t kd[8], kh[8];
      load_key8(row->key, kd);
      load_key8(row->hp, kh);
#pragma unroll
      for (int k = 0; k < 8; ++k) key[k] = hp ? kh[k] : kd[k];
    } else {
      load_key8(hp ? row->hp : row->key, key);
    }
    XorBlock<16, Sp> x;
    x.load(sp, act && !hp ? pay + o : 0u);  // LdsSpaceRaw: in flight during the rounds
    uint32_t smp[4];
    // the sample: 16 bytes at pn_offset + 4 = payload - pn_len + 4 (ciphertext of block 1)
    load_words<4>(sp, hp ? pay + 4u - pn_len : 0u, smp);
    uint32_t ks[16];
    if constexpr (R1)
      chacha20_block(key, cb, r[4], r[5], r[6], chacha20_round1_uniform(key[0], key[1], key[5], row->iv[0]), ks);
    else
      chacha20_block(key, hp ? smp[0] : cb, hp ? smp[1] : r[4], hp ? smp[2] : r[5], hp ? smp[3] : r[6], ks);
    if (hp) {
      r[2] = ks[0];
      r[7] = ks[1];
    } else if (act) {
      x.apply(sp, pay + o, ks, (int)min(64u, P - o));
    }
  }
}

// Seal's pool with the keystream entries ahead of the header-protection entries (above). One scan
// over the records' word 0 gives both prefix sums: the pooled keystream blocks (bits 0-7) in the
// low half, the HP flag (a PN length is recorded) in the high half. Wave-iteration `it` of the pool
// is a keystream iteration for it < NK = ceil(K / 64) (entries 64 it + lane of the K keystream
// entries) and an HP iteration behind them (HP entries 32 (it - NK) + lane / 2 of the H); role r
// takes iterations r, r + W, ... Which kind an iteration is is wave-uniform, and the DPP exchange of
// the pair block runs with every lane active.
// R1: the content key is wave-uniform and round one's part of it hoisted (chacha20_round1_uniform)
template <bool SINGLE, uint32_t IMG = kLdsBytes, uint32_t W = kCcWaves, bool R1 = false, class Sp = LdsSpace>
__device__ __forceinline__ void cc_pool_seal(const CcPool& pool, uint32_t tid = threadIdx.x) {
  static_assert(SINGLE || !R1, "round one is hoisted for wave-uniform keys only");
  constexpr uint32_t kQ = kPktsPerTile * W;  // packets of the workgroup
  static_assert(kQ <= kWave, "one packet per lane in the pool scan");
  static_assert(kQ * 0xffu < 0x10000u, "the keystream prefix sums stay in the low half");
  const int lane = tid & (kWave - 1);
  auto rec = [&](uint32_t q) -> uint32_t* { return cc_rec<IMG>(pool.wg, q); };
  const uint32_t r0l = (uint32_t)lane < kQ ? rec((uint32_t)lane)[0] : 0u;  // lane q: packet q
  const uint32_t nq = (r0l & 0xffu) | ((r0l >> 8 & 7u) ? 0x10000u : 0u);
  const uint32_t incl = wave_incl_scan(nq), excl = incl - nq;
  const uint32_t T = lane_u32(incl, kWave - 1);
  const uint32_t K = T & 0xffffu, H = T >> 16;
  const uint32_t NK = (K + kWave - 1) / kWave, NI = NK + (H + kWave / 2 - 1) / (kWave / 2);
  const uint32_t exk = excl & 0xffffu, exh = excl >> 16;
  Sp sp{};
  sp.base = pool.wg;
  for (uint32_t it = __builtin_amdgcn_readfirstlane(pool.role); it < NI; it += W) {  // wave-uniform
    if (it < NK) {
      const uint32_t e = kWave * it + (uint32_t)lane;
      const uint32_t q = cc_packet_of<kQ>(exk, e);
      const uint32_t eq = (uint32_t)__shfl((int)exk, (int)q, kWave);
      const bool act = e < K;
      const uint32_t* r = rec(q);
      const uint32_t r1 = r[1], pay = r1 & 0x1ffffu, P = r1 >> 17;
      const uint32_t cb = kCcPoolSlot + (e - eq), o = kKsStride * (cb - 1);
      const KeyRow* row = SINGLE || !act ? pool.kt : pool.kt + r[3];  // an idle lane's record may be stale
      uint32_t key[8];
      load_key8(row->key, key);
      XorBlock<16, Sp> x;
      x.load(sp, act ? pay + o : 0u);  // LdsSpaceRaw: in flight during the rounds
      uint32_t ks[16];
      if constexpr (R1)
        chacha20_block(key, cb, r[4], r[5], r[6], chacha20_round1_uniform(key[0], key[1], key[5], row->iv[0]), ks);
      else
        chacha20_block(key, cb, r[4], r[5], r[6], ks);
      if (act) x.apply(sp, pay + o, ks, (int)min(64u, P - o));
    } else {
      const uint32_t h = (uint32_t)lane & 1u, g = (kWave / 2) * (it - NK) + ((uint32_t)lane >> 1);
      const uint32_t q = cc_packet_of<kQ>(exh, g);
      const bool act = g < H;
      uint32_t* r = rec(q);
      const uint32_t pay = r[1] & 0x1ffffu, pn_len = r[0] >> 8 & 7u;
      const KeyRow* row = SINGLE || !act ? pool.kt : pool.kt + r[3];
      // this half's columns of the state: two words each of the constants, of both halves of the
      // HP key and of the sample, the 16 bytes at pn_offset + 4 = payload - pn_len + 4
      const uint2 kb = *(const uint2*)(row->hp + 2u * h), kc = *(const uint2*)(row->hp + 4u + 2u * h);
      uint32_t smp[2];
      load_words<2>(sp, act ? pay + 4u - pn_len + 8u * h : 0u, smp);
      const uint32_t a[2] = {cc_pair_const(h, 0), cc_pair_const(h, 1)}, b[2] = {kb.x, kb.y}, c[2] = {kc.x, kc.y};
      uint32_t m0, m1;
#if MQ_PROF_SKIP & 1  // phase-cost diagnostic build only (tools/phase_cost.py): no rounds
      m0 = a[0] ^ b[0] ^ c[0] ^ smp[0];
      m1 = a[1] ^ b[1] ^ c[1] ^ smp[1];
#else
      chacha20_block_pair(a, b, c, smp, PairSwapDpp{}, m0, m1);
#endif
      if (act && h == 0) {
        r[2] = m0;
        r[7] = m1;
      }
    }
  }
}
// the pool's space for a tile code running on S (the direct path's tiles pool nothing)
template <class S> struct PoolSpace { typedef LdsSpace type; };
template <> struct PoolSpace<LdsSpaceRaw> { typedef LdsSpaceRaw type; };

// ---- MAC phase of a workgroup (the flat octet-tile kernels, chacha_tile) ------------------------
// The per-packet fixed part of the interleaved Poly1305 (the powers of r, the edge steps, the final
// multiply, the group sum and the finish: about 630 of a 1200-B tile's 1120 VALU) is paid per
// wave-instruction stream, which covers 64 / G packets. Between two barriers the MAC of the
// workgroup's 32 packets therefore runs on two waves with G = 4 lanes per packet, 16 packets each,
// instead of on four waves with G = 8: MAC wave m takes packets 16 m .. 16 m + 15 (lane 4 q' + j:
// packet 16 m + q', group lane j). What it needs of a packet waits in the pool record (CcPool) and,
// the one-time key, in the packet's scratch; addresses are the workgroup's. Seal: group lane 0
// stores the tag behind the payload. Open: it writes the verdict (tag XOR received tag) into the
// record and, for a packet that fails, clears the record's pooled blocks, so nothing of it is
// decrypted. The lean stretch's look-ahead reads (poly_tag) end in the next image or in a wave's
// scratch: inside the workgroup's allocation.
// PAIR: poly_tag's pair loop. Off in the multi-key open kernel alone, which measured 0.7 % slower with
// it (124 VGPRs for 120; profiles/r12_ab_bk1024_pair_everywhere.txt).
template <bool OPEN, uint32_t IMG, uint32_t W, bool PAIR = true>
__device__ __forceinline__ void cc_wg_mac(uint8_t* wg, uint32_t m, uint32_t tid) {
  constexpr int G = 4;
  static_assert(kPktsPerTile * W == 2 * (kWave / G), "two MAC waves of 16 packets");
  const int lane = tid & (kWave - 1), j = lane % G;
  const uint32_t q = (kWave / G) * m + (uint32_t)lane / G;
  uint32_t* rec = cc_rec<IMG>(wg, q);
  const uint32_t r0 = rec[0], r1 = rec[1];
  const bool act = (r0 & kCcRecMac) != 0;  // else the record's other words may be stale
  const uint32_t aad_len = act ? r0 >> kCcRecAadShift & kCcRecAadMask : 0u;
  const uint32_t pay = act ? r1 & 0x1ffffu : 0u, P = act ? r1 >> 17 : 0u;
  LdsSpace sp{wg};
  uint32_t tag[4];
  // the key: 8 records on
  poly_tag<G, PAIR>(sp, pay - aad_len, pay, aad_len, P, OtkLds{rec + 8 * kPktsPerTile}, j, act, tag);
  if (OPEN) {
    uint32_t got[4];
    load_words<4>(sp, pay + P, got);
    const uint32_t diff = (tag[0] ^ got[0]) | (tag[1] ^ got[1]) | (tag[2] ^ got[2]) | (tag[3] ^ got[3]);
    if (act && j == 0) {
      rec[2] = diff;
      if (diff) rec[0] = 0;
    }
  } else if (act && j == 0) {
    store_words<4>(sp, pay + P, tag);
  }
}

// The tile code of both layouts: octet tiles (8 lanes per packet, the keystream pool; chacha_tile,
// chacha_protect_tile) and narrow tiles (G = 1, 2, 4 or 8 lanes per packet, no pool; narrow_tile).
struct ChaChaPolicy {
  static constexpr uint32_t kSuite = MQ_SUITE_CHACHA20;

  // RFC 9001 §5.4.1: XOR the mask into the first byte (low 4 / 5 bits) and the PN bytes of a sealed
  // packet whose MAC has been computed (one lane of the packet's group)
  template <class S>
  static __device__ __forceinline__ void apply_hp(const S& sp, typename S::off_t pkt, const mq_pkt_desc& d,
                                                  uint32_t m0, uint32_t m1) {
    sp.st8(pkt, (uint8_t)(sp.ld8(pkt) ^ ((uint8_t)m0 & ((d.flags & MQ_PKT_LONG_HEADER) ? 0x0f : 0x1f))));
    const uint32_t mk = (m0 >> 8) | (m1 << 24);
    for (uint32_t b = 0; b < d.pn_len; ++b)
      sp.st8(pkt + d.pn_offset + b, (uint8_t)(sp.ld8(pkt + d.pn_offset + b) ^ (uint8_t)(mk >> (8 * b))));
  }

  // keystream block `ctr` (>= 1) covers payload [64(ctr-1), min(64 ctr, P)). load_block: the raw
  // HBM dwords under it (direct path; a staged tile XORs in LDS and loads nothing)
  template <class S>
  static __device__ __forceinline__ void load_block(const S& sp, typename S::off_t pay, uint32_t ctr,
                                                    XorBlock<16, S>& x) {
    x.load(sp, pay + kKsStride * (ctr > 0 ? ctr - 1 : 0));
  }
  template <class S>
  static __device__ __forceinline__ void store_block(const S& sp, typename S::off_t pay, uint32_t ctr, uint32_t P,
                                                     const uint32_t (&ks)[16], const XorBlock<16, S>& x) {
    const uint32_t o = kKsStride * (ctr - 1);
    x.apply(sp, pay + o, ks, (int)min(64u, P - o));
  }

  static __device__ __forceinline__ void store_otk(uint32_t* otk, const uint32_t (&ks)[16]) {
    *(uint4*)otk = make_uint4(ks[0], ks[1], ks[2], ks[3]);
    *(uint4*)(otk + 4) = make_uint4(ks[4], ks[5], ks[6], ks[7]);
  }

  // ChaChaHeaderProtection::mask (rustcrypto.rs:197-220): block(hp, ctr = sample[0..4] LE,
  // nonce = sample[4..16]); the mask is keystream bytes 0..4.
  static __device__ __forceinline__ void hp_mask_words(const uint32_t (&smp)[4], const KeyRow* row, uint32_t& m0,
                                                       uint32_t& m1) {
    uint32_t hk[8], blk[16];
    load_key8(row->hp, hk);
    chacha20_block(hk, smp[0], smp[1], smp[2], smp[3], blk);
    m0 = blk[0];
    m1 = blk[1];
  }
  template <class S>
  static __device__ __forceinline__ void hp_mask(const S& sp, typename S::off_t sample_at,
                                                 const KeyRow* row, uint32_t& m0, uint32_t& m1) {
    uint32_t smp[4];
    load_words<4>(sp, sample_at, smp);
    hp_mask_words(smp, row, m0, m1);
  }

  // What both send composites start from: the packet's content key and nonce, and its geometry
  template <class S>
  struct SealPkt {
    uint32_t key[8], n0, n1, n2;
    uint32_t aad_len, P;      // header (the AAD) and payload bytes
    uint32_t nblk;            // ChaCha20 blocks: 0 = Poly1305 key, 1.. = keystream
    typename S::off_t pay;    // the payload
    bool hp;                  // header protection applies (records and plain AEAD rows have none)

    // SCALAR: wave-uniform key material goes to SGPRs. Else it is pinned, and the nonce always is:
    // their loads retire before the caller issues the stager's LDS-DMA (else the first wait covers
    // the DMA too).
    template <bool SCALAR>
    __device__ __forceinline__ void load(typename S::off_t pkt, const PktCtx& c, const KeyRow* row) {
      const mq_pkt_desc& d = c.d;
      load_key8(row->key, key);
      aad_len = c.act ? (uint32_t)d.pn_offset + d.pn_len : 0u;
      P = c.act ? d.len - aad_len - 16 : 0u;
      pay = pkt + aad_len;
      // DirectionalKeys::nonce (src/crypto/mod.rs:66-74): iv ^ (0^32 || BE64(pn))
      n0 = row->iv[0];
      n1 = row->iv[1] ^ bswap32((uint32_t)(c.pn >> 32));
      n2 = row->iv[2] ^ bswap32((uint32_t)c.pn);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (SCALAR) key[i] = __builtin_amdgcn_readfirstlane(key[i]);
        else pin(key[i]);
      }
      pin(n0); pin(n1); pin(n2);
      nblk = 1 + (P + 63) / 64;
      hp = c.act && !(d.flags & MQ_PKT_NO_HP);
    }
  };

  // What both end with: the tag behind the payload, then header protection (transmit.rs:713-738)
  // now that the MAC has read the unprotected header. have: the packet's mask (m0, m1) was made in
  // a keystream slot and is on group lane jh; the other packets' masks this wave computes late, on
  // every lane of the group. store_tag false: the workgroup MAC has stored the tag.
  template <class S>
  static __device__ __forceinline__ void seal_finish(const S& sp, typename S::off_t pkt, const PktCtx& c,
                                                     const KeyRow* row, int j, const SealPkt<S>& k,
                                                     const uint32_t (&tag)[4], bool have, int jh, uint32_t m0,
                                                     uint32_t m1, bool store_tag = true) {
    if (store_tag && c.act && j == 0) store_words<4>(sp, k.pay + k.P, tag);
    const bool late = k.hp && !have;
    if (wave_any(late)) {
      wave_sync();  // ciphertext and tags are in place
      uint32_t a0, a1;
      hp_mask(sp, pkt + c.d.pn_offset + 4, row, a0, a1);
      if (late) {
        m0 = a0;
        m1 = a1;
      }
    }
    wave_sync();
    if (k.hp && j == jh) apply_hp(sp, pkt, c.d, m0, m1);
    wave_sync();
  }

  // send composite (transmit.rs:625-755): keystream block ctr of the packet runs on lane ctr % 8 in
  // iteration ctr / 8 (ctr 0 = the Poly1305 key); with the pool, blocks >= 16 and the
  // header-protection block (its sample is ciphertext of block 1) run in the workgroup's pool
  // before the MACs, and the mask is applied once the MAC has read the unprotected header.
  // R1: round one's wave-uniform part hoisted (single-key kernels; chacha_tile says which)
  // WG: the kernel has the workgroup MAC phase (cc_wg_mac), taken when pool.mac says so: a staged
  // tile hands its packets over in their records; a direct-path tile MACs itself, as without the
  // phase, but runs the phase's barrier and its role
  // HP2: the pool runs its header-protection blocks on lane pairs behind the keystream blocks
  // (cc_pool_seal), else as single-lane entries among them (cc_pool_run)
  template <bool SINGLE, uint32_t IMG = kLdsBytes, uint32_t W = kCcWaves, bool R1 = false, bool WG = false,
            bool HP2 = false, class S, class St>
  static __device__ __forceinline__ void seal(const S& sp, typename S::off_t pkt, PktCtx& c, const KeyRow* row, int j,
                                              St& stg, const CcPool& pool) {
    const mq_pkt_desc& d = c.d;
    SealPkt<S> k;
    k.template load<false>(pkt, c, row);
    const uint32_t P = k.P, nblk = k.nblk;
    const typename S::off_t pay = k.pay;
    stg.issue();  // packet bytes stream into LDS while the first keystream block is computed
    const uint32_t kst = pool.on ? min(nblk, kCcPoolSlot) : nblk;  // blocks of this wave's own slots
    const uint32_t Imax = wave_max_u32(c.act ? (kst + kLanesPerPkt - 1) / kLanesPerPkt : 0u);
    // single key: the key and nonce word 0 are wave-uniform, so is round one's part of them
    ChaChaRound1 r1{};
    static_assert(SINGLE || !R1, "round one is hoisted for wave-uniform keys only");
    if constexpr (R1) r1 = chacha20_round1_uniform(k.key[0], k.key[1], k.key[5], k.n0);
    for (uint32_t it = 0; it < Imax; ++it) {
      const uint32_t ctr = (uint32_t)j + kLanesPerPkt * it;
      const bool a = c.act && ctr < kst;
      XorBlock<16, S> w;
      if (it > 0) load_block(sp, pay, a ? ctr : 0u, w);  // direct path: in flight during the block function
      uint32_t ks[16];
      if constexpr (R1) {
        // the nonce words opaque per iteration: hipcc would otherwise compute columns 2 and 3 of
        // round one once for both iterations and hold them (8 VGPRs: 128 and 20 B of scratch)
        uint32_t m1 = k.n1, m2 = k.n2;
        pin(m1); pin(m2);
        chacha20_block(k.key, ctr, k.n0, m1, m2, r1, ks);
      } else {
        chacha20_block(k.key, ctr, k.n0, k.n1, k.n2, ks);
      }
      if (it == 0) {
        stg.complete();
        MQ_STAMP(c.tile, 2);
        const bool rec = c.act && is_record(d);
        if (wave_any(rec)) {  // TLS record: header (AAD) and inner content type before any use
          if (rec && j == 0) write_record_header(sp, pkt, d);
          wave_sync();
        }
        load_block(sp, pay, a ? ctr : 0u, w);
      }
      if (a && ctr == 0) {
        store_otk(c.otk, ks);  // the Poly1305 key waits in LDS until the MAC
      } else if (a) {
        store_block(sp, pay, ctr, P, ks, w);
      }
      wave_sync();
    }
    if (Imax == 0) stg.complete();
    // the pool takes the HP block when the sample (payload bytes [4 - pn_len, 20 - pn_len)) is all
    // ciphertext; for tiny payloads it reaches into the tag, which only the MAC below produces
    const bool hp_pool = pool.on && k.hp && P + d.pn_len >= 20u;
    const bool wgm = WG && pool.mac;                 // workgroup-uniform
    const bool handed = wgm && pool.on;              // wave-uniform: the workgroup MACs this tile
    if (j == 0) {  // pool record: keystream blocks >= 16 and the HP block; the MAC's inputs
      const uint32_t np = pool.on && c.act && nblk > kCcPoolSlot ? nblk - kCcPoolSlot : 0u;
      const uint32_t hpn = hp_pool ? (uint32_t)d.pn_len : 0u;  // 1..4 (validated)
      const uint32_t mac = handed && c.act ? kCcRecMac | k.aad_len << kCcRecAadShift : 0u;
      pool.rec[0] = np | hpn << 8 | mac;
      if (np || hpn || mac) {
        pool.rec[1] = (pool.base + (uint32_t)pay) | P << 17;
        pool.rec[3] = d.key_id;
        pool.rec[4] = k.n0; pool.rec[5] = k.n1; pool.rec[6] = k.n2;
      }
    }
    __syncthreads();  // every wave's records
    if constexpr (HP2) cc_pool_seal<SINGLE, IMG, W, R1, typename PoolSpace<S>::type>(pool);
    else cc_pool_run<SINGLE, IMG, W, false, typename PoolSpace<S>::type>(pool);
    __syncthreads();  // every pooled block (and mask) is in place before any MAC reads it
    MQ_STAMP(c.tile, 3);
    uint32_t tag[4] = {0, 0, 0, 0};
    if (!handed) poly_tag<kLanesPerPkt>(sp, pkt, pay, k.aad_len, P, OtkLds{c.otk}, j, c.act, tag);
    if (WG && wgm) {
      if (pool.role >= W - 2) cc_wg_mac<false, IMG, W>(pool.wg, pool.role - (W - 2), threadIdx.x);
      __syncthreads();  // every tag is in place
    }
    // the pooled mask waits in the record; without one (direct path, or a sample that reaches
    // into the tag) the wave computes it late; octet lane 0 applies either
    uint32_t m0 = 0, m1 = 0;
    if (hp_pool) {
      m0 = pool.rec[2];
      m1 = pool.rec[7];
    }
    seal_finish(sp, pkt, c, row, j, k, tag, hp_pool, 0, m0, m1, !handed);
    MQ_STAMP(c.tile, 4);
  }

  // send composite (transmit.rs:625-755) on a narrow tile. Slot order: keystream blocks 1 .. nblk-1
  // first, the one-time key (block 0) in slot nblk - 1 — made last, so its 8 words are not held
  // through the loop — then the header-protection block in slot nblk.
  template <int G, bool SINGLE, class S, class St>
  static __device__ __forceinline__ void seal_narrow(const S& sp, typename S::off_t pkt, PktCtx& c, const KeyRow* row,
                                                     int j, St& stg) {
    const mq_pkt_desc& d = c.d;
    SealPkt<S> k;
    k.template load<SINGLE>(pkt, c, row);  // a single-key tile keeps its key in SGPRs
    const uint32_t P = k.P, nblk = k.nblk;
    const typename S::off_t pay = k.pay;
    stg.issue();
    // the header-protection block in slot nblk: its sample (payload [4 - pn_len, 20 - pn_len)) is
    // ciphertext of keystream block 1 (slot 0, iteration 0), so slot nblk must fall in a later
    // iteration (nblk >= G), and must not reach into the tag (only the MAC produces it)
    const bool hp_in = k.hp && P + d.pn_len >= 20u && nblk >= (uint32_t)G;
    const uint32_t S_ = nblk + (hp_in ? 1u : 0u);
    const uint32_t Imax = wave_max_any(c.act ? (S_ + G - 1) / G : 0u);
    uint32_t otk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m0 = 0, m1 = 0;
    for (uint32_t it = 0; it < Imax; ++it) {
      const uint32_t slot = (uint32_t)j + G * it;
      const bool is_otk = c.act && slot + 1 == nblk;
      const uint32_t ctr = is_otk ? 0u : slot + 1;  // keystream block of the slot
      const bool a = c.act && ctr < nblk;            // a keystream block (or the one-time key)
      const bool is_hp = hp_in && slot == nblk;
      uint32_t ks[16];
      if (wave_any(is_hp)) {  // the HP lanes run the HP key on the sample (ciphertext by now)
        uint32_t smp[4], kh[8], kk[8];
        load_words<4>(sp, is_hp ? pay + 4u - d.pn_len : pay, smp);
        load_key8(row->hp, kh);
#pragma unroll
        for (int i = 0; i < 8; ++i) kk[i] = is_hp ? kh[i] : k.key[i];
        chacha20_block(kk, is_hp ? smp[0] : ctr, is_hp ? smp[1] : k.n0, is_hp ? smp[2] : k.n1, is_hp ? smp[3] : k.n2,
                       ks);
      } else {
        chacha20_block(k.key, ctr, k.n0, k.n1, k.n2, ks);
      }
      if (it == 0) {
        stg.complete();
        const bool rec = c.act && is_record(d);
        if (wave_any(rec)) {  // TLS record: header (AAD) and inner content type before any use
          if (rec && j == 0) write_record_header(sp, pkt, d);
          wave_sync();
        }
      }
      // direct path: the block's raw words after the rounds (not in flight during them: 17 VGPRs fewer)
      XorBlock<16, S> w;
      load_block(sp, pay, a && !is_otk ? ctr : 0u, w);
      if (is_otk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) otk[i] = ks[i];
      } else if (a) {
        store_block(sp, pay, ctr, P, ks, w);
      }
      if (is_hp) {
        m0 = ks[0];
        m1 = ks[1];
      }
      wave_sync();
    }
    if (Imax == 0) stg.complete();
    // the one-time key from its group lane (nblk - 1) % G to the whole group
    OtkRegs rs;
    uint32_t tag[4];
    const int src = (int)(threadIdx.x & (kWave - 1)) - j + (int)((nblk + G - 1) % G);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rs.rk[i] = G == 1 ? otk[i] : (uint32_t)__shfl((int)otk[i], src, kWave);
      rs.sk[i] = G == 1 ? otk[4 + i] : (uint32_t)__shfl((int)otk[4 + i], src, kWave);
    }
    poly_tag<G>(sp, pkt, pay, k.aad_len, P, rs, j, c.act, tag);
    // the mask is on group lane nblk % G when slot nblk made it; tiny payloads and G > nblk: one
    // more block for the wave
    seal_finish(sp, pkt, c, row, j, k, tag, hp_in, hp_in ? (int)(nblk % G) : 0, m0, m1);
  }

  // receive composite (recv.rs:340-421 / 953-1025): HP removal, decode_pn, open — verify, only then
  // decrypt. G lanes per packet. POOL (the octet tiles of chacha_tile): the one-time key goes
  // through the packet's LDS scratch and keystream blocks >= 16 to the workgroup's pool, both
  // barriers included; else (narrow tiles) the key travels by DPP and the wave runs every block.
  // R1: round one's wave-uniform part hoisted (single-key octet kernels; chacha_tile says which)
  // WG: the kernel has the workgroup MAC phase (cc_wg_mac), taken when pool.mac says so. A staged
  // tile then writes its pool records before the MAC, as if every packet verified (the MAC clears
  // a failed packet's), hands its packets over between two barriers and takes the verdicts; the
  // pool follows the wave's own blocks with no barrier of its own. A direct-path tile MACs itself
  // and runs the same barriers and its role first, while little is live (the role's registers on
  // top of the direct path's spilled).
  template <int G, bool POOL, bool SINGLE, uint32_t IMG = kLdsBytes, uint32_t W = kCcWaves, bool R1 = false,
            bool WG = false, class S, class St>
  static __device__ __forceinline__ void open(const S& sp, typename S::off_t pkt, PktCtx& c, const KeyRow* row, int j,
                                              bool direct, St& stg, const CcPool& pool = CcPool{}) {
    typedef Grp<G> Gp;
    const mq_pkt_desc& d = c.d;
    constexpr bool kDirect = std::is_same<S, GlobalSpace>::value;
    if constexpr (WG && POOL && kDirect) {
      if (pool.mac) {  // nothing to hand over
        if (j == 0) pool.rec[0] = 0;
        __syncthreads();
        if (pool.role >= W - 2) cc_wg_mac<true, IMG, W, SINGLE>(pool.wg, pool.role - (W - 2), threadIdx.x);
        __syncthreads();
      }
    }
    stg.issue();
    uint32_t pn_len = d.pn_len, trunc = 0;
    uint8_t orig_b0 = 0, b0 = 0;
    uint32_t orig_pn = 0;
    const bool hp = c.act && !(d.flags & MQ_PKT_NO_HP);
    // recv.rs:363-395 / :968-997: mask, unmask byte 0, pn_len, unmask PN, decode_pn. With the
    // pre-pass (wave-uniform) those values arrive with the descriptor, so the nonce and the first
    // keystream block are computed while the packet is still landing in LDS.
    if (c.pre_hp) {
      if (hp) b0 = header_from_prepass(c, pn_len, trunc);
    } else {
      stg.complete();
      if (wave_any(hp)) {  // every lane of a group computes its packet's mask (one block for the wave)
        uint32_t m0, m1;
        hp_mask(sp, hp ? pkt + d.pn_offset + 4 : pkt, row, m0, m1);
        if (hp) b0 = header_from_mask(sp, pkt, c, m0, m1, pn_len, trunc);
      }
    }
    uint32_t key[8];
    load_key8(row->key, key);
    const uint32_t aad_len = c.act ? (uint32_t)d.pn_offset + pn_len : 0u;
    const uint32_t P = c.act ? d.len - aad_len - 16 : 0u;
    const typename S::off_t pay = pkt + aad_len;
    const uint32_t n0 = row->iv[0], n1 = row->iv[1] ^ bswap32((uint32_t)(c.pn >> 32)),
                   n2 = row->iv[2] ^ bswap32((uint32_t)c.pn);
    const uint32_t nblk = 1 + (P + 63) / 64;
    const uint32_t Cmax = Gp::wave_max(c.act ? (nblk + G - 1) / G : 0u);
    // first keystream block of every lane is computed before the MAC (group lane 0: one-time key)
    const uint32_t ctr0 = (uint32_t)j;
    // octet tiles of a single-key kernel: round one's wave-uniform part once for every block
    static_assert((POOL && SINGLE) || !R1, "round one is hoisted for wave-uniform keys only");
    constexpr bool kR1 = R1;
    ChaChaRound1 r1{};
    if constexpr (kR1) r1 = chacha20_round1_uniform(row->key[0], row->key[1], row->key[5], row->iv[0]);
    uint32_t ks0[16];
    if constexpr (kR1) chacha20_block(key, ctr0, n0, n1, n2, r1, ks0);
    else chacha20_block(key, ctr0, n0, n1, n2, ks0);
    if (c.pre_hp) stg.complete();
    if (POOL) MQ_STAMP(c.tile, 2);
    const bool hdr_written = hp && write_unmasked_header(sp, pkt, c, j, b0, pn_len, trunc, orig_b0, orig_pn);
    if (POOL) MQ_STAMP(c.tile, 3);
    if (POOL && c.act && j == 0) store_otk(c.otk, ks0);
    wave_sync();
    const bool wgm = WG && POOL && pool.mac;  // workgroup-uniform
    const bool handed = wgm && !kDirect;       // the workgroup MACs this tile
    auto pool_record = [&]() {  // octet lane 0. Only verified packets are decrypted (no HP block on open)
      const uint32_t np = pool.on && c.act && nblk > kCcPoolSlot ? nblk - kCcPoolSlot : 0u;
      const uint32_t mac = handed && c.act ? kCcRecMac | aad_len << kCcRecAadShift : 0u;
      pool.rec[0] = np | mac;
      if (np || mac) {
        pool.rec[1] = (pool.base + (uint32_t)pay) | P << 17;
        pool.rec[3] = d.key_id;
        pool.rec[4] = n0; pool.rec[5] = n1; pool.rec[6] = n2;
      }
    };
    uint32_t tag[4] = {0, 0, 0, 0}, got[4] = {0, 0, 0, 0};
    if (POOL) {
      if (!handed) poly_tag<G>(sp, pkt, pay, aad_len, P, OtkLds{c.otk}, j, c.act, tag);
    } else {
      OtkRegs rs;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rs.rk[i] = Gp::bcast0(ks0[i]);
        rs.sk[i] = Gp::bcast0(ks0[4 + i]);
      }
      poly_tag<G>(sp, pkt, pay, aad_len, P, rs, j, c.act, tag);
    }
    if (!handed) load_words<4>(sp, pay + P, got);
    uint32_t diff = (tag[0] ^ got[0]) | (tag[1] ^ got[1]) | (tag[2] ^ got[2]) | (tag[3] ^ got[3]);
    if constexpr (WG && POOL && !kDirect) {
      if (wgm) {
        if (j == 0) pool_record();
        __syncthreads();  // every wave's records, keys and unmasked headers
        if (pool.role >= W - 2) cc_wg_mac<true, IMG, W, SINGLE>(pool.wg, pool.role - (W - 2), threadIdx.x);
        __syncthreads();  // every verdict; every MAC has read its ciphertext
        if (handed && c.act) diff = pool.rec[2];
      }
    }
    if (c.act && diff != 0) {  // Error::Crypto, buffer left as received
      c.st = MQ_ERR_CRYPTO;
      c.act = false;
    }
    wave_sync();  // every lane's MAC reads precede any plaintext write
    if (POOL) MQ_STAMP(c.tile, 4);
    if (c.act && ctr0 >= 1 && ctr0 < nblk) {
      XorBlock<16, S> w;
      load_block(sp, pay, ctr0, w);
      store_block(sp, pay, ctr0, P, ks0, w);
    }
    const uint32_t Cown = POOL && pool.on ? min(Cmax, kCcOwnIters) : Cmax;  // later slots: the workgroup's pool
    for (uint32_t it = 1; it < Cown; ++it) {
      const uint32_t ctr = (uint32_t)j + G * it;
      const bool a = c.act && ctr < nblk;
      XorBlock<16, S> w;
      load_block(sp, pay, a ? ctr : 0u, w);
      uint32_t ks[16];
      if constexpr (kR1) chacha20_block(key, ctr, n0, n1, n2, r1, ks);
      else chacha20_block(key, ctr, n0, n1, n2, ks);
      if (a) store_block(sp, pay, ctr, P, ks, w);
    }
    if constexpr (POOL) {
      if (!wgm) {
        if (j == 0) pool_record();
        __syncthreads();  // every wave's MAC has read its ciphertext
      }
      cc_pool_run<SINGLE, IMG, W, R1, typename PoolSpace<S>::type>(pool);
      __syncthreads();
      MQ_STAMP(c.tile, 5);
    } else {
      wave_sync();
    }
    if (direct && hdr_written && !c.act) {  // direct path writes HBM in place: undo the unmask
      sp.st8(pkt, orig_b0);
      for (uint32_t b = 0; b < pn_len; ++b) sp.st8(pkt + d.pn_offset + b, (uint8_t)(orig_pn >> (8 * b)));
    }
  }
};

// ---- narrow tiles: G lanes per packet, 64 / G packets per wave (r05) ---------------------------
// The octet tile gives every packet 8 lanes whatever its length. A 64-B packet needs 2 ChaCha20
// blocks (one-time key, one keystream block) and 5 MAC blocks, so 3/4 of its octet's keystream
// slots idle and the per-packet work (powers of r, the final multiply, the octet reduction, the
// header-protection block, descriptor and placement) is paid per 8 packets: flat 64-B batches ran
// at 122 GiB/s against 1034 at 1200 B. A narrow tile packs Q = 64 / G packets into
// the wave with G in {1, 2, 4} (G = 8: the octet layout without the keystream pool): keystream
// block c of a packet on group lane c % G in iteration c / G, the header-protection block as the
// packet's next slot when it falls in a later iteration than keystream block 1 (whose ciphertext
// is its sample), the MAC a G-way interleaved Horner (multiplier r^G, final r^(G-j), group sum).
// No LDS scratch: the one-time key travels by DPP from group lane 0, the mask stays in the
// registers of the lane that made it, so the whole 10 KiB minus a 64-B read slack holds images.
// Staging maps image chunk c (lane-linear LDS destination, as LDS-DMA requires) to its packet by a
// binary search over the tile's slots; write-back runs per packet, chunk j, j + G, ... on group
// lane j. Used by flat ChaCha20 batches of short packets (mq_launch_chacha picks the narrow kernel
// by the arena's bytes per packet) and by the short length classes of a mixed batch's ChaCha20 list
// (mq_partition.hip regions).
constexpr uint32_t kNarrowSlack = 64;                              // xor_words overreach past an image
constexpr uint32_t kNarrowChunks = (kLdsBytes - kNarrowSlack) / 16;  // 636

template <int G>
struct NarrowStager {
  static constexpr int Q = kWave / G;
  uint8_t* smem;
  const uint8_t* arena;
  uint64_t arena_len;
  uint32_t total;  // image chunks of the tile
  uint32_t slot;   // this lane's packet: first chunk (group-uniform)
  uint64_t base;   // its image start in the arena (16-B aligned)
  int lane;
  uint32_t nch;    // its image chunks (a gap may follow them: narrow_tile)
  uint32_t tail_c = 0xFFFFFFFFu;  // a chunk that would read past the arena end: guarded load
  uint64_t tail_src = 0;

  // the packet of image chunk c < total: the last q with slot_q <= c (an empty packet shares the
  // next one's slot; the later one of equal slots is the one with chunks)
  __device__ __forceinline__ uint32_t owner(uint32_t c) const {
    uint32_t q = 0;
#pragma unroll
    for (int step = Q / 2; step >= 1; step >>= 1) {
      const uint32_t v = (uint32_t)__shfl((int)slot, G * (int)(q + step), kWave);
      if (v <= c) q += step;
    }
    return q;
  }
  __device__ __forceinline__ void issue() {
#if MQ_PROF_SKIP & 8
    return;
#endif
    for (uint32_t k = 0; k < total; k += kWave) {  // wave-uniform
      const uint32_t c = k + (uint32_t)lane;
      const uint32_t q = owner(c < total ? c : 0u);
      const uint32_t sq = (uint32_t)__shfl((int)slot, G * (int)q, kWave);
      const uint64_t bq = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(base >> 32), G * (int)q, kWave) << 32 |
                          (uint32_t)__shfl((int)(uint32_t)base, G * (int)q, kWave);
      const uint64_t src = bq + 16ull * (c - sq);
      const uint32_t nq = (uint32_t)__shfl((int)nch, G * (int)q, kWave);
      if (c < total && c - sq < nq) {  // not a gap chunk
        if (src + 16 <= arena_len)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(arena + src),
                                           (__attribute__((address_space(3))) void*)(smem + 16u * k), 16, 0, 0);
        else {
          tail_c = c;
          tail_src = src;
        }
      }
    }
  }
  __device__ __forceinline__ void complete() {
    wave_sync();  // s_waitcnt vmcnt(0) covers the LDS-DMA writes
    if (tail_c != 0xFFFFFFFFu) *(uint4*)(smem + 16u * tail_c) = load_chunk_guarded(arena, tail_src, arena_len);
    wave_sync();
  }
};

// LDS -> HBM of a narrow tile's packets with write = 1: group lane j stores chunks j, j + G, ... of
// its packet, whole chunks with 16-B stores, the partial first / last chunk byte-exact (bytes of
// neighbouring packets are never touched)
template <int G>
__device__ __forceinline__ void narrow_stage_out(const uint8_t* smem, uint8_t* arena, int j, bool write,
                                                 const Placement& pl) {
#if MQ_PROF_SKIP & 4
  return;
#endif
  const uint32_t nch = write ? pl.nch() : 0u, head = pl.head();
  const uint32_t tail_end = ((head + pl.len - 1u) & 15u) + 1u;
  const uint32_t nmax = wave_max_any(nch);
  uint8_t* dst = arena + pl.base();
  const uint8_t* src = smem + 16u * pl.slot;
  for (uint32_t c = (uint32_t)j; c < nmax + (uint32_t)j; c += G) {  // wave-uniform trip count (nmax / G)
    if (c < nch) {
      const uint32_t lo = c == 0 ? head : 0u, hi = c + 1 == nch ? tail_end : 16u;
      const uint4 v = *(const uint4*)(src + 16u * c);
      if (lo == 0 && hi == 16) {
        *(uint4*)(dst + 16u * c) = v;
      } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t b = lo; b < hi; ++b) dst[16u * c + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
      }
    }
  }
}

// One narrow tile: entries [e0, e0 + Q) of the batch (index != null: of the list `index`, holes
// skipped; else descriptor indices), count = the entries' end. Every lane of the wave calls it.
// RAW: the keystream XOR of staged tiles in its raw-dword form (LdsSpaceRaw; chacha_tile)
template <int G, bool OPEN, bool SINGLE, bool RAW = false>
__device__ __forceinline__ void narrow_tile(uint8_t* wsm, const KeyRow* __restrict__ kt, uint32_t n_rows,
                                            uint8_t* __restrict__ arena, uint64_t arena_len,
                                            const mq_pkt_desc* __restrict__ desc, uint32_t e0, uint32_t count,
                                            const uint32_t* __restrict__ index, uint8_t* __restrict__ status,
                                            uint64_t* __restrict__ pn_out, const uint2* __restrict__ hpm) {
  constexpr int Q = kWave / G;
  const int lane = threadIdx.x & (kWave - 1), j = lane % G;
  PktCtx c;
  const KeyRow* row;
  if (!tile_ctx<MQ_SUITE_CHACHA20, OPEN, SINGLE, G>(0, kt, n_rows, arena_len, desc, count, index, nullptr, hpm,
                                                    TilePrefetch{false, 0u, 0u}, c, row, threadIdx.x, e0))
    return;  // no entry left for this tile
  c.otk = nullptr;
  Placement pl;
  pl.off = c.act ? c.d.offset : 0;
  pl.len = c.act ? c.d.len : 0u;
  const uint64_t nch64 = c.act ? ((pl.off & 15) + (uint64_t)c.d.len + 15) >> 4 : 0u;
  const uint32_t nch = (uint32_t)(nch64 < 0xFFFFu ? nch64 : 0xFFFFu);
  // equal even image sizes (e.g. 256-B packets: 16 chunks) would put every packet's blocks on the
  // same LDS banks: a one-chunk gap after each image when packet 0's size is even and the budget
  // has room (as chacha_tile)
#ifndef MQ_CC_NOPAD  // diagnostic A/B build only: no gaps
  const uint32_t t0 = lane_u32(wave_incl_scan(j == 0 ? nch : 0u), kWave - 1);
  const uint32_t pad = (lane_u32(nch, 0) & 1u) == 0 && t0 + (uint32_t)Q <= kNarrowChunks ? 1u : 0u;
#else
  const uint32_t pad = 0;
#endif
  const uint32_t incl = pad ? wave_incl_scan(j == 0 ? nch + 1u : 0u) : wave_incl_scan(j == 0 ? nch : 0u);
  const uint32_t total = lane_u32(incl, kWave - 1);
  if (total <= kNarrowChunks) {
    pl.slot = incl - nch - pad;
    NarrowStager<G> stg{wsm, arena, arena_len, total, pl.slot, pl.base(), lane, nch};
    typename std::conditional<RAW, LdsSpaceRaw, LdsSpace>::type sp{};
    sp.base = wsm;
    const uint32_t pkt = pl.slot * 16u + pl.head();
    if (OPEN) ChaChaPolicy::open<G, false, SINGLE>(sp, pkt, c, row, j, false, stg);
    else ChaChaPolicy::seal_narrow<G, SINGLE>(sp, pkt, c, row, j, stg);
    wave_sync();
    narrow_stage_out<G>(wsm, arena, j, c.act, pl);
  } else {
    GlobalSpace sp{arena, arena_len};
    NoStager stg;
    if (OPEN) ChaChaPolicy::open<G, false, SINGLE>(sp, pl.off, c, row, j, true, stg);
    else ChaChaPolicy::seal_narrow<G, SINGLE>(sp, pl.off, c, row, j, stg);
  }
  tile_status<OPEN>(c, j, status, pn_out);
}

}  // namespace mq

using namespace mq;

// Tile kernels: one tile per wave, each with its private 10 KiB LDS image, kCcWaves-wave
// workgroups sharing the keystream pool above between two barriers (and, in the flat 10-KiB
// kernels, the MAC phase, cc_wg_mac, between two more). Every wave of a workgroup
// runs every barrier: waves past the batch with an empty record, direct-path tiles (images over
// the budget) with nothing pooled. (A persistent grid walking
// tiles, as the AES kernels use, measured 10 % slower here: identical waves stay in phase, so
// their staging waits line up.) The "1" variants are launched when the key table has a single
// row (every valid packet on row 0): key material then lives in SGPRs.
// tb: the workgroup's block of W tiles (blockIdx.x, or the persistent kernels' current block)
// tid: threadIdx.x (the persistent list kernels pass an opaque copy per tile, so nothing derived
// from it is hoisted out of their loop and held across every tile — that pressure spilled)
// A partition list's narrow regions (mq_partition.hip: reg = tiles of G = 8, 4, 2, 1, then the first
// entries of the G = 4, 2, 1 regions): list tile u >= T8 is narrow tile u - T8 of the G = 4 region,
// and so on. Runs it, if there is one.
template <bool OPEN, bool SINGLE, bool RAW>
__device__ __forceinline__ void chacha_narrow_list(uint8_t* wsm, uint32_t u, const uint32_t* __restrict__ reg,
                                                   const KeyRow* __restrict__ kt, uint32_t n_rows,
                                                   uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const mq_pkt_desc* __restrict__ desc,
                                                   const uint32_t* __restrict__ index, uint8_t* __restrict__ status,
                                                   uint64_t* __restrict__ pn_out, const uint2* __restrict__ hpm) {
  const uint32_t T8 = reg[0], T4 = reg[1], T2 = reg[2], T1 = reg[3], R4 = reg[4], R2 = reg[5], R1 = reg[6];
  if (u < T8) return;
  uint32_t v = u - T8;
  if (v < T4) {
    narrow_tile<4, OPEN, SINGLE, RAW>(wsm, kt, n_rows, arena, arena_len, desc, R4 + 16 * v, R4 + 16 * T4, index, status,
                                 pn_out, hpm);
    return;
  }
  v -= T4;
  if (v < T2) {
    narrow_tile<2, OPEN, SINGLE, RAW>(wsm, kt, n_rows, arena, arena_len, desc, R2 + 32 * v, R2 + 32 * T2, index, status,
                                 pn_out, hpm);
    return;
  }
  v -= T2;
  if (v < T1)
    narrow_tile<1, OPEN, SINGLE, RAW>(wsm, kt, n_rows, arena, arena_len, desc, R1 + 64 * v, R1 + 64 * T1, index, status,
                                 pn_out, hpm);
}

// LIST: a partition list with narrow regions (reg): the octet tiles are the G = 8 region's (count =
// its entries), a workgroup with an octet tile runs the pool's barriers on every wave (its narrow
// waves run their tile first), one without any runs its narrow tiles with no barrier.
// n_rows carries the MQ_CC_SPAN=0 switch in its top bit (a key table never has 2^31 rows).
constexpr uint32_t kCcNoSpan = 0x80000000u;
// and, one bit down, the MQ_CC_WGMAC=0 switch: the per-wave MAC in the kernels that have the
// workgroup MAC phase
constexpr uint32_t kCcNoWgMac = 0x40000000u;
// Roles of a workgroup's waves: role = (w + h) & 3. The pool's wave-iterations fall on roles 0, 1
// and, for seal, 2, the MAC phase on the last two roles, which carry the least pool work (open:
// none; seal: none and the half-filled iteration with the header-protection blocks). Wave w of a
// workgroup usually sits on SIMD w, so h decides which SIMDs of a CU carry which phase, and the two
// kernels want opposite things (config B, ms per 2^20 packets, profiles/r11_ab_rotation_b.txt;
// parent: seal 0.920, open 0.909):
//                                          seal    open
//   h = 0                                  0.891   0.959
//   h = block >> 8                         1.065   0.894
//   h = top bits of block * 0x9E3779B1     0.937   0.944
// Seal runs pool then MAC: with h = 0 the workgroups of a CU that are in different phases use
// different SIMDs. Open runs the MAC first, beside other workgroups' staging waits; there the four
// workgroups that share a CU want four different rotations, and under round-robin dispatch over
// 256 CUs those are blocks 256 apart. Neither mapping is promised by the hardware: no result
// depends on h, only the time. -DMQ_CC_ROLE_FIXED builds h = 0 for both.
template <bool OPEN>
__device__ __forceinline__ uint32_t cc_role(uint32_t tb, uint32_t w, uint32_t W) {
#ifdef MQ_CC_ROLE_FIXED
  (void)tb;
  return w & (W - 1);
#else
  return (w + (OPEN ? tb >> 8 : 0u)) & (W - 1);
#endif
}
// SPAN = false: no span tiles in this kernel, whatever the switch says (chacha_list).
template <bool OPEN, bool SINGLE, bool LIST = false, uint32_t IMG = kLdsBytes, uint32_t W = kCcWaves, bool SPAN = true>
__device__ __forceinline__ void chacha_tile(uint32_t tb, uint32_t tid, const KeyRow* __restrict__ kt, uint32_t n_rows,
                                            uint8_t* __restrict__ arena, uint64_t arena_len,
                                            const mq_pkt_desc* __restrict__ desc, uint32_t n,
                                            const uint32_t* __restrict__ index, const uint32_t* __restrict__ n_dev,
                                            uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,
                                            const uint2* __restrict__ hpm, const uint32_t* __restrict__ reg = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t w = tid >> 6;
  uint8_t* wsm = smem + w * IMG;
  const int lane = tid & (kWave - 1), p = lane / kLanesPerPkt, j = lane % kLanesPerPkt;
  const uint32_t tile_id = tb * W + w;
  // The multi-key seal kernels over partition lists (one-shot and persistent grid) keep the raw-dword
  // XOR: the atomic form costs them scratch (12 and 4 more bytes per lane)
  constexpr bool kRaw = !OPEN && !SINGLE && (LIST || !SPAN);
  typedef typename std::conditional<kRaw, LdsSpaceRaw, LdsSpace>::type Sp;
  // Round one's wave-uniform part is hoisted in the single-key kernels, but not in the persistent
  // list kernels (SPAN = false) nor in the fused protect tile: there it costs scratch (seal list
  // 40 -> 44 B per lane, open list 0 -> 20, protect 0 -> 8)
  constexpr bool kR1 = SINGLE && SPAN;
  // The workgroup MAC phase (cc_wg_mac) and the rotating roles: the flat kernels over 10-KiB images
  constexpr bool kWg = SPAN && !LIST && IMG == kLdsBytes && W == 4;
  // Seal's pool with the header-protection blocks on lane pairs (cc_pool_seal): the flat kernels of
  // every image size, where it changes neither registers nor scratch. Not the kernels over partition
  // lists, where it costs scratch (bytes per lane: seal lgrid 0 -> 12, seal list 40 -> 72, seal
  // list1 36 -> 40; lgrid1 one VGPR). The fused protect tile takes it too (kProtectHp2).
#ifdef MQ_CC_HP_INTERLEAVED
  constexpr bool kHp2 = false;
#else
  constexpr bool kHp2 = !OPEN && !LIST && SPAN;
#endif
  const bool span_ok = SPAN && (n_rows & kCcNoSpan) == 0;
  const bool wgm = kWg && (n_rows & kCcNoWgMac) == 0;
  n_rows &= ~(kCcNoSpan | kCcNoWgMac);
  PktCtx c;
  const KeyRow* row;
  constexpr uint32_t kBudget = IMG - kScratchBytes;  // packet images (9728 B at 10 KiB)
  CcPool pool{false, smem, w * IMG, (uint32_t*)(wsm + kBudget + 32u * (uint32_t)p), kt, kWg ? cc_role<OPEN>(tb, w, W) : w,
              wgm};
  if (LIST) {  // the octet region's entries
    n = kPktsPerTile * __builtin_amdgcn_readfirstlane(reg[0]);
    n_dev = nullptr;
  }
  if (!tile_ctx<MQ_SUITE_CHACHA20, OPEN, SINGLE>(tile_id, kt, n_rows, arena_len, desc, n, index, n_dev, hpm,
                                                 TilePrefetch{false, 0u, 0u}, c, row, tid)) {
    // past the batch (list capacities exceed the count): a whole workgroup leaves at once, a
    // wave of a live workgroup only joins its barriers and pool
    if (tb * W * kPktsPerTile >= (n_dev ? *n_dev : n)) {  // workgroup-uniform
      if (LIST) chacha_narrow_list<OPEN, SINGLE, kRaw>(wsm, tile_id, reg, kt, n_rows, arena, arena_len, desc, index, status,
                                                 pn_out, hpm);
      return;
    }
    if (LIST) {  // this wave's narrow tile, before the barriers (its records are reset after it)
      chacha_narrow_list<OPEN, SINGLE, kRaw>(wsm, tile_id, reg, kt, n_rows, arena, arena_len, desc, index, status, pn_out,
                                       hpm);
      wave_sync();
    }
    // the barriers of ChaChaPolicy::seal / open, and this wave's role in the MAC phase
    if (j == 0) pool.rec[0] = 0;
    __syncthreads();
    if (kWg && OPEN && wgm) {
      if (pool.role >= W - 2) cc_wg_mac<true, IMG, W, SINGLE>(smem, pool.role - (W - 2), tid);
      __syncthreads();
    }
    if constexpr (kHp2) cc_pool_seal<SINGLE, IMG, W, kR1, Sp>(pool, tid);
    else cc_pool_run<SINGLE, IMG, W, OPEN && kR1, Sp>(pool, tid);
    __syncthreads();
    if (kWg && !OPEN && wgm) {
      if (pool.role >= W - 2) cc_wg_mac<false, IMG, W>(smem, pool.role - (W - 2), tid);
      __syncthreads();
    }
    return;
  }
  MQ_STAMP(tile_id, 0);
  c.otk = (uint32_t*)(wsm + IMG - 32u * kPktsPerTile + 32u * (uint32_t)p);
  const uint64_t off = c.act ? c.d.offset : 0;
  Placement pl;
  pl.off = off;
  pl.len = c.act ? c.d.len : 0u;
  const uint64_t nch64 = c.act ? ((off & 15) + (uint64_t)c.d.len + 15) >> 4 : 0u;
  const uint32_t nch = (uint32_t)(nch64 < 0xFFFFu ? nch64 : 0xFFFFu);
  const uint32_t incl = oct_incl_scan(nch);
  const uint32_t total = lane_u32(incl, kWave - 1);
  // Packets of one even image size (lengths a multiple of 32 B at one alignment: 1600, 2048 B...)
  // start their images an even number of chunks apart, so the same keystream dword of every packet
  // sits on one LDS bank: 8-way conflicts in the XOR passes at 2048 B. A 16-B gap after each image
  // staggers them when the budget has room (r05; odd sizes such as config B's 75 chunks get none).
#ifndef MQ_CC_NOPAD  // diagnostic A/B build only: no gaps
  const uint32_t pad = (lane_u32(nch, 0) & 1u) == 0 && (total + kPktsPerTile) * 16u <= kBudget ? 1u : 0u;
#else
  const uint32_t pad = 0;
#endif
  if (total * 16u <= kBudget) {
    pl.slot = incl - nch + (uint32_t)p * pad;
    pool.on = true;
    // Span tile (mq_tile.h DmaStager): eight active packets of whole chunks (offset and length
    // multiples of 16) packed back to back in descriptor order, no gaps between the images — packet
    // p then lies 16 * slot_p bytes after packet 0, which is the one test that covers all seven
    // neighbours — so the tile is one linear run in the arena and the same run in LDS. Config B:
    // 1200 = 75 x 16, an odd chunk count, so no gaps. Staged and, when every packet is still
    // active at the end, stored as one copy; the layout is the per-packet one byte for byte.
    const bool in_span = c.act && (((uint32_t)off | pl.len) & 15u) == 0 && off == lane_u64(off, 0) + 16u * pl.slot;
    const bool span = span_ok && pad == 0 && !wave_any(!in_span);
    DmaStager stg{wsm, arena, arena_len, lane, j, pl, span ? total : 0u};
    Sp sp{};
    sp.base = wsm;
    MQ_STAMP(tile_id, 1);
    const uint32_t pkt = pl.slot * 16u + pl.head();
    if (OPEN) ChaChaPolicy::open<kLanesPerPkt, true, SINGLE, IMG, W, kR1, kWg>(sp, pkt, c, row, j, false, stg, pool);
    else ChaChaPolicy::seal<SINGLE, IMG, W, kR1, kWg, kHp2>(sp, pkt, c, row, j, stg, pool);
    MQ_STAMP(tile_id, 6);
    wave_sync();
    // a packet that failed to open is never stored: such a tile goes back packet by packet
    if (span && !wave_any(!c.act)) stage_out_span(wsm, arena, lane, total, lane_u64(pl.off, 0));
    else stage_out(wsm, arena, lane, c.act, pl);
    MQ_STAMP(tile_id, 7);
  } else {
    GlobalSpace sp{arena, arena_len};
    NoStager stg;
    if (OPEN) ChaChaPolicy::open<kLanesPerPkt, true, SINGLE, IMG, W, kR1, kWg>(sp, off, c, row, j, true, stg, pool);
    else ChaChaPolicy::seal<SINGLE, IMG, W, kR1, kWg, kHp2>(sp, off, c, row, j, stg, pool);
  }
  tile_status<OPEN>(c, j, status, pn_out);
}

#define MQ_CHACHA_KERNELS(NAME_SEAL, NAME_OPEN, SINGLE)                                                   \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_SEAL( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,               \
      const uint32_t* __restrict__ n_dev, uint8_t* __restrict__ status) {                                 \
    chacha_tile<false, SINGLE>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, index, n_dev, status, nullptr, \
                               nullptr);                                                                  \
  }                                                                                                       \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_OPEN( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,               \
      const uint32_t* __restrict__ n_dev, uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,    \
      const uint2* __restrict__ hpm) {                                                                    \
    chacha_tile<true, SINGLE>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, index, n_dev, status, pn_out, hpm); \
  }
MQ_CHACHA_KERNELS(mq_chacha_seal_kernel, mq_chacha_open_kernel, false)
MQ_CHACHA_KERNELS(mq_chacha_seal1_kernel, mq_chacha_open1_kernel, true)

// Flat batches of long packets (r05): the same octet tiles and keystream pool with
// larger LDS images, so eight packets over ~1216 B stay staged instead of running on HBM (direct:
// 358-409 GiB/s at 1232-2048 B, against 1034 at 1200): 13 KiB per wave (4-wave workgroups, 12
// waves per CU: eight images of up to 100 chunks, packets up to ~1570 B at any alignment) or 20 KiB
// (8 waves per CU: 156 chunks, ~2480 B). The waves-per-EU hint gives them the registers of that
// occupancy. (Measured and dropped: 16 KiB in 2-wave workgroups, 10 waves per CU — the pool shared
// by two waves lost more than the occupancy gained: 1800 B 833 vs 945 GiB/s, gpurun_out/r05p.)
constexpr uint32_t kLongImg = 13312, kLongerImg = 20480;
static_assert(kCcWaves * kLongImg * 3 <= kCuLdsBytes && kCcWaves * kLongerImg * 2 <= kCuLdsBytes, "long images per CU");
#define MQ_CHACHA_LONG_KERNELS(NAME_SEAL, NAME_OPEN, SINGLE, IMG, WPE, W)                                   \
  extern "C" __global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(WPE))) void NAME_SEAL( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, uint8_t* __restrict__ status) {                   \
    chacha_tile<false, SINGLE, false, IMG, W>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, nullptr, \
                                              nullptr, status, nullptr, nullptr);                         \
  }                                                                                                       \
  extern "C" __global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(WPE))) void NAME_OPEN( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out, \
      const uint2* __restrict__ hpm) {                                                                    \
    chacha_tile<true, SINGLE, false, IMG, W>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, nullptr, \
                                             nullptr, status, pn_out, hpm);                               \
  }
MQ_CHACHA_LONG_KERNELS(mq_chacha_seal_long_kernel, mq_chacha_open_long_kernel, false, kLongImg, 3, kCcWaves)
MQ_CHACHA_LONG_KERNELS(mq_chacha_seal_long1_kernel, mq_chacha_open_long1_kernel, true, kLongImg, 3, kCcWaves)
MQ_CHACHA_LONG_KERNELS(mq_chacha_seal_longer_kernel, mq_chacha_open_longer_kernel, false, kLongerImg, 2, kCcWaves)
MQ_CHACHA_LONG_KERNELS(mq_chacha_seal_longer1_kernel, mq_chacha_open_longer1_kernel, true, kLongerImg, 2, kCcWaves)

// One-shot grids over a partition list with narrow regions (reg, mq_partition.hip): tile
// tb * W + w is an octet tile of the G = 8 region or a narrow tile after it
#define MQ_CHACHA_LGRID_KERNELS(NAME_SEAL, NAME_OPEN, SINGLE)                                             \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_SEAL( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,               \
      const uint32_t* __restrict__ reg, uint8_t* __restrict__ status) {                                   \
    chacha_tile<false, SINGLE, true>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, index, nullptr, \
                                     status, nullptr, nullptr, reg);                                      \
  }                                                                                                       \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_OPEN( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,    \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,               \
      const uint32_t* __restrict__ reg, uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,      \
      const uint2* __restrict__ hpm) {                                                                    \
    chacha_tile<true, SINGLE, true>(blockIdx.x, threadIdx.x, kt, n_rows, arena, arena_len, desc, n, index, nullptr, \
                                    status, pn_out, hpm, reg);                                            \
  }
MQ_CHACHA_LGRID_KERNELS(mq_chacha_seal_lgrid_kernel, mq_chacha_open_lgrid_kernel, false)
MQ_CHACHA_LGRID_KERNELS(mq_chacha_seal_lgrid1_kernel, mq_chacha_open_lgrid1_kernel, true)

// Partition lists (index != null) run on PERSISTENT workgroups (r04): the list's length is a
// device count, so a grid covering the list capacity (1.6 x the batch in tiles of W) was mostly
// workgroups that read the count and left — config E's ChaCha list has ~15k blocks of work in a
// 52k-block grid, and an empty receive pass spent 350 us dispatching its 32k blocks
// (profiles/r04g_kernel_stats_recv.csv). Here cus x 4 workgroups (16 waves per CU, as the
// one-shot grid) take blocks of W tiles: block blockIdx.x first, then blocks claimed from the
// stream's schedule slot (head 0, one returning atomic per block; the claim for the block after
// next is issued when a block starts and read when it ends, so nobody waits on it), or, without a
// slot, by stride. (Flat batches keep the one-shot grid: a persistent grid measured 10 % slower on
// config B, r02 — identical waves stay in phase and their staging waits line up.)
// SINGLE: the list's packets share one key row (kt points at it)
template <bool OPEN, bool SINGLE>
__device__ __forceinline__ void chacha_list(const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena,
                                            uint64_t arena_len, const mq_pkt_desc* __restrict__ desc, uint32_t n,
                                            const uint32_t* __restrict__ index, const uint32_t* __restrict__ n_dev,
                                            uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,
                                            const uint2* __restrict__ hpm, uint32_t* __restrict__ sched,
                                            const uint32_t* __restrict__ reg) {
  constexpr uint32_t W = kCcWaves;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // the next block goes to every wave through word 7 of wave 0's first pool record, free between
  // tiles (the pool writes it only after the next tile's first barrier); the four 40-KiB
  // workgroups of a CU leave no LDS byte for a variable of its own
  uint32_t* next_slot = (uint32_t*)(smem + kDataBudget) + 7;
  uint32_t tb = blockIdx.x, pend = 0;
  if (threadIdx.x == 0 && sched) pend = __hip_atomic_fetch_add(sched, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)reg;  // the receive passes' partitions have no narrow regions (mq_partition.hip, skip_unkeyed)
  for (;;) {
    const uint32_t count = n_dev ? *n_dev : n;
    if (tb * W * kPktsPerTile >= count) break;  // workgroup-uniform
    uint32_t tid = threadIdx.x;
    // open: an opaque copy per tile (chacha_tile) — 10 spilled VGPRs to 2; seal spills more with it
    // (9 to 24), so it keeps the plain index there
    if (OPEN) asm volatile("" : "+v"(tid));
    // single-key seal: the key table pointer opaque per tile too, so its key words are loaded per
    // tile rather than held in SGPRs across the loop (spilled 29 VGPRs)
    const KeyRow* ktt = kt;
    if (SINGLE && !OPEN) asm volatile("" : "+s"(ktt));
    // no span tiles here: the receive passes' lists are sorted by length class, so their tiles are
    // rarely back to back, and the second copy loop cost these kernels 4-12 more spilled bytes per lane
    chacha_tile<OPEN, SINGLE, false, kLdsBytes, W, false>(tb, tid, ktt, n_rows, arena, arena_len, desc, n, index, n_dev,
                                                          status, pn_out, hpm);
    __syncthreads();  // every wave is done with the tile and its scratch
    if (threadIdx.x == 0) *next_slot = sched ? gridDim.x + pend : tb + gridDim.x;
    __syncthreads();
    tb = (uint32_t)__builtin_amdgcn_readfirstlane((int)*next_slot);  // uniform: keeps tile indexing scalar
    // the claim after this one: its result is used one block later (issued after the barrier, so
    // no barrier waits for it until the next tile's first one)
    if (threadIdx.x == 0 && sched) pend = __hip_atomic_fetch_add(sched, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the last claim is never used, but it must have returned before sched_done can zero head 0
  // (ADVICE r04): consuming its value makes thread 0 wait for it whatever the barrier lowers to
  if (threadIdx.x == 0) asm volatile("" ::"v"(pend));
  __syncthreads();
  sched_done(sched);
}
// The "1" list kernels: every packet of the list is on one key row (the key table has a single
// non-AES row, mq_host.cpp), kt points at it, so key material is wave-uniform, in SGPRs, as in the
// flat single-key kernels.
#define MQ_CHACHA_LIST_KERNELS(NAME_SEAL, NAME_OPEN, SINGLE)                                                \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_SEAL( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,     \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,                \
      const uint32_t* __restrict__ n_dev, uint8_t* __restrict__ status, uint32_t* __restrict__ sched,      \
      const uint32_t* __restrict__ reg) {                                                                  \
    chacha_list<false, SINGLE>(kt, n_rows, arena, arena_len, desc, n, index, n_dev, status, nullptr, nullptr, sched, reg); \
  }                                                                                                        \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_OPEN( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,     \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,                \
      const uint32_t* __restrict__ n_dev, uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,     \
      const uint2* __restrict__ hpm, uint32_t* __restrict__ sched, const uint32_t* __restrict__ reg) {   \
    chacha_list<true, SINGLE>(kt, n_rows, arena, arena_len, desc, n, index, n_dev, status, pn_out, hpm, sched, reg); \
  }
MQ_CHACHA_LIST_KERNELS(mq_chacha_seal_list_kernel, mq_chacha_open_list_kernel, false)
MQ_CHACHA_LIST_KERNELS(mq_chacha_seal_list1_kernel, mq_chacha_open_list1_kernel, true)

// Flat batches of short packets (r05): one wave per 64 consecutive descriptors. The wave sizes
// its 64 images and takes the narrowest lane group whose rounds fit the LDS image: G = 1 (one
// round of 64 packets), 2 (two of 32), 4 (four of 16) or 8 (eight of 8, the octet layout without
// the pool); a round over the budget runs on HBM (direct). No barriers: every wave is independent.
template <bool OPEN, bool SINGLE>
__device__ __forceinline__ void chacha_narrow_flat(const KeyRow* __restrict__ kt, uint32_t n_rows,
                                                   uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const mq_pkt_desc* __restrict__ desc, uint32_t n,
                                                   uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out,
                                                   const uint2* __restrict__ hpm) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t w = wave_id();
  uint8_t* wsm = smem + w * kLdsBytes;
  const uint32_t e0 = (blockIdx.x * kCcWaves + w) * (uint32_t)kWave;
  if (e0 >= n) return;
  const uint32_t lane = threadIdx.x & (kWave - 1), e = e0 + lane;
  uint32_t nch = 0;
  if (e < n) {  // offset and length only; validity is the tile's business (an over-count is harmless)
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(desc + e);
    const uint64_t x = ((dw[0] & 15u) + (uint64_t)dw[2] + 15u) >> 4;
    nch = (uint32_t)(x < 0xFFFFu ? x : 0xFFFFu);
  }
  const uint32_t incl = wave_incl_scan(nch);
  auto fits = [&](uint32_t Q) -> bool {  // every round of Q packets within the budget (uniform)
    for (uint32_t r = 0; r < (uint32_t)kWave / Q; ++r) {
      const uint32_t hi = lane_u32(incl, (int)(r * Q + Q - 1)), lo = r ? lane_u32(incl, (int)(r * Q - 1)) : 0u;
      if (hi - lo > kNarrowChunks) return false;
    }
    return true;
  };
#ifdef MQ_NARROW_ONLY  // register-pressure diagnostic: one lane group only
  (void)fits;
  for (uint32_t r = 0; r < MQ_NARROW_ONLY; ++r)
    narrow_tile<MQ_NARROW_ONLY, OPEN, SINGLE>(wsm, kt, n_rows, arena, arena_len, desc, e0 + 64 / MQ_NARROW_ONLY * r, n,
                                              nullptr, status, pn_out, hpm);
  return;
#endif
  if (fits(64)) {
    narrow_tile<1, OPEN, SINGLE>(wsm, kt, n_rows, arena, arena_len, desc, e0, n, nullptr, status, pn_out, hpm);
  } else if (fits(32)) {
    for (uint32_t r = 0; r < 2; ++r)
      narrow_tile<2, OPEN, SINGLE>(wsm, kt, n_rows, arena, arena_len, desc, e0 + 32 * r, n, nullptr, status, pn_out, hpm);
  } else if (fits(16)) {
    for (uint32_t r = 0; r < 4; ++r)
      narrow_tile<4, OPEN, SINGLE>(wsm, kt, n_rows, arena, arena_len, desc, e0 + 16 * r, n, nullptr, status, pn_out, hpm);
  } else {
    for (uint32_t r = 0; r < 8; ++r)
      narrow_tile<8, OPEN, SINGLE>(wsm, kt, n_rows, arena, arena_len, desc, e0 + 8 * r, n, nullptr, status, pn_out, hpm);
  }
}
#define MQ_CHACHA_NARROW_KERNELS(NAME_SEAL, NAME_OPEN, SINGLE)                                                \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_SEAL( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,        \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, uint8_t* __restrict__ status) {                       \
    chacha_narrow_flat<false, SINGLE>(kt, n_rows, arena, arena_len, desc, n, status, nullptr, nullptr);       \
  }                                                                                                           \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME_OPEN( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, uint8_t* __restrict__ arena, uint64_t arena_len,        \
      const mq_pkt_desc* __restrict__ desc, uint32_t n, uint8_t* __restrict__ status, uint64_t* __restrict__ pn_out, \
      const uint2* __restrict__ hpm) {                                                                        \
    chacha_narrow_flat<true, SINGLE>(kt, n_rows, arena, arena_len, desc, n, status, pn_out, hpm);             \
  }
MQ_CHACHA_NARROW_KERNELS(mq_chacha_seal_narrow_kernel, mq_chacha_open_narrow_kernel, false)
MQ_CHACHA_NARROW_KERNELS(mq_chacha_seal_narrow1_kernel, mq_chacha_open_narrow1_kernel, true)

// ---- fused send composite (mq_batch_protect with the ChaCha20 suite hint, r04) -----------------
// build + seal + header protection in one pass: the tile's eight packets are BUILT from their
// requests straight into the wave's LDS image (layout from mq_build.h, the frames at any alignment
// with unaligned 16-B loads, header / PN / PADDING / tag-room chunks byte-wise), sealed there by the
// same ChaChaPolicy::seal as a staged batch, and written to `out` once. The two-kernel composite
// (mq_build_kernel, then the seal kernel over its descriptors) moved every packet through HBM twice:
// written by the build, read back and rewritten by the seal — 4.9 GB per 2^20 x 1200 B against the
// 2.4 GB of frames in and packets out here. Tiles whose images exceed the LDS budget build in HBM
// (the build kernel's stores) and seal there (direct path). Statuses and lengths as the composite:
// the build's status when it fails (pkt_len = `needed` or 0), else the seal's.
#ifndef MQ_PROTECT_BATCH
#define MQ_PROTECT_BATCH 5
#endif
constexpr uint32_t kProtectBatch = MQ_PROTECT_BATCH;  // image chunks per lane whose loads fly together (5:
                                                      // no spills beside the seal state; 8 or 10 spill)

// Seal's pool with the header-protection blocks on lane pairs (cc_pool_seal), as in the flat seal
// kernels (chacha_tile): it changes neither kernel's registers (128 / 126 VGPRs) nor adds scratch
#ifdef MQ_CC_HP_INTERLEAVED
constexpr bool kProtectHp2 = false;
#else
constexpr bool kProtectHp2 = true;
#endif
template <bool SINGLE>
__device__ __forceinline__ void chacha_protect_tile(uint32_t tb, const KeyRow* __restrict__ kt, uint32_t n_rows,
                                                    const mq_conn_send* __restrict__ conns, uint32_t n_conns,
                                                    const uint8_t* __restrict__ frames, uint64_t frames_len,
                                                    uint8_t* __restrict__ out, uint64_t out_len,
                                                    const mq_send_req* __restrict__ req, uint32_t n,
                                                    uint32_t suite_hint, uint8_t* __restrict__ status,
                                                    uint32_t* __restrict__ pkt_len) {
  constexpr uint32_t W = kCcWaves;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t w = threadIdx.x >> 6;
  uint8_t* wsm = smem + w * kLdsBytes;
  const int lane = threadIdx.x & (kWave - 1), p = lane / kLanesPerPkt, j = lane % kLanesPerPkt;
  const uint32_t tile_id = tb * W + w;
  CcPool pool{false, smem, w * kLdsBytes, (uint32_t*)(wsm + kDataBudget + 32u * (uint32_t)p), kt, w, false};
  const uint32_t tile0 = tile_id * kPktsPerTile;
  if (tile0 >= n) {  // a wave past the batch in a live workgroup joins the barriers and the pool
    if (j == 0) pool.rec[0] = 0;
    __syncthreads();
    if constexpr (kProtectHp2) cc_pool_seal<SINGLE>(pool);
    else cc_pool_run<SINGLE>(pool);
    __syncthreads();
    return;
  }
  PktCtx c;
  c.tile = tile_id;
  c.i = tile0 + (uint32_t)p;
  c.valid = c.i < n;
  c.pre_hp = false;
  c.hm0 = c.hm1 = 0;
  const BuildLayout b = build_layout(c.i, c.valid, kt, n_rows, conns, n_conns, frames_len, out_len, req, suite_hint);
  c.d = b.d;
  c.pn = b.pn;
  if (!c.valid || b.st != MQ_OK) c.st = c.valid ? b.st : (int)MQ_ERR_INVALID_ARG;
  else c.st = validate<MQ_SUITE_CHACHA20, false, SINGLE>(c.d, kt, n_rows, out_len);
  c.act = c.valid && c.st == MQ_OK;
  const KeyRow* row = SINGLE ? kt : kt + (c.act ? c.d.key_id : 0u);
  c.otk = (uint32_t*)(wsm + kLdsBytes - 32u * kPktsPerTile + 32u * (uint32_t)p);
  Placement pl;
  pl.off = c.act ? c.d.offset : 0;
  pl.len = c.act ? c.d.len : 0u;
  const uint64_t nch64 = c.act ? ((pl.off & 15) + (uint64_t)c.d.len + 15) >> 4 : 0u;
  const uint32_t nch = (uint32_t)(nch64 < 0xFFFFu ? nch64 : 0xFFFFu);
  const uint32_t incl = oct_incl_scan(nch);
  const uint32_t total = lane_u32(incl, kWave - 1);
  const uint8_t* fr = frames + b.frames_offset;
  if (total * 16u <= kDataBudget) {
    pl.slot = incl - nch;
    pool.on = true;
    // the image: chunk k holds packet bytes [16k - head, 16k - head + 16); lane j builds k = j,
    // j + 8, ... (kProtectBatch chunks' loads issued before any of their LDS stores)
    uint8_t* img = wsm + 16u * pl.slot;
    const int head = (int)pl.head();
    for (uint32_t k0 = (uint32_t)j; k0 < nch; k0 += kLanesPerPkt * kProtectBatch) {
      uint4 v[kProtectBatch];
#pragma unroll
      for (uint32_t t = 0; t < kProtectBatch; ++t) {
        const uint32_t k = k0 + kLanesPerPkt * t;
        const int x0 = 16 * (int)k - head;
        const bool whole = k < nch && x0 >= (int)b.hp && (uint32_t)x0 + 16u <= b.hp + b.m;
#if MQ_PROF_SKIP & 512  // phase-cost diagnostic: no frames loads
        v[t] = make_uint4(x0, 0, 0, 0);
#else
        v[t] = whole ? ld16(fr + ((uint32_t)x0 - b.hp)) : make_uint4(0, 0, 0, 0);
#endif
      }
#pragma unroll
      for (uint32_t t = 0; t < kProtectBatch; ++t) {
        const uint32_t k = k0 + kLanesPerPkt * t;
        const int x0 = 16 * (int)k - head;
        const bool whole = x0 >= (int)b.hp && (uint32_t)x0 + 16u <= b.hp + b.m;
        const bool zero = x0 >= (int)(b.hp + b.m);  // PADDING / tag room (and bytes past the packet)
        if (k < nch && (whole || zero)) *(uint4*)(img + 16u * k) = v[t];
      }
    }
    // edge chunks, byte-wise, outside the unrolled batch: those holding header / PN bytes, and the
    // one where the frames end mid-chunk
    const uint32_t kh = (uint32_t)(head + (int)b.hp + 15) >> 4, fe = (uint32_t)head + b.hp + b.m;
#if !(MQ_PROF_SKIP & 256)  // phase-cost diagnostic: no edge chunks
    // their frames bytes first (one guarded 16-B load each, zeros elsewhere), then the header and PN
    // bytes on top, eight per lane from the connection row's words: r04's first version built
    // each edge chunk byte by byte on one lane, a dependent load per byte (0.12 of its 1.40 ms,
    // profiles/r04n_protect_phases.txt)
    for (uint32_t k = (uint32_t)j; k < kh && k < nch; k += kLanesPerPkt)
      *(uint4*)(img + 16u * k) = edge_frames(b, fr, 16 * (int)k - head, b.frames_offset, frames_len);
    if ((fe & 15u) && (fe >> 4) >= kh && (fe >> 4) < nch && ((fe >> 4) & (kLanesPerPkt - 1)) == (uint32_t)j)
      *(uint4*)(img + 16u * (fe >> 4)) = edge_frames(b, fr, 16 * (int)(fe >> 4) - head, b.frames_offset, frames_len);
    if (c.act && 8u * (uint32_t)j < b.hp) {
      HeaderLane hl;
      hl.load(b.cp, b.level, j);
      uint8_t* hd = img + head;
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t x = 8u * (uint32_t)j + u;
        if (x < b.hp)
          hd[x] = x < b.hdr ? hl.byte(b.level, b.pn_len, b.payload_length, x, u)
                            : (uint8_t)(b.pn >> (8 * (b.pn_len - 1 - (x - b.hdr))));
      }
    }
#endif
    LdsSpace sp{wsm};
    NoStager stg;  // complete(): the wave's image stores are done before any lane reads the image
    ChaChaPolicy::seal<SINGLE, kLdsBytes, kCcWaves, false, false, kProtectHp2>(sp, pl.slot * 16u + pl.head(), c, row, j, stg, pool);
    wave_sync();
    stage_out(wsm, out, lane, c.act, pl);
  } else {
    if (c.act) build_store<kProtectBatch>(b, j, frames, out);
    wave_sync();  // the packets are in HBM before the seal reads them
    GlobalSpace sp{out, out_len};
    NoStager stg;
    ChaChaPolicy::seal<SINGLE, kLdsBytes, kCcWaves, false, false, kProtectHp2>(sp, c.act ? c.d.offset : 0, c, row, j, stg, pool);
  }
  if (c.valid && j == 0) {
    status[c.i] = (uint8_t)c.st;
    pkt_len[c.i] = (b.st != MQ_OK || c.st == MQ_OK) ? b.len_out : 0u;
  }
}

#define MQ_CHACHA_PROTECT_KERNEL(NAME, SINGLE)                                                             \
  extern "C" __global__ __launch_bounds__(64 * kCcWaves) __attribute__((amdgpu_waves_per_eu(4))) void NAME( \
      const KeyRow* __restrict__ kt, uint32_t n_rows, const mq_conn_send* __restrict__ conns, uint32_t n_conns, \
      const uint8_t* __restrict__ frames, uint64_t frames_len, uint8_t* __restrict__ out, uint64_t out_len,   \
      const mq_send_req* __restrict__ req, uint32_t n, uint32_t suite_hint, uint8_t* __restrict__ status,     \
      uint32_t* __restrict__ pkt_len) {                                                                       \
    chacha_protect_tile<SINGLE>(blockIdx.x, kt, n_rows, conns, n_conns, frames, frames_len, out, out_len, req, n, \
                                suite_hint, status, pkt_len);                                                 \
  }
MQ_CHACHA_PROTECT_KERNEL(mq_chacha_protect_kernel, false)
MQ_CHACHA_PROTECT_KERNEL(mq_chacha_protect1_kernel, true)

extern "C" __global__ __launch_bounds__(256) void mq_chacha_hp_kernel(
    const KeyRow* __restrict__ kt, uint32_t n_rows, const uint32_t* __restrict__ key_ids,
    const uint8_t* __restrict__ samples, uint8_t* __restrict__ masks, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t kid = key_ids[i];
  if (kid >= n_rows || kt[kid].suite != MQ_SUITE_CHACHA20) {
    // rows of neither suite (bad key id, empty row): all-zero mask (include/mq_aead.h); AES
    // rows are the AES kernel's
    if (kid >= n_rows || kt[kid].suite != MQ_SUITE_AES128GCM)
      for (int b = 0; b < 5; ++b) masks[5 * (size_t)i + b] = 0;
    return;
  }
  GlobalSpace sp{const_cast<uint8_t*>(samples), (uint64_t)n * 16};
  uint32_t m0, m1;
  ChaChaPolicy::hp_mask(sp, (uint64_t)i * 16, kt + kid, m0, m1);
  for (int b = 0; b < 4; ++b) masks[5 * (size_t)i + b] = (uint8_t)(m0 >> (8 * b));
  masks[5 * (size_t)i + 4] = (uint8_t)m1;
}

// Open pre-pass: ChaChaHeaderProtection::mask of every packet's sample, one packet per lane, so
// the tile kernel spends no keystream slot of its octet on it. DECODE (the batch open path):
// store the unmasked first byte and truncated PN (prepass_decode) instead of the raw mask
// (which mq_recv.hip's planner consumes).
template <bool DECODE>
__global__ __launch_bounds__(256) void mq_chacha_open_hp_kernel(
    const KeyRow* __restrict__ kt, uint32_t n_rows, const uint8_t* __restrict__ arena, uint64_t arena_len,
    const mq_pkt_desc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ index,
    const uint32_t* __restrict__ n_dev, uint2* __restrict__ hpm) {
  uint32_t i;
  const KeyRow* row;
  uint64_t at;
  mq_pkt_desc d;
  if (!prepass_pick(blockIdx.x * blockDim.x + threadIdx.x, MQ_SUITE_CHACHA20, kt, n_rows, arena_len, desc, n,
                    index, n_dev, i, row, at, d))
    return;
  GlobalSpace sp{const_cast<uint8_t*>(arena), arena_len};
  uint32_t m0, m1;
  if (DECODE) {  // PN bytes and sample (contiguous) and the first byte in one round of loads
    uint32_t w[5];
    uint8_t b0;
    prepass_header(arena, d, b0, w);
    const uint32_t smp[4] = {w[1], w[2], w[3], w[4]};
    ChaChaPolicy::hp_mask_words(smp, row, m0, m1);
    hpm[i] = prepass_decode_words(b0, w[0], d, m0, m1);
  } else {
    ChaChaPolicy::hp_mask(sp, at, row, m0, m1);
    hpm[i] = make_uint2(m0, m1);
  }
}

// ---- host-side launchers (called from mq_host.cpp) -------------------------------------------
// index != null (a partition list, length on the device): the persistent list kernels, cus x 4
// workgroups, sched = the stream's schedule slot (null: static stride)
// Flat batches (no partition list): the kernel family from the batch's bytes per packet `bpp` —
// the caller's length hint (MQ_BATCH_LEN_HINT), else arena_len / n. 0: narrow tiles (a batch
// averaging at most 640 B per packet: short packets, G = 8 / 4 / 2 / 1 lanes chosen per wave;
// configs B and E never), 1: octet tiles over 10-KiB images (config B: 1200), 2: 13-KiB images (eight
// images over 1216 B), 3: 20-KiB images (over 1584 B). Tiles whose images overflow the kernel's LDS
// image take the direct HBM path: right, only slower.
int mq_chacha_flat_kind(uint64_t bpp) {
  constexpr uint64_t kNarrowAvg = 640, kLongAvg0 = 1216, kLongAvg1 = 1584;
  return bpp <= kNarrowAvg ? 0 : bpp <= kLongAvg0 ? 1 : bpp <= kLongAvg1 ? 2 : 3;
}

// The seal / open kernels of each family; one: its single-key kernels
static auto cc_seal_of(bool one) { return one ? mq_chacha_seal1_kernel : mq_chacha_seal_kernel; }
static auto cc_open_of(bool one) { return one ? mq_chacha_open1_kernel : mq_chacha_open_kernel; }
static auto cc_list_seal_of(bool one) { return one ? mq_chacha_seal_list1_kernel : mq_chacha_seal_list_kernel; }
static auto cc_list_open_of(bool one) { return one ? mq_chacha_open_list1_kernel : mq_chacha_open_list_kernel; }
static auto cc_lgrid_seal_of(bool one) { return one ? mq_chacha_seal_lgrid1_kernel : mq_chacha_seal_lgrid_kernel; }
static auto cc_lgrid_open_of(bool one) { return one ? mq_chacha_open_lgrid1_kernel : mq_chacha_open_lgrid_kernel; }
// flat batches off the 10-KiB octet tiles: img 0 the narrow kernels, 1 / 2 the 13- / 20-KiB images
static auto cc_flat_seal_of(int img, bool one) {
  return img == 0   ? (one ? mq_chacha_seal_narrow1_kernel : mq_chacha_seal_narrow_kernel)
         : img == 2 ? (one ? mq_chacha_seal_longer1_kernel : mq_chacha_seal_longer_kernel)
                    : (one ? mq_chacha_seal_long1_kernel : mq_chacha_seal_long_kernel);
}
static auto cc_flat_open_of(int img, bool one) {
  return img == 0   ? (one ? mq_chacha_open_narrow1_kernel : mq_chacha_open_narrow_kernel)
         : img == 2 ? (one ? mq_chacha_open_longer1_kernel : mq_chacha_open_longer_kernel)
                    : (one ? mq_chacha_open_long1_kernel : mq_chacha_open_long_kernel);
}

hipError_t mq_launch_chacha(const mq::BatchArgs& b, const mq::TileLaunch& l) {
  const uint32_t n = l.n, n_rows = b.n_rows;
  const uint32_t tiles = (n + kPktsPerTile - 1) / kPktsPerTile;
  if (tiles == 0) return hipSuccess;
  if (b.open && b.hpm && l.own_hp) {  // !own_hp: mq_launch_mixed_hp covers both suites' lists
    hipLaunchKernelGGL(mq_chacha_open_hp_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, l.s, b.kt, n_rows, b.arena,
                       b.arena_len, b.desc, n, l.index, l.n_dev, b.hpm);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const uint32_t blocks = (tiles + kCcWaves - 1) / kCcWaves;
  // Lists run on the persistent grid when asked for (the receive composite's passes: an empty
  // list then costs 1024 workgroups, not a grid over the list capacity), else on the one-shot grid,
  // which measured 1.1 % faster on config E (r04q: 557.9 vs 551.6 GiB/s, three alternating runs).
  // MQ_CC_LIST=0 / 1 (diagnostic, mq_opts.h: tests run both grids on one batch) forces either.
  const bool persistent = b.sw.cc_list >= 0 ? b.sw.cc_list != 0 : l.persistent;
  // single_row >= 0: every packet of the list is on that row (the single-key kernels)
  const bool one = l.index && l.single_row >= 0 && (uint64_t)l.single_row < n_rows;
  const KeyRow* kl = one ? b.kt + l.single_row : b.kt;
  // MQ_CC_SPAN=0 (diagnostic, mq_opts.h: tests run both copies on one batch): no span tiles in the
  // octet-tile kernels (chacha_tile reads the bit off n_rows)
  // MQ_CC_WGMAC=0 (likewise): the per-wave MAC in the kernels with the workgroup MAC phase
  const uint32_t nr = n_rows | (b.sw.cc_span == 0 ? kCcNoSpan : 0u) | (b.sw.cc_wgmac == 0 ? kCcNoWgMac : 0u);
  const dim3 block(kWave * kCcWaves);
  constexpr uint32_t kLds = kLdsBytes * kCcWaves;
  // One kernel of a family's pair: both take the key rows, the row word, the arena, the descriptors,
  // n, the family's own arguments (mid) and the status; the open kernel then pn_out and hpm.
  auto launch = [&](auto seal, auto open, uint32_t grid, uint32_t lds, const KeyRow* rows, uint32_t row_word,
                    auto... mid) {
    if (b.open)
      hipLaunchKernelGGL(open, dim3(grid), block, lds, l.s, rows, row_word, b.arena, b.arena_len, b.desc, n, mid...,
                         b.status, b.pn_out, b.hpm);
    else  // seal: header protection runs inside the tile kernel (the pool's HP blocks, cc_pool_run)
      hipLaunchKernelGGL(seal, dim3(grid), block, lds, l.s, rows, row_word, b.arena, b.arena_len, b.desc, n, mid...,
                         b.status);
    return hipGetLastError();
  };
  if (l.index && persistent) {  // its kernels end on the schedule slot and the regions instead
    const uint32_t per = (uint32_t)(b.cus > 0 ? b.cus : 256) * 4u, grid = blocks < per ? blocks : per;
    if (b.open)
      hipLaunchKernelGGL(cc_list_open_of(one), dim3(grid), block, kLds, l.s, kl, nr, b.arena, b.arena_len, b.desc, n,
                         l.index, l.n_dev, b.status, b.pn_out, b.hpm, l.sched, l.reg);
    else
      hipLaunchKernelGGL(cc_list_seal_of(one), dim3(grid), block, kLds, l.s, kl, nr, b.arena, b.arena_len, b.desc, n,
                         l.index, l.n_dev, b.status, l.sched, l.reg);
    return hipGetLastError();
  }
  // one-shot grid over the list capacity (every region's tiles fit: a tile holds >= 8 entries)
  if (l.index) return launch(cc_lgrid_seal_of(one), cc_lgrid_open_of(one), blocks, kLds, kl, nr, l.index, l.reg);
  // Flat batches: the kernel family from the bytes per packet (mq_chacha_flat_kind). MQ_CC_NARROW=0 / 1
  // and MQ_CC_LONG=0 / 1 / 2 (diagnostic, mq_opts.h: tests run several kernels on one batch) force
  // the wide / narrow kernels and the 10-, 13- or 20-KiB images.
  const int kind = mq_chacha_flat_kind(b.bpp);
  const bool o1 = n_rows == 1;
  if (b.sw.cc_narrow >= 0 ? b.sw.cc_narrow == 1 : kind == 0) {
    const uint32_t nb = (uint32_t)(((uint64_t)n + kWave * kCcWaves - 1) / (kWave * kCcWaves));
    return launch(cc_flat_seal_of(0, o1), cc_flat_open_of(0, o1), nb, kLds, b.kt, n_rows);
  }
  int img = kind >= 2 ? kind - 1 : 0;  // 0: 10 KiB, 1: 13 KiB, 2: 20 KiB
  if (b.sw.cc_long >= 0) img = b.sw.cc_long >= 2 ? 2 : (int)b.sw.cc_long;
  if (img)
    return launch(cc_flat_seal_of(img, o1), cc_flat_open_of(img, o1), blocks, (img == 2 ? kLongerImg : kLongImg) * kCcWaves,
                  b.kt, nr);
  return launch(cc_seal_of(o1), cc_open_of(o1), blocks, kLds, b.kt, nr, l.index, l.n_dev);
}

hipError_t mq_launch_chacha_protect(const KeyRow* kt, uint32_t n_rows, const mq_conn_send* conns, uint32_t n_conns,
                                    const uint8_t* frames, uint64_t frames_len, uint8_t* out, uint64_t out_len,
                                    const mq_send_req* req, uint32_t n, uint32_t suite_hint, uint8_t* status,
                                    uint32_t* pkt_len, hipStream_t s) {
  const uint32_t tiles = (n + kPktsPerTile - 1) / kPktsPerTile;
  if (tiles == 0) return hipSuccess;
  const uint32_t blocks = (tiles + kCcWaves - 1) / kCcWaves;
  hipLaunchKernelGGL(n_rows == 1 ? mq_chacha_protect1_kernel : mq_chacha_protect_kernel, dim3(blocks),
                     dim3(kWave * kCcWaves), kLdsBytes * kCcWaves, s, kt, n_rows, conns, n_conns, frames, frames_len,
                     out, out_len, req, n, suite_hint, status, pkt_len);
  return hipGetLastError();
}

// header-protection masks of the ChaCha20 rows of `desc` only (mq_recv.hip plans with them)
hipError_t mq_launch_chacha_prepass(const KeyRow* kt, uint32_t n_rows, const uint8_t* arena, uint64_t arena_len,
                                    const mq_pkt_desc* desc, uint32_t n, uint2* hpm, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mq_chacha_open_hp_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, kt, n_rows, arena, arena_len,
                     desc, n, (const uint32_t*)nullptr, (const uint32_t*)nullptr, hpm);
  return hipGetLastError();
}

hipError_t mq_launch_chacha_hp(const KeyRow* kt, uint32_t n_rows, const uint32_t* key_ids,
                               const uint8_t* samples, uint8_t* masks, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mq_chacha_hp_kernel, dim3((n + 255) / 256), dim3(256), 0, s, kt, n_rows, key_ids,
                     samples, masks, n);
  return hipGetLastError();
}

#ifdef MQ_STAMPS
void mq_stamps_set_chacha(uint64_t* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(mq_stamp_buf), &p, sizeof p); }
#endif
