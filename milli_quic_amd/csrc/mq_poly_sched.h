// mq_poly_sched.h — the per-lane schedule of the interleaved Poly1305 (mq_chacha.hip poly_tag), as
// plain integer arithmetic that compiles for the device and for the host (tests/csrc/
// test_poly_sched.cpp checks it exhaustively without a GPU). Included by mq_device.h.
//
// The MAC input of a packet (RFC 8439 §2.8) is nb = A + T + 1 blocks of 16 B: A of AAD (the last
// one zero-padded), T of ciphertext (the last one zero-padded), one of lengths. A group of G lanes
// runs Kmax steps (the wave's maximum of K = ceil(nb / G)); group lane j absorbs MAC block
// i = G k + j - z in step k, where z = G Kmax - nb blocks of zeros (without the 2^128 bit) are
// prepended, so block nb - 1 (the lengths) always falls on lane G - 1 in step Kmax - 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MQ_HD __host__ __device__ __forceinline__
#else
#define MQ_HD inline
#endif

namespace mq {

// Per packet (group-uniform).
struct PolyGeom {
  uint32_t A, T, nb, K;  // AAD blocks, ciphertext blocks, MAC blocks, steps the packet needs alone
};
template <int G>
MQ_HD PolyGeom poly_geom(uint32_t aad_len, uint32_t ct_len) {
  PolyGeom g;
  g.A = (aad_len + 15) >> 4;
  g.T = (ct_len + 15) >> 4;
  g.nb = g.A + g.T + 1;
  g.K = (g.nb + G - 1) / G;
  return g;
}

// Per packet once the wave's Kmax is known. A step k is lean when every lane of the group absorbs a
// whole ciphertext block in it: G k - z >= A (lane 0) and G k + G - 1 - z < ct_full_end (lane
// G - 1), that is k in [k_lo, k_hi). The block a lean step loads for step k + 1 need not be whole:
// the general absorb that follows masks it by `rem` (or replaces it: the lengths block). An inactive
// packet bounds nothing (k_lo = 0, k_hi = all ones); the wave runs the stretch
// [max k_lo, min(min k_hi, Kmax - 1)).
struct PolyLean {
  int z;            // prepended zero blocks
  int ct_full_end;  // first MAC block index behind the whole ciphertext blocks
  uint32_t k_lo, k_hi;
};
// EDGE = false: the stretch ends one step earlier, so that the block it loads last is whole too
// (the narrow lane groups, which keep the former edge steps: mq_chacha.hip poly_tag).
template <int G, bool EDGE = true>
MQ_HD PolyLean poly_lean(uint32_t A, uint32_t nb, uint32_t ct_len, uint32_t Kmax, bool act) {
  PolyLean s;
  s.z = (int)(G * Kmax) - (int)nb;
  s.ct_full_end = (int)A + (int)(ct_len >> 4);
  const int zA = (int)A + s.z;
  s.k_lo = act ? (uint32_t)((zA + G - 1) / G) : 0u;
  const int hi = s.ct_full_end + s.z - (EDGE ? G : 2 * G) + 1;  // lean iff G k + G - 1 - z < ct_full_end
  s.k_hi = !act ? 0xFFFFFFFFu : (hi <= 0 ? 0u : (uint32_t)((hi + G - 1) / G));
  return s;
}

// MAC block i (i < 0: a prepended zero block): where its bytes start and how many are real.
struct PolyBlk {
  bool aad;      // off counts from the packet's first byte, else from the payload (ciphertext)
  uint32_t off;  // meaningless for the blocks that read nothing (pre, lens: the caller reads at 0)
  int rem;       // real bytes from off on (>= 16: a whole block; <= 0 for the lengths block)
  bool pre, lens;
};
MQ_HD PolyBlk poly_blk(uint32_t A, uint32_t T, uint32_t aad_len, uint32_t ct_len, int i) {
  PolyBlk b;
  b.aad = i < (int)A;
  b.pre = i < 0;  // prepended zero block
  b.lens = i == (int)(A + T);
  b.off = b.aad ? 16 * (uint32_t)(i > 0 ? i : 0) : 16 * (uint32_t)(i - (int)A);
  b.rem = b.aad ? (int)aad_len - 16 * i : (int)ct_len - 16 * (i - (int)A);
  return b;
}

}  // namespace mq
