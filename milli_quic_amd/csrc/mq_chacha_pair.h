// mq_chacha_pair.h — the ChaCha20 block function (RFC 8439 §2.3) on a pair of lanes, for a block of
// which only the first keystream words are wanted: a header-protection mask (RFC 9001 §5.4.4) is
// keystream bytes 0..4 of its block. Plain word arithmetic over a word type W and an exchange X
// between the two lanes, so it compiles for the device (W = uint32_t, X = a DPP quad_perm move
// between lanes l and l ^ 1: mq_device.h PairSwapDpp) and for the host (W = both lanes' words side
// by side, X = a swap of the two: tests/csrc/test_chacha_pair.cpp replays it against the plain
// block function without a GPU). Included by mq_device.h.
//
// Half h of the pair holds columns 2h and 2h + 1 of the 4 x 4 state, eight words: a[i] = x[2h + i],
// b[i] = x[4 + 2h + i], c[i] = x[8 + 2h + i], d[i] = x[12 + 2h + i]. A column round is two
// quarter-rounds per lane and no exchange. A diagonal round pairs a of column j with b of column
// j + 1, c of j + 2 and d of j + 3: row a stays, of row b one word comes from the other lane (the
// other moves within the lane, a renaming), of row d likewise, and row c comes over whole — four
// exchanges into the round and four back, none of them after the last round, whose rows b, c and d
// nobody reads. Words 0 and 1 are row a of half 0.
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

template <class W>
MQ_HD void cc_pair_qr(W& a, W& b, W& c, W& d) {
  a = a + b; d = d ^ a; d = (d << 16) | (d >> 16);
  c = c + d; b = b ^ c; b = (b << 12) | (b >> 20);
  a = a + b; d = d ^ a; d = (d << 8) | (d >> 24);
  c = c + d; b = b ^ c; b = (b << 7) | (b >> 25);
}

// the "expand 32-byte k" word 2h + i of half h
MQ_HD uint32_t cc_pair_const(uint32_t h, int i) {
  return i == 0 ? (h ? 0x79622d32u : 0x61707865u) : (h ? 0x6b206574u : 0x3320646eu);
}

// The twenty rounds and the final addition of row a. On half h: a = the constants 2h, 2h + 1,
// b = key words 2h, 2h + 1, c = key words 4 + 2h, 5 + 2h, d = input words 12 + 2h, 13 + 2h (half 0:
// block counter and nonce word 0, half 1: nonce words 1 and 2). Returns keystream words 2h and
// 2h + 1 in ks0 and ks1; the other twelve final additions are not made.
template <class W, class X>
MQ_HD void chacha20_block_pair(const W (&a_in)[2], const W (&b_in)[2], const W (&c_in)[2], const W (&d_in)[2],
                               const X& xchg, W& ks0, W& ks1) {
  W a[2] = {a_in[0], a_in[1]}, b[2] = {b_in[0], b_in[1]}, c[2] = {c_in[0], c_in[1]}, d[2] = {d_in[0], d_in[1]};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 2
#endif
  for (int i = 0; i < 10; ++i) {
    cc_pair_qr(a[0], b[0], c[0], d[0]);
    cc_pair_qr(a[1], b[1], c[1], d[1]);
    // diagonals 2h (b of column 2h + 1: own, c of 2h + 2 and d of 2h + 3: the other lane's) and
    // 2h + 1 (b of 2h + 2 and c of 2h + 3: the other lane's, d of 2h + 4 = 2h: own)
    W b0 = b[1], b1 = xchg(b[0]), c0 = xchg(c[0]), c1 = xchg(c[1]), d0 = xchg(d[1]), d1 = d[0];
    cc_pair_qr(a[0], b0, c0, d0);
    cc_pair_qr(a[1], b1, c1, d1);
    if (i == 9) break;  // row a is final
    b[1] = b0; b[0] = xchg(b1);
    c[0] = xchg(c0); c[1] = xchg(c1);
    d[0] = d1; d[1] = xchg(d0);
  }
  ks0 = a[0] + a_in[0];
  ks1 = a[1] + a_in[1];
}

}  // namespace mq
