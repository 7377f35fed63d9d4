"""Crafted ChaCha20-Poly1305 packets whose Poly1305 accumulator ends on a chosen residue mod
p = 2^130 - 5, and an RFC 8439 reference in pure Python (numpy ChaCha20 blocks, Poly1305 over big
integers) that calls neither the oracle nor the library.

Random packets leave the accumulator in [p, 2^130) with probability 5 / 2^130, so random tests never
run the final conditional subtraction of p, the second fold of the carry out of limb 4, or a carry that
ripples through the whole addition of s. A sender can choose such packets cheaply: in the AEAD MAC
input every 16-byte block m_i carries the 2^128 bit, and the final accumulator is affine in any one
whole ciphertext block,
    h = m_k r^(nb - k) + base (mod p),   so   m_k = (T - base) r^-(nb - k) mod p
reaches the target T; the draw is usable when 2^128 <= m_k < 2^129 (about one in four), otherwise
another free block (or AAD byte, or the packet number) is redrawn.

TARGETS, and the line of p26_finish (milli_quic_amd/csrc/mq_poly26.h) each one is aimed at. A lane
schedule hands p26_finish the sum N = T + k p of its lanes' partials (k >= 1 for G >= 2, and for one
lane whenever the last product is not tiny), so what arrives is c 2^130 + L with L = T - 5 c + (p + 5
when that is negative):
  0, 1, 4   L + 5 c lands in [p, 2^130): `use_g` true, the subtraction of p (g0 .. g4 selected).
  5         L + 5 c is exactly 2^130: the second fold's carry ripples from limb 0 through every
            limb (the carries behind `h.l[0] += c * 5`), then use_g.
  6         2^130 + 1: the same ripple with a limb 0 that stays non-zero.
  p-1, p-6  the largest values below p: g4's borrow (`g4 >> 31`) must keep use_g false with g0 .. g3
            at their largest; p-6 leaves L + 5 c at p - 1 for c = 1.
  p-5       p - 5 + 5 c >= p for every c >= 1: use_g true where p-6 is false, one apart.
  2^128-1   limbs 0 .. 3 all ones, limb 4 = 2^24 - 1: the word packing w0 .. w3 with every bit set
            and the widest carry chain of `+ s`.
  2^128     L = 2^128 - 5 c has limbs 1 .. 3 all ones: adding 5 c back ripples a carry out of limb 0
            up to limb 4 with use_g false, so the words are packed from what the second pass left.
  2^129     the same ripple one bit higher (limb 4 = 2^25: bit 129 is cut by the tag's mod 2^128).
  TAG_ZERO  T = -s mod 2^128: h + s = 2^128 exactly, the `(t >> 32)` carries of the tag addition
            ripple through all four words; the tag is sixteen zero bytes.
  TAG_ONES  T = 2^128 - 1 - s: the tag is sixteen 0xFF bytes, no carry may appear anywhere.
"""
import numpy as np

P = (1 << 130) - 5
M128 = (1 << 128) - 1
TAG_ZERO, TAG_ONES = "TAG_ZERO", "TAG_ONES"
TARGETS = {
    "0": 0, "1": 1, "4": 4, "5": 5, "6": 6, "p-1": P - 1, "p-5": P - 5, "p-6": P - 6,
    "2^128-1": (1 << 128) - 1, "2^128": 1 << 128, "2^129": 1 << 129, TAG_ZERO: TAG_ZERO, TAG_ONES: TAG_ONES,
}
FILLS = ("random", "zeros", "ones")
MAX_DRAWS = 64


# ---- RFC 8439 in pure Python ---------------------------------------------------------------------
def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def chacha20_blocks(key, counter, nonce, n):
    """n consecutive ChaCha20 blocks (RFC 8439 §2.3) from block counter `counter`: 64 n bytes."""
    key, nonce = bytes(key), bytes(nonce)
    assert len(key) == 32 and len(nonce) == 12
    st = np.empty((16, n), dtype=np.uint32)
    st[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    st[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    st[12] = (counter + np.arange(n, dtype=np.uint64)).astype(np.uint32)
    st[13:16] = np.frombuffer(nonce, dtype="<u4")[:, None]
    x = st.copy()

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    x += st
    return np.ascontiguousarray(x.T).astype("<u4").tobytes()


def one_time_key(key, nonce):
    """(r clamped, s) of RFC 8439 §2.6: the first 32 bytes of block 0."""
    otk = chacha20_blocks(key, 0, nonce, 1)[:32]
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    return r, int.from_bytes(otk[16:], "little"), otk


def keystream(key, nonce, n):
    """The n payload keystream bytes (block counter 1 on)."""
    return chacha20_blocks(key, 1, nonce, (n + 63) // 64 or 1)[:n]


def mac_input(aad, ct):
    """RFC 8439 §2.8: AAD || pad16 || ciphertext || pad16 || LE64(len AAD) || LE64(len ciphertext)."""
    aad, ct = bytes(aad), bytes(ct)
    return (aad + bytes(-len(aad) % 16) + ct + bytes(-len(ct) % 16)
            + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little"))


def poly_blocks(msg):
    """The blocks of a MAC input as integers, each with its 2^128 bit (every block is whole)."""
    assert len(msg) % 16 == 0
    return [int.from_bytes(msg[o:o + 16], "little") | (1 << 128) for o in range(0, len(msg), 16)]


def accumulator(r, blocks):
    """Horner over the blocks: the Poly1305 accumulator mod p before s is added."""
    h = 0
    for m in blocks:
        h = (h + m) * r % P
    return h


def tag_of(h, s):
    return ((h + s) & M128).to_bytes(16, "little")


def aead_tag(key, nonce, aad, ct):
    r, s, _ = one_time_key(key, nonce)
    return tag_of(accumulator(r, poly_blocks(mac_input(aad, ct))), s)


def aead_seal(key, nonce, aad, pt):
    """ciphertext || tag (RFC 8439 §2.8)."""
    ct = bytes(a ^ b for a, b in zip(pt, keystream(key, nonce, len(pt))))
    return ct + aead_tag(key, nonce, aad, ct)


def plaintext_for(ct, ks):
    """The plaintext that seals to ciphertext ct under keystream ks."""
    assert len(ks) >= len(ct)
    return (np.frombuffer(bytes(ct), dtype=np.uint8) ^ np.frombuffer(bytes(ks[:len(ct)]), dtype=np.uint8)).tobytes()


def shifted_tag(tag, d):
    """tag + d mod 2^128: d = +-5 is what a spurious or a missing subtraction of p yields (p = -5
    mod 2^128)."""
    return ((int.from_bytes(tag, "little") + d) & M128).to_bytes(16, "little")


# ---- crafting --------------------------------------------------------------------------------------
class NothingFree(Exception):
    """The draw was not usable and the packet has nothing left to redraw (one ciphertext block, no
    free AAD byte): the caller redraws the packet number."""


def target_value(target, s):
    t = TARGETS.get(target, target)
    if t == TAG_ZERO:
        return -s & M128
    if t == TAG_ONES:
        return (M128 - s) & M128
    assert isinstance(t, int) and 0 <= t < P
    return t


def block_index(where, ct_len):
    """Index among the ciphertext blocks of the whole block to solve: "first", "last" (the last whole
    one), "lean" (the middle of the whole blocks: inside the lean stretch of every lane schedule when
    the packet has one) or an index."""
    full = ct_len // 16
    assert full >= 1, "a crafted packet needs one whole ciphertext block"
    k = {"first": 0, "last": full - 1, "lean": full // 2}.get(where, where)
    assert 0 <= k < full
    return k


def craft(key, nonce, aad, ct_len, target, where, fill, rng, free_aad=(), pinned=None):
    """(ct, tag): a ciphertext of ct_len bytes whose Poly1305 accumulator under (key, nonce, aad) is
    `target` (a residue, a name of TARGETS, TAG_ZERO or TAG_ONES), and its tag. The whole ciphertext
    block `where` is solved; the others are random bytes of rng, 0x00 or 0xFF (fill), except bytes
    `pinned` = {index: value} (outside the solved block). A draw that is not usable redraws one other
    block (the last one, or the first when that is the solved one; after the first redraw the fill no
    longer holds there) or, for a packet of a single block, the bytes free_aad of the bytearray aad,
    in place. At most MAX_DRAWS draws; NothingFree when there is nothing to redraw."""
    assert fill in FILLS
    r, s, _ = one_time_key(key, nonce)
    T = target_value(target, s)
    k = block_index(where, ct_len)
    nct = (ct_len + 15) // 16
    if fill == "random":
        ct = bytearray(rng.bytes(ct_len))
    else:
        ct = bytearray((b"\x00" if fill == "zeros" else b"\xff") * ct_len)
    pinned = dict(pinned or {})
    assert all(not 16 * k <= i < 16 * k + 16 for i in pinned)
    # the block a retry redraws: the last one with a free byte, the solved one apart
    spare = next((q for q in range(nct - 1, -1, -1)
                  if q != k and any(i not in pinned for i in range(16 * q, min(16 * q + 16, ct_len)))), None)
    can_redraw_ct = spare is not None
    lo, hi = (16 * spare, min(16 * spare + 16, ct_len)) if can_redraw_ct else (0, 0)
    if not can_redraw_ct and free_aad:
        assert isinstance(aad, bytearray)
    for draw in range(MAX_DRAWS):
        if draw:
            if can_redraw_ct:
                ct[lo:hi] = rng.bytes(hi - lo)
            elif free_aad:
                for i, v in zip(free_aad, rng.bytes(len(free_aad))):
                    aad[i] = v
            else:
                raise NothingFree
        for i, v in pinned.items():
            ct[i] = v
        ct[16 * k:16 * k + 16] = bytes(16)
        blocks = poly_blocks(mac_input(aad, ct))
        at = (len(aad) + 15) // 16 + k  # the solved block's index in the MAC input
        blocks[at] = 0
        base = accumulator(r, blocks)
        m = (T - base) * pow(r, -(len(blocks) - at), P) % P
        if not (1 << 128) <= m < (1 << 129):
            continue
        ct[16 * k:16 * k + 16] = (m - (1 << 128)).to_bytes(16, "little")
        h = accumulator(r, poly_blocks(mac_input(aad, ct)))
        assert h == T, "the crafted packet missed its target"
        return bytes(ct), tag_of(h, s)
    raise RuntimeError(f"no usable draw in {MAX_DRAWS} for target {target!r}")


def craft_any_nonce(key, aad_len, ct_len, target, where, fill, rng):
    """(nonce, aad, ct, tag) for a caller that is free to choose nonce and AAD (the per-packet trait
    calls): random ones of rng; a packet with nothing else to redraw takes another nonce."""
    for _ in range(MAX_DRAWS):
        nonce, aad = rng.bytes(12), bytearray(rng.bytes(aad_len))
        try:
            ct, tag = craft(key, nonce, aad, ct_len, target, where, fill, rng, free_aad=tuple(range(aad_len)))
            return nonce, bytes(aad), ct, tag
        except NothingFree:
            assert ct_len < 32 and aad_len == 0
    raise RuntimeError(f"no usable nonce in {MAX_DRAWS} for target {target!r}")


def nonce_of(iv, pn):
    """DirectionalKeys::nonce through the library's C ABI (a host function)."""
    from milli_quic_amd import crypto
    return crypto.nonce(bytes(iv), int(pn))


def craft_batch(b, picks, rng, free_aad=range(1, 9)):
    """For the QUIC rows `picks` = [(packet, target, where, fill), ...] of a batch b of the batch tests
    (keys, arena, sd, offs, L): the key row and packet number give the nonce, the unprotected header
    in b.arena is the AAD (a draw that is not usable on a one-block packet redraws its connection ID
    bytes free_aad in the arena: no kernel reads them as anything but AAD), the ciphertext is crafted
    and the plaintext that seals to it written into b.arena. Returns {packet: expected tag}."""
    tags = {}
    for p, target, where, fill in picks:
        row = b.keys[int(b.sd["key_id"][p])]
        key, nonce = bytes(row.key), nonce_of(row.iv, b.sd["pn"][p])
        o, n = int(b.sd["offset"][p]), int(b.sd["len"][p])
        na = int(b.sd["pn_offset"][p]) + int(b.sd["pn_len"][p])
        aad = bytearray(b.arena[o:o + na].tobytes())
        ct, tags[p] = craft(key, nonce, aad, n - na - 16, target, where, fill, rng, free_aad=tuple(free_aad))
        b.arena[o:o + na] = np.frombuffer(bytes(aad), dtype=np.uint8)
        b.arena[o + na:o + n - 16] = np.frombuffer(plaintext_for(ct, keystream(key, nonce, len(ct))), dtype=np.uint8)
    return tags


def spread(n, every=2, wheres=("first", "last", "lean"), fills=FILLS, first=0, start=0):
    """Picks for craft_batch: every `every`-th of n packets from `first` on, walking the targets, the
    solved block's place and the fill against each other."""
    names = list(TARGETS)
    return [(p, names[(start + i) % len(names)], wheres[i % len(wheres)], fills[(i // 2) % len(fills)])
            for i, p in enumerate(range(first, n, every))]
