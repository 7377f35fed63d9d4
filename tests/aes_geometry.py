"""A deterministic ladder of AES-128-GCM packets over the header and slot geometry of the streaming
tiles (milli_quic_amd/csrc/mq_aes.hip AesStream::seal / ::open), and the classes of that geometry a
batch covers, computed from the kernel's own formulas restated here.

A tile puts a packet on G lanes (8, 4 or 2): slot b >= 1 is CTR block b, slot 0 is E_K(J0), slots
1 - A .. 0 are the A AAD blocks, slot nblk = 1 + ceil(P / 16) the GHASH length block (and, in seal,
the header-protection block when nblk >= kHpSlotMin); lane j holds slots j, j + G, ... from iteration
it_lo = -wave_max((A + G - 2) / G). Random lengths reach most of this by chance; the ladder walks it:

  HEADERS   (pn_offset, pn_len, flags): an empty AAD, AADs that end on, one before and one after a
            block edge, PNs that straddle the edge between two AAD blocks (pn_offset 13..15, 29..31,
            45..47, 125..127 with pn_len >= 2), byte 0 and the PN up to 20 blocks apart, a TLS record;
  PAYLOADS  P = 0..5 and 16 k - 1, 16 k, 16 k + 1 for k = 0..18 (past 2 G + 2 slots at G = 8), every P
            in 0..300 for one header of each kind, and a few long payloads (LONG_P) so that a whole
            tile of 8-lane packets has more than one lean iteration;
  CTR_EDGE  packets of 4080, 4081 and 4100 bytes with 0..3 AAD blocks: the last length whose counters
            all stay below 256 (the CTR cache), the first one past it, and one more block.

build() lays the packets out back to back (any lead, order and key assignment), writes byte 0 and
the PN bytes, and makes the open descriptors' `largest` walk the three branches of decode_pn
(mq_tile.h; reference src/packet/number.rs:52-70).
"""
from dataclasses import dataclass

import numpy as np

from milli_quic_amd import _lib, workload
from milli_quic_amd.batch import make_descs

AES = _lib.MQ_SUITE_AES128GCM
NO_HP, LONG, RECORD = _lib.MQ_PKT_NO_HP, _lib.MQ_PKT_LONG_HEADER, _lib.MQ_PKT_TLS_RECORD
LANES = (8, 4, 2)

PLAIN_HEADERS = [(0, 0, NO_HP), (15, 1, NO_HP), (16, 0, NO_HP), (17, 0, NO_HP), (33, 4, NO_HP), (5, 0, NO_HP)]
RECORD_HEADER = (5, 0, RECORD)
SHORT_OFFSETS = (1, 9, 12, 13, 14, 15, 16, 17)
LONG_OFFSETS = (26, 28, 29, 30, 31, 32, 44, 45, 46, 47, 48, 60, 124, 125, 126, 127, 128, 140, 141, 320)
SHORT_HEADERS = [(o, pl, 0) for o in SHORT_OFFSETS for pl in (1, 2, 3, 4)]
LONG_HEADERS = [(o, pl, LONG) for o in LONG_OFFSETS for pl in (1, 2, 3, 4)]
HEADERS = PLAIN_HEADERS + [RECORD_HEADER] + SHORT_HEADERS + LONG_HEADERS

PAYLOADS = sorted(set(range(6)) | {16 * k + d for k in range(19) for d in (-1, 0, 1) if 16 * k + d >= 0})
# one header of each kind takes every payload length 0..300: a plain AEAD packet of two AAD blocks,
# the record, a short header, and a long header whose 4-byte PN straddles AAD blocks 1 and 2
SWEEP_HEADERS = [(17, 0, NO_HP), RECORD_HEADER, (9, 2, 0), (29, 4, LONG)]
SWEEP_PAYLOADS = range(301)
# whole tiles of long payloads: lean_end > 1 at G = 8 needs 22 whole blocks (P >= 352) on every packet
# of a tile; 8 lengths x the 4 sweep headers = 32 consecutive packets
LONG_P = (351, 352, 353, 367, 368, 369, 400, 480)
# the CTR cache holds while every counter of the wave stays below 256: packets up to 4080 bytes
CTR_LENS = (4080, 4081, 4100)
CTR_HEADERS = [(0, 0, NO_HP), (9, 2, 0), (26, 4, LONG), (44, 1, LONG)]  # A = 0, 1, 2, 3
RECORD_TYPES = (20, 21, 22, 23)
PN_MODES = ("next", "low_edge", "high_edge", "plus_win", "minus_win")


def is_hp(flags):
    return not flags & NO_HP


def is_record(flags):
    return bool(flags & 0x04)


def min_payload(pn_len, flags):
    """HP packets: the sample [pn_offset + 4, pn_offset + 20) lies inside the packet; records carry
    their inner content type."""
    if is_record(flags):
        return 1
    return 4 - pn_len if is_hp(flags) else 0


def ladder(ctr_edge=True):
    """The ladder as (pn_offset, pn_len, flags, P) rows: payload-major, so that the packets of a tile
    share a payload length and differ in their headers."""
    rows = []
    if ctr_edge:  # at the front: the first 8-lane tile is all CTR-edge packets
        rows += [(o, pl, f, L - o - pl - 16) for L in CTR_LENS for (o, pl, f) in CTR_HEADERS]
    rows += [(o, pl, f, P) for P in PAYLOADS for (o, pl, f) in HEADERS if P >= min_payload(pl, f)]
    rows += [(o, pl, f, P) for P in LONG_P for (o, pl, f) in SWEEP_HEADERS]
    rows += [(o, pl, f, P) for (o, pl, f) in SWEEP_HEADERS for P in SWEEP_PAYLOADS if P >= min_payload(pl, f)]
    return rows


def shortest(rows, max_len=64):
    """The ladder's packets of at most max_len bytes."""
    return [r for r in rows if r[0] + r[1] + r[3] + 16 <= max_len]


def one_per_geometry(rows):
    """Indices into rows: for every (pn_offset, pn_len, flags) the first packet with a payload of at
    least 33 bytes (three payload blocks, the last one partial), else its longest."""
    best = {}
    for i, (o, pl, f, P) in enumerate(rows):
        g = (o, pl, f)
        if g not in best or (rows[best[g]][3] < 33 and P > rows[best[g]][3]):
            best[g] = i
    return sorted(best.values())


# ---- decode_pn (RFC 9000 A.3) -----------------------------------------------------------------------
def decode_branch(trunc, pn_len, largest):
    """(pn, branch) of decode_pn: branch "plus_win", "minus_win" or "candidate"."""
    win = 1 << (8 * pn_len)
    hwin, mask = win >> 1, win - 1
    expected = largest + 1
    cand = (expected & ~mask) | trunc
    if cand + hwin <= expected and cand + win <= (1 << 62):
        return cand + win, "plus_win"
    if cand > expected + hwin and cand >= win:
        return cand - win, "minus_win"
    return cand, "candidate"


def pn_and_largest(pn, pn_len, mode):
    """The packet number (pn with its low 8 pn_len bits adjusted where the mode needs it) and the
    receiver's largest PN for one of PN_MODES."""
    win = 1 << (8 * pn_len)
    hwin, mask = win >> 1, win - 1
    if mode == "next":
        return pn, pn - 1
    if mode == "low_edge":
        return pn, pn - hwin + 1
    if mode == "high_edge":
        return pn, pn + hwin - 2
    if mode == "plus_win":   # expected at the end of the window block below pn's: candidate = pn - win
        pn &= ~hwin          # truncated < hwin
        return pn, pn - (pn & mask) - 2
    assert mode == "minus_win"  # expected at the start of the block above pn's: candidate = pn + win
    pn |= hwin | 1              # truncated > hwin
    return pn, (pn & ~mask) + win - 1


@dataclass
class Batch:
    keys: list
    arena: np.ndarray
    sd: np.ndarray     # seal descriptors
    od: np.ndarray     # open descriptors
    pns: np.ndarray    # what open reports: the packet number, or a record's data_len | type << 32
    rows: list         # (pn_offset, pn_len, flags, P) per descriptor
    branches: dict     # pn_len -> set of decode_pn branches taken


def build(rows, key_of=lambda i: 0, n_keys=1, lead=0, order=None, seed=1, keys=None, decode=None):
    """Descriptors and arena of the packets `rows` in the order `order` (a permutation; default: as
    given), back to back after `lead` bytes; descriptor i has key row key_of(i). Plaintext from the
    SplitMix64 stream; byte 0 (form bit, fixed bit, pn_len - 1, the rest random) and the PN bytes set
    for header-protected packets. The arena ends exactly at the last packet. decode: orc.decode_pn,
    checked against every open descriptor."""
    assert 0 <= lead < 16
    if order is not None:
        assert sorted(order) == list(range(len(rows)))
        rows = [rows[k] for k in order]
    n = len(rows)
    po = np.array([r[0] for r in rows], dtype=np.int64)
    pl = np.array([r[1] for r in rows], dtype=np.int64)
    fl = np.array([r[2] for r in rows], dtype=np.uint8)
    P = np.array([r[3] for r in rows], dtype=np.int64)
    L = po + pl + P + 16
    offs = lead + np.concatenate([[0], np.cumsum(L[:-1])]).astype(np.int64)
    arena = workload.splitmix_bytes(int(offs[-1] + L[-1]), seed=seed)
    rng = np.random.default_rng(seed)
    draw = (1 << 34) + rng.integers(0, 1 << 33, size=n)
    kid = np.array([key_of(i) for i in range(n)], dtype=np.uint32)
    assert (kid < n_keys).all()
    pns = np.zeros(n, dtype=np.uint64)
    largest = np.zeros(n, dtype=np.uint64)
    reserved = np.zeros(n, dtype=np.uint32)
    info = np.zeros(n, dtype=np.uint64)
    turn = {1: 0, 2: 0, 3: 0, 4: 0}
    branches = {1: set(), 2: set(), 3: set(), 4: set()}
    for i in range(n):
        o, f, q = int(offs[i]), int(fl[i]), int(pl[i])
        if is_record(f):
            reserved[i] = RECORD_TYPES[i % 4]
            pns[i] = largest[i] = int(draw[i])
            info[i] = (int(P[i]) - 1) | (int(reserved[i]) << 32)
            continue
        if not is_hp(f):
            pns[i] = largest[i] = info[i] = int(draw[i])
            continue
        mode = PN_MODES[turn[q] % len(PN_MODES)]
        turn[q] += 1
        pn, lg = pn_and_largest(int(draw[i]), q, mode)
        trunc = pn & ((1 << (8 * q)) - 1)
        got, br = decode_branch(trunc, q, lg)
        assert got == pn and (1 << 33) < lg < (1 << 35), (pn, q, mode)
        # the window's edges land in whichever branch the block boundaries make of them
        assert br == {"next": "candidate", "plus_win": "plus_win", "minus_win": "minus_win"}.get(mode, br), (pn, q, mode)
        if decode is not None:
            assert decode(trunc, q, lg) == pn, (pn, q, mode)
        branches[q].add(br)
        pns[i], largest[i], info[i] = pn, lg, pn
        arena[o] = (int(arena[o]) & 0x3C) | 0x40 | (0x80 if f & LONG else 0) | (q - 1)
        for b in range(q):
            arena[o + int(po[i]) + b] = (pn >> (8 * (q - 1 - b))) & 0xFF
    for q in (1, 2, 3, 4):  # a full turn of the modes takes every branch
        assert turn[q] < len(PN_MODES) or branches[q] == {"candidate", "plus_win", "minus_win"}, q
    if keys is None:
        keys = workload.uniform_keys(AES, n_keys)
    args = (offs.astype(np.uint64), L.astype(np.uint32), kid)
    sd = make_descs(*args, pns, po.astype(np.uint16), pl.astype(np.uint8), fl)
    sd["reserved"] = reserved
    # open: pn_len comes from the unmasked first byte (the descriptor's only for packets without HP)
    ofl = np.where(L > _lib.MQ_RECV_MAX_PACKET, fl | _lib.MQ_PKT_NO_RECV_LIMIT, fl).astype(np.uint8)
    od = make_descs(*args, largest, po.astype(np.uint16), np.where(fl & NO_HP, pl, 0).astype(np.uint8), ofl)
    return Batch(keys, arena, sd, od, info, rows, branches)


# ---- the classes of a batch ---------------------------------------------------------------------------
def hp_slot_min(G):
    return G if G >= 4 else 4


def lean_end_of(P, G):
    """lean_end<G> of one packet (the kernel takes the minimum over the wave's packets)."""
    F, E = P >> 4, 2 * G - 2
    return (F - E) // G + 1 if F >= E else 0


def classes(G, rows):
    """The geometry classes that `rows`, laid out in this order on tiles of 64 / G packets (the flat
    kernels: descriptor order), hit at G lanes per packet."""
    hit = set()
    for (o, pl, f, P) in rows:
        aad = o + pl
        A = (aad + 15) >> 4
        nblk = 1 + ((P + 15) >> 4)
        hp, rec = is_hp(f), is_record(f)
        hit.add(("A", min(A, 4)))
        hit.add(("iterations_below_zero", min((A + G - 2) // G, 2)))
        if A:
            hit.add(("aad_last_block", "full" if aad % 16 == 0 else "partial"))
        if hp:
            first, last = o >> 4, (o + pl - 1) >> 4
            hit.add(("byte0_and_pn", "one block" if last == 0 else "two blocks"))
            hit.add(("pn_split", first != last))
            hit.add(("hp_block", "slot nblk" if nblk >= hp_slot_min(G) else "late"))
            hit.add(("sample_in_tag", P < 20 - pl))
        hit.add(("nblk_mod_G", nblk % G))
        it_lo = -((A + G - 2) // G)
        for j in range(G):  # a lane that holds a GHASH block (slots 1 - A .. nblk) has a final multiplier
            if any(1 - A <= b <= nblk for b in range(j + G * it_lo, nblk + 1, G)):
                hit.add(("e1", j, (nblk + G - j) & (G - 1)))
        if P:
            hit.add(("last_block_bytes", P - 16 * ((P - 1) >> 4)))
        hit.add(("record", rec))
    ppt = 64 // G
    for t in range(0, len(rows), ppt):
        tile = rows[t:t + ppt]
        hit.add(("lean_end", min(min(lean_end_of(r[3], G) for r in tile), 2)))
        hit.add(("ctr_cached", not any(r[0] + r[1] + r[3] + 16 > 4080 for r in tile)))
    return hit


def all_classes(G):
    """Every class the ladder claims to cover at G lanes per packet."""
    want = {("A", a) for a in range(5)} | {("iterations_below_zero", v) for v in range(3)}
    want |= {("aad_last_block", v) for v in ("full", "partial")}
    want |= {("byte0_and_pn", v) for v in ("one block", "two blocks")}
    want |= {("pn_split", v) for v in (False, True)}
    want |= {("hp_block", v) for v in ("slot nblk", "late")}
    want |= {("sample_in_tag", v) for v in (False, True)}
    want |= {("nblk_mod_G", v) for v in range(G)}
    want |= {("e1", j, e) for j in range(G) for e in range(G)}
    want |= {("last_block_bytes", v) for v in range(1, 17)}
    want |= {("record", v) for v in (False, True)}
    want |= {("lean_end", v) for v in range(3)}
    want |= {("ctr_cached", v) for v in (False, True)}
    return want
