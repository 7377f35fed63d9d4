"""Steps of the interleaved Poly1305 (mq_chacha.hip poly_tag, schedule in mq_poly_sched.h) against the
oracle byte for byte (arena, statuses, packet numbers), everything through batch.seal / batch.open_.

A lane group of G lanes runs Kmax steps over a packet's nb = A + T + 1 MAC blocks (A of AAD, T of
ciphertext, one of lengths) behind z = G Kmax - nb prepended zero blocks: general steps at the edges,
a lean stretch of whole ciphertext blocks that may run up to step Kmax - 2 and load a partial block
or the slot behind the ciphertext for the final absorb. The batches here pick the geometry per tile:
every residue of nb mod G, Kmax of 1, 2, 3, 4 and 10, ciphertext of 0, 1 and 15 bytes mod 16, every
payload alignment (pn_len), one to three AAD blocks, tiles of unequal packets, inactive octets, narrow
tiles, the direct path, the long-image kernels, a packet that ends with the arena, tampered packets.
Packets are packed back to back between 64 guard bytes of 0xA5 at either end of the arena.
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable, make_descs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHACHA = _lib.MQ_SUITE_CHACHA20
GUARD = 64
SHORT = workload.SHORT_HDR  # 9: first byte + 8-B DCID; the PN follows


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def gpu_run(keys, arena, desc, open_=False):
    kt = KeyTable(keys)
    n = len(desc)
    a, d = to_dev(arena), to_dev(desc)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    pn = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.full((max(batch.workspace_bytes(n), 256),), 0xA5, dtype=torch.uint8, device=DEV)
    if open_:
        batch.open_(kt, a, d, st, pn, CHACHA, ws)
    else:
        batch.seal(kt, a, d, st, CHACHA, ws)
    torch.cuda.synchronize()
    return a.cpu().numpy(), st.cpu().numpy(), pn.cpu().numpy().view(np.uint64)


def oracle_run(orc, keys, arena, desc, open_=False):
    a = arena.copy()
    if open_:
        st, pn = orc.batch_open(keys, a, desc, CHACHA, threads=8)
        return a, st, pn
    return a, orc.batch_seal(keys, a, desc, CHACHA, threads=8), None


class Batch:
    """Packets of ciphertext lengths P packed back to back behind the leading guard. hdr: bytes
    before the PN (9: short header; more: a long header, the AAD is hdr + pn_len bytes). A payload
    too small for the header-protection sample (hdr + 20 > packet) makes a plain AEAD row
    (MQ_PKT_NO_HP). tail: guard bytes behind the last packet (0: it ends with the arena)."""

    def __init__(self, P, pn_len, hdr=SHORT, n_keys=1, seed=5, tail=GUARD):
        P, pn_len = np.asarray(P, dtype=np.int64), np.asarray(pn_len, dtype=np.int64)
        n = len(P)
        hdr = np.broadcast_to(np.asarray(hdr, dtype=np.int64), (n,)).copy()
        self.L = hdr + pn_len + P + 16
        self.aad = hdr + pn_len
        plain = hdr + 20 > self.L
        self.offs = GUARD + np.concatenate([[0], np.cumsum(self.L[:-1])]).astype(np.int64)
        self.end = int(self.offs[-1] + self.L[-1])
        self.tail = tail
        self.keys = workload.uniform_keys(CHACHA, n_keys)
        rng = np.random.default_rng(seed)
        self.pns = np.uint64(1 << 20) + rng.integers(0, 1 << 30, size=n).astype(np.uint64)
        arena = workload.splitmix_bytes(self.end + tail, seed=seed)
        arena[:GUARD] = 0xA5
        arena[self.end:] = 0xA5
        for i in range(n):
            o, pl = int(self.offs[i]), int(pn_len[i])
            if not plain[i]:
                arena[o] = (0x40 if hdr[i] == SHORT else 0xC0) | (pl - 1)
            for b in range(pl):
                arena[o + int(hdr[i]) + b] = (int(self.pns[i]) >> (8 * (pl - 1 - b))) & 0xFF
        self.arena = arena
        self.quic = ~plain
        flags = np.where(plain, _lib.MQ_PKT_NO_HP, np.where(hdr == SHORT, 0, _lib.MQ_PKT_LONG_HEADER)).astype(np.uint8)
        kid = (np.arange(n) % n_keys).astype(np.uint32)
        self.sd = make_descs(self.offs.astype(np.uint64), self.L.astype(np.uint32), kid, self.pns,
                             hdr.astype(np.uint16), pn_len.astype(np.uint8), flags)
        # open: QUIC rows carry the largest PN of the space and learn pn_len from the header
        self.od = self.sd.copy()
        self.od["pn"][self.quic] = self.pns[self.quic] - np.uint64(1)
        self.od["pn_len"][self.quic] = 0

    def guards_intact(self, a):
        return (a[:GUARD] == 0xA5).all() and (a[self.end:] == 0xA5).all() and len(a) == self.end + self.tail

    def mac_blocks(self):
        return (self.aad + 15) // 16 + (self.L - self.aad - 16 + 15) // 16 + 1


def first_diff(b, x, y):
    at = int(np.nonzero(x != y)[0][0])
    p = int(np.searchsorted(b.offs, at, side="right")) - 1
    return f"first difference at arena byte {at}: packet {p}, byte {at - int(b.offs[max(p, 0)])} of {int(b.L[max(p, 0)])}"


def check(orc, b, tamper=()):
    """Seal b, then open the oracle's sealed arena (bits `tamper` = (packet, byte of the packet, bit)
    flipped first): the GPU's arena, statuses and packet numbers are the oracle's, the guards stay.
    Returns (received arena, the oracle's opened arena and statuses)."""
    o_out, o_st, _ = oracle_run(orc, b.keys, b.arena, b.sd)
    assert (o_st == 0).all()
    g_out, g_st, _ = gpu_run(b.keys, b.arena, b.sd)
    assert (g_st == o_st).all(), np.nonzero(g_st != o_st)[0][:8]
    assert g_out.tobytes() == o_out.tobytes(), first_diff(b, g_out, o_out)
    assert b.guards_intact(g_out)
    rx = o_out.copy()
    for p, at, bit in tamper:
        rx[int(b.offs[p]) + (at if at >= 0 else int(b.L[p]) + at)] ^= 1 << bit
    o_back, o_st2, o_pn = oracle_run(orc, b.keys, rx, b.od, open_=True)
    hit = np.isin(np.arange(len(b.sd)), [t[0] for t in tamper])
    assert (o_st2[~hit] == 0).all() and (o_st2[hit] == _lib.MQ_ERR_CRYPTO).all()
    g_back, g_st2, g_pn = gpu_run(b.keys, rx, b.od, open_=True)
    assert (g_st2 == o_st2).all(), np.nonzero(g_st2 != o_st2)[0][:8]
    assert g_back.tobytes() == o_back.tobytes(), first_diff(b, g_back, o_back)
    assert b.guards_intact(g_back)
    ok = (o_st2 == 0) & b.quic
    assert (g_pn[ok] == o_pn[ok]).all() and (g_pn[ok] == b.pns[ok]).all()
    return rx, o_back, o_st2


def ct_len(nb, A, mod):
    """Ciphertext bytes of a packet of nb MAC blocks with A of AAD whose length is `mod` mod 16
    (T = nb - A - 1 blocks; a packet without ciphertext blocks has no ciphertext)."""
    T = nb - A - 1
    assert T >= 0
    return 0 if T == 0 else 16 * T - (16 - mod) % 16


MODS = (0, 1, 15)
KMAX = (1, 2, 3, 4, 10)


def test_octet_tiles_every_residue(orc):
    # tiles of eight equal packets: per (Kmax, ciphertext length mod 16) one batch with one tile per
    # residue z = 8 Kmax - nb; pn_len (payload alignment) turns with the tile and the batch.
    # Kmax = 3 is the first whose lean stretch ends at Kmax - 2. (z = 7 at Kmax = 1 would be a packet
    # of one MAC block: no AAD.)
    turn = 0
    with _lib.option("MQ_CC_NARROW", "0"):
        for kmax in KMAX:
            for mod in MODS:
                P, pls = [], []
                for z in range(8):
                    if 8 * kmax - z < 2:
                        continue
                    P += [ct_len(8 * kmax - z, 1, mod)] * 8
                    pls += [1 + (z + turn) % 4] * 8
                turn += 1
                b = Batch(P, pls, seed=10 * kmax + mod)
                assert ((b.mac_blocks() + 7) // 8 == kmax).all() and len(P) <= 64
                check(orc, b)


# the flat narrow kernel's rule (mq_chacha.hip chacha_narrow_flat): a wave of 64 packets runs one
# lane per packet when their images fit the wave's LDS (636 chunks of 16 B), else two lanes when
# each half fits, else four when each quarter fits
NARROW_LMAX = {1: 150, 2: 290, 4: 600}


def narrow_group(b):
    nch = ((b.offs & 15) + b.L + 15) >> 4
    assert len(nch) <= 64
    c = np.zeros(64, dtype=np.int64)
    c[:len(nch)] = nch
    for G in (1, 2, 4):
        if all(c[r:r + 64 // G].sum() <= 636 for r in range(0, 64, 64 // G)):
            return G
    return 8


def narrow_batch(G, kmax, mod, zs, seed):
    """One wave of 64 packets for the narrow kernel's G-lane groups: tile r (64 / G packets) holds
    equal packets of residue zs[r], or, where zs[r] is None, packets of the longest length that
    keeps the wave on G lanes. None when a packet would be too long for the group."""
    P, pls = [], []
    for r, z in enumerate(zs):
        pl = 1 + (r + kmax + mod) % 4
        p = NARROW_LMAX[G] - SHORT - pl - 16 if z is None else ct_len(G * kmax - z, 1, mod)
        if SHORT + pl + p + 16 > NARROW_LMAX[G]:
            return None
        P += [p] * (64 // G)
        pls += [pl] * (64 // G)
    return Batch(P, pls, seed=seed)


KMAX_NARROW = (1, 2, 3, 4, 9)  # 9: the longest packets of a lane group have 9 G MAC blocks


def narrow_batches(G):
    out = []
    for kmax in KMAX_NARROW:
        for mod in MODS:
            if G == 1:
                plans = [[0]]
            elif G == 2:
                plans = [[0, None], [1, None]]
            else:
                plans = [[0, None, 1, None], [2, None, 3, None]]
            for zs in plans:
                if any(z is not None and G * kmax - z < 2 for z in zs):
                    continue
                b = narrow_batch(G, kmax, mod, zs, seed=1000 * G + 10 * kmax + mod)
                if b is not None:
                    out.append((kmax, zs, b))
    return out


@pytest.mark.parametrize("G", [1, 2, 4])
def test_narrow_tiles_every_residue(orc, G):
    # MQ_CC_NARROW = 1 runs the narrow kernels; which lane group a wave gets follows from its packets
    # (narrow_group), so each batch is one wave whose first tile (G = 4: first and third) holds the
    # equal packets under test
    got = narrow_batches(G)
    assert {z for _, zs, _ in got for z in zs if z is not None} == set(range(G))
    assert {k for k, _, _ in got} == {k for k in KMAX_NARROW if G * k >= 2}
    with _lib.option("MQ_CC_NARROW", "1"):
        for kmax, zs, b in got:
            assert narrow_group(b) == G, (kmax, zs)
            q = 64 // G
            for r, z in enumerate(zs):
                if z is not None:
                    assert ((b.mac_blocks()[q * r:q * r + q] + G - 1) // G == kmax).all()
            check(orc, b)


def test_long_headers_and_inactive_octets(orc):
    with _lib.option("MQ_CC_NARROW", "0"):
        # A = 2 and 3 (AAD of 27..30 and 41..44 bytes), every residue of nb mod 8 at Kmax = 3 and 10
        for hdr, A in ((26, 2), (40, 3)):
            for kmax in (3, 10):
                P, pls = [], []
                for z in range(8):
                    pl = 1 + (z + A) % 4
                    P += [ct_len(8 * kmax - z, A, MODS[z % 3])] * 8
                    pls += [pl] * 8
                b = Batch(P, pls, hdr=hdr, seed=hdr + kmax)
                assert ((b.aad + 15) // 16 == A).all() and ((b.mac_blocks() + 7) // 8 == kmax).all()
                check(orc, b)
        # 1, 3 and 9 packets: the last tile's other octets are inactive
        for n in (1, 3, 9):
            for kmax, mod in ((1, 1), (3, 15), (10, 0)):
                b = Batch([ct_len(8 * kmax - 3, 1, mod)] * n, [1 + (n + k) % 4 for k in range(n)], seed=n)
                check(orc, b)
    # config B's own geometry (1200-B packets, AAD 13 B, ciphertext 1171 B) with idle octets
    check(orc, Batch([1171] * 9, [4] * 9, seed=2))


def test_mixed_tiles(orc):
    # packets of different nb in one tile: klo, khi and Kmax come from the wave reductions. Tile 0
    # holds a packet of one step (Kmax = 1 alone) beside one of ten; the others are random draws.
    rng = np.random.default_rng(41)
    P = [3, 1171, 160, 1170, 16, 1185, 0, 97]
    pls = [2, 4, 1, 3, 4, 2, 4, 1]
    P += list(rng.choice([0, 1, 15, 16, 17, 95, 96, 111, 112, 113, 300, 448, 703, 1100, 1171, 1187], size=56))
    pls += list(rng.integers(1, 5, size=56))
    pls = [max(pl, 4 - p) for p, pl in zip(P, pls)]  # the header-protection sample fits
    b = Batch(P, pls, seed=43)
    nb = b.mac_blocks()
    assert (nb[0] + 7) // 8 == 1 and (nb[1] + 7) // 8 == 10
    for mode in ("0", None):
        with _lib.option("MQ_CC_NARROW", mode):
            check(orc, b)
    # the same on narrow tiles of 4 lanes per packet (packets up to 600 B)
    b = Batch(np.minimum(P, 560), pls, seed=44)
    assert narrow_group(b) == 4
    with _lib.option("MQ_CC_NARROW", "1"):
        check(orc, b)


def test_direct_path_and_long_images(orc):
    # direct path: eight packets over the image budget of the largest (20-KiB) image run on the arena
    for L in (2500, 2531):
        pls = 1 + np.arange(8) % 4
        b = Batch(L - SHORT - pls - 16, pls, seed=L)
        b.sd["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
        b.od["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
        assert b.L.sum() > 20480 - 512  # the image less the wave's scratch
        check(orc, b)
    # a direct tile (its packets exceed the 10-KiB image) between staged tiles of one batch
    P = [1100 if i // 8 != 1 else 1360 + i for i in range(64)]
    b = Batch(P, 1 + np.arange(64) % 4, seed=7)
    assert batch.flat_kind(len(b.arena), 64, CHACHA) == 1 and b.L[8:16].sum() > 10240
    check(orc, b)
    # long-image kernels: 13-KiB (1232..1584 B) and 20-KiB (1600..2400 B) images
    for L, kind in ((1233, 2), (1500, 2), (1601, 3), (2047, 3)):
        pls = 1 + np.arange(24) % 4
        b = Batch(L - SHORT - pls - 16, pls, seed=L)
        assert batch.flat_kind(len(b.arena), 24, CHACHA) == kind
        check(orc, b)


def test_last_packet_ends_the_arena(orc):
    # no guard behind the last packet (as bench.py lays out its arena): the look-ahead load of the
    # last step reads up to 19 bytes behind the tag, which here lie behind the arena
    for P, mode in (([1171] * 16, None), ([1171, 1170, 1169, 1160, 1157, 1156, 1155, 1168] * 2, None),
                    ([1400] * 8, None), ([2400] * 8, None), ([100, 99, 98, 97] * 16, "1"), ([37] * 3, "0")):
        n = len(P)
        b = Batch(P, 1 + np.arange(n) % 4, seed=n + P[0], tail=0)
        if max(P) > 2000:
            b.sd["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
            b.od["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
        assert len(b.arena) == b.end
        with _lib.option("MQ_CC_NARROW", mode):
            check(orc, b)


def test_tampered_packets(orc):
    # one bit flipped in the last ciphertext byte of a partial last block, in the first AAD byte, in
    # the tag: refused with the oracle's status, every received byte kept; the neighbours open
    P = [1171, 1163, 337, 1185] * 6
    pls = [1 + k % 4 for k in range(24)]
    b = Batch(P, pls, seed=19)
    assert all(p % 16 for p in P)
    for name, tam in (("ciphertext", [(8 * t + 3 * t, -17, t) for t in range(3)]),
                      ("aad", [(8 * t + 1 + t, 0, 5 + t) for t in range(3)]),
                      ("tag", [(8 * t + 7 - t, -1 - 5 * t, 7 - t) for t in range(3)])):
        for mode in ("0", None):
            with _lib.option("MQ_CC_NARROW", mode):
                rx, o_back, o_st2 = check(orc, b, tamper=tam)
        for p, _, _ in tam:
            lo, hi = int(b.offs[p]), int(b.offs[p] + b.L[p])
            assert o_back[lo:hi].tobytes() == rx[lo:hi].tobytes(), name
        assert (o_st2 == 0).sum() == 21, name
