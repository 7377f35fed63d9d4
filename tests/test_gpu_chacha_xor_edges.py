"""Edges of the ChaCha20 keystream XOR and of the block function's counter / nonce words, against the
oracle byte for byte (arena, statuses, packet numbers), everything through batch.seal / batch.open_
(and send.protect for the fused build + seal tile).

A staged tile XORs its keystream into the LDS image with atomic XORs, one path for whole and partial
blocks (mq_device.h xor_words for LdsSpace): keystream past the block's length is zeroed, every one
of the 17 memory dwords under the block takes an XOR, so the bytes behind a partial block — the tag,
the next packet's header, the bytes behind the batch — take an XOR of zero and must come back as
they were. The direct path (tiles over the image budget) keeps the raw-dword read-modify-write.
Batches here are short-header packets packed back to back with no gap between 64 guard bytes of
0xA5 at either end of the arena: payload lengths are chosen per packet, the payload's alignment in
its dword through pn_len (pay = offset + 9 + pn_len), and the packet offsets follow from the lengths.
Kernel families (mq_chacha.hip): single-key ("1") and multi-key octet tiles over 10-, 13- and
20-KiB images with the workgroup's keystream pool (blocks >= 16), narrow tiles of 1 / 2 / 4 lanes
per packet, the partition lists of a MQ_SUITE_MIXED batch on either grid, the fused protect tile.
"MQ_CC_NARROW 1, 2 and 4" is read both ways: batches whose packets fit the narrow kernel's 1-, 2- and
4-lane groups, each run with the switch unset and set to 1, 2 and 4.
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, send, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable, make_descs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHACHA = _lib.MQ_SUITE_CHACHA20
GUARD = 64
HDR = workload.SHORT_HDR  # 9: first byte + 8-B DCID; the PN follows
# bytes in the last keystream block
LADDER = (1, 2, 3, 4, 5, 31, 32, 33, 61, 62, 63, 64)


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def gpu_run(keys, arena, desc, open_=False, hint=CHACHA):
    kt = KeyTable(keys)
    n = len(desc)
    a, d = to_dev(arena), to_dev(desc)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    pn = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.full((max(batch.workspace_bytes(n), 256),), 0xA5, dtype=torch.uint8, device=DEV)
    if open_:
        batch.open_(kt, a, d, st, pn, hint, ws)
    else:
        batch.seal(kt, a, d, st, hint, ws)
    torch.cuda.synchronize()
    return a.cpu().numpy(), st.cpu().numpy(), pn.cpu().numpy().view(np.uint64)


def oracle_run(orc, keys, arena, desc, open_=False, hint=CHACHA):
    a = arena.copy()
    if open_:
        st, pn = orc.batch_open(keys, a, desc, hint, threads=8)
        return a, st, pn
    return a, orc.batch_seal(keys, a, desc, hint, threads=8), None


class Batch:
    """Packets of payload lengths P packed back to back between the guards. kind: 0 QUIC short
    header (header protection), 1 plain AEAD row (MQ_PKT_NO_HP), 2 TLS record."""

    def __init__(self, P, pn_len, n_keys=1, pns=None, kind=None, seed=5):
        P, pn_len = np.asarray(P, dtype=np.int64), np.asarray(pn_len, dtype=np.int64)
        n = len(P)
        kind = np.zeros(n, dtype=np.int64) if kind is None else np.asarray(kind)
        pn_len = np.where(kind == 2, 0, pn_len)
        pn_off = np.where(kind == 2, 5, HDR)
        self.L = pn_off + pn_len + P + 16
        self.offs = GUARD + np.concatenate([[0], np.cumsum(self.L[:-1])]).astype(np.int64)
        self.end = int(self.offs[-1] + self.L[-1])
        self.pay_align = (self.offs + pn_off + pn_len) & 3
        self.keys = workload.uniform_keys(CHACHA, n_keys)
        rng = np.random.default_rng(seed)
        if pns is None:
            pns = np.uint64(1 << 20) + rng.integers(0, 1 << 30, size=n).astype(np.uint64)
        self.pns = np.asarray(pns, dtype=np.uint64)
        arena = workload.splitmix_bytes(self.end + GUARD, seed=seed)
        arena[:GUARD] = 0xA5
        arena[self.end:] = 0xA5
        for i in np.nonzero(kind == 0)[0]:
            o, pl = int(self.offs[i]), int(pn_len[i])
            arena[o] = 0x40 | (pl - 1)
            arena[o + 1:o + HDR] = np.frombuffer(workload.DCID8, dtype=np.uint8)
            for b in range(pl):
                arena[o + HDR + b] = (int(self.pns[i]) >> (8 * (pl - 1 - b))) & 0xFF
        self.arena = arena
        self.quic = kind == 0
        flags = np.where(kind == 1, _lib.MQ_PKT_NO_HP, np.where(kind == 2, _lib.MQ_PKT_TLS_RECORD, 0)).astype(np.uint8)
        kid = (np.arange(n) % n_keys).astype(np.uint32)
        args = (self.offs.astype(np.uint64), self.L.astype(np.uint32), kid)
        self.sd = make_descs(*args, self.pns, pn_off.astype(np.uint16), pn_len.astype(np.uint8), flags)
        self.sd["reserved"] = np.where(kind == 2, 23, 0)  # the record's inner content type
        # open: QUIC rows carry the largest PN of the space and learn pn_len from the header
        self.od = self.sd.copy()
        self.od["pn"][self.quic] = self.pns[self.quic] - np.uint64(1)
        self.od["pn_len"][self.quic] = 0
        self.od["reserved"] = 0

    def guards_intact(self, a):
        return (a[:GUARD] == 0xA5).all() and (a[self.end:] == 0xA5).all() and len(a) == self.end + GUARD


def check(orc, b, hint=CHACHA, tamper=(), bad=()):
    """Seal b, then open the oracle's sealed arena (bytes `tamper` = (packet, byte index from the
    packet's end, bit) flipped first): the GPU's arena, statuses and opened packet numbers are the
    oracle's, the guards stay. `bad`: packets expected to be refused on both sides. Returns the
    oracle's sealed arena and (opened arena, open statuses)."""
    o_out, o_st, _ = oracle_run(orc, b.keys, b.arena, b.sd, hint=hint)
    good = ~np.isin(np.arange(len(b.sd)), bad)
    assert (o_st[good] == 0).all() and (o_st[~good] != 0).all()
    g_out, g_st, _ = gpu_run(b.keys, b.arena, b.sd, hint=hint)
    assert (g_st == o_st).all(), np.nonzero(g_st != o_st)[0][:8]
    assert g_out.tobytes() == o_out.tobytes(), first_diff(b, g_out, o_out)
    assert b.guards_intact(g_out)
    rx = o_out.copy()
    for p, back, bit in tamper:
        rx[int(b.offs[p] + b.L[p]) - 1 - back] ^= 1 << bit
    o_back, o_st2, o_pn = oracle_run(orc, b.keys, rx, b.od, open_=True, hint=hint)
    hit = np.isin(np.arange(len(b.sd)), [t[0] for t in tamper])
    assert (o_st2[good & ~hit] == 0).all() and (o_st2[hit] == _lib.MQ_ERR_CRYPTO).all()
    g_back, g_st2, g_pn = gpu_run(b.keys, rx, b.od, open_=True, hint=hint)
    assert (g_st2 == o_st2).all(), np.nonzero(g_st2 != o_st2)[0][:8]
    assert g_back.tobytes() == o_back.tobytes(), first_diff(b, g_back, o_back)
    assert b.guards_intact(g_back)
    ok = (o_st2 == 0) & b.quic
    assert (g_pn[ok] == o_pn[ok]).all() and (g_pn[ok] == b.pns[ok]).all()
    return o_out, rx, o_back, o_st2


def first_diff(b, x, y):
    at = int(np.nonzero(x != y)[0][0])
    p = int(np.searchsorted(b.offs, at, side="right")) - 1
    return f"first difference at arena byte {at}: packet {p}, byte {at - int(b.offs[max(p, 0)])} of {int(b.L[max(p, 0)])}"


def ladder(nfull, tails=LADDER, reps=1):
    """One packet per (tail, payload alignment): nfull whole keystream blocks and `tail` bytes in the
    last one; pn_len is the one that puts the payload at the wanted alignment where the packet lands
    (so it, and the packet offset mod 4, vary along the batch). Returns (P, pn_len)."""
    P, pls, off = [], [], GUARD
    for _ in range(reps):
        for t in tails:
            for al in range(4):
                pl = 1 + (al - off - HDR - 1) % 4
                assert (off + HDR + pl) % 4 == al
                P.append(64 * nfull + t)
                pls.append(pl)
                off += HDR + pl + P[-1] + 16
    return P, pls


# the last block in a wave's iteration 0 (P <= 448), in iteration 1 (P <= 960), in the pool (P > 960;
# pool1200: 19 blocks as a 1200-B packet's, the last one of 19 bytes among the short tails)
CLASSES = {"it0": (5, LADDER), "it1": (13, LADDER), "pool": (17, LADDER), "pool1200": (18, (19,) + LADDER[:5])}


@pytest.mark.parametrize("n_keys", [1, 2])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_tail_ladder(orc, cls, n_keys):
    nfull, tails = CLASSES[cls]
    P, pls = ladder(nfull, tails, reps=-(-64 // (4 * len(tails))))
    b = Batch(P, pls, n_keys, seed=11 + nfull)
    assert 64 <= len(P) <= 256 and set(b.pay_align.tolist()) == {0, 1, 2, 3} and set(pls) == {1, 2, 3, 4}
    assert len(set((b.offs & 3).tolist())) == 4
    if cls == "pool1200":
        assert 1196 <= b.L.max() <= 1200  # block 19 of 19 bytes, as a 1200-B packet's (test_uniform_1200)
    # it0's packets average under 640 B: the product runs them on narrow tiles, MQ_CC_NARROW=0 on
    # the octet tiles this class is about
    for mode in (("0", None) if cls == "it0" else (None,)):
        with _lib.option("MQ_CC_NARROW", mode):
            if mode is None:
                assert batch.flat_kind(len(b.arena), len(P), CHACHA) == (0 if cls == "it0" else 1)
            check(orc, b)


def test_uniform_1200(orc):
    # config B's packets (16-B aligned, span tiles) between the guards: every pooled wave-iteration
    # holds the 19-byte block 19 beside whole blocks
    for pn_len in (1, 2, 3, 4):
        b = Batch([1200 - HDR - pn_len - 16] * 72, [pn_len] * 72, seed=pn_len)
        assert (b.L == 1200).all() and batch.flat_kind(len(b.arena), 72, CHACHA) == 1
        check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 3])
def test_mixed_tiles(orc, n_keys):
    # lengths differ inside every tile (whole-block and partial-block lanes, own iterations and pool
    # entries of different counts in one wave); descriptor 21 (inside the third tile) is invalid
    rng = np.random.default_rng(77 + n_keys)
    n = 128
    P = rng.choice([20, 63, 64, 65, 447, 448, 449, 512, 959, 960, 961, 1024, 1087, 1088, 1153, 1171], size=n)
    P[:8] = [64, 65, 960, 961, 1024, 1025, 1171, 20]
    b = Batch(P, rng.integers(1, 5, size=n), n_keys, seed=3)
    b.sd["key_id"][21] = n_keys
    b.od["key_id"][21] = n_keys
    assert batch.flat_kind(len(b.arena), n, CHACHA) == 1
    o_out, _, o_back, _ = check(orc, b, bad=(21,))
    lo, hi = int(b.offs[21]), int(b.offs[21] + b.L[21])
    assert o_out[lo:hi].tobytes() == b.arena[lo:hi].tobytes() and o_back[lo:hi].tobytes() == b.arena[lo:hi].tobytes()


@pytest.mark.parametrize("n_keys", [1, 2])
@pytest.mark.parametrize("L,kind", [(1232, 2), (1616, 3)])
def test_long_images(orc, L, kind, n_keys):
    # 13- and 20-KiB images; pn_len (and with it the last block's bytes) cycles inside a tile
    pls = 1 + np.arange(72) % 4
    b = Batch(L - HDR - pls - 16, pls, n_keys, seed=L)
    assert (b.L == L).all() and batch.flat_kind(len(b.arena), 72, CHACHA) == kind
    check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 2])
@pytest.mark.parametrize("G,lmax", [(1, 150), (2, 300), (4, 600)])
def test_narrow_groups(orc, G, lmax, n_keys):
    # flat batches of short packets: 64 / 32 / 16 images of at most lmax bytes fit a wave's LDS, so
    # the narrow kernel runs them G lanes per packet; every tail of the ladder at every block count
    # up to lmax, with the switch unset and at 1, 2 and 4
    P, pls, off, k = [], [], GUARD, 0
    nmax = (lmax - HDR - 4 - 16) // 64
    for rep in range(4):
        for t in LADDER:
            nfull = (k * 5 + rep) % nmax if nmax else 0
            k += 1
            for al in range(4 if G == 1 else 2):
                al = (al * 2 + rep) % 4 if G > 1 else al
                pl = 1 + (al - off - HDR - 1) % 4
                p = min(64 * nfull + t, lmax - HDR - pl - 16)
                P.append(p)
                pls.append(pl)
                off += HDR + pl + p + 16
    b = Batch(P, pls, n_keys, seed=G)
    assert 64 <= len(P) <= 256 and b.L.max() <= lmax
    assert batch.flat_kind(len(b.arena), len(P), CHACHA) == 0
    for mode in (None, "1", "2", "4"):
        with _lib.option("MQ_CC_NARROW", mode):
            check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 2])
def test_direct_tile_beside_staged_tiles(orc, n_keys):
    # the fourth tile's eight 1400-B packets exceed the 10-KiB image budget: it runs on the arena
    # (direct path, raw-dword XOR) between staged tiles; ladder tails in every tile
    P, pls = [], []
    for i in range(64):
        pl = 1 + i % 4
        P.append((1344 if i // 8 == 3 else 896) + LADDER[(i * 5) % 12])
        pls.append(pl)
    b = Batch(P, pls, n_keys, seed=9)
    assert batch.flat_kind(len(b.arena), 64, CHACHA) == 1 and b.L[24:32].sum() > 10240
    check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 2])
@pytest.mark.parametrize("grid", [None, "0", "1"])
def test_mixed_suite_lists(orc, grid, n_keys):
    # MQ_SUITE_MIXED: the device partition's ChaCha20 list (octet and narrow regions) on the one-shot
    # grid and on the persistent list kernels ("1"); one key row runs the lists' single-key kernels
    rng = np.random.default_rng(5 + n_keys)
    n = 200
    P = 64 * rng.integers(0, 19, size=n) + rng.choice(LADDER, size=n)
    b = Batch(P, rng.integers(1, 5, size=n), n_keys, seed=13)
    with _lib.option("MQ_CC_LIST", grid):
        check(orc, b, hint=_lib.MQ_SUITE_MIXED)


@pytest.mark.parametrize("cls", ["it1", "pool"])
@pytest.mark.parametrize("pos", [0, 3, 7])
def test_open_failure_keeps_received_bytes(orc, cls, pos):
    # one tampered packet per tile, first / middle / last of its tile: it keeps every received byte
    # (no XOR ran on it, header still protected) and its neighbours open
    nfull, tails = CLASSES[cls]
    P, pls = ladder(nfull, tails)
    P, pls = (P + P)[:64], (pls + pls)[:64]
    b = Batch(P, pls, seed=17)
    tam = [(8 * t + pos, (t * 5) % 40, t % 8) for t in range(8)]  # in the tag or the ciphertext's end
    _, rx, o_back, o_st2 = check(orc, b, tamper=tam)
    for p, _, _ in tam:
        lo, hi = int(b.offs[p]), int(b.offs[p] + b.L[p])
        assert o_back[lo:hi].tobytes() == rx[lo:hi].tobytes()
    assert (o_st2 == 0).sum() == 56


@pytest.mark.parametrize("n_keys", [1, 3])
def test_nonce_words(orc, n_keys):
    # the packet number's high word enters nonce word 1, its low word nonce word 2, nonce word 0 is
    # the row's iv[0] alone: PNs >= 2^32, tiles whose packets differ in the high word, PNs up to
    # 2^62 - 1, and (n_keys = 3) rows of different iv[0] alternating inside every tile
    n = 96
    i = np.arange(n, dtype=np.uint64)
    pns = np.empty(n, dtype=np.uint64)
    pns[:32] = (np.uint64(1) << np.uint64(32)) + i[:32] * np.uint64(0x01000193)          # one high word
    pns[32:64] = ((i[32:64] % np.uint64(8) + np.uint64(1)) << np.uint64(32 + 5)) + i[32:64]  # eight per tile
    pns[64:] = np.uint64((1 << 62) - 1) - (i[64:] - np.uint64(64)) * np.uint64(0x100000001)
    pns[64] = np.uint64((1 << 62) - 1)
    P = [1171, 1088 + 19, 960, 448 + 33][:4] * (n // 4)
    b = Batch(P, 1 + np.arange(n) % 4, n_keys, pns=pns, seed=23)
    if n_keys > 1:
        assert len({bytes(k.iv)[:4] for k in b.keys}) == n_keys
    check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 2])
def test_rows_without_header_protection(orc, n_keys):
    # plain AEAD rows (MQ_PKT_NO_HP: no mask, pn_len 0..4 of AAD behind pn_offset) and TLS records
    # (5-B header written by the seal, inner content type as the last payload byte) among QUIC rows
    rng = np.random.default_rng(31)
    n = 96
    kind = np.arange(n) % 3
    P = 64 * rng.integers(0, 19, size=n) + rng.choice(LADDER, size=n)
    pls = np.where(kind == 1, rng.integers(0, 5, size=n), rng.integers(1, 5, size=n))
    b = Batch(P, pls, n_keys, kind=kind, seed=29)
    check(orc, b)
    for k in (1, 2):  # and whole batches of one kind (every lane of every wave)
        check(orc, Batch(P[:64], pls[:64], n_keys, kind=np.full(64, k), seed=30 + k))


def test_protect_from_frames(orc):
    # the fused build + seal tile (ChaCha20 hint): 1-RTT packets built from frames of the ladder's
    # payload lengths into back-to-back output slots between the guards, against the oracle's
    # protect; the payload is the frames (at least 4 B with the PN: no padding is added above that)
    P, _ = ladder(17, LADDER + (19 + 64,))
    n = len(P)
    w = workload.config_b(8)
    conns = send.make_conns([workload.DCID8], [b""], [[0, 0, 0]])
    fl = np.asarray(P, dtype=np.int64)
    req = np.zeros(n, dtype=send.REQ_DTYPE)
    req["frames_offset"] = np.concatenate([[0], np.cumsum(fl[:-1])]).astype(np.uint64)
    req["pn"] = 0x10000000 + np.arange(n, dtype=np.uint64)
    # PN lengths 1..4 by the distance to the largest acknowledged
    req["largest_acked"] = req["pn"] - (np.uint64(1) << (np.uint64(8) * (np.arange(n, dtype=np.uint64) % np.uint64(4)) + np.uint64(3)))
    req["frame_len"], req["level"] = fl, send.APPLICATION
    req["out_cap"] = HDR + 4 + fl + 16
    req["out_offset"] = GUARD + np.concatenate([[0], np.cumsum(req["out_cap"][:-1].astype(np.int64))]).astype(np.uint64)
    end = int(req["out_offset"][-1]) + int(req["out_cap"][-1])
    frames = workload.splitmix_bytes(int(fl.sum()), seed=3)
    out = np.full(end + GUARD, 0xA5, dtype=np.uint8)
    o_out = out.copy()
    o_st, o_ln = orc.batch_protect(w.keys, conns, frames, o_out, req, CHACHA)
    assert (o_st == 0).all() and len(set(o_ln.tolist())) > 12
    kt = KeyTable(w.keys)
    g = to_dev(out)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    send.protect(kt, to_dev(conns), to_dev(frames), g, to_dev(req), st, ln, CHACHA, ws)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == o_st).all() and (ln.cpu().numpy().view(np.uint32) == o_ln).all()
    assert g.cpu().numpy().tobytes() == o_out.tobytes()
    assert (o_out[:GUARD] == 0xA5).all() and (o_out[end:] == 0xA5).all()
