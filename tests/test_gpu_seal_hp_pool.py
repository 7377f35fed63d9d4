"""Seal's keystream pool with the header-protection blocks on lane pairs (mq_chacha.hip cc_pool_seal,
mq_chacha_pair.h) against the oracle, byte for byte: arena, statuses, and after opening the sealed
batch the packet numbers.

A workgroup of the flat octet kernels pools, per packet, its keystream blocks from slot 16 on
(ciphertext beyond 960 B: one entry per further 64 B) and one header-protection entry when the
16-B sample is all ciphertext (P + pn_len >= 20; else the wave computes the mask late). The pool runs
all keystream entries first, padded to whole wave-iterations, then the HP entries two lanes each, so
the batches here vary what the two prefix sums see: packets with 0, 1, 2 and 4 pooled keystream
entries side by side, packets with and without an HP entry, partial tiles, partial workgroups and a
second workgroup, every PN length (the sample's alignment), both header forms (both first-byte
masks), one key row and three (per-lane HP keys inside a pair iteration), packets packed back to
back at 16-B alignment (span tiles) and at offsets 1, 5 and 15 mod 16, and a refused packet in the
middle of a tile. The arena is padded behind the last packet so that its bytes per packet select
the kernel family under test (batch.flat_kind: 1 the 10-KiB images, 2 and 3 the 13- and 20-KiB ones).
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
SHORT, LONG = 9, 27  # bytes before the PN: first byte + 8-B DCID; a long header
NS = (1, 7, 8, 9, 31, 32, 33, 65)
LEADS = (0, 1, 5, 15)  # offset & 15 of the first packet
POOL_EDGE = (959, 960, 961, 1023, 1024, 1025)  # 0, 0, 1, 1, 1, 2 pooled keystream entries
CONFIG_B = 1171  # payload of a 1200-B short-header packet with a 4-B PN: 4 entries
# bytes per packet that select the kernel family (mq_chacha_flat_kind: <= 640 narrow, <= 1216 the
# 10-KiB images, <= 1584 the 13-KiB, above the 20-KiB)
BPP = {1: 1216, 2: 1584, 3: 1700}


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
    """Packets of payload (ciphertext) lengths P, packed back to back from byte `lead` on; hdr: bytes
    before the PN (SHORT or LONG, per packet). Guard bytes of 0xA5 before and behind, the trailing
    ones stretched until the arena has BPP[kind] bytes per packet (a single 1200-B packet leaves
    room for 16 guard bytes in all before the next family starts)."""

    def __init__(self, P, pn_len, hdr=SHORT, n_keys=1, lead=0, kind=1, seed=7):
        P = np.asarray(P, dtype=np.int64)
        n = len(P)
        pn_len = np.broadcast_to(np.asarray(pn_len, dtype=np.int64), (n,)).copy()
        hdr = np.broadcast_to(np.asarray(hdr, dtype=np.int64), (n,)).copy()
        self.P, self.L = P, hdr + pn_len + P + 16
        self.offs = lead + np.concatenate([[0], np.cumsum(self.L[:-1])]).astype(np.int64)
        self.end = int(self.offs[-1] + self.L[-1])
        size = max(self.end + 1, BPP[kind] * n)
        assert size // n <= BPP[kind], "packets too long for this kernel family"
        self.keys = workload.uniform_keys(CHACHA, n_keys)
        rng = np.random.default_rng(seed)
        self.pns = np.uint64(1 << 20) + rng.integers(0, 1 << 30, size=n).astype(np.uint64)
        arena = workload.splitmix_bytes(size, seed=seed)
        arena[:lead] = 0xA5
        arena[self.end:] = 0xA5
        for i in range(n):
            o, pl = int(self.offs[i]), int(pn_len[i])
            arena[o] = (0x40 if hdr[i] == SHORT else 0xC0) | (pl - 1)
            for b in range(pl):
                arena[o + int(hdr[i]) + b] = (int(self.pns[i]) >> (8 * (pl - 1 - b))) & 0xFF
        self.arena, self.lead = arena, lead
        flags = np.where(hdr == SHORT, 0, _lib.MQ_PKT_LONG_HEADER).astype(np.uint8)
        kid = (np.arange(n) % n_keys).astype(np.uint32)
        self.sd = make_descs(self.offs.astype(np.uint64), self.L.astype(np.uint32), kid, self.pns,
                             hdr.astype(np.uint16), pn_len.astype(np.uint8), flags)
        self.od = self.sd.copy()  # open: the largest PN of the space; pn_len comes from the header
        self.od["pn"] = self.pns - np.uint64(1)
        self.od["pn_len"] = 0
        assert batch.flat_kind(len(arena), n, CHACHA) == kind

    def guards_intact(self, a):
        return (a[:self.lead] == 0xA5).all() and (a[self.end:] == 0xA5).all()


def first_diff(b, x, y):
    at = int(np.nonzero(x != y)[0][0])
    p = max(int(np.searchsorted(b.offs, at, side="right")) - 1, 0)
    return f"first difference at arena byte {at}: packet {p}, byte {at - int(b.offs[p])} of {int(b.L[p])}"


def check(orc, b, refused=()):
    """Seal b on the GPU and in the oracle: same statuses, same arena. Then open what the GPU sealed:
    every packet not in `refused` opens (status 0) to its packet number and the plaintext arena."""
    o_out, o_st, _ = oracle_run(orc, b.keys, b.arena, b.sd)
    good = ~np.isin(np.arange(len(b.sd)), refused)
    assert (o_st[good] == 0).all() and (o_st[~good] == _lib.MQ_ERR_INVALID_ARG).all()
    g_out, g_st, _ = gpu_run(b.keys, b.arena, b.sd)
    assert (g_st == o_st).all(), np.nonzero(g_st != o_st)[0][:8]
    assert g_out.tobytes() == o_out.tobytes(), first_diff(b, g_out, o_out)
    assert b.guards_intact(g_out)
    o_back, o_st2, o_pn = oracle_run(orc, b.keys, g_out, b.od, open_=True)
    g_back, g_st2, g_pn = gpu_run(b.keys, g_out, b.od, open_=True)
    assert (g_st2 == o_st2).all() and (g_st2[good] == 0).all(), np.nonzero(g_st2 != o_st2)[0][:8]
    assert g_back.tobytes() == o_back.tobytes(), first_diff(b, g_back, o_back)
    assert (g_pn[good] == b.pns[good]).all() and (o_pn[good] == b.pns[good]).all()
    for i in np.nonzero(good)[0]:  # the plaintext is back (the tag stays behind it)
        o, e = int(b.offs[i]), int(b.offs[i] + b.L[i]) - 16
        assert g_back[o:e].tobytes() == b.arena[o:e].tobytes(), i
    return g_out


def leads_for(n, turn):
    """First-packet alignments of the turn-th (batch size, PN length) pair of a test's double loop:
    all four for a single packet, which nothing behind it shifts; else one, stepping with the batch
    size as well as the PN length, so that every PN length meets every alignment."""
    return LEADS if n == 1 else (LEADS[(turn + turn // 4) % 4],)


def turned(values, n, by):
    """n values, cycling through `values` from position `by`"""
    return [values[(i + by) % len(values)] for i in range(n)]


@pytest.mark.parametrize("hdr", [SHORT, LONG])
@pytest.mark.parametrize("n_keys", [1, 3])
def test_pool_boundary(orc, n_keys, hdr):
    # neighbours with 0, 0, 1, 1, 1 and 2 pooled keystream entries, every one with an HP entry: the
    # keystream part is never a whole iteration, and packets without a keystream entry sit between
    # packets with some. Every batch size, PN length and alignment.
    turn = 0
    for n in NS:
        for pn_len in (1, 2, 3, 4):
            for lead in leads_for(n, turn):
                check(orc, Batch(turned(POOL_EDGE, n, turn), pn_len, hdr, n_keys, lead=lead, seed=turn))
            turn += 1


@pytest.mark.parametrize("hdr", [SHORT, LONG])
@pytest.mark.parametrize("n_keys", [1, 3])
def test_late_path_boundary(orc, n_keys, hdr):
    # P + pn_len = 19 (the sample reaches into the tag: no pooled HP entry, the mask is made late),
    # 20 and 21 (pooled), beside packets with keystream entries: HP entries without keystream
    # entries, and packets with neither
    turn = 0
    for n in NS:
        for pn_len in (1, 2, 3, 4):
            P = turned((19 - pn_len, 20 - pn_len, 21 - pn_len, 1107, 20 - pn_len, 961, 19 - pn_len), n, turn)
            for lead in leads_for(n, turn):
                check(orc, Batch(P, pn_len, hdr, n_keys, lead=lead, seed=100 + turn))
            turn += 1
    for pn_len in (1, 2, 3, 4):  # a whole workgroup and more on the late path alone: an empty pool
        check(orc, Batch([19 - pn_len] * 33, pn_len, hdr, n_keys, seed=200 + pn_len))


@pytest.mark.parametrize("n_keys", [1, 3])
def test_config_b_payloads(orc, n_keys):
    # 1171-B payloads: four keystream entries and one HP entry per packet, 128 + 32 in a full
    # workgroup (two whole keystream iterations, one whole HP iteration). With a 4-B PN the packets
    # are 1200 B: back to back at lead 0 every full tile is a span tile.
    turn = 0
    for n in NS:
        for pn_len in (1, 2, 3, 4):
            for lead in sorted(set(leads_for(n, turn) + ((0,) if pn_len == 4 else ()))):
                check(orc, Batch([CONFIG_B] * n, pn_len, SHORT, n_keys, lead=lead, seed=300 + turn))
            turn += 1


def mixed(n, hdr_turn=0):
    """Every length above in one batch, PN lengths and header forms turning at other periods"""
    pls = turned((1, 2, 3, 4), n, 1)
    P = []
    for i, pl in enumerate(pls):
        P.append((POOL_EDGE + (19 - pl, 20 - pl, 21 - pl, CONFIG_B, 1171 - 64))[(5 * i) % 11])
    return P, pls, turned((SHORT, LONG, SHORT), n, hdr_turn)


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("n_keys", [1, 3])
def test_entry_count_mix(orc, n_keys, kind):
    # keystream and HP entry counts differ per packet, the keystream part is no whole iteration, and
    # the second workgroup holds one packet. The same batch through the 13- and 20-KiB kernels, whose
    # seal pools are the same code over larger images.
    for n, lead in ((65, 0), (32, 5), (33, 15)):
        P, pls, hdrs = mixed(n, hdr_turn=lead)
        per_wg = [sum(max(0, (p + 63) // 64 - 15) for p in P[i:i + 32]) for i in range(0, n, 32)]
        assert any(k % 64 for k in per_wg)
        check(orc, Batch(P, pls, hdrs, n_keys, lead=lead, kind=kind, seed=400 + n))


@pytest.mark.parametrize("n_keys", [1, 3])
def test_span_tiles_of_unequal_packets(orc, n_keys):
    # packet lengths that are multiples of 16, back to back from a 16-B-aligned start: span tiles
    # whose packets pool 4, 1, 0 and 2 keystream entries
    for n in (32, 33, 65):
        L = np.array(turned((1200, 1040, 976, 1104), n, n))
        b = Batch(L - 16 - SHORT - 4, 4, SHORT, n_keys, seed=500 + n)
        assert ((b.offs | b.L) & 15 == 0).all()
        check(orc, b)


@pytest.mark.parametrize("n_keys", [1, 3])
def test_refused_packet_inside_a_tile(orc, n_keys):
    # key_id == n_rows in the middle of the second tile: its record is cleared (no entry of either
    # kind), it keeps its bytes, and its neighbours' entries close ranks around it
    for P, pls, hdrs in (([CONFIG_B] * 32, 4, SHORT), mixed(32)):
        b = Batch(P, pls, hdrs, n_keys, seed=600)
        bad = 12
        b.sd["key_id"][bad] = n_keys
        b.od["key_id"][bad] = n_keys
        out = check(orc, b, refused=(bad,))
        o, e = int(b.offs[bad]), int(b.offs[bad] + b.L[bad])
        assert out[o:e].tobytes() == b.arena[o:e].tobytes()
