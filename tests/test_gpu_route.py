"""Datagram routing on the GPU (mq_batch_route, mq_cid_table_*) against the Python model of
route_model.py; equality is exact. Sizes 1 / 63 / 64 / 65 lanes around one wave, 257 = one 256-lane
block plus one lane, 5000 = twenty blocks; table capacities 8 / 64 / 4096 (16 / 128 / 8192 slots),
filled to exactly the capacity in some cases."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, recv, route  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402
from milli_quic_amd.key_schedule import derive_initial_secrets, key_material  # noqa: E402

import route_model  # noqa: E402
from recv_traffic import protect_one  # noqa: E402
from route_model import AdmitModel, TableModel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = bytes.fromhex("000102030405060708090a0b0c0d0e0f")
SENT = 0xEE


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def u32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def sentinel(n):
    return torch.full((n,), SENT, dtype=torch.uint8, device=DEV)


def pack_cids(cids):
    """20-byte stride with junk behind each CID (the library must ignore it), and the lengths."""
    a = np.full((max(len(cids), 1), 20), 0xAA, dtype=np.uint8)
    for i, c in enumerate(cids):
        a[i, :min(len(c), 20)] = np.frombuffer(c[:20], dtype=np.uint8)
    return a[:len(cids)], np.array([len(c) for c in cids], dtype=np.uint8)


class Pair:
    """A device table and its model, driven together."""

    def __init__(self, capacity, seed=SEED):
        self.dev, self.model, self.capacity = route.CidTable(capacity, seed), TableModel(capacity), capacity

    def insert(self, cids, conns):
        a, lens = pack_cids(cids)
        st = sentinel(len(cids))
        self.dev.insert(t(a), t(lens), u32(conns), st)
        torch.cuda.synchronize()
        want = self.model.insert(cids, conns)
        assert list(st.cpu().numpy()) == want
        return want

    def remove(self, cids):
        a, lens = pack_cids(cids)
        st = sentinel(len(cids))
        self.dev.remove(t(a), t(lens), st)
        torch.cuda.synchronize()
        want = self.model.remove(cids)
        assert list(st.cpu().numpy()) == want
        return want

    def check_live(self):
        live, tomb, slots = self.dev.stats()
        assert live == len(self.model.map) and slots >= 2 * self.capacity and slots & (slots - 1) == 0
        return live, tomb, slots


def layout(blobs, last_flush=True):
    """Datagrams at byte offsets of all 16 alignments (offset of datagram i = 16-aligned + i % 16);
    with last_flush the last datagram's last byte is the arena's last byte."""
    dg = np.zeros(len(blobs), dtype=recv.DGRAM_DTYPE)
    pos, parts = 0, []
    for i, b in enumerate(blobs):
        start = (pos + 15) // 16 * 16 + i % 16
        parts.append(bytes([0x5A]) * (start - pos) + b)
        dg[i]["offset"], dg[i]["len"], dg[i]["conn"] = start, len(b), 0xABCD0000 + i
        pos = start + len(b)
    arena = np.frombuffer(b"".join(parts) + (b"" if last_flush else b"\x5A" * 7), dtype=np.uint8).copy()
    return arena, dg


def long_hdr(cid, typ=0, version=1, total=0, rng=None):
    """A long header with DCID cid (typ 0 Initial .. 2 Handshake), padded with junk to `total` bytes."""
    b = bytes([0xC0 | typ << 4 | 1]) + version.to_bytes(4, "big") + bytes([len(cid)]) + cid
    if len(b) < total:
        b += rng.bytes(total - len(b)) if rng is not None else bytes(total - len(b))
    return b


def short_hdr(cid, total=0, rng=None):
    b = bytes([0x41]) + cid
    if len(b) < total:
        b += rng.bytes(total - len(b)) if rng is not None else bytes(total - len(b))
    return b


def fill_table(pair, rng, count, sdl):
    """`count` distinct CIDs of lengths 0, 1, 8, 19, 20 and the short-header length -> conn rows."""
    cids, lens = [], [0, 1, 8, 19, 20, sdl, sdl, 8]
    seen = set(pair.model.map)
    k = 0
    while len(cids) < count:
        c = rng.bytes(lens[k % len(lens)])
        k += 1
        if c not in seen:
            seen.add(c)
            cids.append(c)
    conns = [int(x) for x in rng.integers(0, 1 << 20, size=count)]
    assert pair.insert(cids, conns) == [route.OK] * count
    return cids


def near_misses(known, table):
    """CIDs that differ from a known one in the last byte only, or in the length only."""
    out = []
    for c in known:
        if len(c):
            out.append(c[:-1] + bytes([c[-1] ^ 0x01]))
            out.append(c[:-1])
        if len(c) < 20:
            out.append(c + b"\0")
            out.append(c + c[-1:] if c else b"\x00")
    return [c for c in out if c not in table]


def malformed_blobs(sdl, rng):
    m = [b"", long_hdr(rng.bytes(8))[:5], long_hdr(rng.bytes(8))[:13], long_hdr(rng.bytes(20))[:25],
         bytes([0xC1, 0, 0, 0, 1, 21]) + rng.bytes(40), bytes([0xC1, 0, 0, 0, 1, 255]) + rng.bytes(300)]
    if sdl:
        m += [short_hdr(rng.bytes(sdl))[:sdl], bytes([0x40])]
    return m


def lookup_blobs(pair, known, n, sdl, rng):
    table = pair.model.map
    misses = near_misses(known[:40], table)
    mal = malformed_blobs(sdl, rng)
    of_sdl = [c for c in known if len(c) == sdl]
    blobs = []
    for i in range(n):
        kind = i % 7 if i < 14 else int(rng.integers(0, 7))
        total = int(rng.choice([0, 0, 17, 27, 31, 32, 33, 48, 90]))  # around the 16- and 32-byte load paths
        if kind == 0 and of_sdl:
            blobs.append(short_hdr(of_sdl[int(rng.integers(len(of_sdl)))], total, rng))
        elif kind == 1:
            blobs.append(short_hdr(rng.bytes(sdl), total, rng))
        elif kind in (2, 3):
            blobs.append(long_hdr(known[int(rng.integers(len(known)))], int(rng.integers(0, 4)), 1, total, rng))
        elif kind == 4 and misses:
            c = misses[int(rng.integers(len(misses)))]
            blobs.append(long_hdr(c, 0, 1, total, rng) if rng.random() < 0.7 or len(c) != sdl else short_hdr(c, total, rng))
        elif kind == 5:
            blobs.append(mal[int(rng.integers(len(mal)))])
        else:
            blobs.append(long_hdr(rng.bytes(int(rng.choice([0, 1, 8, 19, 20]))), 0, int(rng.integers(0, 2)), total, rng))
    return blobs


def run_route(pair, arena, dg, sdl, admit=None):
    """One device call; returns (status, conn) after checking that nothing else was written."""
    a, d, st = t(arena), t(dg), sentinel(len(dg))
    ws = None
    if admit is not None:
        ws = torch.full((route.workspace_bytes(len(dg)),), 0x3C, dtype=torch.uint8, device=DEV)  # junk: need not be initialised
    route.route(pair.dev, a, d, st, sdl, workspace=ws, admit=admit)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == arena.tobytes()  # the arena is never written
    got = d.cpu().numpy().view(recv.DGRAM_DTYPE)
    assert (got["offset"] == dg["offset"]).all() and (got["len"] == dg["len"]).all()
    return st.cpu().numpy(), got["conn"].copy()


def with_edges(arena, dg):
    """Appends a datagram that ends one byte past the arena, one far outside and one whose offset + len
    wraps around 2^64 (the last regular datagram already ends on the arena's last byte)."""
    extra = np.zeros(3, dtype=recv.DGRAM_DTYPE)
    off = max(len(arena) - 9, 0)
    extra[0] = (off, len(arena) - off + 1, 1)
    extra[1] = (len(arena) + 4096, 40, 2)
    extra[2] = ((1 << 64) - 8, 40, 3)
    return np.concatenate([dg, extra])


LOOKUP_CASES = [(1, 8, 0, 8), (63, 8, 8, 5), (64, 64, 20, 64), (65, 64, 8, 40), (257, 4096, 8, 2000),
                (5000, 4096, 20, 4096)]


@pytest.mark.parametrize("n,capacity,sdl,fill", LOOKUP_CASES)
def test_lookup_vs_model(n, capacity, sdl, fill):
    rng = np.random.default_rng(1000 + n)
    pair = Pair(capacity)
    known = fill_table(pair, rng, fill, sdl)
    blobs = lookup_blobs(pair, known, n, sdl, rng)
    if n > 1:  # the last datagram ends on the arena's last byte and needs all its bytes
        blobs[-1] = long_hdr(known[0], 2)
    arena, dg = layout(blobs)
    assert int(dg[-1]["offset"]) + int(dg[-1]["len"]) == len(arena)
    if n >= 63:
        assert len(set(int(o) % 16 for o in dg["offset"])) == 16
    dg = with_edges(arena, dg)
    before = pair.check_live()
    want_st, want_conn = pair.model.route(arena, dg, sdl)
    st, conn = run_route(pair, arena, dg, sdl)
    assert (st == want_st).all(), np.nonzero(st != want_st)[0][:10]
    assert (conn == want_conn).all(), np.nonzero(conn != want_conn)[0][:10]
    assert list(st[-3:]) == [route.MALFORMED] * 3
    if n > 1:
        assert st[n - 1] == route.HIT
    if n >= 63:
        assert {route.HIT, route.UNKNOWN, route.MALFORMED} <= set(st.tolist())
    # the table is as it was: same counters, same answers
    assert pair.check_live() == before
    st2, conn2 = run_route(pair, arena, dg, sdl)
    assert (st2 == st).all() and (conn2 == conn).all()


def admission_blobs(pair, known, n, sdl, min_len, rng):
    """1-40 distinct new DCIDs in 1-5 datagrams each at scattered positions, among hits, unknown short
    headers, Handshake packets of unknown CIDs, version-0 packets and Initials below min_len."""
    n_groups = max(1, min(40, n // 3))
    new = []
    while len(new) < n_groups:
        c = rng.bytes(int(rng.choice([0, 1, 8, 19, 20]))) if len(new) % 4 else rng.bytes(8)
        if c not in pair.model.map and c not in new:
            new.append(c)
    blobs = []
    for c in new:
        for _ in range(int(rng.integers(1, 6))):
            blobs.append(long_hdr(c, 0, int(rng.choice([1, 0x6b3343cf])), min_len + int(rng.integers(0, 60)), rng))
    blobs = blobs[:n] if len(blobs) > n else blobs
    while len(blobs) < n:
        kind = int(rng.integers(0, 6))
        if kind == 0:
            blobs.append(long_hdr(known[int(rng.integers(len(known)))], int(rng.integers(0, 4)), 1, 40, rng))
        elif kind == 1:
            blobs.append(short_hdr(rng.bytes(sdl), 40, rng))
        elif kind == 2:
            blobs.append(long_hdr(rng.bytes(8), 2, 1, min_len + 10, rng))           # Handshake, unknown CID
        elif kind == 3:
            blobs.append(long_hdr(rng.bytes(8), 0, 0, min_len + 10, rng))           # version 0
        elif kind == 4:
            blobs.append(long_hdr(rng.bytes(8), 0, 1, min_len - 1 - int(rng.integers(0, 40)), rng))  # too short
        else:
            blobs.append(malformed_blobs(sdl, rng)[int(rng.integers(0, 6))])
    order = rng.permutation(len(blobs))
    return [blobs[i] for i in order]


class DevAdmit:
    def __init__(self, n_conns, conn_base, max_new, row_first, min_len):
        self.conns = sentinel(n_conns * recv.CONN_DTYPE.itemsize)
        self.new_dcids, self.new_lens = sentinel(20 * max(max_new, 1)), sentinel(max(max_new, 1))
        self.n_new = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        self.max_new = max_new
        self.admit = route.Admit(self.conns, conn_base, max_new, row_first, self.new_dcids, self.new_lens, self.n_new,
                                 min_initial_len=min_len)
        host = np.frombuffer(bytes([SENT]) * (n_conns * recv.CONN_DTYPE.itemsize), dtype=recv.CONN_DTYPE).copy()
        self.model = AdmitModel(host, conn_base, max_new, row_first, min_len)

    def compare(self):
        m = self.model
        k = len(m.new_dcids)
        assert int(self.n_new.cpu()[0]) == k
        lens = self.new_lens.cpu().numpy()
        assert list(lens[:k]) == [len(c) for c in m.new_dcids]
        assert (lens[k:self.max_new] == 0xFF).all() and (lens[self.max_new:] == SENT).all()
        d = self.new_dcids.cpu().numpy().reshape(-1, 20)
        for i, c in enumerate(m.new_dcids):
            assert d[i].tobytes() == c + bytes(20 - len(c)), i
        assert (d[k:] == SENT).all()
        assert self.conns.cpu().numpy().tobytes() == m.conns.tobytes()  # every byte, untouched rows included


@pytest.mark.parametrize("limit", ["above", "equal", "below", "capacity"])
@pytest.mark.parametrize("n,capacity,sdl,fill", LOOKUP_CASES)
def test_admission_vs_model(n, capacity, sdl, fill, limit):
    rng = np.random.default_rng(2000 + n)
    min_len = 100
    probe = Pair(capacity)
    # how many groups the batch holds decides the fill and max_new of this case
    known = fill_table(probe, rng, min(fill, capacity // 2), sdl)
    blobs = admission_blobs(probe, known, n, sdl, min_len, rng)
    arena, dg = layout(blobs, last_flush=False)
    dg = with_edges(arena, dg)
    groups = len({route_model.route_cid(b, sdl) for b in blobs
                  if route_model.route_cid(b, sdl) is not None and route_model.route_cid(b, sdl) not in probe.model.map
                  and route_model.admissible(b, min_len)})
    assert groups >= 1
    pair = probe
    max_new = {"above": groups + 3, "equal": groups, "below": groups - 1, "capacity": groups + 3}[limit]
    if limit == "capacity":  # the capacity runs out in the middle of the batch's groups (or at once)
        room = min(groups // 2, capacity - len(pair.model.map))
        extra = capacity - len(pair.model.map) - room
        fill_table(pair, rng, extra, sdl)
        assert capacity - len(pair.model.map) == room
    n_conns, conn_base = max_new + 5, 2
    adm = DevAdmit(n_conns, conn_base, max_new, row_first=6, min_len=min_len)
    want_st, want_conn = pair.model.route(arena, dg, sdl, adm.model)
    st, conn = run_route(pair, arena, dg, sdl, adm.admit)
    assert (st == want_st).all(), (np.nonzero(st != want_st)[0][:10], st[st != want_st][:10], want_st[st != want_st][:10])
    assert (conn == want_conn).all()
    adm.compare()
    assert (st != route.DEFERRED).all()
    admitted = len(adm.model.new_dcids)
    assert admitted == min(groups, max_new, capacity - (len(pair.model.map) - admitted))
    if limit in ("below", "capacity") and groups > 1:
        assert (st == route.FULL).any()
    if admitted:
        assert (st == route.NEW).any()
    pair.check_live()
    # the same datagrams again: the admitted connections are in the table now, with the same rows
    want2, wconn2 = pair.model.route(arena, dg, sdl)
    st2, conn2 = run_route(pair, arena, dg, sdl)
    assert (st2 == want2).all() and (conn2 == wconn2).all()
    was_new = st == route.NEW
    assert (st2[was_new] == route.HIT).all() and (conn2[was_new] == conn[was_new]).all()


def test_admission_is_deterministic():
    # two tables in the same state, the same call: the same statuses, rows and new_* arrays
    outs = []
    for _ in range(2):
        r = np.random.default_rng(77)
        pair = Pair(4096)
        known = fill_table(pair, r, 500, 8)
        blobs = admission_blobs(pair, known, 2000, 8, 100, r)
        arena, dg = layout(blobs)
        adm = DevAdmit(64, 0, 30, 0, 100)
        st, conn = run_route(pair, arena, dg, 8, adm.admit)
        outs.append((st.tobytes(), conn.tobytes(), adm.new_dcids.cpu().numpy().tobytes(),
                     adm.new_lens.cpu().numpy().tobytes(), adm.conns.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_route_empty_batch_with_admit():
    # n_dgrams = 0 with admission: n_new = 0 and the 0xFF lengths are written, so the chained
    # derive_initial touches no row of a real connection
    pair = Pair(8)
    adm = DevAdmit(8, 0, 6, 0, 1200)
    none = torch.zeros(0, dtype=torch.uint8, device=DEV)
    route.route(pair.dev, none, none, none, 8, admit=adm.admit)
    route.route(pair.dev, none, none, none, 8)
    torch.cuda.synchronize()
    adm.compare()


def lookup_all(pair, cids):
    """Looks every CID up through Handshake long headers (any length) and compares with the model."""
    arena, dg = layout([long_hdr(c, 2, 1, 32) for c in cids])
    want_st, want_conn = pair.model.route(arena, dg, 8)
    st, conn = run_route(pair, arena, dg, 8)
    assert (st == want_st).all() and (conn == want_conn).all()
    return st, conn


def test_insert_remove_duplicates():
    rng = np.random.default_rng(3)
    pair = Pair(8)
    known = fill_table(pair, rng, 5, 8)
    # against the table: HIT, and the entry keeps its conn; a length over 20 is MALFORMED
    before = dict(pair.model.map)
    assert pair.insert([known[0], known[3], bytes(21)], [999, 998, 1]) == [route.HIT, route.HIT, route.MALFORMED]
    assert pair.model.map == before
    lookup_all(pair, known)
    # within one call: both entries are accepted, a lookup answers one of them
    dup = rng.bytes(8)
    a, lens = pack_cids([dup, dup])
    st = sentinel(2)
    pair.dev.insert(t(a), t(lens), u32([41, 42]), st)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [route.OK, route.OK]
    arena, dg = layout([long_hdr(dup, 2, 1, 32)])
    s, c = run_route(pair, arena, dg, 8)
    assert s[0] == route.HIT and c[0] in (41, 42)
    # one remove frees both: every lookup of it misses, the counters are the model's again
    a, lens = pack_cids([dup])
    st = sentinel(1)
    pair.dev.remove(t(a), t(lens), st)
    torch.cuda.synchronize()
    assert st.cpu().numpy()[0] == route.OK
    s, c = run_route(pair, arena, dg, 8)
    assert s[0] == route.UNKNOWN and c[0] == route.CONN_NONE
    pair.check_live()
    # FULL at capacity: three places left, five candidates -> exactly three get in (which is unspecified)
    more = [rng.bytes(int(k)) for k in (1, 19, 20, 8, 8)]
    a, lens = pack_cids(more)
    st = sentinel(5)
    pair.dev.insert(t(a), t(lens), u32([70, 71, 72, 73, 74]), st)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    assert sorted(got.tolist()) == [route.OK] * 3 + [route.FULL] * 2
    pair.model.map.update({c: 70 + i for i, c in enumerate(more) if got[i] == route.OK})
    assert pair.check_live()[0] == 8
    assert pair.insert([rng.bytes(8), known[1]], [5, 6]) == [route.FULL, route.HIT]
    lookup_all(pair, known + more + [dup])
    # removing unknown and known entries; the freed slots count at once
    assert pair.remove([rng.bytes(8), known[2], known[2][:-1]]) == [route.UNKNOWN, route.OK, route.UNKNOWN]
    assert pair.check_live()[0] == 7
    assert pair.insert([rng.bytes(8)], [5]) == [route.OK]
    lookup_all(pair, known + more)


def test_churn_with_compaction():
    # 8 x capacity entries pass through a 64-entry table (128 slots): without compaction the
    # tombstones of the removals would use up every empty slot
    rng = np.random.default_rng(4)
    capacity = 64
    pair = Pair(capacity)
    ever, compactions, inserted = [], 0, 0
    live = fill_table(pair, rng, capacity, 8)
    ever += live
    inserted += capacity
    step = 0
    while inserted < 8 * capacity:
        out = [live[i] for i in rng.permutation(len(live))[:int(rng.integers(8, 40))]]
        assert pair.remove(out) == [route.OK] * len(out)
        live = [c for c in live if c not in set(out)]
        fresh = [rng.bytes(int(rng.choice([0, 1, 8, 19, 20])) or 8) for _ in range(capacity - len(live))]
        fresh = list(dict.fromkeys(c for c in fresh if c not in pair.model.map))
        if step % 3 == 0 and ever:  # an old CID comes back
            back = ever[int(rng.integers(len(ever)))]
            if fresh and back not in pair.model.map and back not in fresh:
                fresh[0] = back
        assert pair.insert(fresh, [int(x) for x in rng.integers(0, 1 << 30, size=len(fresh))]) == [route.OK] * len(fresh)
        live += fresh
        ever += [c for c in fresh if c not in set(ever)]
        inserted += len(fresh)
        n_live, tomb, slots = pair.check_live()
        assert n_live + tomb <= slots
        if tomb > slots // 4:
            pair.dev.compact()
            compactions += 1
            n_live2, tomb2, _ = pair.check_live()
            assert tomb2 == 0 and n_live2 == n_live
        lookup_all(pair, ever)
        step += 1
    assert compactions >= 2 and len(ever) > 4 * capacity
    pair.dev.compact()
    assert pair.check_live()[1] == 0
    st, _ = lookup_all(pair, ever)
    assert (st == route.HIT).sum() == len(live)


def test_forced_collisions():
    rng = np.random.default_rng(6)
    bits, capacity, sdl, min_len = 4, 256, 8, 100
    pair = Pair(capacity)
    pair.dev.debug_hash_bits(bits)
    known = fill_table(pair, rng, 30, sdl)  # 16 hash values: long chains of colliding entries
    with pytest.raises(Exception):  # not on a table that holds entries
        pair.dev.debug_hash_bits(8)
    new = []
    while len(new) < 40:
        c = rng.bytes(8)
        if c not in pair.model.map and c not in new:
            new.append(c)
    klass = {c: route_model.hash_class(SEED, c, bits) for c in new}
    assert len(set(klass.values())) <= 16 < len(new)
    blobs = []
    for c in new:
        blobs += [long_hdr(c, 0, 1, min_len + int(rng.integers(0, 30)), rng) for _ in range(int(rng.integers(1, 4)))]
    blobs += [long_hdr(known[int(rng.integers(len(known)))], int(rng.integers(0, 4)), 1, 40, rng) for _ in range(60)]
    blobs += [short_hdr(known[int(rng.integers(len(known)))], 30, rng) for _ in range(30)]
    blobs += [short_hdr(rng.bytes(8), 30, rng) for _ in range(20)]
    blobs = [blobs[i] for i in rng.permutation(len(blobs))]
    cid_of = [route_model.route_cid(b, sdl) for b in blobs]
    arena, dg_all = layout(blobs)
    conn_base, final_conn = 0, np.full(len(blobs), route.CONN_NONE, dtype=np.uint32)
    todo = np.arange(len(blobs))
    rounds = 0
    while len(todo):
        rounds += 1
        assert rounds <= 40
        dg = dg_all[todo]
        adm = DevAdmit(64, conn_base, 64 - conn_base, row_first=0, min_len=min_len)
        model_before = copy.deepcopy(pair.model)
        st, conn = run_route(pair, arena, dg, sdl, adm.admit)
        deferred = st == route.DEFERRED
        # without the deferred datagrams, the call did what the model does on the rest
        keep = ~deferred
        want_st, want_conn = pair.model.route(arena, dg[keep], sdl, adm.model)
        assert (st[keep] == want_st).all() and (conn[keep] == want_conn).all()
        adm.compare()
        # every hash class with an admissible miss admitted exactly its first group
        first_of = {}
        for j, i in enumerate(todo):
            c = cid_of[i]
            if c in klass and c not in model_before.map:
                first_of.setdefault(klass[c], c)
        assert adm.model.new_dcids == list(first_of.values())  # in the order of their first datagrams
        for j, i in enumerate(todo):
            c = cid_of[i]
            if c in klass and c not in model_before.map:
                assert (st[j] == route.NEW) == (first_of[klass[c]] == c)
                assert (st[j] == route.DEFERRED) == (first_of[klass[c]] != c)
        if deferred.any():
            assert len(adm.model.new_dcids) >= 1
        final_conn[todo[keep]] = conn[keep]
        conn_base += len(adm.model.new_dcids)
        todo = todo[deferred]
        pair.check_live()
    assert rounds > 1  # 40 CIDs in at most 16 classes: some were deferred
    # in the end every datagram of one CID has one connection, as in the model, and no hit on the
    # colliding older entries went elsewhere
    for i, c in enumerate(cid_of):
        assert final_conn[i] == pair.model.map.get(c, route.CONN_NONE), i
    assert len({pair.model.map[c] for c in new}) == 40
    st, conn = run_route(pair, arena, dg_all, sdl)
    want_st, want_conn = pair.model.route(arena, dg_all, sdl)
    assert (st == want_st).all() and (conn == want_conn).all()


def place(order):
    """(blob) list -> arena with some unaligned datagrams and slack behind, datagram records."""
    dg = np.zeros(len(order), dtype=recv.DGRAM_DTYPE)
    pos, parts = 0, []
    for i, b in enumerate(order):
        start = (pos + 7) // 8 * 8 if i % 3 else pos
        parts.append(bytes(start - pos) + b)
        dg[i]["offset"], dg[i]["len"], dg[i]["conn"] = start, len(b), 0x7777
        pos = start + len(b)
    return np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8).copy(), dg


def test_chain_route_derive_recv_without_readback(orc):
    AES, CHACHA = _lib.MQ_SUITE_AES128GCM, _lib.MQ_SUITE_CHACHA20
    rng = np.random.default_rng(8)
    n_cl, max_new, sdl, row_first = 12, 16, 8, 0
    n_rows = 2 * max_new + n_cl
    dcids = [rng.bytes(int(rng.integers(8, 21))) for _ in range(n_cl)]
    queues = []
    for c, dcid in enumerate(dcids):
        client, _ = derive_initial_secrets(dcid)
        ck = [key_material(AES, client)]
        queues.append([protect_one(orc, ck, dcid, 0, 0, 0, pn, max(pn - 1, 0), rng.bytes(int(rng.integers(30, 300))), True)
                       for pn in (0, 1)])
    order, idx = [], [0] * n_cl
    while any(idx[c] < 2 for c in range(n_cl)):
        c = int(rng.choice([k for k in range(n_cl) if idx[k] < 2]))
        order.append(queues[c][idx[c]])
        idx[c] += 1
    bad = bytearray(queues[3][1])
    bad[-20] ^= 0x10
    order.insert(9, bytes(bad))                                  # a tampered copy: routed, fails to open
    order.insert(4, bytes([0x41]) + rng.bytes(8) + rng.bytes(40))  # a short header nobody knows
    assert all(len(b) >= 1200 for b in order if b[0] & 0x80)
    arena, dg = place(order)

    pair = Pair(64)
    kt = KeyTable([_lib.KeyMaterial() for _ in range(n_rows)])
    n_conns = max_new
    d_conns = torch.zeros(n_conns * recv.CONN_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    new_dcids, new_lens = sentinel(20 * max_new), sentinel(max_new)
    n_new = torch.zeros(1, dtype=torch.int32, device=DEV)
    admit = route.Admit(d_conns, 0, max_new, row_first, new_dcids, new_lens, n_new)  # min_initial_len 1200
    a, d_dg, st = t(arena), t(dg), sentinel(len(dg))
    ws_r = torch.empty(route.workspace_bytes(len(dg)), dtype=torch.uint8, device=DEV)
    d_st = sentinel(max_new)
    max_pkts = len(dg) + 8
    pk = torch.zeros(max_pkts * recv.PKT_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(recv.workspace_bytes(len(dg), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    # one stream, nothing synchronised or read back in between
    route.route(pair.dev, a, d_dg, st, sdl, workspace=ws_r, admit=admit)
    batch.derive_initial(kt, row_first, new_dcids, new_lens, d_st)
    recv.recv(kt, d_conns, a, d_dg, pk, cnt, ws)
    torch.cuda.synchronize()

    # the model's rows and host-derived keys for the oracle
    h_conns = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
    adm = AdmitModel(h_conns, 0, max_new, row_first, 1200)
    want_st, want_conn = pair.model.route(arena, dg, sdl, adm)
    assert (st.cpu().numpy() == want_st).all()
    assert sorted(adm.new_dcids) == sorted(dcids) and (want_st == route.NEW).sum() == 2 * n_cl + 1
    assert list(d_st.cpu().numpy()) == [0] * n_cl + [_lib.MQ_ERR_INVALID_ARG] * (max_new - n_cl)
    keys = [_lib.KeyMaterial() for _ in range(n_rows)]
    for k, dcid in enumerate(adm.new_dcids):
        client, server = derive_initial_secrets(dcid)
        keys[row_first + 2 * k], keys[row_first + 2 * k + 1] = key_material(AES, client), key_material(AES, server)
    h_dg = dg.copy()
    h_dg["conn"] = want_conn
    oa = arena.copy()
    o_pk, o_n = orc.batch_recv(keys, h_conns, oa, h_dg, max_pkts)

    def compare(k):
        assert int(cnt.cpu()[0]) == o_n
        g_pk = pk.cpu().numpy().view(recv.PKT_DTYPE)[:o_n]
        for f in recv.PKT_DTYPE.names:
            assert (g_pk[f] == o_pk[f]).all(), (k, f)
        assert d_dg.cpu().numpy().tobytes() == h_dg.tobytes()
        assert d_conns.cpu().numpy().tobytes() == h_conns.tobytes()
        assert a.cpu().numpy().tobytes() == oa.tobytes()
    compare(0)
    assert (o_pk["status"] == 0).sum() == 2 * n_cl and (o_pk["status"] != 0).sum() == 1
    assert (h_conns["largest_pn"][:n_cl, 0] == 1).all()

    # ---- the handshakes finish: one server-issued 8-byte CID and 1-RTT keys per connection --------
    issued = [rng.bytes(8) for _ in range(n_cl)]
    assert pair.insert(issued, list(range(n_cl))) == [route.OK] * n_cl
    suites = rng.choice([AES, CHACHA], size=n_cl)
    secrets = rng.integers(0, 256, size=(n_cl, 32), dtype=np.uint8)
    app_rows = 2 * max_new + np.arange(n_cl, dtype=np.uint32)
    for suite in (AES, CHACHA):
        sel = np.nonzero(suites == suite)[0]
        s1 = sentinel(len(sel))
        batch.derive_keys(kt, int(suite), t(secrets[sel]), s1, row_idx=u32(app_rows[sel]))
        torch.cuda.synchronize()
        assert (s1.cpu().numpy() == 0).all()
    for c in range(n_cl):
        keys[int(app_rows[c])] = key_material(int(suites[c]), secrets[c].tobytes())
    h_conns["app_row"][:n_cl, 1] = app_rows
    h_conns["flags"][:n_cl] |= recv.HAS_APP
    d_conns.copy_(t(h_conns))
    order = []
    for pn in (0, 1, 2):
        for c in rng.permutation(n_cl):
            order.append(protect_one(orc, keys, issued[c], 2, int(app_rows[c]), 0, pn, max(pn - 1, 0),
                                     rng.bytes(int(rng.integers(1, 300))), False))
    order.insert(5, bytes([0x41]) + rng.bytes(60))
    arena, dg = place(order)
    a, d_dg, st = t(arena), t(dg), sentinel(len(dg))
    max_pkts = len(dg) + 8
    pk = torch.zeros(max_pkts * recv.PKT_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    ws = torch.empty(recv.workspace_bytes(len(dg), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    route.route(pair.dev, a, d_dg, st, sdl)
    recv.recv(kt, d_conns, a, d_dg, pk, cnt, ws)
    torch.cuda.synchronize()
    want_st, want_conn = pair.model.route(arena, dg, sdl)
    assert (st.cpu().numpy() == want_st).all() and (want_st == route.HIT).sum() == 3 * n_cl
    h_dg = dg.copy()
    h_dg["conn"] = want_conn
    oa = arena.copy()
    o_pk, o_n = orc.batch_recv(keys, h_conns, oa, h_dg, max_pkts)
    compare(1)
    assert (o_pk["status"] == 0).sum() == 3 * n_cl
