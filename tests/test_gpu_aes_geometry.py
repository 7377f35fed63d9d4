"""The AES-128-GCM geometry ladder (tests/aes_geometry.py) through every AES tile kernel, against the
oracle on every arena byte, status and packet number: the flat single-key kernels at 8, 4 and 2 lanes
per packet, the flat multi-key kernel on key-uniform and mixed tiles, the partition with the hot
key's segment on the slice kernel or the tile kernel, and the key-segmented kernels forced over
tables whose rows hold no packets, one packet, or more than a slice. Every case asserts the path it
means to run (batch.aes_list_kind, the decision mq_batch_seal / mq_batch_open make). A tamper ladder
flips one bit in every header byte class, AAD block edge, payload edge and tag edge of every header
geometry. Statuses start as 0xEE, so a packet that no kernel touched fails its comparison.
Reference: rustcrypto.rs:38-94, :175-186; transmit.rs:625-755; recv.rs:340-421; number.rs:52-70;
tcp_tls/record.rs:88-143."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import aes_geometry as ag  # noqa: E402
from milli_quic_amd import _lib, batch  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AES, MIXED = _lib.MQ_SUITE_AES128GCM, _lib.MQ_SUITE_MIXED
NARROW_LANES = {None: None, "0": 8, "1": 4, "2": 2}


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def opt(name, v):
    return _lib.option(name, v)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def gpu_run(kt, arena, desc, open_, use_ws, hint):
    n = len(desc)
    a, d = to_dev(arena), to_dev(desc)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    pn = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.full((max(batch.workspace_bytes(n), 256),), 0xA5, dtype=torch.uint8, device=DEV) if use_ws else None
    if open_:  # mq_batch_open, then the inner content types of the batch's TLS records
        batch.open_records(kt, a, d, st, pn, hint, ws)
    else:
        batch.seal(kt, a, d, st, hint, ws)
    torch.cuda.synchronize()
    return a.cpu().numpy(), st.cpu().numpy(), pn.cpu().numpy().view(np.uint64)


class Ref:
    """A batch with the oracle's seal and open of it (computed once, never written again) and its
    device key table."""

    def __init__(self, orc, b, tamper=None):
        self.b = b
        self.sealed = b.arena.copy()
        self.seal_st = orc.batch_seal(b.keys, self.sealed, b.sd, AES, threads=8)
        assert (self.seal_st == 0).all()
        self.wire = self.sealed.copy()  # what open is given
        if tamper is not None:
            tamper(self.wire)
        self.opened = self.wire.copy()
        self.open_st, self.pn = orc.batch_open(b.keys, self.opened, b.od, AES, threads=8)
        self.ok = self.open_st == 0
        if tamper is None:
            assert self.ok.all() and (self.pn == b.pns).all()
        for a in (self.sealed, self.wire, self.opened, self.seal_st, self.open_st, self.pn, b.arena):
            a.setflags(write=False)
        self.kt = KeyTable(b.keys)

    def check(self, hint, use_ws, what, seal=True):
        b = self.b
        if seal:
            out, st, _ = gpu_run(self.kt, b.arena, b.sd, False, use_ws, hint)
            assert (st == self.seal_st).all(), (what, "seal status", np.nonzero(st != self.seal_st)[0][:8])
            self.same_bytes(out, self.sealed, (what, "seal"))
        back, st, pn = gpu_run(self.kt, self.wire, b.od, True, use_ws, hint)
        assert (st == self.open_st).all(), (what, "open status", np.nonzero(st != self.open_st)[0][:8])
        self.same_bytes(back, self.opened, (what, "open"))
        assert (pn[self.ok] == self.pn[self.ok]).all(), (what, "pn", np.nonzero(pn != self.pn)[0][:8])

    def same_bytes(self, got, want, what):
        if got.tobytes() == want.tobytes():
            return
        at = int(np.nonzero(got != want)[0][0])
        i = int(np.searchsorted(self.b.sd["offset"], at, side="right")) - 1
        raise AssertionError((what, "first differing byte", at, "packet", i, self.b.rows[max(i, 0)],
                              "at packet byte", at - int(self.b.sd["offset"][max(i, 0)])))


def shuffled(n, seed=7):
    return [int(x) for x in np.random.default_rng(seed).permutation(n)]


@functools.lru_cache(maxsize=None)
def ladder_rows():
    return ag.ladder()


_refs = {}


def ref_of(orc, name, make):
    if name not in _refs:
        _refs[name] = Ref(orc, make())
    return _refs[name]


def expect_kind(n, n_rows, kind, lanes):
    assert batch.aes_list_kind(n, n_rows) == (kind, lanes), (batch.aes_list_kind(n, n_rows), kind, lanes)


# ---- flat, one row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ladder", "shuffled"])
@pytest.mark.parametrize("lead", [0, 5, 13])
@pytest.mark.parametrize("narrow", [None, "0", "1", "2"])
def test_flat_single_key(orc, narrow, lead, order):
    rows = ladder_rows()
    perm = shuffled(len(rows)) if order == "shuffled" else None
    r = ref_of(orc, ("flat1", lead, order), lambda: ag.build(rows, lead=lead, order=perm, seed=3 + lead))
    n = len(rows)
    with opt("MQ_AES_NARROW", narrow):
        lanes = NARROW_LANES[narrow]
        expect_kind(n, 1, batch.AES_FLAT_SINGLE, lanes or 0)
        # unset: the ladder's ~220 B per packet pick 2 lanes per packet
        assert batch.aes_flat_kind(len(r.b.arena), n, AES) == (lanes or 2)
        for use_ws in (True, False):  # open: the pre-pass's header values, or HP removal in the tile
            r.check(AES, use_ws, (narrow, lead, order, use_ws))


# ---- flat, several rows, no workspace: the multi-key kernel ---------------------------------------------
K_FLAT = 3


def key_uniform(i):
    return (i // 8) % K_FLAT


def key_mixed(i):
    return i % K_FLAT


@pytest.mark.parametrize("keying", ["uniform_tiles", "mixed_tiles"])
@pytest.mark.parametrize("order", ["ladder", "shuffled"])
def test_flat_multi_key(orc, keying, order):
    # without a workspace there are no partition lists: the batch runs the multi-key kernel in
    # descriptor order, tiles of 8 — all of one row (kGhWave) or of three (kGhProduct)
    rows = ladder_rows()
    perm = shuffled(len(rows), 11) if order == "shuffled" else None
    key_of = key_uniform if keying == "uniform_tiles" else key_mixed
    r = ref_of(orc, ("flatK", keying, order),
               lambda: ag.build(rows, key_of=key_of, n_keys=K_FLAT, lead=5, order=perm, seed=21))
    # the flat multi-key launch is the path of every AES-hinted batch over several rows that brings no
    # workspace (include/mq_aead.h); with one, this batch would go through the partition
    assert batch.aes_list_kind(len(rows), K_FLAT)[0] in (batch.AES_PARTITION_HOT, batch.AES_KEY_SEGMENTS)
    r.check(AES, False, (keying, order))


def key_pattern(i):
    # tiles of 8 in turn: all row 0, mixed rows, all row 0, all row 1, all row 0 — the wave's cached
    # row (wt_kid) is kept, dropped by a mixed tile, rebuilt for the same row, replaced, restored
    return (0, i % 3, 0, 1, 0)[(i // 8) % 5]


def test_flat_multi_key_row_cache_over_many_tiles(orc):
    short = ag.shortest(ladder_rows())
    rows = (short * (30000 // len(short) + 1))[:30000]
    assert len(rows) // 8 > 3072  # more tiles than the grid has waves: waves walk several tiles
    r = ref_of(orc, "pattern", lambda: ag.build(rows, key_of=key_pattern, n_keys=3, seed=31))
    assert max(r.b.sd["len"]) <= 64
    r.check(AES, False, "pattern")


# ---- partition: the hot key's segment beside the multi-key kernel -----------------------------------------
def hot_keys(K):
    return lambda i: 0 if (i * 7919) % 10 < 6 else 1 + i % (K - 1)


@pytest.mark.parametrize("hint", [AES, MIXED])
@pytest.mark.parametrize("K", [3, 16])
def test_partition_hot_split(orc, K, hint):
    rows = ladder_rows()
    r = ref_of(orc, ("part", K), lambda: ag.build(rows, key_of=hot_keys(K), n_keys=K, lead=13,
                                                  order=shuffled(len(rows), 5), seed=41))
    share = (r.b.sd["key_id"] == 0).mean()
    assert 0.55 < share < 0.65
    n = len(rows)
    # by itself a batch of this size (512 packets per row or more) takes the key segments: once as
    # the product chooses, then the hot split with the segments switched off
    assert n >= 512 * K
    expect_kind(n, K, batch.AES_KEY_SEGMENTS, 4)
    r.check(hint, True, (K, hint, "product"))
    for hot_seg in (None, "0"):  # the hot segment on the slice kernel, or on the single-key tile kernel
        for narrow in (None, "0", "1", "2"):
            with opt("MQ_AES_SEG", "0"), opt("MQ_AES_HOT_SEG", hot_seg), opt("MQ_AES_NARROW", narrow):
                expect_kind(n, K, batch.AES_PARTITION_HOT, NARROW_LANES[narrow] or 4)
                r.check(hint, True, (K, hint, hot_seg, narrow))


# ---- forced key segments -------------------------------------------------------------------------------
def seg_keys(n, R):
    """key_of for n packets over R rows: rows without packets (the first, the last, two adjacent
    ones), rows with exactly one packet, one row with 40 % of the batch (more than 128 tiles of 8: its
    segment crosses slices), the rest spread over the other rows."""
    if R == 3:
        empty, single, big = {0}, {2: n // 2}, 1
    else:
        empty, single, big = {0, R - 1, 10, 11}, {1: 3, 12: n // 3, R - 2: n - 2}, 5
    others = [r for r in range(R) if r not in empty and r not in single and r != big]
    at = {i: r for r, i in single.items()}

    def key_of(i):
        if i in at:
            return at[i]
        if not others or (i * 7919) % 10 < 4:
            return big
        return others[i % len(others)]
    return key_of, empty, set(single), big


@pytest.mark.parametrize("R", [3, 63, 64, 65, 4096])
def test_forced_key_segments(orc, R):
    rows = ladder_rows()
    if R == 4096:  # the keyed layout needs room for 7 holes per row in the list: ~44 000 packets
        short = ag.shortest(rows)
        rows = (short * (46000 // len(short) + 1))[:46000]
    n = len(rows)
    key_of, empty, single, big = seg_keys(n, R)
    r = ref_of(orc, ("seg", R), lambda: ag.build(rows, key_of=key_of, n_keys=R, lead=5,
                                                 order=shuffled(n, 9) if R != 4096 else None, seed=51))
    per_row = np.bincount(r.b.sd["key_id"], minlength=R)
    assert all(per_row[q] == 0 for q in empty) and all(per_row[q] == 1 for q in single)
    assert per_row[big] > 128 * 8
    if n < 512 * R:  # too few packets per row for the segments by themselves
        expect_kind(n, R, batch.AES_PARTITION_HOT, 4)
    for narrow in ("0", "1", "2"):
        with opt("MQ_AES_SEG", "1"), opt("MQ_AES_NARROW", narrow):
            expect_kind(n, R, batch.AES_KEY_SEGMENTS, NARROW_LANES[narrow])
            r.check(AES, True, (R, narrow))
    with opt("MQ_AES_SEG", "0"):
        expect_kind(n, R, batch.AES_PARTITION_HOT, 4)


# ---- tamper ladder -------------------------------------------------------------------------------------
def flips_of(o, pl, f, P):
    """(packet byte, bit) of every single-bit tamper of a sealed packet with this geometry."""
    aad, n = o + pl, o + pl + P + 16
    out = []
    if ag.is_hp(f):
        out += [(0, 0x04), (0, 0x01), (0, 0x20)]  # protected (reserved / key phase, pn_len), unprotected
    out += [(o + q, 0x10) for q in range(pl)]
    for blk in range((aad + 15) >> 4):
        out += [(16 * blk, 0x80), (min(16 * blk + 15, aad - 1), 0x02)]
    if P:
        out += [(aad, 0x01), (aad + P - 1, 0x40)]
    out += [(n - 16, 0x08), (n - 1, 0x80)]
    return sorted(set(out))


def tamper_batch():
    rows = ag.ladder(ctr_edge=False)
    victims = [rows[i] for i in ag.one_per_geometry(rows)]
    assert {v[:3] for v in victims} == set(ag.HEADERS)
    out, flips, k = [], {}, 0
    for v in victims:  # one copy of the packet per flip, two good packets after each
        for fl in flips_of(*v):
            flips[len(out)] = fl
            out += [v, rows[k % len(rows)], rows[(k + 1) % len(rows)]]
            k += 2
    return out, flips


@pytest.fixture(scope="module")
def tampered(orc):
    rows, flips = tamper_batch()

    def make(key_of, n_keys):
        b = ag.build(rows, key_of=key_of, n_keys=n_keys, lead=5, seed=61)

        def tamper(wire):
            for i, (at, bit) in flips.items():
                wire[int(b.sd["offset"][i]) + at] ^= bit
        r = Ref(orc, b, tamper)
        bad = np.zeros(len(rows), dtype=bool)
        bad[list(flips)] = True
        # every flip fails its packet and no other; a failed packet keeps its bytes, header still masked
        assert (r.open_st[bad] != 0).all() and (r.open_st[~bad] == 0).all()
        assert (r.open_st[bad] == _lib.MQ_ERR_CRYPTO).mean() > 0.95
        for i in list(flips)[::37]:
            o, n = int(b.sd["offset"][i]), int(b.sd["len"][i])
            assert r.opened[o:o + n].tobytes() == r.wire[o:o + n].tobytes()
        return r
    return make


@pytest.fixture(scope="module")
def tampered_single_key(tampered):
    return tampered(lambda i: 0, 1)


@pytest.mark.parametrize("narrow", ["0", "1", "2"])
def test_tamper_flat_single_key(tampered_single_key, narrow):
    r = tampered_single_key
    with opt("MQ_AES_NARROW", narrow):
        expect_kind(len(r.b.sd), 1, batch.AES_FLAT_SINGLE, NARROW_LANES[narrow])
        for use_ws in (True, False):
            r.check(AES, use_ws, ("tamper", narrow, use_ws), seal=False)


def test_tamper_flat_multi_key_mixed_tiles(tampered):
    r = tampered(key_mixed, K_FLAT)
    r.check(AES, False, "tamper mixed", seal=False)


def test_tamper_forced_key_segments(tampered):
    R = 5
    r = tampered(lambda i: (1, 3, 1, 4, 1, 3)[i % 6], R)  # rows 0 and 2 without packets
    for narrow in ("0", "1", "2"):
        with opt("MQ_AES_SEG", "1"), opt("MQ_AES_NARROW", narrow):
            expect_kind(len(r.b.sd), R, batch.AES_KEY_SEGMENTS, NARROW_LANES[narrow])
            r.check(AES, True, ("tamper segments", narrow), seal=False)
