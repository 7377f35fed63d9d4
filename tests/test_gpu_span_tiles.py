"""Span tiles of the ChaCha20-Poly1305 octet kernels (mq_chacha.hip chacha_tile, mq_tile.h DmaStager /
stage_out_span) against the oracle, byte for byte: a tile of eight 16-B-aligned packets packed back
to back, whose images need no gaps, is staged and stored as one linear copy. Every batch runs
with the switch unset and with MQ_CC_SPAN=0 (the per-packet copies); both must give the oracle's
arena, statuses and packet numbers. Batches are workload.uniform ones (L-byte short-header packets
at offsets i * L, the arena exactly n * L bytes), bent where a tile has to fall back: a gap, a
misaligned lead, descriptors in reverse order, an invalid descriptor inside a tile, a packet that
fails to open inside a span (never stored, header still protected).
Image sizes by packet length (mq_chacha_flat_kind): 656 / 672 / 1200 B run the 10-KiB kernels, 1232 B
the 13-KiB ones, 1616 B the 20-KiB ones; 672 B is 42 chunks, an even count, so its images get
the bank-stagger gaps and the tile is no span.
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHACHA = _lib.MQ_SUITE_CHACHA20
MODES = (None, "0")  # MQ_CC_SPAN unset (span tiles) and 0 (never)


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def _span(v):
    """MQ_CC_SPAN for the calls inside the block (mq_debug_option; None: the product choice)."""
    return _lib.option("MQ_CC_SPAN", v)


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


def check_both_modes(orc, keys, arena, sd, od):
    """Seal `arena`, then open the oracle's sealed arena, under every mode: arena, statuses and the
    packet numbers of opened packets equal the oracle's (and so each other's). Returns the oracle's
    (sealed arena, seal statuses, opened arena, open statuses, packet numbers)."""
    o_out, o_st, _ = oracle_run(orc, keys, arena, sd)
    o_back, o_st2, o_pn = oracle_run(orc, keys, o_out, od, open_=True)
    ok = o_st2 == 0
    outs = []
    for mode in MODES:
        with _span(mode):
            g_out, g_st, _ = gpu_run(keys, arena, sd)
            assert (g_st == o_st).all(), (mode, np.nonzero(g_st != o_st)[0][:8])
            assert g_out.tobytes() == o_out.tobytes(), mode
            g_back, g_st2, g_pn = gpu_run(keys, o_out, od, open_=True)
            assert (g_st2 == o_st2).all(), (mode, np.nonzero(g_st2 != o_st2)[0][:8])
            assert g_back.tobytes() == o_back.tobytes(), mode
            assert (g_pn[ok] == o_pn[ok]).all(), mode
            outs.append((g_out, g_st, g_back, g_st2, g_pn[ok]))
    for x, y in zip(outs[0], outs[1]):
        assert x.tobytes() == y.tobytes()
    return o_out, o_st, o_back, o_st2, o_pn


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("L,kind", [(656, 1), (1200, 1), (672, 1), (1232, 2), (1616, 3)])
def test_span_round_trip_shapes(orc, L, kind, n_keys):
    # 8: one tile; 32: one workgroup; 33: a one-packet last tile (no span: seven lanes' packets are
    # missing); 71: a partial last tile and a partial last workgroup
    for n in (8, 32, 33, 71):
        for pn_len in (1, 2, 3, 4):
            w = workload.uniform(n, CHACHA, L=L, pn_len=pn_len, n_keys=n_keys)
            assert len(w.arena) == n * L
            assert batch.flat_kind(len(w.arena), n, CHACHA) == kind
            _, o_st, _, o_st2, o_pn = check_both_modes(orc, w.keys, w.arena, w.seal_desc, w.open_desc)
            assert (o_st == 0).all() and (o_st2 == 0).all() and (o_pn == w.pns).all()


def _shifted(w, shift):
    """The batch with packet i moved up by shift[i] bytes; bytes between packets are 0x5A."""
    L = int(w.seal_desc["len"][0])
    offs = w.seal_desc["offset"].astype(np.int64) + shift
    arena = np.full(int(offs[-1]) + L, 0x5A, np.uint8)
    for i, o in enumerate(offs):
        arena[o:o + L] = w.arena[i * L:(i + 1) * L]
    sd, od = w.seal_desc.copy(), w.open_desc.copy()
    sd["offset"] = offs
    od["offset"] = offs
    return arena, sd, od


@pytest.mark.parametrize("n_keys", [1, 3])
def test_gap_inside_a_tile(orc, n_keys):
    # a 16-B gap after packet 3 of the second tile: that tile falls back, the tiles around it are
    # spans (every offset is still a multiple of 16); the gap keeps its bytes
    w = workload.uniform(71, CHACHA, L=1200, n_keys=n_keys)
    shift = np.where(np.arange(71) > 11, 16, 0)
    arena, sd, od = _shifted(w, shift)
    gap = 12 * 1200
    o_out, o_st, o_back, o_st2, _ = check_both_modes(orc, w.keys, arena, sd, od)
    assert (o_st == 0).all() and (o_st2 == 0).all()
    assert (o_out[gap:gap + 16] == 0x5A).all() and (o_back[gap:gap + 16] == 0x5A).all()


@pytest.mark.parametrize("L", [656, 1200])
def test_misaligned_lead(orc, L):
    # 5 bytes before the first packet: every packet starts 5 bytes into a chunk, no tile is a span
    w = workload.uniform(33, CHACHA, L=L, pn_len=2)
    arena, sd, od = _shifted(w, np.full(33, 5))
    o_out, o_st, o_back, o_st2, _ = check_both_modes(orc, w.keys, arena, sd, od)
    assert (o_st == 0).all() and (o_st2 == 0).all()
    assert (o_out[:5] == 0x5A).all() and (o_back[:5] == 0x5A).all()


@pytest.mark.parametrize("n_keys", [1, 3])
def test_descriptors_in_reverse_order(orc, n_keys):
    # the second tile's descriptors reversed: the same eight packets, but packet p does not follow
    # packet p - 1 in the arena, so the tile's LDS order is not the arena's
    w = workload.uniform(32, CHACHA, L=1200, pn_len=3, n_keys=n_keys)
    sd, od = w.seal_desc.copy(), w.open_desc.copy()
    sd[8:16] = sd[8:16][::-1].copy()
    od[8:16] = od[8:16][::-1].copy()
    _, o_st, _, o_st2, o_pn = check_both_modes(orc, w.keys, w.arena, sd, od)
    assert (o_st == 0).all() and (o_st2 == 0).all()
    assert (o_pn[8:16] == w.pns[8:16][::-1]).all()


@pytest.mark.parametrize("n_keys", [1, 3])
def test_invalid_descriptor_inside_a_tile(orc, n_keys):
    # key_id == n_rows in the middle of an otherwise contiguous tile: that packet is refused and
    # keeps its bytes, the other seven (and the span tiles around) match the oracle
    w = workload.uniform(32, CHACHA, L=1200, n_keys=n_keys)
    bad, L = 12, 1200
    sd, od = w.seal_desc.copy(), w.open_desc.copy()
    sd["key_id"][bad] = n_keys
    od["key_id"][bad] = n_keys
    o_out, o_st, o_back, o_st2, _ = check_both_modes(orc, w.keys, w.arena, sd, od)
    good = np.arange(32) != bad
    assert o_st[bad] == _lib.MQ_ERR_INVALID_ARG and o_st2[bad] == _lib.MQ_ERR_INVALID_ARG
    assert (o_st[good] == 0).all() and (o_st2[good] == 0).all()
    assert o_out[bad * L:(bad + 1) * L].tobytes() == w.arena[bad * L:(bad + 1) * L].tobytes()
    assert o_back[bad * L:(bad + 1) * L].tobytes() == w.arena[bad * L:(bad + 1) * L].tobytes()


@pytest.mark.parametrize("L", [656, 1200, 1232])
@pytest.mark.parametrize("tampered", [(12,), (4, 20)])
def test_open_failure_inside_a_span(orc, L, tampered):
    # one flipped tag bit in one packet in the middle of a contiguous tile, or in one packet in each
    # of two tiles of a workgroup: the packet keeps every received byte (header still protected),
    # its tile is stored packet by packet, everything else opens as the oracle's does
    w = workload.uniform(40, CHACHA, L=L)
    sealed, st, _ = oracle_run(orc, w.keys, w.arena, w.seal_desc)
    assert (st == 0).all()
    bad = sealed.copy()
    for t in tampered:
        bad[(t + 1) * L - 1 - (t % 16)] ^= 1 << (t % 8)
    o_back, o_st, o_pn = oracle_run(orc, w.keys, bad, w.open_desc, open_=True)
    hit = np.isin(np.arange(40), tampered)
    assert (o_st[hit] == _lib.MQ_ERR_CRYPTO).all() and (o_st[~hit] == 0).all()
    for mode in MODES:
        with _span(mode):
            g_back, g_st, g_pn = gpu_run(w.keys, bad, w.open_desc, open_=True)
            assert (g_st == o_st).all(), mode
            assert g_back.tobytes() == o_back.tobytes(), mode
            assert (g_pn[~hit] == o_pn[~hit]).all() and (g_pn[~hit] == w.pns[~hit]).all(), mode
            for t in tampered:
                assert g_back[t * L:(t + 1) * L].tobytes() == bad[t * L:(t + 1) * L].tobytes(), (mode, t)
