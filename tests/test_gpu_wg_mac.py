"""The workgroup MAC phase of the flat ChaCha20-Poly1305 octet kernels (mq_chacha.hip cc_wg_mac: the
Poly1305 of a workgroup's 32 packets on two of its four waves, four lanes per packet, between two
barriers; the waves' roles rotated with the block index, cc_role) against the oracle, byte for byte. Every batch
is sealed, and the oracle's sealed arena opened, with MQ_CC_WGMAC unset (the phase) and at 0 (the
per-wave MAC in the same kernels): arena, statuses and packet numbers equal the oracle's in each.
Shapes: workgroups with 1-4 live waves at every block index up to 7 and at blocks 256, 512 and 768
(open rotates its roles by block >> 8: MAC roles land on dead waves under every rotation), lengths that give the 16 packets of a MAC wave different step counts,
a tampered packet in each of a workgroup's 32 positions, a direct-path tile beside staged ones,
payloads so short that the header-protection sample reaches into the tag (the mask is made after
the MAC's barrier), rows without header protection, invalid descriptors inside a workgroup.
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, workload  # noqa: E402

from test_gpu_chacha_xor_edges import HDR, Batch, first_diff, gpu_run, oracle_run  # noqa: E402

pytestmark = pytest.mark.gpu
CHACHA = _lib.MQ_SUITE_CHACHA20
MODES = (None, "0")  # MQ_CC_WGMAC unset (the workgroup phase) and 0 (the per-wave MAC)
L = 1200
LADDER_MAX = 32 * 7 + 8 * 3 + 7


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def _wgmac(v):
    return _lib.option("MQ_CC_WGMAC", v)


# ---- live and dead waves under every rotation ---------------------------------------------------
_LADDER = {}


def ladder_ref(orc, n_keys):
    """The largest batch of the ladder, sealed and opened by the oracle once: a batch of n packets is
    its first n (packets are independent, offsets i * L)."""
    if n_keys not in _LADDER:
        w = workload.uniform(LADDER_MAX, CHACHA, L=L, pn_len=2, n_keys=n_keys)
        sealed, st, _ = oracle_run(orc, w.keys, w.arena, w.seal_desc)
        back, st2, pn = oracle_run(orc, w.keys, sealed, w.open_desc, open_=True)
        assert (st == 0).all() and (st2 == 0).all() and (pn == w.pns).all()
        _LADDER[n_keys] = (w, sealed, back)
    return _LADDER[n_keys]


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("b", range(8))
def test_live_and_dead_waves(orc, b, n_keys):
    # n = 32 b + 8 k + r: b whole workgroups, then one with k whole tiles and a tile of r packets
    w, sealed, back = ladder_ref(orc, n_keys)
    for k in range(4):
        for r in (0, 1, 7):
            n = 32 * b + 8 * k + r
            if n == 0:
                continue
            plain, rx = w.arena[:n * L], sealed[:n * L]
            for mode in MODES:
                with _wgmac(mode):
                    g_out, g_st, _ = gpu_run(w.keys, plain, w.seal_desc[:n])
                    assert (g_st == 0).all(), (n, mode, np.nonzero(g_st)[0][:8])
                    assert g_out.tobytes() == rx.tobytes(), (n, mode)
                    g_back, g_st2, g_pn = gpu_run(w.keys, rx, w.open_desc[:n], open_=True)
                    assert (g_st2 == 0).all(), (n, mode, np.nonzero(g_st2)[0][:8])
                    assert g_back.tobytes() == back[:n * L].tobytes(), (n, mode)
                    assert (g_pn == w.pns[:n]).all(), (n, mode)


@pytest.mark.parametrize("h", [1, 2, 3])
def test_rotated_roles(orc, h):
    # blocks 256 h and up: the rotations open takes there (role = (w + (block >> 8)) & 3). The last
    # workgroup is block 256 h, with 1-4 live waves; one batch has a tampered packet per MAC wave in
    # that block and in the block before it
    b = 256 * h
    nmax = 32 * b + 8 * 3 + 7
    w = workload.uniform(nmax, CHACHA, L=L, pn_len=4)
    sealed, st, _ = oracle_run(orc, w.keys, w.arena, w.seal_desc)
    back, st2, pn = oracle_run(orc, w.keys, sealed, w.open_desc, open_=True)
    assert (st == 0).all() and (st2 == 0).all() and (pn == w.pns).all()
    bad = sealed.copy()
    hit = np.array([32 * b - 32 + 3, 32 * b - 32 + 29, 32 * b + 9, 32 * b + 30])
    for t in hit:
        bad[(t + 1) * L - 1 - int(t % 16)] ^= 1 << int(t % 8)
    bad_back, bad_st, bad_pn = oracle_run(orc, w.keys, bad, w.open_desc, open_=True)
    ok = ~np.isin(np.arange(nmax), hit)
    assert (bad_st[~ok] == _lib.MQ_ERR_CRYPTO).all() and (bad_st[ok] == 0).all()
    for mode in MODES:
        with _wgmac(mode):
            for n in (32 * b + 1, 32 * b + 8 + 7, 32 * b + 16, nmax):
                g_out, g_st, _ = gpu_run(w.keys, w.arena[:n * L], w.seal_desc[:n])
                assert (g_st == 0).all(), (n, mode)
                assert g_out.tobytes() == sealed[:n * L].tobytes(), (n, mode)
                g_back, g_st2, g_pn = gpu_run(w.keys, sealed[:n * L], w.open_desc[:n], open_=True)
                assert (g_st2 == 0).all(), (n, mode)
                assert g_back.tobytes() == back[:n * L].tobytes(), (n, mode)
                assert (g_pn == w.pns[:n]).all(), (n, mode)
            g_back, g_st2, g_pn = gpu_run(w.keys, bad, w.open_desc, open_=True)
            assert (g_st2 == bad_st).all(), (mode, np.nonzero(g_st2 != bad_st)[0][:8])
            assert g_back.tobytes() == bad_back.tobytes(), mode
            assert (g_pn[ok] == bad_pn[ok]).all(), mode
            for t in hit:  # as received, header still protected
                assert g_back[t * L:(t + 1) * L].tobytes() == bad[t * L:(t + 1) * L].tobytes(), (mode, t)


# ---- batches of chosen lengths -------------------------------------------------------------------
def check_modes(orc, b, tamper=(), bad=(), opts=()):
    """Seal b and open the oracle's sealed arena (bytes `tamper` = (packet, byte index from the
    packet's end, bit) flipped first) under both modes, the oracle's results computed once: arena,
    statuses and opened packet numbers equal, guards intact. `bad`: packets refused on both sides;
    opts: further (switch, value) pairs held meanwhile. Returns (received arena, opened arena)."""
    idx = np.arange(len(b.sd))
    good, hit = ~np.isin(idx, bad), np.isin(idx, [t[0] for t in tamper])
    o_out, o_st, _ = oracle_run(orc, b.keys, b.arena, b.sd)
    assert (o_st[good] == 0).all() and (o_st[~good] != 0).all()
    rx = o_out.copy()
    for p, back, bit in tamper:
        rx[int(b.offs[p] + b.L[p]) - 1 - back] ^= 1 << bit
    o_back, o_st2, o_pn = oracle_run(orc, b.keys, rx, b.od, open_=True)
    assert (o_st2[good & ~hit] == 0).all() and (o_st2[hit] == _lib.MQ_ERR_CRYPTO).all() and (o_st2[~good] != 0).all()
    ok = (o_st2 == 0) & b.quic
    assert (o_pn[ok] == b.pns[ok]).all()
    held = [_lib.option(k, v) for k, v in opts]
    for h in held:
        h.__enter__()
    try:
        for mode in MODES:
            with _wgmac(mode):
                g_out, g_st, _ = gpu_run(b.keys, b.arena, b.sd)
                assert (g_st == o_st).all(), (mode, np.nonzero(g_st != o_st)[0][:8])
                assert g_out.tobytes() == o_out.tobytes(), (mode, first_diff(b, g_out, o_out))
                assert b.guards_intact(g_out)
                g_back, g_st2, g_pn = gpu_run(b.keys, rx, b.od, open_=True)
                assert (g_st2 == o_st2).all(), (mode, np.nonzero(g_st2 != o_st2)[0][:8])
                assert g_back.tobytes() == o_back.tobytes(), (mode, first_diff(b, g_back, o_back))
                assert b.guards_intact(g_back)
                assert (g_pn[ok] == o_pn[ok]).all(), mode
    finally:
        for h in reversed(held):
            h.__exit__(None, None, None)
    for p in np.nonzero(hit)[0]:  # a failed packet: as received, header still protected
        lo, hi = int(b.offs[p]), int(b.offs[p] + b.L[p])
        assert o_back[lo:hi].tobytes() == rx[lo:hi].tobytes()
    return rx, o_back


def mixed_lengths_batch(n_keys):
    # eight lengths interleaved, so every tile and every MAC wave holds all of them (2 to 19 steps of
    # four blocks); the PN length walks against them, and the offsets follow from the lengths
    lens = np.array([64, 79, 80, 81, 656, 1199, 1200, 1216])
    i = np.arange(96)
    pls = 1 + (i // 16 + i) % 4  # every length at every payload alignment
    return Batch(lens[i % 8] - HDR - pls - 16, pls, n_keys, seed=41)


def block_count_batch(n_keys):
    # MAC blocks nb = 1 (AAD) + T + 1 with T = ceil(P / 16): nb = 4 k - 1, 4 k, 4 k + 1 for k = 1, 2, 5,
    # 10 and 19, the last ciphertext block of 5, 15 or 16 bytes; plain AEAD rows (no header
    # protection, AAD of 9 .. 13 bytes) every third packet
    P, pls, kind = [], [], []
    for k in (1, 2, 5, 10, 19):
        for nb in (4 * k - 1, 4 * k, 4 * k + 1):
            for last in (5, 15, 16):
                P.append(16 * (nb - 2) - 16 + last)
                kind.append(1 if len(P) % 3 == 0 else 0)
                pls.append(len(P) % 5 if kind[-1] else 1 + len(P) % 4)
    P, pls, kind = (np.array(x) for x in (P, pls, kind))
    b = Batch(P, pls, n_keys, kind=kind, seed=43)
    T = (P + 15) // 16
    assert set(((T + 2) % 4).tolist()) == {3, 0, 1} and len(P) == 45
    return b


@pytest.mark.parametrize("n_keys", [1, 3])
def test_mixed_lengths_inside_a_workgroup(orc, n_keys):
    b = mixed_lengths_batch(n_keys)
    assert sorted(set(b.L.tolist())) == [64, 79, 80, 81, 656, 1199, 1200, 1216]
    assert set(b.pay_align.tolist()) == {0, 1, 2, 3}
    check_modes(orc, b, opts=(("MQ_CC_NARROW", 0), ("MQ_CC_LONG", 0)))


@pytest.mark.parametrize("n_keys", [1, 3])
def test_mac_block_counts(orc, n_keys):
    b = block_count_batch(n_keys)
    assert set(b.pay_align.tolist()) == {0, 1, 2, 3}
    check_modes(orc, b, opts=(("MQ_CC_NARROW", 0), ("MQ_CC_LONG", 0)))


def uniform_batch(n, n_keys=1, pn_len=3, seed=47):
    return Batch([L - HDR - pn_len - 16] * n, [pn_len] * n, n_keys, seed=seed)


@pytest.mark.parametrize("mac_wave", [0, 1])
def test_tampered_packet_in_every_position(orc, mac_wave):
    # one flipped byte (in the tag or in the ciphertext before it) in position p of the first
    # workgroup and in position p of the second, whose roles are rotated differently; the 16
    # positions of one MAC wave per case
    b = uniform_batch(64)
    assert batch.flat_kind(len(b.arena), 64, CHACHA) == 1
    for p in range(16 * mac_wave, 16 * mac_wave + 16):
        check_modes(orc, b, tamper=[(p, 3 * p % 40, p % 8), (32 + p, 600 + p, (p + 3) % 8)])


def test_whole_workgroup_tampered(orc):
    b = uniform_batch(40, n_keys=3)
    check_modes(orc, b, tamper=[(p, 5 * p % 48, p % 8) for p in range(32)])


def direct_tile_batch(wave):
    # 64 packets: the eight of tile `wave` of the first workgroup and of tile (wave + 1) % 4 of the
    # second are 1400 B (over the 10-KiB image: the direct path), the others 1200 B
    i = np.arange(64)
    big = ((i < 32) & (i // 8 == wave)) | ((i >= 32) & ((i - 32) // 8 == (wave + 1) % 4))
    pls = 1 + i % 4
    b = Batch(np.where(big, 1400, L) - HDR - pls - 16, pls, 2, seed=53 + wave)
    assert b.L[big].sum() == 16 * 1400 and (b.L[~big] == L).all()
    return b, int(np.nonzero(big)[0][3])


@pytest.mark.parametrize("wave", range(4))
def test_direct_tile_beside_staged_tiles(orc, wave):
    b, p_big = direct_tile_batch(wave)
    # a failed packet in the direct tile and one in a staged tile beside it
    check_modes(orc, b, tamper=[(p_big, 7, 1), ((p_big + 8) % 32, 20, 6)], opts=(("MQ_CC_LONG", 0),))


def tiny_payload_batch(n_keys):
    # every fourth packet with payload + pn_len in 4 .. 19: its sample reaches into the tag, so the
    # seal makes its mask after the MAC phase; 1200-B packets around them
    i = np.arange(64)
    tiny = i % 4 == 1
    pls = np.where(tiny, 1 + (i // 4) % 4, 1 + i % 4)
    P = np.where(tiny, 4 + (i // 4) % 16 - pls, L - HDR - pls - 16)
    b = Batch(P, pls, n_keys, seed=59)
    assert ((P + pls)[tiny] < 20).all() and ((P + pls)[tiny] >= 4).all() and len(set((P + pls)[tiny].tolist())) > 8
    return b


@pytest.mark.parametrize("n_keys", [1, 2])
def test_tiny_payloads(orc, n_keys):
    b = tiny_payload_batch(n_keys)
    assert batch.flat_kind(len(b.arena), 64, CHACHA) == 1
    check_modes(orc, b, tamper=[(5, 2, 0), (37, 17, 7)])


def no_hp_batch(n_keys):
    # plain AEAD rows (MQ_PKT_NO_HP, 0 .. 4 bytes of AAD behind pn_offset) and TLS records inside
    # workgroups of QUIC rows
    i = np.arange(64)
    kind = np.where(i % 5 == 2, 1, np.where(i % 7 == 3, 2, 0))
    pls = np.where(kind == 1, i % 5, 1 + i % 4)
    P = np.where(kind == 0, L - HDR - pls - 16, 1100 + 3 * i)
    return Batch(P, pls, n_keys, kind=kind, seed=61), kind


@pytest.mark.parametrize("n_keys", [1, 2])
def test_rows_without_header_protection(orc, n_keys):
    b, kind = no_hp_batch(n_keys)
    assert (kind[:32] == 1).sum() > 3 and (kind[:32] == 2).sum() > 2
    assert batch.flat_kind(len(b.arena), 64, CHACHA) == 1
    check_modes(orc, b)


@pytest.mark.parametrize("n_keys", [1, 3])
def test_invalid_descriptors_inside_a_workgroup(orc, n_keys):
    # a bad key id in the first workgroup's second tile, a length past the arena's end in its last
    # tile and another in the second workgroup: refused, bytes kept, the neighbours sealed and opened
    b = uniform_batch(64, n_keys, pn_len=2, seed=67)
    for d in (b.sd, b.od):
        d["key_id"][11] = n_keys
        d["len"][29] = 1 << 30
        d["len"][40] = len(b.arena)
    rx, o_back = check_modes(orc, b, bad=(11, 29, 40))
    for p in (11, 29, 40):
        lo, hi = int(b.offs[p]), int(b.offs[p] + b.L[p])
        assert o_back[lo:hi].tobytes() == b.arena[lo:hi].tobytes()
