"""The pair loop of the workgroup MAC phase (mq_chacha.hip poly_tag<4, PAIR>: two lean Poly1305
steps per reduction, p26_mul2, then at most one single step) against the oracle, byte for byte: every
batch is sealed, and the oracle's sealed arena opened, with MQ_CC_WGMAC unset (the phase, which runs
the pair loop; the multi-key open kernel's phase keeps the single steps) and at 0 (the per-wave MAC of
the same kernels, which does not), with 1 and 3 keys.
Shapes: lean stretches of 0-5 and 15-17 steps (odd, even, none) derived from a transcription of
mq_poly_sched.h's poly_lean, with the edge steps and with the former ones, so the table holds
whichever the phase runs; every payload alignment (the selector of the look-ahead loads); one short
packet among 15 of 1200 B in every position of a MAC wave (prepended zero blocks shrink the common
stretch); a workgroup whose last tile is partial; a tampered tag and a tampered ciphertext byte inside
the pair loop's range.
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, workload  # noqa: E402

from test_gpu_chacha_xor_edges import HDR, Batch  # noqa: E402
from test_gpu_wg_mac import check_modes  # noqa: E402

pytestmark = pytest.mark.gpu
CHACHA = _lib.MQ_SUITE_CHACHA20
OCTET = (("MQ_CC_NARROW", 0), ("MQ_CC_LONG", 0))  # short packets stay on the octet kernels with the MAC phase
G = 4  # lanes per packet of the workgroup MAC


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


# ---- mq_poly_sched.h in Python --------------------------------------------------------------------
def poly_lean(aad_len, ct_len, kmax, edge):
    A, T = (aad_len + 15) >> 4, (ct_len + 15) >> 4
    nb = A + T + 1
    z = G * kmax - nb
    ct_full_end = A + (ct_len >> 4)
    k_lo = (A + z + G - 1) // G
    hi = ct_full_end + z - (G if edge else 2 * G) + 1
    return k_lo, (0 if hi <= 0 else (hi + G - 1) // G)


def stretch(geom, edge):
    """Lean steps of a MAC wave over packets geom = [(aad_len, ct_len), ...]."""
    kmax = max(((a + 15) >> 4) + ((c + 15) >> 4) + 1 + G - 1 for a, c in geom) // G
    lo, hi = zip(*(poly_lean(a, c, kmax, edge) for a, c in geom))
    klo, khi = max(lo), min(min(hi), kmax - 1)
    return max(khi - klo, 0)


def mac_waves(b):
    """(aad_len, ct_len) of the packets of every MAC wave (16 consecutive packets) of a batch."""
    aad = (b.sd["pn_offset"].astype(np.int64) + b.sd["pn_len"]).tolist()
    ct = (b.L - np.array(aad) - 16).tolist()
    return [list(zip(aad[i:i + 16], ct[i:i + 16])) for i in range(0, len(aad), 16)]


class Uniform:
    """n packets of L bytes at offsets i L (workload.uniform: any DCID length) with what check_modes
    asks of a batch."""

    def __init__(self, n, L, pn_len=4, n_keys=1, dcid=workload.DCID8):
        w = workload.uniform(n, CHACHA, L=L, pn_len=pn_len, dcid=dcid, n_keys=n_keys)
        self.keys, self.arena, self.sd, self.od, self.pns = w.keys, w.arena, w.seal_desc, w.open_desc, w.pns
        self.offs, self.L, self.quic = np.arange(n, dtype=np.int64) * L, np.full(n, L, dtype=np.int64), np.ones(n, dtype=bool)
        self.pay_align = (self.offs + 1 + len(dcid) + pn_len) & 3

    def guards_intact(self, a):
        return len(a) == len(self.arena)


def on_mac_phase_kernels(b):
    """The batch takes the flat octet kernels over 10-KiB images (the ones with the MAC phase) by
    itself; the others are held there by OCTET."""
    return batch.flat_kind(len(b.arena), len(b.sd), CHACHA) == 1


# ---- stretch lengths ------------------------------------------------------------------------------
# 13-B header: with the former edge steps 0 .. 5 lean steps at the first six lengths and 15, 16, 17 at
# the last three; with the G = 4 edge steps every boundary lies 64 B lower
FORMER = (180, 200, 260, 320, 400, 460, 1100, 1200, 1214)
LENGTHS = tuple(sorted(set(FORMER) | {L - 64 for L in FORMER}))
WANT = {0, 1, 2, 3, 4, 5, 15, 16, 17}


def test_stretch_table():
    # the lengths below cover every wanted stretch under either form of the edge steps, so the GPU
    # cases cannot quietly stop covering the odd, the even and the empty stretch
    for edge in (False, True):
        got = {stretch([(13, L - 13 - 16)] * 16, edge) for L in LENGTHS}
        assert WANT <= got, (edge, sorted(got))
    assert [stretch([(13, L - 29)] * 16, False) for L in FORMER] == [0, 1, 2, 3, 4, 5, 15, 16, 17]
    assert [stretch([(13, L - 64 - 29)] * 16, True) for L in FORMER] == [0, 1, 2, 3, 4, 5, 15, 16, 17]


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("L", LENGTHS)
def test_stretch_lengths(orc, L, n_keys):
    b = Uniform(64, L, pn_len=4, n_keys=n_keys)
    assert 8 * L + 3 <= 10240 - 512  # eight packets fit a wave's image: staged tiles
    assert mac_waves(b) == [[(13, L - 29)] * 16] * 4
    check_modes(orc, b, opts=OCTET)


# ---- payload alignment ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 3])
def test_payload_alignments(orc, n_keys):
    seen = {5: set(), 8: set()}
    for d in (5, 8):
        for pn_len in (1, 2, 3, 4):
            b = Uniform(64, 1200, pn_len=pn_len, n_keys=n_keys, dcid=workload.DCID8[:d])
            assert on_mac_phase_kernels(b) and len(set(b.pay_align.tolist())) == 1
            seen[d].add(int(b.pay_align[0]))
            assert stretch(mac_waves(b)[0], False) == 16
            check_modes(orc, b)
    assert seen[5] == seen[8] == {0, 1, 2, 3}


# ---- mixed geometry inside one MAC wave ------------------------------------------------------------
SHORTS = (200, 600, 1000, 264)


def mixed_batches(n_keys):
    """16 batches of 64 packets = 4 MAC waves each: 15 packets of 1200 B and one of 200, 600 or 1000 B,
    over the batches in every one of a MAC wave's 16 positions at every one of the three lengths; and
    one of 264 B likewise (those three give stretches of one parity: 1, 7, 13 lean steps with the
    former edge steps, one more with the G = 4 ones; 264 B gives the other)."""
    combos = [(pos, short) for short in SHORTS for pos in range(16)]
    out = []
    for k in range(0, len(combos), 4):
        L = np.full(64, 1200)
        for wave, (pos, short) in enumerate(combos[k:k + 4]):
            L[16 * wave + pos] = short
        pls = 1 + (np.arange(64) + k) % 4
        out.append(Batch(L - HDR - pls - 16, pls, n_keys, seed=71 + k))
    return out


def test_mixed_geometry_table():
    seen = {False: set(), True: set()}
    short_at = set()
    for b in mixed_batches(1):
        for w, geom in enumerate(mac_waves(b)):
            (pos,) = [i for i, (a, c) in enumerate(geom) if a + c + 16 != 1200]
            short_at.add((pos, geom[pos][0] + geom[pos][1] + 16))
            for edge in (False, True):
                seen[edge].add(stretch(geom, edge))
    assert short_at == {(p, s) for p in range(16) for s in SHORTS}
    for edge in (False, True):  # shorter than the uniform wave's, odd and even
        assert max(seen[edge]) < 16 and {s & 1 for s in seen[edge]} == {0, 1} and len(seen[edge]) >= 3, seen


@pytest.mark.parametrize("n_keys", [1, 3])
def test_mixed_geometry_in_a_mac_wave(orc, n_keys):
    for b in mixed_batches(n_keys):
        assert set(b.pay_align.tolist()) == {0, 1, 2, 3}
        check_modes(orc, b, opts=OCTET)


# ---- a partial last tile ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 3])
def test_partial_last_tile(orc, n_keys):
    # one whole workgroup, then one with a whole tile and a tile of three packets: MAC wave 0 of the
    # second workgroup has 11 live packets, MAC wave 1 none
    b = Uniform(32 + 8 + 3, 1200, pn_len=2, n_keys=n_keys)
    assert on_mac_phase_kernels(b)
    check_modes(orc, b)


# ---- tampering ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 3])
def test_tampered_tag_and_ciphertext(orc, n_keys):
    # (packet, byte from the packet's end, bit): tags (the last 16 bytes) and ciphertext bytes that the
    # pair loop absorbs (steps 1 .. 16 of 19 hold ciphertext bytes 35 .. 1058 of 1171: 128 .. 1151 from
    # the end), in both workgroups and all four MAC waves. check_modes asserts MQ_ERR_CRYPTO for exactly
    # these, their bytes as received, and every other packet opened.
    b = Uniform(64, 1200, pn_len=4, n_keys=n_keys)
    tags = [(0, 0, 0), (13, 15, 7), (17, 8, 3), (47, 5, 1), (63, 11, 6)]
    body = [(2, 128, 0), (15, 600, 5), (16, 1151, 2), (31, 131, 7), (40, 900, 4), (62, 333, 1)]
    assert not {t[0] for t in tags} & {t[0] for t in body}
    check_modes(orc, b, tamper=tags)
    check_modes(orc, b, tamper=body)
    check_modes(orc, b, tamper=tags + body)
