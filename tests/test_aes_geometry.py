"""The AES-128-GCM geometry ladder (tests/aes_geometry.py) on the CPU: it hits every class it claims
at 8, 4 and 2 lanes per packet, the oracle accepts all of it, and the oracle's bytes equal OpenSSL's
(header-protected packets, the same composite) and the per-packet AEAD (plain packets and records)."""
import numpy as np
import pytest

import aes_geometry as ag

AES = ag.AES


@pytest.fixture(scope="module")
def rows():
    return ag.ladder()


@pytest.fixture(scope="module")
def sealed(orc, rows):
    b = ag.build(rows, decode=orc.decode_pn)
    out = b.arena.copy()
    st = orc.batch_seal(b.keys, out, b.sd, AES, threads=8)
    return b, out, st


def test_ladder_shape(rows):
    L = np.array([o + pl + P + 16 for (o, pl, f, P) in rows])
    big = L > 650
    assert big.sum() == len(ag.CTR_LENS) * len(ag.CTR_HEADERS) and set(L[big]) == set(ag.CTR_LENS)
    assert 6500 <= len(rows) <= 9500 and L[~big].sum() < (5 << 19)
    assert {r[:3] for r in rows} >= set(ag.HEADERS)
    for (o, pl, f) in ag.SWEEP_HEADERS:
        assert {r[3] for r in rows if r[:3] == (o, pl, f)} >= set(range(ag.min_payload(pl, f), 301))
    short = ag.shortest(rows)
    assert len(short) >= 300 and max(o + pl + P + 16 for (o, pl, f, P) in short) <= 64


@pytest.mark.parametrize("G", ag.LANES)
def test_every_class_is_hit(rows, G):
    missing = ag.all_classes(G) - ag.classes(G, rows)
    assert not missing, sorted(missing, key=str)
    # the classes of the kernel's constants, restated: the HP block's slot and the lean stretch
    assert ag.hp_slot_min(G) == (G if G >= 4 else 4)
    assert ag.lean_end_of(16 * (2 * G - 2) - 1, G) == 0 and ag.lean_end_of(16 * (2 * G - 2), G) == 1
    assert ag.lean_end_of(16 * (3 * G - 2), G) == 2


def test_every_decode_branch_at_every_pn_len(orc, rows):
    b = ag.build(rows, decode=orc.decode_pn)
    assert all(b.branches[q] == {"candidate", "plus_win", "minus_win"} for q in (1, 2, 3, 4))
    over = b.od["len"] > 2048
    assert ((b.od["flags"] & 0x08 != 0) == over).all() and over.sum() == len(ag.CTR_LENS) * len(ag.CTR_HEADERS)


def test_oracle_accepts_the_ladder(orc, sealed):
    b, out, st = sealed
    assert (st == 0).all(), np.nonzero(st)[0][:8]
    back = out.copy()
    st2, pn = orc.batch_open(b.keys, back, b.od, AES, threads=8)
    assert (st2 == 0).all(), np.nonzero(st2)[0][:8]
    assert (pn == b.pns).all()
    # opened: the plaintext again, but for each record's header and inner content type
    want = b.arena.copy()
    for i in np.nonzero(b.sd["flags"] & 0x04)[0]:
        o, n = int(b.sd["offset"][i]), int(b.sd["len"][i])
        want[o:o + 5] = [23, 3, 3, (n - 5) >> 8, (n - 5) & 0xFF]
        want[o + n - 17] = b.sd["reserved"][i]
    tags = np.zeros(len(want), dtype=bool)
    for o, n in zip(b.sd["offset"], b.sd["len"]):
        tags[int(o) + int(n) - 16:int(o) + int(n)] = True
    assert back[~tags].tobytes() == want[~tags].tobytes()


def test_oracle_equals_openssl_on_header_protected_packets(orc, sealed):
    if not orc.ossl_available():
        pytest.skip("libcrypto.so.3 is absent")
    b, out, _ = sealed
    hp = np.nonzero(b.sd["flags"] & ag.NO_HP == 0)[0]
    assert len(hp) > 6000
    ref = b.arena.copy()
    st = orc.ossl_batch(b.keys, ref, np.ascontiguousarray(b.sd[hp]), False, threads=8)
    assert st is not None and (st == 0).all()
    for i in hp:
        o, n = int(b.sd["offset"][i]), int(b.sd["len"][i])
        assert out[o:o + n].tobytes() == ref[o:o + n].tobytes(), (i, b.rows[i])
    st = orc.ossl_batch(b.keys, ref, np.ascontiguousarray(b.od[hp]), True, threads=8)
    assert (st == 0).all()
    for i in hp:
        o, n = int(b.sd["offset"][i]), int(b.sd["len"][i])
        assert ref[o:o + n - 16].tobytes() == b.arena[o:o + n - 16].tobytes(), (i, b.rows[i])


def test_oracle_equals_per_packet_aead_on_plain_packets_and_records(orc, sealed):
    b, out, _ = sealed
    row = b.keys[0]
    iv = int.from_bytes(bytes(row.iv), "big")
    plain = np.nonzero(b.sd["flags"] & ag.NO_HP)[0]
    assert len(plain) > 600
    for i in plain:
        o, n, na = int(b.sd["offset"][i]), int(b.sd["len"][i]), int(b.sd["pn_offset"][i]) + int(b.sd["pn_len"][i])
        aad, pt = b.arena[o:o + na].tobytes(), b.arena[o + na:o + n - 16].tobytes()
        if b.sd["flags"][i] & 0x04:
            aad = bytes([23, 3, 3, (n - 5) >> 8, (n - 5) & 0xFF])
            pt = pt[:-1] + bytes([int(b.sd["reserved"][i])])
        nonce = (iv ^ int(b.sd["pn"][i])).to_bytes(12, "big")
        rc, ct, _ = orc.aead_seal(AES, bytes(row.key)[:16], nonce, aad, pt)
        assert rc == 0 and out[o:o + n].tobytes() == aad + ct, (i, b.rows[i])
