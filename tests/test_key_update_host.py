"""Host key update (no GPU needed): mq_derive_key_update = derive_next_application_secret +
derive_key_update_keys (reference key_schedule.rs:114-120, connection/keys.rs:386-414) against
RFC 9001 A.5's "quic ku" value and the oracle's HKDF-Expand-Label, chained over five generations
from the reference's own key-update test secrets (key_schedule.rs:309-359); and the three batch
entries' answers without a device."""
import ctypes

import pytest

from milli_quic_amd import _lib, key_schedule

AES, CHACHA = _lib.MQ_SUITE_AES128GCM, _lib.MQ_SUITE_CHACHA20
KEY_LEN = {AES: 16, CHACHA: 32}


def expand(orc, secret, label, length):
    rc, out = orc.hkdf_expand_label(secret, label, b"", length)
    assert rc == 0
    return out


def check_step(orc, suite, secret, cur):
    """One update of (secret, cur) against the oracle; returns (next_secret, next_km)."""
    nxt, km = key_schedule.derive_key_update(secret, cur)
    assert nxt == expand(orc, secret, b"quic ku", 32)
    kl = KEY_LEN[suite]
    assert km.suite == suite and km.reserved == 0
    assert bytes(km.key) == expand(orc, nxt, b"quic key", kl) + bytes(32 - kl)
    assert bytes(km.iv) == expand(orc, nxt, b"quic iv", 12) and bytes(km.pad) == bytes(4)
    assert bytes(km.hp) == bytes(cur.hp)  # the header-protection key is never updated
    return nxt, km


def test_rfc9001_a5_key_update(mqlib, orc, ref_fixtures):
    a5 = ref_fixtures["rfc9001"]["a5"]
    secret = bytes.fromhex(a5["secret"])
    cur = key_schedule.key_material(CHACHA, secret)
    nxt, km = check_step(orc, CHACHA, secret, cur)
    assert nxt.hex().endswith(a5["ku"])  # the fixture holds the tail of RFC 9001 A.5's ku secret
    assert bytes(km.hp).hex() == "25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4"


def test_aes_key_update_vs_oracle(mqlib, orc, ref_fixtures):
    secret = bytes.fromhex(ref_fixtures["rfc9001"]["a5"]["secret"])
    cur = key_schedule.key_material(AES, secret)
    _, km = check_step(orc, AES, secret, cur)
    assert bytes(km.key)[16:] == bytes(16) and bytes(km.hp)[16:] == bytes(16)


@pytest.mark.parametrize("suite", [AES, CHACHA])
@pytest.mark.parametrize("fill", [0xAA, 0xBB])
def test_key_update_chain(mqlib, orc, suite, fill):
    secret = bytes([fill]) * 32
    km = g0 = key_schedule.key_material(suite, secret)
    seen = {secret}
    for _ in range(5):
        secret, km = check_step(orc, suite, secret, km)
        assert bytes(km.hp) == bytes(g0.hp) and secret not in seen
        seen.add(secret)


def test_key_update_in_place_and_unknown_suite(mqlib):
    secret = (ctypes.c_uint8 * 32)(*([0xAA] * 32))
    cur = key_schedule.key_material(CHACHA, bytes(secret))
    want_secret, want = key_schedule.derive_key_update(bytes(secret), cur)
    assert mqlib.mq_derive_key_update(secret, ctypes.byref(cur), ctypes.byref(cur)) == _lib.MQ_OK  # next == cur
    assert bytes(secret) == want_secret and bytes(cur) == bytes(want)
    for suite in (0, 3, _lib.MQ_SUITE_MIXED):
        bad = _lib.KeyMaterial.from_buffer_copy(bytes(cur))
        bad.suite = suite
        out = _lib.KeyMaterial.from_buffer_copy(b"\xEE" * 88)
        assert mqlib.mq_derive_key_update(secret, ctypes.byref(bad), ctypes.byref(out)) == _lib.MQ_ERR_CRYPTO
        assert bytes(secret) == want_secret and bytes(out) == b"\xEE" * 88
    assert mqlib.mq_derive_key_update(None, ctypes.byref(cur), ctypes.byref(cur)) == _lib.MQ_ERR_INVALID_ARG
    assert mqlib.mq_derive_key_update(secret, None, ctypes.byref(cur)) == _lib.MQ_ERR_INVALID_ARG
    assert mqlib.mq_derive_key_update(secret, ctypes.byref(cur), None) == _lib.MQ_ERR_INVALID_ARG
    with pytest.raises(Exception):
        key_schedule.derive_key_update(b"\x01" * 31, cur)


def test_batch_entries_without_device(mqlib):
    # no table can exist without a device (mq_keytable_create answers MQ_ERR_NO_DEVICE), so the
    # batch entries refuse the missing table; nothing falls back to the host path
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        rows = (_lib.KeyMaterial * 1)()
        assert mqlib.mq_keytable_create(rows, 1, ctypes.byref(h)) == _lib.MQ_ERR_NO_DEVICE and not h
    no =(_lib.MQ_ERR_NO_DEVICE, _lib.MQ_ERR_INVALID_ARG)
    buf = ctypes.cast((ctypes.c_uint8 * 64)(), ctypes.c_void_p)
    assert mqlib.mq_batch_derive_keys(None, CHACHA, buf, 0, None, 1, None, buf, None) in no
    assert mqlib.mq_batch_key_update(None, buf, buf, buf, 1, None, buf, None) in no
    assert mqlib.mq_batch_recv_rekey(None, buf, 1, buf, buf, buf, None) in no
