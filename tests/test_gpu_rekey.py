"""Traffic-secret key derivation and key updates on the GPU: mq_batch_derive_keys (install_derived,
reference src/connection/keys.rs:216-279), mq_batch_key_update (derive_next_application_secret +
derive_key_update_keys, key_schedule.rs:114-120, keys.rs:386-414) and mq_batch_recv_rekey, bit-exact
against the oracle's HKDF (pinned to RFC 9001 A.1 / A.5 in test_oracle_golden.py), and usable as
key-table rows: packets sealed with the device-written rows equal the oracle's with host-built
material, and a receive connection table stays on the device across two peer key updates.

Sizes: 1 / 63 / 64 / 65 lanes around one wave, 257 = one 256-lane block plus one lane."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, recv, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

from recv_traffic import assemble  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AES, CHACHA, MIXED = _lib.MQ_SUITE_AES128GCM, _lib.MQ_SUITE_CHACHA20, _lib.MQ_SUITE_MIXED
KM = ctypes.sizeof(_lib.KeyMaterial)


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
    return torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)


def orc_km(orc, suite, secret):
    km = _lib.KeyMaterial()
    assert orc.load().orc_derive_key_material(ctypes.c_uint32(suite), bytes(secret), ctypes.c_size_t(32),
                                              ctypes.byref(km)) == 0
    return km


def orc_update(orc, secret, cur):
    """The oracle's key update: "quic ku", then key / iv of the new secret; the HP key stays."""
    rc, nxt = orc.hkdf_expand_label(secret, b"quic ku", b"", 32)
    assert rc == 0
    km = orc_km(orc, cur.suite, nxt)
    km.hp[:] = cur.hp[:]
    return nxt, km


def secrets_for(ref_fixtures, n, seed):
    s = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[0] = np.frombuffer(bytes.fromhex(ref_fixtures["rfc9001"]["a5"]["secret"]), dtype=np.uint8)
    return s


def copy_km(km):
    return _lib.KeyMaterial.from_buffer_copy(bytes(km))


def seal_on(kt, w, sd, hint):
    a, s = t(w.arena), sentinel(w.n)
    ws = torch.empty(batch.workspace_bytes(w.n), dtype=torch.uint8, device=DEV) if hint == MIXED else None
    batch.seal(kt, a, t(sd), s, hint, ws)
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0).all()
    return a


def check_seal(orc, kt, keys, rows, hint, per_row=1, L=120):
    """Packets sealed with the table's rows `rows` equal the oracle's with the host list `keys`."""
    rows = np.asarray(rows, dtype=np.uint32)
    w = workload.uniform(len(rows) * per_row, CHACHA, L=L, pn_len=2, keys=keys)
    sd = w.seal_desc.copy()
    sd["key_id"] = rows[np.arange(w.n) % len(rows)]
    a = seal_on(kt, w, sd, hint)
    ref = w.arena.copy()
    assert (orc.batch_seal(keys, ref, sd, hint, threads=4) == 0).all()
    assert a.cpu().numpy().tobytes() == ref.tobytes()
    return w, sd, a


@pytest.mark.parametrize("with_km", [True, False])
@pytest.mark.parametrize("scatter", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("suite", [AES, CHACHA])
def test_derive_keys_vs_oracle(orc, ref_fixtures, suite, n, scatter, with_km):
    sec = secrets_for(ref_fixtures, n, seed=n)
    if scatter:  # a seeded permutation of a larger table
        n_rows = 2 * n + 5
        rows = np.random.default_rng(n + 1).permutation(n_rows)[:n].astype(np.uint32)
    else:
        n_rows = n + 4
        rows = 3 + np.arange(n, dtype=np.uint32)
    kt = KeyTable([_lib.KeyMaterial() for _ in range(n_rows)])
    st = sentinel(n)
    km = torch.zeros(KM * n, dtype=torch.uint8, device=DEV) if with_km else None
    batch.derive_keys(kt, suite, t(sec), st, first_row=0 if scatter else 3, row_idx=u32(rows) if scatter else None,
                      km_out=km)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    want = [orc_km(orc, suite, sec[i].tobytes()) for i in range(n)]
    if with_km:
        got = km.cpu().numpy().reshape(n, KM)
        for i in range(n):
            assert got[i].tobytes() == bytes(want[i]), i
    keys = [_lib.KeyMaterial() for _ in range(n_rows)]
    for i in range(n):
        keys[int(rows[i])] = want[i]
    check_seal(orc, kt, keys, rows, suite)


@pytest.mark.parametrize("suite", [AES, CHACHA])
def test_derived_rows_protect_like_oracle(orc, ref_fixtures, suite):
    # rows written on the device seal and open exactly as the oracle does with oracle-derived
    # material, and as a second table built on the host from that material; ChaCha20: the 32-byte
    # HP key goes through header protection
    n = 64
    sec = secrets_for(ref_fixtures, n, seed=9)
    kt = KeyTable([_lib.KeyMaterial() for _ in range(n + 3)])
    st = sentinel(n)
    batch.derive_keys(kt, suite, t(sec), st, first_row=3)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    keys = [_lib.KeyMaterial() for _ in range(3)] + [orc_km(orc, suite, sec[i].tobytes()) for i in range(n)]
    if suite == CHACHA:
        assert any(bytes(k.hp)[16:] != bytes(16) for k in keys[3:])
    w, sd, a = check_seal(orc, kt, keys, 3 + np.arange(n), suite, per_row=4, L=333)
    kt2 = KeyTable(keys)
    a2 = seal_on(kt2, w, sd, suite)
    assert a.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes()
    od = w.open_desc.copy()
    od["key_id"] = sd["key_id"]
    ref = a.cpu().numpy().copy()
    o_st, o_pn = orc.batch_open(keys, ref, od, suite, threads=4)
    s = sentinel(w.n)
    pn = torch.zeros(w.n, dtype=torch.int64, device=DEV)
    batch.open_(kt, a, t(od), s, pn, suite)
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0).all() and (o_st == 0).all()
    assert (pn.cpu().numpy().view(np.uint64) == o_pn).all() and (o_pn == w.pns).all()
    assert a.cpu().numpy().tobytes() == ref.tobytes()


def test_derive_keys_keeps_suite_view(orc, ref_fixtures):
    # consecutive rows keep the table's host view of its suites: a table of AES rows with exactly one
    # ChaCha20 row written by derive_keys runs mixed batches like one built on the host (its ChaCha20
    # list takes the single-key path), and like the oracle after a second row turned ChaCha20
    n_rows = 8
    sec = secrets_for(ref_fixtures, n_rows, seed=21)
    keys = [orc_km(orc, AES, sec[i].tobytes()) for i in range(n_rows)]
    kt = KeyTable(keys)
    for row, s in ((5, sec[0]), (2, sec[1])):
        st = sentinel(1)
        batch.derive_keys(kt, CHACHA, t(s), st, first_row=row)
        torch.cuda.synchronize()
        assert int(st[0]) == 0
        keys[row] = orc_km(orc, CHACHA, s.tobytes())
        check_seal(orc, kt, keys, np.arange(n_rows), MIXED, per_row=24, L=200)


def update_table(orc, ref_fixtures, n, seed):
    """Rows [0, n): generation 0 of n secrets, suites mixed; [n, 2n): rows of a known other key; row
    2n: empty; row 2n + 1: the other key again."""
    sec = secrets_for(ref_fixtures, n, seed=seed)
    suites = np.random.default_rng(seed + 1).choice([AES, CHACHA], size=n)
    suites[0] = CHACHA  # RFC 9001 A.5's secret and suite
    if n > 1:
        suites[1] = AES
    other = orc_km(orc, AES, bytes(range(32)))
    keys = [orc_km(orc, int(suites[i]), sec[i].tobytes()) for i in range(n)]
    keys += [copy_km(other) for _ in range(n)] + [_lib.KeyMaterial(), copy_km(other)]
    return sec, keys, KeyTable(keys)


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_key_update_chain_vs_oracle(orc, ref_fixtures, n, same):
    sec, keys, kt = update_table(orc, ref_fixtures, n, seed=3 * n)
    g0_hp = [bytes(keys[i].hp) for i in range(n)]
    secrets = t(sec)
    host = [sec[i].tobytes() for i in range(n)]
    lo, hi = np.arange(n, dtype=np.uint32), n + np.arange(n, dtype=np.uint32)
    for step in range(3):  # dst != src: the generations go back and forth between the two halves
        src = lo if same or step % 2 == 0 else hi
        dst = lo if same else (hi if step % 2 == 0 else lo)
        st, km = sentinel(n), torch.zeros(KM * n, dtype=torch.uint8, device=DEV)
        batch.key_update(kt, secrets, u32(src), u32(dst), st, km_out=km)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
        for i in range(n):
            host[i], keys[int(dst[i])] = orc_update(orc, host[i], keys[int(src[i])])
        got_s, got = secrets.cpu().numpy().reshape(n, 32), km.cpu().numpy().reshape(n, KM)
        for i in range(n):
            want = keys[int(dst[i])]
            assert got_s[i].tobytes() == host[i], (step, i)
            assert got[i].tobytes() == bytes(want), (step, i)  # suite, key, iv and hp
            assert got[i, 56:88].tobytes() == g0_hp[i], (step, i)
        check_seal(orc, kt, keys, dst, MIXED)
    check_seal(orc, kt, keys, np.arange(2 * n), MIXED)  # both halves: the sources stayed usable too


def test_key_update_error_rows(orc, ref_fixtures):
    n = 8
    sec, keys, kt = update_table(orc, ref_fixtures, n, seed=77)
    n_rows, empty = len(keys), 2 * n
    #            good ...                 src beyond   dst beyond   empty source
    src = list(range(n)) + [n_rows + 5, 1, empty]
    dst = list(range(n, 2 * n)) + [2 * n + 1, n_rows, 2 * n + 1]
    order = np.random.default_rng(5).permutation(len(src))  # the error entries among the good ones
    src, dst = np.asarray(src, dtype=np.uint32)[order], np.asarray(dst, dtype=np.uint32)[order]
    m = len(src)
    s_in = np.random.default_rng(6).integers(0, 256, size=(m, 32), dtype=np.uint8)
    secrets, st, km = t(s_in), sentinel(m), sentinel(KM * m)
    batch.key_update(kt, secrets, u32(src), u32(dst), st, km_out=km)
    torch.cuda.synchronize()
    st, got_s, got = st.cpu().numpy(), secrets.cpu().numpy().reshape(m, 32), km.cpu().numpy().reshape(m, KM)
    for i in range(m):
        if src[i] >= n_rows or dst[i] >= n_rows:
            want = _lib.MQ_ERR_INVALID_ARG
        elif src[i] == empty:
            want = _lib.MQ_ERR_CRYPTO
        else:
            want = _lib.MQ_OK
        assert st[i] == want, (i, src[i], dst[i])
        if want == _lib.MQ_OK:
            nxt, keys[int(dst[i])] = orc_update(orc, s_in[i].tobytes(), keys[int(src[i])])
            assert got_s[i].tobytes() == nxt and got[i].tobytes() == bytes(keys[int(dst[i])])
        else:  # secret and material untouched
            assert got_s[i].tobytes() == s_in[i].tobytes() and (got[i] == 0xEE).all()
    assert sorted(st[st != 0]) == [_lib.MQ_ERR_CRYPTO, _lib.MQ_ERR_INVALID_ARG, _lib.MQ_ERR_INVALID_ARG]
    # the failed entries' destination (2n + 1) and source (1) rows protect as before the call, and the
    # empty row is still empty: every row of the table against the host list
    rows = [r for r in range(n_rows) if r != empty]
    check_seal(orc, kt, keys, rows, MIXED)
    w = workload.uniform(2, CHACHA, L=120, pn_len=2, keys=keys)
    sd = w.seal_desc.copy()
    sd["key_id"] = empty
    a, s = t(w.arena), sentinel(2)
    batch.seal(kt, a, t(sd), s, MIXED, torch.empty(batch.workspace_bytes(2), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert (s.cpu().numpy() != 0).all() and a.cpu().numpy().tobytes() == w.arena.tobytes()


def host_rekey(orc, keys, conns, secrets, pool_first):
    """mq_batch_recv_rekey restated: per connection with HAS_APP and without HAS_NEXT, the next
    generation goes into the lowest row of its 4-row pool that holds neither the current nor (with
    HAS_PREV) the previous generation."""
    st = np.zeros(len(conns), dtype=np.uint8)
    for i in range(len(conns)):
        f = int(conns[i]["flags"])
        if not f & recv.HAS_APP or f & recv.HAS_NEXT:
            continue
        pool = int(pool_first[i])
        if pool + 4 > len(keys):
            st[i] = _lib.MQ_ERR_INVALID_ARG
            continue
        prev, cur = int(conns[i]["app_row"][0]), int(conns[i]["app_row"][1])
        if cur >= len(keys) or keys[cur].suite not in (AES, CHACHA):
            st[i] = _lib.MQ_ERR_CRYPTO
            continue
        taken = {cur, prev} if f & recv.HAS_PREV else {cur}
        dst = min(r for r in range(pool, pool + 4) if r not in taken)
        secrets[i], keys[dst] = orc_update(orc, secrets[i], keys[cur])
        conns[i]["app_row"][2] = dst
        conns[i]["flags"] = f | recv.HAS_NEXT
    return st


def test_recv_chain_without_host_keys(orc, ref_fixtures):
    # Two peer key updates with the connection table never leaving the device: the 1-RTT keys come
    # from derive_keys, every later generation from recv.rekey between the receive batches. The
    # peer's traffic is protected on the host with a real "quic ku" chain s0 -> s1 -> s2.
    n_conns, no_app, short_pool = 24, 22, 23
    rng = np.random.default_rng(31)
    suites = rng.choice([AES, CHACHA], size=n_conns)
    suites[0], suites[1] = CHACHA, AES
    s0 = secrets_for(ref_fixtures, n_conns, seed=32)
    pool_first = (1 + 4 * np.arange(n_conns)).astype(np.uint32)
    n_rows = int(pool_first[short_pool]) + 2  # the last connection's pool runs past the table
    conns = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
    conns["app_row"][:, 1] = pool_first
    conns["dcid_len"], conns["flags"] = 8, recv.HAS_APP
    conns["flags"][no_app] = 0
    # the peer's send keys: generations 0..2 of every connection (sender rows 3c + g), and its packets
    tx_keys, scripts1, scripts2 = [], [], []
    for c in range(n_conns):
        sec, km = s0[c].tobytes(), orc_km(orc, int(suites[c]), s0[c].tobytes())
        for g in range(3):
            tx_keys.append(km)
            sec, km = orc_update(orc, sec, km)
        names = {"g0": 3 * c, "g1": 3 * c + 1, "g2": 3 * c + 2}
        dcid = rng.bytes(8)

        def dg(name, phase, pns):
            return [[(name, 2, phase, pn, rng.bytes(int(rng.integers(1, 300))), False)] for pn in pns]
        scripts1.append((dcid, names, dg("g0", 0, (1, 2, 3)) + dg("g1", 1, (4, 5, 7))))
        scripts2.append((dcid, names, dg("g1", 1, (6, 8)) + dg("g2", 0, (9, 10, 12))))
    batches = [assemble(orc, tx_keys, conns, sc, seed=40 + k, extras=False) for k, sc in enumerate((scripts1, scripts2))]

    # host side: a key list with the table's row numbering, advanced by host_rekey
    keys = [_lib.KeyMaterial() for _ in range(n_rows)]
    for c in range(n_conns):
        keys[int(pool_first[c])] = orc_km(orc, int(suites[c]), s0[c].tobytes())
    h_conns, h_sec = conns.copy(), [s0[c].tobytes() for c in range(n_conns)]

    kt = KeyTable([_lib.KeyMaterial() for _ in range(n_rows)])
    d_conns, d_sec, d_pool = t(conns), t(s0), u32(pool_first)
    for suite in (AES, CHACHA):
        idx = np.nonzero(suites == suite)[0]
        st = sentinel(len(idx))
        batch.derive_keys(kt, suite, t(s0[idx]), st, row_idx=u32(pool_first[idx]))
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()

    def rekey_and_compare():
        st = sentinel(n_conns)
        recv.rekey(kt, d_conns, d_sec, d_pool, st)
        torch.cuda.synchronize()
        want = host_rekey(orc, keys, h_conns, h_sec, pool_first)
        assert want[short_pool] == _lib.MQ_ERR_INVALID_ARG and want[no_app] == 0
        assert (st.cpu().numpy() == want).all()
        got = d_conns.cpu().numpy().view(recv.CONN_DTYPE)
        assert (got["app_row"] == h_conns["app_row"]).all() and (got["flags"] == h_conns["flags"]).all()
        assert got.tobytes() == h_conns.tobytes()
        assert d_sec.cpu().numpy().tobytes() == b"".join(h_sec)

    rekey_and_compare()
    assert (h_conns["flags"][:no_app] == recv.HAS_APP | recv.HAS_NEXT).all()
    for k, (arena, dgrams) in enumerate(batches):
        max_pkts = len(dgrams) + 8
        a = t(arena)
        pk = torch.zeros(max_pkts * recv.PKT_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.empty(recv.workspace_bytes(len(dgrams), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
        recv.recv(kt, d_conns, a, t(dgrams), pk, cnt, ws)
        torch.cuda.synchronize()
        oa = arena.copy()
        o_pk, o_n = orc.batch_recv(keys, h_conns, oa, dgrams, max_pkts)
        assert int(cnt.cpu()[0]) == o_n == len(dgrams)
        g_pk = pk.cpu().numpy().view(recv.PKT_DTYPE)[:o_n]
        for f in recv.PKT_DTYPE.names:
            assert (g_pk[f] == o_pk[f]).all(), (k, f, np.nonzero(g_pk[f] != o_pk[f])[0][:10])
        assert d_conns.cpu().numpy().tobytes() == h_conns.tobytes()
        assert a.cpu().numpy().tobytes() == oa.tobytes()
        # every connection with a pool opened all its packets and confirmed one key update per batch
        ok = np.isin(dgrams["conn"], np.arange(no_app))
        assert (o_pk["status"][ok] == 0).all() and (o_pk["status"][~ok] != 0).any()
        assert (h_conns["key_updates"][:no_app] == k + 1).all() and (o_pk["key_gen"][ok] == 2).sum() == no_app
        assert (h_conns["flags"][:no_app] == recv.HAS_APP | recv.HAS_PREV).all()
        rekey_and_compare()
    # the third generation reused the pool row the first one left
    assert (h_conns["app_row"][:no_app, 2] == pool_first[:no_app]).all()


def test_rekey_bounds(orc, ref_fixtures):
    kt = KeyTable([_lib.KeyMaterial() for _ in range(8)])
    none8, none32 = torch.zeros(0, dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    batch.derive_keys(kt, AES, none8, none8, first_row=8)  # n = 0: MQ_OK, nothing launched
    batch.key_update(kt, none8, none32, none32, none8)
    recv.rekey(kt, none8, none8, none32, none8)
    sec, st = t(secrets_for(ref_fixtures, 4, seed=1)), sentinel(4)
    with pytest.raises(Exception):  # first_row + n beyond the table: nothing launched
        batch.derive_keys(kt, CHACHA, sec, st, first_row=5)
    with pytest.raises(Exception):  # unknown suite
        batch.derive_keys(kt, 3, sec, st, first_row=0)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0xEE).all()
    batch.derive_keys(kt, CHACHA, sec, st, row_idx=u32([0, 8, 7, 1 << 31]))  # per-row bounds
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [0, _lib.MQ_ERR_INVALID_ARG, 0, _lib.MQ_ERR_INVALID_ARG]
