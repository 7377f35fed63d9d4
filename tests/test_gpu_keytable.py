"""mq_keytable_update (KeyTable.update) against a model list of key material on the host: after every
step a small batch over all rows (24 packets of 200 B per row) is sealed and opened with the MIXED
hint and with each single-suite hint, and statuses, bytes and packet numbers equal the oracle's with
the model. The steps walk what the update keeps besides the rows themselves: the expanded round keys
and GHASH powers of a row (build_row), and the host view of the rows' suites (kt_mirror: the count
of non-AES rows, which sends a mixed batch's ChaCha20 list down the single-key path when it is 1,
and `derived`, which rules that path out once rows were written on the device). A count that
drifted would run a whole list with the wrong row's key."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, crypto, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402
from milli_quic_amd.key_schedule import make_key_material  # noqa: E402

from test_gpu_rekey import copy_km, orc_km, orc_update, sentinel, t, u32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AES, CHACHA, MIXED = _lib.MQ_SUITE_AES128GCM, _lib.MQ_SUITE_CHACHA20, _lib.MQ_SUITE_MIXED
PER_ROW, LEN = 24, 200


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


_rng = np.random.default_rng(2024)


def fresh(suite, key=None, iv=None):
    """A row of `suite` with new random key, iv and hp (or the given key / iv)."""
    klen = 16 if suite == AES else 32
    return make_key_material(suite, key if key is not None else _rng.bytes(klen),
                             iv if iv is not None else _rng.bytes(12), _rng.bytes(klen))


def empty():
    return _lib.KeyMaterial()  # suite 0: every packet on it is rejected


def run(kt, arena, desc, hint, open_):
    n = len(desc)
    a, st = t(arena), sentinel(n)
    pn = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.full((max(batch.workspace_bytes(n), 256),), 0xA5, dtype=torch.uint8, device=DEV)
    if open_:
        batch.open_(kt, a, t(desc), st, pn, hint, ws)
    else:
        batch.seal(kt, a, t(desc), st, hint, ws)
    torch.cuda.synchronize()
    return a.cpu().numpy(), st.cpu().numpy(), pn.cpu().numpy().view(np.uint64)


def check(orc, kt, model, what):
    """Seal and open 24 packets per row with the table; the oracle does the same with the model."""
    assert kt.rows == len(model)
    w = workload.uniform(PER_ROW * len(model), AES, L=LEN, pn_len=3, keys=model, seed=len(what))
    suites = np.array([m.suite for m in model])[w.seal_desc["key_id"]]
    for hint in (MIXED, AES, CHACHA):
        ref = w.arena.copy()
        o_st = orc.batch_seal(model, ref, w.seal_desc, hint, threads=4)
        served = suites != 0 if hint == MIXED else suites == hint
        assert ((o_st == 0) == served).all(), (what, hint)  # the model itself: only those rows seal
        out, st, _ = run(kt, w.arena, w.seal_desc, hint, False)
        assert (st == o_st).all(), (what, hint, "seal status", np.nonzero(st != o_st)[0][:8], st[st != o_st][:8])
        assert out.tobytes() == ref.tobytes(), (what, hint, "seal")
        back = ref.copy()
        o_st, o_pn = orc.batch_open(model, back, w.open_desc, hint, threads=4)
        assert ((o_st == 0) == served).all(), (what, hint)
        got, st, pn = run(kt, ref, w.open_desc, hint, True)
        assert (st == o_st).all(), (what, hint, "open status", np.nonzero(st != o_st)[0][:8], st[st != o_st][:8])
        assert got.tobytes() == back.tobytes(), (what, hint, "open")
        assert (pn[served] == o_pn[served]).all() and (pn[served] == w.pns[served]).all(), (what, hint)


def update(kt, model, first_row, rows):
    kt.update(first_row, rows)
    model[first_row:first_row + len(rows)] = [copy_km(r) for r in rows]


def start(orc, suites):
    model = [fresh(s) if s else empty() for s in suites]
    kt = KeyTable(model)
    model = [copy_km(m) for m in model]
    check(orc, kt, model, "created")
    return kt, model


def test_update_rows_and_suite_counts(orc):
    # non-AES rows of the table: 2 -> 1 -> 0 -> 1 -> 2, with the one row, a sub-range and the last row
    kt, model = start(orc, [AES, CHACHA, AES, CHACHA, AES, AES])
    update(kt, model, 2, [fresh(AES)])
    check(orc, kt, model, "one row")
    update(kt, model, 3, [fresh(AES), fresh(AES)])           # a sub-range: row 3 ChaCha20 -> AES, 2 -> 1
    check(orc, kt, model, "sub-range, one ChaCha20 row left")
    update(kt, model, 5, [fresh(AES)])
    check(orc, kt, model, "last row")
    update(kt, model, 1, [fresh(AES)])                       # 1 -> 0
    check(orc, kt, model, "no ChaCha20 row")
    update(kt, model, 4, [fresh(CHACHA)])                    # 0 -> 1: row 4 is the single non-AES row
    check(orc, kt, model, "one ChaCha20 row again")
    update(kt, model, 0, [fresh(CHACHA)])                    # 1 -> 2
    check(orc, kt, model, "two ChaCha20 rows")
    update(kt, model, 0, [fresh(AES)])                       # 2 -> 1
    update(kt, model, 4, [empty()])                          # the single non-AES row is an empty one
    check(orc, kt, model, "the only non-AES row is empty")
    update(kt, model, 4, [fresh(CHACHA)])
    update(kt, model, 3, [empty()])                          # one ChaCha20 row and one empty row
    check(orc, kt, model, "a ChaCha20 row and an empty row")
    update(kt, model, 0, [fresh(CHACHA), fresh(CHACHA), fresh(CHACHA), fresh(AES), fresh(AES), fresh(CHACHA)])
    check(orc, kt, model, "every row at once")


@pytest.mark.parametrize("suite", [AES, CHACHA])
def test_update_rebuilds_the_row(orc, suite):
    # the same key with a new IV only (the round keys and GHASH powers stay, the nonce changes), then
    # a new key under the same IV (they must not stay)
    kt, model = start(orc, [AES, suite, CHACHA])
    cur = model[1]
    klen = 16 if suite == AES else 32
    nxt = copy_km(cur)
    ctypes.memmove(nxt.iv, _rng.bytes(12), 12)
    update(kt, model, 1, [nxt])
    check(orc, kt, model, "new iv")
    nxt = copy_km(nxt)
    ctypes.memmove(nxt.key, _rng.bytes(klen), klen)
    update(kt, model, 1, [nxt])
    check(orc, kt, model, "new key")
    nxt = copy_km(nxt)
    ctypes.memmove(nxt.hp, _rng.bytes(klen), klen)
    update(kt, model, 1, [nxt])
    check(orc, kt, model, "new hp key")


def test_update_after_rows_written_on_the_device(orc):
    kt, model = start(orc, [AES, CHACHA, 0, 0, AES, AES, 0])
    # derive_initial: rows 2 (client) and 3 (server) of one DCID
    dcid = bytes.fromhex("8394c8f03e515708")
    dc = np.zeros(20, dtype=np.uint8)
    dc[:8] = np.frombuffer(dcid, dtype=np.uint8)
    st = sentinel(1)
    batch.derive_initial(kt, 2, t(dc), t(np.array([8], dtype=np.uint8)), st)
    torch.cuda.synchronize()
    assert st.cpu().numpy()[0] == 0
    c, s = orc.derive_initial_secrets(dcid)
    model[2], model[3] = orc_km(orc, AES, c), orc_km(orc, AES, s)
    check(orc, kt, model, "derive_initial")
    update(kt, model, 3, [fresh(CHACHA)])
    check(orc, kt, model, "update after derive_initial")
    update(kt, model, 1, [fresh(AES)])  # one ChaCha20 row left (row 3), on a table with device-written rows
    check(orc, kt, model, "one ChaCha20 row after derive_initial")

    # derive_keys with row_idx: rows 6 and 0
    sec = _rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
    st = sentinel(2)
    batch.derive_keys(kt, CHACHA, t(sec), st, row_idx=u32([6, 0]))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    model[6], model[0] = orc_km(orc, CHACHA, sec[0].tobytes()), orc_km(orc, CHACHA, sec[1].tobytes())
    check(orc, kt, model, "derive_keys with row_idx")
    update(kt, model, 5, [fresh(CHACHA), fresh(AES)])
    check(orc, kt, model, "update after derive_keys")

    # key_update of row 0 in place
    secret = sec[1].copy()
    st = sentinel(1)
    batch.key_update(kt, t(secret), u32([0]), u32([0]), st)
    torch.cuda.synchronize()
    assert st.cpu().numpy()[0] == 0
    _, model[0] = orc_update(orc, secret.tobytes(), model[0])
    check(orc, kt, model, "key_update")
    update(kt, model, 0, [fresh(AES), fresh(AES)])
    check(orc, kt, model, "update after key_update")


def test_update_with_consecutive_derive_keys(orc):
    # consecutive rows written on the device keep the host view exact: the table goes to one ChaCha20
    # row by a derivation, and an update moves that row
    kt, model = start(orc, [CHACHA, AES, CHACHA, AES])
    sec = _rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
    st = sentinel(2)
    batch.derive_keys(kt, AES, t(sec), st, first_row=1)   # rows 1, 2 -> AES: row 0 is the one ChaCha20 row
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    model[1], model[2] = orc_km(orc, AES, sec[0].tobytes()), orc_km(orc, AES, sec[1].tobytes())
    check(orc, kt, model, "one ChaCha20 row by derivation")
    update(kt, model, 0, [fresh(AES)])
    update(kt, model, 3, [fresh(CHACHA)])
    check(orc, kt, model, "the ChaCha20 row moved")


def test_update_bounds(orc):
    kt, model = start(orc, [AES, CHACHA, AES, AES])
    for first, n in ((4, 1), (3, 2), (0, 5), (0xFFFFFFFF, 2)):
        with pytest.raises(crypto.InvalidArgument):
            kt.update(first, [fresh(CHACHA) for _ in range(n)])
    check(orc, kt, model, "refused updates")
    for first in (0, 2, 4):  # nothing to write, at any row up to the end
        kt.update(first, [])
    with pytest.raises(crypto.InvalidArgument):
        kt.update(5, [])
    check(orc, kt, model, "empty updates")
