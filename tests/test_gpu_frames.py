"""The frame index on the GPU: mq_batch_frames against the Python model (frames_model.py) — every
summary field, every record, the total and the connection flags equal, the arena untouched. The
call reads plaintext, so most tests lay fabricated mq_recv_pkt records over a plaintext arena; the
chained tests run it behind mq_batch_recv on one stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, frames, recv  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

import frames_model as fm  # noqa: E402
from recv_traffic import assemble, build_traffic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def gpu_scan(arena, pkts, n_dev, max_frames, dgrams=None, n_conns=0, max_pkts=None, extra_conn_words=0):
    """One call. Returns (summary of all max_pkts entries, the max_frames records, total, conn_flags
    with their guard words, the arena afterwards, the record buffer's guard bytes)."""
    max_pkts = len(pkts) if max_pkts is None else max_pkts
    a, pk = t(arena), t(pkts[:max_pkts]) if max_pkts else torch.zeros(0, dtype=torch.uint8, device=DEV)
    if max_pkts > len(pkts):
        pk = torch.cat([t(pkts), torch.zeros((max_pkts - len(pkts)) * 32, dtype=torch.uint8, device=DEV)])
    n = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    summ = torch.full((max_pkts * 16,), GUARD, dtype=torch.uint8, device=DEV)
    rec = torch.full(((max_frames + 2) * 48,), GUARD, dtype=torch.uint8, device=DEV)
    total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(frames.workspace_bytes(max_pkts), dtype=torch.uint8, device=DEV)
    dg = cf = None
    if dgrams is not None:
        dg = t(dgrams)
        cf = torch.full((n_conns + extra_conn_words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    frames.scan(a, pk, n, summ, rec[:max_frames * 48], total, ws, dgrams=dg,
                conn_flags=cf[:n_conns] if cf is not None else None)
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    return (summ.cpu().numpy().view(frames.PKT_FRAMES_DTYPE), r[:max_frames * 48].view(frames.FRAME_DTYPE),
            int(total.cpu().numpy().view(np.uint32)[0]), None if cf is None else cf.cpu().numpy().view(np.uint32),
            a.cpu().numpy(), r[max_frames * 48:])


def check(got, want, n_pkts, max_frames=None):
    summ, rec, total = got[0], got[1], got[2]
    w_summ, w_rec, _ = want
    assert total == len(w_rec)
    for f in frames.PKT_FRAMES_DTYPE.names:
        bad = np.nonzero(summ[f][:n_pkts] != w_summ[f][:n_pkts])[0]
        assert len(bad) == 0, (f, bad[:8], summ[bad[:4]], w_summ[bad[:4]])
    k = len(w_rec) if max_frames is None else min(max_frames, len(w_rec))
    for f in frames.FRAME_DTYPE.names if k else ():
        bad = np.nonzero((rec[f][:k] != w_rec[f][:k]).reshape(k, -1).any(axis=1))[0]
        assert len(bad) == 0, (f, bad[:8], rec[bad[:4]], w_rec[bad[:4]])
    assert (got[5] == GUARD).all()


# ---- 1. ladder -------------------------------------------------------------------------------------
# The host table has about 2 450 payloads, most of them a few bytes long; each at all 16 alignments
# makes about 44 k packets in 2.6 MB of arena: one call, and half a second of model.
@pytest.fixture(scope="module")
def ladder():
    base = fm.host_cases()
    payloads, aligns = [], []
    for c in base:                               # the host table, each case at all 16 arena alignments
        for al in range(16):
            payloads.append(c)
            aligns.append(al)
    for k, c in enumerate(fm.padding_cases()):
        payloads.append(c)
        aligns.append((5 * k) % 16)
    for al in range(16):                         # payload lengths 0 and 1 at every alignment
        payloads += [b"", b"\x01", b"\x00", b"\x40"]
        aligns += [al] * 4
    # behind every 9th packet one that did not open: its bytes are poison that would decode as frames
    poison = fm.build(0x06, (3, 5), b"\x01" * 5) + b"\x01\x1c\x01\x02\x00" + bytes(3) + b"\x1f"
    mixed, mixed_al, dead = [], [], []
    for k, (c, al) in enumerate(zip(payloads, aligns)):
        mixed.append(c)
        mixed_al.append(al)
        if k % 9 == 4:
            dead.append(len(mixed))
            mixed.append(poison[:1 + k % len(poison)])
            mixed_al.append(k % 16)
    arena, pkts = fm.lay_out(mixed, mixed_al)
    pkts["status"][dead] = [[_lib.MQ_ERR_CRYPTO, _lib.MQ_ERR_DEFERRED, _lib.MQ_ERR_PROTOCOL][i % 3] for i in dead]
    # the last packet ends on the arena's last byte; two records leave the arena
    tail = fm.build(0x06, (7, 30), bytes(30)) + bytes(40) + b"\x01"
    last = np.zeros(3, dtype=recv.PKT_DTYPE)
    last[0]["offset"], last[0]["len"], last[0]["payload_offset"] = len(arena), 9 + len(tail) + 16, 9
    arena = np.concatenate([arena, np.frombuffer(b"\xAA" * 9 + tail + b"\xAA" * 16, dtype=np.uint8)])
    last[1]["offset"], last[1]["len"], last[1]["payload_offset"] = len(arena) - 20, 21, 2      # one byte too far
    last[2]["offset"], last[2]["len"], last[2]["payload_offset"] = len(arena) + 1, 20, 2       # starts outside
    pkts = np.concatenate([pkts, last])
    extra = np.zeros(2, dtype=recv.PKT_DTYPE)     # a header that leaves no room for the tag; a valid empty payload
    extra[0]["offset"], extra[0]["len"], extra[0]["payload_offset"] = 0, 20, 5
    extra[1]["offset"], extra[1]["len"], extra[1]["payload_offset"] = 0, 21, 5
    pkts = np.concatenate([pkts, extra])
    want = fm.run(arena, pkts, len(pkts))
    return arena, pkts, want


def test_ladder(ladder):
    arena, pkts, want = ladder
    assert len(pkts) >= 16 * len(fm.host_cases())  # about 40 k small packets, 3 MB of arena, one call
    st = want[0]["status"]
    assert (st == fm.OK).sum() > 1000 and (st == fm.ERR_FRAME).sum() > 1000 and (st == fm.SKIPPED).sum() > 4000
    assert list(st[-5:]) == [fm.OK, fm.INVALID, fm.INVALID, fm.INVALID, fm.OK]
    assert want[0]["n_frames"].max() == 300 and want[0]["n_padding"].max() >= 1100
    got = gpu_scan(arena, pkts, len(pkts), len(want[1]) + 16)
    check(got, want, len(pkts))
    assert got[4].tobytes() == arena.tobytes()


# ---- 2. capacity and count ---------------------------------------------------------------------------
def test_capacity_and_count(ladder):
    arena, pkts, want = ladder
    total = len(want[1])
    cap = total // 3
    got = gpu_scan(arena, pkts, len(pkts), cap)                       # max_frames below the total
    check(got, want, len(pkts), max_frames=cap)
    again = gpu_scan(arena, pkts, len(pkts), cap)                     # two runs, identical output
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and got[2] == again[2]
    check(gpu_scan(arena, pkts, len(pkts), 0), want, len(pkts), max_frames=0)
    # *n_pkts_dev above max_pkts: the first max_pkts packets; below: the summaries beyond stay untouched
    m = 1000
    w = fm.run(arena, pkts[:m], m)
    check(gpu_scan(arena, pkts, len(pkts) + 77, len(w[1]), max_pkts=m), w, m)
    got = gpu_scan(arena, pkts, m, len(w[1]))
    check(got, w, m)
    assert (got[0].view(np.uint8).reshape(-1, 16)[m:] == GUARD).all()
    # zero packets: by the device count, and by max_pkts
    got = gpu_scan(arena, pkts, 0, 4)
    assert got[2] == 0 and (got[0].view(np.uint8) == GUARD).all() and (got[1].view(np.uint8) == GUARD).all()
    got = gpu_scan(arena, pkts, 5, 4, max_pkts=0)
    assert got[2] == 0 and (got[1].view(np.uint8) == GUARD).all()


# ---- 3. connection flags ---------------------------------------------------------------------------
def test_connection_flags():
    close = fm.build(0x1C, (1, 2, 0))
    ack = fm.build(0x02, (5, 0, 0, 1))
    # (payload, level, conn)
    rows = [(b"\x01", 0, 0), (ack, 1, 0), (b"\x01", 2, 0),                      # conn 0: levels 0 and 2
            (ack + bytes(9), 0, 1), (ack, 2, 1),                                # conn 1: nothing elicits
            (b"\x01" + close, 1, 2),                                            # conn 2: close at level 1
            (b"\x01" + close + b"\x3f", 2, 3),                                  # conn 3: close, then an error
            (b"\x01\x1f", 0, 4), (b"\x01", 1, 4),                               # conn 4: an error and a clean packet
            (b"\x01" + close, 2, _lib.MQ_CONN_NONE), (b"\x1f", 2, 7),           # no connection; beyond n_conns
            (fm.build(0x1D, (3, 0)), 0, 6)]                                     # conn 6: application close
    arena, pkts = fm.lay_out([r[0] for r in rows], level=0)
    pkts["level"] = [r[1] for r in rows]
    dg = np.zeros(len(rows) + 1, dtype=recv.DGRAM_DTYPE)
    dg["conn"][:len(rows)] = [r[2] for r in rows]
    dg["conn"][len(rows)] = 5
    pkts = np.concatenate([pkts, pkts[:2]])
    pkts[-2]["dgram"] = len(rows) + 5        # a datagram index beyond n_dgrams is ignored
    pkts[-1]["dgram"], pkts[-1]["status"] = len(rows), _lib.MQ_ERR_CRYPTO   # conn 5: only a packet that did not open
    n_conns = 7
    want = fm.run(arena, pkts, len(pkts), dg, n_conns)
    assert list(want[2]) == [0b101, 0, 0b1010, 0b11000, 0b10010, 0, 0b1001]
    got = gpu_scan(arena, pkts, len(pkts), 64, dgrams=dg, n_conns=n_conns, extra_conn_words=2)
    check(got, want, len(pkts))
    assert list(got[3][:n_conns]) == list(want[2]) and list(got[3][n_conns:]) == [0x5A5A5A5A] * 2


# ---- 4. seeded differential fuzz ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_vs_model(seed):
    payloads = fm.fuzz_batch(seed, 3000)
    rng = np.random.default_rng(100 + seed)
    arena, pkts = fm.lay_out(payloads, aligns=[int(x) for x in rng.integers(0, 16, len(payloads))], gap=0)
    dg = np.zeros(len(pkts), dtype=recv.DGRAM_DTYPE)
    dg["conn"] = rng.integers(0, 40, len(pkts))
    want = fm.run(arena, pkts, len(pkts), dg, 32)
    st = want[0]["status"]
    assert (st == fm.OK).sum() >= 750 and (st == fm.ERR_FRAME).sum() >= 750
    got = gpu_scan(arena, pkts, len(pkts), len(want[1]), dgrams=dg, n_conns=32)
    check(got, want, len(pkts))
    assert list(got[3]) == list(want[2])
    assert got[4].tobytes() == arena.tobytes()


# ---- 5. chained behind mq_batch_recv -----------------------------------------------------------------
def chain(keys_or_kt, conns, arena, dgrams, max_pkts, max_frames, before=None):
    kt = keys_or_kt if isinstance(keys_or_kt, KeyTable) else KeyTable(keys_or_kt)
    c, a, dg = t(conns), t(arena), t(dgrams)
    pk = torch.zeros(max_pkts * recv.PKT_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(recv.workspace_bytes(len(dgrams), max_pkts, len(conns)), dtype=torch.uint8, device=DEV)
    summ = torch.zeros(max_pkts * 16, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(max_frames * 48, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    cf = torch.zeros(len(conns), dtype=torch.int32, device=DEV)
    ws_f = torch.empty(frames.workspace_bytes(max_pkts), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    if before is not None:
        before(kt)
    recv.recv(kt, c, a, dg, pk, n, ws)              # one stream, nothing read back in between
    frames.scan(a, pk, n, summ, rec, total, ws_f, dgrams=dg, conn_flags=cf)
    torch.cuda.synchronize()
    return (summ.cpu().numpy().view(frames.PKT_FRAMES_DTYPE), rec.cpu().numpy().view(frames.FRAME_DTYPE),
            int(total.cpu()[0]), cf.cpu().numpy().view(np.uint32), None, np.full(1, GUARD, dtype=np.uint8))


def test_chained_behind_recv(orc):
    keys, conns, scripts = build_traffic(orc, seed=21, n_conns=8, n_app=40)
    arena, dgrams = assemble(orc, keys, conns, scripts, seed=21)
    oa = arena.copy()
    o_pk, o_n = orc.batch_recv(keys, conns.copy(), oa, dgrams, 1 << 12)
    want = fm.run(oa, o_pk[:o_n], o_n, dgrams, len(conns))   # the model over the oracle's plaintext
    assert (want[0]["status"] == fm.SKIPPED).sum() > 0 and (want[0]["status"] != fm.SKIPPED).sum() > 300
    got = chain(keys, conns, arena, dgrams, 1 << 12, len(want[1]) + 8)
    check(got, want, o_n)
    assert list(got[3]) == list(want[2])


def test_chained_rfc9001_a2(ref_fixtures):
    fx = ref_fixtures["rfc9001"]
    arena = np.frombuffer(bytes.fromhex(fx["a2_protected"]), dtype=np.uint8).copy()
    dcid = bytes.fromhex(fx["dcid"])
    dgrams = np.zeros(1, dtype=recv.DGRAM_DTYPE)
    dgrams[0] = (0, len(arena), 0)
    conns = np.zeros(1, dtype=recv.CONN_DTYPE)
    conns[0]["initial_row"], conns[0]["flags"], conns[0]["dcid_len"] = 0, recv.HAS_INITIAL, 8

    def derive(kt):
        d = np.zeros(20, dtype=np.uint8)
        d[:len(dcid)] = list(dcid)
        st = torch.zeros(1, dtype=torch.uint8, device=DEV)
        derive.keep = (t(d), t(np.array([len(dcid)], dtype=np.uint8)), st)
        batch.derive_initial(kt, 0, derive.keep[0], derive.keep[1], st)

    kt = KeyTable([_lib.KeyMaterial(), _lib.KeyMaterial()])
    summ, rec, total, cf, _, _ = chain(kt, conns, arena, dgrams, 4, 8, before=derive)
    assert total == 1 and summ[0]["status"] == fm.OK and summ[0]["n_frames"] == 1 and summ[0]["flags"] == 1
    r = rec[0]
    assert (r["pkt"], r["pos"], r["type"], r["level"], r["data_len"]) == (0, 0, 0x06, 0, 241)
    assert list(r["v"]) == [0, 0, 0, 0] and r["len"] == r["data_pos"] + 241
    assert summ[0]["n_padding"] == 1162 - int(r["len"]) and list(cf) == [0b001]
