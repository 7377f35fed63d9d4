"""Stream data on the GPU: mq_batch_stream_data and mq_batch_stream_read against the Python model
(stream_data_model.py) — stream tables, every byte of every stream buffer, events and their count equal,
guard bytes around every table untouched, the arena unchanged. The calls read frame records, so most tests
craft mq_recv_pkt / mq_dgram / mq_frame arrays directly; the chained test runs recv -> frames -> stream_data
on one stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, frames, recv  # noqa: E402
from milli_quic_amd import stream_data as sd  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

import frames_model as fm  # noqa: E402
import stream_data_model as m  # noqa: E402
from recv_traffic import assemble, build_traffic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = m.GUARD
ROW = sd.CONN_STREAMS_DTYPE.itemsize


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def guarded(a, pad=64):
    """The array's bytes on the device between two runs of guard bytes: (whole tensor, the inner view)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    whole = torch.full((len(raw) + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    whole[pad:pad + len(raw)] = torch.from_numpy(raw.copy()).to(DEV)
    return whole, whole[pad:pad + len(raw)]


def guards_ok(whole, pad=64):
    return bool((whole[:pad] == GUARD).all()) and bool((whole[-pad:] == GUARD).all())


def gpu_deliver(arena, pkts, n_pkts, dgrams, frs, n_frames, streams, bufs, stream_buf, initial_max, flags=0,
                max_frames=None):
    """One call over guarded tables. Returns (streams, bufs, evts) as the model does, and the whole event table."""
    max_frames = len(frs) if max_frames is None else max_frames
    n_conns = len(streams)
    ar_w, ar = guarded(arena)
    pk, dg, fr = t(pkts), t(dgrams), t(frs[:max_frames])
    np_d = torch.tensor([n_pkts], dtype=torch.int32, device=DEV)
    nf_d = torch.tensor([n_frames], dtype=torch.int32, device=DEV)
    st_w, st = guarded(streams, pad=ROW)
    bf_w, bf = guarded(bufs, pad=4096)
    ev_w, ev = guarded(np.full(max_frames * 32, GUARD, dtype=np.uint8))
    n_ev = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(sd.workspace_bytes(max_frames, n_conns), dtype=torch.uint8, device=DEV)
    sd.deliver(ar, pk, np_d, dg, fr, nf_d, st, bf, stream_buf, initial_max, ev, n_ev, ws, flags=flags)
    torch.cuda.synchronize()
    assert guards_ok(ar_w) and guards_ok(st_w, ROW) and guards_ok(bf_w, 4096) and guards_ok(ev_w)
    assert ar.cpu().numpy().tobytes() == np.ascontiguousarray(arena).tobytes()   # the arena is only read
    n = int(n_ev.cpu().numpy().view(np.uint32)[0])
    table = ev.cpu().numpy()
    assert n <= max_frames and (table[32 * n:] == GUARD).all()                    # nothing behind the last event
    return (st.cpu().numpy().view(sd.CONN_STREAMS_DTYPE), bf.cpu().numpy(), table[:32 * n].view(sd.EVT_DTYPE))


def same(got, want, name=""):
    g_st, g_bf, g_ev = got
    w_st, w_bf, w_ev = want
    assert len(g_ev) == len(w_ev), (name, len(g_ev), len(w_ev))
    bad = np.nonzero(g_ev.view(np.uint8).reshape(-1, 32) != w_ev.view(np.uint8).reshape(-1, 32))[0]
    assert len(bad) == 0, (name, bad[:4], g_ev[bad[:2]], w_ev[bad[:2]])
    bad = np.nonzero((g_st.view(np.uint8).reshape(-1, ROW) != w_st.view(np.uint8).reshape(-1, ROW)).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:8])
    bad = np.nonzero(g_bf != w_bf)[0]
    assert len(bad) == 0, (name, "buffer bytes", bad[:8], len(bad))


def both(recs, n_conns, pre, P, seed=0, name=""):
    arena, pkts, dg, fr = m.make_batch(recs, n_conns, seed)
    streams, bufs = m.state_rows(n_conns, P["stream_buf"], pre)
    args = (arena, pkts, len(pkts), dg, fr, len(fr), streams, bufs, P["stream_buf"], P["initial_max"],
            sd.CLIENT if P["client"] else 0)
    want = m.run(*args)
    got = gpu_deliver(*args)
    same(got, want, name)
    return args, got, want


def buffer_of(streams, bufs, stream_buf, conn, sid):
    row = streams[conn]["buf"]
    s = next(s for s in range(sd.SLOTS) if row[s]["used"] and row[s]["stream_id"] == sid)
    at = (conn * sd.SLOTS + s) * stream_buf
    return row[s], bufs[at:at + int(row[s]["len"])].tobytes()


# ---- 1. the reference's unit cases, each a one-connection batch ------------------------------------------
@pytest.mark.parametrize("case", m.REFERENCE_BUF_CASES, ids=[c[0] for c in m.REFERENCE_BUF_CASES])
def test_reference_buffer_cases(case):
    name, frames_, data, next_offset, fin = case
    P = dict(stream_buf=64, initial_max=65536, client=True)
    _, (st, bufs, ev), _ = both([m.S(0, 5, off, d, f) for off, d, f in frames_], 1, None, P, name=name)
    hdr, got = buffer_of(st, bufs, 64, 0, 5)
    assert got == data and hdr["next_offset"] == next_offset and bool(hdr["fin_received"]) == fin


def test_reference_stream_map_cases():
    P = dict(stream_buf=64, initial_max=65536, client=True)
    _, (st, _, ev), _ = both([m.S(0, 4, 0, 3)], 1, None, P)              # get_or_create_rejects_own_stream_type
    assert not st["map"]["flags"].any() and ev["mark"][0] == 0xFF
    _, (st, _, ev), _ = both([m.S(0, 5, 0, 3), m.S(0, 7, 0, 3), m.S(0, 5, 3, 3)], 1, None, P)  # peer bidi, uni, existing
    assert [int(x) for x in st["map"][0]["id"][:2]] == [5, 7] and list(ev["map_slot"]) == [0, 1, 0]
    assert list(st["map"][0]["flags"][:3]) == [sd.USED | sd.HAS_RECV | sd.HAS_SEND, sd.USED | sd.HAS_RECV, 0]
    assert (st["max_bidi_remote"][0], st["max_uni_remote"][0]) == (2, 2)
    _, (st, _, ev), _ = both([m.S(0, 5, 50, 50, True), m.S(0, 5, 100, 10)], 1, None, P)        # recv_data_past_fin_offset
    assert list(ev["mark"]) == [sd.MARK_OK, sd.STREAM_STATE_ERROR] and st["map"][0]["recv_state"][0] == sd.DATA_RECVD
    _, (st, _, ev), _ = both([m.S(0, 5, 0, 600)], 1, None, dict(P, stream_buf=1024, initial_max=1000))
    assert st["map"][0]["recv_max_data_next"][0] == 1600 and st["map"][0]["recv_max_data"][0] == 1000


# ---- 2. ladder ------------------------------------------------------------------------------------------
LADDER = m.ladder_cases()


@pytest.mark.parametrize("case", LADDER, ids=[c[0] for c in LADDER])
def test_ladder(case):
    name, n_conns, recs, pre, P = case
    _, (st, bufs, ev), _ = both(recs, n_conns, pre, P, name=name)
    if name == "flow_control_after_fin":
        e = st["map"][0][0]
        assert ev["mark"][1] == sd.FLOW_CONTROL_ERROR and ev["copy_len"][1] == 30
        assert (e["recv_state"], e["fin_offset"], e["recv_offset"]) == (sd.SIZE_KNOWN, 40, 10)
    if name == "full_buffer_then_fin":
        assert ev["copy_len"][1] == 0 and ev["flags"][1] & sd.TRUNCATED and ev["flags"][1] & sd.FIN_SET
    if name == "33_ids":
        assert list(ev["map_slot"][:33]) == list(range(32)) + [sd.NONE]
    if name == "33_buffers":
        assert list(ev["store"]) == [sd.STORE_NO_BUFFER, sd.STORE_COPIED, sd.STORE_NO_BUFFER]
    if name == "clamped_on_load":
        assert (st["buf"][0][0]["len"], st["buf"][0][0]["read_offset"]) == (64, 9)
    if name == "not_selected_each_kind":
        assert len(ev) == 2
    if name == "copy_65535":
        assert list(ev["copy_len"]) == [65535, 65535, 18]


def test_counts_are_read_on_the_device():
    recs = [m.S(0, 5, 5 * k, 5) for k in range(8)]
    P = dict(stream_buf=64, initial_max=65536, client=True)
    arena, pkts, dg, fr = m.make_batch(recs, 1, per_pkt=2)
    streams, bufs = m.state_rows(1, 64, None)
    for n_pkts, n_frames, max_frames, n_evts in ((len(pkts), 5, 8, 5), (len(pkts), 0, 8, 0), (len(pkts), 1000, 8, 8),
                                                 (2, 1000, 8, 4), (0, 8, 8, 0), (0x7FFFFFFF, 0x7FFFFFFF, 6, 6)):
        args = (arena, pkts, n_pkts, dg, fr[:max_frames], n_frames, streams, bufs, 64, 65536, sd.CLIENT)
        got = gpu_deliver(*args)
        same(got, m.run(*args), (n_pkts, n_frames, max_frames))
        assert len(got[2]) == n_evts


# ---- 3. state across calls --------------------------------------------------------------------------------
def test_state_across_calls():
    recs, pre, P = m.fuzz_batch(11, n_conns=16)
    arena, pkts, dg, fr = m.make_batch(recs, 16, 11)
    streams, bufs = m.state_rows(16, P["stream_buf"], pre)
    tail = (P["stream_buf"], P["initial_max"], sd.CLIENT)
    whole = gpu_deliver(arena, pkts, len(pkts), dg, fr, len(fr), streams, bufs, *tail)
    same(whole, m.run(arena, pkts, len(pkts), dg, fr, len(fr), streams, bufs, *tail))
    h = len(fr) // 2
    one = gpu_deliver(arena, pkts, len(pkts), dg, fr[:h], h, streams, bufs, *tail)
    two = gpu_deliver(arena, pkts, len(pkts), dg, fr[h:], len(fr) - h, one[0], one[1], *tail)
    assert two[0].tobytes() == whole[0].tobytes() and two[1].tobytes() == whole[1].tobytes()
    ev = np.concatenate([one[2], two[2]])
    ev["frame"][len(one[2]):] += h
    assert ev.tobytes() == whole[2].tobytes()


# ---- 4. fuzz against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_vs_model(seed):
    recs, pre, P = m.fuzz_batch(seed)
    args, got, want = both(recs, 40, pre, P, seed, name=f"seed {seed}")
    cov = m.fuzz_coverage(args[6], want[0], want[2])
    for k, v in cov.items():
        assert v >= (20 if k.startswith(("mark_", "store_")) else 1), (k, cov)
    again = gpu_deliver(*args)   # determinism: the same inputs again, byte for byte
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))


def test_fuzz_as_server():
    recs, pre, P = m.fuzz_batch(4, client=False)
    both(recs, 40, pre, P, 4, name="server")


# ---- 5. the read side -----------------------------------------------------------------------------------------
def gpu_read(streams, bufs, stream_buf, reqs, out):
    st_w, st = guarded(streams, pad=ROW)
    bf_w, bf = guarded(bufs, pad=4096)
    out_w, o = guarded(out, pad=256)
    res_w, rs = guarded(np.full(len(reqs) * 8, GUARD, dtype=np.uint8))
    ws = torch.empty(sd.read_workspace_bytes(len(reqs), len(streams)), dtype=torch.uint8, device=DEV)
    sd.read(st, bf, stream_buf, t(reqs), o, rs, ws)
    torch.cuda.synchronize()
    assert guards_ok(st_w, ROW) and guards_ok(bf_w, 4096) and guards_ok(out_w, 256) and guards_ok(res_w)
    assert bf.cpu().numpy().tobytes() == bufs.tobytes()       # the buffers are only read
    return st.cpu().numpy().view(sd.CONN_STREAMS_DTYPE), o.cpu().numpy(), rs.cpu().numpy().view(sd.READ_RES_DTYPE)


def same_read(got, want, name=""):
    assert got[2].tobytes() == want[2].tobytes(), (name, got[2], want[2])
    assert got[0].tobytes() == want[0].tobytes(), name
    bad = np.nonzero(got[1] != want[1])[0]
    assert len(bad) == 0, (name, bad[:8])


def test_read_cases():
    P = dict(stream_buf=64, initial_max=65536, client=True)
    recs = [m.S(0, 5, 0, 40), m.S(0, 9, 0, 10, True), m.S(1, 5, 0, 0, True), m.S(1, 9, 0, 7)]
    _, (st, bufs, _), _ = both(recs, 2, None, P)
    reqs = np.zeros(9, dtype=sd.READ_REQ_DTYPE)
    reqs["conn"] = [0, 0, 0, 1, 1, 1, 2, 0, 0]
    reqs["stream_id"] = [5, 9, 5, 5, 9, 13, 5, 9, 5]
    reqs["cap"] = [16, 64, 16, 8, 0, 8, 8, 8, 200]
    reqs["out_offset"] = [0, 16, 80, 96, 104, 104, 104, 104, 0]
    out = np.full(128, GUARD, dtype=np.uint8)
    got = gpu_read(st, bufs, 64, reqs, out)
    same_read(got, m.read(st, bufs, 64, reqs, out))
    assert list(got[2]["status"]) == [0, 0, _lib.MQ_ERR_DEFERRED, 0, 0, sd.WOULD_BLOCK, _lib.MQ_ERR_INVALID_ARG,
                                      _lib.MQ_ERR_DEFERRED, _lib.MQ_ERR_INVALID_ARG]
    assert list(got[2]["fin"][:4]) == [0, 1, 0, 1] and list(got[0]["buf"][0]["used"][:2]) == [1, 0]
    # the rest of stream 5 in two reads, then WouldBlock: no FIN was received
    st2 = got[0]
    for cap, copied, status in ((16, 16, 0), (64, 8, 0), (64, 0, sd.WOULD_BLOCK)):
        q = reqs[:1].copy()
        q["cap"] = cap
        g = gpu_read(st2, bufs, 64, q, out)
        same_read(g, m.read(st2, bufs, 64, q, out))
        assert (g[2]["copied"][0], g[2]["status"][0]) == (copied, status)
        st2 = g[0]


@pytest.mark.parametrize("seed", [1, 2])
def test_read_behind_fuzz(seed):
    recs, pre, P = m.fuzz_batch(seed)
    arena, pkts, dg, fr = m.make_batch(recs, 40, seed)
    streams, bufs = m.state_rows(40, P["stream_buf"], pre)
    st, bf, _ = m.run(arena, pkts, len(pkts), dg, fr, len(fr), streams, bufs, P["stream_buf"], P["initial_max"], sd.CLIENT)
    rng = np.random.default_rng(seed)
    used = [(c, s) for c in range(40) for s in range(sd.SLOTS) if st[c]["buf"][s]["used"]]
    pick = [used[i] for i in rng.integers(0, len(used), 3 * len(used) // 2)]     # some buffers twice: deferred
    reqs = np.zeros(len(pick) + 8, dtype=sd.READ_REQ_DTYPE)
    reqs["conn"][:len(pick)] = [c for c, _ in pick]
    reqs["stream_id"][:len(pick)] = [st[c]["buf"][s]["stream_id"] for c, s in pick]
    reqs["conn"][len(pick):] = [0, 1, 2, 3, 40, 41, m.CONN_NONE, 5]
    reqs["stream_id"][len(pick):] = 123456
    reqs["cap"] = rng.choice([0, 1, 15, 16, 17, 100, 511, 512, 513, 4096], len(reqs))
    reqs["out_offset"] = np.cumsum(reqs["cap"]) - reqs["cap"] + 3
    out = np.full(int(reqs["cap"].sum()) + 3 - 4096, GUARD, dtype=np.uint8)     # the last large ranges leave `out`
    want = m.read(st, bf, P["stream_buf"], reqs, out)
    for code in (0, _lib.MQ_ERR_DEFERRED, sd.WOULD_BLOCK, _lib.MQ_ERR_INVALID_ARG):
        assert (want[2]["status"] == code).sum() >= 4, code
    assert (want[2]["fin"] == 1).sum() >= 4
    got = gpu_read(st, bf, P["stream_buf"], reqs, out)
    same_read(got, want, f"seed {seed}")
    again = gpu_read(st, bf, P["stream_buf"], reqs, out)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))


# ---- 6. chained: recv -> frames -> stream_data -------------------------------------------------------------------
def test_chained_recv_frames_stream_data(orc):
    keys, conns, scripts = build_traffic(orc, seed=37, n_conns=8, n_app=40)
    rng = np.random.default_rng(37)
    for c, (dcid, rows, dgs) in enumerate(scripts):   # STREAM frames, two streams per connection, mostly in order
        cur = {1: 0, 7: 0}
        for parts in dgs:
            for q, part in enumerate(parts):
                body = b"\x01" + fm.build(0x10, (1 << 20,))   # never too short for the header-protection sample
                for sid in (1, 7):
                    n = int(rng.integers(0, 90))
                    off = cur[sid] + (7 if rng.random() < 0.1 else 0)
                    fin = rng.random() < 0.01
                    if rng.random() < 0.5:
                        body += fm.build(0x0e | int(fin), (sid, off, n), tail=rng.bytes(n))
                        if off == cur[sid]:
                            cur[sid] += n
                if rng.random() < 0.02:
                    body += fm.build(0x04, (7, 0, cur[7]))
                tailing = rng.bytes(int(rng.integers(1, 60)))
                body += fm.build(0x08, (1,), tail=tailing) if rng.random() < 0.3 else b""   # no OFF, no LEN: to the end
                parts[q] = part[:4] + (body,) + part[5:]
    arena, dgrams = assemble(orc, keys, conns, scripts, seed=37)
    n_conns, max_pkts, max_frames, stream_buf, initial_max = len(conns), 1 << 12, 1 << 13, 2048, 1 << 14
    oa, oc = arena.copy(), conns.copy()
    o_pk, o_n = orc.batch_recv(keys, oc, oa, dgrams, max_pkts)
    _, w_rec, _ = fm.run(oa, o_pk[:o_n], o_n, dgrams, n_conns)
    w_rec = np.asarray(w_rec, dtype=frames.FRAME_DTYPE)
    streams, bufs = m.state_rows(n_conns, stream_buf)
    want = m.run(oa, o_pk[:o_n], o_n, dgrams, w_rec, len(w_rec), streams, bufs, stream_buf, initial_max, sd.CLIENT)
    assert len(want[2]) > 150 and (want[2]["store"] == sd.STORE_COPIED).sum() > 60 and (want[2]["flags"] & sd.RESET).any()
    kt = KeyTable(keys)
    c_d, a_d, dg_d = t(conns), t(arena), t(dgrams)
    pk = torch.zeros(max_pkts * 32, dtype=torch.uint8, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    summ = torch.zeros(max_pkts * 16, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(max_frames * 48, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    st_d, bf_d = t(streams), t(bufs)
    ev = torch.full((max_frames * 32,), GUARD, dtype=torch.uint8, device=DEV)
    n_ev = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_r = torch.empty(recv.workspace_bytes(len(dgrams), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    ws_f = torch.empty(frames.workspace_bytes(max_pkts), dtype=torch.uint8, device=DEV)
    ws_s = torch.empty(sd.workspace_bytes(max_frames, n_conns), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    recv.recv(kt, c_d, a_d, dg_d, pk, n, ws_r)          # one stream, nothing read back in between
    frames.scan(a_d, pk, n, summ, rec, total, ws_f)
    sd.deliver(a_d, pk, n, dg_d, rec, total, st_d, bf_d, stream_buf, initial_max, ev, n_ev, ws_s, flags=sd.CLIENT)
    torch.cuda.synchronize()
    k = int(n_ev.cpu()[0])
    got = (st_d.cpu().numpy().view(sd.CONN_STREAMS_DTYPE), bf_d.cpu().numpy(), ev.cpu().numpy()[:32 * k].view(sd.EVT_DTYPE))
    same(got, want, "chained")
