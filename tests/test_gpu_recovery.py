"""Loss recovery on the GPU: mq_batch_sent and mq_batch_recovery against the Python model (recovery_model.py) —
every byte of every state row, events, lost packets, both counts and the timeouts equal, guard bytes around
every table untouched, the arena unchanged. The calls read request and frame records, so most tests craft
mq_send_req / mq_recv_pkt / mq_dgram / mq_frame arrays directly; the chained test runs recv -> frames -> acks ->
protect -> sent -> recovery on one stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, acks, frames, recv, send  # noqa: E402
from milli_quic_amd import recovery as rc  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

import recovery_model as m  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = m.GUARD
ROW = rc.CONN_RECOVERY_DTYPE.itemsize
T_GUARD = 0xA5A5A5A5A5A5A5A5   # a timeout that was not written


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


def gpu_sent(reqs, status, pkt_len, now, rows):
    """One mq_batch_sent over guarded tables: (rows, timeouts) as the model returns them."""
    n_conns = len(rows)
    rw_w, rw = guarded(rows, pad=ROW)
    to_w, to = guarded(np.full(n_conns, T_GUARD, dtype=np.uint64))
    ws = torch.empty(rc.sent_workspace_bytes(len(reqs), n_conns), dtype=torch.uint8, device=DEV)
    rc.sent(t(reqs), t(status), t(pkt_len), t(now), rw, ws, timeouts=to)
    torch.cuda.synchronize()
    assert guards_ok(rw_w, ROW) and guards_ok(to_w)
    return rw.cpu().numpy().view(rc.CONN_RECOVERY_DTYPE), to.cpu().numpy().view(np.uint64)


def gpu_recovery(arena, pkts, n_pkts, dgrams, now, frs, n_frames, drop, rows, flags=0, max_frames=None, max_lost=256):
    """One mq_batch_recovery over guarded tables: (rows, evts, lost written, timeouts, n_lost)."""
    max_frames = len(frs) if max_frames is None else max_frames
    n_conns = len(rows)
    ar_w, ar = guarded(arena)
    pk, dg, fr, nw = t(pkts), t(dgrams), t(frs[:max_frames]), t(now)
    np_d = torch.tensor([n_pkts], dtype=torch.int32, device=DEV)
    nf_d = torch.tensor([n_frames], dtype=torch.int32, device=DEV)
    rw_w, rw = guarded(rows, pad=ROW)
    ev_w, ev = guarded(np.full(max_frames * 32, GUARD, dtype=np.uint8))
    lo_w, lo = guarded(np.full(max_lost * 16, GUARD, dtype=np.uint8))
    to_w, to = guarded(np.full(n_conns, T_GUARD, dtype=np.uint64))
    n_ev = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    n_lo = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(rc.workspace_bytes(max_frames, n_conns), dtype=torch.uint8, device=DEV)
    rc.process(ar, pk, np_d, dg, nw, fr, nf_d, rw, ev, n_ev, lo, n_lo, ws, drop_mask=None if drop is None else t(np.array(drop, np.uint8)),
               timeouts=to, flags=flags)
    torch.cuda.synchronize()
    assert guards_ok(ar_w) and guards_ok(rw_w, ROW) and guards_ok(ev_w) and guards_ok(lo_w) and guards_ok(to_w)
    assert ar.cpu().numpy().tobytes() == np.ascontiguousarray(arena).tobytes()   # the arena is only read
    n = int(n_ev.cpu().numpy().view(np.uint32)[0])
    total = int(n_lo.cpu().numpy().view(np.uint32)[0])
    table, ltable = ev.cpu().numpy(), lo.cpu().numpy()
    kept = min(total, max_lost)
    assert n <= max_frames and (table[32 * n:] == GUARD).all() and (ltable[16 * kept:] == GUARD).all()
    return (rw.cpu().numpy().view(rc.CONN_RECOVERY_DTYPE), table[:32 * n].view(rc.EVT_DTYPE),
            ltable[:16 * kept].view(rc.LOST_DTYPE), to.cpu().numpy().view(np.uint64), total)


def same_rows(got, want, name=""):
    bad = np.nonzero((got.view(np.uint8).reshape(-1, ROW) != want.view(np.uint8).reshape(-1, ROW)).any(axis=1))[0]
    if len(bad):
        c = int(bad[0])
        diff = [f for f in rc.CONN_RECOVERY_DTYPE.names if got[c][f].tobytes() != want[c][f].tobytes()]
        slots = np.nonzero(got[c]["sent"] != want[c]["sent"])[0][:4] if "sent" in diff else []
        assert False, (name, "rows", bad[:8], diff, [(f, got[c][f], want[c][f]) for f in diff if f != "sent"][:4],
                       [(int(s), got[c]["sent"][s], want[c]["sent"][s]) for s in slots])


def same(got, want, name="", max_lost=256):
    g_rows, g_ev, g_lost, g_to, g_total = got
    w_rows, w_ev, w_lost, w_to = want
    assert len(g_ev) == len(w_ev), (name, len(g_ev), len(w_ev))
    bad = np.nonzero(g_ev.view(np.uint8).reshape(-1, 32) != w_ev.view(np.uint8).reshape(-1, 32))[0]
    assert len(bad) == 0, (name, bad[:4], g_ev[bad[:2]], w_ev[bad[:2]])
    assert g_total == len(w_lost), (name, g_total, len(w_lost))
    assert g_lost.tobytes() == w_lost[:max_lost].tobytes(), (name, g_lost[:4], w_lost[:4])
    same_rows(g_rows, w_rows, name)
    assert g_to.tobytes() == w_to.tobytes(), (name, g_to, w_to)


def timeouts0(n):
    return np.full(n, T_GUARD, dtype=np.uint64)


def both(n, pre, sends, recs, drop, flags, seed=0, name="", rows=None):
    """Sends (if any), then the records, on the device and in the model. Returns the model's inputs and both results."""
    rows = m.state_rows(n, pre) if rows is None else rows
    if sends:
        s_args = m.make_sends(sends)
        w_rows, w_to = m.run_sent(*s_args, rows, timeouts0(n))
        g_rows, g_to = gpu_sent(*s_args, rows)
        same_rows(g_rows, w_rows, name + " sent")
        assert g_to.tobytes() == w_to.tobytes(), (name, "sent timeouts", g_to, w_to)
        rows = g_rows
    arena, pkts, dg, now, fr = m.make_batch(recs, n, seed)
    args = (arena, pkts, len(pkts), dg, now, fr, len(fr), drop, rows, flags)
    want = m.run_recovery(*args, timeouts0(n))
    got = gpu_recovery(*args)
    same(got, want, name)
    return args, got, want


# ---- 1. ladder ------------------------------------------------------------------------------------------------
LADDER = m.ladder_cases()


@pytest.mark.parametrize("case", LADDER, ids=[c[0] for c in LADDER])
def test_ladder(case):
    name, n, pre, sends, recs, drop, flags = case
    _, (rows, ev, lost, to, total), _ = both(n, pre, sends, recs, drop, flags, name=name)
    c, base = n - 1, name.rsplit("-", 1)[0]
    assert (to[:c] == T_GUARD).all()                      # the connections without records: no timeout written
    if base == "send_129th":
        assert rows[c]["count"] == 128 and rows[c]["bytes_in_flight"] == 128 * 1200 + 1300
    if base == "acked_33":
        assert (ev["n_acked"][0], ev["n_acked_cc"][0], rows[c]["bytes_in_flight"]) == (33, 32, 1200)
    if base == "lost_65":
        assert (ev["n_lost"][0], ev["flags"][0] & rc.LOST_CUT, rows[c]["have"] & rc.HAVE_LOSS_TIME << 2) == (64, rc.LOST_CUT, 0)
    if base == "lost_65_timer_before_break":
        assert rows[c]["loss_time"][2] == 3990
    if base == "pairs_17":
        assert (ev["n_acked"][0], ev["flags"][0] & rc.RANGES_CUT) == (17, rc.RANGES_CUT)
    if base == "arena_end_one_past":
        assert len(ev) == 0 and rows[c]["count"] == 20
    if base == "duplicate_pn_lost_later_slot":
        assert [(int(p["pn"]), int(p["size"])) for p in lost] == [(7, 111)]
    if base == "drop_mask_alone":
        assert (rows[c]["count"], total, to[c]) == (5, 0, 1040 + 1_024_000)
    if base == "handshake_done_then_ack_client":
        assert rows[c]["flags"] & rc.CONFIRMED and rows[c]["smoothed_rtt"] == 109_375 and rows[c]["count"] == 0


# ---- 2. overflow and device counts ----------------------------------------------------------------------------------
def test_lost_overflow_and_device_counts():
    pre = {c: m.seed_sent([(i, 2, 1000 + i, 100 + i) for i in range(30)]) for c in range(3)}
    recs = [m.A(c, 2, 9 + 10 * k, 0, now=5000 + k) for k in range(3) for c in range(3)]    # 9 ACKs, 7 or 9 losses each
    rows = m.state_rows(3, pre)
    arena, pkts, dg, now, fr = m.make_batch(recs, 3)
    full = m.run_recovery(arena, pkts, len(pkts), dg, now, fr, len(fr), None, rows, 0, timeouts0(3))
    assert len(full[2]) == 3 * 25 and list(full[1]["lost_first"][:4]) == [0, 7, 14, 21]
    for max_lost in (0, 1, 20, 74, 75):
        got = gpu_recovery(arena, pkts, len(pkts), dg, now, fr, len(fr), None, rows, 0, max_lost=max_lost)
        same(got, full, f"max_lost {max_lost}", max_lost=max_lost)
        assert got[4] == 75 and len(got[2]) == max_lost
    for n_pkts, n_frames, max_frames, n_evts in ((len(pkts), 5, 9, 5), (len(pkts), 0, 9, 0), (len(pkts), 1000, 9, 9), (4, 1000, 9, 4),
                                                 (0, 9, 9, 0), (0x7FFFFFFF, 0x7FFFFFFF, 6, 6)):
        args = (arena, pkts, n_pkts, dg, now, fr[:max_frames], n_frames, None, rows, 0)
        got = gpu_recovery(*args)
        same(got, m.run_recovery(*args, timeouts0(3)), (n_pkts, n_frames, max_frames))
        assert len(got[1]) == n_evts


# ---- 3. state across calls, determinism ---------------------------------------------------------------------------------
def test_state_across_calls():
    _, sends, recs, drop, flags = m.fuzz_batch(11, n_conns=16, n_sends=600, n_acks=200)
    hs, hr = len(sends) // 2, len(recs) // 2

    def sequence():
        rows, out = m.state_rows(16), []
        for s, r, d in ((sends[:hs], recs[:hr], drop), (sends[hs:], recs[hr:], None)):
            s_args = m.make_sends(s)
            rows, to = gpu_sent(*s_args, rows)
            out.append((rows, to))
            arena, pkts, dg, now, fr = m.make_batch(r, 16, 11)
            got = gpu_recovery(arena, pkts, len(pkts), dg, now, fr, len(fr), d, rows, flags)
            out.append(got)
            rows = got[0]
        return out

    rows = m.state_rows(16)
    want = []
    for s, r, d in ((sends[:hs], recs[:hr], drop), (sends[hs:], recs[hr:], None)):
        rows, to = m.run_sent(*m.make_sends(s), rows, timeouts0(16))
        want.append((rows, to))
        arena, pkts, dg, now, fr = m.make_batch(r, 16, 11)
        w = m.run_recovery(arena, pkts, len(pkts), dg, now, fr, len(fr), d, rows, flags, timeouts0(16))
        want.append(w)
        rows = w[0]
    got = sequence()
    for k in (0, 2):
        same_rows(got[k][0], want[k][0], f"sent {k}")
        assert got[k][1].tobytes() == want[k][1].tobytes()
    for k in (1, 3):
        same(got[k], want[k], f"recovery {k}")
    assert len(want[3][1]) > 30 and len(want[1][2]) + len(want[3][2]) > 20
    again = sequence()   # determinism: the whole sequence from the same inputs, byte for byte
    for a, b in zip(again, got):
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- 4. fuzz against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_vs_model(seed):
    pre, sends, recs, drop, flags = m.fuzz_batch(seed)
    cov = {}
    rows1, _ = m.run_sent(*m.make_sends(sends), m.state_rows(64), None, cov)
    args, got, want = both(64, pre, sends, recs, drop, flags, seed, name=f"seed {seed}")
    m.run_recovery(*args, None, cov)
    assert 450 < len(want[1]) and len(want[2]) > 100, (len(want[1]), len(want[2]))
    for what in ("full_tracker", "rtt_sample", "pn_threshold_loss", "time_threshold_loss", "loss_timer", "recovery_entry",
                 "ack_slow_start", "ack_recovery", "ack_avoidance"):
        assert cov.get(what, 0) >= 1, (what, cov)
    assert (want[1]["flags"] & rc.RANGES_CUT).any() and (want[1]["flags"] & rc.RANGES_BROKE).any()
    again = gpu_recovery(*args)   # determinism: the same inputs again, byte for byte
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, got))


# ---- 5. chained: recv -> frames -> acks -> protect -> sent -> recovery ---------------------------------------------------
def test_chained(orc):
    inp, w_rows1, want, cov = m.chained_expectation(orc)
    n_conns, max_pkts, max_acks, stride = len(inp["conns"]), inp["max_pkts"], inp["max_acks"], inp["stride"]
    max_frames, max_lost = 1 << 13, 1 << 10
    kt = KeyTable(inp["keys"])
    c_d, a_d, dg_d, sc_d = t(inp["conns"]), t(inp["arena"]), t(inp["dgrams"]), t(inp["s_conns"])
    now_d, sent_now_d = t(inp["now"]), t(inp["sent_now"])
    pk = torch.zeros(max_pkts * 32, dtype=torch.uint8, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    summ = torch.zeros(max_pkts * 16, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(max_frames * 48, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    cf = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
    trk = torch.zeros(3 * n_conns * acks.TRACKER_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    pend = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
    fr = torch.full((max_acks * acks.FRAME_MAX,), GUARD, dtype=torch.uint8, device=DEV)
    rq = torch.zeros(max_acks * 48, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    nx = t(np.array(inp["next_pn"], dtype=np.uint64))
    out = torch.full((max_acks * stride,), GUARD, dtype=torch.uint8, device=DEV)
    st = torch.full((max_acks,), 0x77, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(max_acks, dtype=torch.int32, device=DEV)
    rw_w, rw = guarded(inp["rows"], pad=ROW)
    to = t(np.full(n_conns, 7, dtype=np.uint64))
    ev = torch.full((max_frames * 32,), GUARD, dtype=torch.uint8, device=DEV)
    lo = torch.full((max_lost * 16,), GUARD, dtype=torch.uint8, device=DEV)
    n_ev = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_lo = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_r = torch.empty(recv.workspace_bytes(len(inp["dgrams"]), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    ws_f = torch.empty(frames.workspace_bytes(max_pkts), dtype=torch.uint8, device=DEV)
    ws_a = torch.empty(acks.workspace_bytes(max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    ws_p = torch.empty(send.workspace_bytes(max_acks), dtype=torch.uint8, device=DEV)
    ws_s = torch.empty(rc.sent_workspace_bytes(max_acks, n_conns), dtype=torch.uint8, device=DEV)
    ws_c = torch.empty(rc.workspace_bytes(max_frames, n_conns), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    recv.recv(kt, c_d, a_d, dg_d, pk, n, ws_r)          # one stream, nothing read back in between
    frames.scan(a_d, pk, n, summ, rec, total, ws_f, dgrams=dg_d, conn_flags=cf)
    acks.track_and_build(pk, n, dg_d, trk, pend, ws_a, summary=summ, conn_flags=cf,
                         build=acks.Build(fr, rq, cnt, c_d, nx, stride, acks.CLIENT))
    send.protect(kt, sc_d, fr, out, rq, st, ln, _lib.MQ_SUITE_MIXED, ws_p)
    rc.sent(rq, st, ln, sent_now_d, rw, ws_s, timeouts=to)
    rc.process(a_d, pk, n, dg_d, now_d, rec, total, rw, ev, n_ev, lo, n_lo, ws_c, timeouts=to, flags=rc.CLIENT)
    torch.cuda.synchronize()
    assert guards_ok(rw_w, ROW) and int(cnt.cpu()[0]) == inp["n_acks"]
    k, total_lost = int(n_ev.cpu()[0]), int(n_lo.cpu()[0])
    got = (rw.cpu().numpy().view(rc.CONN_RECOVERY_DTYPE), ev.cpu().numpy()[:32 * k].view(rc.EVT_DTYPE),
           lo.cpu().numpy()[:16 * min(total_lost, max_lost)].view(rc.LOST_DTYPE), to.cpu().numpy().view(np.uint64), total_lost)
    same(got, want, "chained", max_lost=max_lost)
    assert got[0][0]["count"] < 128 and cov["full_tracker"] >= 1
