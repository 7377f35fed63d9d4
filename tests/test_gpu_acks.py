"""ACKs on the GPU: mq_batch_acks against the Python model (acks_model.py) — trackers, pending bits,
the ACK count, frames, requests and next_pn equal, guard bytes around every table untouched. The call
reads packet records, so most tests craft mq_recv_pkt / mq_dgram / mq_pkt_frames arrays directly; the
chained test runs recv -> frames -> acks -> protect on one stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, acks, frames, recv, send  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

import acks_model as am  # noqa: E402
import frames_model as fm  # noqa: E402
from recv_traffic import assemble, build_traffic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5
TR = acks.TRACKER_DTYPE.itemsize


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
    h = whole.cpu().numpy()
    return (h[:pad] == GUARD).all() and (h[-pad:] == GUARD).all()


def default_build(n_conns, max_acks, flags=0):
    return dict(max_acks=max_acks, out_stride=96, flags=flags,
                largest_pn=[[1000 * c + 10 * lv + 1 for lv in range(3)] for c in range(n_conns)],
                next_pn=[(7 * k + 3) << (k % 40) for k in range(3 * n_conns)])


def gpu_acks(pkts, n_dev, dgrams, trackers, pending, summary=None, conn_flags=None, build=None, max_pkts=None):
    """One call over guarded tables. Returns (trackers, pending, out) as the model does, out with the raw
    frame slots beside the rest."""
    max_pkts = len(pkts) if max_pkts is None else max_pkts
    n_conns = len(pending)
    pk = t(pkts[:max_pkts])
    n = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    dg = t(dgrams)
    tr_w, tr = guarded(trackers, pad=TR)
    pe_w, pe = guarded(pending)
    summ = t(summary[:max_pkts]) if summary is not None else None
    cf = t(conn_flags.astype(np.uint32)) if conn_flags is not None else None
    ws = torch.empty(acks.workspace_bytes(max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    b = keep = None
    if build is not None:
        m = build["max_acks"]
        fr_w, fr = guarded(np.full(m * acks.FRAME_MAX, GUARD, dtype=np.uint8))
        rq_w, rq = guarded(np.full(m * 48, GUARD, dtype=np.uint8))
        np_w, nx = guarded(np.array(build["next_pn"], dtype=np.uint64))
        cn = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
        cn["largest_pn"] = np.array(build["largest_pn"], dtype=np.uint64).reshape(n_conns, 3)
        total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        b = acks.Build(fr, rq, total, t(cn), nx, build["out_stride"], build["flags"])
        keep = (fr_w, rq_w, np_w)
    acks.track_and_build(pk, n, dg, tr, pe, ws, summary=summ, conn_flags=cf, build=b)
    torch.cuda.synchronize()
    assert guards_ok(tr_w, TR) and guards_ok(pe_w)
    out = None
    if build is not None:
        assert all(guards_ok(w) for w in keep)
        out = dict(n_acks=int(total.cpu().numpy().view(np.uint32)[0]), slots=fr.cpu().numpy().reshape(m, acks.FRAME_MAX),
                   reqs=rq.cpu().numpy().view(send.REQ_DTYPE), next_pn=nx.cpu().numpy().view(np.uint64))
    return tr.cpu().numpy().view(acks.TRACKER_DTYPE), pe.cpu().numpy().view(np.uint32), out


def same(got, want, name=""):
    g_tr, g_pe, g_out = got
    w_tr, w_pe, w_out = want
    bad = np.nonzero((g_tr.view(np.uint8).reshape(-1, TR) != w_tr.view(np.uint8).reshape(-1, TR)).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:8], g_tr[bad[:2]], w_tr[bad[:2]])
    assert list(g_pe) == list(w_pe), name
    assert (g_out is None) == (w_out is None)
    if w_out is None:
        return
    assert g_out["n_acks"] == w_out["n_acks"], name
    assert g_out["reqs"].tobytes() == w_out["reqs"].tobytes(), (name, g_out["reqs"], w_out["reqs"])
    assert list(g_out["next_pn"]) == list(w_out["next_pn"]), name
    for k, slot in enumerate(g_out["slots"]):
        f = w_out["frames"][k] if k < len(w_out["frames"]) else b""
        assert slot[:len(f)].tobytes() == f, (name, k, slot[:len(f)].tobytes().hex(), f.hex())
        assert (slot[len(f):] == GUARD).all(), (name, k)   # nothing behind the frame, nothing in an unused slot


def both(events, n_conns, pre=None, pending=None, with_summary=True, with_flags=True, build="default", name="",
         fix=None):
    pkts, dg, summ, flags = am.make_batch(events, n_conns)
    rows = am.tracker_rows(n_conns, pre)
    if fix is not None:
        fix(rows)
    pend = np.zeros(n_conns, dtype=np.uint32) if pending is None else np.array(pending, dtype=np.uint32)
    b = default_build(n_conns, 3 * n_conns + 2) if build == "default" else build
    args = (pkts, len(pkts), dg, rows, pend, summ if with_summary else None, flags if with_flags else None, b)
    want = am.run(*args)
    got = gpu_acks(*args)
    same(got, want, name)
    return got, want


# ---- 1. the reference's unit cases, each a one-connection batch ------------------------------------------
@pytest.mark.parametrize("case", am.REFERENCE_CASES, ids=[c[0] for c in am.REFERENCE_CASES])
def test_reference_cases(case):
    name, pns, ranges = case
    got, want = both([(0, 0, pn) for pn in pns], 1, pending=[0] if pns else [1], build=default_build(1, 2, acks.CLIENT))
    assert am.load_tracker(got[0][0]).ranges == ranges
    if not pns:  # build_ack_frame_empty_tracker_returns_none: nothing built, the bit stays set
        assert got[2]["n_acks"] == 0 and list(got[1]) == [1] and got[2]["reqs"]["conn"][0] == am.CONN_NONE
    else:
        assert got[2]["n_acks"] == 1 and list(got[1]) == [0] and got[2]["slots"][0][0] == 0x02
        assert got[2]["reqs"]["flags"][0] == send.PAD_TO_MIN


# ---- 2. ladder --------------------------------------------------------------------------------------------
LADDER = am.ladder_cases()


@pytest.mark.parametrize("case", LADDER, ids=[c[0] for c in LADDER])
def test_ladder(case):
    name, n_conns, events, pre = case
    fix = None
    if name == "tracker_n_40":   # a tracker word above 32 is clamped on load
        def fix(rows):
            rows[1]["n"] = 40
    got, want = both(events, n_conns, pre, name=name, fix=fix)
    if name == "frame_515_bytes":
        assert got[2]["reqs"]["frame_len"][0] == 515
    if name == "tracker_n_40":
        assert got[0][1]["n"] == 32
    if name == "excluded_each_kind":
        assert am.load_tracker(got[0][2]).ranges == [(1, 1), (3, 3), (17, 17)]


def test_no_summary_records_the_frame_error_packet():
    ev = [(0, 2, 1), (0, 2, 5, "frame"), (0, 2, 9, "invalid"), (0, 2, 11, "status")]
    got, _ = both(ev, 1, with_summary=False)
    assert am.load_tracker(got[0][2]).ranges == [(1, 1), (5, 5), (9, 9)]
    got, _ = both(ev, 1, with_summary=True)
    assert am.load_tracker(got[0][2]).ranges == [(1, 1)]


def test_count_is_read_on_the_device():
    ev = [(0, 2, pn) for pn in (1, 2, 3, 9, 10, 20)]
    pkts, dg, summ, flags = am.make_batch(ev, 1)
    for n_dev, ranges in ((4, [(1, 3), (9, 9)]), (0, []), (1000, [(1, 3), (9, 10), (20, 20)])):
        args = (pkts, n_dev, dg, am.tracker_rows(1), np.zeros(1, np.uint32), summ, flags, default_build(1, 2))
        got = gpu_acks(*args)
        same(got, am.run(*args))
        assert am.load_tracker(got[0][2]).ranges == ranges


# ---- 3. state across calls --------------------------------------------------------------------------------
def test_state_across_calls():
    n_conns, events = am.fuzz_events(11, n_pkts=3000, big=1200)
    pkts, dg, summ, flags = am.make_batch(events, n_conns)
    zero = np.zeros(n_conns, np.uint32)
    whole = gpu_acks(pkts, len(pkts), dg, am.tracker_rows(n_conns), zero, summ, flags)
    same(whole, am.run(pkts, len(pkts), dg, am.tracker_rows(n_conns), zero, summ, flags))
    h = len(pkts) // 2
    _, _, _, f1 = am.make_batch(events[:h], n_conns)
    _, _, _, f2 = am.make_batch(events[h:], n_conns)
    one = gpu_acks(pkts[:h], h, dg, am.tracker_rows(n_conns), zero, summ[:h], f1)       # build = NULL: bits are set
    assert list(one[1]) == list(f1) and one[2] is None
    b = default_build(n_conns, 3 * n_conns)
    args = (pkts[h:], len(pkts) - h, dg, one[0], one[1], summ[h:], f2, b)
    two = gpu_acks(*args)                                                                # ... and built by call 2
    same(two, am.run(*args))
    assert two[0].tobytes() == whole[0].tobytes()
    assert (two[1] == 0).all() and two[2]["n_acks"] == int(sum(bin(int(x)).count("1") for x in whole[1]))


# ---- 4. capacity ------------------------------------------------------------------------------------------
def test_capacity():
    ev = [(c, lv, 10 * c + lv + q) for q in (0, 1, 5) for c in range(6) for lv in range(3) if (c + lv) % 4]
    due = len({(c, lv) for c, lv, _ in ev})
    pkts, dg, summ, flags = am.make_batch(ev, 6)
    b = default_build(6, 5)
    args = (pkts, len(pkts), dg, am.tracker_rows(6), np.zeros(6, np.uint32), summ, flags, b)
    got, want = gpu_acks(*args), am.run(*args)
    same(got, want)
    assert got[2]["n_acks"] == due > 5 and [(int(r["conn"]), int(r["level"])) for r in got[2]["reqs"]] == \
        sorted({(c, lv) for c, lv, _ in ev})[:5]
    rest = int(sum(bin(int(x)).count("1") for x in got[1]))
    assert rest == due - 5
    # the second call builds the remainder; its tail requests are null requests
    b2 = dict(b, next_pn=got[2]["next_pn"], max_acks=due)
    args = (pkts[:0], 0, dg, got[0], got[1], None, None, b2)
    got2, want2 = gpu_acks(*args, max_pkts=0), am.run(*args)
    same(got2, want2)
    assert got2[2]["n_acks"] == rest and (got2[1] == 0).all()
    tail = got2[2]["reqs"][rest:]
    assert (tail["conn"] == am.CONN_NONE).all() and (tail["frame_len"] == 0).all()
    # max_acks = 0: the count alone
    b0 = dict(b, max_acks=0)
    args = (pkts, len(pkts), dg, am.tracker_rows(6), np.zeros(6, np.uint32), summ, flags, b0)
    got0 = gpu_acks(*args)
    same(got0, am.run(*args))
    assert got0[2]["n_acks"] == due and list(got0[1]) == list(flags)


# ---- 5. fuzz against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_vs_model(seed):
    n_conns, events = am.fuzz_events(seed)
    pkts, dg, summ, flags = am.make_batch(events, n_conns)
    rng = np.random.default_rng(seed)
    pend = rng.integers(0, 8, n_conns).astype(np.uint32)
    b = default_build(n_conns, max(1, 2 * n_conns))
    args = (pkts, len(pkts), dg, am.tracker_rows(n_conns), pend, summ, flags, b)
    want = am.run(*args)
    assert (want[0]["n"] == 32).any() and 19000 < len(pkts) < 22000
    got = gpu_acks(*args)
    same(got, want, f"seed {seed}")
    # determinism: the same inputs again, byte for byte
    again = gpu_acks(*args)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    for f in ("slots", "reqs", "next_pn"):
        assert again[2][f].tobytes() == got[2][f].tobytes(), f
    assert again[2]["n_acks"] == got[2]["n_acks"]


# ---- 6. chained: recv -> frames -> acks -> protect ------------------------------------------------------------
def test_chained_recv_frames_acks_protect(orc):
    keys, conns, scripts = build_traffic(orc, seed=31, n_conns=8, n_app=40)
    for c, (dcid, rows, dgs) in enumerate(scripts):   # well-formed frame streams, so that packets get recorded
        for parts in dgs:
            for q, part in enumerate(parts):
                body = b"\x01" + fm.build(0x10, (1 << 20,)) if (c + part[3]) % 5 else fm.build(0x02, (3, 0, 0, 1))
                if (c + part[3]) % 17 == 16:
                    body = b"\x1f" + body             # an unknown frame type: MQ_ERR_FRAME, not recorded
                parts[q] = part[:4] + (body,) + part[5:]
    arena, dgrams = assemble(orc, keys, conns, scripts, seed=31)
    n_conns, max_pkts, max_frames, max_acks, stride = len(conns), 1 << 12, 1 << 13, 3 * len(conns) + 3, 1280
    # the oracle's records, the frame model's summaries and the ACK model over both
    oa, oc = arena.copy(), conns.copy()
    o_pk, o_n = orc.batch_recv(keys, oc, oa, dgrams, max_pkts)
    w_summ, _, w_flags = fm.run(oa, o_pk[:o_n], o_n, dgrams, n_conns)
    next_pn = [(1 << 21) + 17 * k for k in range(3 * n_conns)]
    b = dict(max_acks=max_acks, out_stride=stride, flags=acks.CLIENT, largest_pn=oc["largest_pn"], next_pn=next_pn)
    want = am.run(o_pk[:o_n], o_n, dgrams, am.tracker_rows(n_conns), np.zeros(n_conns, np.uint32), w_summ,
                  np.array(w_flags, dtype=np.uint32), b)
    n_acks = want[2]["n_acks"]
    assert (w_summ["status"] == fm.ERR_FRAME).sum() > 3 and 8 < n_acks < max_acks
    # the send side answers with the same keys: Initial, Handshake and the current 1-RTT generation
    s_conns = send.make_conns([bytes([c + 1] * 8) for c in range(n_conns)], [b"\x09\x08"] * n_conns,
                              [[int(conns[c]["initial_row"]), int(conns[c]["handshake_row"]), int(conns[c]["app_row"][1])]
                               for c in range(n_conns)])
    kt = KeyTable(keys)
    c_d, a_d, dg_d, sc_d = t(conns), t(arena), t(dgrams), t(s_conns)
    pk = torch.zeros(max_pkts * 32, dtype=torch.uint8, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    summ = torch.zeros(max_pkts * 16, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(max_frames * 48, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    cf = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
    trk = torch.zeros(3 * n_conns * TR, dtype=torch.uint8, device=DEV)
    pend = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
    fr = torch.full((max_acks * acks.FRAME_MAX,), GUARD, dtype=torch.uint8, device=DEV)
    rq = torch.zeros(max_acks * 48, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    nx = t(np.array(next_pn, dtype=np.uint64))
    out = torch.full((max_acks * stride,), GUARD, dtype=torch.uint8, device=DEV)
    st = torch.full((max_acks,), 0x77, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(max_acks, dtype=torch.int32, device=DEV)
    ws_r = torch.empty(recv.workspace_bytes(len(dgrams), max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    ws_f = torch.empty(frames.workspace_bytes(max_pkts), dtype=torch.uint8, device=DEV)
    ws_a = torch.empty(acks.workspace_bytes(max_pkts, n_conns), dtype=torch.uint8, device=DEV)
    ws_p = torch.empty(send.workspace_bytes(max_acks), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    recv.recv(kt, c_d, a_d, dg_d, pk, n, ws_r)          # one stream, nothing read back in between
    frames.scan(a_d, pk, n, summ, rec, total, ws_f, dgrams=dg_d, conn_flags=cf)
    acks.track_and_build(pk, n, dg_d, trk, pend, ws_a, summary=summ, conn_flags=cf,
                         build=acks.Build(fr, rq, cnt, c_d, nx, stride, acks.CLIENT))
    send.protect(kt, sc_d, fr, out, rq, st, ln, _lib.MQ_SUITE_MIXED, ws_p)
    torch.cuda.synchronize()
    got = (trk.cpu().numpy().view(acks.TRACKER_DTYPE), pend.cpu().numpy().view(np.uint32),
           dict(n_acks=int(cnt.cpu()[0]), slots=fr.cpu().numpy().reshape(max_acks, acks.FRAME_MAX),
                reqs=rq.cpu().numpy().view(send.REQ_DTYPE), next_pn=nx.cpu().numpy().view(np.uint64)))
    same(got, want, "chained")
    st_h, ln_h, out_h = st.cpu().numpy(), ln.cpu().numpy().view(np.uint32), out.cpu().numpy().reshape(max_acks, stride)
    assert (st_h[:n_acks] == 0).all() and (st_h[n_acks:] == _lib.MQ_ERR_INVALID_ARG).all()
    assert (out_h[n_acks:] == GUARD).all()               # the null requests' output bytes are untouched
    # every produced packet opens under the oracle with the expected PN; its payload is the model's frame
    # and the PADDING behind it
    reqs = want[2]["reqs"]
    peer = np.zeros(n_acks, dtype=recv.CONN_DTYPE)
    p_dg = np.zeros(n_acks, dtype=recv.DGRAM_DTYPE)
    for k in range(n_acks):
        c = int(reqs["conn"][k])
        peer[k]["initial_row"], peer[k]["handshake_row"] = conns[c]["initial_row"], conns[c]["handshake_row"]
        peer[k]["app_row"] = [0, conns[c]["app_row"][1], conns[c]["app_row"][2]]
        peer[k]["dcid_len"], peer[k]["flags"] = 8, recv.HAS_INITIAL | recv.HAS_HANDSHAKE | recv.HAS_APP
        peer[k]["largest_pn"] = int(reqs["pn"][k]) - 1
        p_dg[k] = (k * stride, int(ln_h[k]), k)
        assert (out_h[k, ln_h[k]:] == GUARD).all()
    flat = out_h.reshape(-1).copy()
    p_pk, p_n = orc.batch_recv(keys, peer, flat, p_dg, 2 * n_acks)
    assert p_n == n_acks and (p_pk["status"][:p_n] == 0).all()
    for k in range(n_acks):
        r = p_pk[k]
        assert (int(r["dgram"]), int(r["pn"]), int(r["level"])) == (k, int(reqs["pn"][k]), int(reqs["level"][k]))
        body = flat[int(r["offset"]) + int(r["payload_offset"]):int(r["offset"]) + int(r["len"]) - 16].tobytes()
        f = want[2]["frames"][k]
        assert body[:len(f)] == f and not any(body[len(f):])
        if r["level"] == 0:
            assert ln_h[k] >= 1200                        # MQ_ACKS_CLIENT: the ACK-only Initial is padded
