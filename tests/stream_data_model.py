"""Python model of mq_batch_stream_data and mq_batch_stream_read: Frame::Stream / Frame::ResetStream of
dispatch_frame (reference src/connection/recv.rs:620-644, 661-669), StreamMap::get_or_create, mark_recv
and handle_reset (src/transport/stream.rs:227-280, 325-388, 405-424), store_stream_data and stream_recv
(src/connection/mod.rs:769-842, 660-687), restated in their loop form as a sequential replay over numpy
records, plus the generators of the batches that the host replay, the GPU ladder and the fuzz share."""
import numpy as np

from milli_quic_amd import frames, recv
from milli_quic_amd import stream_data as sd

CONN_NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
VARINT_MAX = (1 << 62) - 1
GUARD = 0xA5


# ---- one entry, one buffer (plain dicts of ints) ---------------------------------------------------------
def new_entry(sid, initial_max):  # stream.rs:253-276, 129-137
    bidi = sid & 2 == 0
    return dict(id=sid, recv_offset=0, recv_max_data=initial_max, recv_max_data_next=initial_max, fin_offset=0,
                flags=sd.USED | sd.HAS_RECV | (sd.HAS_SEND if bidi else 0), recv_state=sd.RECV)


def local_entry(sid, initial_max=65536, bidi=True):  # open_bidi / open_uni, stream.rs:186-223
    e = new_entry(sid, initial_max)
    e["flags"] = sd.USED | sd.HAS_SEND | (sd.HAS_RECV if bidi else 0)
    return e


def mark_recv(e, offset, length, fin):  # stream.rs:325-388
    if not e["flags"] & sd.HAS_RECV:
        return sd.INVALID_STATE
    if e["recv_state"] not in (sd.RECV, sd.SIZE_KNOWN):
        return sd.STREAM_STATE_ERROR
    end = offset + length
    if e["flags"] & sd.HAS_FIN:
        if end > e["fin_offset"]:
            return sd.FINAL_SIZE_ERROR
        if fin and end != e["fin_offset"]:
            return sd.FINAL_SIZE_ERROR
    if fin:
        e["fin_offset"], e["recv_state"] = end, sd.SIZE_KNOWN
        e["flags"] |= sd.HAS_FIN
    if end > e["recv_max_data"]:
        return sd.FLOW_CONTROL_ERROR
    e["recv_offset"] = max(e["recv_offset"], end)
    if e["flags"] & sd.HAS_FIN and e["recv_offset"] >= e["fin_offset"]:
        e["recv_state"] = sd.DATA_RECVD
    remaining = max(e["recv_max_data"] - e["recv_offset"], 0)
    window = e["recv_max_data_next"]
    if remaining < window // 2:
        e["recv_max_data_next"] = (e["recv_offset"] + window) & M64  # wrapping, where the reference would overflow
    return sd.MARK_OK


def handle_reset(e, final_size):  # stream.rs:405-424
    if not e["flags"] & sd.HAS_RECV:
        return sd.INVALID_STATE
    if e["recv_state"] not in (sd.RECV, sd.SIZE_KNOWN, sd.DATA_RECVD):
        return sd.STREAM_STATE_ERROR
    if e["flags"] & sd.HAS_FIN and e["fin_offset"] != final_size:
        return sd.FINAL_SIZE_ERROR
    e["fin_offset"], e["recv_state"] = final_size, sd.RESET_RECVD
    e["flags"] |= sd.HAS_FIN
    return sd.MARK_OK


def store(b, offset, length, fin, stream_buf):
    """store_stream_data on its buffer (mod.rs:817-840): (store, flags, skip, copy_len, dst)."""
    if offset > b["next_offset"]:
        return sd.STORE_GAP, 0, 0, 0, 0
    if offset + length <= b["next_offset"]:
        if fin:
            b["fin_received"] = 1
        return sd.STORE_DUPLICATE, sd.FIN_SET if fin else 0, 0, 0, 0
    skip = b["next_offset"] - offset
    copy_len = min(length - skip, stream_buf - b["len"])
    dst = b["len"]
    b["len"] += copy_len
    b["next_offset"] += copy_len
    flags = sd.TRUNCATED if copy_len < length - skip else 0
    if fin:
        b["fin_received"] = 1
        flags |= sd.FIN_SET
    return sd.STORE_COPIED, flags, skip, copy_len, dst


ENTRY_FIELDS = ("id", "recv_offset", "recv_max_data", "recv_max_data_next", "fin_offset", "flags", "recv_state")
BUF_FIELDS = ("stream_id", "next_offset", "len", "read_offset", "used", "fin_received")


def load_conn(row, stream_buf):
    m = [{f: int(row["map"][s][f]) for f in ENTRY_FIELDS} for s in range(sd.SLOTS)]
    bufs = []
    for s in range(sd.SLOTS):
        b = {f: int(row["buf"][s][f]) for f in BUF_FIELDS}
        b["used"], b["fin_received"] = int(b["used"] != 0), int(b["fin_received"] != 0)
        b["len"] = min(b["len"], stream_buf)             # clamped on load
        b["read_offset"] = min(b["read_offset"], b["len"])
        bufs.append(b)
    return dict(map=m, buf=bufs, max_bidi_remote=int(row["max_bidi_remote"]), max_uni_remote=int(row["max_uni_remote"]))


def store_conn(row, c):  # whole, but never the reserved bytes
    for s in range(sd.SLOTS):
        for f in ENTRY_FIELDS:
            row["map"][s][f] = c["map"][s][f]
        for f in BUF_FIELDS:
            row["buf"][s][f] = c["buf"][s][f]
    row["max_bidi_remote"], row["max_uni_remote"] = c["max_bidi_remote"], c["max_uni_remote"]


def find(c, sid):
    return next((s for s, e in enumerate(c["map"]) if e["flags"] & sd.USED and e["id"] == sid), None)


def apply(c, ftype, sid, a, length, is_client, initial_max, stream_buf):
    """One selected record on a connection (recv.rs:620-644, 661-669): the event's decided fields."""
    o = dict(map_slot=sd.NONE, buf_slot=sd.NONE, mark=0xFF, store=sd.STORE_NONE, flags=0, skip=0, copy_len=0, dst=0)
    is_stream = ftype >= 0x08
    m = find(c, sid)
    if m is None and is_stream and (sid & 1) == (1 if is_client else 0):
        m = next((s for s, e in enumerate(c["map"]) if not e["flags"] & sd.USED), None)
        if m is not None:
            c["map"][m] = new_entry(sid, initial_max)
            key = "max_bidi_remote" if sid & 2 == 0 else "max_uni_remote"
            if sid // 4 >= c[key]:
                c[key] = sid // 4 + 1
            o["flags"] |= sd.NEW_STREAM
    if m is None:
        return o
    o["map_slot"] = m
    if not is_stream:
        o["mark"] = handle_reset(c["map"][m], a)
        o["flags"] |= sd.RESET
        return o
    fin = bool(ftype & 1)
    o["mark"] = mark_recv(c["map"][m], a, length, fin)
    o["flags"] |= sd.READABLE
    b = next((s for s, x in enumerate(c["buf"]) if x["used"] and x["stream_id"] == sid), None)
    if b is None:
        b = next((s for s, x in enumerate(c["buf"]) if not x["used"]), None)
        if b is None:
            o["store"] = sd.STORE_NO_BUFFER
            return o
        c["buf"][b] = dict(stream_id=sid, next_offset=0, len=0, read_offset=0, used=1, fin_received=0)
        o["flags"] |= sd.NEW_BUF
    o["buf_slot"] = b
    st, fl, skip, copy_len, dst = store(c["buf"][b], a, length, fin, stream_buf)
    o["store"] = st
    o["flags"] |= fl
    if st == sd.STORE_COPIED:
        o["skip"], o["copy_len"], o["dst"] = skip, copy_len, dst
    return o


# ---- the calls -------------------------------------------------------------------------------------------
def selected(arena_len, pkts, n_pkts, dgrams, frs, n_frames, n_conns):
    """(record index, conn, arena offset of the data) of every selected record, in record order."""
    n_p, n_f = min(int(n_pkts), len(pkts)), min(int(n_frames), len(frs))
    out = []
    for k in range(n_f):
        f = frs[k]
        t = int(f["type"])
        if not (t == 0x04 or 0x08 <= t <= 0x0f) or f["pkt"] >= n_p:
            continue
        p = pkts[int(f["pkt"])]
        if p["dgram"] >= len(dgrams):
            continue
        c = int(dgrams["conn"][p["dgram"]])
        if c >= n_conns:
            continue
        src = int(p["offset"]) + int(p["payload_offset"]) + int(f["data_pos"])
        if t != 0x04 and src + int(f["data_len"]) > arena_len:
            continue
        out.append((k, c, src))
    return out


def run(arena, pkts, n_pkts, dgrams, frs, n_frames, streams, bufs, stream_buf, initial_max, flags=0):
    """mq_batch_stream_data: returns (streams, bufs, evts) as new arrays, evts holding the events written."""
    streams, bufs = streams.copy(), bufs.copy()
    n_conns = len(streams)
    is_client = bool(flags & sd.CLIENT)
    conns, evts = {}, []
    for k, c, src in selected(len(arena), pkts, n_pkts, dgrams, frs, n_frames, n_conns):
        if c not in conns:
            conns[c] = load_conn(streams[c], stream_buf)
        f = frs[k]
        t = int(f["type"])
        a, length = (int(f["v"][2]), 0) if t == 0x04 else (int(f["v"][1]), int(f["data_len"]))
        o = apply(conns[c], t, int(f["v"][0]), a, length, is_client, initial_max, stream_buf)
        from_ = 0
        if o["store"] == sd.STORE_COPIED:
            from_ = src + o["skip"]
            at = (c * sd.SLOTS + o["buf_slot"]) * stream_buf + o["dst"]
            bufs[at:at + o["copy_len"]] = arena[from_:from_ + o["copy_len"]]
        evts.append((k, c, from_, o["dst"], o["copy_len"], o["skip"], o["map_slot"], o["buf_slot"], o["mark"],
                     o["store"], o["flags"], t, (0, 0)))
    for c, st in conns.items():  # a connection without records is left as it is
        store_conn(streams[c], st)
    return streams, bufs, np.array(evts, dtype=sd.EVT_DTYPE)


def read(streams, bufs, stream_buf, reqs, out):
    """mq_batch_stream_read: returns (streams, out, res) as new arrays."""
    before, streams, out = streams, streams.copy(), out.copy()  # every request names its buffer in the state before
    res = np.zeros(len(reqs), dtype=sd.READ_RES_DTYPE)
    claimed = set()
    for k, q in enumerate(reqs):
        c, cap, off = int(q["conn"]), int(q["cap"]), int(q["out_offset"])
        if c >= len(streams) or off > len(out) or cap > len(out) - off:
            res[k] = (0, 3, 0, sd.NONE, 0)                # MQ_ERR_INVALID_ARG
            continue
        row, was = streams[c]["buf"], before[c]["buf"]
        s = next((s for s in range(sd.SLOTS) if was[s]["used"] and was[s]["stream_id"] == q["stream_id"]), None)
        if s is None:
            res[k] = (0, sd.WOULD_BLOCK, 0, sd.NONE, 0)
            continue
        if (c, s) in claimed:
            res[k] = (0, 9, 0, s, 0)                      # MQ_ERR_DEFERRED
            continue
        claimed.add((c, s))
        ln = min(int(row[s]["len"]), stream_buf)
        ro = min(int(row[s]["read_offset"]), ln)
        fin_received = row[s]["fin_received"] != 0
        if ln == ro:
            if fin_received:
                row[s]["len"], row[s]["read_offset"], row[s]["used"] = ln, ro, 0
                res[k] = (0, 0, 1, s, 0)
            else:
                res[k] = (0, sd.WOULD_BLOCK, 0, s, 0)
            continue
        n = min(ln - ro, cap)
        at = (c * sd.SLOTS + s) * stream_buf + ro
        out[off:off + n] = bufs[at:at + n]
        fin = fin_received and ro + n >= ln
        row[s]["len"], row[s]["read_offset"], row[s]["used"] = ln, ro + n, 0 if fin else 1
        res[k] = (n, 0, int(fin), s, 0)
    return streams, out, res


# ---- batches ---------------------------------------------------------------------------------------------
def S(conn, sid, offset, data, fin=False, **kw):
    """A STREAM record: data is bytes, or a length (random bytes)."""
    return dict(kw, conn=conn, type=0x0e | int(fin), id=sid, a=offset, data=data)


def R(conn, sid, final_size, **kw):
    return dict(kw, conn=conn, type=0x04, id=sid, a=final_size, data=b"")


def other(conn, ftype, sid=5):
    """A record of another type with a stream id in v[0]: ignored."""
    return dict(conn=conn, type=ftype, id=sid, a=0, data=8)


def make_batch(recs, n_conns, seed=0, per_pkt=3):
    """Crafted device inputs for a list of records: (arena, pkts, dgrams, frames). Up to per_pkt records of
    one connection share a packet; the data sits at every byte alignment between filler bytes. A record's
    `bad` says why it must not be selected: "pkt", "dgram", "conn" or "arena"."""
    rng = np.random.default_rng(1000 + seed)
    chunks, pos = [], 0
    pk, fr = [], []
    dg = np.zeros(n_conns + 1, dtype=recv.DGRAM_DTYPE)
    dg["conn"] = list(range(n_conns)) + [CONN_NONE]
    dg["len"] = 1200

    def filler(n):
        nonlocal pos
        chunks.append(rng.integers(0, 256, n, dtype=np.uint8))
        pos += n

    open_pkt = {}  # conn -> [pkt index, records so far, payload position]
    for r in recs:
        data = r["data"]
        if not isinstance(data, (bytes, bytearray)):
            data = rng.integers(0, 256, int(data), dtype=np.uint8).tobytes()
        bad = r.get("bad")
        # the records of a packet are laid out back to back in the arena, so a packet stays open only while
        # its connection's records follow each other
        cur = open_pkt.get(r["conn"])
        if bad or cur is None or cur[0] != len(pk) - 1 or cur[1] >= per_pkt or cur[2] + len(data) + 40 > 60000:
            filler(int(rng.integers(0, 38)))
            po = int(rng.integers(1, 40))
            pk.append([pos, 0, po, r["conn"]])           # offset, len (patched below), payload_offset, dgram
            filler(po)
            cur = open_pkt[r["conn"]] = [len(pk) - 1, 0, 0]
        p = pk[cur[0]]
        head = int(rng.integers(1, 20))                  # the frame's own header bytes
        filler(head)
        data_pos = cur[2] + head
        chunks.append(np.frombuffer(data, dtype=np.uint8))
        pos += len(data)
        cur[1] += 1
        cur[2] = data_pos + len(data)
        p[1] = p[2] + cur[2] + 16
        v = (r["id"], r["a"], 0, 0) if r["type"] != 0x04 else (r["id"], 7, r["a"], 0)
        pkt = cur[0]
        if bad == "pkt":
            pkt = 1 << 30
        elif bad == "dgram":
            p[3] = 1 << 20
        elif bad == "conn":
            p[3] = n_conns
        fr.append((pkt, data_pos - head, min(head + len(data), 0xFFFF), r["type"], 2, data_pos, len(data), 0, v))
        if bad == "arena":
            p[0] = -1                                    # patched below: the data range leaves the arena by a byte
            p.append(data_pos + len(data))
        if bad:
            del open_pkt[r["conn"]]
    filler(16 + int(rng.integers(0, 38)))
    arena = np.concatenate(chunks)
    pkts = np.zeros(len(pk), dtype=recv.PKT_DTYPE)
    for i, p in enumerate(pk):
        off = p[0] if p[0] >= 0 else len(arena) - p[2] - p[4] + 1
        pkts[i]["offset"], pkts[i]["len"], pkts[i]["payload_offset"], pkts[i]["dgram"] = off, p[1], p[2], p[3]
        pkts[i]["level"], pkts[i]["pn"] = 2, i
    return arena, pkts, dg, np.array(fr, dtype=frames.FRAME_DTYPE)


def state_rows(n_conns, stream_buf, pre=None):
    """(streams, bufs) for n_conns connections: zero state, bufs guard-filled, with `pre` seeded:
    {conn: dict(map={slot: entry}, buf={slot: (stream_id, next_offset, data, read_offset, fin_received)})}."""
    streams = np.zeros(n_conns, dtype=sd.CONN_STREAMS_DTYPE)
    bufs = np.full(n_conns * sd.SLOTS * stream_buf, GUARD, dtype=np.uint8)
    for c, st in (pre or {}).items():
        for s, e in st.get("map", {}).items():
            for f in ENTRY_FIELDS:
                streams[c]["map"][s][f] = e[f]
        for s, (sid, nxt, data, ro, fin) in st.get("buf", {}).items():
            streams[c]["buf"][s] = (sid, nxt, len(data), ro, 1, fin, (0,) * 6)
            at = (c * sd.SLOTS + s) * stream_buf
            bufs[at:at + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        for f in ("max_bidi_remote", "max_uni_remote"):
            streams[c][f] = st.get(f, 0)
    return streams, bufs


# ---- the reference's unit cases, values restated ----------------------------------------------------------
# stream_recv_buf_tests (mod.rs:2116-2198): (name, [(offset, data, fin)], buffer bytes, next_offset, fin_received)
REFERENCE_BUF_CASES = [
    ("in_order_data_appended", [(0, b"hello", False)], b"hello", 5, False),
    ("gap_drops_frame", [(0, b"hello", False), (10, b"world", False)], b"hello", 5, False),
    ("duplicate_data_skipped", [(0, b"hello", False), (0, b"hello", False)], b"hello", 5, False),
    ("partial_overlap_appends_new_tail", [(0, b"hel", False), (1, b"ello", False)], b"hello", 5, False),
    ("sequential_in_order_frames", [(0, b"hel", False), (3, b"lo ", False), (6, b"world", True)], b"hello world", 11,
     True),
    ("fin_on_duplicate_is_recorded", [(0, b"done", False), (0, b"done", True)], b"done", 4, True),
]


# ---- ladder ----------------------------------------------------------------------------------------------
def ladder_cases():
    """(name, n_conns, records, pre, params); params = dict(stream_buf, initial_max, client)."""
    P = dict(stream_buf=64, initial_max=1 << 16, client=True)
    big = dict(P, initial_max=VARINT_MAX)
    out = []

    def case(name, recs, pre=None, n_conns=1, **kw):
        out.append((name, n_conns, recs, pre, dict(P, **kw)))

    case("in_order", [S(0, 5, 0, 7), S(0, 5, 7, 21), S(0, 5, 28, 1)])
    case("duplicate", [S(0, 5, 0, 9), S(0, 5, 0, 9), S(0, 5, 3, 4)])
    case("overlap_new_tail", [S(0, 5, 0, 9), S(0, 5, 4, 17), S(0, 5, 25, 3), S(0, 5, 1, 30)])
    case("gap", [S(0, 5, 0, 5), S(0, 5, 10, 5), S(0, 5, 5, 5), S(0, 5, 1, 0)])
    case("fin_on_duplicate", [S(0, 5, 0, 4), S(0, 5, 0, 4, True)])
    case("fin_on_gap_not_set", [S(0, 5, 0, 4), S(0, 5, 9, 4, True)])
    for room in (0, 1, 16):
        case(f"room_{room}", [S(0, 5, 0, 64 - room), S(0, 5, 64 - room, 40), S(0, 5, 64, 3)])
    case("full_buffer_then_fin", [S(0, 5, 0, 64), S(0, 5, 64, 9, True), S(0, 5, 64, 9, True)])
    case("data_len_0", [S(0, 5, 0, 0), S(0, 5, 0, 6), S(0, 5, 6, 0), S(0, 5, 3, 0), S(0, 5, 6, 0, True), S(0, 9, 0, 0, True)])
    case("end_at_varint_max", [S(0, 5, VARINT_MAX - 30, 30), S(0, 9, VARINT_MAX - 20, 20, True), S(0, 9, 0, 5)],
         {0: dict(buf={3: (9, VARINT_MAX - 20, b"abc", 1, 0)})}, **big)
    case("flow_control_after_fin", [S(0, 5, 0, 10), S(0, 5, 10, 30, True), S(0, 5, 40, 0)], initial_max=32)
    # a FIN offset above recv_offset in state SizeKnown is what the FlowControlError path leaves behind
    case("final_size_beyond_fin", [S(0, 5, 0, 10), S(0, 5, 10, 30, True), S(0, 5, 10, 31), S(0, 5, 10, 30)],
         initial_max=32)
    case("final_size_other_fin", [S(0, 5, 0, 10), S(0, 5, 10, 30, True), S(0, 5, 10, 5, True), S(0, 5, 10, 30, True)],
         initial_max=32)
    case("reset_then_stream", [S(0, 5, 0, 4), R(0, 5, 20), S(0, 5, 4, 6), R(0, 5, 20)])
    case("reset_other_final_size", [S(0, 5, 0, 4, True), R(0, 5, 9), R(0, 5, 4), S(0, 9, 0, 3), S(0, 9, 8, 2, True), R(0, 9, 11)])
    case("reset_unknown_id", [R(0, 5, 0), R(0, 4, 0), S(0, 5, 0, 3)])
    case("own_id_as_client", [S(0, 4, 0, 5), S(0, 6, 0, 5), S(0, 5, 0, 5), S(0, 7, 0, 5)])
    case("own_id_as_server", [S(0, 5, 0, 5), S(0, 7, 0, 5), S(0, 4, 0, 5), S(0, 6, 0, 5)], client=False)
    case("seeded_local_bidi", [S(0, 4, 0, 5), S(0, 4, 5, 5, True)], {0: dict(map={2: local_entry(4)})})
    case("seeded_local_uni_no_recv", [S(0, 6, 0, 5), R(0, 6, 5), S(0, 6, 5, 5)], {0: dict(map={1: local_entry(6, bidi=False)})})
    ids33 = [4 * k + 1 + 2 * (k % 2) for k in range(33)]
    case("33_ids", [S(0, i, 0, 3) for i in ids33] + [S(0, ids33[32], 0, 3), R(0, ids33[32], 3), S(0, ids33[7], 3, 3)])
    full = {0: dict(buf={s: (4 * s + 1001, 4, b"full", 0, 0) for s in range(32)})}
    case("33_buffers", [S(0, 5, 0, 3), S(0, 1001, 4, 3), S(0, 5, 3, 3, True)], full)
    case("buf_slot_differs", [S(0, 5, 0, 3), S(0, 9, 0, 3), S(0, 5, 3, 3)],
         {0: dict(buf={0: (77, 0, b"", 0, 0), 2: (81, 0, b"", 0, 0)}, map={0: local_entry(8)})})
    case("remote_counters", [S(0, 41, 0, 1), S(0, 5, 0, 1), S(0, 83, 0, 1), S(0, 7, 0, 1)],
         {0: dict(max_bidi_remote=3, max_uni_remote=30)})
    case("auto_tune", [S(0, 5, 0, 600), S(0, 5, 600, 300)], stream_buf=1024, initial_max=1000)
    case("auto_tune_wraps", [S(0, 4, 0, 10)],
         {0: dict(map={0: dict(local_entry(4), recv_max_data=100, recv_max_data_next=M64 - 3)})})
    case("clamped_on_load", [S(0, 5, 12, 8)], {0: dict(buf={0: (5, 12, b"x" * 64, 9, 0)})})
    case("not_selected_each_kind", [S(0, 5, 0, 4), other(0, 0x05), other(0, 0x11), other(0, 0x06), other(0, 0x10),
                                    S(0, 5, 4, 4, bad="pkt"), S(0, 5, 4, 4, bad="dgram"), S(0, 5, 4, 4, bad="conn"),
                                    S(0, 5, 4, 4, bad="arena"), S(0, 5, 4, 5)])
    case("untouched_connection", [S(0, 5, 0, 4), S(2, 5, 0, 4)], {1: dict(buf={0: (5, 99, b"keep", 9, 3)})}, n_conns=3)
    # every source / destination alignment, chunk counts around the lanes of a copy group
    align, offs = [], {}
    for k, n in enumerate([1, 15, 16, 17, 31, 33, 47, 63, 64, 65, 255, 257, 511, 513, 1023, 1025, 2047, 2049, 4099] + list(range(1, 49))):
        sid = 5 + 4 * (k % 5)
        align.append(S(k % 2, sid, offs.get((k % 2, sid), 0), n))
        offs[(k % 2, sid)] = offs.get((k % 2, sid), 0) + n
    case("copy_alignments", align, n_conns=2, stream_buf=8192, initial_max=1 << 20)
    case("copy_65535", [S(0, 5, 0, 65535), S(0, 5, 65535, 65535), S(0, 5, 131070, 70)], stream_buf=131088,
         initial_max=1 << 20)
    return out


# ---- fuzz ------------------------------------------------------------------------------------------------
def fuzz_batch(seed, n_conns=40, client=True):
    """(records, pre, params): interleaved per-stream scripts over connections of several kinds."""
    rng = np.random.default_rng(seed)
    params = dict(stream_buf=512, initial_max=1024, client=client)
    peer = 1 if client else 0
    pre, per_conn = {}, []
    for c in range(n_conns):
        kind = ("plain", "plain", "many", "bufs_full", "shifted", "local", "plain", "resets")[c % 8]
        ids = [4 * int(k) + peer + 2 * int(rng.integers(0, 2)) for k in rng.choice(200, int(rng.integers(1, 7)), False)]
        if kind == "many":
            ids = [4 * k + peer + 2 * (k % 2) for k in range(int(rng.integers(36, 44)))]
        if kind == "bufs_full":
            pre[c] = dict(buf={s: (4 * s + 4000 + peer, 7, b"earlier", int(rng.integers(0, 8)), int(s % 2)) for s in range(32)})
            ids += [4000 + peer, 4004 + peer]
        if kind == "shifted":
            pre[c] = dict(buf={0: (4 * 999 + peer, 0, b"", 0, 0)}, max_bidi_remote=int(rng.integers(0, 300)))
        if kind == "local":
            mine = [4 * k + (1 - peer) for k in range(3)] + [4 * k + (1 - peer) + 2 for k in range(3)]
            pre[c] = dict(map={int(s): local_entry(i, 1024, bidi=i & 2 == 0) for s, i in zip((1, 4, 9, 12, 20, 31), mine)})
            ids += mine
        ids += [4 * int(rng.integers(0, 50)) + (1 - peer)]  # an own-initiated id nobody opened
        scripts = []
        for sid in ids:
            sc, cur, last = [], 0, (0, 1)
            n = int(rng.integers(2, 5)) if kind == "many" else int(rng.integers(3, 16))
            for q in range(n):
                u = rng.random()
                ln = int(rng.integers(0, 200)) if rng.random() < 0.9 else int(rng.integers(200, 700))
                if u < 0.55:
                    sc.append(S(c, sid, cur, ln))
                    last, cur = (cur, ln), cur + ln
                elif u < 0.67:
                    sc.append(S(c, sid, last[0], last[1], rng.random() < 0.3))
                elif u < 0.77 and cur:
                    back = int(rng.integers(0, min(cur, 100)))
                    sc.append(S(c, sid, cur - back, back + ln))
                    last, cur = (cur - back, back + ln), cur + ln
                elif u < 0.85:
                    sc.append(S(c, sid, cur + int(rng.integers(1, 50)), ln, rng.random() < 0.3))
                elif u < 0.89:                           # again from where a full buffer stalls
                    sc.append(S(c, sid, min(cur, params["stream_buf"]), ln + 1, rng.random() < 0.5))
                elif u < 0.94:
                    sc.append(S(c, sid, cur, ln, True))
                    last, cur = (cur, ln), cur + ln
                else:
                    sc.append(R(c, sid, cur + int(rng.integers(0, 2)) * 5))
            if kind == "resets" and rng.random() < 0.6:
                sc.insert(int(rng.integers(0, len(sc))), R(c, sid, int(rng.integers(0, 300))))
            scripts.append(sc)
        recs = []                                         # the connection's scripts, interleaved in order
        while scripts:
            k = int(rng.integers(0, len(scripts)))
            recs.append(scripts[k].pop(0))
            if not scripts[k]:
                scripts.pop(k)
        if rng.random() < 0.5:
            recs.insert(int(rng.integers(0, len(recs) + 1)), other(c, int(rng.choice([0x05, 0x06, 0x11]))))
        per_conn.append(recs)
    out = []                                              # the connections, interleaved in runs
    while per_conn:
        k = int(rng.integers(0, len(per_conn)))
        take = int(rng.integers(1, 6))
        out += per_conn[k][:take]
        del per_conn[k][:take]
        if not per_conn[k]:
            per_conn.pop(k)
    return out, pre, params


def fuzz_coverage(streams_before, streams, evts):
    """The conditions on the fuzz inputs that both test files assert, as a dict of counts."""
    cov = {f"mark_{m}": int((evts["mark"] == m).sum()) for m in (0, 1, 2, 3, 4, 0xFF)}
    cov.update({f"store_{s}": int((evts["store"] == s).sum()) for s in range(5)})
    map_full = ((streams["map"]["flags"] & sd.USED) != 0).all(axis=1)
    refused = {int(c) for c in evts["conn"][(evts["mark"] == 0xFF) & (evts["type"] >= 8)]}
    cov["map_full_and_refused"] = sum(1 for c in np.nonzero(map_full)[0] if int(c) in refused)
    buf_full = (streams_before["buf"]["used"] != 0).all(axis=1) | (streams["buf"]["used"] != 0).all(axis=1)
    no_buf = {int(c) for c in evts["conn"][evts["store"] == sd.STORE_NO_BUFFER]}
    cov["bufs_full_and_store_1"] = sum(1 for c in np.nonzero(buf_full)[0] if int(c) in no_buf)
    t = (evts["flags"] & sd.TRUNCATED != 0) & (evts["copy_len"] == 0) & (evts["flags"] & sd.FIN_SET != 0)
    cov["truncated_empty_fin"] = int(t.sum())
    has = evts["buf_slot"] != sd.NONE
    cov["slot_differs"] = int((evts["buf_slot"][has] != evts["map_slot"][has]).sum())
    return cov
