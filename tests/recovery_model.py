"""Python model of mq_batch_sent and mq_batch_recovery: a literal restatement of the reference's
SentPacketTracker (src/transport/recovery.rs), LossDetector (src/transport/loss.rs) and
CongestionController (src/transport/congestion.rs), and of the two arms that drive them: the sent-packet
bookkeeping of build_*_packet (src/connection/transmit.rs:610-619) and Frame::Ack / Frame::HandshakeDone in
dispatch_frame (src/connection/recv.rs:563-612, 692-704). Slot array of 128, caps of 16 / 32 / 64, integer
arithmetic with u64 saturation where the reference saturates. The runners take the same arrays as the
device calls."""
import numpy as np

from milli_quic_amd import frames, recv, send
from milli_quic_amd import recovery as rc

U64 = (1 << 64) - 1
CONN_NONE = 0xFFFFFFFF
GUARD = 0xA5
N_SLOTS, MAX_PAIRS, MAX_NEWLY_ACKED, MAX_LOST = 128, 16, 32, 64
TIME_NUM, TIME_DEN, PACKET_THRESHOLD, GRANULARITY, INITIAL_RTT = 9, 8, 3, 1_000, 333_000
ALL_FLAGS = rc.USED | rc.ACK_ELICITING | rc.IN_FLIGHT


def sat_sub(a, b):
    return a - b if a > b else 0


# ---- recovery.rs ---------------------------------------------------------------------------------------
class SentPacket:
    def __init__(self, pn, level, time_sent, size, flags=ALL_FLAGS):
        self.pn, self.level, self.time_sent, self.size, self.flags = pn, level, time_sent, size, flags

    ack_eliciting = property(lambda self: bool(self.flags & rc.ACK_ELICITING))
    in_flight = property(lambda self: bool(self.flags & rc.IN_FLIGHT))


class AckResult:
    def __init__(self):
        self.newly_acked, self.largest_newly_acked, self.n_removed = [], None, 0
        self.broke = False


class SentPacketTracker:
    def __init__(self, n=N_SLOTS):
        self.entries, self.count = [None] * n, 0

    def on_packet_sent(self, pkt):  # recovery.rs:49-66
        for i, slot in enumerate(self.entries):
            if slot is None:
                self.entries[i] = pkt
                self.count += 1
                return True
        return False

    def on_ack_received(self, level, largest_ack, first_ack_range, ranges):  # recovery.rs:70-128
        result = AckResult()
        first_lo = sat_sub(largest_ack, first_ack_range)
        acked_ranges = [(first_lo, largest_ack)]
        smallest = first_lo
        for gap, ack_range in ranges:
            if smallest < gap + 2:
                result.broke = True
                break
            range_largest = smallest - gap - 2
            range_smallest = sat_sub(range_largest, ack_range)
            acked_ranges.append((range_smallest, range_largest))
            smallest = range_smallest
        for i, pkt in enumerate(self.entries):
            if pkt is None or pkt.level != level:
                continue
            if any(lo <= pkt.pn <= hi for lo, hi in acked_ranges):
                if len(result.newly_acked) < MAX_NEWLY_ACKED:   # heapless push, result dropped
                    result.newly_acked.append(pkt)
                if result.largest_newly_acked is None or pkt.pn > result.largest_newly_acked.pn:
                    result.largest_newly_acked = pkt
                result.n_removed += 1
                self.entries[i] = None
                self.count -= 1
        return result

    def sent_below_pn(self, level, threshold):  # recovery.rs:139-144
        return [p for p in self.entries if p is not None and p.level == level and p.pn < threshold]

    def remove(self, level, pn):  # recovery.rs:147-159
        for i, pkt in enumerate(self.entries):
            if pkt is not None and pkt.level == level and pkt.pn == pn:
                self.entries[i] = None
                self.count -= 1
                return pkt
        return None

    def drop_space(self, level):  # recovery.rs:162-171
        for i, pkt in enumerate(self.entries):
            if pkt is not None and pkt.level == level:
                self.entries[i] = None
                self.count -= 1

    def has_ack_eliciting_in_flight(self, level):  # recovery.rs:179-184
        return any(p is not None and p.level == level and p.ack_eliciting and p.in_flight for p in self.entries)


# ---- loss.rs ---------------------------------------------------------------------------------------------
class LossDetector:
    def __init__(self, max_ack_delay_us):
        self.largest_acked = [None] * 3
        self.smoothed_rtt_, self.rttvar, self.min_rtt, self.latest_rtt = None, 0, U64, 0
        self.pto_count = 0
        self.time_of_last_ack_eliciting = [None] * 3
        self.max_ack_delay = max_ack_delay_us
        self.loss_time = [None] * 3

    def update_rtt(self, latest_rtt, ack_delay, handshake_confirmed):  # loss.rs:68-101
        self.latest_rtt = latest_rtt
        if self.min_rtt == U64 or latest_rtt < self.min_rtt:
            self.min_rtt = latest_rtt
        if self.smoothed_rtt_ is None:
            self.smoothed_rtt_ = latest_rtt
            self.rttvar = latest_rtt // 2
            return
        srtt = self.smoothed_rtt_
        adjusted = latest_rtt
        if handshake_confirmed:
            capped = min(ack_delay, self.max_ack_delay)
            if latest_rtt > self.min_rtt + capped:
                adjusted = latest_rtt - capped
        self.rttvar = (3 * self.rttvar + abs(srtt - adjusted)) // 4
        self.smoothed_rtt_ = (7 * srtt + adjusted) // 8

    def on_ack_received(self, level, largest_acked):  # loss.rs:104-113
        prev = self.largest_acked[level]
        if prev is None or largest_acked > prev:
            self.largest_acked[level] = largest_acked

    def smoothed_rtt(self):
        return INITIAL_RTT if self.smoothed_rtt_ is None else self.smoothed_rtt_

    def loss_delay(self):
        return max(max(self.smoothed_rtt(), self.latest_rtt) * TIME_NUM // TIME_DEN, GRANULARITY)

    def detect_lost_packets(self, level, tracker, now):  # loss.rs:117-172; also returns "the 65th loss broke the scan"
        largest_acked = self.largest_acked[level]
        if largest_acked is None:
            return [], None, False
        loss_delay = self.loss_delay()
        lost_send_time = sat_sub(now, loss_delay)
        lost_pns, loss_time, cut = [], None, False
        for pkt in tracker.sent_below_pn(level, largest_acked + 1):
            if pkt.pn > largest_acked:
                continue
            if largest_acked >= pkt.pn + PACKET_THRESHOLD or pkt.time_sent <= lost_send_time:
                if len(lost_pns) == MAX_LOST:
                    cut = True
                    break
                lost_pns.append(pkt.pn)
                continue
            deadline = pkt.time_sent + loss_delay
            loss_time = deadline if loss_time is None else min(loss_time, deadline)
        self.loss_time[level] = loss_time
        return lost_pns, loss_time, cut

    def pto_duration(self):  # loss.rs:176-185
        rttvar = self.rttvar if self.smoothed_rtt_ is not None else INITIAL_RTT // 2
        return self.smoothed_rtt() + max(4 * rttvar, GRANULARITY) + self.max_ack_delay

    def pto_timeout(self, tracker):  # loss.rs:188-228, wrapping
        pto = (self.pto_duration() * (1 << min(self.pto_count, 62))) & U64
        if not any(tracker.has_ack_eliciting_in_flight(l) for l in range(3)):
            return None
        times = [t for t in self.time_of_last_ack_eliciting if t is not None]
        return (max(times) + pto) & U64 if times else None

    def on_pto(self):
        self.pto_count += 1

    def next_timeout(self, tracker):  # loss.rs:241-260
        cands = [t for t in self.loss_time if t is not None]
        pto = self.pto_timeout(tracker)
        if pto is not None:
            cands.append(pto)
        return min(cands) if cands else None

    def on_ack_eliciting_sent(self, level, now):
        self.time_of_last_ack_eliciting[level] = now

    def drop_space(self, level):  # loss.rs:283-288
        self.largest_acked[level] = self.time_of_last_ack_eliciting[level] = self.loss_time[level] = None


# ---- congestion.rs -----------------------------------------------------------------------------------------
class CongestionController:
    def __init__(self, mds):
        self.minimum_window = 2 * mds
        self.cwnd = max(10 * mds, 14_720)
        self.ssthresh = U64
        self.bytes_in_flight = 0
        self.recovery_start_time = None
        self.persistent_congestion_threshold = 0
        self.max_datagram_size = mds

    def on_packet_sent(self, nbytes):
        self.bytes_in_flight = (self.bytes_in_flight + nbytes) & U64

    def in_recovery(self, sent_time):
        return self.recovery_start_time is not None and sent_time <= self.recovery_start_time

    def in_slow_start(self):
        return self.cwnd < self.ssthresh

    def on_packet_acked(self, nbytes, sent_time):  # congestion.rs:54-72
        self.bytes_in_flight = sat_sub(self.bytes_in_flight, nbytes)
        if self.in_recovery(sent_time):
            return "recovery"
        if self.in_slow_start():
            self.cwnd += nbytes
            return "slow_start"
        if self.cwnd:
            self.cwnd += self.max_datagram_size * nbytes // self.cwnd
        return "avoidance"

    def on_packet_lost(self, nbytes, sent_time, now):  # congestion.rs:75-87
        self.bytes_in_flight = sat_sub(self.bytes_in_flight, nbytes)
        if self.in_recovery(sent_time):
            return False
        self.recovery_start_time = now
        self.ssthresh = max(self.cwnd // 2, self.minimum_window)
        self.cwnd = self.ssthresh
        return True


# ---- one connection: the three structures and the two arms ------------------------------------------------------
class Conn:
    def __init__(self, max_ack_delay_us=25_000, mds=1200):
        self.tracker, self.ld, self.cc = SentPacketTracker(), LossDetector(max_ack_delay_us), CongestionController(mds)
        self.flags, self.reserved = 0, 0
        self.cov = {}   # what happened, for the coverage checks

    def hit(self, what):
        self.cov[what] = self.cov.get(what, 0) + 1

    def sent(self, pn, level, now, pkt_len):  # transmit.rs:610-619
        if not self.tracker.on_packet_sent(SentPacket(pn, level, now, pkt_len & 0xFFFF)):
            self.hit("full_tracker")
        self.ld.on_ack_eliciting_sent(level, now)
        self.cc.on_packet_sent(pkt_len)

    def drop(self, level):
        self.tracker.drop_space(level)
        self.ld.drop_space(level)

    def handshake_done(self):  # recv.rs:694-703 on a client
        self.flags |= rc.CONFIRMED
        self.drop(1)

    def ack(self, level, largest, ack_delay, first_range, range_bytes, now):  # recv.rs:563-612
        """Returns (n_acked, n_acked_cc, flags, largest_newly_acked pn, [lost SentPacket])."""
        pairs, pos, flags = [], 0, 0
        while True:
            gap, pos1 = varint_at(range_bytes, pos)
            rng, pos2 = varint_at(range_bytes, pos1) if gap is not None else (None, pos)
            if rng is None:
                break
            pos = pos2
            if len(pairs) == MAX_PAIRS:
                flags |= rc.RANGES_CUT
                break
            pairs.append((gap, rng))
        res = self.tracker.on_ack_received(level, largest, first_range, pairs)
        if res.broke:
            flags |= rc.RANGES_BROKE
        self.ld.on_ack_received(level, largest)
        top = res.largest_newly_acked
        if top is not None:
            if top.time_sent > 0 and now >= top.time_sent:
                self.ld.update_rtt(now - top.time_sent, ack_delay, bool(self.flags & rc.CONFIRMED))
                flags |= rc.RTT
                self.hit("rtt_sample")
            self.ld.pto_count = 0
        for pkt in res.newly_acked:
            self.hit("ack_" + self.cc.on_packet_acked(pkt.size, pkt.time_sent))
        if res.n_removed > MAX_NEWLY_ACKED:
            self.hit("acked_beyond_32")
        la = self.ld.largest_acked[level]
        lost_send_time = sat_sub(now, self.ld.loss_delay())
        for p in self.tracker.sent_below_pn(level, la + 1):
            self.hit("pn_threshold_loss" if la >= p.pn + PACKET_THRESHOLD else
                     "time_threshold_loss" if p.time_sent <= lost_send_time else "loss_timer")
        lost_pns, _, cut = self.ld.detect_lost_packets(level, self.tracker, now)
        if cut:
            flags |= rc.LOST_CUT
        lost = []
        for pn in lost_pns:
            p = self.tracker.remove(level, pn)
            if p is not None:
                if self.cc.on_packet_lost(p.size, p.time_sent, now):
                    self.hit("recovery_entry")
                lost.append(p)
        return res.n_removed, len(res.newly_acked), flags, top.pn if top is not None else 0, lost

    def timeout(self):
        t = self.ld.next_timeout(self.tracker)
        return U64 if t is None else t


def varint_at(b, pos):
    """decode_varint at b[pos:]: (value, next position), or (None, pos) when it does not fit."""
    if pos >= len(b):
        return None, pos
    n = 1 << (b[pos] >> 6)
    if len(b) - pos < n:
        return None, pos
    v = b[pos] & 0x3F
    for k in range(1, n):
        v = v << 8 | b[pos + k]
    return v, pos + n


def varint(v, width=None):
    """encode_varint, in the shortest form or in `width` bytes."""
    n = width or (1 if v < 64 else 2 if v < 16384 else 4 if v < (1 << 30) else 8)
    assert v < 1 << (8 * n - 2)
    return bytes([(v >> (8 * (n - 1 - k)) & 0xFF) | ((n.bit_length() - 1) << 6 if k == 0 else 0) for k in range(n)])


def pair_bytes(pairs, widths=None):
    out = b""
    for i, (gap, rng) in enumerate(pairs):
        w = widths[i % len(widths)] if widths else None
        out += varint(gap, w) + varint(rng, w)
    return out


# ---- rows ---------------------------------------------------------------------------------------------------
def load_conn(row):
    c = Conn()
    ld, cc, have = c.ld, c.cc, int(row["have"])
    for l in range(3):
        ld.largest_acked[l] = int(row["largest_acked"][l]) if have >> l & 1 else None
        ld.time_of_last_ack_eliciting[l] = int(row["time_of_last_ack_eliciting"][l]) if have >> (3 + l) & 1 else None
        ld.loss_time[l] = int(row["loss_time"][l]) if have >> (6 + l) & 1 else None
    ld.smoothed_rtt_ = int(row["smoothed_rtt"]) if have & rc.HAVE_SRTT else None
    ld.rttvar, ld.min_rtt, ld.latest_rtt = int(row["rttvar"]), int(row["min_rtt"]), int(row["latest_rtt"])
    ld.max_ack_delay, ld.pto_count = int(row["max_ack_delay"]), int(row["pto_count"])
    cc.cwnd, cc.ssthresh, cc.bytes_in_flight = int(row["cwnd"]), int(row["ssthresh"]), int(row["bytes_in_flight"])
    cc.recovery_start_time = int(row["recovery_start_time"]) if have & rc.HAVE_RECOVERY_START else None
    cc.persistent_congestion_threshold = int(row["persistent_congestion_threshold"])
    cc.max_datagram_size, cc.minimum_window = int(row["max_datagram_size"]), int(row["minimum_window"])
    c.flags = int(row["flags"])
    c.have_other = have & ~0x7FF
    c.tracker.count = int(row["count"])
    for i, e in enumerate(row["sent"]):
        if e["flags"] & rc.USED:
            c.tracker.entries[i] = SentPacket(int(e["pn"]), int(e["level"]), int(e["time_sent"]), int(e["size"]), int(e["flags"]))
    return c


def store_conn(row, c):  # whole, but never `reserved`; an Option that is None is 0
    ld, cc, have = c.ld, c.cc, c.have_other
    for l in range(3):
        for name, shift, v in (("largest_acked", 0, ld.largest_acked[l]), ("time_of_last_ack_eliciting", 3, ld.time_of_last_ack_eliciting[l]),
                               ("loss_time", 6, ld.loss_time[l])):
            row[name][l] = 0 if v is None else v
            have |= (v is not None) << (shift + l)
    row["smoothed_rtt"] = 0 if ld.smoothed_rtt_ is None else ld.smoothed_rtt_
    have |= rc.HAVE_SRTT if ld.smoothed_rtt_ is not None else 0
    row["rttvar"], row["min_rtt"], row["latest_rtt"], row["max_ack_delay"] = ld.rttvar, ld.min_rtt, ld.latest_rtt, ld.max_ack_delay
    row["cwnd"], row["ssthresh"], row["bytes_in_flight"] = cc.cwnd & U64, cc.ssthresh, cc.bytes_in_flight
    row["recovery_start_time"] = 0 if cc.recovery_start_time is None else cc.recovery_start_time
    have |= rc.HAVE_RECOVERY_START if cc.recovery_start_time is not None else 0
    row["persistent_congestion_threshold"] = cc.persistent_congestion_threshold
    row["max_datagram_size"], row["minimum_window"] = cc.max_datagram_size, cc.minimum_window
    row["have"], row["pto_count"], row["count"], row["flags"] = have, c.ld.pto_count, c.tracker.count & 0xFFFFFFFF, c.flags
    for i, p in enumerate(c.tracker.entries):
        row["sent"][i] = (0, 0, 0, 0, 0, 0) if p is None else (p.pn, p.time_sent, p.size, p.level, p.flags, 0)


def state_rows(n_conns, pre=None, max_ack_delay_us=25_000, mds=1200):
    """Fresh rows as mq_recovery_state_init leaves them (without the library), then `pre`: {conn: function(Conn)}."""
    rows = np.zeros(n_conns, dtype=rc.CONN_RECOVERY_DTYPE)
    for c in range(n_conns):
        conn = Conn(max_ack_delay_us, mds)
        conn.have_other = 0
        if pre and c in pre:
            pre[c](conn)
        store_conn(rows[c], conn)
    return rows


# ---- the calls -------------------------------------------------------------------------------------------------
def run_sent(reqs, status, pkt_len, now, rec, timeouts=None, cov=None):
    """mq_batch_sent: returns (rec, timeouts) as new arrays."""
    rec = rec.copy()
    timeouts = None if timeouts is None else timeouts.copy()
    conns = {}
    for i, q in enumerate(reqs):
        c, level = int(q["conn"]), int(q["level"])
        if status[i] != 0 or c >= len(rec) or level >= 3:
            continue
        if c not in conns:
            conns[c] = load_conn(rec[c])
        conns[c].sent(int(q["pn"]), level, int(now[i]), int(pkt_len[i]))
    for c, conn in conns.items():
        store_conn(rec[c], conn)
        if timeouts is not None:
            timeouts[c] = conn.timeout()
        if cov is not None:
            for k, v in conn.cov.items():
                cov[k] = cov.get(k, 0) + v
    return rec, timeouts


def selected(arena_len, pkts, n_pkts, dgrams, frs, n_frames, n_conns, flags):
    """(record index, conn, arena offset of the range bytes, datagram) of every selected record, in record order."""
    n_p, n_f = min(int(n_pkts), len(pkts)), min(int(n_frames), len(frs))
    out = []
    for k in range(n_f):
        f = frs[k]
        t = int(f["type"])
        ack = t in (0x02, 0x03)
        if not (ack or (t == 0x1e and flags & rc.CLIENT)) or f["level"] >= 3 or f["pkt"] >= n_p:
            continue
        p = pkts[int(f["pkt"])]
        if p["dgram"] >= len(dgrams):
            continue
        c = int(dgrams["conn"][p["dgram"]])
        if c >= n_conns:
            continue
        src = int(p["offset"]) + int(p["payload_offset"]) + int(f["data_pos"])
        if ack and src + int(f["data_len"]) > arena_len:
            continue
        out.append((k, c, src, int(p["dgram"])))
    return out


def run_recovery(arena, pkts, n_pkts, dgrams, dgram_now, frs, n_frames, drop_mask, rec, flags=0, timeouts=None, cov=None):
    """mq_batch_recovery: returns (rec, evts, lost, timeouts) as new arrays; lost holds every lost packet (the
    device writes the first max_lost of them and reports their number)."""
    rec = rec.copy()
    timeouts = None if timeouts is None else timeouts.copy()
    conns, evts, lost = {}, [], []
    if drop_mask is not None:
        for c in range(len(rec)):
            if drop_mask[c] & 7:
                conns[c] = load_conn(rec[c])
                for l in range(3):
                    if drop_mask[c] >> l & 1:
                        conns[c].drop(l)
    for k, c, src, d in selected(len(arena), pkts, n_pkts, dgrams, frs, n_frames, len(rec), flags):
        if c not in conns:
            conns[c] = load_conn(rec[c])
        f = frs[k]
        if f["type"] == 0x1e:
            conns[c].handshake_done()
            continue
        data = bytes(arena[src:src + int(f["data_len"])])
        level = int(f["level"])
        n_acked, n_cc, fl, top, gone = conns[c].ack(level, int(f["v"][0]), int(f["v"][1]), int(f["v"][3]), data, int(dgram_now[d]))
        evts.append((k, c, n_acked, n_cc, len(gone), fl, len(lost), 0, top))
        lost += [(p.pn, c, p.size, level, 0) for p in gone]
    for c, conn in conns.items():
        store_conn(rec[c], conn)
        if timeouts is not None:
            timeouts[c] = conn.timeout()
        if cov is not None:
            for k, v in conn.cov.items():
                cov[k] = cov.get(k, 0) + v
    return rec, np.array(evts, dtype=rc.EVT_DTYPE), np.array(lost, dtype=rc.LOST_DTYPE), timeouts


# ---- batches ---------------------------------------------------------------------------------------------------
def A(conn, level, largest, first_range=0, pairs=(), now=0, delay=0, type=0x02, widths=None, raw=None, **kw):
    """An ACK record; `pairs` are (gap, range), encoded in `widths` bytes each (cycled), or `raw` range bytes."""
    data = raw if raw is not None else pair_bytes(pairs, widths)
    return dict(kw, conn=conn, type=type, level=level, v=(largest, delay, len(pairs), first_range), data=data, now=now)


def H(conn, now=0, level=2, **kw):
    return dict(kw, conn=conn, type=0x1e, level=level, v=(0, 0, 0, 0), data=b"", now=now)


def other(conn, ftype, now=0):
    return dict(conn=conn, type=ftype, level=2, v=(5, 0, 0, 0), data=b"\x00\x00", now=now)


def make_batch(recs, n_conns, seed=0):
    """Crafted device inputs for a list of records: (arena, pkts, dgrams, dgram_now, frames). Every record has
    its own packet and datagram unless it says same_pkt=True (it joins the packet before it). A record's `bad`
    says why it must not be selected: "pkt", "dgram", "conn" or "arena" (its range bytes leave the arena by one
    byte); at_end=True puts the last record's range bytes at the very end of the arena."""
    rng = np.random.default_rng(2000 + seed)
    chunks, pos = [], 0
    pk, fr, dg, patch = [], [], [], []

    def filler(n):
        nonlocal pos
        chunks.append(rng.integers(0, 256, n, dtype=np.uint8))
        pos += n

    cur = None   # payload position in the open packet
    for i, r in enumerate(recs):
        data, bad = r["data"], r.get("bad")
        if not (r.get("same_pkt") and pk):
            filler(int(rng.integers(0, 20)))
            po = int(rng.integers(1, 40))
            dg.append([r["conn"], r["now"]])
            pk.append([pos, 0, po, len(dg) - 1])
            filler(po)
            cur = 0
        p = pk[-1]
        head = int(rng.integers(1, 12))
        filler(head)
        data_pos = cur + head
        chunks.append(np.frombuffer(data, dtype=np.uint8))
        pos += len(data)
        cur = data_pos + len(data)
        p[1] = p[2] + cur + 16
        pkt = len(pk) - 1
        if bad == "pkt":
            pkt = 1 << 30
        elif bad == "dgram":
            p[3] = 1 << 20
        elif bad == "conn":
            dg[-1][0] = n_conns + (i & 1) * (CONN_NONE - n_conns)
        elif bad == "arena":
            patch.append((len(pk) - 1, data_pos + len(data), 1))
        if r.get("at_end"):
            assert i == len(recs) - 1
        fr.append((pkt, data_pos - head, head + len(data), r["type"], r["level"], data_pos, len(data), 0, r["v"]))
    if not (recs and recs[-1].get("at_end")):
        filler(16 + int(rng.integers(0, 20)))
    arena = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    pkts = np.zeros(len(pk), dtype=recv.PKT_DTYPE)
    for i, p in enumerate(pk):
        pkts[i]["offset"], pkts[i]["len"], pkts[i]["payload_offset"], pkts[i]["dgram"] = p[0], p[1], p[2], p[3]
        pkts[i]["level"], pkts[i]["pn"] = 2, i
    for i, end, over in patch:
        pkts[i]["offset"] = len(arena) - int(pkts[i]["payload_offset"]) - end + over
    dgrams = np.zeros(len(dg), dtype=recv.DGRAM_DTYPE)
    dgrams["conn"], dgrams["len"] = [d[0] for d in dg], 1200
    now = np.array([d[1] for d in dg], dtype=np.uint64)
    return arena, pkts, dgrams, now, np.array(fr, dtype=frames.FRAME_DTYPE)


def make_sends(sends):
    """(reqs, status, pkt_len, now) for a list of (conn, level, pn, now, pkt_len[, status])."""
    reqs = np.zeros(len(sends), dtype=send.REQ_DTYPE)
    status = np.zeros(len(sends), dtype=np.uint8)
    for i, s in enumerate(sends):
        reqs[i]["conn"], reqs[i]["level"], reqs[i]["pn"] = s[0], s[1], s[2]
        status[i] = s[5] if len(s) > 5 else 0
    return (reqs, status, np.array([s[4] for s in sends], dtype=np.uint32), np.array([s[3] for s in sends], dtype=np.uint64))


def seed_sent(entries):
    """A `pre` function that puts (pn, level, time_sent, size[, slot[, flags]]) into a fresh connection and counts
    them in flight, as sends would have."""
    def fill(conn):
        for e in entries:
            p = SentPacket(e[0], e[1], e[2], e[3], e[5] if len(e) > 5 else ALL_FLAGS)
            if len(e) > 4 and e[4] is not None:
                conn.tracker.entries[e[4]] = p
                conn.tracker.count += 1
            else:
                conn.tracker.on_packet_sent(p)
            conn.ld.on_ack_eliciting_sent(e[1], e[2])
            conn.cc.on_packet_sent(e[3])
    return fill


def chain(*fns):
    def fill(conn):
        for f in fns:
            f(conn)
    return fill


def ladder_cases():
    """(name, n_conns, pre, sends or None, records, drop_mask or None, flags). The case's connection is
    n_conns - 1, so with 3 and 9 connections several share a block and the others have no records."""
    cases = []

    def add(name, pre, recs, sends=None, drop=None, flags=0):
        for n in (1, 3, 9):
            c = n - 1
            cases.append((f"{name}-{n}", n, {c: pre} if pre else None,
                          None if sends is None else [(c,) + s for s in sends],
                          [dict(r, conn=c) for r in recs], None if drop is None else [0] * c + [drop], flags))

    def app(n, t0=1000, size=1200, first_pn=0):  # n packets at level 2, pn and time rising
        return seed_sent([(first_pn + i, 2, t0 + 10 * i, size) for i in range(n)])

    for n in (63, 64, 65, 127, 128):   # filled to exactly n entries, then one or two more sends and an ACK of the last
        add(f"fill_{n}", app(n), [A(0, 2, n + 1, 1, now=90_000)], sends=[(2, n, 80_000, 1300), (2, n + 1, 80_010, 70_000)])
    add("send_129th", app(128), [A(0, 0, 0, 0, now=90_000)], sends=[(2, 128, 80_000, 1300)])
    add("ack_high_half_only", app(128), [A(0, 2, 127, 27, now=3000)])
    add("acked_32", app(40), [A(0, 2, 39, 31, now=3000)])
    add("acked_33", app(40), [A(0, 2, 39, 32, now=3000)])
    # losses by the PN threshold: 64 and 65 of them, then entries behind the break that would set the timer
    for n in (64, 65):
        pre = chain(app(n), seed_sent([(1001, 2, 2950, 100), (1002, 2, 2960, 100), (1003, 2, 2970, 100)]))
        add(f"lost_{n}", pre, [A(0, 2, 1003, 0, now=3000)])
    add("lost_65_timer_before_break", chain(seed_sent([(997, 2, 2990, 100)]), app(70), seed_sent([(998, 2, 2995, 100), (999, 2, 2999, 50)])),
        [A(0, 2, 999, 0, now=3000)])
    pairs16 = [(0, 0)] * 16
    add("pairs_16", app(60), [A(0, 2, 59, 0, pairs16, now=3000)])
    add("pairs_17", app(60), [A(0, 2, 59, 0, pairs16 + [(0, 0)], now=3000)])
    add("pairs_40", app(100), [A(0, 2, 99, 0, [(0, 0)] * 40, now=3000)])
    add("break_first_pair", app(20), [A(0, 2, 5, 4, [(0, 0), (0, 0)], now=3000)])
    add("break_middle_pair", app(20), [A(0, 2, 9, 1, [(0, 1), (3, 0), (0, 0), (0, 0)], now=3000)])
    add("break_then_cut", app(20), [A(0, 2, 9, 8, [(5, 0)] + [(0, 0)] * 16, now=3000)])
    add("first_range_above_largest", app(20), [A(0, 2, 5, 100, [(0, 0)], now=3000)])
    add("varint_widths", app(60), [A(0, 2, 59, 1, [(0, 1), (1, 0), (2, 2), (0, 0), (1, 1)], now=3000, widths=(1, 2, 4, 8))])
    add("truncated_pair", app(20), [A(0, 2, 19, 0, raw=pair_bytes([(0, 0)]) + b"\x40", now=3000), A(0, 2, 10, 0, raw=b"\x01\xc0\x00", now=3100)])
    add("arena_end_exact", app(20), [A(0, 2, 19, 0, [(0, 0), (1, 1)], now=3000, at_end=True)])
    add("arena_end_one_past", app(20), [A(0, 2, 19, 0, [(0, 0), (1, 1)], now=3000, bad="arena")])
    add("not_selected", app(20), [A(0, 2, 19, 0, now=3000, bad="pkt"), A(0, 2, 18, 0, now=3000, bad="dgram"), A(0, 2, 17, 0, now=3000, bad="conn"),
                                  A(0, 3, 16, 0, now=3000), other(0, 0x06), other(0, 0x1c), A(0, 2, 15, 0, now=3000, bad="conn"), A(0, 2, 3, 0, now=3000)])
    add("level_mismatch", chain(app(10), seed_sent([(3, 0, 500, 300), (4, 1, 600, 400)])), [A(0, 0, 4, 4, now=3000), A(0, 1, 9, 9, now=3100)])
    add("largest_acked_already_above", chain(app(10), lambda c: c.ld.on_ack_received(2, 50)), [A(0, 2, 8, 0, now=3000)])
    add("ack_type_3", app(10), [A(0, 2, 9, 2, now=3000, type=0x03)])
    add("time_sent_zero", seed_sent([(0, 2, 0, 100), (1, 2, 0, 100)]), [A(0, 2, 1, 0, now=3000)])
    add("now_before_time_sent", seed_sent([(0, 2, 5000, 100), (1, 2, 5000, 100)]), [A(0, 2, 1, 0, now=3000)])
    # srtt 10 000 -> loss delay 11 250 (loss.rs time_threshold_loss): lost at exactly now - 11 250, not one later
    rtt = lambda c: c.ld.update_rtt(10_000, 0, False)  # noqa: E731
    add("time_sent_eq_lost_send_time", chain(rtt, seed_sent([(0, 2, 1_000, 100), (1, 2, 1_001, 100), (2, 2, 0, 100)])),
        [A(0, 2, 2, 0, now=12_250)])
    first = lambda c: c.ld.update_rtt(100_000, 0, False)  # noqa: E731
    confirmed = lambda c: setattr(c, "flags", rc.CONFIRMED)  # noqa: E731
    for name, pre in (("", first), ("_confirmed", chain(first, confirmed))):
        add(f"ack_delay_above_max{name}", chain(pre, seed_sent([(0, 2, 1000, 100)])), [A(0, 2, 0, 0, now=201_000, delay=50_000)])
        add(f"ack_delay_below_max{name}", chain(pre, seed_sent([(0, 2, 1000, 100)])), [A(0, 2, 0, 0, now=201_000, delay=10_000)])
        add(f"ack_delay_not_subtracted{name}", chain(pre, seed_sent([(0, 2, 1000, 100)])), [A(0, 2, 0, 0, now=121_000, delay=50_000)])
    # recovery: a loss enters it; a second loss sent before recovery_start does not; an ack of a pre-recovery packet
    # does not grow the window, one sent after it does (avoidance, cwnd == ssthresh)
    add("recovery_sequence", seed_sent([(i, 2, 1000 + 100 * i, 1200) for i in range(12)]),
        [A(0, 2, 4, 0, now=400_000), A(0, 2, 8, 0, now=400_100), A(0, 2, 9, 0, now=400_200), A(0, 2, 20, 0, now=900_000)],
        sends=[(2, 20, 500_000, 1200)])
    add("cwnd_eq_ssthresh", chain(seed_sent([(0, 2, 1000, 1200), (1, 2, 1100, 1200)]), lambda c: setattr(c.cc, "ssthresh", c.cc.cwnd)),
        [A(0, 2, 1, 1, now=5000)])
    add("cwnd_below_ssthresh_by_one", chain(seed_sent([(0, 2, 1000, 1200), (1, 2, 1100, 1200)]), lambda c: setattr(c.cc, "ssthresh", c.cc.cwnd + 1)),
        [A(0, 2, 1, 1, now=5000)])
    # the same pn in two slots: the lost one is the later slot, remove() takes the earlier one
    add("duplicate_pn_lost_later_slot", chain(rtt, seed_sent([(7, 2, 11_000, 111), (7, 2, 500, 222), (9, 2, 11_500, 100)])),
        [A(0, 2, 9, 0, now=12_000)])
    add("duplicate_pn_both_lost", seed_sent([(7, 2, 1000, 111), (7, 2, 1100, 222), (20, 2, 1200, 100)]), [A(0, 2, 20, 0, now=3000)])
    add("duplicate_pn_acked", seed_sent([(7, 2, 1000, 111), (7, 2, 1100, 222)]), [A(0, 2, 7, 0, now=3000)])
    add("drop_mask_alone", chain(app(5), seed_sent([(0, 0, 100, 500), (1, 1, 200, 600)]), lambda c: c.ld.on_ack_received(0, 3)), [], drop=3)
    add("drop_mask_then_ack", chain(app(5), seed_sent([(0, 0, 100, 500), (1, 1, 200, 600)])), [A(0, 1, 1, 0, now=3000), A(0, 2, 4, 0, now=3100)], drop=2)
    hd = chain(first, seed_sent([(0, 1, 500, 300), (0, 2, 1000, 100)]))
    add("handshake_done_then_ack_client", hd, [H(0, now=201_000), A(0, 2, 0, 0, now=201_000, delay=50_000, same_pkt=True), A(0, 1, 0, 0, now=201_100)],
        flags=rc.CLIENT)
    add("handshake_done_ignored_as_server", hd, [H(0, now=201_000), A(0, 2, 0, 0, now=201_000, delay=50_000, same_pkt=True), A(0, 1, 0, 0, now=201_100)])
    add("pto_backoff_reset", chain(first, app(3), lambda c: (c.ld.on_pto(), c.ld.on_pto())), [A(0, 2, 0, 0, now=150_000)])
    add("records_150", app(100), [A(0, 2, (37 * i) % 100, i % 3 == 0, now=3000 + 7 * i) for i in range(150)])   # three chunks of records
    add("stale_unused_entry", chain(app(3), lambda c: c.tracker.entries.__setitem__(5, SentPacket(99, 2, 77, 88, flags=rc.IN_FLIGHT))),
        [A(0, 2, 99, 0, now=3000)], sends=[(2, 3, 2000, 100)])
    return cases


def fuzz_batch(seed, n_conns=64, n_sends=2000, n_acks=600):
    """Seeded traffic: (pre, sends, records, drop_mask, flags). A few connections send far more than they get
    acked (full tracker), some ACKs arrive late (time-threshold losses), reordered or with gaps."""
    rng = np.random.default_rng(seed)
    sends, recs = [], []
    next_pn = [[0, 0, 0] for _ in range(n_conns)]
    sent_log = [[[], [], []] for _ in range(n_conns)]
    heavy = set(int(c) for c in rng.choice(n_conns, 3, replace=False))
    t = 1000
    for _ in range(n_sends):
        c = int(rng.integers(0, n_conns)) if rng.random() < 0.7 else int(rng.choice(sorted(heavy)))
        level = int(rng.choice([0, 1, 2, 2, 2, 2]))
        t += int(rng.integers(1, 400))
        status = 0 if rng.random() < 0.95 else int(rng.choice([2, 3, 5]))
        conn = c if rng.random() < 0.97 else int(rng.choice([n_conns, CONN_NONE]))
        pn = next_pn[c][level]
        sends.append((conn, level if rng.random() < 0.99 else 3, pn, t, int(rng.choice([40, 1200, 1350, 66_000])), status))
        if status == 0 and conn == c:
            next_pn[c][level] += 1 + (rng.random() < 0.05)
            sent_log[c][level].append((pn, t))
    t_end = t
    for _ in range(n_acks):
        c = int(rng.integers(0, n_conns))
        level = int(rng.choice([0, 1, 2, 2, 2, 2]))
        log = sent_log[c][level]
        if not log or (c in heavy and rng.random() < 0.7):
            continue
        pn, ts = log[int(rng.integers(0, len(log)))]
        kind = rng.random()
        now = ts + int(rng.integers(1, 60_000)) if kind < 0.6 else t_end + int(rng.integers(0, 2_000_000)) if kind < 0.9 else sat_sub(ts, 5)
        pairs = [(int(rng.integers(0, 4)), int(rng.integers(0, 3))) for _ in range(int(rng.choice([0, 0, 1, 2, 5, 20])))]
        recs.append(A(c, level, pn + int(rng.integers(0, 3)), int(rng.integers(0, 6)), pairs, now=now,
                      delay=int(rng.integers(0, 60_000)), type=int(rng.choice([2, 2, 3])),
                      widths=None if rng.random() < 0.7 else (1, 2, 4, 8),
                      bad=None if rng.random() < 0.97 else str(rng.choice(["pkt", "dgram", "conn"]))))
        if rng.random() < 0.03:
            recs.append(H(c, now=now))
        if rng.random() < 0.05:
            recs.append(other(c, int(rng.choice([0x01, 0x06, 0x08, 0x1c]))))
    drop = np.zeros(n_conns, dtype=np.uint8)
    drop[rng.choice(n_conns, 4, replace=False)] = [1, 2, 3, 4]
    return None, sends, recs, drop, rc.CLIENT


# ---- the chained test's traffic -----------------------------------------------------------------------------------
CHAIN_SEED, CHAIN_CONNS, CHAIN_APP = 37, 8, 40


def chained_traffic(orc, build_traffic, assemble, fm, seed=CHAIN_SEED):
    """Traffic for recv -> frames -> recovery and acks -> protect -> sent: recv_traffic's connections with an ACK
    frame in (almost) every packet's payload, connections that have 60 1-RTT packets outstanding (connection 0: a
    nearly full tracker), and one time per datagram. Returns (keys, conns, arena, dgrams, dgram_now, rec rows)."""
    keys, conns, scripts = build_traffic(orc, seed=seed, n_conns=CHAIN_CONNS, n_app=CHAIN_APP)
    rng = np.random.default_rng(seed)
    for c, (dcid, rows, dgs) in enumerate(scripts):
        k = 0
        for parts in dgs:
            for q, part in enumerate(parts):
                level = part[1]
                body = b"\x01" + fm.build(0x10, (1 << 20,))     # never too short for the header-protection sample
                if level < 2:
                    body += fm.build(0x02, (part[3], 0, 0, 0))
                else:
                    if rng.random() < 0.8:                      # a missing ACK leaves a gap behind the next one
                        pairs = [(0, 0)] if rng.random() < 0.2 and k >= 4 else []
                        first = int(rng.integers(0, 2)) if k >= 1 + 3 * len(pairs) else 0
                        tail = b"".join(varint(g) + varint(r) for g, r in pairs)
                        body += fm.build(0x02 + (k % 5 == 4), (k, int(rng.integers(0, 40_000)), len(pairs), first), tail=tail)
                        if k % 5 == 4:
                            body += fm.build(0x00, (1, 2, 3))[1:]   # the ECN counts of an ACK of type 0x03
                    if k == 20 and c % 2:
                        body += b"\x1e"                         # HANDSHAKE_DONE
                    k += 1
                    # PADDING keeps a tampered byte (20 from the end) behind the header-protection sample, so a
                    # tampered packet fails in the AEAD alone and the receive composite defers nothing
                    body += b"\x00" * 40
                parts[q] = part[:4] + (body,) + part[5:]
    arena, dgrams = assemble(orc, keys, conns, scripts, seed=seed)
    seen = {}
    now = np.zeros(len(dgrams), dtype=np.uint64)
    for i, c in enumerate(dgrams["conn"]):
        seen[int(c)] = seen.get(int(c), 0) + 1
        now[i] = 4000 + 5000 * seen[int(c)] + (40_000 if seen[int(c)] % 9 == 0 else 0)
    pre = {c: seed_sent([(0, 0, 500, 1200), (1, 0, 600, 1200), (0, 1, 700, 300), (1, 1, 800, 300)] +
                        [(i, 2, 1000 + 5000 * i, 1200) for i in range(123 if c == 0 else 60)])
           for c in range(CHAIN_CONNS)}
    return keys, conns, arena, dgrams, now, state_rows(CHAIN_CONNS, pre)


def chained_expectation(orc, seed=CHAIN_SEED):
    """The expected result of the chained GPU test, from the oracle and the models alone: recv and frames, the ACKs
    due and their packets (acks -> protect -> sent), then the received ACK frames (recovery)."""
    from milli_quic_amd import _lib, acks
    import acks_model as am
    import frames_model as fm
    from recv_traffic import assemble, build_traffic
    keys, conns, arena, dgrams, now, rows = chained_traffic(orc, build_traffic, assemble, fm, seed)
    n_conns, max_pkts, max_acks, stride = len(conns), 1 << 12, 3 * len(conns) + 3, 1280
    oa, oc = arena.copy(), conns.copy()
    o_pk, o_n = orc.batch_recv(keys, oc, oa, dgrams, max_pkts)
    w_summ, w_rec, w_flags = fm.run(oa, o_pk[:o_n], o_n, dgrams, n_conns)
    w_rec = np.asarray(w_rec, dtype=frames.FRAME_DTYPE)
    next_pn = [(1 << 21) + 17 * k for k in range(3 * n_conns)]
    b = dict(max_acks=max_acks, out_stride=stride, flags=acks.CLIENT, largest_pn=oc["largest_pn"], next_pn=next_pn)
    built = am.run(o_pk[:o_n], o_n, dgrams, am.tracker_rows(n_conns), np.zeros(n_conns, np.uint32), w_summ,
                   np.array(w_flags, dtype=np.uint32), b)[2]
    s_conns = send.make_conns([bytes([c + 1] * 8) for c in range(n_conns)], [b"\x09\x08"] * n_conns,
                              [[int(conns[c]["initial_row"]), int(conns[c]["handshake_row"]), int(conns[c]["app_row"][1])]
                               for c in range(n_conns)])
    reqs = built["reqs"]
    out = np.zeros(max_acks * stride, dtype=np.uint8)
    slots = np.zeros((max_acks, acks.FRAME_MAX), dtype=np.uint8)      # frame k at k * FRAME_MAX, as the requests say
    for k, frame in enumerate(built["frames"][:max_acks]):
        slots[k, :len(frame)] = np.frombuffer(bytes(frame), dtype=np.uint8)
    st, ln = orc.batch_protect(keys, s_conns, slots.reshape(-1), out, reqs, _lib.MQ_SUITE_MIXED)
    sent_now = 900_000 + 10 * np.arange(max_acks, dtype=np.uint64)
    cov = {}
    rows1, t1 = run_sent(reqs, st, ln, sent_now, rows, np.full(n_conns, 7, dtype=np.uint64), cov)
    want = run_recovery(oa, o_pk[:o_n], o_n, dgrams, now, w_rec, len(w_rec), None, rows1, rc.CLIENT, t1, cov)
    inputs = dict(keys=keys, conns=conns, arena=arena, dgrams=dgrams, now=now, rows=rows, s_conns=s_conns,
                  next_pn=next_pn, max_pkts=max_pkts, max_acks=max_acks, stride=stride, sent_now=sent_now,
                  n_acks=built["n_acks"])
    return inputs, rows1, want, cov
