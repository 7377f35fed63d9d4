"""Python model of mq_batch_acks: RecvPnTracker::record and insert_range (reference
src/connection/mod.rs:224-296), build_ack_frame (src/connection/transmit.rs:321-380) with the ACK
encoder (src/frame/mod.rs:482-508), restated in their loop form, and the call's bookkeeping (which
packets are recorded, pending bits, capacity, requests, next_pn), plus the generators of the cases
that the host replay, the GPU ladder and the fuzz share."""
import numpy as np

from milli_quic_amd import acks, frames, recv, send
from frames_model import encode_varint

OK, ERR_FRAME, SKIPPED, INVALID = frames.OK, frames.ERR_FRAME, frames.SKIPPED, frames.ERR_INVALID_ARG
CONN_NONE = 0xFFFFFFFF
CAP = acks.RANGES
PN_MAX = (1 << 62) - 1


class Tracker:
    """RecvPnTracker in its default (no `alloc`) form: heapless::Vec<(u64, u64), 32>."""

    def __init__(self, ranges=()):
        self.ranges = [tuple(r) for r in ranges]

    def largest(self):
        return self.ranges[-1][1] if self.ranges else None

    def record(self, pn):  # mod.rs:224-278
        merge_left = merge_right = None
        for i, (start, end) in enumerate(self.ranges):
            if start <= pn <= end:
                return  # already tracked
            if pn == end + 1:
                merge_left = i
            if pn + 1 == start:
                merge_right = i
        if merge_left is not None and merge_right is not None:
            new_start, new_end = self.ranges[merge_left][0], self.ranges[merge_right][1]
            first_rm, second_rm = (merge_right, merge_left) if merge_left < merge_right else (merge_left, merge_right)
            del self.ranges[first_rm]
            del self.ranges[second_rm]
            self.insert_range(new_start, new_end)
        elif merge_left is not None:
            self.ranges[merge_left] = (self.ranges[merge_left][0], pn)
        elif merge_right is not None:
            self.ranges[merge_right] = (pn, self.ranges[merge_right][1])
        else:
            if len(self.ranges) == CAP:  # is_full(): drop the lowest (oldest) range
                del self.ranges[0]
            self.insert_range(pn, pn)

    def insert_range(self, start, end):  # mod.rs:281-295
        pos = len(self.ranges)
        for i, (s, _) in enumerate(self.ranges):
            if s > start:
                pos = i
                break
        self.ranges.append((start, end))
        if pos < len(self.ranges) - 1:  # rotate the tail right by one
            self.ranges[pos:] = [self.ranges[-1]] + self.ranges[pos:-1]


def build_ack_frame(ranges):
    """transmit.rs:321-380 over mod.rs:482-508: the frame's bytes, or None for an empty tracker."""
    if not ranges:
        return None
    highest_start, highest_end = ranges[-1]
    range_buf, count = b"", 0
    prev_smallest = highest_start
    for r_start, r_end in reversed(ranges[:-1]):
        pair = encode_varint(prev_smallest - r_end - 2) + encode_varint(r_end - r_start)
        assert len(range_buf) + len(pair) <= 512  # the reference's range_buf; 31 pairs take at most 496
        range_buf += pair
        count += 1
        prev_smallest = r_start
    return (encode_varint(0x02) + encode_varint(highest_end) + encode_varint(0) + encode_varint(count)
            + encode_varint(highest_end - highest_start) + range_buf)


# ---- the call ------------------------------------------------------------------------------------------
def load_tracker(row):
    n = min(int(row["n"]), CAP)  # a loaded n above 32 is clamped
    return Tracker((int(s), int(e)) for s, e in row["range"][:n])


def store_tracker(row, t):
    row["n"] = len(t.ranges)
    row["range"] = 0
    for i, (s, e) in enumerate(t.ranges):
        row["range"][i] = (s, e)


def run(pkts, n_pkts, dgrams, trackers, pending, summary=None, conn_flags=None, build=None):
    """mq_batch_acks: returns (trackers, pending, out) as new arrays; out is None without `build`, else a
    dict of n_acks, frames (the bytes of every built ACK), reqs (all max_acks of them) and next_pn.
    build = dict(max_acks, out_stride, flags, largest_pn[n_conns][3], next_pn[3 n_conns])."""
    trackers, pending = trackers.copy(), pending.copy()
    n_conns = len(pending)
    n = min(int(n_pkts), len(pkts))
    touched = {}
    for i in range(n):
        p = pkts[i]
        if p["status"] != OK or p["level"] >= 3 or p["dgram"] >= len(dgrams):
            continue
        c = int(dgrams["conn"][p["dgram"]])
        if c >= n_conns:
            continue
        if summary is not None and summary["status"][i] != OK:
            continue
        t = 3 * c + int(p["level"])
        if t not in touched:
            touched[t] = load_tracker(trackers[t])
        touched[t].record(int(p["pn"]))
    for t, tr in touched.items():  # a tracker without packets is left as it is
        store_tracker(trackers[t], tr)
    if conn_flags is not None:
        pending |= conn_flags.astype(np.uint32) & np.uint32(7)
    if build is None:
        return trackers, pending, None
    max_acks = build["max_acks"]
    reqs = np.zeros(max_acks, dtype=send.REQ_DTYPE)
    reqs["conn"] = CONN_NONE
    next_pn = np.array(build["next_pn"], dtype=np.uint64).copy()
    out_frames, k = [], 0
    for c in range(n_conns):
        for level in range(3):
            t = 3 * c + level
            if not pending[c] >> level & 1:
                continue
            frame = build_ack_frame(load_tracker(trackers[t]).ranges)
            if frame is None:
                continue  # the bit stays set
            if k < max_acks:
                flags = send.PAD_TO_MIN if level == 0 and build["flags"] & acks.CLIENT else 0
                reqs[k] = (acks.FRAME_MAX * k, k * build["out_stride"], next_pn[t], build["largest_pn"][c][level],
                           len(frame), build["out_stride"], c, level, flags, 0)
                next_pn[t] += np.uint64(1)
                pending[c] &= ~np.uint32(1 << level)
                out_frames.append(frame)
            k += 1
    return trackers, pending, dict(n_acks=k, frames=out_frames, reqs=reqs, next_pn=next_pn)


# ---- batches ---------------------------------------------------------------------------------------------
def make_batch(events, n_conns):
    """events: (conn, level, pn) or (conn, level, pn, kind), in arrival order, each a packet in a datagram
    of its own. kind excludes the packet one way: 'status', 'frame', 'invalid', 'skipped', 'dgram', 'conn',
    'level3'. Returns pkts, dgrams, summary and the conn_flags of a batch whose recorded packets are all
    ack-eliciting."""
    n = len(events)
    pkts = np.zeros(n, dtype=recv.PKT_DTYPE)
    dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
    summ = np.zeros(n, dtype=frames.PKT_FRAMES_DTYPE)
    flags = np.zeros(n_conns, dtype=np.uint32)
    for i, ev in enumerate(events):
        c, level, pn = ev[:3]
        kind = ev[3] if len(ev) > 3 else None
        pkts[i]["pn"], pkts[i]["dgram"], pkts[i]["level"], pkts[i]["len"] = pn, i, level, 40
        dg[i]["conn"], dg[i]["len"] = c, 40
        summ[i]["flags"] = 1
        if kind == "status":
            pkts[i]["status"], summ[i]["status"] = 1, SKIPPED
        elif kind == "skipped":
            summ[i]["status"] = SKIPPED
        elif kind == "frame":
            summ[i]["status"] = ERR_FRAME
        elif kind == "invalid":
            summ[i]["status"] = INVALID
        elif kind == "dgram":
            pkts[i]["dgram"] = n + 5
        elif kind == "conn":
            dg[i]["conn"] = CONN_NONE
        elif kind == "level3":
            pkts[i]["level"] = 3
        else:
            assert kind is None, kind
            flags[c] |= 1 << level
    return pkts, dg, summ, flags


def tracker_rows(n_conns, preload=None):
    rows = np.zeros(3 * n_conns, dtype=acks.TRACKER_DTYPE)
    for t, ranges in (preload or {}).items():
        store_tracker(rows[t], Tracker(ranges))
    return rows


def wide_ranges(n=CAP, unit=1 << 31):
    """n ranges whose lengths and gaps all take 8-byte varints: with 32 of them the 515-byte frame."""
    return [(2 * i * unit + 5, (2 * i + 1) * unit + 5) for i in range(n)]


REFERENCE_CASES = [  # recv_pn_tracker_tests (mod.rs:1980-2076) and the build_ack_frame cases (transmit.rs:1201-1280)
    ("single_pn_produces_single_range", [5], [(5, 5)]),
    ("contiguous_pns_merge_into_one_range", [0, 1, 2, 3], [(0, 3)]),
    ("non_contiguous_pns_produce_multiple_ranges", [0, 1, 5, 6, 10], [(0, 1), (5, 6), (10, 10)]),
    ("filling_gap_merges_ranges", [0, 2, 1], [(0, 2)]),
    ("out_of_order_pns_correctly_tracked", [5, 3, 1, 4, 2], [(1, 5)]),
    ("duplicate_pn_is_idempotent", [3, 3, 3], [(3, 3)]),
    ("full_tracker_drops_lowest_range", [100 * i for i in range(32)] + [5000],
     [(100 * i, 100 * i) for i in range(1, 32)] + [(5000, 5000)]),
    ("largest_returns_none_when_empty", [], []),
    ("extend_lower_bound", [5, 4], [(4, 5)]),
    ("build_ack_frame_single_range", [0, 1, 2], [(0, 2)]),
    ("build_ack_frame_multiple_ranges", [0, 1, 5, 6, 10], [(0, 1), (5, 6), (10, 10)]),
]


WIDTH_EDGES = (63, 64, 16383, 16384, (1 << 30) - 1, 1 << 30)  # the last 1-, 2-, 4-byte value and the one above it


def gap_edge_pns():
    """Single packet numbers whose gaps (next - this - 2) are the width edges."""
    pns = [9]
    for g in WIDTH_EDGES:
        pns.append(pns[-1] + g + 2)
    return pns


def ladder_cases():
    """(name, n_conns, events, preload) — one batch each."""
    full = [100 * i + 1000 for i in range(CAP)]          # 32 stand-alone ranges: 1000, 1100, ..., 4100
    one = lambda pns, level=2: [(0, level, pn) for pn in pns]  # noqa: E731
    cases = [(f"ref_{name}", 1, one(pns, 0), None) for name, pns, _ in REFERENCE_CASES]
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        cases.append((f"in_order_{n}", 1, one(range(7, 7 + n)), None))
    cases += [
        ("duplicate_inside_run", 1, one([10, 11, 12, 12, 13, 14, 11, 15]), None),
        ("descending_70", 1, one(range(169, 99, -1)), None),
        ("descending_70_gaps", 1, one(range(3 * 69, -1, -3)), None),
        ("bridging_pn", 1, one([1, 2, 3, 7, 8, 9, 5, 4, 6]), None),
        ("run_absorbs_ranges", 1, one([20, 24, 27, 40] + list(range(10, 30))), None),
        ("run_reaches_next_range", 1, one([30, 31, 50] + list(range(10, 30))), None),
        ("standalone_33rd_drops_lowest", 1, one(full + [9000]), None),
        ("standalone_below_full", 1, one(full + [3]), None),
        ("standalone_below_full_then_more", 1, one(full + [3, 1, 2, 500, 8000]), None),
        ("adjacent_to_dropped", 1, one(full + [9000, 1001, 999]), None),
        ("run_into_full", 1, one(full + list(range(5000, 5040)) + list(range(1050, 1101))), None),
        ("pn_zero_and_max", 1, one([0, PN_MAX, 1, PN_MAX - 1, PN_MAX - 3]), None),
        ("gap_width_edges", 1, one(gap_edge_pns()), None),
        ("len_width_edges", 1, one([(i << 32) + L for i, L in enumerate(WIDTH_EDGES)]),
         {2: [(i << 32, (i << 32) + L - 1) for i, L in enumerate(WIDTH_EDGES)]}),
        ("frame_515_bytes", 1, one([wide_ranges()[-1][1] + 1, wide_ranges()[3][0] - 1]), {2: wide_ranges()}),
        ("three_levels_interleaved", 1, [(0, (i * 7) % 3, 100 * ((i * 7) % 3) + i // 3 + (5 if i % 11 == 0 else 0))
                                         for i in range(90)], None),
        ("five_conns_interleaved", 5, [((i * 3) % 5, 2 if i % 4 else 1, 1000 * ((i * 3) % 5) + (i // 5) * (1 + i % 2))
                                       for i in range(200)], None),
        ("excluded_each_kind", 2, [(0, 2, 1), (0, 2, 2, "status"), (0, 2, 3), (0, 2, 5, "frame"), (0, 2, 7, "invalid"),
                                   (0, 2, 9, "skipped"), (0, 2, 11, "dgram"), (0, 2, 13, "conn"), (0, 2, 15, "level3"),
                                   (1, 0, 4), (0, 2, 17)], None),
        ("tracker_n_40", 2, [(0, 1, 77), (0, 1, 5000), (1, 2, 1)], {1: [(10 * i, 10 * i + 3) for i in range(CAP)]}),
    ]
    return cases


def fuzz_sequence(rng, n, start=0, stretch=80):
    """n packet numbers as a lossy, reordering path delivers them: in-order stretches, small gaps,
    local reordering, duplicates, and jumps that leave more ranges behind than a tracker holds."""
    out, pn = [], start
    while len(out) < n:
        roll = rng.random()
        if roll < 0.45:      # an in-order stretch
            k = int(rng.integers(1, stretch))
            out += range(pn, pn + k)
            pn += k
        elif roll < 0.70:    # a small gap
            pn += int(rng.integers(1, 4))
            out.append(pn)
            pn += 1
        elif roll < 0.82:    # a window delivered out of order
            k = int(rng.integers(2, 12))
            w = list(range(pn, pn + k))
            rng.shuffle(w)
            out += w
            pn += k
        elif roll < 0.90 and out:  # duplicates of recent packets
            out += [out[-int(rng.integers(1, min(len(out), 40) + 1))] for _ in range(int(rng.integers(1, 4)))]
        elif roll < 0.96 and out:  # late arrivals from far back (below the tracker's ranges, or in an old gap)
            out.append(max(0, out[-1] - int(rng.integers(50, 5000))))
        else:                # a jump
            pn += int(rng.integers(100, 1 << int(rng.integers(8, 34))))
    return out[:n]


def fuzz_events(seed, n_pkts=20000, big=8000):
    """About n_pkts packets over 1..300 connections, connection 0 holding about `big` of them, interleaved
    in arrival order; a few packets excluded."""
    rng = np.random.default_rng(seed)
    n_conns = int(rng.integers(1, 301))
    if n_conns == 1:
        big = n_pkts
    seqs = {}
    rest = n_pkts - big
    for c in range(n_conns):
        per = big if c == 0 else max(1, rest // max(1, n_conns - 1))
        for level in (0, 1, 2):
            share = per if level == 2 else int(rng.integers(0, 6))
            if share:
                seqs[(c, level)] = fuzz_sequence(rng, share, start=int(rng.integers(0, 1 << int(rng.integers(1, 40)))))
    order = np.concatenate([np.full(len(v), i) for i, v in enumerate(seqs.values())])
    rng.shuffle(order)
    keys, at = list(seqs), [0] * len(seqs)
    events = []
    for q in order:
        c, level = keys[q]
        kind = ("frame", "status", "conn")[int(rng.integers(0, 3))] if rng.random() < 0.01 else None
        events.append((c, level, seqs[keys[q]][at[q]]) + ((kind,) if kind else ()))
        at[q] += 1
    return n_conns, events
