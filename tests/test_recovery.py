"""Loss recovery without a GPU: the Python model (recovery_model.py) against the reference's own unit-test
values, the kernels' shared integer code (milli_quic_amd/csrc/mq_recovery.h) replayed on the host against the
model, the C ABI's struct sizes, constants and argument checks, and the coverage that the chained GPU test's
traffic must have.

tests/csrc/test_recovery_host.cpp is built with g++ -fsanitize=address,undefined and run as its own process;
it reads a table of per-connection sequences and expected outcomes that this test writes from the model."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from milli_quic_amd import _lib
from milli_quic_amd import recovery as rc

import recovery_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP, INITIAL, HANDSHAKE = 2, 0, 1


def pkt(pn, level, time_sent, size):
    return m.SentPacket(pn, level, time_sent, size)


# ---- 1. the model against the reference's own unit-test values ---------------------------------------------------
def test_model_loss_rs_rtt():
    ld = m.LossDetector(25_000)
    assert ld.smoothed_rtt() == 333_000                                   # default_rtt_when_no_samples
    ld.update_rtt(100_000, 0, False)                                      # first_rtt_sample_sets_smoothed
    assert (ld.smoothed_rtt(), ld.rttvar, ld.min_rtt) == (100_000, 50_000, 100_000)
    ld.update_rtt(120_000, 0, False)                                      # subsequent_rtt_samples_use_ewma
    assert (ld.rttvar, ld.smoothed_rtt()) == (42_500, 102_500)
    ld = m.LossDetector(25_000)                                           # rtt_with_ack_delay_capped
    ld.update_rtt(100_000, 0, False)
    ld.update_rtt(120_000, 50_000, True)                                  # 120k <= 100k + 25k: nothing subtracted
    assert ld.smoothed_rtt() == 102_500
    ld = m.LossDetector(25_000)
    ld.update_rtt(100_000, 0, False)
    ld.update_rtt(200_000, 50_000, True)                                  # capped to 25k: adjusted 175k
    assert ld.smoothed_rtt() == 109_375


def test_model_loss_rs_detection():
    tr = m.SentPacketTracker(32)                                          # packet_number_threshold_loss
    for pn in range(5):
        tr.on_packet_sent(pkt(pn, APP, 1000 + pn * 1000, 100))
    ld = m.LossDetector(25_000)
    ld.update_rtt(50_000, 0, False)
    ld.on_ack_received(APP, 4)
    tr.remove(APP, 4)
    lost, _, _ = ld.detect_lost_packets(APP, tr, 1_000_000)
    assert 0 in lost and 1 in lost
    tr = m.SentPacketTracker(32)                                          # time_threshold_loss
    tr.on_packet_sent(pkt(0, APP, 1_000, 100))
    tr.on_packet_sent(pkt(1, APP, 2_000, 100))
    ld = m.LossDetector(25_000)
    ld.update_rtt(10_000, 0, False)
    ld.on_ack_received(APP, 1)
    tr.remove(APP, 1)
    lost, timer, _ = ld.detect_lost_packets(APP, tr, 12_250)
    assert lost == [0] and timer is None
    tr = m.SentPacketTracker(32)
    tr.on_packet_sent(pkt(0, APP, 1_000, 100))
    ld = m.LossDetector(25_000)
    ld.update_rtt(10_000, 0, False)
    ld.on_ack_received(APP, 1)
    lost, timer, _ = ld.detect_lost_packets(APP, tr, 12_000)
    assert lost == [] and timer == 12_250
    tr = m.SentPacketTracker(32)                                          # loss_timer_deadline
    for pn in range(3):
        tr.on_packet_sent(pkt(pn, APP, 1_000 * (pn + 1), 100))
    ld = m.LossDetector(25_000)
    ld.update_rtt(10_000, 0, False)
    ld.on_ack_received(APP, 2)
    tr.remove(APP, 2)
    lost, timer, _ = ld.detect_lost_packets(APP, tr, 5_000)
    assert lost == [] and timer == 12_250 and ld.loss_time[APP] == 12_250


def test_model_loss_rs_pto_and_drop():
    ld = m.LossDetector(25_000)                                           # pto_duration_calculation
    assert ld.pto_duration() == 1_024_000
    ld.update_rtt(100_000, 0, False)
    assert ld.pto_duration() == 325_000
    tr = m.SentPacketTracker(16)                                          # pto_backoff
    tr.on_packet_sent(pkt(0, APP, 1000, 100))
    ld.on_ack_eliciting_sent(APP, 1000)
    assert ld.pto_timeout(tr) == 1000 + 325_000
    ld.on_pto()
    assert ld.pto_timeout(tr) == 1000 + 325_000 * 2
    ld.on_pto()
    assert ld.pto_timeout(tr) == 1000 + 325_000 * 4 and ld.next_timeout(tr) == 1000 + 325_000 * 4
    ld = m.LossDetector(25_000)                                           # drop_space_clears_state
    ld.on_ack_received(INITIAL, 5)
    ld.on_ack_eliciting_sent(INITIAL, 1000)
    ld.loss_time[0] = 5000
    ld.drop_space(INITIAL)
    assert (ld.largest_acked[0], ld.time_of_last_ack_eliciting[0], ld.loss_time[0]) == (None, None, None)
    assert m.LossDetector(25_000).pto_timeout(m.SentPacketTracker(16)) is None   # no_pto_without_ack_eliciting_in_flight


def test_model_recovery_rs():
    tr = m.SentPacketTracker(16)                                          # track_and_ack_packets
    for pn, ts in ((0, 100), (1, 200), (2, 300)):
        tr.on_packet_sent(pkt(pn, INITIAL, ts, 1200))
    assert tr.count == 3
    res = tr.on_ack_received(INITIAL, 2, 2, [])
    assert (len(res.newly_acked), res.largest_newly_acked.pn, tr.count) == (3, 2, 0)
    tr = m.SentPacketTracker(16)                                          # ack_with_gaps
    for pn in range(6):
        tr.on_packet_sent(pkt(pn, APP, pn * 100, 100))
    res = tr.on_ack_received(APP, 5, 0, [(1, 1)])
    assert sorted(p.pn for p in res.newly_acked) == [1, 2, 5] and tr.count == 3
    tr = m.SentPacketTracker(4)                                           # capacity_limit
    assert all(tr.on_packet_sent(pkt(pn, INITIAL, pn * 100, 100)) for pn in range(4))
    assert not tr.on_packet_sent(pkt(4, INITIAL, 400, 100))
    tr = m.SentPacketTracker(16)                                          # sent_below_pn_filtering
    for pn, ts in ((0, 100), (1, 200), (5, 300)):
        tr.on_packet_sent(pkt(pn, APP, ts, 100))
    assert len(tr.sent_below_pn(APP, 3)) == 2
    tr = m.SentPacketTracker(16)                                          # drop_space_removes_all
    for pn, lvl in ((0, INITIAL), (1, HANDSHAKE), (2, APP)):
        tr.on_packet_sent(pkt(pn, lvl, 100, 100))
    tr.drop_space(INITIAL)
    assert tr.count == 2 and not tr.has_ack_eliciting_in_flight(INITIAL) and tr.has_ack_eliciting_in_flight(HANDSHAKE)
    tr = m.SentPacketTracker(16)                                          # has_ack_eliciting_in_flight_correctness
    tr.on_packet_sent(pkt(0, INITIAL, 100, 100))
    tr.on_packet_sent(m.SentPacket(1, HANDSHAKE, 200, 100, flags=rc.USED | rc.IN_FLIGHT))
    assert tr.has_ack_eliciting_in_flight(INITIAL) and not tr.has_ack_eliciting_in_flight(HANDSHAKE)
    tr = m.SentPacketTracker(16)                                          # remove_packet
    tr.on_packet_sent(pkt(0, INITIAL, 100, 100))
    tr.on_packet_sent(pkt(1, INITIAL, 200, 100))
    assert tr.remove(INITIAL, 0).pn == 0 and tr.count == 1 and tr.remove(INITIAL, 0) is None
    tr = m.SentPacketTracker(16)                                          # ack_wrong_level_is_noop
    tr.on_packet_sent(pkt(0, INITIAL, 100, 100))
    assert len(tr.on_ack_received(APP, 0, 0, []).newly_acked) == 0 and tr.count == 1


def test_model_congestion_rs():
    cc = m.CongestionController(1200)                                     # initial_state
    assert (cc.cwnd, cc.ssthresh, cc.bytes_in_flight, cc.in_slow_start()) == (14_720, m.U64, 0, True)
    assert m.CongestionController(1500).cwnd == 15_000                    # initial_window_large_mds
    cc.on_packet_sent(1200)                                               # slow_start_increase
    cc.on_packet_acked(1200, 1000)
    assert (cc.cwnd, cc.bytes_in_flight) == (14_720 + 1200, 0)
    cc = m.CongestionController(1200)                                     # slow_start_to_congestion_avoidance
    for i in range(10):
        cc.on_packet_sent(1200)
        cc.on_packet_acked(1200, i * 1000)
    before = cc.cwnd
    cc.on_packet_sent(1200)
    cc.on_packet_lost(1200, 11_000, 12_000)
    assert cc.ssthresh == cc.cwnd == max(before // 2, 2400) == 13_360 and not cc.in_slow_start()
    cc = m.CongestionController(1200)                                     # congestion_avoidance_increase
    cc.on_packet_sent(1200)
    cc.on_packet_lost(1200, 1000, 2000)
    after = cc.cwnd
    cc.on_packet_sent(1200)
    assert cc.on_packet_acked(1200, 3000) == "avoidance" and cc.cwnd == after + 1200 * 1200 // after == 7360 + 195
    cc = m.CongestionController(1200)                                     # loss_triggers_recovery, no_double_recovery
    cc.on_packet_lost(1200, 1000, 2000)
    assert cc.in_recovery(1000) and cc.in_recovery(2000) and not cc.in_recovery(2001)
    assert not cc.on_packet_lost(1200, 500, 3000) and cc.cwnd == 7360
    cc = m.CongestionController(1200)                                     # acked_during_recovery_no_increase
    cc.on_packet_sent(1200)
    cc.on_packet_sent(1200)
    cc.on_packet_lost(1200, 1000, 2000)
    assert cc.on_packet_acked(1200, 1500) == "recovery" and cc.cwnd == 7360 and cc.bytes_in_flight == 0


def test_model_ladder_expectations():
    got = {}
    for name, n, pre, sends, recs, drop, flags in m.ladder_cases():
        if not name.endswith("-1"):
            continue
        rows = m.state_rows(n, pre)
        if sends:
            rows, _ = m.run_sent(*m.make_sends(sends), rows)
        arena, pkts, dg, now, fr = m.make_batch(recs, n)
        got[name[:-2]] = m.run_recovery(arena, pkts, len(pkts), dg, now, fr, len(fr), drop, rows, flags)
    ev = lambda name, k=0: got[name][1][k]  # noqa: E731
    assert got["send_129th"][0][0]["count"] == 128 and got["send_129th"][0][0]["bytes_in_flight"] == 128 * 1200 + 1300
    assert (ev("acked_32")["n_acked"], ev("acked_32")["n_acked_cc"]) == (32, 32)
    assert (ev("acked_33")["n_acked"], ev("acked_33")["n_acked_cc"]) == (33, 32)
    assert (got["acked_32"][0][0]["bytes_in_flight"], got["acked_33"][0][0]["bytes_in_flight"]) == (0, 1200)   # the 33rd stays in flight
    assert (ev("lost_64")["n_lost"], ev("lost_64")["flags"] & rc.LOST_CUT) == (64, 0)
    assert (ev("lost_65")["n_lost"], ev("lost_65")["flags"] & rc.LOST_CUT) == (64, rc.LOST_CUT)
    assert got["lost_64"][0][0]["loss_time"][2] == 3950 and not got["lost_65"][0][0]["have"] & rc.HAVE_LOSS_TIME << 2
    assert got["lost_65_timer_before_break"][0][0]["loss_time"][2] == 3990
    assert (ev("pairs_16")["n_acked"], ev("pairs_16")["flags"] & rc.RANGES_CUT) == (17, 0)
    assert (ev("pairs_17")["n_acked"], ev("pairs_17")["flags"] & rc.RANGES_CUT) == (17, rc.RANGES_CUT)
    assert (ev("break_first_pair")["n_acked"], ev("break_first_pair")["flags"] & rc.RANGES_BROKE) == (5, rc.RANGES_BROKE)
    assert (ev("break_middle_pair")["n_acked"], ev("break_middle_pair")["flags"] & rc.RANGES_BROKE) == (5, rc.RANGES_BROKE)
    assert ev("break_then_cut")["flags"] & 6 == 6 and ev("first_range_above_largest")["n_acked"] == 6
    assert ev("varint_widths")["n_acked"] == 11
    assert len(got["arena_end_exact"][1]) == 1 and len(got["arena_end_one_past"][1]) == 0 and len(got["not_selected"][1]) == 1
    assert [int(x) for x in got["level_mismatch"][1]["n_acked"]] == [1, 1] and got["level_mismatch"][0][0]["count"] == 10
    assert got["largest_acked_already_above"][0][0]["largest_acked"][2] == 50
    assert not ev("time_sent_zero")["flags"] & rc.RTT and not ev("now_before_time_sent")["flags"] & rc.RTT
    assert [int(p["pn"]) for p in got["time_sent_eq_lost_send_time"][2]] == [0]
    srtt = lambda name: int(got[name][0][0]["smoothed_rtt"])  # noqa: E731
    assert srtt("ack_delay_above_max") == srtt("ack_delay_below_max") == 112_500
    assert (srtt("ack_delay_above_max_confirmed"), srtt("ack_delay_below_max_confirmed")) == (109_375, 111_250)
    assert srtt("ack_delay_not_subtracted_confirmed") == 102_500
    row, evs, lost, _ = got["recovery_sequence"]
    assert [int(x) for x in evs["n_lost"]] == [2, 3, 1, 3] and row[0]["recovery_start_time"] == 400_000
    assert (row[0]["cwnd"], row[0]["ssthresh"]) == (7960 + 1200 * 1200 // 7960, 7960)   # one entry, one ack in avoidance
    assert got["cwnd_eq_ssthresh"][0][0]["cwnd"] == 14_720 + 97 + 97
    assert got["cwnd_below_ssthresh_by_one"][0][0]["cwnd"] == 14_720 + 1200 + 1200 * 1200 // 15_920
    assert [(int(p["pn"]), int(p["size"])) for p in got["duplicate_pn_lost_later_slot"][2]] == [(7, 111)]
    assert [int(p["size"]) for p in got["duplicate_pn_both_lost"][2]] == [111, 222]
    row = got["drop_mask_alone"][0][0]
    assert (row["count"], row["have"] & 0x1FF, row["bytes_in_flight"]) == (5, rc.HAVE_LAST_SENT << 2, 5 * 1200 + 1100)
    assert srtt("handshake_done_then_ack_client") == 109_375
    assert srtt("handshake_done_ignored_as_server") == (7 * 112_500 + 200_600) // 8    # both ACKs give a sample
    assert got["handshake_done_then_ack_client"][0][0]["count"] == 0 and len(got["handshake_done_then_ack_client"][1]) == 2
    assert got["pto_backoff_reset"][0][0]["pto_count"] == 0


# ---- 2. the shared integer code on the host ----------------------------------------------------------------------
def host_batches():
    out = [(n, pre, sends, recs, drop, flags, 0) for _, n, pre, sends, recs, drop, flags in m.ladder_cases()]
    for seed in (1, 2, 3):
        pre, sends, recs, drop, flags = m.fuzz_batch(seed)
        out.append((64, pre, sends, recs, drop, flags, seed))
    return out


def test_recovery_host_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    blob, n_cases, n_sends, n_acks, n_lost = [], 0, 0, 0, 0
    for n, pre, sends, recs, drop, flags, seed in host_batches():
        rows0 = m.state_rows(n, pre)
        t0 = np.zeros(n, dtype=np.uint64)
        rows1, t1 = (rows0, t0)
        by_conn = {}
        if sends:
            reqs, status, ln, now = m.make_sends(sends)
            rows1, t1 = m.run_sent(reqs, status, ln, now, rows0, t0)
            for i, q in enumerate(reqs):
                if status[i] == 0 and q["conn"] < n and q["level"] < 3:
                    by_conn.setdefault(int(q["conn"]), []).append(struct.pack("<QQII", int(q["pn"]), int(now[i]), int(ln[i]), int(q["level"])))
        arena, pkts, dg, now_d, fr = m.make_batch(recs, n, seed)
        rows2, evts, lost, t2 = m.run_recovery(arena, pkts, len(pkts), dg, now_d, fr, len(fr), drop, rows1, flags, t0)
        ev_of = {int(e["frame"]): e for e in evts}
        rec_of = {}
        for k, c, src, d in m.selected(len(arena), pkts, len(pkts), dg, fr, len(fr), n, flags):
            f = fr[k]
            data = bytes(arena[src:src + int(f["data_len"])])
            b = struct.pack("<IIQQQQI", int(f["type"]), int(f["level"]), int(f["v"][0]), int(f["v"][1]), int(f["v"][3]),
                            int(now_d[d]), len(data)) + data
            if k in ev_of:
                e = ev_of[k]
                b += struct.pack("<IIIIQ", int(e["n_acked"]), int(e["n_acked_cc"]), int(e["n_lost"]), int(e["flags"]),
                                 int(e["largest_newly_acked"]))
                for p in lost[int(e["lost_first"]):int(e["lost_first"]) + int(e["n_lost"])]:
                    b += struct.pack("<QII", int(p["pn"]), int(p["size"]), int(p["level"]))
                n_acks += 1
                n_lost += int(e["n_lost"])
            rec_of.setdefault(c, []).append(b)
        for c in range(n):
            s, r = by_conn.get(c, []), rec_of.get(c, [])
            blob.append(rows0[c].tobytes() + struct.pack("<I", len(s)) + b"".join(s) + rows1[c].tobytes() + struct.pack("<Q", int(t1[c])))
            blob.append(struct.pack("<II", int(drop[c]) if drop is not None else 0, len(r)) + b"".join(r))
            blob.append(rows2[c].tobytes() + struct.pack("<Q", int(t2[c])))
            n_cases += 1
            n_sends += len(s)
    assert n_cases > 600 and n_sends > 5000 and n_acks > 1500 and n_lost > 300
    table = tmp_path / "cases.bin"
    table.write_bytes(struct.pack("<I", n_cases) + b"".join(blob))
    exe = tmp_path / "test_recovery_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_recovery_host.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"recovery host ok {n_cases} cases {n_sends} sends {n_acks} acks {n_lost} lost" in r.stdout


# ---- 3. ABI ------------------------------------------------------------------------------------------------------
def test_recovery_abi_structs():
    assert (rc.SENT_DTYPE.itemsize, rc.CONN_RECOVERY_DTYPE.itemsize, rc.EVT_DTYPE.itemsize, rc.LOST_DTYPE.itemsize) == \
        (24, 3264, 32, 16)
    off = lambda dt, f: dt.fields[f][1]  # noqa: E731
    assert [off(rc.SENT_DTYPE, f) for f in ("pn", "time_sent", "size", "level", "flags", "reserved")] == [0, 8, 16, 18, 19, 20]
    assert [off(rc.CONN_RECOVERY_DTYPE, f) for f in (
        "largest_acked", "time_of_last_ack_eliciting", "loss_time", "smoothed_rtt", "rttvar", "min_rtt", "latest_rtt",
        "max_ack_delay", "cwnd", "ssthresh", "bytes_in_flight", "recovery_start_time", "persistent_congestion_threshold",
        "max_datagram_size", "minimum_window", "have", "pto_count", "count", "flags", "reserved", "sent")] == \
        [0, 24, 48, 72, 80, 88, 96, 104, 112, 120, 128, 136, 144, 152, 160, 168, 172, 176, 180, 184, 192]
    assert [off(rc.EVT_DTYPE, f) for f in ("frame", "conn", "n_acked", "n_acked_cc", "n_lost", "flags", "lost_first",
                                           "reserved", "largest_newly_acked")] == [0, 4, 8, 10, 12, 14, 16, 20, 24]
    assert [off(rc.LOST_DTYPE, f) for f in ("pn", "conn", "size", "level", "reserved")] == [0, 8, 12, 14, 15]
    assert (rc.SLOTS, rc.CLIENT, rc.CONFIRMED) == (128, 1, 1)
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("MQ_SENT_SLOTS", "128"), ("MQ_SENT_USED", "0x01"), ("MQ_SENT_ACK_ELICITING", "0x02"),
                        ("MQ_SENT_IN_FLIGHT", "0x04"), ("MQ_RECOVERY_CONFIRMED", "0x01"), ("MQ_RECOVERY_CLIENT", "0x01"),
                        ("MQ_ACKEVT_RTT", "0x01"), ("MQ_ACKEVT_RANGES_CUT", "0x02"), ("MQ_ACKEVT_RANGES_BROKE", "0x04"),
                        ("MQ_ACKEVT_LOST_CUT", "0x08")):
        assert re.search(r"#define %s\s+%s\b" % (name, value), text), name
    for name, size in (("mq_sent_pkt", 24), ("mq_conn_recovery", 3264), ("mq_ack_evt", 32), ("mq_lost_pkt", 16)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), text), name
    for cite in ("transmit.rs:610-619, 743-752", "recv.rs:563-612", "recv.rs:692-704", "recovery.rs:162-171",
                 "loss.rs:283-288", "loss.rs:68-101", "loss.rs:117-172", "loss.rs:188-260", "congestion.rs:54-72",
                 "congestion.rs:75-87", "mod.rs:322", "mod.rs:566-568"):
        assert cite in text, cite


def test_recovery_state_init(mqlib):
    assert mqlib.mq_recovery_state_init(None, 25_000, 1200) == _lib.MQ_ERR_INVALID_ARG
    for delay, mds in ((25_000, 1200), (0, 1500), (7, 1472), (1 << 40, 65_527)):
        row = np.full(1, 0xFF, dtype=np.uint8).repeat(rc.CONN_RECOVERY_DTYPE.itemsize).view(rc.CONN_RECOVERY_DTYPE)
        assert mqlib.mq_recovery_state_init(row.ctypes.data_as(ctypes.c_void_p), delay, mds) == 0
        assert row.tobytes() == m.state_rows(1, None, delay, mds).tobytes()
        assert rc.state_rows(3, delay, mds).tobytes() == m.state_rows(3, None, delay, mds).tobytes()
    assert (m.state_rows(1)[0]["cwnd"], m.state_rows(1, None, 0, 1500)[0]["cwnd"]) == (14_720, 15_000)


def test_recovery_argument_checks_without_device(mqlib):
    # the argument check comes before the device check, and nothing is launched: these hold with and
    # without a GPU (the pointers are never dereferenced)
    INV = _lib.MQ_ERR_INVALID_ARG
    A, odd, odd4 = 0x1000, 0x1008, 0x1004
    f = mqlib.mq_batch_recovery

    def call(arena=A, arena_len=1 << 20, pkts=A, n_pkts=A, max_pkts=4, dgrams=A, n_dgrams=4, dgram_now=A, frames=A,
             n_frames=A, max_frames=8, drop=None, rec=A, n_conns=2, evts=A, n_evts=A, lost=A, max_lost=8, n_lost=A,
             timeouts=None, flags=0, ws=A):
        return f(arena, arena_len, pkts, n_pkts, max_pkts, dgrams, n_dgrams, dgram_now, frames, n_frames, max_frames,
                 drop, rec, n_conns, evts, n_evts, lost, max_lost, n_lost, timeouts, flags, ws, None)

    for bad in (dict(arena=None), dict(pkts=None), dict(n_pkts=None), dict(dgrams=None), dict(dgram_now=None),
                dict(frames=None), dict(n_frames=None), dict(evts=None), dict(rec=None), dict(n_evts=None),
                dict(n_lost=None), dict(lost=None), dict(ws=None), dict(ws=None, max_frames=0),
                dict(n_evts=None, max_frames=0), dict(n_lost=None, max_frames=0), dict(rec=None, max_frames=0),
                dict(lost=None, max_frames=0), dict(max_frames=(1 << 26) + 1), dict(n_conns=(1 << 30) + 1),
                dict(pkts=odd), dict(dgrams=odd), dict(frames=odd), dict(rec=odd), dict(evts=odd), dict(lost=odd),
                dict(ws=odd), dict(dgram_now=odd4), dict(timeouts=odd4)):
        assert call(**bad) == INV, bad
    g = mqlib.mq_batch_sent

    def sent(reqs=A, status=A, pkt_len=A, n=5, now=A, rec=A, n_conns=2, timeouts=None, ws=A):
        return g(reqs, status, pkt_len, n, now, rec, n_conns, timeouts, ws, None)

    for bad in (dict(reqs=None), dict(status=None), dict(pkt_len=None), dict(now=None), dict(rec=None), dict(ws=None),
                dict(ws=None, n=0), dict(rec=None, n=0), dict(n=(1 << 26) + 1), dict(n_conns=(1 << 30) + 1),
                dict(reqs=odd), dict(rec=odd), dict(ws=odd), dict(now=odd4), dict(timeouts=odd4), dict(pkt_len=0x1002)):
        assert sent(**bad) == INV, bad
    assert mqlib.mq_batch_recovery_workspace_size(0, 0) > 0 and mqlib.mq_batch_sent_workspace_size(0, 0) > 0
    assert mqlib.mq_batch_recovery_workspace_size(1 << 20, 4096) >= (48 << 20) + 4096 * 2048
    assert mqlib.mq_batch_sent_workspace_size(1 << 20, 4096) >= 16 << 20
    import torch
    if not torch.cuda.is_available():  # no device: nothing falls back to the host
        ND = _lib.MQ_ERR_NO_DEVICE
        assert call() == ND and call(max_frames=0, arena=None, pkts=None, frames=None, evts=None, dgram_now=None) == ND
        assert call(n_conns=0, rec=None) == ND and call(max_lost=0, lost=None) == ND and call(timeouts=odd, drop=0x1001) == ND
        assert sent() == ND and sent(n=0, reqs=None, status=None, pkt_len=None, now=None) == ND
        assert sent(n_conns=0, rec=None) == ND and sent(timeouts=odd, status=0x1001, pkt_len=odd4) == ND


# ---- 4. what the chained test's traffic must contain ----------------------------------------------------------------
def test_chained_traffic_coverage(orc):
    inputs, rows1, (rows2, evts, lost, _), cov = m.chained_expectation(orc)
    for what in ("rtt_sample", "pn_threshold_loss", "time_threshold_loss", "recovery_entry", "ack_avoidance", "full_tracker"):
        assert cov.get(what, 0) >= 1, (what, cov)
    assert len(evts) > 150 and len(lost) > 20 and (rows2["flags"] & rc.CONFIRMED).sum() >= 2
    assert rows1[0]["count"] == 128 and inputs["n_acks"] >= 3 * len(rows1) - 4
