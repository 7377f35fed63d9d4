"""ACK tracking and building without a GPU: the Python model (acks_model.py) against the reference's own
unit-test cases, its frames through the frame model's decoder, the kernels' shared integer code
(milli_quic_amd/csrc/mq_acks.h) replayed on the host against the model, and the C ABI's struct sizes
and argument checks.

tests/csrc/test_acks_host.cpp is built with g++ -fsanitize=address,undefined and run as its own
process; it reads a table of sequences and expected trackers and frames that this test writes from
the model, and replays every sequence packet number by packet number and run by run."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from milli_quic_amd import _lib, acks

import acks_model as am
import frames_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recorded(pns, pre=()):
    t = am.Tracker(pre)
    for pn in pns:
        t.record(pn)
    return t


def test_model_reference_tracker_cases():
    # recv_pn_tracker_tests (mod.rs:1980-2076), values restated
    for name, pns, want in am.REFERENCE_CASES:
        assert recorded(pns).ranges == want, name
    assert recorded([5]).largest() == 5 and recorded([]).largest() is None
    t = recorded(100 * i for i in range(32))                      # full_tracker_drops_lowest_range
    assert len(t.ranges) == 32 and t.ranges[0] == (0, 0)
    t.record(5000)
    assert len(t.ranges) == 32 and t.ranges[0] == (100, 100) and t.ranges[31] == (5000, 5000)
    # the lowest range goes even when the new PN lies below every range: it becomes the new lowest
    t = recorded([100 * i + 1000 for i in range(32)] + [3])
    assert len(t.ranges) == 32 and t.ranges[0] == (3, 3) and t.ranges[1] == (1100, 1100)
    # so the result depends on arrival order: not "the top 32 ranges of the set"
    assert recorded([3] + [100 * i + 1000 for i in range(32)]).ranges[0] == (1000, 1000)


def test_model_reference_build_cases():
    # build_ack_frame_{single_range, multiple_ranges, empty_tracker_returns_none} (transmit.rs:1201-1280)
    f = am.build_ack_frame(recorded([0, 1, 2]).ranges)
    assert f == bytes([0x02, 2, 0, 0, 2])
    f = am.build_ack_frame(recorded([0, 1, 5, 6, 10]).ranges)
    assert len(f) > 5 and f == bytes([0x02, 10, 0, 2, 0, 2, 1, 2, 1])  # [10,10]; gap 2 -> [5,6]; gap 2 -> [0,1]
    assert am.build_ack_frame(recorded([]).ranges) is None
    assert len(am.build_ack_frame(am.wide_ranges())) == 515 <= acks.FRAME_MAX


def ranges_of_frame(frame):
    """The frame through the frame model's decoder: type 0x02, and the tracker its fields spell."""
    f, used = fm.decode(frame)
    assert used == len(frame) and f["type"] == 0x02 and f["aux"] == 0
    largest, delay, count, first = f["v"]
    assert delay == 0
    raw = frame[f["data_pos"]:f["data_pos"] + f["data_len"]]
    out, smallest = [(largest - first, largest)], largest - first
    for _ in range(count):
        gap, n1 = fm.decode_varint(raw)
        length, n2 = fm.decode_varint(raw[n1:])
        assert raw[:n1] == fm.encode_varint(gap) and raw[n1:n1 + n2] == fm.encode_varint(length)  # shortest form
        raw = raw[n1 + n2:]
        end = smallest - gap - 2
        out.insert(0, (end - length, end))
        smallest = end - length
    assert raw == b""
    return out


def test_model_frames_decode():
    for name, n_conns, events, pre in am.ladder_cases():
        pkts, dg, summ, flags = am.make_batch(events, n_conns)
        trackers, _, _ = am.run(pkts, len(pkts), dg, am.tracker_rows(n_conns, pre), np.zeros(n_conns, np.uint32), summ)
        for row in trackers:
            ranges = am.load_tracker(row).ranges
            frame = am.build_ack_frame(ranges)
            assert (frame is None) == (not ranges), name
            if frame is not None:
                assert ranges_of_frame(frame) == ranges, name


def test_model_bookkeeping():
    ev = [(0, 2, 1), (1, 0, 5), (1, 2, 9), (2, 1, 4), (0, 2, 3, "frame")]
    pkts, dg, summ, flags = am.make_batch(ev, 4)
    assert list(flags) == [4, 5, 2, 0]
    pend = np.array([0, 0, 0, 1], dtype=np.uint32)               # connection 3: pending, but nothing tracked
    b = dict(max_acks=2, out_stride=100, flags=acks.CLIENT, largest_pn=[[7, 8, 9]] * 4, next_pn=list(range(12)))
    tr, p, out = am.run(pkts, len(pkts), dg, am.tracker_rows(4), pend, summ, flags, b)
    assert out["n_acks"] == 4 and len(out["frames"]) == 2 and list(p) == [0, 4, 2, 1]
    assert list(out["reqs"]["conn"]) == [0, 1] and list(out["reqs"]["level"]) == [2, 0]
    assert list(out["reqs"]["flags"]) == [0, 1] and list(out["reqs"]["pn"]) == [2, 3]
    assert list(out["next_pn"]) == [0, 1, 3, 4, 4, 5, 6, 7, 8, 9, 10, 11]
    assert am.load_tracker(tr[2]).ranges == [(1, 1)]              # the MQ_ERR_FRAME packet is not recorded
    tr2, _, _ = am.run(pkts, len(pkts), dg, am.tracker_rows(4), pend, None, flags)
    assert am.load_tracker(tr2[2]).ranges == [(1, 1), (3, 3)]     # ... unless no summary is given
    b["next_pn"] = out["next_pn"]
    tr3, p3, out3 = am.run(pkts[:0], 0, dg, tr, p, None, None, b)   # the next call builds the remainder
    assert out3["n_acks"] == 2 and list(out3["reqs"]["conn"]) == [1, 2] and list(p3) == [0, 0, 0, 1]
    b0 = dict(b, max_acks=0)
    _, p4, out4 = am.run(pkts[:0], 0, dg, tr, p, None, None, b0)
    assert out4["n_acks"] == 2 and list(p4) == list(p) and len(out4["reqs"]) == 0


def host_cases():
    """(pre, pns) per tracker: the reference cases, every tracker of the ladder, and random sequences."""
    cases = [((), pns) for _, pns, _ in am.REFERENCE_CASES]
    for name, n_conns, events, pre in am.ladder_cases():
        per = {}
        for ev in events:
            if len(ev) == 3:
                per.setdefault(3 * ev[0] + ev[1], []).append(ev[2])
        cases += [(tuple((pre or {}).get(t, ())), pns) for t, pns in per.items()]
    rng = np.random.default_rng(5)
    for k in range(3000):
        n = int(rng.integers(1, 400))
        cases.append(((), am.fuzz_sequence(rng, n, start=int(rng.integers(0, 1 << int(rng.integers(1, 50)))),
                                           stretch=(80, 12, 3)[k % 3])))
    return cases


def test_acks_host_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    cases = host_cases()
    blob = [struct.pack("<I", len(cases))]
    n_full = 0
    for pre, pns in cases:
        t = recorded(pns, pre)
        n_full += len(t.ranges) == 32
        frame = am.build_ack_frame(t.ranges) or b""
        blob.append(struct.pack("<I", len(pre)) + b"".join(struct.pack("<QQ", *r) for r in pre))
        blob.append(struct.pack("<I", len(pns)) + np.asarray(pns, dtype="<u8").tobytes())
        blob.append(struct.pack("<I", len(t.ranges)) + b"".join(struct.pack("<QQ", *r) for r in t.ranges))
        blob.append(struct.pack("<I", len(frame)) + frame)
    assert n_full > 300  # the random sequences overflow the cap often enough
    table = tmp_path / "cases.bin"
    table.write_bytes(b"".join(blob))
    exe = tmp_path / "test_acks_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_acks_host.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"acks host ok {len(cases)} cases" in r.stdout and f"{n_full} full longest 515" in r.stdout


def test_acks_abi_structs():
    assert acks.TRACKER_DTYPE.itemsize == 528 and ctypes.sizeof(_lib.AckBuild) == 56
    from milli_quic_amd import send
    assert send.REQ_DTYPE.itemsize == 48
    off = lambda dt, f: dt.fields[f][1]  # noqa: E731
    assert [off(acks.TRACKER_DTYPE, f) for f in ("n", "reserved", "range")] == [0, 4, 16]
    assert [getattr(_lib.AckBuild, f).offset for f in ("ack_frames", "reqs", "n_acks", "conns", "next_pn", "max_acks",
                                                       "out_stride", "flags", "reserved")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert (acks.RANGES, acks.FRAME_MAX, acks.CLIENT) == (32, 528, 1)
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define MQ_PN_TRACKER_RANGES\s+32\b", text) and re.search(r"#define MQ_ACK_FRAME_MAX\s+528\b", text)
    assert re.search(r"#define MQ_ACKS_CLIENT\s+0x01\b", text)
    for cite in ("recv.rs:248-249", "mod.rs:194-296", "mod.rs:224-278", "transmit.rs:321-380", "mod.rs:482-508",
                 "recv.rs:231-257", "transmit.rs:169-173", "transmit.rs:188", "Cargo.toml:9"):
        assert cite in text, cite


def test_acks_argument_checks_without_device(mqlib):
    # the argument check comes before the device check, and nothing is launched: these hold with and
    # without a GPU (the pointers are never dereferenced)
    INV = _lib.MQ_ERR_INVALID_ARG
    A = 0x1000   # a non-NULL, 16-byte aligned pointer that an argument error never reaches
    odd = 0x1008
    f = mqlib.mq_batch_acks

    def build(**kw):
        b = _lib.AckBuild()
        b.ack_frames, b.reqs, b.n_acks, b.conns, b.next_pn = A, A, A, A, A
        b.max_acks, b.out_stride = 4, 64
        for k, v in kw.items():
            setattr(b, k, v)
        return ctypes.byref(b)

    def call(pkts=A, n_dev=A, max_pkts=4, summary=None, dgrams=A, n_dgrams=4, conn_flags=None, trackers=A, pending=A,
             n_conns=2, build=None, ws=A):
        return f(pkts, n_dev, max_pkts, summary, dgrams, n_dgrams, conn_flags, trackers, pending, n_conns, build, ws, None)

    for bad in (dict(pkts=None), dict(n_dev=None), dict(dgrams=None), dict(trackers=None), dict(pending=None),
                dict(ws=None), dict(ws=None, max_pkts=0), dict(max_pkts=(1 << 24) + 1), dict(n_conns=(1 << 30) + 1),
                dict(pkts=odd), dict(summary=odd), dict(dgrams=odd), dict(trackers=odd), dict(ws=odd),
                dict(build=build(ack_frames=None)), dict(build=build(reqs=None)), dict(build=build(n_acks=None)),
                dict(build=build(conns=None)), dict(build=build(next_pn=None)), dict(build=build(out_stride=0)),
                dict(build=build(reqs=odd)), dict(build=build(conns=odd)), dict(build=build(n_acks=None, max_acks=0))):
        assert call(**bad) == INV, bad
    assert mqlib.mq_batch_acks_workspace_size(0, 0) > 0
    assert mqlib.mq_batch_acks_workspace_size(1 << 20, 4096) >= 40 << 20
    import torch
    if not torch.cuda.is_available():  # no device: nothing falls back to the host
        assert call() == _lib.MQ_ERR_NO_DEVICE
        assert call(max_pkts=0) == _lib.MQ_ERR_NO_DEVICE
        assert call(build=build()) == _lib.MQ_ERR_NO_DEVICE
        assert call(build=build(max_acks=0, ack_frames=None, reqs=None)) == _lib.MQ_ERR_NO_DEVICE
        assert call(pkts=None, n_dev=None, dgrams=None, max_pkts=0) == _lib.MQ_ERR_NO_DEVICE
