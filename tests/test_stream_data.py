"""Stream bookkeeping and delivery without a GPU: the Python model (stream_data_model.py) against the
reference's own unit-test cases, the kernels' shared integer code (milli_quic_amd/csrc/mq_stream_data.h)
replayed on the host against the model, the C ABI's struct sizes, constants and argument checks, and the
coverage that the fuzz batches of the GPU test must have.

tests/csrc/test_stream_data_host.cpp is built with g++ -fsanitize=address,undefined and run as its own
process; it reads a table of per-connection sequences and expected outcomes that this test writes from
the model."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from milli_quic_amd import _lib
from milli_quic_amd import stream_data as sd

import stream_data_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_run(recs, n_conns, pre, params, seed=0):
    arena, pkts, dg, fr = m.make_batch(recs, n_conns, seed)
    streams, bufs = m.state_rows(n_conns, params["stream_buf"], pre)
    out = m.run(arena, pkts, len(pkts), dg, fr, len(fr), streams, bufs, params["stream_buf"], params["initial_max"],
                sd.CLIENT if params["client"] else 0)
    return (arena, pkts, dg, fr, streams, bufs), out


def buffer_of(streams, bufs, stream_buf, conn, sid):
    row = streams[conn]["buf"]
    s = next(s for s in range(sd.SLOTS) if row[s]["used"] and row[s]["stream_id"] == sid)
    at = (conn * sd.SLOTS + s) * stream_buf
    return row[s], bufs[at:at + int(row[s]["len"])].tobytes()


# ---- the reference's unit cases ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", m.REFERENCE_BUF_CASES, ids=[c[0] for c in m.REFERENCE_BUF_CASES])
def test_model_reference_buffer_cases(case):
    # stream_recv_buf_tests (mod.rs:2116-2198); stream id 5 as the client, where the reference calls
    # store_stream_data directly with id 4
    name, frames_, data, next_offset, fin = case
    P = dict(stream_buf=64, initial_max=65536, client=True)
    _, (streams, bufs, evts) = model_run([m.S(0, 5, off, d, f) for off, d, f in frames_], 1, None, P)
    hdr, got = buffer_of(streams, bufs, 64, 0, 5)
    assert got == data and hdr["next_offset"] == next_offset and bool(hdr["fin_received"]) == fin
    assert len(evts) == len(frames_) and (evts["flags"] & sd.READABLE).all()


def test_model_reference_stream_map_cases():
    P = dict(stream_buf=64, initial_max=65536, client=True)
    # get_or_create_rejects_own_stream_type (stream.rs:781-789): nothing created, the frame has no stream
    _, (st, _, ev) = model_run([m.S(0, 0, 0, 3)], 1, None, P)
    assert not st["map"]["flags"].any() and ev["mark"][0] == 0xFF and ev["store"][0] == sd.STORE_NONE
    # get_or_create_peer_bidi (:791-799) and _peer_uni (:801-809)
    _, (st, _, ev) = model_run([m.S(0, 1, 0, 3), m.S(0, 3, 0, 3)], 1, None, P)
    assert [int(x) for x in st["map"][0]["id"][:2]] == [1, 3]
    assert st["map"][0]["flags"][0] == sd.USED | sd.HAS_RECV | sd.HAS_SEND
    assert st["map"][0]["flags"][1] == sd.USED | sd.HAS_RECV
    assert (st["max_bidi_remote"][0], st["max_uni_remote"][0]) == (1, 1)
    # get_or_create_returns_existing (:811-818)
    _, (st, _, ev) = model_run([m.S(0, 1, 0, 3), m.S(0, 1, 3, 3)], 1, None, P)
    assert list(ev["map_slot"]) == [0, 0] and list(ev["flags"] & sd.NEW_STREAM) == [1, 0]
    assert ((st["map"][0]["flags"] & sd.USED) != 0).sum() == 1
    # recv_data_past_fin_offset (:823-840): FIN at 100 via (50, 50, fin); the simplified offset jumps to 100,
    # so the state is DataRecvd and (100, 10) is an error
    _, (st, _, ev) = model_run([m.S(0, 1, 0, 100, True)], 1, None, dict(P, stream_buf=128))
    assert ev["mark"][0] == sd.MARK_OK and st["map"][0]["recv_state"][0] == sd.DATA_RECVD
    _, (st, _, ev) = model_run([m.S(0, 1, 50, 50, True), m.S(0, 1, 100, 10)], 1, None, P)
    assert list(ev["mark"]) == [sd.MARK_OK, sd.STREAM_STATE_ERROR]
    assert st["map"][0]["fin_offset"][0] == 100 and st["map"][0]["recv_state"][0] == sd.DATA_RECVD
    # recv_auto_max_stream_data (:872-882): 600 of 1000 bytes -> remaining 400 < 500 -> next = 600 + 1000
    _, (st, _, ev) = model_run([m.S(0, 1, 0, 600)], 1, None, dict(P, stream_buf=1024, initial_max=1000))
    e = st["map"][0][0]
    assert e["recv_max_data_next"] == 1600 > e["recv_max_data"] == 1000 and e["recv_offset"] == 600


def test_model_ladder_expectations():
    got = {}
    for name, n_conns, recs, pre, P in m.ladder_cases():
        got[name] = model_run(recs, n_conns, pre, P)[1]
    ev = got["flow_control_after_fin"][2]
    e = got["flow_control_after_fin"][0]["map"][0][0]
    assert ev["mark"][1] == sd.FLOW_CONTROL_ERROR and ev["store"][1] == sd.STORE_COPIED and ev["copy_len"][1] == 30
    assert (e["recv_state"], e["fin_offset"], e["recv_offset"], e["flags"] & sd.HAS_FIN) == (sd.SIZE_KNOWN, 40, 10, sd.HAS_FIN)
    assert list(got["final_size_beyond_fin"][2]["mark"][2:3]) == [sd.FINAL_SIZE_ERROR]
    assert list(got["final_size_other_fin"][2]["mark"][2:3]) == [sd.FINAL_SIZE_ERROR]
    ev = got["reset_then_stream"][2]
    assert list(ev["mark"]) == [0, 0, sd.STREAM_STATE_ERROR, sd.STREAM_STATE_ERROR] and ev["store"][2] == sd.STORE_COPIED
    assert list(got["reset_other_final_size"][2]["mark"][[1, 5]]) == [sd.FINAL_SIZE_ERROR] * 2
    ev = got["full_buffer_then_fin"][2]
    assert ev["copy_len"][1] == 0 and ev["flags"][1] & sd.TRUNCATED and ev["flags"][1] & sd.FIN_SET
    ev = got["fin_on_gap_not_set"][2]
    assert ev["store"][1] == sd.STORE_GAP and not ev["flags"][1] & sd.FIN_SET
    assert not got["fin_on_gap_not_set"][0]["buf"][0]["fin_received"][0]
    ev = got["33_ids"][2]
    assert list(ev["map_slot"][:33]) == list(range(32)) + [sd.NONE] and list(ev["mark"][32:35]) == [0xFF, 0xFF, 0xFF]
    assert ev["map_slot"][35] == 7
    ev = got["33_buffers"][2]
    assert list(ev["store"]) == [sd.STORE_NO_BUFFER, sd.STORE_COPIED, sd.STORE_NO_BUFFER]
    ev = got["seeded_local_uni_no_recv"][2]
    assert list(ev["mark"]) == [sd.INVALID_STATE] * 3 and list(ev["store"]) == [4, 0, 4]
    assert got["auto_tune_wraps"][0]["map"][0][0]["recv_max_data_next"] == 6
    assert got["end_at_varint_max"][0]["buf"][0][3]["next_offset"] == m.VARINT_MAX
    assert len(got["not_selected_each_kind"][2]) == 2
    st = got["clamped_on_load"][0]["buf"][0][0]
    assert (st["len"], st["read_offset"]) == (64, 9) and got["clamped_on_load"][2]["flags"][0] & sd.TRUNCATED
    ev = got["copy_alignments"][2]
    assert len({int(x) % 16 for x in ev["src"]}) == 16 and len({int(x) % 16 for x in ev["dst"]}) == 16
    assert (ev["store"] == sd.STORE_COPIED).all() and not (ev["flags"] & sd.TRUNCATED).any()


def test_model_read():
    P = dict(stream_buf=64, initial_max=65536, client=True)
    recs = [m.S(0, 5, 0, 40), m.S(0, 9, 0, 10, True), m.S(1, 5, 0, 0, True), m.S(1, 9, 0, 7)]
    _, (st, bufs, _) = model_run(recs, 2, None, P)
    reqs = np.zeros(9, dtype=sd.READ_REQ_DTYPE)
    reqs["conn"] = [0, 0, 0, 1, 1, 1, 2, 0, 0]
    reqs["stream_id"] = [5, 9, 5, 5, 9, 13, 5, 9, 5]
    reqs["cap"] = [16, 64, 16, 8, 0, 8, 8, 8, 200]
    reqs["out_offset"] = [0, 16, 80, 96, 104, 104, 104, 104, 0]
    out = np.full(128, m.GUARD, dtype=np.uint8)
    st2, out2, res = m.read(st, bufs, 64, reqs, out)
    assert [tuple(int(x) for x in r)[:4] for r in res] == [
        (16, 0, 0, 0), (10, 0, 1, 1), (0, 9, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, sd.WOULD_BLOCK, 0, sd.NONE),
        (0, 3, 0, sd.NONE), (0, 9, 0, 1), (0, 3, 0, sd.NONE)]
    assert out2[:16].tobytes() == bufs[:16].tobytes() and out2[16:26].tobytes() == bufs[64:74].tobytes()
    assert (out2[26:] == m.GUARD).all()
    assert list(st2["buf"][0]["used"][:2]) == [1, 0] and list(st2["buf"][1]["used"][:2]) == [0, 1]
    assert st2["buf"][0]["read_offset"][0] == 16
    # the rest of stream 5, then WouldBlock: no FIN was received
    st3, out3, res3 = m.read(st2, bufs, 64, reqs[:1].copy(), out)
    reqs2 = reqs[:2].copy()
    reqs2["stream_id"], reqs2["cap"] = [5, 5], [64, 64]
    st4, _, res4 = m.read(st3, bufs, 64, reqs2[:1], out)
    st5, _, res5 = m.read(st4, bufs, 64, reqs2[:1], out)
    assert (res3["copied"][0], res4["copied"][0], res5["status"][0]) == (16, 8, sd.WOULD_BLOCK)


# ---- the shared integer code on the host ---------------------------------------------------------------------
def host_cases():
    """Per-connection sequences: (params, state before, records with outcomes, state after, reads, state after the
    reads) from every ladder case and every connection of the fuzz batches."""
    batches = [(recs, n, pre, P, 0) for _, n, recs, pre, P in m.ladder_cases()]
    for seed in (1, 2, 3):
        recs, pre, P = m.fuzz_batch(seed)
        batches.append((recs, 40, pre, P, seed))
    recs, pre, P = m.fuzz_batch(4, client=False)
    batches.append((recs, 40, pre, P, 4))
    cases = []
    for recs, n_conns, pre, P, seed in batches:
        (arena, pkts, dg, fr, st0, bufs0), (st1, bufs1, evts) = model_run(recs, n_conns, pre, P, seed)
        for c in range(n_conns):
            ev = evts[evts["conn"] == c]
            used = [s for s in range(sd.SLOTS) if st1[c]["buf"][s]["used"]]
            reqs = np.zeros(len(used), dtype=sd.READ_REQ_DTYPE)
            reqs["conn"], reqs["stream_id"] = c, [st1[c]["buf"][s]["stream_id"] for s in used]
            reqs["cap"] = [(0, 5, 1 << 18)[(s + c) % 3] for s in used]
            reqs["out_offset"] = np.cumsum(reqs["cap"]) - reqs["cap"]
            st2, _, res = m.read(st1, bufs1, P["stream_buf"], reqs, np.zeros(int(reqs["cap"].sum()), dtype=np.uint8))
            cases.append((P, st0[c], ev, fr, st1[c], reqs, res, st2[c]))
    return cases


def test_stream_data_host_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    cases = host_cases()
    blob = [struct.pack("<I", len(cases))]
    n_recs = n_reads = 0
    for P, before, ev, fr, after, reqs, res, after_reads in cases:
        blob.append(struct.pack("<IQI", P["stream_buf"], P["initial_max"], int(P["client"])) + before.tobytes())
        blob.append(struct.pack("<I", len(ev)))
        for e in ev:
            f = fr[int(e["frame"])]
            t = int(f["type"])
            a, ln = (int(f["v"][2]), 0) if t == 0x04 else (int(f["v"][1]), int(f["data_len"]))
            blob.append(struct.pack("<IIQQIHH5B3x", t, ln, int(f["v"][0]), a, int(e["dst"]), int(e["copy_len"]),
                                    int(e["skip"]), int(e["map_slot"]), int(e["buf_slot"]), int(e["mark"]),
                                    int(e["store"]), int(e["flags"])))
        blob.append(after.tobytes() + struct.pack("<I", len(reqs)))
        for q, r in zip(reqs, res):
            blob.append(struct.pack("<IIIBB2x", int(r["slot"]), int(q["cap"]), int(r["copied"]), int(r["status"]),
                                    int(r["fin"])))
        blob.append(after_reads.tobytes())
        n_recs += len(ev)
        n_reads += len(reqs)
    assert n_recs > 8000 and n_reads > 1000
    table = tmp_path / "cases.bin"
    table.write_bytes(b"".join(blob))
    exe = tmp_path / "test_stream_data_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_stream_data_host.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"stream data host ok {len(cases)} cases {n_recs} records {n_reads} reads" in r.stdout


# ---- ABI -----------------------------------------------------------------------------------------------------
def test_stream_data_abi_structs():
    assert (sd.ENTRY_DTYPE.itemsize, sd.BUF_DTYPE.itemsize, sd.CONN_STREAMS_DTYPE.itemsize, sd.EVT_DTYPE.itemsize,
            sd.READ_REQ_DTYPE.itemsize, sd.READ_RES_DTYPE.itemsize) == (48, 32, 2592, 32, 32, 8)
    off = lambda dt, f: dt.fields[f][1]  # noqa: E731
    assert [off(sd.ENTRY_DTYPE, f) for f in ("id", "recv_offset", "recv_max_data", "recv_max_data_next", "fin_offset",
                                             "flags", "recv_state", "reserved")] == [0, 8, 16, 24, 32, 40, 41, 42]
    assert [off(sd.BUF_DTYPE, f) for f in ("stream_id", "next_offset", "len", "read_offset", "used", "fin_received",
                                           "reserved")] == [0, 8, 16, 20, 24, 25, 26]
    assert [off(sd.CONN_STREAMS_DTYPE, f) for f in ("map", "buf", "max_bidi_remote", "max_uni_remote", "reserved")] == \
        [0, 1536, 2560, 2568, 2576]
    assert [off(sd.EVT_DTYPE, f) for f in ("frame", "conn", "src", "dst", "copy_len", "skip", "map_slot", "buf_slot",
                                           "mark", "store", "flags", "type", "reserved")] == \
        [0, 4, 8, 16, 20, 22, 24, 25, 26, 27, 28, 29, 30]
    assert [off(sd.READ_REQ_DTYPE, f) for f in ("conn", "cap", "stream_id", "out_offset", "reserved")] == [0, 4, 8, 16, 24]
    assert [off(sd.READ_RES_DTYPE, f) for f in ("copied", "status", "fin", "slot", "reserved")] == [0, 4, 5, 6, 7]
    assert (sd.SLOTS, sd.CLIENT, sd.WOULD_BLOCK) == (32, 1, 11)
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define MQ_STREAM_SLOTS\s+32\b", text) and re.search(r"#define MQ_STREAMS_CLIENT\s+0x01\b", text)
    assert re.search(r"#define MQ_STREAM_WOULD_BLOCK\s+11\b", text)
    for name, size in (("mq_stream_entry", 48), ("mq_stream_buf", 32), ("mq_conn_streams", 2592), ("mq_stream_evt", 32)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), text), name
    for cite in ("recv.rs:620-644", "stream.rs:227-280, 325-388", "mod.rs:769-842", "mod.rs:660-687", "stream.rs:405-424",
                 "recv.rs:661-669", "recv.rs:529-542", "Cargo.toml:9"):
        assert cite in text, cite


def test_stream_data_argument_checks_without_device(mqlib):
    # the argument check comes before the device check, and nothing is launched: these hold with and
    # without a GPU (the pointers are never dereferenced)
    INV = _lib.MQ_ERR_INVALID_ARG
    A, odd = 0x1000, 0x1008
    f = mqlib.mq_batch_stream_data

    def call(arena=A, arena_len=1 << 20, pkts=A, n_pkts=A, max_pkts=4, dgrams=A, n_dgrams=4, frames=A, n_frames=A,
             max_frames=8, streams=A, n_conns=2, bufs=A, stream_buf=64, initial_max=65536, flags=0, evts=A, n_evts=A,
             ws=A):
        return f(arena, arena_len, pkts, n_pkts, max_pkts, dgrams, n_dgrams, frames, n_frames, max_frames, streams,
                 n_conns, bufs, stream_buf, initial_max, flags, evts, n_evts, ws, None)

    for bad in (dict(arena=None), dict(pkts=None), dict(n_pkts=None), dict(dgrams=None), dict(frames=None),
                dict(n_frames=None), dict(evts=None), dict(streams=None), dict(bufs=None), dict(n_evts=None),
                dict(ws=None), dict(ws=None, max_frames=0), dict(n_evts=None, max_frames=0),
                dict(streams=None, max_frames=0), dict(bufs=None, max_frames=0),
                dict(max_frames=(1 << 26) + 1), dict(n_conns=(1 << 30) + 1),
                dict(stream_buf=0), dict(stream_buf=8), dict(stream_buf=72), dict(stream_buf=(1 << 24) + 16),
                dict(pkts=odd), dict(dgrams=odd), dict(frames=odd), dict(streams=odd), dict(evts=odd), dict(ws=odd)):
        assert call(**bad) == INV, bad
    g = mqlib.mq_batch_stream_read

    def read(streams=A, n_conns=2, bufs=A, stream_buf=64, reqs=A, n_reqs=3, out=A, out_len=64, res=A, ws=A):
        return g(streams, n_conns, bufs, stream_buf, reqs, n_reqs, out, out_len, res, ws, None)

    for bad in (dict(streams=None), dict(bufs=None), dict(reqs=None), dict(out=None), dict(res=None), dict(ws=None),
                dict(ws=None, n_reqs=0), dict(n_reqs=(1 << 26) + 1), dict(n_conns=(1 << 30) + 1), dict(stream_buf=0),
                dict(stream_buf=24), dict(stream_buf=1 << 25), dict(streams=odd), dict(reqs=odd), dict(ws=odd),
                dict(res=0x1004)):
        assert read(**bad) == INV, bad
    assert mqlib.mq_batch_stream_data_workspace_size(0, 0) > 0
    assert mqlib.mq_batch_stream_data_workspace_size(1 << 20, 4096) >= 28 << 20
    assert mqlib.mq_batch_stream_read_workspace_size(1000, 10) >= 4 * (1000 + 320)
    import torch
    if not torch.cuda.is_available():  # no device: nothing falls back to the host
        ND = _lib.MQ_ERR_NO_DEVICE
        assert call() == ND and call(max_frames=0) == ND and call(n_conns=0, streams=None, bufs=None) == ND
        assert call(max_frames=0, arena=None, pkts=None, frames=None, evts=None) == ND
        assert call(stream_buf=16) == ND and call(stream_buf=1 << 24) == ND
        assert read() == ND and read(n_reqs=0, streams=None, bufs=None, reqs=None, out=None, res=None) == ND
        assert read(res=odd) == ND                         # the results are 8-byte entries


# ---- what the fuzz batches must contain ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_coverage(seed):
    recs, pre, P = m.fuzz_batch(seed)
    (_, _, _, _, st0, _), (st1, _, evts) = model_run(recs, 40, pre, P, seed)
    cov = m.fuzz_coverage(st0, st1, evts)
    for k, v in cov.items():
        assert v >= (20 if k.startswith(("mark_", "store_")) else 1), (k, cov)
    assert 1500 < len(evts) < 4000
