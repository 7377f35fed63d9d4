"""The frame index without a GPU: the Python model (frames_model.py) against the reference's own
frame/mod.rs unit-test cases and the committed packets, the kernels' shared integer code
(milli_quic_amd/csrc/mq_frames.h) replayed on the host against the model, and the C ABI's struct
sizes and argument checks.

tests/csrc/test_frames_host.cpp is built with g++ -fsanitize=address,undefined and run as its own
process; it reads a table of payloads and expected outcomes that this test writes from the model."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from milli_quic_amd import _lib, frames
from milli_quic_amd.batch import make_descs

import frames_model as fm
from frames_model import FrameEncodingError, build, decode, vi, walk
from helpers import curl_desc_and_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fails(buf):
    with pytest.raises(FrameEncodingError):
        decode(buf)
    return True


def test_model_varint():
    # RFC 9000 A.1 examples (the reference's varint tests use the same four)
    for hexs, val in (("c2197c5eff14e88c", 151288809941952652), ("9d7f3e7d", 494878333), ("7bbd", 15293), ("25", 37),
                      ("4025", 37)):
        b = bytes.fromhex(hexs)
        assert fm.decode_varint(b) == (val, len(b))
    for w in (1, 2, 4, 8):
        assert fm.decode_varint(vi(5, w) + b"\xff") == (5, w)
    for b in (b"", b"\x40", b"\x80\x00\x00", b"\xc0" + bytes(6)):
        with pytest.raises(fm.BufferTooSmall):
            fm.decode_varint(b)
    assert fm.decode_varint(vi(fm.VARINT_MAX))[0] == (1 << 62) - 1


def test_model_reference_unit_cases():
    # reference src/frame/mod.rs tests, values restated
    assert decode(b"\x00") == (dict(type=0, v=[0, 0, 0, 0], data_pos=0, data_len=0, aux=0), 1)
    assert decode(b"\x01")[0]["type"] == 1 and decode(b"\x1e")[0]["type"] == 0x1E
    f, n = decode(build(0x02, (42, 10, 0, 5)))                      # roundtrip_ack_no_ranges_no_ecn
    assert (f["v"], f["data_len"], n) == ([42, 10, 0, 5], 0, 5)
    f, n = decode(build(0x02, (100, 50, 1, 10, 2, 3)))              # roundtrip_ack_with_ranges
    assert f["v"] == [100, 50, 1, 10] and (f["data_pos"], f["data_len"]) == (6, 2) and n == 8
    f, n = decode(build(0x03, (200, 25, 0, 0, 10, 20, 5)))          # roundtrip_ack_with_ecn
    assert f["v"] == [200, 25, 0, 0] and f["aux"] == 6 and n == 9
    f, n = decode(b"\x08" + vi(5) + b"abc")                         # decode_stream_no_length_bit
    assert (f["v"][0], f["v"][1], f["data_pos"], f["data_len"], n) == (5, 0, 2, 3, 5)
    f, n = decode(build(0x06, (0, 0)))                              # roundtrip_crypto_empty
    assert (f["data_pos"], f["data_len"], n) == (3, 0, 3)
    f, n = decode(build(0x18, (1, 0, 4), bytes([1, 2, 3, 4]) + b"\xaa" * 16))  # roundtrip_new_connection_id
    assert (f["v"][:2], f["data_pos"], f["data_len"], f["aux"], n) == ([1, 0], 4, 4, 8, 24)
    f, n = decode(build(0x1C, (0x0A, 0x06, 4), b"oops"))            # connection_close_transport
    assert (f["v"][:2], f["data_len"]) == ([0x0A, 0x06], 4)
    f, n = decode(build(0x1D, (0x0A, 4), b"oops"))
    assert (f["v"][:2], f["data_len"]) == ([0x0A, 0], 4)
    assert fails(b"")                                               # decode_empty_buffer
    assert fails(vi(0x1F))                                          # decode_unknown_frame_type
    assert fails(vi(0x04))                                          # decode_truncated_reset_stream
    assert fails(vi(0xFF)) and fails(vi(0x1000))                    # unknown_frame_type_{large,2byte}_varint
    assert fails(build(0x18, (0, 0, 21)))                           # new_connection_id_cid_too_long
    assert fails(build(0x18, (0, 0, 21), bytes(21 + 16)))           # ... whatever follows
    big = (1 << 62) - 1                                             # roundtrip_large_varint_values
    assert decode(build(0x04, (big, big, big)))[0]["v"] == [big, big, big, 0]
    for t in range(0x08, 0x10):                                     # stream_all_flag_combinations
        body = [4] + ([9] if t & 4 else []) + ([3] if t & 2 else [])
        f, n = decode(build(t, body, b"xyz"))
        assert (f["type"], f["v"][0], f["v"][1], f["data_len"]) == (t, 4, 9 if t & 4 else 0, 3)
    # decode_multiple_frames_sequentially, as dispatch_frames walks them
    s, recs = walk(b"\x01" + build(0x10, (1000,)) + build(0x19, (7,)))
    assert s["status"] == fm.OK and [r[2] for r in recs] == [1, 0x10, 0x19] and [r[0] for r in recs] == [0, 1, 4]
    # ack_with_many_ranges: 20 pairs; the records keep the raw bytes, the 16-range cap is the consumer's
    f, n = decode(build(0x02, (1000, 0, 20, 0) + (1, 1) * 20))
    assert f["data_len"] == 40
    # 2-, 4- and 8-byte encodings of a type are accepted; lengths past 2^32 do not wrap
    assert decode(vi(1, 8))[1] == 8 and decode(vi(0, 2))[0]["type"] == 0
    assert fails(build(0x06, (0, (1 << 32) + 2), b"ab"))


def test_model_summary():
    s, recs = walk(b"")
    assert s == dict(status=fm.OK, err_pos=0, n_padding=0, flags=0, close=False) and recs == []
    s, recs = walk(bytes(5) + build(0x02, (1, 0, 0, 0)) + bytes(3))
    assert (s["n_padding"], s["flags"], len(recs)) == (8, 0, 1)          # ACK and PADDING elicit nothing
    s, recs = walk(b"\x01" + build(0x1C, (1, 2, 0)) + b"\x1f\x01")
    assert (s["status"], s["err_pos"], s["flags"], s["close"], len(recs)) == (fm.ERR_FRAME, 5, 1, True, 2)


def _open_vector(orc, p):
    km = _lib.KeyMaterial()
    km.suite = p["suite"]
    for name in ("key", "iv", "hp"):
        b = bytes.fromhex(p[name])
        getattr(km, name)[:len(b)] = list(b)
    arena = np.frombuffer(bytes.fromhex(p["protected"]), dtype=np.uint8).copy()
    flags = _lib.MQ_PKT_LONG_HEADER if p["long_header"] else 0
    opn = make_descs([0], [p["len"]], [0], [p["largest_pn"]], [p["pn_offset"]], [0], [flags])
    st, _ = orc.batch_open([km], arena, opn, _lib.MQ_SUITE_MIXED)
    assert st[0] == 0
    return arena.tobytes()[p["pn_offset"] + p["pn_len"]:p["len"] - 16]


def test_model_committed_packets(orc, packet_vectors, ref_fixtures):
    by = {p["name"]: p for p in packet_vectors}
    a2 = _open_vector(orc, by["rfc9001-A.2"])                            # the client Initial
    s, recs = walk(a2)
    assert len(a2) == 1162 and s["status"] == fm.OK and s["flags"] == 1
    assert [(r[2], r[6][1], r[4]) for r in recs] == [(0x06, 0, 241)] and s["n_padding"] == 1162 - recs[0][1]
    s, recs = walk(_open_vector(orc, by["rfc9001-A.3"]))                 # the server Initial
    assert s["status"] == fm.OK and s["n_padding"] == 0
    assert [(r[2], r[6], r[4]) for r in recs] == [(0x02, [0, 0, 0, 0], 0), (0x06, [0, 0, 0, 0], 90)]
    s, recs = walk(_open_vector(orc, by["rfc9001-A.5"]))                 # the ChaCha20 short-header packet
    assert s["status"] == fm.OK and [r[2] for r in recs] == [0x01] and s["n_padding"] == 0
    # the reference's captured curl Initial
    data, dcid, pn_offset, length, client = curl_desc_and_keys(orc, ref_fixtures, orc.derive_initial_secrets)
    km = _lib.KeyMaterial()
    km.suite = _lib.MQ_SUITE_AES128GCM
    km.key[:16] = list(orc.hkdf_expand_label(client, b"quic key", b"", 16)[1])
    km.iv[:12] = list(orc.hkdf_expand_label(client, b"quic iv", b"", 12)[1])
    km.hp[:16] = list(orc.hkdf_expand_label(client, b"quic hp", b"", 16)[1])
    arena = np.frombuffer(data, dtype=np.uint8).copy()
    opn = make_descs([0], [pn_offset + length], [0], [0], [pn_offset], [0], [_lib.MQ_PKT_LONG_HEADER])
    st, _ = orc.batch_open([km], arena, opn, _lib.MQ_SUITE_AES128GCM)
    assert st[0] == 0
    pn_len = int(arena[0] & 3) + 1
    s, recs = walk(arena.tobytes()[pn_offset + pn_len:pn_offset + length - 16])
    # it starts with a CRYPTO frame at payload position 0 (curl sends its ClientHello in pieces, out of
    # order: this first piece carries the stream bytes from 756 on)
    assert s["status"] == fm.OK and recs[0][0] == 0 and recs[0][2] == 0x06 and recs[0][6][1] == 756
    assert {r[2] for r in recs} <= {0x01, 0x06} and s["flags"] == 1
    assert sum(r[1] for r in recs) + s["n_padding"] == length - pn_len - 16


def test_case_tables_cover_both_sides():
    cases = fm.host_cases() + fm.padding_cases()
    st = [walk(c)[0]["status"] for c in cases]
    assert st.count(fm.OK) > 300 and st.count(fm.ERR_FRAME) > 1000
    types = {r[2] for c in cases for r in walk(c)[1]}
    assert types == set(range(0x01, 0x1F))
    # the fuzz leaves at least a quarter of its packets clean and at least a quarter erroring
    for seed in (1, 2, 3):
        batch = fm.fuzz_batch(seed, 3000)
        assert all(1 <= len(p) <= 1400 for p in batch)
        st = [walk(p)[0]["status"] for p in batch]
        assert st.count(fm.OK) >= 750 and st.count(fm.ERR_FRAME) >= 750, (seed, st.count(fm.OK))


def test_frames_host_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    cases = fm.host_cases() + fm.padding_cases() + fm.fuzz_batch(9, 300)
    blob = [struct.pack("<I", len(cases))]
    n_err = 0
    for c in cases:
        s, recs = walk(c)
        n_err += s["status"] == fm.ERR_FRAME
        blob.append(struct.pack("<I", len(c)) + c)
        blob.append(struct.pack("<HHHBB", len(recs), s["err_pos"], s["n_padding"], s["status"], s["flags"]))
        arr = np.zeros(len(recs), dtype=frames.FRAME_DTYPE)
        for k, (pos, used, t, dp, dl, aux, v) in enumerate(recs):
            arr[k] = (0, pos, used, t, 0, dp, dl, aux, v)
        blob.append(arr.tobytes())
    table = tmp_path / "cases.bin"
    table.write_bytes(b"".join(blob))
    exe = tmp_path / "test_frames_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_frames_host.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"frames host ok {len(cases)} cases" in r.stdout and f"{n_err} errors" in r.stdout


def test_frames_abi_structs():
    assert frames.FRAME_DTYPE.itemsize == 48 and frames.PKT_FRAMES_DTYPE.itemsize == 16
    off = lambda dt, f: dt.fields[f][1]  # noqa: E731
    assert [off(frames.FRAME_DTYPE, f) for f in ("pkt", "pos", "len", "type", "level", "data_pos", "data_len", "aux",
                                                 "v")] == [0, 4, 6, 8, 9, 10, 12, 14, 16]
    assert [off(frames.PKT_FRAMES_DTYPE, f) for f in ("first", "n_frames", "err_pos", "n_padding", "status", "flags",
                                                      "reserved")] == [0, 4, 6, 8, 10, 11, 12]
    assert (frames.ERR_FRAME, frames.SKIPPED, frames.ACK_ELICITING, frames.CONN_CLOSE, frames.CONN_ERROR) == \
        (10, 0xFF, 1, 8, 16)
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define MQ_ERR_FRAME\s+10\b", text) and re.search(r"#define MQ_FRAMES_SKIPPED\s+0xFF\b", text)
    for cite in ("recv.rs:518-545", "mod.rs:228-461", "mod.rs:183-190", "mod.rs:200-207", "recv.rs:533-539",
                 "recv.rs:235-237", "recv.rs:231-257"):
        assert cite in text, cite
    assert _lib.status_str(frames.ERR_FRAME) == "frame encoding"


def test_frames_argument_checks_without_device(mqlib):
    # the argument check comes before the device check, and nothing is launched: these hold with and
    # without a GPU (the pointers are never dereferenced)
    INV = _lib.MQ_ERR_INVALID_ARG
    A = ctypes.c_void_p(0x1000)   # a non-NULL, 16-byte aligned pointer that an argument error never reaches
    odd = ctypes.c_void_p(0x1008)
    f = mqlib.mq_batch_frames

    def call(arena=A, pkts=A, n_dev=A, max_pkts=4, dgrams=None, n_dgrams=0, summary=A, recs=A, max_frames=8, n_frames=A,
             conn_flags=None, n_conns=0, ws=A):
        return f(arena, 100, pkts, n_dev, max_pkts, dgrams, n_dgrams, summary, recs, max_frames, n_frames, conn_flags,
                 n_conns, ws, None)

    for bad in (dict(arena=None), dict(pkts=None), dict(n_dev=None), dict(summary=None), dict(recs=None),
                dict(n_frames=None), dict(ws=None), dict(n_frames=None, max_pkts=0), dict(ws=None, max_pkts=0),
                dict(dgrams=A, n_dgrams=1), dict(conn_flags=A, n_conns=1), dict(max_pkts=(1 << 24) + 1),
                dict(pkts=odd), dict(summary=odd), dict(recs=odd), dict(ws=odd),
                dict(dgrams=odd, n_dgrams=1, conn_flags=A, n_conns=1)):
        assert call(**bad) == INV, bad
    assert mqlib.mq_batch_frames_workspace_size(0) > 0
    assert mqlib.mq_batch_frames_workspace_size(1 << 20) >= 8 << 20
    import torch
    if not torch.cuda.is_available():  # no device: nothing falls back to the host
        assert call() == _lib.MQ_ERR_NO_DEVICE
        assert call(max_pkts=0) == _lib.MQ_ERR_NO_DEVICE
        assert call(recs=None, max_frames=0) == _lib.MQ_ERR_NO_DEVICE
