"""Datagram routing without a GPU: the Python model (route_model.py) against the reference's
decode_dcid cases, the kernels' shared integer code (milli_quic_amd/csrc/mq_route.h) replayed on the
host against the model, and the C ABI's struct sizes and argument checks.

tests/csrc/test_route_host.cpp is built with g++ -fsanitize=address,undefined and run as its own
process; it reads a table of expected outcomes that this test writes from the model: every datagram
length 0-40, both header forms, DCID lengths 0-21, version 0 and non-zero, the four long-header
types."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from milli_quic_amd import _lib, packet, recv, route

import route_model
from route_model import TableModel, decode_dcid, route_cid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DCID = bytes([1, 2, 3, 4])


def test_model_reference_decode_dcid_cases():
    # reference src/packet/mod.rs:295-314: decode_dcid_long_header / decode_dcid_short_header
    hdr, _ = packet.initial_header(DCID, b"\x0a\x0b", b"", 1, 10)
    buf = hdr + bytes(256 - len(hdr))
    assert decode_dcid(buf, 4) == DCID
    hdr, _ = packet.short_header(DCID, 1)
    assert hdr[0] == 0x40
    assert decode_dcid(hdr + bytes(64 - len(hdr)), 4) == DCID


def test_model_decode_dcid_none_branches():
    hdr, _ = packet.initial_header(DCID, b"", b"", 1, 10)
    assert decode_dcid(b"", 4) is None                      # empty
    assert decode_dcid(hdr[:5], 4) is None                  # 5 bytes of a long header
    assert decode_dcid(hdr[:6 + 3], 4) is None              # one byte short of the DCID's end
    assert decode_dcid(hdr[:6 + 4], 4) == DCID
    short, _ = packet.short_header(DCID, 1)
    assert decode_dcid(short[:4], 4) is None                # short header, one byte short
    assert decode_dcid(short[:5], 4) == DCID
    assert decode_dcid(bytes([0x40]), 0) == b""             # the empty CID is a CID
    # ours: a long-header DCID over 20 bytes is no table key
    long21 = bytes([0xC0, 0, 0, 0, 1, 21]) + bytes(21)
    assert decode_dcid(long21, 4) == bytes(21) and route_cid(long21, 4) is None


def test_model_route_steps():
    m = TableModel(capacity=3)
    assert m.insert([b"", DCID], [7, 8]) == [route.OK, route.OK]
    assert m.insert([DCID, bytes(21)], [9, 9]) == [route.HIT, route.MALFORMED] and m.map[DCID] == 8
    ini = lambda cid, pad=0: bytes([0xC3, 0, 0, 0, 1, len(cid)]) + cid + bytes(pad)  # noqa: E731
    blobs = [bytes([0x40]) + DCID, ini(b"\x55" * 5, 40), ini(b"\x66" * 5, 40), ini(b"\x55" * 5, 40), ini(DCID),
             bytes([0xE0, 0, 0, 0, 1, 2, 9, 9]) + bytes(40), bytes([0xC0, 0, 0, 0, 0, 2, 9, 9]) + bytes(40),
             ini(b"\x77", 2), b""]
    arena = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    dg = np.zeros(len(blobs) + 1, dtype=recv.DGRAM_DTYPE)
    dg["len"][:-1] = [len(b) for b in blobs]
    dg["offset"][:-1] = np.cumsum([0] + [len(b) for b in blobs[:-1]])
    dg[-1] = (len(arena) - 1, 2, 0)  # ends one byte past the arena
    st, conn = m.route(arena, dg, 4)
    U, M = route.UNKNOWN, route.MALFORMED
    assert list(st) == [route.HIT, U, U, U, route.HIT, U, U, U, M, M]
    conns = np.zeros(8, dtype=recv.CONN_DTYPE)
    adm = route_model.AdmitModel(conns, conn_base=2, max_new=4, row_first=10, min_initial_len=40)
    st, conn = m.route(arena, dg, 4, adm)
    # capacity 3, two live: one group admitted (the first by arrival), the second FULL; Handshake,
    # version 0 and the short Initial stay UNKNOWN
    assert list(st) == [route.HIT, route.NEW, route.FULL, route.NEW, route.HIT, U, U, U, M, M]
    assert list(conn[:5]) == [8, 2, route.CONN_NONE, 2, 8] and adm.new_dcids == [b"\x55" * 5]
    assert conns[2]["initial_row"] == 10 and conns[2]["flags"] == recv.HAS_INITIAL and conns[2]["dcid_len"] == 4
    assert m.remove([DCID, DCID]) == [route.OK, route.UNKNOWN]


def host_cases(rng):
    """(datagram, short_dcid_len, min_initial_len) over every length 0-40."""
    cases = []
    for ln in range(41):
        for L in range(22):
            for typ in range(4):
                for version in (0, 1, 0x01000000):
                    b0 = 0x80 | typ << 4 | int(rng.integers(0, 16)) | (0x40 if rng.random() < 0.5 else 0)
                    d = bytes([b0]) + version.to_bytes(4, "big") + bytes([L]) + rng.bytes(40)
                    cases.append((d[:ln], int(rng.integers(0, 21)), int(rng.choice([0, 20, 30]))))
        for sdl in range(21):
            d = bytes([int(rng.integers(0, 128))]) + rng.bytes(40)
            cases.append((d[:ln], sdl, 0))
    return cases


def test_route_header_host_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    rng = np.random.default_rng(11)
    seed = bytes(range(16))
    lines, n_cid, n_adm = [], 0, 0
    for d, sdl, min_len in host_cases(rng):
        cid = route_cid(d, sdl)
        adm = cid is not None and route_model.admissible(d, min_len)
        n_cid += cid is not None
        n_adm += adm
        want = "M" if cid is None else (cid.hex() or "-")
        lines.append(f"D {d.hex() or '-'} {sdl} {min_len} {want} {int(adm)}")
    assert n_cid > 1000 and n_adm > 100 and len(lines) - n_cid > 1000
    hashed = [b"", b"\0", DCID, bytes(20), bytes(range(20)), rng.bytes(8), rng.bytes(19)]
    lines += [f"H {seed.hex()} {c.hex() or '-'}" for c in hashed]
    table = tmp_path / "cases.txt"
    table.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "test_route_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_route_host.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"route host ok {len(lines) - len(hashed)}" in r.stdout
    # the Python restatement of the hash (used by the forced-collision GPU test) is the C++ one
    got = dict(l.split()[1:] for l in r.stdout.splitlines() if l.startswith("H "))
    for c in hashed:
        assert int(got[c.hex() or "-"], 16) == route_model.sip13_cid(seed, c), c.hex()
    assert route_model.hash_class(seed, b"", 4) != route_model.hash_class(seed, b"\0", 4)


def test_route_abi_structs():
    assert ctypes.sizeof(_lib.RouteAdmit) == 56
    assert _lib.RouteAdmit.n_conns.offset == 8 and _lib.RouteAdmit.min_initial_len.offset == 24
    assert _lib.RouteAdmit.new_dcids.offset == 32 and _lib.RouteAdmit.n_new.offset == 48
    assert recv.DGRAM_DTYPE.itemsize == 16 and recv.DGRAM_DTYPE.fields["conn"][1] == 12
    assert recv.CONN_DTYPE.itemsize == 64
    assert (route.HIT, route.NEW, route.UNKNOWN, route.MALFORMED, route.FULL, route.DEFERRED) == (0, 1, 2, 3, 4, 5)
    assert route.CONN_NONE == 0xFFFFFFFF
    import re
    text = open(_lib.HEADER_PATH).read()
    for name, val in (("HIT", 0), ("NEW", 1), ("UNKNOWN", 2), ("MALFORMED", 3), ("FULL", 4), ("DEFERRED", 5)):
        assert re.search(rf"#define MQ_ROUTE_{name}\s+{val}\b", text), name
    for cite in ("decode_dcid.rs:9-37", "recv.rs:275-278", "§5.2", "§14.1", "§17.2"):
        assert cite in text, cite


def test_route_argument_checks_without_device(mqlib):
    # the argument check comes before the device check, and nothing is launched: these hold with and
    # without a GPU (the pointers are never dereferenced)
    INV = _lib.MQ_ERR_INVALID_ARG
    fake = ctypes.c_void_p(0x1000)  # a non-NULL table / buffer that an argument error never reaches
    h = ctypes.c_void_p()
    assert mqlib.mq_cid_table_create(8, None, ctypes.byref(h)) == INV
    assert mqlib.mq_cid_table_create(8, bytes(16), None) == INV
    assert mqlib.mq_cid_table_insert(None, None, None, None, 0, None, None) == INV
    assert mqlib.mq_cid_table_insert(fake, None, fake, fake, 1, fake, None) == INV
    assert mqlib.mq_cid_table_insert(fake, fake, fake, fake, 1, None, None) == INV
    assert mqlib.mq_cid_table_remove(fake, fake, None, 1, fake, None) == INV
    assert mqlib.mq_cid_table_remove(None, None, None, 0, None, None) == INV
    assert mqlib.mq_cid_table_compact(None, None) == INV
    assert mqlib.mq_cid_table_stats(None, None, None, None, None) == INV
    assert mqlib.mq_debug_cid_table_hash_bits(None, 4) == INV
    assert mqlib.mq_debug_cid_table_hash_bits(fake, 0) == INV
    mqlib.mq_cid_table_free(None)
    r = mqlib.mq_batch_route
    assert r(fake, fake, 100, fake, 1, 21, None, fake, fake, None) == INV          # short_dcid_len > 20
    assert r(fake, None, 100, fake, 1, 8, None, fake, fake, None) == INV           # NULL with n > 0
    assert r(fake, fake, 100, None, 1, 8, None, fake, fake, None) == INV
    assert r(fake, fake, 100, fake, 1, 8, None, None, fake, None) == INV
    assert r(None, fake, 100, fake, 1, 8, None, fake, fake, None) == INV
    adm = _lib.RouteAdmit(conns=0x1000, n_conns=8, conn_base=5, max_new=4, row_first=0, min_initial_len=1200,
                          new_dcids=0x1000, new_dcid_lens=0x1000, n_new=0x1000)
    assert r(fake, fake, 100, fake, 1, 8, ctypes.byref(adm), fake, fake, None) == INV  # conn_base + max_new > n_conns
    adm.conn_base = 4
    assert r(fake, fake, 100, fake, 1, 8, ctypes.byref(adm), fake, None, None) == INV  # admission needs the workspace
    adm.n_new = None
    assert r(fake, fake, 100, fake, 1, 8, ctypes.byref(adm), fake, fake, None) == INV
    assert mqlib.mq_batch_route_workspace_size(0) > 0
    assert mqlib.mq_batch_route_workspace_size(1 << 20) >= (32 + 4 + 4 + 4 + 16 + 8) << 20
    import torch
    if not torch.cuda.is_available():  # no device: a table cannot exist, and nothing falls back to the host
        assert mqlib.mq_cid_table_create(8, bytes(16), ctypes.byref(h)) == _lib.MQ_ERR_NO_DEVICE
        with pytest.raises(Exception):
            route.CidTable(8, bytes(16))
