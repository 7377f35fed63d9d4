"""Throughput of the SURVEY §8f components on one MI355X (device-resident, HIP events on the launch
stream; median of `reps`). Prints one JSON object; the round's copy lives in profiles/.

  derive   mq_batch_derive_initial: 2^20 client DCIDs (8 B) -> 2^21 key-table rows
  protect  mq_batch_protect: 2^20 x 1171-B frames -> 1200-B 1-RTT packets (ChaCha20, 4096 keys)
  recv     mq_batch_recv: the same 2^20 packets as one-packet datagrams of 4096 connections (and of
           1024, 64, 4, 1 connections); a 4096-datagram sample byte-checked against the oracle
  records  mq_batch_seal_records / open_records: 2^20 x 1200-B and 2^16 x 16 KiB TLS records
           (AES-128-GCM)
  hp_mask  mq_batch_hp_mask (SURVEY §8d "mask-only timing"): 2^20 16-B samples -> 5-B masks,
           AES-128 (config C keys) and ChaCha20 (config B keys)
  rekey    mq_batch_derive_keys / mq_batch_key_update: 2^20 traffic secrets -> rows, per suite; a
           4096-row sample of the key material byte-checked against the host functions; the host
           path (HKDF per row + one mq_keytable_update) over 2^14 of the same rows
  route    mq_batch_route over 2^20 x 1200-B datagrams: all hits over 4096 connections (with
           mq_batch_recv over the same batch), all hits over 2^20 connections (a 64-MiB table), and an
           Initial flood of 2^20 distinct new DCIDs with max_new = 2^20 (with mq_batch_derive_initial
           over what it admitted); 4096 datagrams of each run checked against tests/route_model.py
  frames   mq_batch_frames over 2^20 opened packets (its own mode only): the recv mode's 1200-B 1-RTT
           batch with frame streams of an ACK, three control frames and a STREAM frame to the end, behind
           mq_batch_recv of the same run, and an Initial-shaped plaintext batch (a 300-B CRYPTO frame, the
           rest PADDING); 4096 packets of each checked against tests/frames_model.py
  acks     mq_batch_acks (track + build) over 2^20 opened packets (its own mode only): the frames mode's
           1-RTT batch behind mq_batch_recv and mq_batch_frames of the same run, over 4096, 64 and 1
           connections in order and over 4096 connections with loss and reordering (gaps of 2..300 with
           p = 0.02, ~40000 with p = 0.001, adjacent packets swapped with p = 0.01); every timed call
           starts from empty trackers; a sample of connections checked against tests/acks_model.py
  streamdata  mq_batch_stream_data and mq_batch_stream_read (its own mode only) over 2^20 plaintext packets
           of 1200 B with one 1150-B STREAM frame each, in order on 32 streams per connection, over 4096 and
           64 connections: the whole call from empty stream tables, the payload rate (bytes read + written)
           beside a device-to-device copy of the same bytes, then one read request per buffer; a sample of
           buffers compared with the arena's bytes
  recovery  mq_batch_sent and mq_batch_recovery (its own mode only) over 2^20 packets and 4096 connections: 256
           sends per connection into fresh rows, then one ACK frame of one packet number per packet, in order;
           every timed call starts from the same rows; counts, windows, RTT and events checked on the host
Usage: python tools/bench_aux.py [reps] | rekey [reps] | recv reps conns... | route [reps] | frames [reps] | acks [reps [batch]] | streamdata [reps [batch]] | recovery [reps]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from milli_quic_amd import _lib, batch, recv, send, tls_record, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402

DEV = torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def timed_all(fn, reps):
    """One warm-up call, then `reps` timed ones: (median, min, max) in ms."""
    out = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out[1:])), float(min(out[1:])), float(max(out[1:]))


def timed(fn, reps):
    return timed_all(fn, reps)[0]


def bench_derive(reps, n=1 << 20):
    kt = KeyTable([_lib.KeyMaterial() for _ in range(2 * n)])
    dc = t(workload.splitmix_bytes(20 * n, seed=9))
    ln = torch.full((n,), 8, dtype=torch.uint8, device=DEV)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ms = timed(lambda: batch.derive_initial(kt, 0, dc, ln, st), reps)
    assert int((st != 0).sum()) == 0
    return {"connections": n, "ms": round(ms, 4), "connections_per_s": round(n / ms * 1e3)}


def bench_protect_recv(reps, n=1 << 20, n_conns=4096, only="both"):
    fl = 1171
    w = workload.uniform(64, _lib.MQ_SUITE_CHACHA20, n_keys=n_conns)
    kt = KeyTable(w.keys)
    conns = send.make_conns([workload.DCID8] * n_conns, [b""] * n_conns, [[k, k, k] for k in range(n_conns)])
    req = np.zeros(n, dtype=send.REQ_DTYPE)
    i = np.arange(n, dtype=np.uint64)
    req["frames_offset"], req["out_offset"] = i * np.uint64(fl), i * np.uint64(1200)
    req["pn"] = np.uint64(0x10000000) + i // np.uint64(n_conns)
    req["largest_acked"] = req["pn"] - np.uint64(1 << 24)
    req["frame_len"], req["out_cap"], req["level"] = fl, 1200, send.APPLICATION
    req["conn"] = (i % np.uint64(n_conns)).astype(np.uint32)
    frames = t(workload.splitmix_bytes(n * fl, seed=3))
    out = torch.zeros(n * 1200, dtype=torch.uint8, device=DEV)
    dc, dr = t(conns), t(req)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    ms_p = timed(lambda: send.protect(kt, dc, frames, out, dr, st, ln, _lib.MQ_SUITE_CHACHA20, ws),
                 reps if only != "recv" else 0)
    assert int((st != 0).sum()) == 0
    if only == "protect":
        return ({"ms": round(ms_p, 4)}, None)
    sealed = out.clone()
    rc = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
    rc["app_row"][:, 1] = np.arange(n_conns)
    rc["dcid_len"], rc["flags"] = 8, recv.HAS_APP
    dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
    dg["offset"], dg["len"], dg["conn"] = i * np.uint64(1200), 1200, req["conn"]
    dgt = t(dg)
    pk = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    rws = torch.empty(recv.workspace_bytes(n, n, n_conns), dtype=torch.uint8, device=DEV)
    ct0 = t(rc)
    ct = ct0.clone()

    def one_recv():
        out.copy_(sealed)
        ct.copy_(ct0)
        recv.recv(kt, ct, out, dgt, pk, cnt, rws)
    copy_ms = timed(lambda: (out.copy_(sealed), ct.copy_(ct0)), reps)
    ms_r = timed(one_recv, reps) - copy_ms
    got = pk.cpu().numpy().view(recv.PKT_DTYPE)
    assert int(cnt[0]) == n and (got["status"] == 0).all()
    checked = sample_check(kt_rows=w.keys, rc=rc, sealed=sealed, opened=out, got=got, dg=dg)
    wire = n * 1200
    return ({"packets": n, "connections": n_conns, "ms": round(ms_p, 4),
             "GiB_per_s_wire": round(wire / ms_p * 1e3 / 2 ** 30, 1)},
            {"packets": n, "connections": n_conns, "ms": round(ms_r, 4),
             "GiB_per_s_wire": round(wire / ms_r * 1e3 / 2 ** 30, 1), "sample_checked": checked})


def sample_check(kt_rows, rc, sealed, opened, got, dg, k=4096, seed=12):
    """Byte check of a sample of the receive run: the oracle's receive composite
    (the checker) on k sampled datagrams, from the sealed bytes, must give the same records and
    the same opened bytes as the GPU's full run. The PNs are 4-byte encoded, so a sampled packet
    decodes the same without its connection's earlier packets."""
    from oracle import oracle
    oracle.load()
    rng = np.random.default_rng(seed)
    n = len(dg)
    idx = np.sort(rng.choice(n, size=min(k, n), replace=False))
    sd = dg[idx].copy()
    L = int(dg["len"][0])
    arena = np.zeros(len(idx) * L, dtype=np.uint8)
    sealed_np = sealed.cpu().numpy()
    opened_np = opened.cpu().numpy()
    for j, g in enumerate(idx):
        o = int(dg["offset"][g])
        arena[j * L:(j + 1) * L] = sealed_np[o:o + L]
    sd["offset"] = np.arange(len(idx), dtype=np.uint64) * np.uint64(L)
    o_pk, o_n = oracle.batch_recv(kt_rows, rc.copy(), arena, sd, len(idx), threads=16)
    assert o_n == len(idx) and (o_pk["status"] == 0).all(), "oracle sample failed"
    gp = got[idx]  # one packet per datagram: record index = datagram index
    assert (gp["pn"] == o_pk["pn"]).all() and (gp["status"] == o_pk["status"]).all()
    for j, g in enumerate(idx):
        o = int(dg["offset"][g])
        assert opened_np[o:o + L].tobytes() == arena[j * L:(j + 1) * L].tobytes(), f"datagram {g} differs"
    return len(idx)


def bench_records(reps, n, L):
    km = workload.key_material(_lib.MQ_SUITE_AES128GCM, workload.A1_SERVER_SECRET)
    kt = KeyTable([km])
    i = np.arange(n, dtype=np.uint64)
    a = t(workload.splitmix_bytes(n * L, seed=4))
    sd = t(tls_record.record_descs(i * np.uint64(L), L, 0, i, 23))
    od = t(tls_record.record_descs(i * np.uint64(L), L, 0, i))
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    info = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.empty(max(batch.workspace_bytes(n), 256), dtype=torch.uint8, device=DEV)
    ms_s = timed(lambda: batch.seal_records(kt, a, sd, st, _lib.MQ_SUITE_AES128GCM, ws), reps)
    assert int((st != 0).sum()) == 0
    ms_o = timed(lambda: (batch.seal_records(kt, a, sd, st, _lib.MQ_SUITE_AES128GCM, ws),
                          batch.open_records(kt, a, od, st, info, _lib.MQ_SUITE_AES128GCM, ws)), reps) - ms_s
    assert int((st != 0).sum()) == 0
    wire = n * L
    return {"records": n, "record_bytes": L, "seal_ms": round(ms_s, 4), "open_ms": round(ms_o, 4),
            "GiB_per_s_seal_open": round(2 * wire / (ms_s + ms_o) * 1e3 / 2 ** 30, 1)}


def bench_hp_mask(reps, suite, n=1 << 20):
    secret = workload.A1_SERVER_SECRET if suite == _lib.MQ_SUITE_AES128GCM else workload.A5_SECRET
    km = workload.key_material(suite, secret)
    kt = KeyTable([km])
    smp = workload.splitmix_bytes(16 * n, seed=11)
    s_d = t(smp)
    kid = torch.zeros(n, dtype=torch.int32, device=DEV)
    masks = torch.zeros(5 * n, dtype=torch.uint8, device=DEV)
    ms = timed(lambda: batch.hp_mask(kt, kid, s_d, masks), reps)  # parity: tests/test_gpu_parity.py
    return {"samples": n, "ms": round(ms, 4), "masks_per_s": round(n / ms * 1e3)}


def bench_rekey(reps, suite, n=1 << 20, n_host=1 << 14, k=4096):
    """derive_keys and key_update (dst == src) over n rows of one suite; a k-row sample of km_out
    byte-checked against the host functions; the host path for the first n_host of the same rows:
    mq_derive_key_material (mq_derive_key_update) per row through ctypes plus one mq_keytable_update."""
    import ctypes
    import time
    from milli_quic_amd import key_schedule
    lib = _lib.load()
    KM = ctypes.sizeof(_lib.KeyMaterial)
    kt = KeyTable([_lib.KeyMaterial() for _ in range(n)])
    sec = workload.splitmix_bytes(32 * n, seed=13).reshape(n, 32)
    s_d, st = t(sec), torch.zeros(n, dtype=torch.uint8, device=DEV)
    km = torch.zeros(KM * n, dtype=torch.uint8, device=DEV)
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    ms_d = timed(lambda: batch.derive_keys(kt, suite, s_d, st, km_out=km), reps)
    assert int((st != 0).sum()) == 0
    km0 = km.cpu().numpy().reshape(n, KM)
    pick = np.random.default_rng(12).choice(n, size=k, replace=False)
    host0 = {int(i): key_schedule.key_material(suite, sec[i].tobytes()) for i in pick}
    assert all(km0[i].tobytes() == bytes(host0[i]) for i in host0)
    s_u = s_d.clone()
    batch.key_update(kt, s_u, rows, rows, st, km_out=km)  # generation 1 of every row, then the timed ones
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    km1, s1 = km.cpu().numpy().reshape(n, KM), s_u.cpu().numpy().reshape(n, 32)
    for i in host0:
        nxt, want = key_schedule.derive_key_update(sec[i].tobytes(), host0[i])
        assert s1[i].tobytes() == nxt and km1[i].tobytes() == bytes(want)
    ms_u = timed(lambda: batch.key_update(kt, s_u, rows, rows, st, km_out=km), reps)
    assert int((st != 0).sum()) == 0
    # host path: HKDF per row on one thread, then the synchronous row upload
    arr = (_lib.KeyMaterial * n_host)()
    blobs = [sec[i].tobytes() for i in range(n_host)]
    t0 = time.perf_counter()
    for i in range(n_host):
        lib.mq_derive_key_material(suite, blobs[i], 32, ctypes.byref(arr[i]))
    assert lib.mq_keytable_update(kt.handle, 0, arr, n_host) == 0
    h_d = time.perf_counter() - t0
    bufs = [(ctypes.c_uint8 * 32).from_buffer_copy(b) for b in blobs]
    t0 = time.perf_counter()
    for i in range(n_host):
        lib.mq_derive_key_update(bufs[i], ctypes.byref(arr[i]), ctypes.byref(arr[i]))
    assert lib.mq_keytable_update(kt.handle, 0, arr, n_host) == 0
    h_u = time.perf_counter() - t0
    assert bytes(arr[int(pick[0]) % n_host]) == km1[int(pick[0]) % n_host].tobytes()
    out = {"rows": n, "sample_checked": k, "host_rows": n_host,
           "derive_keys_ms": round(ms_d, 4), "derive_keys_rows_per_s": round(n / ms_d * 1e3),
           "key_update_ms": round(ms_u, 4), "key_update_rows_per_s": round(n / ms_u * 1e3),
           "host_derive_rows_per_s": round(n_host / h_d), "host_key_update_rows_per_s": round(n_host / h_u)}
    out["derive_keys_vs_host"] = round(out["derive_keys_rows_per_s"] / out["host_derive_rows_per_s"], 1)
    out["key_update_vs_host"] = round(out["key_update_rows_per_s"] / out["host_key_update_rows_per_s"], 1)
    return out


def route_sample_check(table_cids, table_conns, arena, dg, st, conn, sdl, idx, admit=None):
    """Datagrams idx of a timed route run against the Python model (tests/route_model.py), which gets
    their bytes and the table entries they can hit."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import route_model
    L = int(dg["len"][0])
    model = route_model.TableModel(1 << 30)
    model.map = dict(zip(table_cids, table_conns))
    rows = arena.view(-1, L)[torch.from_numpy(idx.astype(np.int64)).to(DEV)].cpu().numpy()
    sub = np.zeros(len(idx), dtype=recv.DGRAM_DTYPE)
    sub["offset"], sub["len"] = np.arange(len(idx), dtype=np.uint64) * np.uint64(L), L
    adm = None
    if admit is not None:
        adm = route_model.AdmitModel(np.zeros(len(idx), dtype=recv.CONN_DTYPE), 0, len(idx), admit, L)
    want_st, want_conn = model.route(rows.reshape(-1), sub, sdl, adm)
    got_st, got_conn = st.cpu().numpy()[idx], conn[idx]
    assert (got_st == want_st).all() and (got_conn == want_conn).all(), "route sample differs from the model"
    return len(idx)


def bench_route(reps, n=1 << 20, L=1200, k=4096):
    from milli_quic_amd import route
    seed = bytes(range(16))
    res = {}
    i = np.arange(n, dtype=np.uint64)
    pick = np.sort(np.random.default_rng(12).choice(n, size=k, replace=False))

    def dgrams(conn_fill):
        dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
        dg["offset"], dg["len"], dg["conn"] = i * np.uint64(L), L, conn_fill
        return dg

    def fill(table, cids8, n_conns):
        c20 = np.zeros((n_conns, 20), dtype=np.uint8)
        c20[:, :8] = cids8
        st = torch.full((n_conns,), 0xEE, dtype=torch.uint8, device=DEV)
        table.insert(t(c20), torch.full((n_conns,), 8, dtype=torch.uint8, device=DEV),
                     torch.arange(n_conns, dtype=torch.int32, device=DEV), st)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        assert table.stats()[0] == n_conns

    # ---- all hits over 4096 connections: real 1-RTT packets, so that mq_batch_recv runs on what
    # ---- the route call filled in
    n_conns, fl = 4096, 1171
    w = workload.uniform(64, _lib.MQ_SUITE_CHACHA20, n_keys=n_conns)
    kt = KeyTable(w.keys)
    cids = workload.splitmix_bytes(8 * n_conns, seed=21).reshape(n_conns, 8)
    conns = send.make_conns([c.tobytes() for c in cids], [b""] * n_conns, [[c, c, c] for c in range(n_conns)])
    req = np.zeros(n, dtype=send.REQ_DTYPE)
    req["frames_offset"], req["out_offset"] = i * np.uint64(fl), i * np.uint64(L)
    req["pn"] = np.uint64(0x10000000) + i // np.uint64(n_conns)
    req["largest_acked"] = req["pn"] - np.uint64(1 << 24)
    req["frame_len"], req["out_cap"], req["level"] = fl, L, send.APPLICATION
    req["conn"] = (i % np.uint64(n_conns)).astype(np.uint32)
    frames = t(workload.splitmix_bytes(n * fl, seed=3))
    out = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    send.protect(kt, t(conns), frames, out, t(req), st, ln, _lib.MQ_SUITE_CHACHA20, ws)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    del frames, ws
    sealed = out.clone()
    table = route.CidTable(n_conns, seed)
    fill(table, cids, n_conns)
    dgt = t(dgrams(0xDEAD))
    ms = timed(lambda: route.route(table, out, dgt, st, 8), reps)
    got = dgt.cpu().numpy().view(recv.DGRAM_DTYPE)["conn"]
    assert int((st != 0).sum()) == 0 and (got == req["conn"]).all()
    checked = route_sample_check([c.tobytes() for c in cids], range(n_conns), out, dgrams(0), st, got, 8, pick)
    rc = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
    rc["app_row"][:, 1] = np.arange(n_conns)
    rc["dcid_len"], rc["flags"] = 8, recv.HAS_APP
    pk = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    rws = torch.empty(recv.workspace_bytes(n, n, n_conns), dtype=torch.uint8, device=DEV)
    ct0 = t(rc)
    ct = ct0.clone()
    copy_ms = timed(lambda: (out.copy_(sealed), ct.copy_(ct0)), reps)
    ms_r = timed(lambda: (out.copy_(sealed), ct.copy_(ct0), recv.recv(kt, ct, out, dgt, pk, cnt, rws)), reps) - copy_ms
    assert int(cnt[0]) == n and (pk.cpu().numpy().view(recv.PKT_DTYPE)["status"] == 0).all()
    res["hits_4096_connections"] = {
        "datagrams": n, "connections": n_conns, "route_ms": round(ms, 4), "Mdgrams_per_s": round(n / ms / 1e3, 1),
        "recv_ms": round(ms_r, 4), "route_over_recv": round(ms / ms_r, 4), "sample_checked": checked}
    del sealed, pk, rws, kt, table

    # ---- all hits over 2^20 connections (2^21 slots of 32 B = 64 MiB), datagram i -> a random connection
    n_conns = n
    cids = workload.splitmix_bytes(8 * n_conns, seed=22).reshape(n_conns, 8)
    perm = np.random.default_rng(5).permutation(n_conns).astype(np.uint32)
    rows = out.view(n, L)
    rows[:, 0] = 0x41
    rows[:, 1:9] = t(cids[perm]).view(n, 8)
    table = route.CidTable(n_conns, seed)
    fill(table, cids, n_conns)
    dgt = t(dgrams(0xDEAD))
    ms = timed(lambda: route.route(table, out, dgt, st, 8), reps)
    got = dgt.cpu().numpy().view(recv.DGRAM_DTYPE)["conn"]
    assert int((st != 0).sum()) == 0 and (got == perm).all()
    sub = {cids[perm[j]].tobytes(): int(perm[j]) for j in pick}
    checked = route_sample_check(list(sub), list(sub.values()), out, dgrams(0), st, got, 8, pick)
    res["hits_1M_connections"] = {
        "datagrams": n, "connections": n_conns, "table_MiB": table.stats()[2] * 32 >> 20, "route_ms": round(ms, 4),
        "Mdgrams_per_s": round(n / ms / 1e3, 1), "route_over_recv_4096": round(ms / ms_r, 4), "sample_checked": checked}
    del table

    # ---- Initial flood: every datagram the first Initial of a new connection -----------------------
    hdr = np.zeros((n, 14), dtype=np.uint8)
    hdr[:, 0], hdr[:, 4], hdr[:, 5] = 0xC3, 1, 8
    hdr[:, 6:14] = cids[perm]
    rows[:, :14] = t(hdr).view(n, 14)
    d_conns = torch.zeros(n * recv.CONN_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    new_dcids = torch.zeros(20 * n, dtype=torch.uint8, device=DEV)
    new_lens = torch.zeros(n, dtype=torch.uint8, device=DEV)
    n_new = torch.zeros(1, dtype=torch.int32, device=DEV)
    admit = route.Admit(d_conns, 0, n, 0, new_dcids, new_lens, n_new)
    rws = torch.empty(route.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    times = []
    for _ in range(reps + 1):  # an empty table per run (created outside the timed span)
        table = route.CidTable(n, seed)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        route.route(table, out, dgt, st, 8, workspace=rws, admit=admit)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times[1:]))
    got = dgt.cpu().numpy().view(recv.DGRAM_DTYPE)["conn"]
    assert int(n_new[0]) == n and int((st != route.NEW).sum()) == 0 and (got == i.astype(np.uint32)).all()
    assert table.stats()[0] == n
    assert new_dcids.view(n, 20)[:, :8].cpu().numpy().tobytes() == cids[perm].tobytes()
    # a prefix is self-contained (ranks count the new DCIDs before each datagram)
    checked = route_sample_check([], [], out, dgrams(0), st, got, 8, np.arange(k), admit=0)
    kt = KeyTable([_lib.KeyMaterial() for _ in range(2 * n)])
    dst = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ms_d = timed(lambda: batch.derive_initial(kt, 0, new_dcids, new_lens, dst), reps)
    assert int((dst != 0).sum()) == 0
    res["initial_flood"] = {
        "datagrams": n, "new_connections": n, "route_ms": round(ms, 4), "Mdgrams_per_s": round(n / ms / 1e3, 1),
        "derive_initial_ms": round(ms_d, 4), "route_over_derive": round(ms / ms_d, 4), "sample_checked": checked}
    return res


def frames_sample_check(arena, pkts, summ, rec, idx, L):
    """Packets idx of a timed mq_batch_frames run against the Python model (tests/frames_model.py),
    which gets their bytes: every summary field but `first`, and every record."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import frames_model
    rows = arena.view(-1, L)[torch.from_numpy(idx.astype(np.int64)).to(DEV)].cpu().numpy()
    sub = pkts[idx].copy()
    sub["offset"] = np.arange(len(idx), dtype=np.uint64) * np.uint64(L)
    w_summ, w_rec, _ = frames_model.run(rows.reshape(-1), sub, len(idx))
    for f in ("n_frames", "err_pos", "n_padding", "status", "flags"):
        assert (summ[f][idx] == w_summ[f]).all(), f"frames sample: summary {f} differs from the model"
    got = np.concatenate([rec[int(summ["first"][g]):int(summ["first"][g]) + int(summ["n_frames"][g])] for g in idx])
    assert len(got) == len(w_rec) and (got["pkt"] == idx[w_rec["pkt"]]).all()
    for f in ("pos", "len", "type", "level", "data_pos", "data_len", "aux", "v"):
        assert (got[f] == w_rec[f]).all(), f"frames sample: record {f} differs from the model"
    return len(idx)


def bench_frames(reps, n=1 << 20, n_conns=4096, L=1200, k=4096):
    """mq_batch_frames behind mq_batch_recv over 2^20 opened packets: the `recv` mode's 1-RTT batch
    with real frame streams, and an Initial-shaped plaintext batch (a CRYPTO frame, the rest PADDING)."""
    from milli_quic_amd import frames as fr
    fl = 1171
    i = np.arange(n, dtype=np.uint64)
    pick = np.sort(np.random.default_rng(12).choice(n, size=k, replace=False))
    # ---- 1-RTT: ACK (one extra range), MAX_DATA, MAX_STREAM_DATA, PING, STREAM (OFF, no LEN) to the end
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from frames_model import build, vi
    head = (build(0x02, (0x0FFFFFF0, 250, 1, 3, 1, 2)) + build(0x10, (1 << 24,)) + build(0x11, (4, 1 << 20)) + b"\x01"
            + b"\x0c" + vi(4) + vi(1 << 31))
    fs = workload.splitmix_bytes(n * fl, seed=3).reshape(n, fl)
    fs[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    fs[:, 6] = (i & np.uint64(0xFF)).astype(np.uint8)  # the ACK delay's low byte differs per packet
    w = workload.uniform(64, _lib.MQ_SUITE_CHACHA20, n_keys=n_conns)
    kt = KeyTable(w.keys)
    conns = send.make_conns([workload.DCID8] * n_conns, [b""] * n_conns, [[c, c, c] for c in range(n_conns)])
    req = np.zeros(n, dtype=send.REQ_DTYPE)
    req["frames_offset"], req["out_offset"] = i * np.uint64(fl), i * np.uint64(L)
    req["pn"] = np.uint64(0x10000000) + i // np.uint64(n_conns)
    req["largest_acked"] = req["pn"] - np.uint64(1 << 24)
    req["frame_len"], req["out_cap"], req["level"] = fl, L, send.APPLICATION
    req["conn"] = (i % np.uint64(n_conns)).astype(np.uint32)
    fs_d = t(fs)
    del fs
    out = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    send.protect(kt, t(conns), fs_d, out, t(req), st, ln, _lib.MQ_SUITE_CHACHA20, ws)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    del fs_d, ws
    sealed = out.clone()
    rc = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
    rc["app_row"][:, 1] = np.arange(n_conns)
    rc["dcid_len"], rc["flags"] = 8, recv.HAS_APP
    dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
    dg["offset"], dg["len"], dg["conn"] = i * np.uint64(L), L, req["conn"]
    dgt = t(dg)
    pk = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    rws = torch.empty(recv.workspace_bytes(n, n, n_conns), dtype=torch.uint8, device=DEV)
    ct0 = t(rc)
    ct = ct0.clone()
    copy_ms = timed(lambda: (out.copy_(sealed), ct.copy_(ct0)), reps)
    ms_r = timed(lambda: (out.copy_(sealed), ct.copy_(ct0), recv.recv(kt, ct, out, dgt, pk, cnt, rws)), reps) - copy_ms
    assert int(cnt[0]) == n and (pk.cpu().numpy().view(recv.PKT_DTYPE)["status"] == 0).all()
    del sealed, rws
    max_frames = 5 * n
    summ = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(max_frames * 48, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    cf = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
    fws = torch.empty(fr.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    ms_f = timed(lambda: fr.scan(out, pk, cnt, summ, rec, total, fws, dgrams=dgt, conn_flags=cf), reps)
    h_summ = summ.cpu().numpy().view(fr.PKT_FRAMES_DTYPE)
    assert int(total[0]) == 5 * n and (h_summ["status"] == 0).all() and (h_summ["n_frames"] == 5).all()
    assert int((cf != 4).sum()) == 0  # every connection: an ack-eliciting 1-RTT packet
    checked = frames_sample_check(out, pk.cpu().numpy().view(recv.PKT_DTYPE), h_summ,
                                  rec.cpu().numpy().view(fr.FRAME_DTYPE), pick, L)
    res = {"one_rtt": {"packets": n, "records": 5 * n, "frames_ms": round(ms_f, 4), "recv_ms": round(ms_r, 4),
                       "frames_over_recv": round(ms_f / ms_r, 4), "Mpkts_per_s": round(n / ms_f / 1e3, 1),
                       "sample_checked": checked}}
    # ---- Initial-shaped: 22 header bytes, CRYPTO (offset 0, 300 bytes), PADDING up to the tag; plaintext, with
    # ---- fabricated packet records (the scan reads nothing else)
    po = 22
    crypto = build(0x06, (0, 300))
    rows = out.view(n, L)
    rows.zero_()
    rows[:, :po] = 0xC3
    rows[:, po:po + len(crypto)] = t(np.frombuffer(crypto, dtype=np.uint8))
    rows[:, po + len(crypto):po + len(crypto) + 300] = 0x5C
    rows[:, L - 16:] = 0xEE
    pkts = np.zeros(n, dtype=recv.PKT_DTYPE)
    pkts["offset"], pkts["len"], pkts["dgram"], pkts["payload_offset"] = i * np.uint64(L), L, i.astype(np.uint32), po
    pk.copy_(t(pkts))
    ms_i = timed(lambda: fr.scan(out, pk, cnt, summ, rec, total, fws, dgrams=dgt, conn_flags=cf), reps)
    h_summ = summ.cpu().numpy().view(fr.PKT_FRAMES_DTYPE)
    assert int(total[0]) == n and (h_summ["status"] == 0).all() and (h_summ["n_frames"] == 1).all()
    assert (h_summ["n_padding"] == L - 16 - po - len(crypto) - 300).all() and int((cf != 1).sum()) == 0
    checked = frames_sample_check(out, pkts, h_summ, rec.cpu().numpy().view(fr.FRAME_DTYPE), pick, L)
    res["initial_shaped"] = {"packets": n, "records": n, "padding_bytes_per_packet": L - 16 - po - len(crypto) - 300,
                             "frames_ms": round(ms_i, 4), "recv_ms_one_rtt": round(ms_r, 4),
                             "frames_over_recv": round(ms_i / ms_r, 4), "Mpkts_per_s": round(n / ms_i / 1e3, 1),
                             "sample_checked": checked}
    return res


def acks_pns(n, n_conns, lossy, seed=7):
    """Packet i belongs to connection i % n_conns and is its (i // n_conns)-th arrival. In order: PNs
    step by 1. Lossy: gaps of 2..300 (p = 0.02) and of ~40000 (p = 0.001), adjacent arrivals swapped
    (p = 0.01), per connection."""
    per = n // n_conns
    if not lossy:
        return (np.uint64(0x10000000) + np.arange(n, dtype=np.uint64) // np.uint64(n_conns))
    rng = np.random.default_rng(seed)
    inc = np.ones((n_conns, per), dtype=np.int64)
    u = rng.random((n_conns, per))
    inc[u < 0.02] = rng.integers(2, 300, size=int((u < 0.02).sum()))
    inc[u < 0.001] = 40000 + rng.integers(0, 1000, size=int((u < 0.001).sum()))
    pns = np.cumsum(inc, axis=1) + 0x10000000
    swap = np.nonzero(rng.random((n_conns, per // 2)) < 0.02)   # pairs (2k, 2k + 1): 0.01 per packet
    a, b = pns[swap[0], 2 * swap[1]].copy(), pns[swap[0], 2 * swap[1] + 1].copy()
    pns[swap[0], 2 * swap[1]], pns[swap[0], 2 * swap[1] + 1] = b, a
    return np.ascontiguousarray(pns.T).reshape(-1).astype(np.uint64)


def bench_acks(reps, n=1 << 20, L=1200, k=12, only=None):
    """recv -> frames -> acks over 2^20 1-RTT packets, each step timed on the same batch; `only` names the
    one batch to run (profiler runs)."""
    from milli_quic_amd import acks as ak, frames as fr
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import acks_model as am
    from frames_model import build, vi
    fl = 1171
    i = np.arange(n, dtype=np.uint64)
    head = (build(0x02, (0x0FFFFFF0, 250, 1, 3, 1, 2)) + build(0x10, (1 << 24,)) + build(0x11, (4, 1 << 20)) + b"\x01"
            + b"\x0c" + vi(4) + vi(1 << 31))
    fs = workload.splitmix_bytes(n * fl, seed=3).reshape(n, fl)
    fs[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    fs_d = t(fs)
    del fs
    out = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    sealed = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    res = {}
    for name, n_conns, lossy in (("in_order_4096", 4096, False), ("in_order_64", 64, False), ("in_order_1", 1, False),
                                 ("lossy_4096", 4096, True)):
        if only is not None and name != only:
            continue
        w = workload.uniform(64, _lib.MQ_SUITE_CHACHA20, n_keys=n_conns)
        kt = KeyTable(w.keys)
        conns = send.make_conns([workload.DCID8] * n_conns, [b""] * n_conns, [[c, c, c] for c in range(n_conns)])
        pns = acks_pns(n, n_conns, lossy)
        req = np.zeros(n, dtype=send.REQ_DTYPE)
        req["frames_offset"], req["out_offset"] = i * np.uint64(fl), i * np.uint64(L)
        req["pn"] = pns
        req["largest_acked"] = pns - np.uint64(1 << 24)
        req["frame_len"], req["out_cap"], req["level"] = fl, L, send.APPLICATION
        req["conn"] = (i % np.uint64(n_conns)).astype(np.uint32)
        st = torch.zeros(n, dtype=torch.uint8, device=DEV)
        ln = torch.zeros(n, dtype=torch.int32, device=DEV)
        ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
        send.protect(kt, t(conns), fs_d, out, t(req), st, ln, _lib.MQ_SUITE_CHACHA20, ws)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        del ws
        sealed.copy_(out)
        rc = np.zeros(n_conns, dtype=recv.CONN_DTYPE)
        rc["app_row"][:, 1] = np.arange(n_conns)
        rc["dcid_len"], rc["flags"] = 8, recv.HAS_APP
        dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
        dg["offset"], dg["len"], dg["conn"] = i * np.uint64(L), L, req["conn"]
        dgt = t(dg)
        pk = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        rws = torch.empty(recv.workspace_bytes(n, n, n_conns), dtype=torch.uint8, device=DEV)
        ct0 = t(rc)
        ct = ct0.clone()
        copy_ms = timed(lambda: (out.copy_(sealed), ct.copy_(ct0)), reps)
        r_ms = [x - copy_ms for x in timed_all(lambda: (out.copy_(sealed), ct.copy_(ct0),
                                                       recv.recv(kt, ct, out, dgt, pk, cnt, rws)), reps)]
        h_pk = pk.cpu().numpy().view(recv.PKT_DTYPE)
        assert int(cnt[0]) == n and (h_pk["status"] == 0).all() and (h_pk["pn"] == pns).all()
        del rws
        summ = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        rec = torch.zeros(5 * n * 48, dtype=torch.uint8, device=DEV)
        total = torch.zeros(1, dtype=torch.int32, device=DEV)
        cf = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
        fws = torch.empty(fr.workspace_bytes(n), dtype=torch.uint8, device=DEV)
        f_ms = timed_all(lambda: fr.scan(out, pk, cnt, summ, rec, total, fws, dgrams=dgt, conn_flags=cf), reps)
        assert int(total[0]) == 5 * n and int((cf != 4).sum()) == 0
        del rec, fws
        trk = torch.zeros(3 * n_conns * 528, dtype=torch.uint8, device=DEV)
        pend = torch.zeros(n_conns, dtype=torch.int32, device=DEV)
        nx0 = t(np.arange(3 * n_conns, dtype=np.uint64) + np.uint64(100))
        nx = nx0.clone()
        max_acks = n_conns + 8
        frs = torch.zeros(max_acks * ak.FRAME_MAX, dtype=torch.uint8, device=DEV)
        rq = torch.zeros(max_acks * 48, dtype=torch.uint8, device=DEV)
        na = torch.zeros(1, dtype=torch.int32, device=DEV)
        aws = torch.empty(ak.workspace_bytes(n, n_conns), dtype=torch.uint8, device=DEV)
        b = ak.Build(frs, rq, na, ct, nx, 96)
        reset_ms = timed(lambda: (trk.zero_(), pend.zero_(), nx.copy_(nx0)), reps)
        a_ms = [x - reset_ms for x in timed_all(lambda: (trk.zero_(), pend.zero_(), nx.copy_(nx0),
                                                         ak.track_and_build(pk, cnt, dgt, trk, pend, aws, summary=summ,
                                                                            conn_flags=cf, build=b)), reps)]
        # the last timed call against the model, on a sample of connections
        h_trk = trk.cpu().numpy().view(ak.TRACKER_DTYPE)
        h_rq, h_fr = rq.cpu().numpy().view(send.REQ_DTYPE), frs.cpu().numpy().reshape(max_acks, ak.FRAME_MAX)
        assert int(na[0]) == n_conns and int((pend != 0).sum()) == 0
        assert (h_rq["conn"][:n_conns] == np.arange(n_conns)).all() and (h_rq["conn"][n_conns:] == 0xFFFFFFFF).all()
        per = pns.reshape(-1, n_conns)
        for c in sorted(set(int(x) for x in np.random.default_rng(12).choice(n_conns, size=min(k, n_conns), replace=False))):
            m = am.Tracker()
            for pn in per[:, c].tolist():
                m.record(pn)
            assert am.load_tracker(h_trk[3 * c + 2]).ranges == m.ranges, f"acks sample: tracker of connection {c}"
            f = am.build_ack_frame(m.ranges)
            assert h_fr[c, :len(f)].tobytes() == f and h_rq["frame_len"][c] == len(f) and h_rq["pn"][c] == 100 + 3 * c + 2
        rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
        res[name] = {"packets": n, "connections": n_conns, "acks_built": n_conns,
                     "ranges_per_tracker_mean": round(float(h_trk["n"][2::3].mean()), 2),
                     "acks_ms_median_min_max": rnd(a_ms), "frames_ms_median_min_max": rnd(f_ms),
                     "recv_ms_median_min_max": rnd(r_ms), "acks_over_frames": round(a_ms[0] / f_ms[0], 4),
                     "acks_over_recv": round(a_ms[0] / r_ms[0], 4), "sample_checked": min(k, n_conns), "reps": reps}
        del summ, trk, aws, pk, dgt
    return res


def bench_streamdata(reps, n=1 << 20, L=1200, k=12, only=None):
    """mq_batch_stream_data over crafted packet and frame records (the call reads nothing else), then
    mq_batch_stream_read of every buffer; `only` names the one batch to run (profiler runs)."""
    from milli_quic_amd import frames as fr, stream_data as sd
    po, dp, dl = 30, 7, 1150                 # payload offset, the frame's data position and length
    i = np.arange(n, dtype=np.uint64)
    arena_h = workload.splitmix_bytes(n * L, seed=5)
    arena = t(arena_h)
    res = {}
    for name, n_conns in (("in_order_4096", 4096), ("in_order_64", 64)):
        if only is not None and name != only:
            continue
        per = n // (n_conns * sd.SLOTS)       # frames per stream
        stream_buf = (per * dl + 15) // 16 * 16
        conn = (i % np.uint64(n_conns)).astype(np.uint32)
        slot = ((i // np.uint64(n_conns)) % np.uint64(sd.SLOTS))
        nth = i // np.uint64(n_conns * sd.SLOTS)
        pk = np.zeros(n, dtype=recv.PKT_DTYPE)
        pk["offset"], pk["len"], pk["dgram"], pk["payload_offset"], pk["level"], pk["pn"] = i * np.uint64(L), L, conn, po, 2, i
        dg = np.zeros(n_conns, dtype=recv.DGRAM_DTYPE)
        dg["len"], dg["conn"] = L, np.arange(n_conns)
        f = np.zeros(n, dtype=fr.FRAME_DTYPE)
        f["pkt"], f["len"], f["type"], f["level"], f["data_pos"], f["data_len"] = i, dp + dl, 0x0e, 2, dp, dl
        f["v"][:, 0], f["v"][:, 1] = slot * np.uint64(4) + np.uint64(1), nth * np.uint64(dl)
        pk_d, dg_d, f_d = t(pk), t(dg), t(f)
        cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
        st = torch.zeros(n_conns * sd.CONN_STREAMS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        bufs = torch.zeros(n_conns * sd.SLOTS * stream_buf, dtype=torch.uint8, device=DEV)
        ev = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
        n_ev = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.empty(sd.workspace_bytes(n, n_conns), dtype=torch.uint8, device=DEV)
        reset_ms = timed(lambda: st.zero_(), reps)
        d_ms = [x - reset_ms for x in timed_all(lambda: (st.zero_(), sd.deliver(
            arena, pk_d, cnt, dg_d, f_d, cnt, st, bufs, stream_buf, 1 << 40, ev, n_ev, ws, flags=sd.CLIENT)), reps)]
        h_ev = ev.cpu().numpy().view(sd.EVT_DTYPE)
        assert int(n_ev[0]) == n and (h_ev["store"] == sd.STORE_COPIED).all() and (h_ev["copy_len"] == dl).all()
        assert (h_ev["mark"] == 0).all() and (h_ev["buf_slot"] == slot).all()
        rng = np.random.default_rng(12)
        for c, s_ in zip(rng.integers(0, n_conns, k), rng.integers(0, sd.SLOTS, k)):
            at = (int(c) * sd.SLOTS + int(s_)) * stream_buf
            got = bufs[at:at + per * dl].cpu().numpy()
            first = int(s_) * n_conns + int(c)
            rows = arena_h.reshape(n, L)[first::n_conns * sd.SLOTS, po + dp:po + dp + dl]
            assert got.tobytes() == rows.tobytes(), f"streamdata sample: buffer {s_} of connection {c}"
        moved = 2.0 * n * dl
        side = torch.empty(n * dl, dtype=torch.uint8, device=DEV)
        c_ms = timed_all(lambda: side.copy_(arena[:n * dl]), reps)
        # read every buffer whole
        n_reqs = n_conns * sd.SLOTS
        q = np.zeros(n_reqs, dtype=sd.READ_REQ_DTYPE)
        j = np.arange(n_reqs, dtype=np.uint64)
        q["conn"], q["stream_id"] = j // np.uint64(sd.SLOTS), (j % np.uint64(sd.SLOTS)) * np.uint64(4) + np.uint64(1)
        q["cap"], q["out_offset"] = per * dl, j * np.uint64(per * dl)
        q_d = t(q)
        rs = torch.zeros(n_reqs * 8, dtype=torch.uint8, device=DEV)
        rws = torch.empty(sd.read_workspace_bytes(n_reqs, n_conns), dtype=torch.uint8, device=DEV)
        st0 = st.clone()
        copy_ms = timed(lambda: st.copy_(st0), reps)
        r_ms = [x - copy_ms for x in timed_all(lambda: (st.copy_(st0), sd.read(st, bufs, stream_buf, q_d, side, rs, rws)),
                                               reps)]
        h_rs = rs.cpu().numpy().view(sd.READ_RES_DTYPE)
        assert (h_rs["status"] == 0).all() and (h_rs["copied"] == per * dl).all()
        rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
        res[name] = {"packets": n, "connections": n_conns, "frames_per_stream": per, "stream_buf": stream_buf,
                     "deliver_ms_median_min_max": rnd(d_ms), "deliver_payload_GBps": round(moved / d_ms[0] / 1e6, 1),
                     "copy_ms_median_min_max": rnd(c_ms), "copy_GBps": round(moved / c_ms[0] / 1e6, 1),
                     "read_ms_median_min_max": rnd(r_ms), "read_GBps": round(moved / r_ms[0] / 1e6, 1),
                     "sample_checked": k, "reps": reps}
        del bufs, side, ws, ev
    return res


def bench_recovery(reps, n=1 << 20, n_conns=4096, L=1200):
    """mq_batch_sent and mq_batch_recovery over crafted request, packet and frame records (the calls read nothing
    else): packet i belongs to connection i % n_conns and is its (i // n_conns)-th, one ACK frame of one packet
    number per packet, in order. Each connection sends 256 packets, of which its 128-slot tracker keeps 128 (the rest
    are the reference's silently dropped sends, still counted in flight), and receives 256 ACKs, 128 of which find
    their packet."""
    from milli_quic_amd import frames as fr, recovery as rcv
    i = np.arange(n, dtype=np.uint64)
    conn = (i % np.uint64(n_conns)).astype(np.uint32)
    nth = i // np.uint64(n_conns)
    per = n // n_conns
    rq = np.zeros(n, dtype=send.REQ_DTYPE)
    rq["conn"], rq["level"], rq["pn"] = conn, 2, nth
    st_d, ln_d = t(np.zeros(n, dtype=np.uint8)), t(np.full(n, L, dtype=np.uint32))
    rq_d, now_d = t(rq), t(np.uint64(1000) + nth * np.uint64(50))
    pk = np.zeros(n, dtype=recv.PKT_DTYPE)
    pk["offset"], pk["len"], pk["dgram"], pk["payload_offset"], pk["level"], pk["pn"] = i * np.uint64(64), 64, i, 30, 2, nth
    dg = np.zeros(n, dtype=recv.DGRAM_DTYPE)
    dg["offset"], dg["len"], dg["conn"] = i * np.uint64(64), 64, conn
    f = np.zeros(n, dtype=fr.FRAME_DTYPE)
    f["pkt"], f["len"], f["type"], f["level"], f["data_pos"] = i, 5, 0x02, 2, 5
    f["v"][:, 0], f["v"][:, 1] = nth % np.uint64(rcv.SLOTS), 100
    pk_d, dg_d, f_d = t(pk), t(dg), t(f)
    dnow_d = t(np.uint64(40_000) + nth * np.uint64(50))
    arena = torch.zeros(n * 64, dtype=torch.uint8, device=DEV)
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    rows0 = t(rcv.state_rows(n_conns, 25_000, L))
    rows = rows0.clone()
    ev = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    lost = torch.zeros(4096 * 16, dtype=torch.uint8, device=DEV)
    n_ev, n_lo = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    to = torch.zeros(n_conns, dtype=torch.int64, device=DEV)
    ws_s = torch.empty(rcv.sent_workspace_bytes(n, n_conns), dtype=torch.uint8, device=DEV)
    ws_r = torch.empty(rcv.workspace_bytes(n, n_conns), dtype=torch.uint8, device=DEV)
    copy_ms = timed(lambda: rows.copy_(rows0), reps)
    s_ms = [x - copy_ms for x in timed_all(lambda: (rows.copy_(rows0), rcv.sent(rq_d, st_d, ln_d, now_d, rows, ws_s, timeouts=to)), reps)]
    sent_rows = rows.clone()
    h = sent_rows.cpu().numpy().view(rcv.CONN_RECOVERY_DTYPE)
    assert (h["count"] == rcv.SLOTS).all() and (h["bytes_in_flight"] == per * L).all()
    assert (h["sent"]["pn"] == np.arange(rcv.SLOTS)).all() and (h["time_of_last_ack_eliciting"][:, 2] == 1000 + (per - 1) * 50).all()
    r_ms = [x - copy_ms for x in timed_all(lambda: (rows.copy_(sent_rows), rcv.process(
        arena, pk_d, cnt, dg_d, dnow_d, f_d, cnt, rows, ev, n_ev, lost, n_lo, ws_r, timeouts=to)), reps)]
    h = rows.cpu().numpy().view(rcv.CONN_RECOVERY_DTYPE)
    h_ev = ev.cpu().numpy().view(rcv.EVT_DTYPE)
    assert int(n_ev[0]) == n and int(n_lo[0]) == 0 and (h["count"] == 0).all() and not h["sent"]["flags"].any()
    assert (h["bytes_in_flight"] == (per - rcv.SLOTS) * L).all() and (h["cwnd"] == max(10 * L, 14720) + rcv.SLOTS * L).all()
    assert (h_ev["n_acked"] == (nth < rcv.SLOTS)).all() and (h_ev["frame"] == i).all() and (h["smoothed_rtt"] == 39_000).all()
    rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
    return {"packets": n, "connections": n_conns, "sends_per_connection": per, "acks_per_connection": per,
            "sent_ms_median_min_max": rnd(s_ms), "sent_Mpkts_per_s": round(n / s_ms[0] / 1e3, 1),
            "recovery_ms_median_min_max": rnd(r_ms), "recovery_Macks_per_s": round(n / r_ms[0] / 1e3, 1), "reps": reps}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "recovery":  # loss recovery runs only: recovery [REPS]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
        print(json.dumps({"device": torch.cuda.get_device_name(0), "recovery": bench_recovery(reps)}), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "streamdata":  # stream data runs only: streamdata [REPS [BATCH]]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
        only = sys.argv[3] if len(sys.argv) > 3 else None
        print(json.dumps({"device": torch.cuda.get_device_name(0), "streamdata": bench_streamdata(reps, only=only)}),
              flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "acks":  # ACK runs only: acks [REPS [BATCH]]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
        only = sys.argv[3] if len(sys.argv) > 3 else None
        print(json.dumps({"device": torch.cuda.get_device_name(0), "acks": bench_acks(reps, only=only)}), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "frames":  # frame index runs only: frames [REPS]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        print(json.dumps({"device": torch.cuda.get_device_name(0), "frames": bench_frames(reps)}), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "route":  # routing runs only: route [REPS]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        print(json.dumps({"device": torch.cuda.get_device_name(0), "route": bench_route(reps)}), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "rekey":  # key derivation / update runs only: rekey [REPS]
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        res = {"device": torch.cuda.get_device_name(0),
               "rekey_aes": bench_rekey(reps, _lib.MQ_SUITE_AES128GCM),
               "rekey_chacha": bench_rekey(reps, _lib.MQ_SUITE_CHACHA20)}
        print(json.dumps(res), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "recv":  # receive runs only: recv REPS CONNS...
        assert _lib.load().mq_device_init(0) == 0
        reps = int(sys.argv[2])
        res = {f"recv_{nc}_connections": bench_protect_recv(reps, n_conns=nc, only="recv")[1]
               for nc in map(int, sys.argv[3:])}
        print(json.dumps(res), flush=True)
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    assert _lib.load().mq_device_init(0) == 0
    res = {"device": torch.cuda.get_device_name(0), "derive": bench_derive(reps)}
    res["protect"], res["recv"] = bench_protect_recv(reps)
    # the receive walk over few connections (r05: runs cut into segments of kSeg packets per wave)
    for nc in (1024, 64, 4, 1):
        res[f"recv_{nc}_connections"] = bench_protect_recv(reps, n_conns=nc, only="recv")[1]
    res["records_1200"] = bench_records(reps, 1 << 20, 1200)
    res["records_16k"] = bench_records(reps, 1 << 16, 16384 + 5 + 17)
    res["hp_mask_aes"] = bench_hp_mask(reps, _lib.MQ_SUITE_AES128GCM)
    res["hp_mask_chacha"] = bench_hp_mask(reps, _lib.MQ_SUITE_CHACHA20)
    res["rekey_aes"] = bench_rekey(reps, _lib.MQ_SUITE_AES128GCM)
    res["rekey_chacha"] = bench_rekey(reps, _lib.MQ_SUITE_CHACHA20)
    res["route"] = bench_route(reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
