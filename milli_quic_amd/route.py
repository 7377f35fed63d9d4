"""Datagram routing on the GPU: a device-resident connection-ID table and mq_batch_route.

The step in front of ``recv.recv``: every datagram's Destination Connection ID is extracted as the
reference's decode_dcid does (src/packet/decode_dcid.rs:9-37), looked up in the table, and
``dgrams[].conn`` is filled in on the device. With an ``Admit`` the call also opens the connections
of first Initial packets (src/connection/recv.rs:275-278; RFC 9000 §5.2, §14.1, §17.2) in a form
that ``batch.derive_initial`` and ``recv.recv`` take next on the same stream, with nothing read back.
All arrays are device uint8 / int32 tensors; the semantics are spelled out in include/mq_aead.h.
"""
import ctypes

from . import _lib
from .batch import _nbytes, _opt_ptr, _stream_ptr
from .crypto import InvalidArgument, _raise
from .recv import CONN_DTYPE, DGRAM_DTYPE

CONN_NONE = _lib.MQ_CONN_NONE
OK = _lib.MQ_OK
HIT, NEW, UNKNOWN, MALFORMED, FULL, DEFERRED = (_lib.MQ_ROUTE_HIT, _lib.MQ_ROUTE_NEW, _lib.MQ_ROUTE_UNKNOWN,
                                                _lib.MQ_ROUTE_MALFORMED, _lib.MQ_ROUTE_FULL, _lib.MQ_ROUTE_DEFERRED)
MAX_CID_LEN = 20


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class CidTable:
    """mq_cid_table: CIDs of 0..20 bytes -> connection rows, on the device it was created on.
    ``seed`` (16 bytes, random per process) keys the hash. Calls are stream-ordered: keep them on
    one stream."""

    def __init__(self, capacity, seed):
        seed = bytes(seed)
        if len(seed) != 16:
            raise InvalidArgument("seed must be 16 bytes")
        h = ctypes.c_void_p()
        _raise(_lib.load().mq_cid_table_create(capacity, seed, ctypes.byref(h)))
        self._h = h
        self.capacity = capacity

    @property
    def handle(self):
        return self._h

    def insert(self, cids, lens, conn, status, stream=None):
        """n entries: cids (n x 20 bytes), lens (n bytes), conn (n x uint32 / int32). status[i]: OK,
        HIT (already there, entry unchanged), FULL or MALFORMED (length over 20)."""
        n = lens.numel()
        if _nbytes(cids) < MAX_CID_LEN * n or _nbytes(conn) < 4 * n or status.numel() < n:
            raise InvalidArgument("cids needs 20 bytes, conn 4 bytes and status 1 byte per entry")
        _raise(_lib.load().mq_cid_table_insert(self._h, _ptr(cids), _ptr(lens), _ptr(conn), n, _ptr(status),
                                               _stream_ptr(stream)))

    def remove(self, cids, lens, status, stream=None):
        """status[i]: OK or UNKNOWN."""
        n = lens.numel()
        if _nbytes(cids) < MAX_CID_LEN * n or status.numel() < n:
            raise InvalidArgument("cids needs 20 bytes and status 1 byte per entry")
        _raise(_lib.load().mq_cid_table_remove(self._h, _ptr(cids), _ptr(lens), n, _ptr(status),
                                               _stream_ptr(stream)))

    def compact(self, stream=None):
        """Rehash the live entries and drop the tombstones of earlier removals."""
        _raise(_lib.load().mq_cid_table_compact(self._h, _stream_ptr(stream)))

    def stats(self, stream=None):
        """(live entries, tombstones, slots); waits for the stream."""
        live, tomb, slots = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _raise(_lib.load().mq_cid_table_stats(self._h, _stream_ptr(stream), ctypes.byref(live), ctypes.byref(tomb),
                                              ctypes.byref(slots)))
        return live.value, tomb.value, slots.value

    def debug_hash_bits(self, bits):
        """Diagnostic, empty table only: keep the low `bits` of the hash (forces collisions)."""
        _raise(_lib.load().mq_debug_cid_table_hash_bits(self._h, bits))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.load().mq_cid_table_free(h)
            self._h = None


class Admit:
    """mq_route_admit: admitted connection k (in the order of each new DCID's first datagram) gets
    row conn_base + k of ``conns`` (zeroed, initial_row = row_first + 2k, HAS_INITIAL, dcid_len),
    its DCID in new_dcids[k] / new_dcid_lens[k] and a table entry; n_new (one int32 / uint32) gets
    the count, new_dcid_lens beyond it 0xFF — what ``batch.derive_initial(kt, row_first, new_dcids,
    new_dcid_lens, ..)`` takes next (client keys in row_first + 2k, server keys in row_first + 2k + 1)."""

    def __init__(self, conns, conn_base, max_new, row_first, new_dcids, new_dcid_lens, n_new, min_initial_len=1200):
        if _nbytes(new_dcids) < MAX_CID_LEN * max_new or _nbytes(new_dcid_lens) < max_new or _nbytes(n_new) < 4:
            raise InvalidArgument("new_dcids needs 20 bytes and new_dcid_lens 1 byte per admitted connection")
        self.tensors = (conns, new_dcids, new_dcid_lens, n_new)  # kept alive with the struct
        self.c = _lib.RouteAdmit(conns=conns.data_ptr(), n_conns=conns.numel() // CONN_DTYPE.itemsize,
                                 conn_base=conn_base, max_new=max_new, row_first=row_first,
                                 min_initial_len=min_initial_len, new_dcids=new_dcids.data_ptr(),
                                 new_dcid_lens=new_dcid_lens.data_ptr(), n_new=n_new.data_ptr())


def workspace_bytes(n_dgrams):
    return _lib.load().mq_batch_route_workspace_size(n_dgrams)


def route(table, arena, dgrams, status, short_dcid_len, workspace=None, admit=None, stream=None):
    """mq_batch_route: writes dgrams[i].conn (CONN_NONE unless HIT or NEW) and status[i] for every
    datagram of the device arena. ``workspace`` (workspace_bytes(n) bytes) is needed with ``admit``."""
    n = dgrams.numel() // DGRAM_DTYPE.itemsize
    if status.numel() < n:
        raise InvalidArgument("status needs one byte per datagram")
    if admit is not None and n and (workspace is None or _nbytes(workspace) < workspace_bytes(n)):
        raise InvalidArgument(f"workspace needs {workspace_bytes(n)} bytes for {n} datagrams")
    rc = _lib.load().mq_batch_route(table.handle, _ptr(arena), arena.numel(), _ptr(dgrams), n, short_dcid_len,
                                    ctypes.byref(admit.c) if admit is not None else None, _ptr(status),
                                    _opt_ptr(workspace), _stream_ptr(stream))
    _raise(rc)
