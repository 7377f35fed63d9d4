"""Stream data on the GPU: per-stream bookkeeping and the payload gather behind the frame index.

What the reference does with a STREAM frame (Frame::Stream in dispatch_frame, reference
src/connection/recv.rs:620-644: StreamMap::get_or_create and mark_recv, src/transport/stream.rs:227-388,
then store_stream_data, src/connection/mod.rs:769-842) and with RESET_STREAM (recv.rs:661-669).
``deliver`` runs mq_batch_stream_data over the device tensors that ``recv.recv`` and ``frames.scan`` leave
behind: both counts are read on the device, so recv -> frames -> stream_data chain on one stream with
nothing read back. ``read`` is the reference's stream_recv (mod.rs:660-687) for a batch of requests. The
state that stays resident between calls is ``streams`` (``CONN_STREAMS_DTYPE``, one row per connection)
and ``bufs`` (``SLOTS * stream_buf`` bytes per connection). The semantics are spelled out in
include/mq_aead.h.
"""
import ctypes

import numpy as np

from . import _lib
from .batch import _nbytes, _stream_ptr
from .crypto import InvalidArgument, _raise
from .frames import FRAME_DTYPE
from .recv import DGRAM_DTYPE, PKT_DTYPE

SLOTS = _lib.MQ_STREAM_SLOTS
CLIENT = _lib.MQ_STREAMS_CLIENT
WOULD_BLOCK = _lib.MQ_STREAM_WOULD_BLOCK
NONE = 0xFF                                                   # map_slot / buf_slot / slot: none; mark: not run
# ENTRY_DTYPE flags and recv_state
USED, HAS_RECV, HAS_SEND, HAS_FIN = 0x01, 0x02, 0x04, 0x08
RECV, SIZE_KNOWN, DATA_RECVD, RESET_RECVD, DATA_READ, RESET_READ = range(6)
# EVT_DTYPE mark, store and flags
MARK_OK, INVALID_STATE, STREAM_STATE_ERROR, FINAL_SIZE_ERROR, FLOW_CONTROL_ERROR = range(5)
STORE_NONE, STORE_NO_BUFFER, STORE_GAP, STORE_DUPLICATE, STORE_COPIED = range(5)
NEW_STREAM, NEW_BUF, FIN_SET, TRUNCATED, READABLE, RESET = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
MAX_FRAMES, MAX_CONNS, MAX_REQS = 1 << 26, 1 << 30, 1 << 26

ENTRY_DTYPE = np.dtype([
    ("id", "<u8"), ("recv_offset", "<u8"), ("recv_max_data", "<u8"), ("recv_max_data_next", "<u8"),
    ("fin_offset", "<u8"), ("flags", "u1"), ("recv_state", "u1"), ("reserved", "u1", 6),
])
BUF_DTYPE = np.dtype([
    ("stream_id", "<u8"), ("next_offset", "<u8"), ("len", "<u4"), ("read_offset", "<u4"), ("used", "u1"),
    ("fin_received", "u1"), ("reserved", "u1", 6),
])
CONN_STREAMS_DTYPE = np.dtype([
    ("map", ENTRY_DTYPE, SLOTS), ("buf", BUF_DTYPE, SLOTS), ("max_bidi_remote", "<u8"), ("max_uni_remote", "<u8"),
    ("reserved", "<u8", 2),
])
EVT_DTYPE = np.dtype([
    ("frame", "<u4"), ("conn", "<u4"), ("src", "<u8"), ("dst", "<u4"), ("copy_len", "<u2"), ("skip", "<u2"),
    ("map_slot", "u1"), ("buf_slot", "u1"), ("mark", "u1"), ("store", "u1"), ("flags", "u1"), ("type", "u1"),
    ("reserved", "u1", 2),
])
READ_REQ_DTYPE = np.dtype([("conn", "<u4"), ("cap", "<u4"), ("stream_id", "<u8"), ("out_offset", "<u8"),
                           ("reserved", "<u8")])
READ_RES_DTYPE = np.dtype([("copied", "<u4"), ("status", "u1"), ("fin", "u1"), ("slot", "u1"), ("reserved", "u1")])
assert (ENTRY_DTYPE.itemsize, BUF_DTYPE.itemsize, CONN_STREAMS_DTYPE.itemsize, EVT_DTYPE.itemsize,
        READ_REQ_DTYPE.itemsize, READ_RES_DTYPE.itemsize) == (48, 32, 2592, 32, 32, 8)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def workspace_bytes(max_frames, n_conns):
    return _lib.load().mq_batch_stream_data_workspace_size(max_frames, n_conns)


def read_workspace_bytes(n_reqs, n_conns):
    return _lib.load().mq_batch_stream_read_workspace_size(n_reqs, n_conns)


def _state(streams, bufs, stream_buf):
    n_conns = _nbytes(streams) // CONN_STREAMS_DTYPE.itemsize
    if _nbytes(streams) != CONN_STREAMS_DTYPE.itemsize * n_conns:
        raise InvalidArgument("streams holds one 2592-byte row per connection")
    if _nbytes(bufs) < SLOTS * stream_buf * n_conns:
        raise InvalidArgument(f"bufs needs {SLOTS} * stream_buf bytes per connection")
    return n_conns


def deliver(arena, pkts, n_pkts, dgrams, frames, n_frames, streams, bufs, stream_buf, initial_max_stream_data, evts,
            n_evts, workspace, flags=0, stream=None):
    """mq_batch_stream_data over device tensors: ``arena``, ``pkts`` (PKT_DTYPE, its size is max_pkts) and
    ``n_pkts`` as ``recv.recv`` left them, ``dgrams`` (DGRAM_DTYPE), ``frames`` (FRAME_DTYPE, its size is
    max_frames) and ``n_frames`` as ``frames.scan`` wrote them. ``streams`` (CONN_STREAMS_DTYPE: its size
    gives n_conns) and ``bufs`` are updated in place; ``evts`` (EVT_DTYPE, max_frames entries) receives one
    event per processed record and ``n_evts`` (one int32 / uint32) their number. ``flags``: CLIENT."""
    max_pkts = _nbytes(pkts) // PKT_DTYPE.itemsize
    n_dgrams = _nbytes(dgrams) // DGRAM_DTYPE.itemsize
    max_frames = _nbytes(frames) // FRAME_DTYPE.itemsize
    n_conns = _state(streams, bufs, stream_buf)
    if _nbytes(evts) < EVT_DTYPE.itemsize * max_frames:
        raise InvalidArgument("evts needs 32 bytes per frame record")
    if _nbytes(n_pkts) < 4 or _nbytes(n_frames) < 4 or _nbytes(n_evts) < 4:
        raise InvalidArgument("n_pkts, n_frames and n_evts are one 32-bit word each")
    if _nbytes(workspace) < workspace_bytes(max_frames, n_conns):
        raise InvalidArgument(f"workspace needs {workspace_bytes(max_frames, n_conns)} bytes")
    rc = _lib.load().mq_batch_stream_data(_ptr(arena), arena.numel(), _ptr(pkts), _ptr(n_pkts), max_pkts, _ptr(dgrams),
                                          n_dgrams, _ptr(frames), _ptr(n_frames), max_frames, _ptr(streams), n_conns,
                                          _ptr(bufs), stream_buf, initial_max_stream_data, flags, _ptr(evts),
                                          _ptr(n_evts), _ptr(workspace), _stream_ptr(stream))
    _raise(rc)


def read(streams, bufs, stream_buf, reqs, out, res, workspace, stream=None):
    """mq_batch_stream_read over device tensors: ``reqs`` (READ_REQ_DTYPE; its size is n_reqs) are answered
    into ``res`` (READ_RES_DTYPE) and ``out``; the buffer headers in ``streams`` advance. Output ranges of
    different requests must not overlap."""
    n_conns = _state(streams, bufs, stream_buf)
    n_reqs = _nbytes(reqs) // READ_REQ_DTYPE.itemsize
    if _nbytes(res) < READ_RES_DTYPE.itemsize * n_reqs:
        raise InvalidArgument("res needs 8 bytes per request")
    if _nbytes(workspace) < read_workspace_bytes(n_reqs, n_conns):
        raise InvalidArgument(f"workspace needs {read_workspace_bytes(n_reqs, n_conns)} bytes")
    rc = _lib.load().mq_batch_stream_read(_ptr(streams), n_conns, _ptr(bufs), stream_buf, _ptr(reqs), n_reqs, _ptr(out),
                                          out.numel(), _ptr(res), _ptr(workspace), _stream_ptr(stream))
    _raise(rc)
