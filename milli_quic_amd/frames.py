"""Frame index on the GPU: the frames of every opened packet as fixed-size records.

The step behind ``recv.recv``: dispatch_frames (reference src/connection/recv.rs:518-545) calling
frame::decode (src/frame/mod.rs:228-461) in a loop. ``scan`` runs mq_batch_frames over the packet
records and the plaintext arena that ``recv.recv`` leaves on the device and yields one ``FRAME_DTYPE``
record per frame other than PADDING, in arrival order, one ``PKT_FRAMES_DTYPE`` summary per packet and,
optionally, one flag word per connection. The packet count is read on the device, so the call chains
behind ``recv.recv`` on one stream with nothing read back. The semantics are spelled out in
include/mq_aead.h.
"""
import ctypes

import numpy as np

from . import _lib
from .batch import _nbytes, _opt_ptr, _stream_ptr
from .crypto import InvalidArgument, _raise
from .recv import DGRAM_DTYPE, PKT_DTYPE

OK = _lib.MQ_OK
ERR_FRAME = _lib.MQ_ERR_FRAME
ERR_INVALID_ARG = _lib.MQ_ERR_INVALID_ARG
SKIPPED = _lib.MQ_FRAMES_SKIPPED
ACK_ELICITING = _lib.MQ_FRAMES_ACK_ELICITING            # PKT_FRAMES_DTYPE flags
CONN_CLOSE, CONN_ERROR = _lib.MQ_CONN_FRAMES_CLOSE, _lib.MQ_CONN_FRAMES_ERROR  # conn_flags, beside bit `level`
MAX_PKTS = 1 << 24

FRAME_DTYPE = np.dtype([
    ("pkt", "<u4"), ("pos", "<u2"), ("len", "<u2"), ("type", "u1"), ("level", "u1"), ("data_pos", "<u2"),
    ("data_len", "<u2"), ("aux", "<u2"), ("v", "<u8", 4),
])
PKT_FRAMES_DTYPE = np.dtype([
    ("first", "<u4"), ("n_frames", "<u2"), ("err_pos", "<u2"), ("n_padding", "<u2"), ("status", "u1"),
    ("flags", "u1"), ("reserved", "<u4"),
])
assert FRAME_DTYPE.itemsize == 48 and PKT_FRAMES_DTYPE.itemsize == 16


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def workspace_bytes(max_pkts):
    return _lib.load().mq_batch_frames_workspace_size(max_pkts)


def scan(arena, pkts, n_pkts, summary, frames, n_frames, workspace, dgrams=None, conn_flags=None, stream=None):
    """mq_batch_frames over device tensors: ``pkts`` (PKT_DTYPE records, its size is max_pkts) and
    ``n_pkts`` (one int32 / uint32) as ``recv.recv`` wrote them, ``summary`` (PKT_FRAMES_DTYPE, one per
    packet record), ``frames`` (FRAME_DTYPE, its size is max_frames) and ``n_frames`` (one int32 /
    uint32: the total, which may exceed max_frames). ``dgrams`` and ``conn_flags`` (one int32 / uint32
    per connection) are given together or not at all."""
    max_pkts = _nbytes(pkts) // PKT_DTYPE.itemsize
    max_frames = _nbytes(frames) // FRAME_DTYPE.itemsize
    if _nbytes(summary) < PKT_FRAMES_DTYPE.itemsize * max_pkts:
        raise InvalidArgument("summary needs 16 bytes per packet record")
    if _nbytes(n_pkts) < 4 or _nbytes(n_frames) < 4:
        raise InvalidArgument("n_pkts and n_frames are one 32-bit word each")
    if _nbytes(workspace) < workspace_bytes(max_pkts):
        raise InvalidArgument(f"workspace needs {workspace_bytes(max_pkts)} bytes for {max_pkts} packet records")
    if (dgrams is None) != (conn_flags is None):
        raise InvalidArgument("dgrams and conn_flags are given together or not at all")
    n_dgrams = _nbytes(dgrams) // DGRAM_DTYPE.itemsize if dgrams is not None else 0
    n_conns = _nbytes(conn_flags) // 4 if conn_flags is not None else 0
    rc = _lib.load().mq_batch_frames(_ptr(arena), arena.numel(), _ptr(pkts), _ptr(n_pkts), max_pkts,
                                     _opt_ptr(dgrams), n_dgrams, _ptr(summary), _ptr(frames), max_frames,
                                     _ptr(n_frames), _opt_ptr(conn_flags), n_conns, _ptr(workspace),
                                     _stream_ptr(stream))
    _raise(rc)
