"""ACKs on the GPU: received-PN trackers and ACK frames behind the frame index.

The per-packet work between ``frames.scan`` and ``send.protect``: every opened packet's number is
recorded in the tracker of its (connection, level) (track_received_pn -> RecvPnTracker::record,
reference src/connection/recv.rs:248-249, src/connection/mod.rs:194-296), and a tracker whose level
has seen an ack-eliciting packet is turned into an ACK frame with a send request of its own
(build_ack_frame, src/connection/transmit.rs:321-380). ``track_and_build`` runs mq_batch_acks over
the device tensors that ``recv.recv`` and ``frames.scan`` leave behind; the packet count is read on
the device, so recv -> frames -> acks -> protect chain on one stream with nothing read back. The
state that stays resident between calls is ``trackers`` (``TRACKER_DTYPE``, 3 per connection),
``pending`` (one word per connection) and ``next_pn`` (3 per connection). The semantics are spelled
out in include/mq_aead.h.
"""
import ctypes

import numpy as np

from . import _lib
from .batch import _nbytes, _opt_ptr, _stream_ptr
from .crypto import InvalidArgument, _raise
from .frames import PKT_FRAMES_DTYPE
from .recv import CONN_DTYPE, DGRAM_DTYPE, PKT_DTYPE
from .send import REQ_DTYPE

RANGES = _lib.MQ_PN_TRACKER_RANGES
FRAME_MAX = _lib.MQ_ACK_FRAME_MAX
CLIENT = _lib.MQ_ACKS_CLIENT

TRACKER_DTYPE = np.dtype([("n", "<u4"), ("reserved", "<u4", 3), ("range", "<u8", (RANGES, 2))])
assert TRACKER_DTYPE.itemsize == 528 and ctypes.sizeof(_lib.AckBuild) == 56


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def workspace_bytes(max_pkts, n_conns):
    return _lib.load().mq_batch_acks_workspace_size(max_pkts, n_conns)


class Build:
    """The build half's outputs (mq_ack_build): ``ack_frames`` (FRAME_MAX bytes per ACK), ``reqs``
    (send.REQ_DTYPE; its size is max_acks), ``n_acks`` (one int32 / uint32: the ACKs due, which may
    exceed max_acks), ``conns`` (recv.CONN_DTYPE, for largest_pn), ``next_pn`` (3 uint64 per
    connection, in/out), ``out_stride`` (output bytes per ACK packet) and ``flags`` (CLIENT)."""

    def __init__(self, ack_frames, reqs, n_acks, conns, next_pn, out_stride, flags=0):
        self.ack_frames, self.reqs, self.n_acks, self.conns, self.next_pn = ack_frames, reqs, n_acks, conns, next_pn
        self.out_stride, self.flags = out_stride, flags
        self.max_acks = _nbytes(reqs) // REQ_DTYPE.itemsize

    def struct(self, n_conns):
        if _nbytes(self.ack_frames) < FRAME_MAX * self.max_acks:
            raise InvalidArgument(f"ack_frames needs {FRAME_MAX} bytes per request")
        if _nbytes(self.n_acks) < 4:
            raise InvalidArgument("n_acks is one 32-bit word")
        if _nbytes(self.conns) < CONN_DTYPE.itemsize * n_conns or _nbytes(self.next_pn) < 24 * n_conns:
            raise InvalidArgument("conns needs 64 and next_pn 24 bytes per connection")
        b = _lib.AckBuild()
        b.ack_frames, b.reqs, b.n_acks = self.ack_frames.data_ptr(), self.reqs.data_ptr(), self.n_acks.data_ptr()
        b.conns, b.next_pn = self.conns.data_ptr(), self.next_pn.data_ptr()
        b.max_acks, b.out_stride, b.flags = self.max_acks, self.out_stride, self.flags
        return b


def track_and_build(pkts, n_pkts, dgrams, trackers, pending, workspace, summary=None, conn_flags=None, build=None,
                    stream=None):
    """mq_batch_acks over device tensors: ``pkts`` (PKT_DTYPE records, its size is max_pkts) and
    ``n_pkts`` as ``recv.recv`` wrote them, ``dgrams`` (DGRAM_DTYPE), ``trackers`` (TRACKER_DTYPE, three
    per connection: its size gives n_conns) and ``pending`` (one int32 / uint32 per connection), both
    updated in place. ``summary`` and ``conn_flags`` are what ``frames.scan`` wrote (optional: without
    ``summary`` every opened packet is recorded, without ``conn_flags`` nothing new becomes pending).
    ``build`` is a ``Build`` or None (track only)."""
    max_pkts = _nbytes(pkts) // PKT_DTYPE.itemsize
    n_dgrams = _nbytes(dgrams) // DGRAM_DTYPE.itemsize
    n_conns = _nbytes(trackers) // (3 * TRACKER_DTYPE.itemsize)
    if _nbytes(trackers) != 3 * TRACKER_DTYPE.itemsize * n_conns or _nbytes(pending) < 4 * n_conns:
        raise InvalidArgument("trackers holds three 528-byte trackers and pending one word per connection")
    if summary is not None and _nbytes(summary) < PKT_FRAMES_DTYPE.itemsize * max_pkts:
        raise InvalidArgument("summary needs 16 bytes per packet record")
    if conn_flags is not None and _nbytes(conn_flags) < 4 * n_conns:
        raise InvalidArgument("conn_flags needs one word per connection")
    if _nbytes(n_pkts) < 4:
        raise InvalidArgument("n_pkts is one 32-bit word")
    if _nbytes(workspace) < workspace_bytes(max_pkts, n_conns):
        raise InvalidArgument(f"workspace needs {workspace_bytes(max_pkts, n_conns)} bytes")
    b = build.struct(n_conns) if build is not None else None
    rc = _lib.load().mq_batch_acks(_ptr(pkts), _ptr(n_pkts), max_pkts, _opt_ptr(summary), _ptr(dgrams), n_dgrams,
                                   _opt_ptr(conn_flags), _ptr(trackers), _ptr(pending), n_conns,
                                   ctypes.byref(b) if b is not None else None, _ptr(workspace), _stream_ptr(stream))
    _raise(rc)
