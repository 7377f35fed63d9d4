"""Loss recovery on the GPU: sent-packet tracking behind ``send.protect`` and received ACK frames behind
the frame index.

What the reference does for every packet it sends (src/connection/transmit.rs:610-619, 743-752) and for
every ACK frame it receives (Frame::Ack in dispatch_frame, src/connection/recv.rs:563-612, with
Frame::HandshakeDone, recv.rs:692-704) on its SentPacketTracker, LossDetector and CongestionController
(src/transport/recovery.rs, loss.rs, congestion.rs). ``sent`` runs mq_batch_sent over the request, status
and length tables of ``send.protect``; ``process`` runs mq_batch_recovery over the device tensors that
``recv.recv`` and ``frames.scan`` leave behind. Both counts are read on the device, so
recv -> frames -> recovery and acks -> protect -> sent chain on one stream with nothing read back. The
state that stays resident between calls is ``rec`` (``CONN_RECOVERY_DTYPE``, one row per connection). The
semantics are spelled out in include/mq_aead.h.
"""
import ctypes

import numpy as np

from . import _lib
from .batch import _nbytes, _stream_ptr
from .crypto import InvalidArgument, _raise
from .frames import FRAME_DTYPE
from .recv import DGRAM_DTYPE, PKT_DTYPE

SLOTS = _lib.MQ_SENT_SLOTS
CLIENT = _lib.MQ_RECOVERY_CLIENT
CONFIRMED = _lib.MQ_RECOVERY_CONFIRMED
USED, ACK_ELICITING, IN_FLIGHT = 0x01, 0x02, 0x04                       # SENT_DTYPE flags
RTT, RANGES_CUT, RANGES_BROKE, LOST_CUT = 0x01, 0x02, 0x04, 0x08        # EVT_DTYPE flags
# CONN_RECOVERY_DTYPE have: bit l of each group of three is level l
HAVE_LARGEST_ACKED, HAVE_LAST_SENT, HAVE_LOSS_TIME, HAVE_SRTT, HAVE_RECOVERY_START = 1 << 0, 1 << 3, 1 << 6, 1 << 9, 1 << 10
NONE = 0xFFFFFFFFFFFFFFFF                                               # a timeout that is None; min_rtt before a sample
MAX_FRAMES, MAX_REQS, MAX_CONNS = 1 << 26, 1 << 26, 1 << 30

SENT_DTYPE = np.dtype([("pn", "<u8"), ("time_sent", "<u8"), ("size", "<u2"), ("level", "u1"), ("flags", "u1"),
                       ("reserved", "<u4")])
CONN_RECOVERY_DTYPE = np.dtype([
    ("largest_acked", "<u8", 3), ("time_of_last_ack_eliciting", "<u8", 3), ("loss_time", "<u8", 3),
    ("smoothed_rtt", "<u8"), ("rttvar", "<u8"), ("min_rtt", "<u8"), ("latest_rtt", "<u8"), ("max_ack_delay", "<u8"),
    ("cwnd", "<u8"), ("ssthresh", "<u8"), ("bytes_in_flight", "<u8"), ("recovery_start_time", "<u8"),
    ("persistent_congestion_threshold", "<u8"), ("max_datagram_size", "<u8"), ("minimum_window", "<u8"),
    ("have", "<u4"), ("pto_count", "<u4"), ("count", "<u4"), ("flags", "<u4"), ("reserved", "<u8"),
    ("sent", SENT_DTYPE, SLOTS),
])
EVT_DTYPE = np.dtype([
    ("frame", "<u4"), ("conn", "<u4"), ("n_acked", "<u2"), ("n_acked_cc", "<u2"), ("n_lost", "<u2"), ("flags", "<u2"),
    ("lost_first", "<u4"), ("reserved", "<u4"), ("largest_newly_acked", "<u8"),
])
LOST_DTYPE = np.dtype([("pn", "<u8"), ("conn", "<u4"), ("size", "<u2"), ("level", "u1"), ("reserved", "u1")])
assert (SENT_DTYPE.itemsize, CONN_RECOVERY_DTYPE.itemsize, EVT_DTYPE.itemsize, LOST_DTYPE.itemsize) == (24, 3264, 32, 16)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def state_rows(n_conns, max_ack_delay_us=25_000, max_datagram_size=1200):
    """``n_conns`` fresh rows (host, CONN_RECOVERY_DTYPE) as mq_recovery_state_init fills them."""
    rows = np.zeros(n_conns, dtype=CONN_RECOVERY_DTYPE)
    if n_conns:
        one = np.zeros(1, dtype=CONN_RECOVERY_DTYPE)
        _raise(_lib.load().mq_recovery_state_init(one.ctypes.data_as(ctypes.c_void_p), max_ack_delay_us,
                                                  max_datagram_size))
        rows[:] = one[0]
    return rows


def workspace_bytes(max_frames, n_conns):
    return _lib.load().mq_batch_recovery_workspace_size(max_frames, n_conns)


def sent_workspace_bytes(n, n_conns):
    return _lib.load().mq_batch_sent_workspace_size(n, n_conns)


def _rows(rec):
    n_conns = _nbytes(rec) // CONN_RECOVERY_DTYPE.itemsize
    if _nbytes(rec) != CONN_RECOVERY_DTYPE.itemsize * n_conns:
        raise InvalidArgument("rec holds one 3264-byte row per connection")
    return n_conns


def sent(reqs, status, pkt_len, now, rec, workspace, timeouts=None, stream=None):
    """mq_batch_sent over device tensors: ``reqs`` (send.REQ_DTYPE; its size is n), ``status`` (uint8) and
    ``pkt_len`` (int32 / uint32) as ``send.protect`` took and left them, ``now`` (int64 / uint64, n entries,
    microseconds). ``rec`` (CONN_RECOVERY_DTYPE: its size gives n_conns) is updated in place; ``timeouts``
    (int64 / uint64, n_conns entries, optional) receives next_timeout of the connections that recorded a packet."""
    n = _nbytes(reqs) // 48
    n_conns = _rows(rec)
    if _nbytes(status) < n or _nbytes(pkt_len) < 4 * n or _nbytes(now) < 8 * n:
        raise InvalidArgument("status, pkt_len and now need one entry per request")
    if timeouts is not None and _nbytes(timeouts) < 8 * n_conns:
        raise InvalidArgument("timeouts needs 8 bytes per connection")
    if _nbytes(workspace) < sent_workspace_bytes(n, n_conns):
        raise InvalidArgument(f"workspace needs {sent_workspace_bytes(n, n_conns)} bytes")
    rc = _lib.load().mq_batch_sent(_ptr(reqs), _ptr(status), _ptr(pkt_len), n, _ptr(now), _ptr(rec), n_conns,
                                   _ptr(timeouts), _ptr(workspace), _stream_ptr(stream))
    _raise(rc)


def process(arena, pkts, n_pkts, dgrams, dgram_now, frames, n_frames, rec, evts, n_evts, lost, n_lost, workspace,
            drop_mask=None, timeouts=None, flags=0, stream=None):
    """mq_batch_recovery over device tensors: ``arena``, ``pkts`` (PKT_DTYPE, its size is max_pkts) and ``n_pkts``
    as ``recv.recv`` left them, ``dgrams`` (DGRAM_DTYPE) with ``dgram_now`` (int64 / uint64, one time per
    datagram, microseconds), ``frames`` (FRAME_DTYPE, its size is max_frames) and ``n_frames`` as ``frames.scan``
    wrote them. ``rec`` (CONN_RECOVERY_DTYPE: its size gives n_conns) is updated in place; ``evts`` (EVT_DTYPE,
    max_frames entries) receives one event per processed ACK record and ``n_evts`` their number; ``lost``
    (LOST_DTYPE, its size is max_lost) the lost packets and ``n_lost`` their total, which can exceed max_lost.
    ``drop_mask`` (uint8 per connection, optional): levels to drop first. ``flags``: CLIENT."""
    max_pkts = _nbytes(pkts) // PKT_DTYPE.itemsize
    n_dgrams = _nbytes(dgrams) // DGRAM_DTYPE.itemsize
    max_frames = _nbytes(frames) // FRAME_DTYPE.itemsize
    max_lost = _nbytes(lost) // LOST_DTYPE.itemsize
    n_conns = _rows(rec)
    if _nbytes(evts) < EVT_DTYPE.itemsize * max_frames:
        raise InvalidArgument("evts needs 32 bytes per frame record")
    if _nbytes(dgram_now) < 8 * n_dgrams:
        raise InvalidArgument("dgram_now needs 8 bytes per datagram")
    if _nbytes(n_pkts) < 4 or _nbytes(n_frames) < 4 or _nbytes(n_evts) < 4 or _nbytes(n_lost) < 4:
        raise InvalidArgument("n_pkts, n_frames, n_evts and n_lost are one 32-bit word each")
    if drop_mask is not None and _nbytes(drop_mask) < n_conns:
        raise InvalidArgument("drop_mask needs one byte per connection")
    if timeouts is not None and _nbytes(timeouts) < 8 * n_conns:
        raise InvalidArgument("timeouts needs 8 bytes per connection")
    if _nbytes(workspace) < workspace_bytes(max_frames, n_conns):
        raise InvalidArgument(f"workspace needs {workspace_bytes(max_frames, n_conns)} bytes")
    rc = _lib.load().mq_batch_recovery(_ptr(arena), arena.numel(), _ptr(pkts), _ptr(n_pkts), max_pkts, _ptr(dgrams),
                                       n_dgrams, _ptr(dgram_now), _ptr(frames), _ptr(n_frames), max_frames,
                                       _ptr(drop_mask), _ptr(rec), n_conns, _ptr(evts), _ptr(n_evts), _ptr(lost),
                                       max_lost, _ptr(n_lost), _ptr(timeouts), flags, _ptr(workspace),
                                       _stream_ptr(stream))
    _raise(rc)
