"""Pure-Python model of mq_batch_route and the connection-ID table (include/mq_aead.h, steps 1-6):
a dict keyed by ``bytes``, no hash. The reference for test_route.py and test_gpu_route.py; every
comparison against it is exact.

decode_dcid restates the reference's src/packet/decode_dcid.rs:9-37; the admission rule is the
reference's first-Initial rule (src/connection/recv.rs:275-278) with RFC 9000 §14.1 / §17.2.
"""
import numpy as np

from milli_quic_amd import recv
from milli_quic_amd.route import (CONN_NONE, DEFERRED, FULL, HIT, MALFORMED, MAX_CID_LEN, NEW, OK,  # noqa: F401
                                  UNKNOWN)


def decode_dcid(datagram, short_dcid_len):
    """decode_dcid.rs:9-37: the DCID of a datagram, or None."""
    if len(datagram) == 0:
        return None
    if datagram[0] & 0x80:
        if len(datagram) < 6:
            return None
        end = 6 + datagram[5]
        if len(datagram) < end:
            return None
        return bytes(datagram[6:end])
    end = 1 + short_dcid_len
    if len(datagram) < end:
        return None
    return bytes(datagram[1:end])


def route_cid(datagram, short_dcid_len):
    """Step 2: decode_dcid, plus our rule that a long-header DCID over 20 bytes is malformed."""
    cid = decode_dcid(datagram, short_dcid_len)
    if cid is None or len(cid) > MAX_CID_LEN:
        return None
    return cid


def admissible(datagram, min_initial_len):
    """Step 4 for a datagram whose CID missed (admit given)."""
    return bool(datagram[0] & 0x80) and (datagram[0] & 0x30) == 0 and bytes(datagram[1:5]) != bytes(4) \
        and len(datagram) >= min_initial_len


class AdmitModel:
    def __init__(self, conns, conn_base, max_new, row_first, min_initial_len=1200):
        self.conns = conns  # numpy recv.CONN_DTYPE, updated in place
        self.conn_base, self.max_new, self.row_first, self.min_initial_len = conn_base, max_new, row_first, min_initial_len
        self.new_dcids = []  # bytes, one per admitted connection


class TableModel:
    def __init__(self, capacity):
        self.capacity = capacity
        self.map = {}

    def insert(self, cids, conns):
        """One insert call of distinct CIDs -> statuses."""
        st = []
        for cid, conn in zip(cids, conns):
            if len(cid) > MAX_CID_LEN:
                st.append(MALFORMED)
            elif cid in self.map:
                st.append(HIT)
            elif len(self.map) >= self.capacity:
                st.append(FULL)
            else:
                self.map[cid] = conn
                st.append(OK)
        return st

    def remove(self, cids):
        return [OK if self.map.pop(cid, None) is not None else UNKNOWN for cid in cids]

    def route(self, arena, dgrams, short_dcid_len, admit=None):
        """Steps 1-6. Returns (status, conn) arrays; with admit, admit.new_dcids and admit.conns are
        updated and the new entries inserted."""
        n = len(dgrams)
        status = np.zeros(n, dtype=np.uint8)
        conn = np.full(n, CONN_NONE, dtype=np.uint32)
        groups = {}  # cid -> datagram indices, in order of each group's first datagram
        for i in range(n):
            off, ln = int(dgrams[i]["offset"]), int(dgrams[i]["len"])
            if off + ln > len(arena):
                status[i] = MALFORMED
                continue
            d = bytes(arena[off:off + ln])
            cid = route_cid(d, short_dcid_len)
            if cid is None:
                status[i] = MALFORMED
            elif cid in self.map:
                status[i], conn[i] = HIT, self.map[cid]
            elif admit is not None and admissible(d, admit.min_initial_len):
                groups.setdefault(cid, []).append(i)
            else:
                status[i] = UNKNOWN
        if admit is not None:
            limit = min(admit.max_new, self.capacity - len(self.map))
            admit.new_dcids = []
            for k, (cid, members) in enumerate(groups.items()):
                if k < limit:
                    c = admit.conn_base + k
                    status[members], conn[members] = NEW, c
                    admit.new_dcids.append(cid)
                    self.map[cid] = c
                    row = np.zeros(1, dtype=recv.CONN_DTYPE)
                    row["initial_row"], row["flags"], row["dcid_len"] = admit.row_first + 2 * k, recv.HAS_INITIAL, short_dcid_len
                    admit.conns[c] = row[0]
                else:
                    status[members] = FULL
        return status, conn


# ---- not part of the model: the table's hash, for the tests that force collisions --------------------
_M64 = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M64


def sip13_cid(seed, cid):
    """mq_route.h route_sip13: SipHash-1-3 under the 16-byte seed over the CID zero-padded to three
    64-bit words, its length in the top byte of the last (test_route.py pins it to the C++ code)."""
    k0, k1 = int.from_bytes(seed[:8], "little"), int.from_bytes(seed[8:], "little")
    v = [k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573]

    def rnd():
        v[0] = (v[0] + v[1]) & _M64; v[1] = _rotl(v[1], 13) ^ v[0]; v[0] = _rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & _M64; v[3] = _rotl(v[3], 16) ^ v[2]
        v[0] = (v[0] + v[3]) & _M64; v[3] = _rotl(v[3], 21) ^ v[0]
        v[2] = (v[2] + v[1]) & _M64; v[1] = _rotl(v[1], 17) ^ v[2]; v[2] = _rotl(v[2], 32)

    pad = bytes(cid) + bytes(24 - len(cid))
    words = [int.from_bytes(pad[8 * q:8 * q + 8], "little") for q in range(3)]
    words[2] |= len(cid) << 56
    for m in words:
        v[3] ^= m
        rnd()
        v[0] ^= m
    v[2] ^= 0xFF
    rnd(), rnd(), rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def hash_class(seed, cid, bits):
    """The slot word's class with mq_debug_cid_table_hash_bits(bits): CIDs collide iff equal here."""
    return (sip13_cid(seed, cid) & ((1 << min(bits, 59)) - 1), len(cid))
