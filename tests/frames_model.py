"""Python model of mq_batch_frames: decode_varint (reference src/varint.rs:31-67), frame::decode
(src/frame/mod.rs:228-461) and dispatch_frames' summary (src/connection/recv.rs:518-545), restated,
plus the generators of the cases that the host replay, the GPU ladder and the fuzz share."""
import numpy as np

from milli_quic_amd import frames, recv

OK, ERR_FRAME, SKIPPED, INVALID = frames.OK, frames.ERR_FRAME, frames.SKIPPED, frames.ERR_INVALID_ARG
VARINT_MAX = (1 << 62) - 1


class FrameEncodingError(Exception):
    pass


class BufferTooSmall(Exception):
    pass


def encode_varint(v, width=None):
    """The shortest encoding, or the one of `width` bytes (1, 2, 4, 8)."""
    if width is None:
        width = 1 if v < 1 << 6 else 2 if v < 1 << 14 else 4 if v < 1 << 30 else 8
    assert v < 1 << (8 * width - 2), (v, width)
    return (v | {1: 0, 2: 1, 4: 2, 8: 3}[width] << (8 * width - 2)).to_bytes(width, "big")


def decode_varint(buf):
    """varint.rs:31-67: (value, length)."""
    if len(buf) == 0:
        raise BufferTooSmall(1)
    n = 1 << (buf[0] >> 6)
    if len(buf) < n:
        raise BufferTooSmall(n)
    return int.from_bytes(bytes([buf[0] & 0x3F]) + bytes(buf[1:n]), "big"), n


class _Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def varint(self):  # read_varint, mod.rs:183-190
        if self.pos >= len(self.buf):
            raise FrameEncodingError
        try:
            v, n = decode_varint(self.buf[self.pos:])
        except BufferTooSmall:
            raise FrameEncodingError from None
        self.pos += n
        return v

    def bytes(self, n):  # read_bytes, mod.rs:200-207: (position, length)
        if self.pos > len(self.buf) or len(self.buf) - self.pos < n:
            raise FrameEncodingError
        at = self.pos
        self.pos += n
        return at, n


def decode(buf):
    """frame::decode: (fields, consumed); fields = dict(type, v[4], data_pos, data_len, aux), the
    positions relative to buf. Raises FrameEncodingError."""
    r = _Reader(buf)
    t = r.varint()
    v, data, aux = [0, 0, 0, 0], (0, 0), 0
    if t in (0x00, 0x01, 0x1E):
        pass
    elif t in (0x02, 0x03):
        v = [r.varint(), r.varint(), r.varint(), r.varint()]
        start = r.pos
        k = 0
        while k < v[2]:  # fails where the bytes run out: at most len / 2 rounds
            r.varint()
            r.varint()
            k += 1
        data = (start, r.pos - start)
        if t == 0x03:
            aux = r.pos
            r.varint(), r.varint(), r.varint()
    elif t == 0x04:
        v[0:3] = [r.varint(), r.varint(), r.varint()]
    elif t in (0x05, 0x11, 0x15):
        v[0:2] = [r.varint(), r.varint()]
    elif t == 0x06:
        v[1] = r.varint()
        data = r.bytes(r.varint())
    elif t == 0x07:
        data = r.bytes(r.varint())
    elif 0x08 <= t <= 0x0F:
        v[0] = r.varint()
        if t & 0x04:
            v[1] = r.varint()
        if t & 0x02:
            data = r.bytes(r.varint())
        else:
            data = (r.pos, len(buf) - r.pos)
            r.pos = len(buf)
    elif t in (0x10, 0x12, 0x13, 0x14, 0x16, 0x17, 0x19):
        v[0] = r.varint()
    elif t == 0x18:
        v[0:2] = [r.varint(), r.varint()]
        n = r.varint()
        if n > 20:
            raise FrameEncodingError
        data = r.bytes(n)
        aux = r.bytes(16)[0]
    elif t in (0x1A, 0x1B):
        data = r.bytes(8)
    elif t in (0x1C, 0x1D):
        v[0] = r.varint()
        if t == 0x1C:
            v[1] = r.varint()
        data = r.bytes(r.varint())
    else:
        raise FrameEncodingError
    return dict(type=t, v=v, data_pos=data[0], data_len=data[1], aux=aux), r.pos


def walk(payload):
    """dispatch_frames over one payload: (summary dict, records). A record is (pos, len, type,
    data_pos, data_len, aux, v) with positions relative to the payload."""
    payload = bytes(payload)
    pos, recs, pads, flags, close = 0, [], 0, 0, False
    status, err_pos = OK, 0
    while pos < len(payload):
        try:
            f, used = decode(payload[pos:])
        except FrameEncodingError:
            status, err_pos = ERR_FRAME, pos
            break
        if f["type"] == 0:
            pads += 1
        else:
            if f["type"] not in (0x02, 0x03):
                flags |= frames.ACK_ELICITING
            close = close or f["type"] in (0x1C, 0x1D)
            # a frame's data and aux positions lie behind its type byte: 0 means "no such field"
            dp = f["data_pos"] + pos if f["data_pos"] else 0
            recs.append((pos, used, f["type"], dp, f["data_len"], f["aux"] + pos if f["aux"] else 0, f["v"]))
        pos += used
    return dict(status=status, err_pos=err_pos, n_padding=pads, flags=flags, close=close), recs


def run(arena, pkts, n_pkts, dgrams=None, n_conns=0):
    """mq_batch_frames over host arrays: (summary, records, conn_flags)."""
    arena = np.asarray(arena, dtype=np.uint8)
    n = min(int(n_pkts), len(pkts))
    summary = np.zeros(n, dtype=frames.PKT_FRAMES_DTYPE)
    out = []
    conn_flags = np.zeros(n_conns, dtype=np.uint32)
    for i in range(n):
        pk = pkts[i]
        summary[i]["first"] = len(out)
        if pk["status"] != OK:
            summary[i]["status"] = SKIPPED
            continue
        off, ln, po = int(pk["offset"]), int(pk["len"]), int(pk["payload_offset"])
        if off > len(arena) or ln > len(arena) - off or po + 16 > ln or ln - po - 16 > 0xFFFF:
            summary[i]["status"] = INVALID
            continue
        s, recs = walk(arena[off + po:off + ln - 16].tobytes())
        for (pos, used, t, dp, dl, aux, v) in recs:
            out.append((i, pos, used, t, int(pk["level"]), dp, dl, aux, v))
        summary[i]["n_frames"], summary[i]["err_pos"] = len(recs), s["err_pos"]
        summary[i]["n_padding"], summary[i]["status"], summary[i]["flags"] = s["n_padding"], s["status"], s["flags"]
        if dgrams is not None and int(pk["dgram"]) < len(dgrams):
            c = int(dgrams[int(pk["dgram"])]["conn"])
            if c < n_conns:
                if s["status"] == OK and s["flags"] and pk["level"] < 3:
                    conn_flags[c] |= 1 << int(pk["level"])
                if s["close"]:
                    conn_flags[c] |= frames.CONN_CLOSE
                if s["status"] == ERR_FRAME:
                    conn_flags[c] |= frames.CONN_ERROR
    rec = np.zeros(len(out), dtype=frames.FRAME_DTYPE)
    for k, (i, pos, used, t, level, dp, dl, aux, v) in enumerate(out):
        rec[k] = (i, pos, used, t, level, dp, dl, aux, v)
    return summary, rec, conn_flags


# ---- frame builders ---------------------------------------------------------------------------------
def vi(v, w=None):
    return encode_varint(v, w)


def build(t, fields=(), tail=b"", tw=None, w=None):
    """type, varint fields and a tail of raw bytes; tw / w force the type's / the fields' width."""
    return vi(t, tw) + b"".join(vi(x, w) for x in fields) + tail


def sample_frames(w=None, tw=None):
    """One well-formed frame of every type (STREAM: all 8 flag combinations), every varint at width w.
    Frames that run to the payload's end (STREAM without LEN) come last in no list: each is alone."""
    D = bytes(range(1, 8))
    out = [
        build(0x00, tw=tw), build(0x01, tw=tw), build(0x1E, tw=tw),
        build(0x02, (9, 3, 0, 4), tw=tw, w=w),
        build(0x02, (60, 3, 2, 4, 1, 2, 3, 4), tw=tw, w=w),
        build(0x03, (9, 3, 1, 4, 1, 2, 7, 8, 9), tw=tw, w=w),
        build(0x04, (5, 6, 7), tw=tw, w=w), build(0x05, (5, 6), tw=tw, w=w),
        build(0x06, (11, len(D)), D, tw=tw, w=w), build(0x07, (len(D),), D, tw=tw, w=w),
        build(0x10, (37,), tw=tw, w=w), build(0x11, (4, 38), tw=tw, w=w), build(0x12, (39,), tw=tw, w=w),
        build(0x13, (40,), tw=tw, w=w), build(0x14, (41,), tw=tw, w=w), build(0x15, (8, 42), tw=tw, w=w),
        build(0x16, (43,), tw=tw, w=w), build(0x17, (44,), tw=tw, w=w),
        build(0x18, (3, 1, 8), bytes(range(8)) + bytes(range(16, 32)), tw=tw, w=w),
        build(0x19, (2,), tw=tw, w=w), build(0x1A, (), bytes(range(8)), tw=tw), build(0x1B, (), bytes(range(8)), tw=tw),
        build(0x1C, (10, 6, 3), b"why", tw=tw, w=w), build(0x1D, (10, 3), b"why", tw=tw, w=w),
    ]
    for t in range(0x08, 0x10):
        f = [4] + ([33] if t & 4 else []) + ([len(D)] if t & 2 else [])
        out.append(build(t, f, D, tw=tw, w=w))
    return out


def host_cases():
    """The payloads of the host replay and of the GPU ladder (ISSUE: every frame type, every prefix of
    each, every field at the 4 varint widths, wide type encodings, unknown types, CID lengths, length
    fields at and past the end and beyond 2^32, ACK range counts, the 8 STREAM flag combinations)."""
    cases = [b""]
    for w in (None, 1, 2, 4, 8):
        for f in sample_frames(w=w):
            cases += [f[:k] for k in range(1, len(f) + 1)]   # every prefix, the frame itself last
            cases.append(f + b"\x01")                          # followed by a PING
            cases.append(b"\x01\x00" + f)
    for tw in (2, 4, 8):
        for f in sample_frames(tw=tw):
            cases += [f, f[:len(f) - 1], b"\x00" * 3 + f + b"\x00" * 2]
    for t in (0x1F, 0x20, 0x3F, 0x40, VARINT_MAX):
        cases += [vi(t), b"\x01" + vi(t) + b"\x01", vi(t, 8)]
    for n in (20, 21):  # cid_len
        cases += [build(0x18, (1, 0, n), bytes(n + 16)), build(0x18, (1, 0, n), bytes(n + 15)),
                  build(0x18, (1, 0, n), bytes(n + 17))]
    D = bytes(10)
    for big in (10, 11, 1 << 32, (1 << 32) + 5, (1 << 32) + 10, VARINT_MAX):  # lengths against 10 bytes left
        cases += [build(0x06, (0, big), D), build(0x07, (big,), D), build(0x0A, (1, big), D),
                  build(0x0E, (1, 2, big), D), build(0x1C, (1, 2, big), D), build(0x1D, (1, big), D),
                  build(0x18, (1, 0, big), D + bytes(16))]
    pairs = b"\x01\x02" * 3
    for cnt in (0, 1, 3, 4, VARINT_MAX):  # ack_range_count against three pairs
        cases += [build(0x02, (5, 0, cnt, 1), pairs), build(0x03, (5, 0, cnt, 1), pairs + b"\x01\x02\x03"),
                  build(0x02, (5, 0, cnt, 1), pairs) + b"\x01"]
    cases.append(build(0x02, (5, 0, 2, 1), vi(1, 8) + vi(2, 4) + vi(3, 2) + vi(4, 1)))
    return cases


def padding_cases():
    """Padding runs of every length around the window sizes, before, between and behind frames, so that
    frame headers straddle every window edge."""
    runs = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1100)
    ack = build(0x03, (1 << 40, 300, 1, 70000, 1 << 20, 5, 7, 8, 9))   # a 30-byte header
    crypto = build(0x06, (1 << 33, 20), bytes(range(100, 120)))
    cases = []
    for r in runs:
        z = bytes(r)
        cases += [z, z + b"\x01", b"\x01" + z, ack + z + crypto + z, z + ack + z, z + crypto, z + ack[:11],
                  crypto + z + b"\x1f"]
    for lead in list(range(0, 40)) + list(range(96, 136)) + list(range(224, 264)) + list(range(480, 520)):
        cases.append(bytes(lead) + ack + b"\x01")  # the header slides over the window edges
    cases.append(b"\x01" * 300)
    cases.append(b"\x40\x00" * 5 + b"\x01" + b"\x80\x00\x00\x00")  # PADDING in longer encodings of type 0
    return cases


# ---- fuzz ------------------------------------------------------------------------------------------
def fuzz_payload(rng, max_len=1400):
    """A generated frame sequence of 1..max_len bytes; about half of them get a mutation."""
    out = b""
    target = int(rng.integers(1, max_len + 1))
    while len(out) < target:
        k = int(rng.integers(0, 12))
        if k == 0:
            out += bytes(int(rng.integers(1, 400)))
        elif k == 1:
            cnt = int(rng.integers(0, 6))
            body = b"".join(vi(int(rng.integers(0, 1 << 14))) for _ in range(2 * cnt))
            t = int(rng.choice([2, 3]))
            ecn = b"".join(vi(int(rng.integers(0, 1 << 20))) for _ in range(3)) if t == 3 else b""
            out += build(t, (int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 14)), cnt,
                             int(rng.integers(0, 64))), body + ecn)
        elif k == 2:
            n = int(rng.integers(0, 500))
            out += build(0x06, (int(rng.integers(0, 1 << 20)), n), rng.bytes(n))
        elif k in (3, 4):
            t = int(rng.integers(0x08, 0x10)) | 0x02
            n = int(rng.integers(0, 600))
            f = [int(rng.integers(0, 1 << 10))] + ([int(rng.integers(0, 1 << 40))] if t & 4 else []) + [n]
            out += build(t, f, rng.bytes(n))
        else:
            fs = sample_frames(w=int(rng.choice([1, 2, 4, 8])) if rng.random() < 0.3 else None)
            f = fs[int(rng.integers(0, len(fs)))]
            if 0x08 <= f[0] <= 0x0F and not f[0] & 0x02 and rng.random() < 0.8:
                continue  # a STREAM frame to the end swallows the rest: keep those rare
            out += f
    out = bytearray(out[:max_len])
    m = rng.random()
    if m < 0.2 and len(out) > 1:
        out = out[:int(rng.integers(1, len(out)))]                       # truncation
    elif m < 0.4:
        for _ in range(int(rng.integers(1, 9))):
            out[int(rng.integers(0, len(out)))] ^= 1 << int(rng.integers(0, 8))  # bit flips
    elif m < 0.55:
        for _ in range(int(rng.integers(1, 4))):                         # length-field edits
            out[int(rng.integers(0, len(out)))] = int(rng.choice([0x3F, 0x7F, 0xBF, 0xFF, 0x40]))
    elif m < 0.65:
        at = int(rng.integers(0, len(out)))                              # a stray byte moves what follows
        out = (out[:at] + bytes([int(rng.integers(0, 256))]) + out[at:])[:max_len]
    return bytes(out)


def fuzz_batch(seed, n):
    rng = np.random.default_rng(seed)
    return [fuzz_payload(rng) for _ in range(n)]


# ---- arenas ----------------------------------------------------------------------------------------
def lay_out(payloads, aligns=None, level=None, poison=None, gap=3):
    """Payloads as opened packets in one plaintext arena: a header of 1..40 bytes in front of each and a
    16-byte tag behind it (both 0xAA-filled: bytes that a read outside the payload would take for
    frames); payload i starts at an arena address = aligns[i] mod 16. Returns (arena, pkts)."""
    pkts = np.zeros(len(payloads), dtype=recv.PKT_DTYPE)
    chunks, off = [], 0
    for i, p in enumerate(payloads):
        po = 1 + (7 * i) % 40
        if aligns is not None:
            pad = (aligns[i] - (off + po)) % 16
            chunks.append(b"\xAA" * pad)
            off += pad
        fill = 0xAA if poison is None else poison
        blob = bytes([fill]) * po + bytes(p) + bytes([fill]) * 16
        pkts[i]["offset"], pkts[i]["len"], pkts[i]["payload_offset"] = off, len(blob), po
        pkts[i]["level"] = (i % 3) if level is None else level
        pkts[i]["dgram"] = i
        chunks.append(blob)
        off += len(blob)
        if gap:
            chunks.append(b"\x01" * gap)
            off += gap
    arena = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    return arena, pkts
