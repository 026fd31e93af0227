"""Shared by tests/test_protocol_model.py (CPU) and tests/test_gpu_protocol.py:
the expected values of wsg_check_protocol and the batches they are asked of.

judge() and loop() are a plain sequential statement of the rule table in
include/wsg_capi.h (one frame, then one stream after the other), written
without layout.protocol_plan and without csrc/wsg_proto.h.  No test lives
here."""
import numpy as np

import cppserver_amd as ca
from cppserver_amd.layout import RECV_INFO

U64_MAX = 2 ** 64 - 1
TEXT, BINARY, CONT, CLOSE, PING, PONG = 0x1, 0x2, 0x0, 0x8, 0x9, 0xA
FIN = 0x80
ANY, SERVER, CLIENT = 0, 1, 2
NONE = (0xFF, 0xFFFF, 0xFFFFFFFF)   # a verdict of all 0xFF: (code, status, frame)
CLOSE_STATUSES = [0, 999] + list(range(1000, 1017)) + [1100, 2000, 2999, 3000, 3999, 4000, 4999, 5000, 65535]
LEGAL = set(range(1000, 1004)) | set(range(1007, 1015)) | set(range(3000, 5000))


# ------------------------------------------------------------------ the rule
def judge(rec, wire, is_open, nbytes, role, max_message):
    """One frame: (code or 0, status or 0, open after, bytes after)."""
    op, fin, masked = int(rec["opcode"]), bool(rec["fin"]), bool(rec["masked"])
    length, rsv, error = int(rec["len"]), int(rec["b0"]) & 0x70, int(rec["error"])
    control = bool(op & 8)
    reserved = 3 <= op <= 7 or 0xB <= op <= 0xF
    if error or control or reserved:
        open_after, bytes_after = is_open, nbytes
    elif op in (1, 2):
        open_after, bytes_after = not fin, length
    else:
        open_after, bytes_after = not fin, min(nbytes + length, U64_MAX)
    carried = None
    if op == 8 and length >= 2:
        at = int(rec["payload_off"])
        b = [int(wire[at]), int(wire[at + 1])] if at + 2 <= len(wire) else None
        if b is None:
            carried = 0
        else:
            if masked:
                key = int(rec["key"])
                b = [b[0] ^ (key & 0xFF), b[1] ^ ((key >> 8) & 0xFF)]
            carried = b[0] << 8 | b[1]
    code, status = 0, 0
    if error:
        code = 2
    elif rsv:
        code = 3
    elif reserved:
        code = 4
    elif (role == SERVER and not masked) or (role == CLIENT and masked):
        code = 5
    elif control and not fin:
        code = 6
    elif control and length > 125:
        code = 7
    elif op == 0 and not is_open:
        code = 8
    elif op in (1, 2) and is_open:
        code = 9
    elif op == 8 and length == 1:
        code = 10
    elif op == 8 and length >= 2 and carried not in LEGAL:
        code = 11
    elif op in (0, 1, 2) and max_message != 0 and bytes_after > max_message:
        code = 12
    elif op == 8:
        code = 1
    if code == 1:
        status = 1005 if length == 0 else carried
    elif code == 12:
        status = 1009
    elif code:
        status = 1002
    return code, status, open_after, bytes_after


def loop(info, stream_first, proto_in, role, max_message, wire, consumed=None):
    """Every stream walked frame by frame.  Returns (verdicts, states,
    result): per stream (code, status, frame) or NONE; (bytes, open) out;
    [violating streams, the lowest or U64_MAX, streams closed cleanly]."""
    ns = len(stream_first) - 1
    verdicts, states = [], []
    for j in range(ns):
        lo, hi = int(stream_first[j]), int(stream_first[j + 1])
        nbytes, is_open = (int(proto_in[j][0]), bool(proto_in[j][1])) if proto_in is not None else (0, False)
        stop = hi if consumed is None else lo + int(consumed[j])
        kept = (nbytes, int(is_open))
        verdict = NONE
        for i in range(lo, hi):
            code, status, is_open, nbytes = judge(info[i], wire, is_open, nbytes, role, max_message)
            if code and verdict is NONE:
                verdict = (code, status, i)
            if i + 1 == stop:
                kept = (nbytes, int(is_open))
        verdicts.append(verdict)
        states.append(kept)
    bad = [j for j, v in enumerate(verdicts) if v is not NONE and v[0] >= 2]
    closed = sum(1 for v in verdicts if v[0] == 1)
    return verdicts, states, [len(bad), bad[0] if bad else U64_MAX, closed]


# ------------------------------------------------------------------ frames and batches
def frame(b0, payload=b"", key=None):
    """One frame with first byte b0 and exactly this payload; masked with the
    little-endian key when one is given."""
    payload = bytes(payload)
    n = len(payload)
    mbit = 0x80 if key is not None else 0
    if n < 126:
        hdr = bytes([b0, mbit | n])
    elif n < 65536:
        hdr = bytes([b0, mbit | 126]) + n.to_bytes(2, "big")
    else:
        hdr = bytes([b0, mbit | 127]) + n.to_bytes(8, "big")
    if key is None:
        return hdr + payload
    kb = int(key).to_bytes(4, "little")
    pad = np.frombuffer(kb * (n // 4 + 1), dtype=np.uint8)[:n]
    return hdr + kb + (np.frombuffer(payload, dtype=np.uint8) ^ pad).tobytes()


def close(status=None, reason=b"", key=None, b0=FIN | CLOSE):
    body = b"" if status is None else int(status).to_bytes(2, "big") + bytes(reason)
    return frame(b0, body, key)


class Batch:
    """Streams (lists of frames, each a frame's bytes; the batch's last frame
    may be cut short) laid out as the decode calls take them, with the
    RECV_INFO records the decode leaves: wsg_header_unpack's fields, or, for a
    frame that runs past the wire, the error record (payload_off = the frame's
    start, error = WSG_ETRUNC, everything else 0)."""

    def __init__(self, streams):
        self.streams = [list(s) for s in streams]
        frames = [f for s in self.streams for f in s]
        self.n, self.n_streams = len(frames), len(self.streams)
        sizes = [len(f) for f in frames]
        self.fs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if self.n else \
            np.zeros(0, dtype=np.uint64)
        self.wire = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
        self.stream_first = np.concatenate([[0], np.cumsum([len(s) for s in self.streams])]).astype(np.int32)
        self.info = np.zeros(self.n, dtype=RECV_INFO)
        cache = {}
        for i, f in enumerate(frames):
            r = cache.get(f)
            if r is None:
                rc, r = ca.header_unpack(f[:14])
                whole = rc == 0 and int(r["hdr_len"]) + int(r["len"]) == len(f)
                assert whole or i == self.n - 1, "only the last frame may be cut short"
                if not whole:
                    r = np.zeros((), dtype=RECV_INFO)
                    r["error"] = ca.WSG_ETRUNC
                cache[f] = r = r.copy()
            self.info[i] = r
            self.info["payload_off"][i] = int(self.fs[i]) + int(r["hdr_len"])

    def expect(self, role=ANY, max_message=0, proto_in=None, consumed=None):
        return loop(self.info, self.stream_first, proto_in, role, max_message, self.wire, consumed)


# ------------------------------------------------------------------ cases
EVERY_CODE_LIMIT = 100


def every_code_streams():
    """name -> frames: one stream per code 1-12 (judged as a server with
    max_message = EVERY_CODE_LIMIT; every frame but those of `mask` is
    masked) and three clean ones.  `frame_error` ends in a frame cut short and
    must be the batch's last stream."""
    k = 0x1F2E3D4C
    return {
        "clean_text": [frame(FIN | TEXT, b"hello", k)],
        "closed": [frame(FIN | BINARY, b"x" * 10, k), close(1000, b"bye", k)],
        "rsv": [frame(FIN | TEXT | 0x40, b"compressed?", k)],
        "opcode": [frame(FIN | 0x3, b"", k), frame(FIN | TEXT, b"after", k)],
        "mask": [frame(FIN | TEXT, b"plain")],
        "clean_fragments": [frame(TEXT, b"a" * 40, k), frame(FIN | PING, b"p", k), frame(CONT, b"b" * 40, k),
                            frame(FIN | CONT, b"c" * 20, k)],
        "ctrl_fragment": [frame(PING, b"", k)],
        "ctrl_long": [frame(FIN | PING, b"p" * 126, k)],
        "cont": [frame(FIN | CONT, b"nothing to continue", k)],
        "data": [frame(TEXT, b"open", k), frame(FIN | BINARY, b"interloper", k)],
        "close_len": [frame(FIN | CLOSE, b"\x03", k)],
        "close_code": [close(1005, b"", k)],
        "too_big": [frame(BINARY, b"z" * 60, k), frame(CONT, b"z" * 40, k), frame(FIN | CONT, b"z", k)],
        "clean_empty": [],
        "frame_error": [frame(FIN | PONG, b"", k), frame(FIN | BINARY, b"q" * 30, k)[:9]],
    }


EVERY_CODE_WANT = {"clean_text": 0xFF, "closed": 1, "rsv": 3, "opcode": 4, "mask": 5, "clean_fragments": 0xFF,
                   "ctrl_fragment": 6, "ctrl_long": 7, "cont": 8, "data": 9, "close_len": 10, "close_code": 11,
                   "too_big": 12, "clean_empty": 0xFF, "frame_error": 2}


def close_status_streams():
    """One stream per (status, masked): a close frame carrying it and a reason."""
    out = []
    for s in CLOSE_STATUSES:
        out.append([close(s, b"why", key=0xC0FFEE00 + s)])
        out.append([close(s, b"why")])
    return out


def fuzz(seed):
    """(streams, role, max_message, proto_in) of one fuzz batch: 1-40 streams
    of 0-60 frames (short streams more likely than long ones, so that a batch
    keeps some clean), each frame a valid next frame of its stream with
    probability about 0.9 and one of the violations otherwise."""
    rng = np.random.default_rng(seed)
    role = int(rng.integers(0, 3))
    limit = int(rng.choice([0, 0, 50, 200, 1000]))
    n_streams = min(int(1 + 40 * rng.random() ** 0.5), 40)   # few-stream batches rarer: one stream cannot be both kinds
    streams, proto_in = [], []

    def key():
        """The mask a valid frame carries under the role."""
        masked = role == SERVER or (role == ANY and rng.random() < 0.5)
        return int(rng.integers(1, 2 ** 32)) if masked else None

    def wrong_key():
        return None if role == SERVER else int(rng.integers(1, 2 ** 32))

    for _ in range(n_streams):
        count = int(60 * rng.random() ** 3 + rng.random())   # 0..60, half of them below 8
        is_open, nbytes = bool(rng.random() < 0.2), 0
        if is_open:
            nbytes = int(rng.integers(0, 40))
        proto_in.append((nbytes, int(is_open)))
        frames = []
        for _ in range(count):
            room = (limit - nbytes if is_open else limit) if limit else 300
            size = int(rng.integers(0, max(min(room, 300), 0) + 1))
            body = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            if rng.random() < 0.9:
                pick = rng.random()
                if pick < 0.2:
                    f = frame(FIN | int(rng.choice([PING, PONG])), body[:125], key())
                elif pick < 0.24:
                    f = close(int(rng.choice([1000, 1001, 1003, 1011, 3000, 4999])), body[:20], key()) \
                        if rng.random() < 0.7 else close(None, key=key())
                else:
                    fin = bool(rng.random() < 0.5)
                    op = CONT if is_open else int(rng.choice([TEXT, BINARY]))
                    f = frame((FIN if fin else 0) | op, body, key())
                    nbytes = nbytes + size if is_open else size
                    is_open = not fin
            else:
                bad = int(rng.integers(0, 10))
                if bad == 0:
                    f = frame(FIN | BINARY | int(rng.choice([0x10, 0x20, 0x40, 0x70])), body, key())
                elif bad == 1:
                    f = frame(FIN | int(rng.choice([3, 4, 5, 6, 7, 0xB, 0xC, 0xD, 0xE, 0xF])), body[:100], key())
                elif bad == 2 and role != ANY:
                    f = frame(FIN | PING, body[:100], wrong_key())
                elif bad == 3:
                    f = frame(int(rng.choice([PING, PONG, CLOSE])), body[:100], key())
                elif bad == 4:
                    f = frame(FIN | PING, bytes(int(rng.integers(126, 400))), key())
                elif bad == 5:
                    f = frame(FIN | (int(rng.choice([TEXT, BINARY])) if is_open else CONT), body, key())
                elif bad == 6:
                    f = frame(FIN | CLOSE, b"\x03", key())
                elif bad == 7:
                    f = close(int(rng.choice([0, 999, 1004, 1005, 1006, 1015, 2999, 5000, 65535])), b"", key())
                elif limit:
                    over = bytes(limit + 1)
                    f = frame(FIN | (CONT if is_open else BINARY), over, key())
                else:
                    f = frame(FIN | TEXT | 0x40, body, key())
            frames.append(f)
        streams.append(frames)
    return streams, role, limit, proto_in
