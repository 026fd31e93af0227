"""Shared by tests/test_messages_model.py (CPU) and tests/test_gpu_messages.py:
batches of streams for wsg_decode_messages and the checks of a result against
the oracle's sessions.  No test lives here."""
import numpy as np

import cppserver_amd as ca
import oracle
from cppserver_amd import layout
from tests import kat
from tests.test_gpu_rx_batch import OPCODES

MSG_FIELDS = ["off", "len", "stream", "first_frame", "nframes", "status", "kind", "opcode"]
INFO_FIELDS = ["payload_off", "len", "key", "opcode", "fin", "masked", "hdr_len", "b0", "error"]


def raw_frame(b0, payload=b"", key=None):
    """One frame with first byte b0 and exactly this payload (no status
    prefix, whatever the opcode); masked with the little-endian key if given."""
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


def sent(frames, key=0x0A0B0C0D):
    """Frames [(opcode byte, mask, payload[, status])] as one oracle session
    sends them (PrepareSendFrame, its status prefix included)."""
    enc = oracle.Session(key)
    return [enc.prepare_send(f[0], f[1], f[2], f[3] if len(f) > 3 else 0) for f in frames]


def random_frames(rng, n, max_len, masked_p=0.7):
    """n frames as tests/test_gpu_rx_batch.py:_stream builds them."""
    enc = oracle.Session()
    out = []
    for _ in range(n):
        op = int(rng.choice(OPCODES))
        mask = bool(rng.random() < masked_p)
        status = int(rng.integers(-3, 70000)) if rng.random() < 0.3 else 0
        size = int(rng.choice([0, 1, 2, 125, 126, 127, 65535, 65536]) if rng.random() < 0.2 and max_len > 65536
                   else rng.integers(0, max_len))
        enc.set_send_key(int(rng.integers(0, 2**32)))
        out.append(enc.prepare_send(op, mask, rng.integers(0, 256, size, dtype=np.uint8).tobytes(), status))
    return out


def kat_stream(name):
    (v,) = [v for v in kat.load()["decode"] if v["name"] == name]
    return [bytes.fromhex(c) for c in v["chunks"]], kat.events_of(v)


def quirk_streams():
    """name -> list of frames (each a whole frame's bytes), the fragment and
    quirk cases of the reference's message logic (ws.cpp:399-452)."""
    text = 0x01
    return {
        "rfc_fragmented_hello": kat_stream("rfc_fragmented_hello")[0],
        "q5_continuation_concat": kat_stream("q5_continuation_concat")[0],
        # 0x80 after a finished text message is another text message
        "continuation_after_fin": sent([(text, True, b"hel"), (0x00, True, b"lo "), (0x80, True, b"world"),
                                        (0x80, True, b"again")]),
        # the control frame's payload lands in the text buffer and its opcode sticks
        "ping_inside_text": sent([(text, True, b"ab"), (0x89, True, b"pp"), (0x80, True, b"cd"),
                                  (0x81, True, b"after")]),
        "close_one_byte": [raw_frame(0x88, b"\x03", key=0x11223344)],
        "close_empty": [raw_frame(0x88, b"")],
        "close_status_text": sent([(0x88, True, b"bye", 1001)]),
        # the two status bytes in different frames, empty frames in between
        "close_status_split": [raw_frame(0x08, b"\x03", key=0xA1B2C3D4), raw_frame(0x00, b""),
                               raw_frame(0x00, b"", key=7), raw_frame(0x80, b"\xe9gone", key=0x01020304)],
        "unknown_opcode_3": [raw_frame(0x83, b"zzz", key=5), raw_frame(0x80, b"q"), raw_frame(0x81, b"ok", key=9)],
        "tail_only": sent([(text, True, b"abc"), (0x00, False, b"def")]),
        "empty": [],
        "fin_then_tail": sent([(0x82, True, bytes(range(200))), (0x02, True, b"open"), (0x00, True, b"...")]),
        "pong_rsv": [raw_frame(0xCA, b"rsv bits kept out of the opcode", key=0xDEADBEEF)],
    }


class Batch:
    """Streams (lists of whole frames) laid out as wsg_decode_messages takes
    them: the wire, the frame starts, stream_first."""

    def __init__(self, streams):
        self.streams = [list(s) for s in streams]
        frames = [f for s in self.streams for f in s]
        sizes = np.array([len(f) for f in frames], dtype=np.uint64)
        self.fs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if len(frames) else \
            np.zeros(0, dtype=np.uint64)
        self.wire = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
        self.stream_first = np.concatenate([[0], np.cumsum([len(s) for s in self.streams])]).astype(np.int32)
        for f, s in zip(frames, self.fs):   # the framing is the host framer's (header_unpack)
            rc, r = ca.header_unpack(f[:14])
            assert rc == 0 and int(r["hdr_len"]) + int(r["len"]) == len(f), "not one whole frame"
        self.n = len(frames)
        self.n_streams = len(self.streams)

    def oracle_decode(self):
        rc, out, info = oracle.decode_batch(self.wire, self.fs)
        assert rc == 0
        return out, info


def dense(out, info, stream_first, state):
    """The message buffer: the unmasked payloads of every consumed frame, back to back."""
    parts = []
    for j in range(len(stream_first) - 1):
        lo = int(stream_first[j])
        for i in range(lo, lo + int(state["consumed"][j])):
            parts.append(out[int(info["payload_off"][i]):][: int(info["len"][i])])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def events_by_stream(msgs, msg_bytes, n_streams):
    """Per stream, its records that fire a callback, as the oracle's events."""
    msg_bytes = np.asarray(msg_bytes)
    ev = [[] for _ in range(n_streams)]
    for m in msgs:
        if int(m["kind"]) != 0:
            ev[int(m["stream"])].append((int(m["kind"]), msg_bytes[int(m["off"]):][: int(m["len"])].tobytes(),
                                         int(m["status"])))
    return ev


def records_events(msgs, msg_bytes, j):
    n = max(j, int(msgs["stream"].max()) if len(msgs) else 0) + 1
    return events_by_stream(msgs, msg_bytes, n)[j]


def check_events(batch, msgs, buf, new_state, info, state=None):
    """Records + bytes against one oracle session per stream fed the stream's
    consumed frames (seeded with the state's opcode)."""
    ev = events_by_stream(msgs, buf, batch.n_streams)
    for j, frames in enumerate(batch.streams):
        consumed = int(new_state["consumed"][j])
        assert consumed <= len(frames)
        ref = oracle.Session()
        if state is not None and int(state["opcode"][j]):   # put the session's _ws_opcode where the seed says
            ref.prepare_receive(raw_frame(int(state["opcode"][j]), b""))
        assert ev[j] == session_events(frames[:consumed], ref), "stream %d" % j
        # the tail holds no FIN frame
        assert not any(info["fin"][int(batch.stream_first[j]) + consumed: int(batch.stream_first[j + 1])])


def session_events(frames, session=None):
    s = session or oracle.Session()
    s.prepare_receive(b"".join(frames))
    return s.events()


def check_model(batch, state=None):
    """message_plan over the oracle's RECV_INFO against one oracle session
    per stream; returns (msgs, count, new_state, dense bytes, out, info)."""
    out, info = batch.oracle_decode()
    msgs, count, new_state = layout.message_plan(info, batch.stream_first, state, payload=out)
    buf = dense(out, info, batch.stream_first, new_state)
    assert int(count[0]) == len(msgs) and int(count[1]) == len(buf)
    check_events(batch, msgs, buf, new_state, info, state)
    return msgs, count, new_state, buf, out, info


def same_fields(got, want, fields):
    for f in fields:
        assert np.array_equal(got[f], want[f]), f
