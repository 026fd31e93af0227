"""Shared by tests/test_frames_model.py (CPU) and tests/test_gpu_frames.py:
streams of raw bytes for wsg_frame_streams, a framer built from the oracle
alone, and batches of streams laid out in one wire.  No test lives here."""
import numpy as np

import oracle
from cppserver_amd import layout
from tests import kat
from tests import messages_cases as mc

U64_MAX = 2**64 - 1
LENGTHS = [0, 1, 125, 126, 127, 65535, 65536]


def oracle_walk(data):
    """Frame starts and bytes in whole frames of one stream, from
    oracle.Session.required() alone (as test_oracle.py's
    test_required_receive_frame_size_walk feeds a session): feed what it asks
    for, stop when fewer bytes remain than it asks for.  Not for a header
    that announces more bytes than a vector can hold (the session reserves
    the frame's size when the header is complete)."""
    data = bytes(data)
    rx = oracle.Session()
    at, starts = 0, []
    while True:
        rx.prepare_receive(b"")        # a finished frame is reset by the next call
        start = at
        while True:
            r = rx.required()
            if r == 0:
                break
            if len(data) - at < r:
                return starts, start
            rx.prepare_receive(data[at: at + r])
            at += r
        starts.append(start)


def header(b0, length, key=None, form=None):
    """A header announcing `length` payload bytes; form 126 / 127 forces the
    extended form whatever the length."""
    mbit = 0x80 if key is not None else 0
    if form is None:
        form = 0 if length < 126 else 126 if length < 65536 else 127
    if form == 0:
        h = bytes([b0, mbit | length])
    elif form == 126:
        h = bytes([b0, mbit | 126]) + length.to_bytes(2, "big")
    else:
        h = bytes([b0, mbit | 127]) + length.to_bytes(8, "big")
    return h + (int(key).to_bytes(4, "little") if key is not None else b"")


def cut_cases():
    """name -> (stream bytes, whole frames, consumed, need): a lead frame, then
    a frame of every length of LENGTHS, masked and unmasked, cut after every
    header byte, at the header's end, in the middle of the payload, one byte
    short, and not at all."""
    rng = np.random.default_rng(11)
    lead = mc.raw_frame(0x81, b"lead", key=0x01020304)
    cases = {}
    for n in LENGTHS:
        for key in (None, 0xA1B2C3D4):
            payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            frame = mc.raw_frame(0x82, payload, key=key)
            hdr = len(frame) - n
            cuts = sorted(set(list(range(hdr + 1)) + [hdr + n // 2, len(frame) - 1, len(frame)]))
            for c in cuts:
                if c == len(frame):
                    want = (2, len(lead) + len(frame), 0)
                elif c == 0:
                    want = (1, len(lead), 0)
                elif c == 1:
                    want = (1, len(lead), 2)
                elif c < hdr:
                    want = (1, len(lead), hdr)
                else:
                    want = (1, len(lead), len(frame))
                cases["len%d_%s_cut%d" % (n, "masked" if key is not None else "plain", c)] = (lead + frame[:c],) + want
    return cases


def huge_cases():
    """The 127 form with a length no wire holds: a frame that never completes."""
    lead = mc.raw_frame(0x82, b"x" * 7)
    cases = {}
    for length in (2**63, U64_MAX):
        for key in (None, 0x0BADF00D):
            h = header(0x82, length, key=key, form=127)
            tail = h + b"some payload bytes"
            need = min(len(h) + length, U64_MAX)
            cases["huge_%x_%s" % (length, "masked" if key is not None else "plain")] = (lead + tail, 1, len(lead), need)
    return cases


def tiny_cases():
    return {"empty": (b"", 0, 0, 0), "one_byte": (b"\x81", 0, 0, 2), "one_frame_empty": (b"\x81\x00", 1, 2, 0),
            "two_then_byte": (b"\x81\x00\x81\x00\xff", 2, 4, 2)}


def clean_streams():
    """name -> stream bytes of whole frames: the quirk streams of the message
    tests and the KAT decode streams."""
    out = {"quirk_" + k: b"".join(v) for k, v in mc.quirk_streams().items()}
    for v in kat.load()["decode"]:
        out["kat_" + v["name"]] = b"".join(bytes.fromhex(c) for c in v["chunks"])
    return out


def model_streams():
    """name -> (bytes, oracle-walkable) of every model case."""
    out = {k: (v, True) for k, v in clean_streams().items()}
    out.update({k: (v[0], True) for k, v in cut_cases().items()})
    out.update({k: (v[0], True) for k, v in tiny_cases().items()})
    out.update({k: (v[0], False) for k, v in huge_cases().items()})
    return out


class Wire:
    """Streams (bytes) laid out in one wire in order: `gaps[j]` junk bytes in
    front of stream j (default: stream j starts j % 5 bytes behind stream
    j - 1), 64 junk bytes behind the last."""

    def __init__(self, streams, gaps=None, lead=0, seed=5):
        rng = np.random.default_rng(seed)
        self.streams = [bytes(s) for s in streams]
        ns = len(self.streams)
        gaps = [j % 5 for j in range(ns)] if gaps is None else list(gaps)
        lens = np.array([len(s) for s in self.streams], dtype=np.uint64)
        g = np.array(gaps, dtype=np.uint64)
        ends = np.cumsum(lens + g) + np.uint64(lead)
        self.spans = np.zeros(ns, dtype=layout.STREAM_SPAN)
        self.spans["off"] = ends - lens
        self.spans["len"] = lens
        total = (int(ends[-1]) if ns else lead) + 64
        self.wire = rng.integers(0, 256, total, dtype=np.uint8)
        for s, off in zip(self.streams, self.spans["off"]):
            self.wire[int(off): int(off) + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.n_streams = ns


def check_against_oracle(w, fs, sf, spans_out, which=None):
    """A plan (frame_plan's, or the device's) against the oracle walk of each
    stream of Wire w (only streams `which`, by index, when given)."""
    for j in (range(w.n_streams) if which is None else which):
        starts, consumed = oracle_walk(w.streams[j])
        off = int(w.spans["off"][j])
        got = [int(x) - off for x in fs[int(sf[j]): int(sf[j + 1])]]
        assert got == starts, "stream %d" % j
        assert int(spans_out["consumed"][j]) == consumed, "stream %d" % j
