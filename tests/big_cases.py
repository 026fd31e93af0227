"""Shared by tests/test_big_cases_model.py (CPU) and
tests/test_gpu_over_4gib.py: expectations for batches whose wire, message
buffer or reply wire passes 2^31 and 2^32 bytes, where no Python model can be
run over the bytes.  Every expectation is the model's result for the same
streams laid out compactly, translated: shift_frames / shift_info move the
offsets that depend on where a stream lies in the wire, prepend_filler puts
one large single-frame stream in front of a batch.  The CPU file proves the
three against the models themselves at small sizes.  No test lives here."""
import functools

import numpy as np

import oracle
from cppserver_amd import layout
from cppserver_amd.layout import CB_RECEIVED, MSG, STREAM_SPAN, STREAM_STATE, WS_BINARY, frame_size
from tests import frames_cases as fc
from tests import messages_cases as mc
from tests import utf8_cases as uc

MARK31, MARK32 = 1 << 31, 1 << 32
MARKS = (MARK31, MARK32)          # 2^31 catches a sign extension, 2^32 a truncation
SENTINEL = 0xA5


# ------------------------------------------------------------- the translation
def _per_frame(stream_first, per_stream):
    """A per-stream value repeated for each of the stream's frames."""
    return np.repeat(np.asarray(per_stream, dtype=np.uint64), np.diff(np.asarray(stream_first).astype(np.int64)))


def _moved(compact_spans, real_spans):
    """Per stream, real offset - compact offset (mod 2^64)."""
    a = np.asarray(compact_spans, dtype=STREAM_SPAN)
    b = np.asarray(real_spans, dtype=STREAM_SPAN)
    assert len(a) == len(b) and np.array_equal(a["len"], b["len"]), "not the same streams"
    return b["off"] - a["off"]


def shift_frames(plan, compact_spans, real_spans):
    """layout.frame_plan's (frame_start, stream_first, spans_out, count) of
    streams laid out at compact_spans -> the plan of the same streams at
    real_spans: every stream's frame starts move by the difference of its two
    offsets; consumed, need, stream_first and count do not depend on where a
    stream lies."""
    fs, sf, spans_out, count = plan
    out = np.array(np.asarray(real_spans, dtype=STREAM_SPAN), copy=True)
    out["consumed"] = spans_out["consumed"]
    out["need"] = spans_out["need"]
    return (np.asarray(fs, dtype=np.uint64) + _per_frame(sf, _moved(compact_spans, real_spans)), np.array(sf, copy=True),
            out, np.array(count, copy=True))


def shift_info(info, stream_first, compact_spans, real_spans):
    """RECV_INFO of the compact layout's frames -> that of the real layout's:
    payload_off moves as the frame starts do, every other field stays."""
    out = np.array(info, copy=True)
    out["payload_off"] = out["payload_off"] + _per_frame(stream_first, _moved(compact_spans, real_spans))
    return out


def prepend_filler(msgs, count, L0, state=None):
    """The message table (msgs, count[, state]) of a batch -> that of the
    batch with one more stream in front, holding a single FIN binary frame of
    L0 payload bytes: its record first, every other record L0 bytes further
    into the dense buffer, one stream and one frame later."""
    first = np.zeros(1, dtype=MSG)
    first["off"], first["len"], first["stream"], first["first_frame"], first["nframes"] = 0, L0, 0, 0, 1
    first["kind"], first["opcode"] = CB_RECEIVED, WS_BINARY
    rest = np.array(np.asarray(msgs, dtype=MSG), copy=True)
    rest["off"] += np.uint64(L0)
    rest["stream"] += 1
    rest["first_frame"] += 1
    table = np.concatenate([first, rest])
    new_count = np.array([int(count[0]) + 1, int(count[1]) + L0], dtype=np.uint64)
    if state is None:
        return table, new_count
    head = np.zeros(1, dtype=STREAM_STATE)
    head["consumed"], head["opcode"] = 1, WS_BINARY
    return table, new_count, np.concatenate([head, np.asarray(state, dtype=STREAM_STATE)])


def prepend_filler_reply(reply_plan, reply_op, mask, L0):
    """layout.reply_plan's (reply_off, stream_reply, count) of a batch -> that
    of the batch with the filler stream in front: the filler's reply frame
    comes first, everything else moves by its size."""
    reply_off, stream_reply, rcount = reply_plan
    op = int(reply_op[CB_RECEIVED])
    op = layout.WS_FIN | WS_BINARY if op == layout.REPLY_SAME else op
    size0 = frame_size(op, mask, L0) if op else 0
    return (np.concatenate([[0], np.asarray(reply_off, dtype=np.uint64) + np.uint64(size0)]).astype(np.uint64),
            np.concatenate([[0], np.asarray(stream_reply, dtype=np.uint64) + np.uint64(size0)]).astype(np.uint64),
            np.array([int(rcount[0]) + size0, int(rcount[1]) + (1 if size0 else 0)], dtype=np.uint64))


def want_behind_prefix(prefix_len, tail):
    """uc.want of prefix + tail for a prefix that is valid UTF-8 and ends on a
    code point boundary: such a prefix adds its length (the decoder's state
    behind it is the initial one)."""
    return prefix_len + uc.want(tail)


# ------------------------------------------------------------ streams in a wire
def batch_spans(batch):
    """The spans of a messages_cases.Batch: its streams back to back from 0."""
    lens = np.array([sum(len(f) for f in s) for s in batch.streams], dtype=np.uint64)
    spans = np.zeros(batch.n_streams, dtype=STREAM_SPAN)
    spans["len"] = lens
    spans["off"] = np.cumsum(lens) - lens
    return spans


def place(data, spans, total, fill=SENTINEL):
    """A wire of `total` bytes of `fill` with the streams' bytes at their spans."""
    wire = np.full(total, fill, dtype=np.uint8)
    for d, s in zip(data, spans):
        assert int(s["len"]) == len(d)
        wire[int(s["off"]): int(s["off"]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    return wire


class Sparse:
    """Streams, each a list of whole frames and the bytes of a partial frame
    behind them, at chosen wire offsets (increasing, not overlapping).  The
    compact layout (fc.Wire, the streams back to back from 0) is what the
    models are run on."""

    def __init__(self, streams, offs):
        self.frames = [list(f) for f, _ in streams]
        self.tails = [bytes(t) for _, t in streams]
        self.data = [b"".join(f) + t for f, t in zip(self.frames, self.tails)]
        self.streams = self.data                      # (with spans and n_streams: what fc.check_against_oracle reads)
        self.n_streams = len(self.data)
        self.compact = fc.Wire(self.data, gaps=[0] * self.n_streams)
        self.spans = np.zeros(self.n_streams, dtype=STREAM_SPAN)
        self.spans["off"] = np.array([int(o) for o in offs], dtype=np.uint64)
        self.spans["len"] = self.compact.spans["len"]
        ends = [int(o) + len(d) for o, d in zip(offs, self.data)]
        assert all(int(o) >= e for o, e in zip(list(offs)[1:], ends)), "streams overlap"
        self.end = ends[-1] if ends else 0

    @functools.cached_property
    def model(self):
        """The models on the compact layout: dict of plan (layout.frame_plan),
        info, msgs, count, state, buf (the dense message bytes), lowered (each
        span's consumed as wsg_decode_streams leaves it), batch (the whole
        frames as a messages_cases.Batch, for the oracle's sessions).  The
        oracle's sessions are asked too (mc.check_model)."""
        w = self.compact
        plan = layout.frame_plan(w.wire, w.spans)
        fs, sf = plan[0], plan[1]
        rc, out, info = oracle.decode_batch(w.wire, fs)
        assert rc == 0
        msgs, count, state = layout.message_plan(info, sf, None, payload=out)
        buf = mc.dense(out, info, sf, state)
        batch = mc.Batch(self.frames)                 # the whole frames alone: what a session is fed
        assert batch.n == int(plan[3][0]) and np.array_equal(batch.stream_first, sf.astype(np.int32))
        b_msgs, b_count, b_state, b_buf, _, b_info = mc.check_model(batch)
        mc.same_fields(msgs, b_msgs, mc.MSG_FIELDS)   # nothing in them depends on the tails between the streams
        mc.same_fields(state, b_state, ["consumed", "opcode"])
        assert [int(x) for x in count] == [int(x) for x in b_count] and np.array_equal(buf, b_buf)
        mc.same_fields(info, shift_info(b_info, sf, batch_spans(batch), _whole(w.spans, plan)),
                       mc.INFO_FIELDS)
        lowered = np.array(plan[2]["consumed"], copy=True)
        for j in range(self.n_streams):
            first, nj, used = int(sf[j]), int(sf[j + 1]) - int(sf[j]), int(state["consumed"][j])
            if used < nj:                             # the first tail frame's start in the stream
                lowered[j] = int(fs[first + used]) - int(w.spans["off"][j])
        return dict(plan=plan, info=info, msgs=msgs, count=count, state=state, buf=buf, lowered=lowered, batch=batch)

    def want_frames(self):
        """frame_plan of the real layout."""
        return shift_frames(self.model["plan"], self.compact.spans, self.spans)

    def want_info(self):
        return shift_info(self.model["info"], self.model["plan"][1], self.compact.spans, self.spans)


def _whole(spans, plan):
    """spans cut down to their whole frames (len = consumed)."""
    out = np.array(spans, copy=True)
    out["len"] = plan[2]["consumed"]
    return out


# ----------------------------------------------- section 1: streams at the marks
# (form, masked): the six header forms, 2, 6, 4, 8, 10 and 14 bytes
HEADER_FORMS = [(0, False), (0, True), (126, False), (126, True), (127, False), (127, True)]
TOP = MARK32 + (1 << 30) + 13                 # the last stream of every case
SPARSE_WIRE = MARK32 + (1 << 30) + (1 << 20)  # bytes of the sparse wire
MEET = MARK32 - 1024                          # one stream ends here and the next begins here


def header_bytes(form, masked):
    return {0: 2, 126: 4, 127: 10}[form] + (4 if masked else 0)


def forced_frame(b0, payload, key=None, form=None):
    """mc.raw_frame with the length form forced (fc.header)."""
    payload = bytes(payload)
    if key is None:
        return fc.header(b0, len(payload), None, form) + payload
    kb = np.frombuffer(int(key).to_bytes(4, "little") * (len(payload) // 4 + 1), dtype=np.uint8)[: len(payload)]
    return fc.header(b0, len(payload), key, form) + (np.frombuffer(payload, dtype=np.uint8) ^ kb).tobytes()


def straddler(rng, mark, form, masked, s, misalign, payload_len, lead=0, open_tail=False):
    """((frames, tail), offset): a filler frame, the frame under test X, a
    2-byte frame, then one byte of a header (need 2); X's header starts at
    mark - lead - s, and the stream at an offset that is `misalign` mod 16.
    open_tail: a whole non-FIN frame behind the 2-byte frame, which
    wsg_decode_streams lowers consumed to."""
    key = int(rng.integers(1, 2**32)) if masked else None
    x = forced_frame(int(rng.choice([0x81, 0x82])), rng.integers(0, 256, payload_len, dtype=np.uint8).tobytes(), key, form)
    assert len(x) == header_bytes(form, masked) + payload_len
    at = mark - lead - s                                   # X's first header byte
    flen = 304 + (at - 8 - misalign) % 16                  # a masked 126-form filler: 8 header bytes
    filler = mc.raw_frame(0x82, rng.integers(0, 256, flen, dtype=np.uint8).tobytes(), key=int(rng.integers(1, 2**32)))
    off = at - len(filler)
    assert len(filler) == 8 + flen and off % 16 == misalign
    frames = [filler, x, b"\x81\x00"]
    if open_tail:
        frames.append(mc.raw_frame(0x01, b"open", key=int(rng.integers(1, 2**32))))
    return (frames, b"\x81"), off


@functools.lru_cache(maxsize=None)
def sparse_cases():
    """name -> Sparse: for every header form and every split s of X's header
    across the marks (s = 0: the header at the mark; s = its length: the
    payload's first byte at the mark) one batch of, in wire order: a clean
    stream at offset 3, a stream straddling 2^31, a stream that ends at
    2^32 - 1024, one that begins there, a stream straddling 2^32, and a
    stream at 2^32 + 2^30 + 13.  X carries 200 bytes (120 in the 7-bit form,
    which cannot announce 200); per mark one more case whose X is a masked
    127-form frame of 70 000 bytes that begins below the mark and ends above
    it.  The streams' start misalignment runs over 0..15 across the cases,
    and one straddler per mark and form has a whole non-FIN frame behind its
    last FIN frame."""
    quirks = mc.quirk_streams()
    names = [k for k in sorted(quirks) if quirks[k]]
    cases = {}

    def add(name, rng, a, b, meet=True):
        (sa, off_a), (sb, off_b) = a, b
        streams, offs = [(quirks[names[len(cases) % len(names)]], b"")], [3]
        streams.append(sa)
        offs.append(off_a)
        if meet:
            before = [mc.raw_frame(0x82, rng.integers(0, 256, 77, dtype=np.uint8).tobytes(),
                                   key=int(rng.integers(1, 2**32))), mc.raw_frame(0x01, b"no fin")]
            streams += [(before, b""), (mc.random_frames(rng, 3, 150), b"\x82\x7e")]
            offs += [MEET - sum(len(f) for f in before), MEET]
        streams += [sb, (mc.random_frames(rng, 4, 300), b"\x88")]
        offs += [off_b, TOP]
        cases[name] = Sparse(streams, offs)

    for form, masked in HEADER_FORMS:
        hdr = header_bytes(form, masked)
        size = 120 if form == 0 else 200
        for s in range(hdr + 1):
            rng = np.random.default_rng(1000 * hdr + s)
            i = len(cases)
            add("hdr%d_s%d" % (hdr, s), rng,
                straddler(rng, MARK31, form, masked, s, (7 * i) % 16, size, open_tail=s == 1),      # 7 is odd: both
                straddler(rng, MARK32, form, masked, s, (7 * i + 5) % 16, size, open_tail=s == 2))  # run over 0..15
    # (the jump streams begin below 2^32 - 1024: no pair of streams meets there in these two)
    for i, lead in enumerate((33333, 69990)):               # X's payload begins lead - 14 bytes below the mark
        rng = np.random.default_rng(77 + i)
        add("jump_lead%d" % lead, rng,
            straddler(rng, MARK31, 127, True, 0, 3 + i, 70000, lead=lead, open_tail=i == 0),
            straddler(rng, MARK32, 127, True, 0, 11 + i, 70000, lead=lead, open_tail=i == 1), meet=False)
    return cases


# --------------------------------------- section 2: a filler in front of a batch
FILLER_KEY = 0x5EC7A11D
DENSE_WIRE = MARK32 + (1 << 20)   # bytes of the dense wire


def dense_runs():
    """name -> (streams, target): about a dozen small streams (lists of whole
    frames) to lay out behind the filler, and the offset in their own dense
    message buffer that the filler's length brings to 2^32:
    (i) byte 5 of a single-frame text message of 40 bytes; (ii) the boundary
    between fragments 2 and 3 of a 4-fragment message; (iii) between the two
    status bytes of a close message whose body comes in frames of one byte
    and the rest; (iv) a message's first byte, an empty message in front."""
    out = {}
    for name in ("text", "fragments", "close", "first_byte"):
        rng = np.random.default_rng({"text": 21, "fragments": 22, "close": 23, "first_byte": 24}[name])
        key = lambda: int(rng.integers(1, 2**32))   # noqa: E731
        lead = [mc.random_frames(rng, int(rng.integers(1, 5)), 120) for _ in range(2)]
        if name == "text":
            special = [mc.raw_frame(0x81, uc.mixed_text(rng, 40), key=key())]
            inside = 5
        elif name == "fragments":
            sizes = [33, 18, 27, 9]
            special = [mc.raw_frame((0x02 if i == 0 else 0) | (0x80 if i == 3 else 0),
                                    rng.integers(0, 256, n, dtype=np.uint8).tobytes(), key=key())
                       for i, n in enumerate(sizes)]
            inside = sizes[0] + sizes[1]
        elif name == "close":
            special = [mc.raw_frame(0x08, b"\x03", key=key()), mc.raw_frame(0x80, b"\xe9going away", key=key())]
            inside = 1
        else:
            special = [mc.raw_frame(0x81, b"", key=key()), mc.raw_frame(0x82, bytes(range(50)), key=key())]
            inside = 0
        ahead = [mc.raw_frame(0x82, rng.integers(0, 256, 61, dtype=np.uint8).tobytes(), key=key())]
        rest = [mc.random_frames(rng, int(rng.integers(0, 6)), 200) for _ in range(8)]
        rest.append([mc.raw_frame(0x89, b"ping", key=key()), mc.raw_frame(0x01, b"tail")])
        streams = lead + [ahead + special] + rest
        # the special message's first byte in the streams' own dense buffer
        batch = mc.Batch(streams)
        msgs, _, _, _, _, info = mc.check_model(batch)
        first_frame = int(batch.stream_first[2]) + 1
        (m,) = [r for r in msgs if int(r["first_frame"]) == first_frame + (1 if name == "first_byte" else 0)]
        start = int(m["off"]) - (2 if int(m["kind"]) == layout.CB_CLOSE and name == "close" else 0)
        out[name] = (streams, start + inside)
    return out
