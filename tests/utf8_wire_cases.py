"""Shared by tests/test_utf8_wire_model.py (CPU), tests/test_gpu_utf8_wire.py
and tests/test_gpu_validated_reply.py: batches for wsg_check_utf8_wire, the
UTF-8 check that reads the masked, fragmented wire.  Case builders only: the
expected values are layout.utf8_wire_plan's, held against Python's strict
decoder over what the oracle's sessions deliver (check_case).  No test lives
here."""
import numpy as np

import cppserver_amd as ca
import oracle
from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import messages_cases as mc
from tests import reply_cases as rc
from tests import utf8_cases as uc

TEXT, BINARY, CLOSE, PING, CONT, FIN = 0x1, 0x2, 0x8, 0x9, 0x0, 0x80
DEFAULT = layout.UTF8_TEXT | layout.UTF8_CLOSE
WHICH = (DEFAULT, layout.UTF8_EVERY)
ALL_WHICH = (0, layout.UTF8_TEXT, layout.UTF8_CLOSE, layout.UTF8_EVERY, DEFAULT)
frame = mc.raw_frame

# 2-, 3- and 4-byte sequences: valid ones at the ends of their ranges, and the
# overlong / surrogate / > U+10FFFF forms, bad by their second byte alone.
SEQUENCES = [b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xe0\x9f\xbf", b"\xed\x9f\xbf", b"\xed\xa0\x80",
             b"\xef\xbf\xbf", uc.EURO, b"\xf0\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xf4\x8f\xbf\xbf",
             b"\xf4\x90\x80\x80", uc.GRIN, b"\xc0\x80", b"\xc1\xbf"]


class Case:
    """One batch: streams of whole frames, the streams' opcode seeds."""

    def __init__(self, streams, opcodes=None):
        self.batch = mc.Batch(streams)
        self.state = None
        if opcodes is not None:
            self.state = np.zeros(self.batch.n_streams, dtype=layout.STREAM_STATE)
            self.state["opcode"] = opcodes


def _keys(seed):
    rng = np.random.default_rng(seed)
    return lambda: int(rng.integers(1, 2**32))


def aligned_streams(payloads, masked=True, seed=1, b0=FIN | TEXT):
    """One stream per (payload, a), a in 0..15: an unmasked binary pad frame
    and then the payload as one frame whose first payload byte lies at wire
    offset a mod 16 (payloads shorter than 126 bytes)."""
    key = _keys(seed)
    streams, at = [], 0
    for p in payloads:
        assert len(p) < 126
        for a in range(16):
            hdr = 6 if masked else 2
            pad = (a - (at + 2 + hdr)) % 16
            s = [frame(FIN | BINARY, b"\xff" * pad), frame(b0, p, key=key() if masked else None)]
            assert (at + 2 + pad + hdr) % 16 == a
            at += sum(len(f) for f in s)
            streams.append(s)
    return streams


def kat_alignments():
    return Case(aligned_streams(list(uc.kat().values())))


def phases():
    """Payload lengths 0..20 at every wire alignment, unmasked and masked:
    mixed text, every third one damaged."""
    rng = np.random.default_rng(2)
    texts = []
    for n in range(21):
        t = uc.mixed_text(rng, n)
        texts.append(uc.corrupt(rng, t) if n % 3 == 1 else t)
    return Case(aligned_streams(texts, masked=True, seed=3) + aligned_streams(texts, masked=False))


def _cuts(seq, pieces):
    """seq cut into `pieces` non-empty parts, every way."""
    if pieces == 1:
        return [[seq]]
    return [[seq[:c]] + rest for c in range(1, len(seq) - pieces + 2) for rest in _cuts(seq[c:], pieces - 1)]


def _message(parts, key, between=None, head=b"", tail=b""):
    """One text message whose fragments are head + parts[0], parts[1], ...,
    parts[-1] + tail, each under its own key; `between` (a list of frames)
    after every fragment but the last."""
    frames = []
    last = len(parts) - 1
    for i, p in enumerate(parts):
        data = (head if i == 0 else b"") + p + (tail if i == last else b"")
        frames.append(frame((TEXT if i == 0 else CONT) | (FIN if i == last else 0), data, key=key()))
        if i != last and between:
            frames += between
    return frames


def split_sequences():
    """Every sequence cut at every position across two fragments, across
    three and four fragments of one byte each where it is long enough, bare
    and inside text, and with empty fragments between (masked and not)."""
    key = _keys(4)
    streams = []
    for seq in SEQUENCES:
        for pieces in range(2, len(seq) + 1):
            for parts in _cuts(seq, pieces):
                streams.append(_message(parts, key))
                streams.append(_message(parts, key, head=b"ab", tail=b"yz"))
                streams.append(_message(parts, key, between=[frame(CONT, b"", key=key()), frame(CONT, b"")]))
    return Case(streams)


def ping_between():
    """The missing continuation byte as the payload of a ping between the
    fragments, with and without FIN: the reference appends a control frame's
    payload to the message buffer (and its opcode sticks), so the bytes of
    E2 | ping 82 | AC FIN are one valid string in that buffer."""
    key = _keys(5)
    streams = []
    for seq in SEQUENCES:
        if len(seq) < 3:
            continue
        for b0 in (PING, FIN | PING):
            streams.append([frame(TEXT, b"t" + seq[:1], key=key()), frame(b0, seq[1:2], key=key()),
                            frame(FIN | CONT, seq[2:] + b"z", key=key()), frame(FIN | TEXT, seq, key=key())])
    return Case(streams)


def _spots(size, poff, edges, rng, damage):
    """`size` ASCII bytes with a 3- or 4-byte sequence straddling every wire
    offset in `edges` by 1, 2 and 3 bytes in turn (the payload starts at wire
    offset poff); `damage`: the index of the sequence to cut short, or None."""
    text = bytearray(rng.integers(0x20, 0x7F, size, dtype=np.uint8).tobytes())
    k = 0
    for e in edges:
        seq = (uc.EURO, uc.GRIN)[k & 1]
        before = 1 + k % (len(seq) - 1)
        at = e - poff - before
        if at < 0 or at + len(seq) > size:
            continue
        text[at: at + len(seq)] = seq if k != damage else seq[:-1] + b"A"
        k += 1
    return bytes(text), k


def chunk_and_row_edges():
    """One masked frame of 5000 bytes: sequences straddling 16-byte chunk
    edges and 1 KiB row edges of the wire, whole, and each damaged in turn."""
    rng = np.random.default_rng(6)
    edges = [16, 32, 48, 1024, 2048, 2064, 3072, 4096, 4112]
    _, count = _spots(5000, 8, edges, rng, None)
    streams = []
    for damage in [None] + list(range(count)):
        text, _ = _spots(5000, 8, edges, np.random.default_rng(6), damage)
        streams.append(text)
    # (each stream in a batch of its own: the payload's wire offset is the header's 8 bytes)
    return [Case([[frame(FIN | TEXT, t, key=0xA1B2C3D4 + i)]]) for i, t in enumerate(streams)]


def piece_edges():
    """Fragments of 4096 +- 3 bytes behind a message of odd length, under
    different keys: sequences across every fragment edge, and across the
    multiples of 4096 of the dense offset and of the wire offset; whole, and
    with one of them damaged."""
    cases = []
    sizes = [4093, 4099, 4096, 4095, 4097, 4094, 8200]
    for damage in (None, 0, 3, 7, 11):
        rng = np.random.default_rng(7)
        key = _keys(8)
        head = frame(FIN | TEXT, b"odd" * 11 + uc.EURO, key=key())   # 36 bytes: the dense offsets start odd
        total = sum(sizes)
        text = bytearray(rng.integers(0x20, 0x7F, total, dtype=np.uint8).tobytes())
        # positions in the message: the fragment edges, the dense and the wire multiples of 4096
        marks, at, wire = [], 0, len(head)
        for s in sizes:
            wire += 8                                 # a masked frame with a 16-bit length
            marks += [at] + [x - 36 for x in range(4096, total + 36, 4096) if at <= x - 36 < at + s]
            marks += [at + (w - wire) for w in range((wire // 4096 + 1) * 4096, wire + s, 4096)]
            at, wire = at + s, wire + s
        k, last = 0, -16
        for m in sorted(set(marks)):
            seq = (uc.GRIN, uc.EURO)[k & 1]
            at = m - (1 + k % (len(seq) - 1))
            if at < last + 8 or at + len(seq) > total:   # (not on top of the sequence before it)
                continue
            text[at: at + len(seq)] = seq if k != damage else b"\xbf" + seq[1:]
            k, last = k + 1, at
        assert k > 11
        parts, at = [], 0
        for s in sizes:
            parts.append(bytes(text[at: at + s]))
            at += s
        cases.append(Case([[head] + _message(parts, key)]))
    return cases


def message_boundaries():
    """No context across messages: A ends E2 82 and the next message of the
    stream begins AC; the same with the neighbour in another stream."""
    key = _keys(9)
    a, b = b"text \xe2\x82", b"\xac more"
    return Case([[frame(FIN | TEXT, a, key=key()), frame(FIN | TEXT, b, key=key())],
                 [frame(TEXT, a[:3], key=key()), frame(FIN | CONT, a[3:], key=key())],
                 [frame(FIN | TEXT, b, key=key())],
                 [frame(FIN | TEXT, uc.EURO, key=key()), frame(FIN | TEXT, b"", key=key()),
                  frame(FIN | TEXT, uc.EURO[:2], key=key()), frame(FIN | TEXT, b""), frame(FIN | TEXT, uc.EURO[2:])]])


def close_reasons():
    key = _keys(10)
    st = (1000).to_bytes(2, "big")
    return Case([
        # the status split over two 1-byte frames
        [frame(CLOSE, st[:1], key=key()), frame(CONT, st[1:], key=key()), frame(FIN | CONT, "grüß".encode(), key=key())],
        [frame(CLOSE, st[:1], key=key()), frame(CONT, st[1:], key=key()), frame(FIN | CONT, b"\xbfbad", key=key())],
        # status bytes that look like a lead sequence in front of a reason that begins with 80
        [frame(FIN | CLOSE, b"\xc3\xa9\x80reason", key=key())],
        [frame(FIN | CLOSE, b"\xe2\x82\xac", key=key())],          # status E2 82, reason AC
        [frame(FIN | CLOSE, b"\xc3" + b"\xa9ok", key=key())],      # status C3 A9, reason "ok"
        # a reason that ends in a truncated sequence
        [frame(FIN | CLOSE, st + b"bye " + uc.GRIN[:3], key=key())],
        [frame(CLOSE, st + b"bye " + uc.GRIN[:2], key=key()), frame(FIN | CONT, uc.GRIN[2:], key=key())],
        # bodies of 0 and 1 bytes, and the status alone
        [frame(FIN | CLOSE, b"", key=key())], [frame(FIN | CLOSE, b"\xff", key=key())], [frame(FIN | CLOSE, st)],
    ])


def selection():
    """A binary message full of FF, a kind-0 message (opcode 3), text and a
    close reason, valid and not: for every `which`."""
    key = _keys(11)
    return Case([[frame(FIN | BINARY, b"\xff" * 40, key=key()), frame(FIN | 0x3, b"\xff\xfe", key=key()),
                  frame(FIN | TEXT, b"ok \xff", key=key()), frame(FIN | PING, b"\xc0", key=key()),
                  frame(FIN | TEXT, uc.EURO, key=key())],
                 [frame(FIN | CLOSE, (1001).to_bytes(2, "big") + b"\x80", key=key())],
                 [frame(FIN | CLOSE, (1001).to_bytes(2, "big") + b"fine", key=key())]])


def tails():
    """Text fragments with bad bytes behind a stream's last FIN frame yield nothing."""
    key = _keys(12)
    return Case([[frame(FIN | TEXT, b"kept " + uc.EURO, key=key()), frame(TEXT, b"\xff\xff open", key=key()),
                  frame(CONT, b"\xc0", key=key())],
                 [frame(TEXT, b"\xff never finished", key=key())],
                 [frame(FIN | TEXT, b"next " + uc.GRIN, key=key())]])


def random_fragments():
    """Random bytes in fragments of 1 to 4097 bytes, as text and as binary."""
    rng = np.random.default_rng(15)
    return Case([rc.fragments(rng, 0x81, [1, 2, 3, 5, 4097]), rc.fragments(rng, 0x82, [5, 4097, 3, 2, 1]),
                 rc.fragments(rng, 0x81, [4097, 1])])


def carry_over():
    """(first call, second call): a message whose first fragment lies in the
    first call's tail and is submitted again, with the opcode the first call
    returned as the stream's seed."""
    key = _keys(13)
    done = frame(FIN | BINARY, b"\x00\x01", key=key())
    first = frame(TEXT, b"caf\xc3", key=key())
    rest = [frame(CONT, b"\xa9 \xe2", key=key()), frame(FIN | CONT, b"\x82\xac!", key=key()),
            frame(FIN | TEXT, b"\xac", key=key())]
    return [[done, first]], [[first] + rest]


def many_messages(count=4096 + 7):
    """More one-frame text messages than 64 * 64: three rounds of the 64-probe
    search; a handful invalid, the first and the last among them."""
    rng = np.random.default_rng(14)
    bad = {0, 1, 63, 64, 4095, 4096, count - 1}
    frames = []
    for i in range(count):
        t = uc.mixed_text(rng, int(rng.integers(1, 24)))
        frames.append(frame(FIN | TEXT, uc.corrupt(rng, t) if i in bad else t, key=i + 1))
    return Case([frames[: count // 2], frames[count // 2:]]), bad


def fuzz(seed):
    """checked_reply_cases.fuzz_batch with every data frame's payload replaced
    by text of the same length (mixed_text, one in three damaged); returns
    (Case, role, max_message, proto_in)."""
    batch, role, limit, proto_in, state = cc.fuzz_batch(seed)
    rng = np.random.default_rng(5000 + seed)
    streams = []
    for s in batch.streams:
        out = []
        for f in s:
            rc_, r = ca.header_unpack(f[:14])
            assert rc_ == 0
            b0, size = f[0], int(r["len"])
            if (b0 & 0x0F) in (CONT, TEXT, BINARY) and size:
                t = uc.mixed_text(rng, size)
                if rng.random() < 0.33:
                    t = uc.corrupt(rng, t)
                f = frame(b0, t, key=int(r["key"]) if int(r["masked"]) else None)
            out.append(f)
        streams.append(out)
    c = Case(streams, state["opcode"])
    assert np.array_equal(c.batch.fs, batch.fs)
    return c, role, limit, proto_in


def small_cases():
    """name -> Case: everything a test runs as one batch."""
    out = {"kat_alignments": kat_alignments(), "phases": phases(), "split_sequences": split_sequences(),
           "ping_between": ping_between(), "message_boundaries": message_boundaries(),
           "close_reasons": close_reasons(), "selection": selection(), "tails": tails(),
           "random_fragments": random_fragments()}
    for i, c in enumerate(chunk_and_row_edges()):
        out["chunk_row_%d" % i] = c
    for i, c in enumerate(piece_edges()):
        out["piece_edges_%d" % i] = c
    return out


# ------------------------------------------------------------ expected values
def model(case, which, wire=None):
    """layout.utf8_wire_plan over the oracle's decode of the case's wire (or
    of a damaged copy): (rc, info, msgs, count, valid, result)."""
    b = case.batch
    code, out, info = oracle.decode_batch(b.wire if wire is None else wire, b.fs)
    msgs, count, valid, result = layout.utf8_wire_plan(info, b.stream_first, case.state, out, which)
    return code, info, msgs, count, valid, result


def selected(m, which):
    kind, op = int(m["kind"]), int(m["opcode"])
    return bool(which & layout.UTF8_EVERY) or (bool(which & layout.UTF8_TEXT) and kind == 1 and op == TEXT) or \
        (bool(which & layout.UTF8_CLOSE) and kind == 2)


def check_case(case, which):
    """The model's answer against Python's strict decoder applied to what one
    oracle session per stream delivers (text to onWSReceived, the reason to
    onWSClose: mc.check_model holds the table and its bytes against the
    sessions' events); returns the model's tuple."""
    b = case.batch
    msgs, count, new_state, buf, _, _ = mc.check_model(b, case.state)
    code, info, m2, c2, valid, result = model(case, which)
    assert code == 0
    mc.same_fields(m2, msgs, mc.MSG_FIELDS)
    assert [int(x) for x in c2] == [int(x) for x in count]
    want = [uc.want(buf[int(m["off"]):][: int(m["len"])].tobytes()) if selected(m, which) else int(m["len"])
            for m in msgs]
    assert [int(x) for x in valid] == want
    bad = [i for i, m in enumerate(msgs) if want[i] < int(m["len"])]
    sel = [m for m in msgs if selected(m, which)]
    assert [int(x) for x in result] == [len(bad), bad[0] if bad else cc.U64_MAX, len(sel),
                                        sum(int(m["len"]) for m in sel)]
    return code, info, msgs, count, valid, result

