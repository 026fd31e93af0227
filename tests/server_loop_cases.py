"""Shared by tests/golden/make_rfc6455.py, tests/test_rfc6455_model.py (CPU)
and tests/test_gpu_server_loop.py: the connections an echo server is fed over
many cut reads, the driver of that loop, a numpy step for it, and the
comparison of the project's rule with a recorded outside reader
(tests/golden/rfc6455.json).

The connections are rebuilt from SEED; the fixture holds a digest of each, the
reader's outcomes and the named classes in which the two may differ.  No test
lives here."""
import functools
import hashlib
import json
import os

import numpy as np

import cppserver_amd as ca
import oracle
from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import frames_cases as fc
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import reply_cases as rc

U64_MAX = 2 ** 64 - 1
NONE = cc.NONE
SEED = 6470                  # one whose connections put at least one into every class of the fixture
N_CONNECTIONS = 264          # more than one block (256) of streams in the first rounds
LIMITS = (0, 400)            # max_message: none, and one that fragmented messages outgrow
WHICH = layout.UTF8_TEXT | layout.UTF8_CLOSE
MAX_ROUNDS = 40
WIRE_MAX = 1 << 20
REST = -1                    # a read that delivers everything left
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfc6455.json")
# header forms of a masked frame: 2, 4 and 10 bytes plus the key
HEADER_FORMS = {6: 5, 8: 300, 14: 65536}   # header bytes -> a payload length that has it
# the records of the fixture: (max_message, the reader decodes text)
RECORDS = [(limit, decode) for limit in LIMITS for decode in (False, True)]
CAP_ABC, CAP_D = 0.05, 0.10


def record_name(limit, decode):
    return "max%d_%s" % (limit, "utf8" if decode else "raw")


def digest(data, n=12):
    return hashlib.sha256(bytes(data)).hexdigest()[:n]


# ------------------------------------------------------------------ payloads
def utf8_text(rng, n):
    """Exactly n bytes of valid UTF-8 mixing 1- to 4-byte sequences."""
    out, left = [], n
    while left:
        size = min(int(rng.integers(1, 5)), left)
        if size == 1:
            cp = int(rng.integers(0x20, 0x7F))
        elif size == 2:
            cp = int(rng.integers(0x80, 0x800))
        elif size == 3:
            cp = int(rng.integers(0x800, 0xD800)) if rng.random() < 0.8 else int(rng.integers(0xE000, 0x10000))
        else:
            cp = int(rng.integers(0x10000, 0x110000))
        out.append(chr(cp))
        left -= size
    data = "".join(out).encode("utf-8")
    assert len(data) == n
    return data


def corrupted(rng, data):
    """(bytes that are not UTF-8, a split point or None): a truncated
    sequence at the end, a byte no sequence holds, a stray continuation, an
    overlong form, a surrogate, or the head of a sequence whose rest never
    comes, to be split from what follows it."""
    kind = int(rng.integers(0, 6))
    at = None
    if kind == 0:
        data = data + [b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98"][int(rng.integers(0, 3))]
    elif kind == 1:
        k = int(rng.integers(0, len(data) + 1))
        data = data[:k] + b"\xff" + data[k:]
    elif kind == 2:
        data = b"\x80" + data
    elif kind == 3:
        data = data + b"\xc0\xaf"
    elif kind == 4:
        data = b"\xed\xa0\x80" + data
    else:
        head = utf8_text(rng, int(rng.integers(0, 20)))
        at = len(head) + 2
        data = head + b"\xf0\x9f" + b"plain " + data
    try:
        data.decode("utf-8")
    except UnicodeDecodeError:
        return data, at
    raise AssertionError("a corruption that is valid UTF-8")


def split(rng, data, parts, at=None):
    """data in `parts` pieces cut at random bytes (inside sequences too), one
    of the cuts at `at` when given."""
    cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, parts - 1))
    if at is not None and cuts:
        cuts[0] = at
        cuts.sort()
    cuts = [0] + cuts + [len(data)]
    return [data[cuts[i]: cuts[i + 1]] for i in range(parts)]


# ------------------------------------------------------------------ connections
class Conn:
    """One connection: whole frames, then `tail`, the head of one more frame
    (the connection ends inside it).  `first_read`: the size of its first
    read when the schedule does not choose it; `late`: rounds of small reads
    before the rest of a large frame is delivered."""

    def __init__(self, name, frames, tail=b"", first_read=None, late=None):
        self.name, self.frames, self.tail = name, [bytes(f) for f in frames], bytes(tail)
        self.first_read, self.late = first_read, late
        self.data = b"".join(self.frames) + self.tail


P_INTERLEAVE = 0.04   # a control frame between fragments: class (d), kept rare
BAD_STATUSES = [0, 999, 1004, 1005, 1006, 1015, 2999, 5000, 65535]


def _random_frames(rng):
    """0-40 frames, each a valid next frame of its connection with probability
    about 0.9 and one of protocol_cases.fuzz's violations otherwise; every
    frame masked, text and close reasons UTF-8 unless corrupted."""
    f, F = pc.frame, pc.FIN
    count = int(40 * rng.random() ** 3 + rng.random())
    frames, plan, is_open = [], [], False

    def key():
        return int(rng.integers(1, 2 ** 32))

    def control():
        return f(F | int(rng.choice([pc.PING, pc.PONG])), rc.data(rng, int(rng.integers(0, 126))), key())

    while len(frames) < count:
        body = rc.data(rng, int(rng.integers(0, 301)))
        if rng.random() < 0.9:
            if is_open:
                if rng.random() < P_INTERLEAVE:
                    frames.append(control())
                    continue
                part = plan.pop(0)
                is_open = bool(plan)
                frames.append(f((0 if is_open else F) | pc.CONT, part, key()))
                continue
            pick = rng.random()
            if pick < 0.2:
                frames.append(control())
            elif pick < 0.24:
                if rng.random() < 0.3:
                    frames.append(pc.close(None, key=key()))
                else:
                    reason = utf8_text(rng, int(rng.integers(0, 21)))
                    if rng.random() < 0.1:
                        reason = corrupted(rng, reason)[0]
                    frames.append(pc.close(int(rng.choice([1000, 1001, 1003, 1011, 3000, 4999])), reason, key()))
            else:
                op = int(rng.choice([pc.TEXT, pc.BINARY]))
                parts = 1 if rng.random() < 0.5 else int(rng.integers(2, 7))
                total = int(rng.integers(0, 301)) if parts == 1 else int(rng.integers(0, 150 * parts))
                at = None
                if op == pc.TEXT:
                    data = utf8_text(rng, total)
                    if rng.random() < 0.08:
                        data, at = corrupted(rng, data)
                else:
                    data = rc.data(rng, total)
                pieces = [p[:300] for p in split(rng, data, parts, at)]
                plan = pieces[1:]
                is_open = bool(plan)
                frames.append(f((0 if is_open else F) | op, pieces[0], key()))
        else:
            bad = int(rng.integers(0, 9))
            if bad == 0:
                frames.append(f(F | pc.BINARY | int(rng.choice([0x10, 0x20, 0x40, 0x70])), body, key()))
            elif bad == 1:
                frames.append(f(F | int(rng.choice([3, 4, 5, 6, 7, 0xB, 0xC, 0xD, 0xE, 0xF])), body[:100], key()))
            elif bad == 2:
                frames.append(f(int(rng.choice([pc.PING, pc.PONG, pc.CLOSE])), body[:100], key()))
            elif bad == 3:
                frames.append(f(F | pc.PING, bytes(int(rng.integers(126, 400))), key()))
            elif bad == 4:   # a new data frame inside a message, a continuation outside one
                fin = F if rng.random() < 0.7 else 0
                frames.append(f(fin | (int(rng.choice([pc.TEXT, pc.BINARY])) if is_open else pc.CONT), body, key()))
            elif bad == 5:
                frames.append(f(F | pc.CLOSE, b"\x03", key()))
            elif bad == 6:
                frames.append(pc.close(int(rng.choice(BAD_STATUSES)), b"", key()))
            elif bad == 7:   # a violation only under the limit
                frames.append(f(F | (pc.CONT if is_open else pc.BINARY), bytes(LIMITS[1] + 1), key()))
                is_open, plan = False, []
            else:
                frames.append(f(F | pc.TEXT | 0x40, body, key()))
    return frames


def _deterministic():
    f, F = pc.frame, pc.FIN
    rng = np.random.default_rng(SEED + 1)
    k = 0x1F2E3D4C
    hello = [f(F | pc.TEXT, "grüß dich".encode(), k)]
    out = [Conn("lengths", [f(F | pc.BINARY, rc.data(rng, n), k + n) for n in (125, 126, 127, 65535, 65536)])]
    text = utf8_text(rng, 333)
    pieces = split(rng, text, 6)
    out.append(Conn("six_fragments", [f((F if i == 5 else 0) | (pc.TEXT if i == 0 else pc.CONT), p, k + i)
                                      for i, p in enumerate(pieces)] + hello))
    three = split(rng, text, 3)
    out.append(Conn("ping_pong_between", [f(pc.TEXT, three[0], 1), f(F | pc.PING, b"ping", 2), f(pc.CONT, three[1], 3),
                                          f(F | pc.PONG, b"pong", 4), f(F | pc.CONT, three[2], 5)] + hello))
    out.append(Conn("close_empty", hello + [pc.close(None, key=k)] + hello))
    out.append(Conn("close_one_byte", hello + [f(F | pc.CLOSE, b"\x03", k)] + hello))
    for status in (1000, 1003, 1007, 1014, 3000, 3999, 4000, 4999):
        out.append(Conn("close_%d" % status, hello + [pc.close(status, "schluß".encode(), k + status)] + hello))
    whole = f(F | pc.BINARY, rc.data(rng, 300), k)
    out.append(Conn("ends_in_header", hello, tail=whole[:5]))
    out.append(Conn("ends_in_payload", hello + [f(pc.TEXT, b"open", 7)], tail=f(F | pc.CONT, rc.data(rng, 300), k)[:100]))
    out.append(Conn("empty", []))
    lead = f(F | pc.TEXT, b"lead", 9)
    late = 0
    for hdr, n in HEADER_FORMS.items():
        for c in range(1, hdr):
            big = n > 60000
            out.append(Conn("header%d_cut%d" % (hdr, c), [lead, f(F | pc.BINARY, rc.data(rng, n), k + c),
                                                          f(F | pc.PING, b"behind", c)],
                            first_read=len(lead) + c, late=late if big else None))
            late += big
    return out


@functools.lru_cache(maxsize=None)
def connections():
    det = _deterministic()
    rng = np.random.default_rng(SEED)
    out = list(det)
    while len(out) < N_CONNECTIONS:
        frames = _random_frames(rng)
        tail = b""
        if rng.random() < 0.1:   # the connection ends inside one more frame, valid wherever it comes
            whole = pc.frame(pc.FIN | pc.PING, rc.data(rng, int(rng.integers(0, 126))), 11)
            tail = whole[: int(rng.integers(1, len(whole)))]
        out.append(Conn("random%d" % len(out), frames, tail))
    return out


def send_keys():
    return np.random.default_rng(SEED + 2).integers(0, 2 ** 32, N_CONNECTIONS).astype(np.uint32)


# ------------------------------------------------------------------ the whole connections in one call
@functools.lru_cache(maxsize=None)
def whole_batch():
    return mc.Batch([c.frames for c in connections()])


@functools.lru_cache(maxsize=None)
def utf8_verdicts():
    """checked_reply_cases.utf8_also over every connection's whole frames."""
    batch = whole_batch()
    w = cc.expected(batch)
    out_o, info = batch.oracle_decode()
    return tuple(cc.utf8_also(w.msgs, mc.dense(out_o, info, batch.stream_first, w.state), WHICH, batch.n_streams))


@functools.lru_cache(maxsize=None)
def one_call(limit, validating, rule, mask):
    """checked_reply_cases.expected of every whole connection as one stream
    of one call, as a server."""
    keys = send_keys() if mask else None
    return cc.expected(whole_batch(), rule, mask, keys, role=pc.SERVER, max_message=limit,
                       also=list(utf8_verdicts()) if validating else None)


def local(verdicts, stream_first):
    """Verdicts with the frame as an index within the stream."""
    return [v if v == NONE else (v[0], v[1], v[2] - int(stream_first[j])) for j, v in enumerate(verdicts)]


def rule_loop(limit):
    """protocol_cases.loop over the whole connections (verdicts, local)."""
    b = pc.Batch([c.frames for c in connections()])
    return local(b.expect(pc.SERVER, limit)[0], b.stream_first)


def with_utf8(verdicts):
    """Local protocol verdicts merged with the UTF-8 verdicts."""
    sf = whole_batch().stream_first
    glob = [v if v == NONE else (v[0], v[1], v[2] + int(sf[j])) for j, v in enumerate(verdicts)]
    return local(cc.merged(glob, list(utf8_verdicts()), sf), sf)


# ------------------------------------------------------------------ the agreement domain
SECTIONS = {
    "a": "RFC 6455 7.4.1, 7.4.2: 1006 and 5000+ must not be set in a close frame; WSG_PV_CLOSE_CODE, 1002",
    "b": "RFC 6455 5.4, 5.5 against 7.4.1 (1009): one frame breaks two rules, the lowest code answers, 1002",
    "c": "RFC 6455 5.4: a new data frame inside an open message; WSG_PV_DATA, 1002",
    "d": "control frames between fragments: their payload joins the message buffer and the opcode sticks "
         "(the reference's behaviour, kept on purpose); verdicts of the frame rules are compared, payloads and "
         "UTF-8 are not",
    "e": "RFC 6455 5.5.1, 8.1: an invalid close reason is judged by the validating chain only; without it the "
         "close is clean (WSG_PV_CLOSED, the status it carries)",
}


def _walk(frames, limit):
    """Per frame (record, open before, bytes before) by protocol_cases.judge."""
    b = pc.Batch([frames])
    out, is_open, nbytes = [], False, 0
    for i in range(b.n):
        out.append((b.info[i], is_open, nbytes))
        _, _, is_open, nbytes = pc.judge(b.info[i], b.wire, is_open, nbytes, pc.SERVER, limit)
    return b, out


def in_class_d(conn, limit, project):
    """A control frame inside an open message in front of the terminal frame,
    or the terminal frame itself when it is such a frame and no violation of
    the frame rules (a clean close, or its reason judged: the close message's
    buffer begins with the open message's bytes)."""
    _, walk = _walk(conn.frames, limit)
    stop = len(walk) if project == NONE else project[2] + (project[0] in (layout.PV_CLOSED, layout.PV_UTF8))
    return any(int(r["opcode"]) & 8 and is_open for r, is_open, _ in walk[:stop])


def classify(conn, limit, decode, project, reader):
    """None when the project's verdict (code, status, frame) or NONE and the
    reader's outcome (status, frame) or None agree; else the class's letter,
    or "?" for a difference no class explains."""
    if project == NONE and reader is None:
        return None
    if project != NONE and reader is not None and tuple(reader) == (project[1], project[2]):
        return None
    if project == NONE or (reader is not None and reader[1] < project[2]):
        return "?"
    code, status, t = project
    b, walk = _walk(conn.frames, limit)
    rec, is_open, nbytes = walk[t]
    here = reader is not None and reader[1] == t
    if code == layout.PV_CLOSE_CODE and here:
        at = int(rec["payload_off"])
        key = int(rec["key"])
        carried = (int(b.wire[at]) ^ (key & 0xFF)) << 8 | (int(b.wire[at + 1]) ^ ((key >> 8) & 0xFF))
        if (carried == 1006 or carried >= 5000) and reader[0] == carried:
            return "a"
    if status == 1002 and here and reader[0] == 1009 and limit:
        return "b"
    if code == layout.PV_DATA and not here and (not rec["fin"] or nbytes == 0):
        return "c"
    if code == layout.PV_CLOSED and here and reader[0] == 1007 and not decode and int(rec["len"]) > 2:
        return "e"
    return "?"


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def reader_outcomes(limit, decode):
    """Per connection the fixture's (status, frame) or None, its class or None, in class (d) or not."""
    rows = fixture()["connections"]
    name = record_name(limit, decode)
    return [(tuple(r[name]["reader"]) if r[name]["reader"] is not None else None, r[name].get("class"),
             bool(r[name].get("d"))) for r in rows]


def check_against_reader(verdicts, limit, decode, what):
    """Local verdicts of every connection against the fixture's record: equal
    to the reader's inside the agreement domain, to the recorded project-side
    value in classes (a) to (c) and (e).  With decode, class (d) is left out
    (its UTF-8 is not compared)."""
    rows = fixture()["connections"]
    name = record_name(limit, decode)
    compared = 0
    for j, (v, row) in enumerate(zip(verdicts, rows)):
        r = row[name]
        if r.get("d") and decode:
            continue
        compared += 1
        where = "%s: connection %d (%s), %s" % (what, j, row["name"], name)
        if r.get("class"):
            assert list(v) == r["project"], where + ", class " + r["class"]
        elif r["reader"] is None:
            assert v == NONE, where
        else:
            assert v != NONE and [v[1], v[2]] == r["reader"], where
    return compared


# ------------------------------------------------------------------ replies taken apart
def unpack(out):
    """A connection's output as [(first header byte, data, status)] by the
    oracle alone: its walk finds the frames, a session their callbacks."""
    out = bytes(out)
    starts, used = fc.oracle_walk(out)
    assert used == len(out), "the output does not end at a frame's end"
    s = oracle.Session()
    s.prepare_receive(out)
    ev = s.events()
    assert len(ev) == len(starts), "a reply frame that fires no callback"
    return [(out[at], e[1], e[2]) for at, e in zip(starts, ev)]


def echoed(frames):
    """The data messages among unpacked reply frames: (type, length, digest)."""
    return [(b0 & 0x0F, len(data), digest(data)) for b0, data, _ in frames if b0 & 0x0F in (pc.TEXT, pc.BINARY)]


# ------------------------------------------------------------------ the schedule
def schedule(seed):
    """Per connection its read sizes, one per round, the last of them REST:
    0, 1, 2, 3, up to 700 bytes or everything.  A header-cut connection's
    first read ends inside its second frame's header; the rest of a large
    frame comes at a round of its own, so that a round's wire stays small."""
    rng = np.random.default_rng([SEED, seed])
    out = []
    for j, c in enumerate(connections()):
        sizes = []
        if c.first_read is not None:
            sizes.append(c.first_read)
        if c.late is not None:
            sizes += [int(x) for x in rng.integers(0, 3, 2 + c.late)]
        else:
            last = 8 + (j + seed) % 20
            while len(sizes) < last:
                pick = int(rng.integers(0, 12))
                if pick == 11:
                    break
                sizes.append(pick if pick < 4 else int(rng.integers(4, 701)))
        out.append(sizes + [REST])
    return out


class Run:
    """What drive() leaves: per connection the output, the verdict (frame
    within the connection) or NONE, and for one that was never dropped the
    final (bytes, open), opcode and left-over bytes."""


def drive(step, seed, keys=None):
    """The echo server's loop over every connection.  ``step(wire, spans,
    opcodes, proto, keys, frame_cap)`` is one round's call: see model_step
    for what it returns."""
    conns = connections()
    reads = schedule(seed)
    n = len(conns)
    rng = np.random.default_rng([SEED, seed, 1])
    run = Run()
    run.out = [bytearray() for _ in range(n)]
    run.verdict = [NONE] * n
    run.proto, run.opcode, run.left = [(0, 0)] * n, [0] * n, [b""] * n
    run.header_cuts, run.max_streams, run.max_frames, run.max_wire, run.rounds = set(), 0, 0, 0, 0
    run.resubmitted = run.tail_close = 0
    pos, pending, frames_done, rounds_of = [0] * n, [b""] * n, [0] * n, [0] * n
    frames_left = [len(c.frames) for c in conns]
    bounds = [np.cumsum([0] + [len(f) for f in c.frames]) for c in conns]
    live = list(range(n))
    while live:
        assert run.rounds < MAX_ROUNDS, "the loop does not end"
        chunks, spans, at = [], np.zeros(len(live), dtype=layout.STREAM_SPAN), 0
        for s, j in enumerate(live):
            size = reads[j][rounds_of[j]]
            rounds_of[j] += 1
            total = len(conns[j].data)
            new = conns[j].data[pos[j]:] if size == REST else conns[j].data[pos[j]: pos[j] + size]
            pos[j] += len(new)
            k = int(np.searchsorted(bounds[j], pos[j], side="right")) - 1   # the frame pos lies in
            if pos[j] < total and k < len(conns[j].frames):
                rec = ca.header_unpack(conns[j].frames[k][:14])[1]
                inside = pos[j] - int(bounds[j][k])
                if 0 < inside < int(rec["hdr_len"]):
                    run.header_cuts.add((int(rec["hdr_len"]), inside))
            run.resubmitted += bool(pending[j]) and not new
            pending[j] += new
            gap = rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes()
            chunks += [gap, pending[j]]
            spans["off"][s], spans["len"][s] = at + len(gap), len(pending[j])
            at += len(gap) + len(pending[j])
        chunks.append(bytes(64))
        wire = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        assert len(wire) < WIRE_MAX, "round %d: a wire of %d bytes" % (run.rounds, len(wire))
        frame_cap = min(len(wire) // 2, sum(frames_left[j] for j in live)) + 1
        r = step(wire, spans, np.array([run.opcode[j] for j in live], dtype=np.uint8), [run.proto[j] for j in live],
                 None if keys is None else keys[live], frame_cap)
        run.rounds += 1
        run.max_streams = max(run.max_streams, len(live))
        run.max_frames = max(run.max_frames, int(r.stream_first[-1]))
        run.max_wire = max(run.max_wire, len(wire))
        still = []
        for s, j in enumerate(live):
            run.out[j] += bytes(r.reply[int(r.stream_reply[s]): int(r.stream_reply[s + 1])])
            v = r.verdict[s]
            assert (v != NONE) == (int(r.close_off[s]) != U64_MAX), "connection %d: a verdict without a close frame" % j
            if v != NONE:   # disconnected: its later bytes are never submitted
                first = int(r.stream_first[s])
                assert first <= v[2] < int(r.stream_first[s + 1])
                run.verdict[j] = (v[0], v[1], v[2] - first + frames_done[j])
                run.tail_close += v[2] - first >= int(r.frames_consumed[s])
                continue
            frames_done[j] += int(r.frames_consumed[s])
            frames_left[j] -= int(r.frames_consumed[s])
            pending[j] = pending[j][int(r.bytes_consumed[s]):]
            run.opcode[j], run.proto[j] = int(r.opcode[s]), (int(r.proto[s][0]), int(r.proto[s][1]))
            if pos[j] < len(conns[j].data):
                still.append(j)
            else:
                run.left[j] = pending[j]
        live = still
    run.out = [bytes(o) for o in run.out]
    return run


# ------------------------------------------------------------------ one round in numpy
class Step:
    """One round's results: reply (uint8), stream_reply, close_off, verdict
    (tuples, frames of this round's table), stream_first, frames_consumed,
    bytes_consumed (the lowered span.consumed), opcode, proto [(bytes, open)]."""


def lowered(frame_start, stream_first, spans_off, spans_consumed, frames_consumed):
    """span.consumed lowered to the start of each stream's first tail frame."""
    out = []
    for j in range(len(spans_off)):
        first, used = int(stream_first[j]), int(frames_consumed[j])
        nj = int(stream_first[j + 1]) - first
        out.append(int(frame_start[first + used]) - int(spans_off[j]) if used < nj else int(spans_consumed[j]))
    return out


def model_step(rule, mask, limit, validating):
    """The round as layout.frame_plan, message_plan, protocol_plan and
    checked_reply_plan give it; the reply frames' bytes come from the
    oracle's sessions (reply_cases.plan_replies)."""
    def step(wire, spans, opcodes, proto, keys, frame_cap):
        ns = len(spans)
        fs, sf, spans_out, count = layout.frame_plan(wire, spans)
        assert int(count[0]) <= frame_cap
        rc_, out_o, info = oracle.decode_batch(wire, fs)
        assert rc_ == 0
        state = np.zeros(ns, dtype=layout.STREAM_STATE)
        state["opcode"] = opcodes
        msgs, _, new_state = layout.message_plan(info, sf, state, payload=out_o)
        pin = np.zeros(ns, dtype=layout.PROTO_STATE)
        for j, (nbytes, is_open) in enumerate(proto):
            pin[j] = (nbytes, is_open, 0)
        pv, proto_out, _ = layout.protocol_plan(info, sf, pin, pc.SERVER, limit, wire, consumed=new_state["consumed"])
        buf = mc.dense(out_o, info, sf, new_state)
        also = None
        if validating:
            valid, _ = layout.utf8_plan(msgs, buf, WHICH)
            also = layout.utf8_verdicts(msgs, valid, WHICH, ns)
        eff = layout.merge_verdicts(pv, also, sf)
        reply_off, stream_reply, close_off, rcount = layout.checked_reply_plan(msgs, eff, rule, mask, keys, n_streams=ns)
        reply = np.zeros(int(rcount[0]), dtype=np.uint8)
        every = rc.plan_replies(msgs, buf, rule, mask, keys)
        verdict = cc.verdict_tuples(eff)
        fin = msgs["first_frame"].astype(np.int64) + msgs["nframes"] - 1
        for q, m in enumerate(msgs):
            v = verdict[int(m["stream"])]
            if v == NONE or fin[q] < v[2]:
                reply[int(reply_off[q]): int(reply_off[q]) + len(every[q])] = np.frombuffer(every[q], dtype=np.uint8)
        for j, v in enumerate(verdict):
            if v != NONE:
                key = int(keys[j]) if keys is not None else 0
                close = oracle.Session(key).prepare_send(0x88, mask, b"", 1000 if v[1] == 1005 else v[1])
                reply[int(close_off[j]): int(close_off[j]) + len(close)] = np.frombuffer(close, dtype=np.uint8)
        r = Step()
        r.reply, r.stream_reply, r.close_off, r.verdict, r.stream_first = reply, stream_reply, close_off, verdict, sf
        r.frames_consumed, r.opcode = new_state["consumed"], new_state["opcode"]
        r.bytes_consumed = lowered(fs, sf, spans["off"], spans_out["consumed"], new_state["consumed"])
        r.proto = [(int(p["bytes"]), int(p["open"])) for p in proto_out]
        return r
    return step


# ------------------------------------------------------------------ what every run must satisfy
def check_run(run, limit, validating, rule, mask, what):
    """One drive() against the one-call expectation, the fixture and the
    shape every output has."""
    conns = connections()
    w = one_call(limit, validating, rule, mask)
    sf = whole_batch().stream_first
    want = local(w.verdict, sf)
    for j, c in enumerate(conns):
        where = "%s: connection %d (%s)" % (what, j, c.name)
        assert run.out[j] == w.by_stream[j], where
        assert run.verdict[j] == want[j], where
        if want[j] == NONE:   # never dropped: the carries are the one call's
            assert run.proto[j] == (int(w.proto["bytes"][j]), int(w.proto["open"][j])), where
            assert run.opcode[j] == int(w.state["opcode"][j]), where
            assert run.left[j] == b"".join(c.frames[int(w.state["consumed"][j]):]) + c.tail, where
    check_against_reader(run.verdict, limit, validating, what)
    rows = fixture()["connections"]
    name = record_name(limit, validating)
    for j, c in enumerate(conns):
        where = "%s: connection %d (%s)" % (what, j, c.name)
        frames = unpack(run.out[j])
        closes = [k for k, (b0, _, _) in enumerate(frames) if b0 & 0x0F == pc.CLOSE]
        v = run.verdict[j]
        if v == NONE:
            assert closes == [], where
        else:
            assert closes == [len(frames) - 1], where
            assert frames[-1][2] == (1000 if v[1] == 1005 else v[1]) and frames[-1][1] == b"", where
        if rows[j][name].get("d") or rows[j][record_name(limit, False)].get("d"):
            continue
        stop = len(c.frames) if v == NONE else v[2]
        delivered = [(t, n, d) for at, t, n, d in rows[j]["messages"] if at < stop]
        got = echoed(frames)
        if rule[1] != layout.REPLY_SAME:   # every data message answered as binary: the type is not echoed
            got, delivered = [g[1:] for g in got], [g[1:] for g in delivered]
        assert got == [tuple(x) for x in delivered], where
