"""Shared by tests/test_relay_model.py (CPU), tests/test_gpu_relay.py and
tests/test_gpu_relay_loop.py: what wsg_relay_validated must leave in d_relay,
built without layout.relay_plan.

The expectation is built the way checked_reply_cases.expected builds replies:
per stream an oracle session is fed the frames in front of the effective
terminal frame, and each relayed callback becomes
oracle.Session(0).prepare_send(op, False, data), the status form for a
close-kind message (that is expected() itself with the relay rule, mask 0 and
no keys; under WSG_ASSEMBLY_RFC rfc_assembly_cases.expected).  The frames are
joined per group in d_order's order by plain loops.  No test lives here."""
import numpy as np

import cppserver_amd as ca
import oracle
from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import rfc_assembly_cases as ac
from tests import reply_cases as rc
from tests import server_loop_cases as sl

U64_MAX = cc.U64_MAX
NONE = cc.NONE
WHICH = layout.UTF8_TEXT | layout.UTF8_CLOSE
CHAT_REPLY, CHAT_RELAY = layout.CHAT_REPLY, layout.CHAT_RELAY
SAME = (0, layout.REPLY_SAME, 0, 0, 0)
# relay rules with the reply rule that goes with each (no kind in both)
RULES = {
    "chat": (CHAT_REPLY, CHAT_RELAY),
    "same": ((0, 0, 0x88, 0x8A, 0), SAME),
    "ping_as_ping": ((0, layout.REPLY_SAME, 0, 0, 0), (0, 0, 0, 0x89, 0)),
    "close_kind": ((0, 0x82, 0, 0x8A, 0), (0, 0, 0x88, 0, layout.REPLY_SAME)),
    "everything": ((0, 0, 0, 0, 0), (0, layout.REPLY_SAME, 0x88, 0x89, layout.REPLY_SAME)),
    "none": (rc.SAME_CLOSE_PONG, (0, 0, 0, 0, 0)),
}


class Rooms:
    """d_order and d_group_first of one call (None, None: one room of everyone)."""

    def __init__(self, order=None, group_first=None):
        self.order = None if order is None else np.asarray(order, dtype=np.uint32)
        self.group_first = None if group_first is None else np.asarray(group_first, dtype=np.uint32)

    def positions(self, ns):
        return list(range(ns)) if self.order is None else [int(j) for j in self.order]

    def bounds(self, ns):
        return [0, ns] if self.group_first is None else [int(x) for x in self.group_first]


def rooms(ns, kind, seed=0):
    """Named room tables over ns streams."""
    rng = np.random.default_rng([77, seed, ns])
    if kind == "null":
        return Rooms()
    if kind == "two":
        return Rooms(None, [0, ns // 2, ns])
    if kind == "each":
        return Rooms(np.arange(ns)[::-1], np.arange(ns + 1))
    if kind == "empty_rooms":   # empty rooms first, in the middle and last
        cut = sorted(int(x) for x in rng.integers(0, ns + 1, 2))
        return Rooms(rng.permutation(ns), [0, 0, cut[0], cut[0], cut[0], cut[1], ns, ns])
    if kind == "reversed":
        return Rooms(np.arange(ns)[::-1], [0, ns])
    if kind == "random":
        ng = int(rng.integers(1, 6))
        return Rooms(rng.permutation(ns), [0] + sorted(int(x) for x in rng.integers(0, ns + 1, ng - 1)) + [ns])
    raise KeyError(kind)


ROOM_KINDS = ("null", "two", "each", "empty_rooms", "reversed", "random")


class Relay:
    """The relay side of one call: relay (bytes), relay_off (per message,
    U64_MAX: not relayed), group_relay, count [bytes, frames, 0], and per
    stream the frames it contributed."""


def joined(frames, msgs, ns, rooms):
    """The per-message relay frames (b"": not relayed) of a Want laid out as
    d_relay: by position, within a stream by message."""
    r = Relay()
    of_stream = [[] for _ in range(ns)]
    for q, m in enumerate(msgs):
        if frames[q]:
            of_stream[int(m["stream"])].append(q)
    r.by_stream = [[frames[q] for q in qs] for qs in of_stream]
    r.frame_of = {q: frames[q] for qs in of_stream for q in qs}
    r.relay_off = [U64_MAX] * len(msgs)
    parts, at, pos_start = [], 0, []
    for j in rooms.positions(ns):
        pos_start.append(at)
        for q in of_stream[j]:
            r.relay_off[q] = at
            parts.append(frames[q])
            at += len(frames[q])
    pos_start.append(at)
    r.relay = b"".join(parts)
    r.group_relay = [pos_start[p] for p in rooms.bounds(ns)]
    r.count = [len(r.relay), sum(1 for f in frames if f), 0]
    return r


def nothing(n_msgs, rooms, ns):
    """What broken room tables leave."""
    r = Relay()
    r.relay, r.relay_off, r.count = b"", [U64_MAX] * n_msgs, [0, 0, 0]
    r.group_relay = [0] * len(rooms.bounds(ns))
    r.by_stream, r.frame_of = [[] for _ in range(ns)], {}
    return r


def validated_want(batch, rule, mask=0, keys=None, state=None, role=pc.ANY, max_message=0, proto_in=None, also=None,
                   which=WHICH, rfc=False):
    """The Want of wsg_reply_validated for ``rule`` (either assembly mode)."""
    if rfc:
        return ac.expected(batch, rule, mask, keys, state, role, max_message, proto_in, also, which=which)
    damaged = not hasattr(batch, "streams")   # a round's table: no sessions, the records' bytes
    wire = batch.wire if damaged else None
    w0 = cc.expected(batch, rule, mask, keys, state, role, max_message, proto_in, None, wire)
    out_o = oracle.decode_batch(batch.wire, batch.fs)[1]
    buf = mc.dense(out_o, w0.info, batch.stream_first, w0.state)
    utf8 = cc.utf8_also(w0.msgs, buf, which, batch.n_streams)
    eff = ac.effective_also(utf8, also, batch.stream_first)
    w = cc.expected(batch, rule, mask, keys, state, role, max_message, proto_in, eff, wire)
    w.buf = buf
    return w


def expected(batch, relay_op, rooms, state=None, role=pc.ANY, max_message=0, proto_in=None, also=None, which=WHICH,
             rfc=False):
    """(Want of the relay rule with mask 0 and no keys, Relay)."""
    w = validated_want(batch, relay_op, 0, None, state, role, max_message, proto_in, also, which, rfc)
    return w, joined(w.frames, w.msgs, batch.n_streams, rooms)


# ------------------------------------------------------------------ the model
def model_relay(w, relay_op, rooms, ns):
    """layout.relay_plan's tables with the records' frames placed by them."""
    eff = cc.verdict_array(w.verdict)
    relay_off, group_relay, count = layout.relay_plan(w.msgs, eff, relay_op, rooms.order, rooms.group_first)
    every = rc.plan_replies(w.msgs, w.buf, relay_op, 0, None)
    out = np.zeros(int(count[0]), dtype=np.uint8)
    r = Relay()
    r.by_stream, r.frame_of = [[] for _ in range(ns)], {}
    for q, m in enumerate(w.msgs):
        if int(relay_off[q]) != U64_MAX:
            out[int(relay_off[q]): int(relay_off[q]) + len(every[q])] = np.frombuffer(every[q], dtype=np.uint8)
            r.by_stream[int(m["stream"])].append(every[q])
            r.frame_of[q] = every[q]
    r.relay, r.relay_off = out.tobytes(), [int(x) for x in relay_off]
    r.group_relay, r.count = [int(x) for x in group_relay], [int(x) for x in count]
    return r


def same_relay(a, b):
    assert a.relay == b.relay and a.relay_off == b.relay_off
    assert a.group_relay == b.group_relay and a.count == b.count and a.by_stream == b.by_stream


# ------------------------------------------------------------------ cases
K = cc.K


def rule_streams():
    """A message in front of the terminal frame, one at it and one behind it:
    invalid text (1007), a protocol violator, a clean close, max_message
    (protocol_cases.EVERY_CODE_LIMIT) exceeded, and clean streams."""
    f, F = pc.frame, pc.FIN
    hello = f(F | pc.TEXT, "grüß dich".encode(), K)
    return [[hello, f(F | pc.TEXT, b"bad \xff text", 3), f(F | pc.TEXT, b"behind", 4)],
            [hello, f(F | pc.PING, b"pp", 5), f(F | pc.TEXT | 0x40, b"rsv", 6), hello],
            [f(F | pc.BINARY, b"\xff\xfe", 7), pc.close(1000, b"bye", 8), hello],
            [hello, f(pc.BINARY, b"z" * 60, 9), f(pc.CONT, b"z" * 40, 10), f(F | pc.CONT, b"z", 11), hello],
            [],
            [f(pc.TEXT, b"frag", 12), f(pc.CONT, b"", 13), f(F | pc.CONT, b"ments", 14), f(F | pc.PONG, b"", 15),
             f(F | pc.PING, b"q" * 125, 16), f(pc.TEXT, b"tail", 17)],
            [pc.close(3000, b"", 18)]]


def header_form_streams(rng):
    """Payloads of 0, 1, 125, 126, 127, 65535 and 65536 bytes, each behind a
    filler message of 0..15 bytes, so that its relay frame starts at every
    phase mod 16 of d_relay (stream k: phase k; one room, identity order)."""
    streams, at = [], 0
    for phase in range(16):
        frames = []
        for n in (0, 1, 125, 126, 127, 65535, 65536):
            pad = (phase - at - 2) % 16   # a text frame of `pad` bytes: pad + 2 on the relay
            frames.append(mc.raw_frame(0x81, b"f" * pad, key=int(rng.integers(1, 2 ** 32))))
            frames.append(mc.raw_frame(0x82, rc.data(rng, n), key=int(rng.integers(1, 2 ** 32))))
            at += pad + 2
            assert at % 16 == phase
            at += layout.frame_size(0x82, False, n)
        streams.append(frames)
    return streams


def piece_edge_streams(rng, phase):
    """Payloads of 4095, 4096, 4097 and 3 * 4096 + 5 bytes whose relay
    payloads start at ``phase`` mod 128 of d_relay (the gather cuts pieces at
    the destination's 128-byte lines), each behind two filler messages."""
    frames, at = [], 0
    for n in (4095, 4096, 4097, 3 * 4096 + 5):
        want = (phase - at - 4) % 128       # relay bytes of the fillers, mod 128 (the big frame's header: 4)
        a = next(a for a in (60, 58, 56) if (want - a - 4) % 128 <= 125)
        for pad in (a, (want - a - 4) % 128):
            frames.append(mc.raw_frame(0x82, b"p" * pad, key=int(rng.integers(1, 2 ** 32))))
            at += pad + 2
        assert (at + 4) % 128 == phase
        frames.append(mc.raw_frame(0x82, rc.data(rng, n), key=int(rng.integers(1, 2 ** 32))))
        at += 4 + n
    return [frames]


def fragment_streams(rng):
    """A message of 1, 2 and 64 fragments, empty fragments, fragment
    boundaries on the chunk edges of the destination (4 bytes of header in
    front: fragments of 12, 16, 4096 - 16 ... bytes)."""
    return [rc.fragments(rng, 0x82, [300]) + rc.fragments(rng, 0x82, [7, 9]),
            rc.fragments(rng, 0x82, [int(x) for x in rng.integers(0, 40, 64)]),
            rc.fragments(rng, 0x82, [0, 5, 0, 0, 3, 0]) + rc.fragments(rng, 0x82, [0, 0]),
            rc.fragments(rng, 0x82, [12, 16, 4096 - 16, 16, 1, 15, 4096, 4096 + 16, 3])]


def many_streams(ns, rng):
    """ns streams of one 1-byte text message each."""
    return [[mc.raw_frame(0x81, bytes([65 + j % 26]), key=int(k))] for j, k in
            enumerate(rng.integers(1, 2 ** 32, ns))]


# ------------------------------------------------------------------ the chat loop
class Table(ac.Table):
    pass


def round_want(cases, wire, spans, st, proto, limit, rule):
    """A round of the loop under ``rule`` with mask 0: the Want of either mode
    over layout.frame_plan's table."""
    fs, sf, _, _ = layout.frame_plan(wire, spans)
    ns = len(sf) - 1
    state = np.zeros(ns, dtype=layout.STREAM_STATE)
    rfc = cases is ac
    state["ahead" if rfc else "opcode"] = st
    return validated_want(Table(wire, fs, sf), rule, 0, None, state, pc.SERVER, limit, proto, None, WHICH, rfc)


def model_step(cases, reply_op, relay_op, limit, rooms, log):
    """kc.drive's ``step`` over the model: the reply side is the cases' own
    model_step, the relay side layout.relay_plan over the same round; every
    round's Relay and message streams are appended to ``log``."""
    base = sl.model_step(reply_op, 0, limit, True) if cases is sl else ac.model_step(reply_op, 0, True)

    def step(wire, spans, st, proto, keys, frame_cap):
        r = base(wire, spans, st, proto, keys, frame_cap)
        w = round_want(cases, wire, spans, st, proto, limit, relay_op)
        ns = len(spans)
        m = model_relay(w, relay_op, rooms, ns)
        same_relay(m, joined(w.frames, w.msgs, ns, rooms))
        m.merged = merged_out(w.msgs, w.verdict, reply_op, r.reply, r.stream_reply, m.frame_of, ns)
        log.append(m)
        return r
    return step


def split_frames(data):
    """Unmasked or masked whole frames, back to back, as a list."""
    data, out, at = bytes(data), [], 0
    while at < len(data):
        rc_, rec = ca.header_unpack(data[at: at + 14])
        assert rc_ == 0
        size = int(rec["hdr_len"]) + int(rec["len"])
        out.append(data[at: at + size])
        at += size
    assert at == len(data)
    return out


def merged_out(msgs, verdict, reply_op, reply, stream_reply, frame_of, ns):
    """Per stream, what the connection would have been sent had its room been
    itself alone: its relay frames and its replies in message order, the close
    frame last.  With mask 0 this is wsg_reply_validated's output under the
    union of the two rules, which server_loop_cases.check_run can judge whole
    (its last stanza compares the data messages a connection gets back, and
    the chat rule answers none of them)."""
    out = []
    last = msgs["first_frame"].astype(np.int64) + msgs["nframes"] - 1
    for j in range(ns):
        mine = iter(split_frames(bytes(reply[int(stream_reply[j]): int(stream_reply[j + 1])])))
        v = verdict[j]
        parts = []
        for q in np.nonzero(msgs["stream"] == j)[0]:
            kind = int(msgs["kind"][q])
            if int(q) in frame_of:
                parts.append(frame_of[int(q)])
            elif kind and reply_op[kind] and (v == NONE or last[q] < v[2]):
                parts.append(next(mine))
        out.append(b"".join(parts + list(mine)))
    return out


def loop_rooms(n, seed=5):
    """5 rooms over n connections, one of them empty, in a random order."""
    rng = np.random.default_rng([n, seed])
    cuts = sorted(int(x) for x in rng.integers(1, n, 3))
    return Rooms(rng.permutation(n), [0, cuts[0], cuts[1], cuts[1], cuts[2], n])


def per_connection(log):
    """Every connection's relay frames over all rounds, joined."""
    n = len(log[0].by_stream)
    return [b"".join(f for rnd in log for f in rnd.by_stream[j]) for j in range(n)]


def check_loop(log, rooms, one_call_frames, min_conns=128, min_msgs=200):
    """A run's per-round Relays against the one-call run over the whole
    connections, and the conditions that keep the check from passing on nothing."""
    got = per_connection(log)
    n = len(got)
    for j in range(n):
        assert got[j] == b"".join(one_call_frames[j]), "connection %d" % j
    relaying = sum(1 for j in range(n) if got[j])
    messages = sum(len(rnd.by_stream[j]) for rnd in log for j in range(n))
    print("relaying connections", relaying, "relayed messages", messages, "rounds", len(log))
    assert relaying >= min_conns and messages >= min_msgs
    b = rooms.bounds(n)
    for g in range(len(b) - 1):
        if b[g + 1] > b[g]:
            assert any(rnd.group_relay[g + 1] > rnd.group_relay[g] for rnd in log), "room %d relays in no round" % g
    for rnd in log:   # every group range is its members' frames in order
        pos = rooms.positions(n)
        for g in range(len(b) - 1):
            want = b"".join(f for p in range(b[g], b[g + 1]) for f in rnd.by_stream[pos[p]])
            assert rnd.relay[rnd.group_relay[g]: rnd.group_relay[g + 1]] == want, "room %d" % g
