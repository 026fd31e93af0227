"""Shared by tests/golden/make_rfc6455_messages.py, tests/test_rfc_assembly_model.py
(CPU), tests/test_gpu_rfc_assembly.py and tests/test_gpu_rfc_loop.py: streams
with control frames between the fragments of their messages, what every call
that honours WSG_ASSEMBLY_RFC must write for them, the connections of the
fixture tests/golden/rfc6455_messages.json and a cut-read loop over them.

expected() is built on layout.message_plan(assembly=RFC), the model the issue
names; what checks the model itself is the recorded outside reader (the
fixture), Python's strict UTF-8 decoder and the oracle's sessions, which make
every reply frame's bytes.  No test lives here."""
import bisect
import functools
import json
import os

import numpy as np

import oracle
from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import reply_cases as rc
from tests import server_loop_cases as sl

RFC, REFERENCE = layout.ASSEMBLY_RFC, layout.ASSEMBLY_REFERENCE
NONE, U64_MAX = cc.NONE, cc.U64_MAX
WHICH = layout.UTF8_TEXT | layout.UTF8_CLOSE
f, F = pc.frame, pc.FIN
K = 0x1F2E3D4C
CTL_SIZES = (0, 1, 125)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfc6455_messages.json")
SEED = 5420                  # see make_rfc6455_messages.py: the caps hold under it
N_CONNECTIONS = 200
CAP_INTERLEAVED, CAP_CLASSES = 0.25, 0.05


# ------------------------------------------------------------------ streams
def fragmented(rng, op, parts, gaps, text=True):
    """One message of `parts` fragments with the frames of gaps[g] (a list)
    between fragment g and g + 1."""
    size = int(rng.integers(parts, 40 * parts))
    data = sl.utf8_text(rng, size) if op == pc.TEXT and text else rc.data(rng, size)
    out = []
    for i, p in enumerate(sl.split(rng, data, parts)):
        out.append(f((F if i == parts - 1 else 0) | (op if i == 0 else pc.CONT), p, K + i))
        if i < parts - 1:
            out += gaps.get(i, [])
    return out


def interleaved_streams():
    """Pings and pongs of 0, 1 and 125 bytes at every gap of 2- to 5-fragment
    text and binary messages: one stream with a control frame in every gap per
    (parts, opcode, control, size), one per single gap, each with a message
    behind it."""
    rng = np.random.default_rng(1)
    behind = [f(F | pc.TEXT, b"behind", 7)]
    out = []
    for parts in (2, 3, 4, 5):
        for op in (pc.TEXT, pc.BINARY):
            for ctl in (pc.PING, pc.PONG):
                for size in CTL_SIZES:
                    gaps = {g: [f(F | ctl, rc.data(rng, size), 90 + g)] for g in range(parts - 1)}
                    out.append(fragmented(rng, op, parts, gaps) + behind)
            for g in range(parts - 1):
                out.append(fragmented(rng, op, parts, {g: [f(F | pc.PING, b"one", 3), f(F | pc.PONG, b"", 4)]}))
    return out


def special_streams():
    """name -> frames: a close between fragments, UTF-8 sequences cut across
    two fragments with a ping in the cut whose payload would complete or break
    them, the Autobahn shapes 5.3-5.8 and 5.19/5.20, frame errors' stand-ins
    (non-FIN control frames, reserved opcodes) inside a run, runs left open."""
    ping, pong = F | pc.PING, F | pc.PONG
    euro = "€".encode()                   # e2 82 ac
    smile = "\U0001F600".encode()         # f0 9f 98 80
    return {
        "close_between": [f(pc.TEXT, b"ab", 1), pc.close(1000, b"bye", 2), f(F | pc.CONT, b"cd", 3)],
        "close_empty_between": [f(pc.BINARY, b"ab", 1), pc.close(None, key=2), f(F | pc.CONT, b"cd", 3)],
        "cut_completed_by_ping": [f(pc.TEXT, b"ab" + euro[:1], 1), f(ping, euro[1:], 2), f(F | pc.CONT, euro[1:] + b"!", 3)],
        "cut_broken_by_ping": [f(pc.TEXT, smile[:2], 1), f(ping, b"\xff\xfe", 2), f(F | pc.CONT, smile[2:], 3)],
        "cut_ping_is_the_rest": [f(pc.TEXT, euro[:2], 1), f(ping, euro[2:], 2), f(F | pc.CONT, b"x", 3),
                                 f(F | pc.TEXT, b"after", 4)],
        "cut_twice": [f(pc.TEXT, smile[:1], 1), f(ping, smile[1:], 2), f(pc.CONT, smile[1:3], 3), f(pong, smile[3:], 4),
                      f(F | pc.CONT, smile[3:], 5)],
        "autobahn_5_3": [f(pc.TEXT, b"fragment1", 1), f(F | pc.CONT, b"fragment2", 2)],
        "autobahn_5_5": [f(pc.BINARY, b"fragment1", 1), f(F | pc.CONT, b"fragment2", 2)],
        "autobahn_5_6": [f(pc.TEXT, b"fragment1", 1), f(ping, b"ping", 2), f(F | pc.CONT, b"fragment2", 3)],
        "autobahn_5_7": [f(pc.TEXT, b"fragment1", 1), f(ping, b"", 2), f(F | pc.CONT, b"fragment2", 3)],
        "autobahn_5_8": [f(pc.BINARY, b"fragment1", 1), f(pong, b"unsolicited", 2), f(ping, b"ping", 3),
                         f(F | pc.CONT, b"fragment2", 4)],
        "autobahn_5_19": [f(pc.TEXT, b"fragment1", 1), f(pc.CONT, b"fragment2", 2), f(ping, b"pongme 1!", 3),
                          f(pc.CONT, b"fragment3", 4), f(pc.CONT, b"fragment4", 5), f(ping, b"pongme 2!", 6),
                          f(F | pc.CONT, b"fragment5", 7)],
        "autobahn_5_20": [f(pc.BINARY, b"fragment1", 1), f(pc.CONT, b"fragment2", 2), f(ping, b"pongme 1!", 3),
                          f(pc.CONT, b"fragment3", 4), f(pc.CONT, b"fragment4", 5), f(ping, b"pongme 2!", 6),
                          f(F | pc.CONT, b"fragment5", 7), f(F | pc.TEXT, b"next", 8)],
        "nonfin_control_inside": [f(pc.TEXT, b"ab", 1), f(pc.PING, b"never delivered", 2), f(ping, b"x", 3),
                                  f(F | pc.CONT, b"cd", 4)],
        "reserved_inside": [f(pc.TEXT, b"ab", 1), f(F | 0xB, b"rsv ctl", 2), f(0x3, b"joins", 3), f(F | pc.CONT, b"cd", 4)],
        "open_run": [f(F | pc.TEXT, b"done", 1), f(pc.TEXT, b"ab", 2), f(ping, b"x", 3), f(pong, b"y", 4), f(pc.CONT, b"c", 5)],
        "controls_only": [f(ping, b"a", 1), f(pong, b"b", 2), f(ping, b"", 3)],
        "cont_only_run": [f(pc.CONT, b"no opcode", 1), f(ping, b"p", 2), f(F | pc.CONT, b"at all", 3)],
        "empty": [],
    }


def random_frames(rng, p_interleave=0.35, count=None):
    """server_loop_cases._random_frames with interleaving common: 0-40 frames,
    each a valid next frame with probability about 0.9 and one of
    protocol_cases.fuzz's violations otherwise; every frame masked."""
    count = int(40 * rng.random() ** 3 + rng.random()) if count is None else count
    frames, plan, is_open = [], [], False

    def key():
        return int(rng.integers(1, 2 ** 32))

    def control():
        if rng.random() < 0.08:
            return pc.close(int(rng.choice([1000, 1001, 3000])), sl.utf8_text(rng, int(rng.integers(0, 12))), key())
        return f(F | int(rng.choice([pc.PING, pc.PONG])), rc.data(rng, int(rng.choice([0, 1, 5, 125]))), key())

    while len(frames) < count:
        body = rc.data(rng, int(rng.integers(0, 301)))
        if rng.random() < 0.9:
            if is_open:
                if rng.random() < p_interleave:
                    frames.append(control())
                    continue
                part = plan.pop(0)
                is_open = bool(plan)
                frames.append(f((0 if is_open else F) | pc.CONT, part, key()))
                continue
            pick = rng.random()
            if pick < 0.15:
                frames.append(control())
            else:
                op = int(rng.choice([pc.TEXT, pc.BINARY]))
                parts = 1 if rng.random() < 0.3 else int(rng.integers(2, 6))
                total = int(rng.integers(0, 301)) if parts == 1 else int(rng.integers(0, 120 * parts))
                at = None
                if op == pc.TEXT:
                    data = sl.utf8_text(rng, total)
                    if rng.random() < 0.08:
                        data, at = sl.corrupted(rng, data)
                else:
                    data = rc.data(rng, total)
                pieces = [p[:300] for p in sl.split(rng, data, parts, at)]
                plan = pieces[1:]
                is_open = bool(plan)
                frames.append(f((0 if is_open else F) | op, pieces[0], key()))
        else:
            bad = int(rng.integers(0, 8))
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
                frames.append(pc.close(int(rng.choice(sl.BAD_STATUSES)), b"", key()))
            else:
                frames.append(f(F | pc.TEXT | 0x40, body, key()))
    return frames


def fuzz(seed):
    """(batch, role, max_message, proto_in, state): protocol_cases.fuzz's
    streams for even seeds, random_frames' (interleaving common) for odd
    ones; the state's ahead is 0, 1, 2 or more than any stream holds."""
    rng = np.random.default_rng(7000 + seed)
    if seed & 1:
        streams = [random_frames(rng) for _ in range(int(rng.integers(1, 24)))]
        role, limit, proto_in = pc.SERVER, int(rng.choice([0, 0, 200, 1000])), None
    else:
        streams, role, limit, proto_in = pc.fuzz(seed)
    state = np.zeros(len(streams), dtype=layout.STREAM_STATE)
    state["ahead"] = rng.choice([0, 0, 1, 2, 60000], len(streams))
    state["opcode"] = rng.choice([0, 1, 9], len(streams))   # ignored on input
    return mc.Batch(streams), role, limit, proto_in, state


# ------------------------------------------------------------------ what a call must write
def dense(out, info, msgs):
    """The message buffer: every message's frames' unmasked payloads, back to back."""
    parts = [out[int(info["payload_off"][i]):][: int(info["len"][i])]
             for frames in layout.message_frames(info, msgs, RFC) for i in frames]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def word(v):
    return U64_MAX if v == NONE else v[0] | v[1] << 16 | v[2] << 32


def effective_also(utf8, also, stream_first):
    """The UTF-8 verdict, the caller's entry where it names a frame of the
    stream, the lower word where both exist (wsg_reply_validated's d_also')."""
    out = []
    for j, u in enumerate(utf8):
        a = NONE if also is None else also[j]
        if a != NONE and not int(stream_first[j]) <= a[2] < int(stream_first[j + 1]):
            a = NONE
        out.append(a if word(a) < word(u) else u)
    return out


def expected(batch, rule=rc.ECHO, mask=0, keys=None, state=None, role=pc.ANY, max_message=0, proto_in=None, also=None,
             which=None, ahead_cap=layout.AHEAD_CAP, checked=True):
    """A checked_reply_cases.Want under WSG_ASSEMBLY_RFC.  ``which`` not None:
    wsg_reply_validated (the UTF-8 verdicts by Python's strict decoder, merged
    with ``also``; w.valid and w.utf8_result by layout.utf8_plan).  ``checked``
    False: no verdict at all, as wsg_reply_messages answers."""
    w = cc.Want()
    n, ns = batch.n, batch.n_streams
    w.rc, out_o, w.info = oracle.decode_batch(batch.wire, batch.fs)
    assert w.rc == 0
    w.msgs, w.count, w.state = layout.message_plan(w.info, batch.stream_first, state, payload=out_o, assembly=RFC,
                                                   ahead_cap=ahead_cap)
    w.buf = dense(out_o, w.info, w.msgs)
    assert int(w.count[1]) == len(w.buf)
    pin = None
    if proto_in is not None:
        pin = np.zeros(ns, dtype=layout.PROTO_STATE)
        for j, (nbytes, is_open) in enumerate(proto_in):
            pin[j] = (nbytes, is_open, 0)
    pv, w.proto, _ = layout.protocol_plan(w.info, batch.stream_first, pin, role, max_message, batch.wire,
                                          consumed=w.state["consumed"])
    if which is not None:
        also = effective_also(cc.utf8_also(w.msgs, w.buf, which, ns), also, batch.stream_first)
        w.valid, w.utf8_result = layout.utf8_plan(w.msgs, w.buf, which)
    w.verdict = cc.merged(cc.verdict_tuples(pv), also, batch.stream_first) if checked else [NONE] * ns
    bad = [j for j, v in enumerate(w.verdict) if v != NONE and v[0] >= 2]
    w.result = [len(bad), bad[0] if bad else U64_MAX, sum(1 for v in w.verdict if v[0] == 1)]
    fin = w.msgs["first_frame"].astype(np.int64) + w.msgs["nframes"] - 1
    every = rc.plan_replies(w.msgs, w.buf, rule, mask, keys)
    w.frames = [fr if w.verdict[int(m["stream"])] == NONE or fin[q] < w.verdict[int(m["stream"])][2] else b""
                for q, (m, fr) in enumerate(zip(w.msgs, every))]
    items = [(int(fin[q]), 0, w.frames[q]) for q in range(len(w.frames))]
    w.close = [b""] * ns
    for j, v in enumerate(w.verdict):
        if v != NONE:
            key = int(keys[j]) if keys is not None else 0
            w.close[j] = oracle.Session(key).prepare_send(0x88, mask, b"", 1000 if v[1] == 1005 else v[1])
            items.append((v[2], 1, w.close[j]))
    items.sort(key=lambda it: (it[0], it[1]))
    w.reply = b"".join(it[2] for it in items)
    at = [it[0] for it in items]
    ends = np.concatenate([[0], np.cumsum([len(it[2]) for it in items], dtype=np.int64)])

    def before(k):
        return int(ends[bisect.bisect_left(at, k)])

    w.reply_off = [before(int(x)) for x in fin] + [len(w.reply)]
    w.stream_reply = [before(int(batch.stream_first[j])) for j in range(ns)] + [len(w.reply)]
    w.close_off = [before(v[2]) if v != NONE else U64_MAX for v in w.verdict]
    nclose = sum(1 for v in w.verdict if v != NONE)
    w.rcount = [len(w.reply), sum(1 for fr in w.frames if fr) + nclose, nclose]
    w.by_stream = [w.reply[w.stream_reply[j]: w.stream_reply[j + 1]] for j in range(ns)]
    assert len(w.reply) <= len(batch.wire) + 14 * n
    return w


def plain_replies(w, rule, mask, keys, ns):
    """wsg_reply_messages' outputs from a Want made without any verdict."""
    sizes = [len(fr) for fr in w.frames]
    reply_off = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]
    per = np.zeros(ns + 1, dtype=np.int64)
    for m, s in zip(w.msgs, sizes):
        per[int(m["stream"]) + 1] += s
    return b"".join(w.frames), reply_off, [int(x) for x in np.cumsum(per)], [sum(sizes), sum(1 for s in sizes if s)]


# ------------------------------------------------------------------ the fixture's connections
@functools.lru_cache(maxsize=None)
def connections():
    """Named streams first, random ones behind them, as server_loop_cases.Conn."""
    out = [sl.Conn(name, frames) for name, frames in special_streams().items()]
    out += [sl.Conn("interleaved%d" % k, frames) for k, frames in enumerate(interleaved_streams()[::3])]
    rng = np.random.default_rng(SEED)
    while len(out) < N_CONNECTIONS:
        frames = random_frames(rng, p_interleave=0.15)
        tail = b""
        if rng.random() < 0.1:
            whole = f(F | pc.PING, rc.data(rng, int(rng.integers(0, 126))), 11)
            tail = whole[: int(rng.integers(1, len(whole)))]
        out.append(sl.Conn("random%d" % len(out), frames, tail))
    return out


def send_keys():
    return np.random.default_rng(SEED + 2).integers(0, 2 ** 32, N_CONNECTIONS).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def whole_batch():
    return mc.Batch([c.frames for c in connections()])


@functools.lru_cache(maxsize=None)
def one_call(validating, rule, mask):
    """Every whole connection as one stream of one call, as a server."""
    return expected(whole_batch(), rule, mask, send_keys() if mask else None, role=pc.SERVER,
                    which=WHICH if validating else None)


def has_interleaving(frames):
    """A FIN control frame between the fragments of a message (by the frame rules' walk)."""
    b = pc.Batch([frames])
    is_open, nbytes = False, 0
    for i in range(b.n):
        if int(b.info["opcode"][i]) & 8 and is_open:
            return True
        code, _, is_open, nbytes = pc.judge(b.info[i], b.wire, is_open, nbytes, pc.SERVER, 0)
        if code:
            return False
    return False


def model_events(conn_index, validating):
    """What the model delivers for one connection in front of its terminal
    frame: [[FIN frame within the connection, opcode, length, digest]], and the
    terminal (status, frame) or None."""
    w = one_call(validating, rc.SAME_CLOSE_PONG, 0)
    lo = int(whole_batch().stream_first[conn_index])
    v = w.verdict[conn_index]
    out = []
    for m in w.msgs[w.msgs["stream"] == conn_index]:
        fin = int(m["first_frame"]) + int(m["nframes"]) - 1
        if int(m["kind"]) and (v == NONE or fin < v[2]):
            data = w.buf[int(m["off"]):][: int(m["len"])].tobytes()
            out.append([fin - lo, int(m["opcode"]), len(data), sl.digest(data)])
    return out, (None if v == NONE else (v[1], v[2] - lo))


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


# ------------------------------------------------------------------ the loop over cut reads
def schedule(seed):
    """Per connection its read sizes, one per round, then everything left."""
    rng = np.random.default_rng([SEED, seed])
    out = []
    for j in range(N_CONNECTIONS):
        sizes = []
        while len(sizes) < 6 + (j + seed) % 10:
            pick = int(rng.integers(0, 12))
            if pick == 11:
                break
            sizes.append(pick if pick < 4 else int(rng.integers(4, 701)))
        out.append(sizes + [sl.REST])
    return out


def drive(step, seed, keys=None):
    """server_loop_cases.drive over connections(), carrying d_state[j].ahead
    where that carries the opcode.  ``step(wire, spans, ahead, proto, keys,
    frame_cap)`` returns a server_loop_cases.Step with .ahead for .opcode."""
    conns, reads = connections(), schedule(seed)
    n = len(conns)
    rng = np.random.default_rng([SEED, seed, 1])
    run = sl.Run()
    run.out, run.verdict = [bytearray() for _ in range(n)], [NONE] * n
    run.proto, run.ahead, run.left, run.rounds, run.max_streams = [(0, 0)] * n, [0] * n, [b""] * n, 0, 0
    run.carried_ahead = 0
    pos, pending, frames_done, rounds_of = [0] * n, [b""] * n, [0] * n, [0] * n
    live = list(range(n))
    while live:
        assert run.rounds < sl.MAX_ROUNDS, "the loop does not end"
        chunks, spans, at = [], np.zeros(len(live), dtype=layout.STREAM_SPAN), 0
        for s, j in enumerate(live):
            size = reads[j][rounds_of[j]]
            rounds_of[j] += 1
            new = conns[j].data[pos[j]:] if size == sl.REST else conns[j].data[pos[j]: pos[j] + size]
            pos[j] += len(new)
            pending[j] += new
            gap = rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes()
            chunks += [gap, pending[j]]
            spans["off"][s], spans["len"][s] = at + len(gap), len(pending[j])
            at += len(gap) + len(pending[j])
        chunks.append(bytes(64))
        wire = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
        frame_cap = len(wire) // 2 + 1
        r = step(wire, spans, np.array([run.ahead[j] for j in live], dtype=np.uint16), [run.proto[j] for j in live],
                 None if keys is None else keys[live], frame_cap)
        run.rounds += 1
        run.max_streams = max(run.max_streams, len(live))
        still = []
        for s, j in enumerate(live):
            run.out[j] += bytes(r.reply[int(r.stream_reply[s]): int(r.stream_reply[s + 1])])
            v = r.verdict[s]
            assert (v != NONE) == (int(r.close_off[s]) != U64_MAX)
            if v != NONE:   # disconnected: its later bytes are never submitted
                run.verdict[j] = (v[0], v[1], v[2] - int(r.stream_first[s]) + frames_done[j])
                continue
            frames_done[j] += int(r.frames_consumed[s])
            pending[j] = pending[j][int(r.bytes_consumed[s]):]
            run.ahead[j], run.proto[j] = int(r.ahead[s]), (int(r.proto[s][0]), int(r.proto[s][1]))
            run.carried_ahead += run.ahead[j] > 0
            if pos[j] < len(conns[j].data):
                still.append(j)
            else:
                run.left[j] = pending[j]
        live = still
    run.out = [bytes(o) for o in run.out]
    return run


class Table:
    """A round's frame table as expected() reads a messages_cases.Batch (gaps lie between the spans)."""

    def __init__(self, wire, fs, stream_first):
        self.wire, self.fs, self.stream_first = wire, fs, np.asarray(stream_first).astype(np.int32)
        self.n, self.n_streams = len(fs), len(stream_first) - 1


def model_step(rule, mask, validating, ahead_cap=layout.AHEAD_CAP):
    """One round as layout.frame_plan and expected() give it."""
    def step(wire, spans, ahead, proto, keys, frame_cap):
        ns = len(spans)
        fs, sf, spans_out, count = layout.frame_plan(wire, spans)
        assert int(count[0]) <= frame_cap
        state = np.zeros(ns, dtype=layout.STREAM_STATE)
        state["ahead"] = ahead
        w = expected(Table(wire, fs, sf), rule, mask, keys, state, pc.SERVER, 0, proto, which=WHICH if validating else None,
                     ahead_cap=ahead_cap)
        r = sl.Step()
        r.reply, r.stream_reply, r.close_off = np.frombuffer(w.reply, dtype=np.uint8), w.stream_reply, w.close_off
        r.verdict, r.stream_first = w.verdict, sf
        r.frames_consumed, r.ahead = w.state["consumed"], w.state["ahead"]
        r.bytes_consumed = sl.lowered(fs, sf, spans["off"], spans_out["consumed"], w.state["consumed"])
        r.proto = [(int(p["bytes"]), int(p["open"])) for p in w.proto]
        return r
    return step


def check_run(run, validating, rule, mask, what):
    """One drive() against the one-call expectation: outputs, verdicts and
    carries; every ping in front of the terminal frame answered exactly once,
    its pong in front of the echo of the message it arrived in."""
    conns = connections()
    w = one_call(validating, rule, mask)
    sf = whole_batch().stream_first
    want = sl.local(w.verdict, sf)
    for j, c in enumerate(conns):
        where = "%s: connection %d (%s)" % (what, j, c.name)
        assert run.out[j] == w.by_stream[j], where
        assert run.verdict[j] == want[j], where
        if want[j] == NONE:
            assert run.proto[j] == (int(w.proto["bytes"][j]), int(w.proto["open"][j])), where
            assert run.ahead[j] == int(w.state["ahead"][j]), where
            assert run.left[j] == b"".join(c.frames[int(w.state["consumed"][j]):]) + c.tail, where
        if rule[3]:   # pings are answered: one pong per delivered ping, in the order of the FIN frames
            mine = w.msgs[w.msgs["stream"] == j]
            fin = mine["first_frame"].astype(np.int64) + mine["nframes"] - 1
            stop = 2 ** 62 if w.verdict[j] == NONE else w.verdict[j][2]
            answered = [int(m["kind"]) for m, e in zip(mine, fin) if e < stop and int(rule[int(m["kind"])])]
            got = [b0 & 0x0F for b0, _, _ in sl.unpack(run.out[j])]
            got = got[:-1] if w.verdict[j] != NONE else got
            assert len(got) == len(answered), where
            assert [g == pc.PONG for g in got] == [k == layout.CB_PING for k in answered], where
