"""Shared by tests/test_checked_reply_model.py (CPU) and
tests/test_gpu_checked_reply.py: what wsg_reply_checked must write, built
without layout.checked_reply_plan / merge_verdicts / utf8_verdicts.

The protocol's verdicts come from layout.protocol_plan and are merged with a
d_also by a plain loop over the streams.  Per stream one oracle session is fed
the frames in front of the terminal frame only (all of them without a
verdict); it supplies the callbacks, reply_cases.reply_frame their frames, and
oracle.Session(key).prepare_send(0x88, mask, b"", status) the close frame.
No test lives here."""
import bisect

import numpy as np

import oracle
from cppserver_amd import layout
from cppserver_amd.layout import PROTO_VERDICT
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import reply_cases as rc

U64_MAX = 2 ** 64 - 1
NONE = (0xFF, 0xFFFF, 0xFFFFFFFF)


def verdict_array(tuples):
    """[(code, status, frame) or NONE] -> PROTO_VERDICT records."""
    v = np.zeros(len(tuples), dtype=PROTO_VERDICT)
    for j, (code, status, frame) in enumerate(tuples):
        v[j] = (code, 0xFF if (code, status, frame) == NONE else 0, status, frame)
    return v


def verdict_tuples(v):
    v = np.asarray(v, dtype=PROTO_VERDICT)
    return [(int(r["code"]), int(r["status"]), int(r["frame"])) for r in v]


def merged(proto, also, stream_first):
    """The effective verdicts, one stream after the other (tuples)."""
    out = []
    for j, p in enumerate(proto):
        a = NONE if also is None else also[j]
        lo, hi = int(stream_first[j]), int(stream_first[j + 1])
        if a == NONE or not lo <= a[2] < hi:
            out.append(p)
        elif p == NONE or a[2] < p[2]:
            out.append(a)
        elif a[2] == p[2] and p[0] == 1 and a[0] >= 2:   # a violation beats a clean close
            out.append(a)
        else:
            out.append(p)
    return out


def utf8_also(msgs, buf, which, n_streams):
    """wsg_check_utf8 + wsg_utf8_verdicts as a loop over the records: per
    stream the first selected message that is not valid UTF-8 (tuples)."""
    out = [NONE] * n_streams
    for m in msgs:
        kind, op, j = int(m["kind"]), int(m["opcode"]), int(m["stream"])
        sel = bool(which & 4) or (bool(which & 1) and kind == 1 and op == 1) or (bool(which & 2) and kind == 2)
        if not sel or out[j] != NONE:
            continue
        data = np.asarray(buf)[int(m["off"]):][: int(m["len"])].tobytes()
        try:
            data.decode("utf-8")
        except UnicodeDecodeError:
            out[j] = (13, 1007, int(m["first_frame"]) + int(m["nframes"]) - 1)
    return out


class Want:
    """Everything one wsg_reply_checked call must leave."""


def expected(batch, rule=rc.ECHO, mask=0, keys=None, state=None, role=pc.ANY, max_message=0, proto_in=None,
             also=None, wire=None):
    """``batch``: a messages_cases.Batch; ``also``: tuples per stream or None;
    ``wire``: a damaged copy of the batch's wire (then no session is
    consulted: the callbacks come from message_plan over the oracle's records
    of that wire, as tests/test_gpu_reply.py::run_damaged takes them)."""
    w = Want()
    n, ns = batch.n, batch.n_streams
    damaged = wire is not None
    wire = batch.wire if wire is None else wire
    w.rc, out_o, w.info = oracle.decode_batch(wire, batch.fs)
    assert damaged or w.rc == 0
    w.msgs, w.count, w.state = layout.message_plan(w.info, batch.stream_first, state, payload=out_o)
    pin = None
    if proto_in is not None:
        pin = np.zeros(ns, dtype=layout.PROTO_STATE)
        for j, (nbytes, is_open) in enumerate(proto_in):
            pin[j] = (nbytes, is_open, 0)
    pv, w.proto, _ = layout.protocol_plan(w.info, batch.stream_first, pin, role, max_message, wire,
                                          consumed=w.state["consumed"])
    w.verdict = merged(verdict_tuples(pv), also, batch.stream_first)
    bad = [j for j, v in enumerate(w.verdict) if v != NONE and v[0] >= 2]
    w.result = [len(bad), bad[0] if bad else U64_MAX, sum(1 for v in w.verdict if v[0] == 1)]
    # the callbacks in front of each stream's terminal frame
    fin = w.msgs["first_frame"].astype(np.int64) + w.msgs["nframes"] - 1
    frames = [b""] * len(w.msgs)
    if damaged:
        buf = mc.dense(out_o, w.info, batch.stream_first, w.state)
        every = rc.plan_replies(w.msgs, buf, rule, mask, keys)
        for q, m in enumerate(w.msgs):
            v = w.verdict[int(m["stream"])]
            if v == NONE or fin[q] < v[2]:
                frames[q] = every[q]
    else:
        ops = rc.event_opcodes(w.info, batch.stream_first, state)
        of_stream = [[] for _ in range(ns)]
        for q in range(len(w.msgs)):
            of_stream[int(w.msgs["stream"][q])].append(q)
        for j, fr in enumerate(batch.streams):
            v = w.verdict[j]
            lo = int(batch.stream_first[j])
            ref = oracle.Session()
            if state is not None and int(state["opcode"][j]):
                ref.prepare_receive(mc.raw_frame(int(state["opcode"][j]), b""))
            ev = mc.session_events(fr if v == NONE else fr[: v[2] - lo], ref)
            key = int(keys[j]) if keys is not None else 0
            mine = [q for q in of_stream[j] if int(w.msgs["kind"][q]) and (v == NONE or fin[q] < v[2])]
            assert len(mine) == len(ev), "stream %d: %d messages in front of the terminal frame, %d callbacks" % (
                j, len(mine), len(ev))
            for q, o, e in zip(mine, ops[j], ev):
                assert rc.KINDS[o] == e[0] == int(w.msgs["kind"][q])
                frames[q] = rc.reply_frame(rule, mask, key, e[0], o, e[1], e[2])
    w.frames = frames
    # replies at their FIN frames and close frames at their terminal frames, in frame order
    items = [(int(fin[q]), 0, frames[q]) for q in range(len(frames))]
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
        """Reply bytes that belong to frames in front of frame k."""
        return int(ends[bisect.bisect_left(at, k)])

    w.reply_off = [before(int(f)) for f in fin] + [len(w.reply)]
    w.stream_reply = [before(int(batch.stream_first[j])) for j in range(ns)] + [len(w.reply)]
    w.close_off = [before(v[2]) if v != NONE else U64_MAX for v in w.verdict]
    nclose = sum(1 for v in w.verdict if v != NONE)
    w.rcount = [len(w.reply), sum(1 for f in frames if f) + nclose, nclose]
    w.by_stream = [w.reply[w.stream_reply[j]: w.stream_reply[j + 1]] for j in range(ns)]
    assert len(w.reply) <= len(wire) + 14 * n   # wsg_capi.h's bound: the unanswered frames pay for the close frame
    return w


def check_model(w, batch, rule, mask, keys, also):
    """layout.merge_verdicts / checked_reply_plan against a Want."""
    eff = verdict_array(w.verdict)
    reply_off, stream_reply, close_off, count = layout.checked_reply_plan(w.msgs, eff, rule, mask, keys,
                                                                          n_streams=batch.n_streams)
    assert [int(x) for x in reply_off] == w.reply_off
    assert [int(x) for x in stream_reply] == w.stream_reply
    assert [int(x) for x in close_off] == w.close_off
    assert [int(x) for x in count] == w.rcount


# ------------------------------------------------------------------ cases
K = 0x1F2E3D4C


def code_streams():
    """name -> (frames, the terminal frame's index in the stream, code,
    status): codes 3-12 and the clean closes, as a server with max_message =
    protocol_cases.EVERY_CODE_LIMIT, the terminal frame first, in the middle
    or last, with messages behind it."""
    f, F = pc.frame, pc.FIN
    ok = [f(F | pc.TEXT, b"hello", K), f(F | pc.PING, b"pp", K)]
    return {
        "rsv_first": ([f(F | pc.TEXT | 0x40, b"compressed?", K)] + ok, 0, 3, 1002),
        "opcode_middle": (ok + [f(F | 0x3, b"", K)] + ok, 2, 4, 1002),
        "mask_last": (ok + [f(F | pc.TEXT, b"plain")], 2, 5, 1002),
        "ctrl_fragment": (ok + [f(pc.PING, b"", K), f(F | pc.BINARY, b"behind", K)], 2, 6, 1002),
        "ctrl_long": ([f(F | pc.PING, b"p" * 126, K)] + ok, 0, 7, 1002),
        "cont": (ok + [f(F | pc.CONT, b"nothing to continue", K)] + ok, 2, 8, 1002),
        "data": ([f(pc.TEXT, b"open", K), f(F | pc.BINARY, b"interloper", K)] + ok, 1, 9, 1002),
        "close_len": (ok + [f(F | pc.CLOSE, b"\x03", K)], 2, 10, 1002),
        "close_code": ([pc.close(1005, b"", K)] + ok, 0, 11, 1002),
        "too_big": ([f(pc.BINARY, b"z" * 60, K), f(pc.CONT, b"z" * 40, K), f(F | pc.CONT, b"z", K)] + ok, 2, 12, 1009),
        "closed_1000": (ok + [pc.close(1000, b"bye", K)] + ok, 2, 1, 1000),
        "closed_3000": ([pc.close(3000, b"", K)], 0, 1, 3000),
        "closed_empty": (ok + [pc.close(None, key=K)], 2, 1, 1005),
        # the terminal frame in the tail of a stream with no message at all
        "tail_rsv": ([f(pc.TEXT | 0x20, b"never finished", K)], 0, 3, 1002),
        # ... and inside a fragmented message whose FIN arrives later: unanswered
        "inside_fragments": (ok + [f(pc.TEXT, b"a", K), f(F | pc.PING | 0x10, b"", K), f(F | pc.CONT, b"b", K)] + ok,
                             3, 3, 1002),
    }


def clean_streams():
    f, F = pc.frame, pc.FIN
    return [[f(F | pc.TEXT, b"hello", K)], [],
            [f(pc.TEXT, b"a" * 40, K), f(F | pc.PING, b"p", K), f(pc.CONT, b"b" * 40, K), f(F | pc.CONT, b"c" * 20, K)],
            [f(F | pc.BINARY, b"q" * 90, K), f(pc.BINARY, b"tail", K)]]


def code_batch():
    """Every code_streams() stream among clean ones; returns (batch, names,
    first stream index of each name)."""
    cs = code_streams()
    clean = clean_streams()
    streams, at = [], {}
    for k, name in enumerate(sorted(cs)):
        streams.append(clean[k % len(clean)])
        at[name] = len(streams)
        streams.append(cs[name][0])
    streams.append(clean[0])
    return mc.Batch(streams), at


def fuzz_batch(seed):
    """(batch, role, max_message, proto_in, state): protocol_cases.fuzz's
    streams (valid next frames with violations mixed in), every frame whole."""
    streams, role, limit, proto_in = pc.fuzz(seed)
    rng = np.random.default_rng(1000 + seed)
    state = np.zeros(len(streams), dtype=layout.STREAM_STATE)
    state["opcode"] = rng.choice([0, 0, 1, 2, 9], len(streams))
    return mc.Batch(streams), role, limit, proto_in, state


def tiny_fuzz_batch(seed):
    """test_gpu_reply._tiny_streams' kind with random opcodes, RSV bits and
    masks: most streams end at a violation within a few frames."""
    rng = np.random.default_rng(seed)
    n, ns = int(rng.integers(1, 120)), int(rng.integers(1, 9))
    frames = []
    for _ in range(n):
        op = int(rng.choice([0, 1, 2, 9, 10, 8, 3], p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05]))
        fin = 0x80 if rng.random() < 0.6 else 0
        rsv = int(rng.choice([0x10, 0x20, 0x40])) if rng.random() < 0.03 else 0
        body = rc.data(rng, int(rng.integers(0, 9)))
        if op == 8 and rng.random() < 0.7:
            body = int(rng.choice([1000, 1001, 3000, 1005, 999])).to_bytes(2, "big") + body[:3]
        key = int(rng.integers(0, 2**32)) if rng.random() < 0.85 else None
        frames.append(mc.raw_frame(fin | rsv | op, body, key=key))
    cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, ns - 1)), [n]])
    return mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(ns)])
