"""Shared by tests/test_reply_model.py (CPU) and tests/test_gpu_reply.py: the
reply frames wsg_reply_messages must write, taken from the oracle's sessions,
and the batches both files use.  No test lives here."""
import numpy as np

import oracle
from cppserver_amd import layout
from cppserver_amd.layout import CB_CLOSE, REPLY_SAME, WS_FIN
from tests import messages_cases as mc

ECHO = layout.ECHO_REPLY
# every kind answered: text as text, binary as binary, a close with a close
# (status only), a ping with a pong, a pong with nothing
SAME_CLOSE_PONG = (0, REPLY_SAME, 0x88, 0x8A, 0)
NONE = (0, 0, 0, 0, 0)
# a pong answered too, and a received message with a ping (the prefix on data)
EVERYTHING = (0, 0x89, 0x88, 0x8A, REPLY_SAME)
RULES = {"echo": ECHO, "same_close_pong": SAME_CLOSE_PONG, "none": NONE, "everything": EVERYTHING}

KINDS = {1: 1, 2: 1, 8: 2, 9: 3, 10: 4}   # opcode -> WSG_CB_*
KEY4 = 0xD4C3B2A1                          # four distinct key bytes


def event_opcodes(info, stream_first, state=None):
    """Per stream, the _ws_opcode (ws.cpp:326: the last non-zero opcode, else
    the seed) at every FIN frame that fires a callback, from the oracle's
    RECV_INFO: the opcode WSG_REPLY_SAME answers with."""
    out = []
    for j in range(len(stream_first) - 1):
        op = int(state["opcode"][j]) if state is not None else 0
        ops = []
        for i in range(int(stream_first[j]), int(stream_first[j + 1])):
            op = int(info["opcode"][i]) or op
            if info["fin"][i] and op in KINDS:
                ops.append(op)
        out.append(ops)
    return out


def reply_frame(rule, mask, key, kind, opcode, data, status):
    """What a session with _ws_send_mask = key sends for one callback (b"": nothing)."""
    op = int(rule[kind])
    op = WS_FIN | opcode if op == REPLY_SAME else op
    if not op:
        return b""
    if kind == CB_CLOSE:
        return oracle.Session(key).prepare_send(op, mask, b"", status)
    return oracle.Session(key).prepare_send(op, mask, data, 0)


def oracle_replies(batch, rule, mask, keys=None, state=None):
    """Per stream, the reply frame of every callback one oracle session fires
    when it is fed the stream's frames (seeded as messages_cases.check_events
    seeds it; the frames of the tail fire nothing), in order."""
    _, info = batch.oracle_decode()
    ops = event_opcodes(info, batch.stream_first, state)
    out = []
    for j, frames in enumerate(batch.streams):
        ref = oracle.Session()
        if state is not None and int(state["opcode"][j]):
            ref.prepare_receive(mc.raw_frame(int(state["opcode"][j]), b""))
        ev = mc.session_events(frames, ref)
        assert len(ev) == len(ops[j]) and all(KINDS[o] == e[0] for o, e in zip(ops[j], ev)), "stream %d" % j
        key = int(keys[j]) if keys is not None else 0
        out.append([reply_frame(rule, mask, key, e[0], o, e[1], e[2]) for o, e in zip(ops[j], ev)])
    return out


def plan_replies(msgs, buf, rule, mask, keys=None):
    """One reply frame (or b"") per record of a message_plan table whose bytes
    are buf (messages_cases.dense): for damaged wires, where no session is
    consulted."""
    out = []
    for m in msgs:
        kind = int(m["kind"])
        key = int(keys[int(m["stream"])]) if keys is not None else 0
        data = np.asarray(buf)[int(m["off"]):][: int(m["len"])].tobytes()
        out.append(reply_frame(rule, mask, key, kind, int(m["opcode"]), data, int(m["status"])) if kind else b"")
    return out


def per_message(msgs, by_stream):
    """The per-stream reply lists laid against a message table: kind-0 records
    fire no callback and get b""."""
    at = [0] * len(by_stream)
    out = []
    for m in msgs:
        j = int(m["stream"])
        if int(m["kind"]) == 0:
            out.append(b"")
        else:
            out.append(by_stream[j][at[j]])
            at[j] += 1
    assert at == [len(s) for s in by_stream]
    return out


def check_plan(batch, rule, mask, keys=None, state=None):
    """layout.reply_plan over the message_plan table against the lengths of
    the oracle's frames; returns (msgs, msg count, new state, reply_off,
    stream_reply, reply count, reply bytes)."""
    msgs, count, new_state, buf, out, info = mc.check_model(batch, state)
    by_stream = oracle_replies(batch, rule, mask, keys, state)
    frames = per_message(msgs, by_stream)
    reply_off, stream_reply, rcount = layout.reply_plan(msgs, rule, mask, keys, n_streams=batch.n_streams)
    sizes = [len(f) for f in frames]
    assert [int(x) for x in reply_off] == [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]
    assert [int(x) for x in rcount] == [sum(sizes), sum(1 for s in sizes if s)]
    ends = np.cumsum([sum(len(f) for f in s) for s in by_stream])
    assert [int(x) for x in stream_reply] == [0] + [int(x) for x in ends]
    # wsg_capi.h's bound: a reply adds at most 16 bytes to its data, every frame spent 2 on its header
    assert sum(sizes) <= len(batch.wire) + 14 * batch.n
    return msgs, count, new_state, reply_off, stream_reply, rcount, b"".join(frames)


def data(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def header_form_stream(rng):
    """Single-frame messages at every header form of the reply: binary of
    0..65536 bytes, pings whose +2 prefix crosses 125/126 and 65535/65536."""
    frames = [mc.raw_frame(0x82, data(rng, n), key=int(rng.integers(1, 2**32)))
              for n in (0, 1, 125, 126, 127, 65535, 65536)]
    frames += [mc.raw_frame(0x89, data(rng, n), key=int(rng.integers(1, 2**32)))
               for n in (0, 1, 123, 124, 125, 65533, 65534)]
    return frames


def fragments(rng, b0, sizes):
    """One message in len(sizes) frames, each with its own receive key."""
    last = len(sizes) - 1
    return [mc.raw_frame((b0 & 0x0F if i == 0 else 0) | (0x80 if i == last else 0), data(rng, n),
                         key=int(rng.integers(1, 2**32))) for i, n in enumerate(sizes)]
