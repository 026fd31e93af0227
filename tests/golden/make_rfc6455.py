"""Write tests/golden/rfc6455.json: what an outside RFC 6455 reader makes of
the connections of tests/server_loop_cases.py.

The reader is aiohttp's pure-Python WebSocketReader
(aiohttp._websocket.reader_py, aiohttp 3.14), which shares no code with this
project.  Every connection is fed to it frame by frame, under each
max_message of server_loop_cases.LIMITS, once with decode_text=False and once
with decode_text=True.  The reader rejects size >= max_msg_size, so it gets
max_message + 1 (and 0, its "no limit", for max_message 0).

Per connection the fixture holds a digest of its bytes, the data messages the
reader delivered (FIN frame, opcode, length, digest), and per record the
reader's terminal outcome (status, frame) or null: the status of a protocol
error, or of the close frame it delivered (1005 for an empty one).  Where the
project's rule (protocol_cases.loop, merged with the UTF-8 verdicts for the
decode_text=True records) says something else, the record names the class
that explains it and the project-side value; a difference no class explains
makes this script fail, as does a class count above its cap.  No wire bytes
are stored: the connections are rebuilt from server_loop_cases.SEED.

Needs aiohttp and the built package; runs on the CPU.

Run:  python tests/golden/make_rfc6455.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import server_loop_cases as sl  # noqa: E402


class Queue:
    """What the reader writes to."""

    def __init__(self):
        self.items, self.exc = [], None

    def feed_data(self, msg, size):
        self.items.append(msg)

    def set_exception(self, exc, exc_cause=None):
        self.exc = exc

    def feed_eof(self):
        pass


def read(conn, limit, decode):
    """((status, frame) or None, [[FIN frame, opcode, length, digest]]) of one connection."""
    from aiohttp import WSMsgType
    from aiohttp._websocket.reader_py import WebSocketReader

    q = Queue()
    reader = WebSocketReader(q, limit + 1 if limit else 0, compress=False, decode_text=decode)
    messages = []
    for i, frame in enumerate(conn.frames):
        reader.feed_data(frame)
        for m in q.items:
            if m.type == WSMsgType.CLOSE:
                return (int(m.data) or 1005, i), messages
            if m.type in (WSMsgType.TEXT, WSMsgType.BINARY):
                data = m.data.encode("utf-8") if isinstance(m.data, str) else bytes(m.data)
                messages.append([i, int(m.type), len(data), sl.digest(data)])
        q.items.clear()
        if q.exc is not None:
            return (int(q.exc.code), i), messages
    reader.feed_data(conn.tail)
    assert not q.items and q.exc is None, "the reader judged a frame that is not whole"
    return None, messages


def outcomes():
    """The fixture's "connections" rows without the project-side fields: what
    the reader alone says."""
    rows = []
    for c in sl.connections():
        row = {"name": c.name, "sha256": sl.digest(c.data, 16), "bytes": len(c.data), "frames": len(c.frames)}
        for limit, decode in sl.RECORDS:
            outcome, messages = read(c, limit, decode)
            row[sl.record_name(limit, decode)] = {"reader": list(outcome) if outcome else None}
            if (limit, decode) == (0, False):
                row["messages"] = messages
            else:   # a stricter record delivers a prefix of them
                assert messages == row["messages"][: len(messages)]
        rows.append(row)
    return rows


def build():
    rows = outcomes()
    conns = sl.connections()
    counts = {}
    for limit, decode in sl.RECORDS:
        name = sl.record_name(limit, decode)
        project = sl.rule_loop(limit)
        if decode:
            project = sl.with_utf8(project)
        tally = {k: 0 for k in "abcde"}
        for c, row, p in zip(conns, rows, project):
            r = row[name]
            if sl.in_class_d(c, limit, p):
                r["d"] = True
                tally["d"] += 1
                if decode:   # the UTF-8 of a message with control payloads in it is not compared
                    continue
            cls = sl.classify(c, limit, decode, p, tuple(r["reader"]) if r["reader"] else None)
            assert cls != "?", "%s, %s: the reader says %s, the project %s: no class explains it" % (
                c.name, name, r["reader"], p)
            if cls:
                r["class"], r["project"] = cls, list(p)
                tally[cls] += 1
        n = len(conns)
        assert tally["a"] + tally["b"] + tally["c"] + tally["e"] <= sl.CAP_ABC * n, (name, tally)
        assert tally["d"] <= sl.CAP_D * n, (name, tally)
        counts[name] = tally
    import aiohttp
    head = {
        "reader": "the WebSocketReader that tests/golden/make_rfc6455.py names", "reader_version": aiohttp.__version__,
        "seed": sl.SEED, "connections": len(conns), "limits": list(sl.LIMITS), "role": "WSG_PROTO_SERVER",
        "caps": {"a+b+c+e": sl.CAP_ABC, "d": sl.CAP_D},
        "classes": sl.SECTIONS,
        "counts": counts,
    }
    return head, rows


def dump(head, rows):
    lines = ["{", ' "header": ' + json.dumps(head, indent=1).replace("\n", "\n ") + ",", ' "connections": [']
    lines += ["  " + json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(rows) else "") for i, r in enumerate(rows)]
    lines += [" ]", "}", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    head, rows = build()
    text = dump(head, rows)
    with open(sl.FIXTURE, "w") as fh:
        fh.write(text)
    print("wrote %s: %d bytes" % (os.path.relpath(sl.FIXTURE), len(text)))
    for name, tally in head["counts"].items():
        print(name, tally)
    print("terminal frames:", sum(1 for r in rows if r[sl.record_name(0, False)]["reader"]), "of", len(rows))
