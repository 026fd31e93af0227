"""Write tests/golden/rfc6455_messages.json: what an outside RFC 6455 reader
delivers for the connections of tests/rfc_assembly_cases.py, control frames
between fragments included.

The reader is aiohttp's pure-Python WebSocketReader
(aiohttp._websocket.reader_py, aiohttp 3.14), which shares no code with this
project.  Every connection is fed to it frame by frame, with no size limit,
once with decode_text=False ("raw") and once with decode_text=True ("utf8").

Per connection the fixture holds a digest of its bytes, whether a control
frame lies between the fragments of one of its messages, and per record the
sequence the reader delivered up to its terminal event, as [frame, type,
length, digest] with pings and pongs among the data messages, and that event:
(status, frame) or null, the status of a protocol error or of the close frame
(1005 for an empty one).  Where the project's verdict under WSG_ASSEMBLY_RFC
differs, the record names the class of server_loop_cases.SECTIONS that explains
it and the project-side value.  Class (d) does not exist under this rule.

The script refuses to write a fixture in which fewer than a quarter of the
connections have a control frame between fragments, in which more than 5 % of
the connections fall into classes (a), (b), (c) and (e) together, in which a
difference has no class, or in which a connection's delivered messages differ
from layout.message_plan(assembly=RFC)'s (order, kind, opcode, bytes) in
front of the earlier of the two terminal frames.  No wire bytes are stored:
the connections are rebuilt from rfc_assembly_cases.SEED.

Needs aiohttp and the built package; runs on the CPU.

Run:  python tests/golden/make_rfc6455_messages.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests.golden.make_rfc6455 import Queue  # noqa: E402

RECORDS = (("raw", False), ("utf8", True))


def read(conn, decode):
    """((status, frame) or None, [[frame, type, length, digest]]) of one connection."""
    from aiohttp import WSMsgType
    from aiohttp._websocket.reader_py import WebSocketReader

    q = Queue()
    reader = WebSocketReader(q, 0, compress=False, decode_text=decode)
    events = []
    for i, frame in enumerate(conn.frames):
        reader.feed_data(frame)
        for m in q.items:
            if m.type == WSMsgType.CLOSE:
                return (int(m.data) or 1005, i), events
            data = m.data.encode("utf-8") if isinstance(m.data, str) else bytes(m.data)
            events.append([i, int(m.type), len(data), sl.digest(data)])
        q.items.clear()
        if q.exc is not None:
            return (int(q.exc.code), i), events
    reader.feed_data(conn.tail)
    assert not q.items and q.exc is None, "the reader judged a frame that is not whole"
    return None, events


def build():
    conns = ac.connections()
    rows, classes, interleaved = [], 0, 0
    for j, c in enumerate(conns):
        row = {"name": c.name, "sha256": sl.digest(c.data, 16), "frames": len(c.frames),
               "interleaved": ac.has_interleaving(c.frames)}
        interleaved += row["interleaved"]
        in_class = False
        for name, decode in RECORDS:
            reader, events = read(c, decode)
            mine, project = ac.model_events(j, decode)
            v = ac.one_call(decode, ac.rc.SAME_CLOSE_PONG, 0).verdict[j]
            local = ac.NONE if v == ac.NONE else (v[0], v[1], project[1])
            rec = {"reader": list(reader) if reader else None, "events": events}
            cls = sl.classify(c, 0, decode, local, reader)
            assert cls != "?", "%s, %s: reader %r, project %r: no class explains it" % (c.name, name, reader, local)
            if cls:
                rec["class"], rec["project"] = cls, list(local)
                in_class = True
            stop = min(len(c.frames) if reader is None else reader[1], len(c.frames) if project is None else project[1])
            assert [e for e in events if e[0] < stop] == [e for e in mine if e[0] < stop], \
                "%s, %s: the model delivers other messages than the reader" % (c.name, name)
            row[name] = rec
        classes += in_class
        rows.append(row)
    n = len(conns)
    assert interleaved >= ac.CAP_INTERLEAVED * n, "%d of %d connections interleave" % (interleaved, n)
    assert classes <= ac.CAP_CLASSES * n, "%d of %d connections in classes (a), (b), (c), (e)" % (classes, n)
    return {"seed": ac.SEED, "reader": "aiohttp._websocket.reader_py.WebSocketReader, aiohttp 3.14",
            "interleaved": interleaved, "in_classes": classes, "connections": rows}


if __name__ == "__main__":
    out = build()
    with open(ac.FIXTURE, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("connections", len(out["connections"]), "interleaved", out["interleaved"], "in classes", out["in_classes"])
