"""WSG_ASSEMBLY_RFC without a GPU: layout.message_plan(assembly=RFC) and
utf8_wire_plan(assembly=RFC) against the recorded outside reader
(tests/golden/rfc6455_messages.json) and Python's strict decoder, the cut-read
loop against the one-call result, the `ahead` cap, and the reference mode of
the model against the plan as it was."""
import ctypes

import numpy as np
import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import reply_cases as rc
from tests import rfc_assembly_cases as ac
from tests import server_loop_cases as sl

RFC = ac.RFC
f, F = pc.frame, pc.FIN


def plan(streams, state=None, cap=layout.AHEAD_CAP):
    b = mc.Batch(streams)
    out, info = b.oracle_decode()
    msgs, count, new_state = layout.message_plan(info, b.stream_first, state, payload=out, assembly=RFC, ahead_cap=cap)
    return b, info, msgs, new_state, ac.dense(out, info, msgs)


def test_knob_is_exported_and_abi_stays_3():
    L = ctypes.CDLL(ca.LIB_PATH)
    assert hasattr(L, "wsg_set_assembly") and hasattr(L, "wsg_get_assembly")
    assert ca.lib().wsg_abi_version() == 3
    assert ca.lib().wsg_set_assembly(None, RFC) == ca.WSG_EINVAL and ca.lib().wsg_get_assembly(None) == ca.WSG_EINVAL
    assert (layout.ASSEMBLY_REFERENCE, layout.ASSEMBLY_RFC) == (0, 1)
    assert layout.STREAM_STATE.itemsize == 8 and layout.STREAM_STATE.fields["ahead"][1] == 6
    assert layout.STREAM_STATE.fields["opcode"][1] == 4 and layout.STREAM_STATE.fields["consumed"][1] == 0


def test_the_issue_example():
    """TEXT(!fin) "ab", PING "x", CONT(fin) "cd": a ping of its own in front of the text message "abcd"."""
    _, _, msgs, state, buf = plan([[f(pc.TEXT, b"ab", 1), f(F | pc.PING, b"x", 2), f(F | pc.CONT, b"cd", 3)]])
    assert [(int(m["kind"]), int(m["opcode"]), int(m["first_frame"]), int(m["nframes"])) for m in msgs] == \
        [(layout.CB_PING, 9, 1, 1), (layout.CB_RECEIVED, 1, 0, 3)]
    assert [buf[int(m["off"]):][: int(m["len"])].tobytes() for m in msgs] == [b"x", b"abcd"]
    assert int(state["consumed"][0]) == 3 and int(state["ahead"][0]) == 0 and int(state["opcode"][0]) == 0


def test_messages_against_the_recorded_reader():
    """Every connection of the fixture: digest, interleaving, and per record
    the delivered messages (order, type, length, bytes) in front of the earlier
    terminal frame and the terminal event, the reader's or the class's."""
    fx = ac.fixture()
    conns = ac.connections()
    assert fx["seed"] == ac.SEED and len(fx["connections"]) == len(conns) == ac.N_CONNECTIONS
    rows = fx["connections"]
    assert sum(r["interleaved"] for r in rows) >= ac.CAP_INTERLEAVED * len(rows)
    assert sum(1 for r in rows if any("class" in r[k] for k in ("raw", "utf8"))) <= ac.CAP_CLASSES * len(rows)
    compared = 0
    for j, (c, row) in enumerate(zip(conns, rows)):
        assert row["sha256"] == sl.digest(c.data, 16) and row["interleaved"] == ac.has_interleaving(c.frames), c.name
        for name, decode in (("raw", False), ("utf8", True)):
            rec = row[name]
            mine, project = ac.model_events(j, decode)
            reader = rec["reader"]
            if "class" in rec:
                assert project is not None and list(project) == rec["project"][1:], (c.name, name)
            else:
                assert (None if project is None else list(project)) == reader, (c.name, name)
            stop = min(len(c.frames) if reader is None else reader[1], len(c.frames) if project is None else project[1])
            assert [e for e in mine if e[0] < stop] == [e for e in rec["events"] if e[0] < stop], (c.name, name)
            compared += len([e for e in mine if e[0] < stop])
    assert compared > 2 * len(rows)   # the comparison is not vacuous: more than one message per record on average


def test_text_against_the_strict_decoder():
    """utf8_wire_plan(assembly=RFC) over every named and interleaved stream:
    valid[m] == len exactly where Python decodes the message's own bytes."""
    streams = list(ac.special_streams().values()) + ac.interleaved_streams()
    b = mc.Batch(streams)
    out, info = b.oracle_decode()
    msgs, count, valid, result = layout.utf8_wire_plan(info, b.stream_first, None, out, ac.WHICH, assembly=RFC)
    buf = ac.dense(out, info, msgs)
    texts = bad = 0
    for m, v in zip(msgs, valid):
        data = buf[int(m["off"]):][: int(m["len"])].tobytes()
        if (int(m["kind"]), int(m["opcode"])) == (layout.CB_RECEIVED, 1) or int(m["kind"]) == layout.CB_CLOSE:
            texts += 1
            try:
                data.decode("utf-8")
                assert int(v) == len(data)
            except UnicodeDecodeError as e:
                assert int(v) == e.start
                bad += 1
        else:
            assert int(v) == len(data)
    assert texts > 40 and bad >= 1 and int(result[0]) == bad
    named = dict(zip(ac.special_streams(), range(len(streams))))
    by_stream = {j: [(int(m["opcode"]), int(v) == int(m["len"])) for m, v in zip(msgs, valid) if int(m["stream"]) == j]
                 for j in named.values()}
    assert by_stream[named["cut_completed_by_ping"]] == [(9, True), (1, True)]      # the ping's bytes are not the text's
    assert by_stream[named["cut_broken_by_ping"]] == [(9, True), (1, True)]
    assert by_stream[named["cut_ping_is_the_rest"]] == [(9, True), (1, False), (1, True)]
    assert by_stream[named["cut_twice"]] == [(9, True), (10, True), (1, True)]


def test_reference_mode_is_the_plan_as_it_was():
    """assembly=REFERENCE (and the default) against the walk message_plan was
    before the knob, restated here, on the interleaved streams and fuzz batches."""
    def before(info, stream_first, state):
        kinds = {1: 1, 2: 1, 8: 2, 9: 3, 10: 4}
        rows, used, cons, ops = [], 0, [], []
        for j in range(len(stream_first) - 1):
            lo, hi = int(stream_first[j]), int(stream_first[j + 1])
            op, first = int(state["opcode"][j]), lo
            fins = [i for i in range(lo, hi) if info["fin"][i]]
            for i in range(lo, fins[-1] + 1 if fins else lo):
                op = int(info["opcode"][i]) or op
                if info["fin"][i]:
                    size = sum(int(info["len"][k]) for k in range(first, i + 1))
                    cut = 2 if op == 8 and size >= 2 else 0   # a close's status leaves the callback's data
                    rows.append((used + cut, size - cut, j, first, i - first + 1, kinds.get(op, 0), op))
                    used += size
                    first = i + 1
            cons.append(first - lo)
            ops.append(op)
        return rows, used, cons, ops

    for seed in range(12):
        batch, _, _, _, state = ac.fuzz(seed)
        _, info = batch.oracle_decode()
        rows, used, cons, ops = before(info, batch.stream_first, state)
        for kw in ({}, {"assembly": layout.ASSEMBLY_REFERENCE}):
            msgs, count, new = layout.message_plan(info, batch.stream_first, state, **kw)
            got = [(int(m["off"]), int(m["len"]), int(m["stream"]), int(m["first_frame"]), int(m["nframes"]),
                    int(m["kind"]), int(m["opcode"])) for m in msgs]
            assert got == rows and [int(count[0]), int(count[1])] == [len(rows), used]
            assert [int(x) for x in new["consumed"]] == cons and [int(x) for x in new["opcode"]] == ops
            assert not new["ahead"].any() and not new["_pad"].any()


@pytest.mark.parametrize("name", sorted(ac.special_streams()))
def test_two_calls_at_every_cut(name):
    """A stream cut at every frame boundary into two calls (the second gets the
    first's tail and state): the messages of both calls are the one call's, in
    order, every control frame delivered exactly once."""
    frames = ac.special_streams()[name]
    _, _, whole, _, wbuf = plan([frames])
    want = [(int(m["opcode"]), wbuf[int(m["off"]):][: int(m["len"])].tobytes(), int(m["status"])) for m in whole]
    for cut in range(len(frames) + 1):
        _, _, m1, s1, b1 = plan([frames[:cut]])
        rest = frames[int(s1["consumed"][0]): cut] + frames[cut:]
        _, _, m2, _, b2 = plan([rest], s1)
        got = [(int(m["opcode"]), b[int(m["off"]):][: int(m["len"])].tobytes(), int(m["status"]))
               for ms, b in ((m1, b1), (m2, b2)) for m in ms]
        assert got == want, cut


def test_ahead_cap_holds_and_skips():
    """The model at a cap of 3: six pings between two fragments.  Without the
    FIN frame three are delivered and ahead is 3; the resubmission skips those
    three and delivers the other three with the message, in frame order; a
    resubmission that still lacks the FIN frame delivers nothing twice."""
    pings = [f(F | pc.PING, bytes([65 + k]), 9) for k in range(6)]
    head, last = [f(pc.TEXT, b"ab", 1)] + pings, f(F | pc.CONT, b"cd", 2)
    _, _, m1, s1, b1 = plan([head], cap=3)
    assert [b1[int(m["off"]):][: int(m["len"])].tobytes() for m in m1] == [b"A", b"B", b"C"]
    assert (int(s1["consumed"][0]), int(s1["ahead"][0])) == (0, 3)
    _, _, m2, s2, _ = plan([head + pings[:1]], s1, cap=3)
    assert len(m2) == 0 and (int(s2["consumed"][0]), int(s2["ahead"][0])) == (0, 3)
    _, _, m3, s3, b3 = plan([head + [last]], s1, cap=3)
    assert [b3[int(m["off"]):][: int(m["len"])].tobytes() for m in m3] == [b"D", b"E", b"F", b"abcd"]
    assert [int(m["first_frame"]) for m in m3] == [4, 5, 6, 0] and int(m3["nframes"][3]) == 8
    assert (int(s3["consumed"][0]), int(s3["ahead"][0])) == (8, 0)
    # one call with everything: the held ones come with the message, all six once
    _, _, m4, _, b4 = plan([head + [last]], cap=3)
    assert [b4[int(m["off"]):][: int(m["len"])].tobytes() for m in m4] == [b"A", b"B", b"C", b"D", b"E", b"F", b"abcd"]
    # ahead applies to the first run only
    st = np.zeros(1, dtype=layout.STREAM_STATE)
    st["ahead"] = 1
    two = [f(pc.TEXT, b"a", 1), pings[0], f(F | pc.CONT, b"b", 2), f(pc.TEXT, b"c", 3), pings[1], f(F | pc.CONT, b"d", 4)]
    _, _, m5, _, b5 = plan([two], st)
    assert [b5[int(m["off"]):][: int(m["len"])].tobytes() for m in m5] == [b"ab", b"B", b"cd"]


CONFIGS = [(False, rc.SAME_CLOSE_PONG, 0), (True, rc.ECHO, 1)]


@pytest.mark.parametrize("validating,rule,mask", CONFIGS)
def test_loop_over_cut_reads(validating, rule, mask):
    """Two random schedules of cut reads over the fixture's connections with
    the model as the round: every connection's output is the one call's."""
    keys = ac.send_keys() if mask else None
    runs = [ac.drive(ac.model_step(rule, mask, validating), seed, keys) for seed in (0, 1)]
    for seed, run in enumerate(runs):
        ac.check_run(run, validating, rule, mask, "schedule %d" % seed)
    assert runs[0].out == runs[1].out and runs[0].carried_ahead > 0


def test_loop_under_a_low_cap():
    """The same loop with the model's cap at 1: held control frames arrive with their run's FIN frame."""
    run = ac.drive(ac.model_step(rc.SAME_CLOSE_PONG, 0, False, ahead_cap=1), 2)
    w = ac.expected(ac.whole_batch(), rc.SAME_CLOSE_PONG, 0, None, role=pc.SERVER, ahead_cap=1)
    assert run.out == w.by_stream
    # (runs with a second control frame inside them exist: the hold is taken)
    assert any(int(m["nframes"]) >= 5 and int(m["opcode"]) < 8 for m in w.msgs)
