"""The frame-sequence rule against an outside RFC 6455 reader, and the echo
server's loop over cut reads in numpy (no GPU).

tests/golden/rfc6455.json records what aiohttp's pure-Python WebSocketReader
makes of the connections of tests/server_loop_cases.py (see
tests/golden/make_rfc6455.py).  Three statements of the project's rule are
held against it: protocol_cases.loop, layout.protocol_plan and the C helper
wsg_proto_judge, each merged with the UTF-8 verdicts where the reader decodes
text.  Then server_loop_cases.drive runs the loop with a step made of
layout's plans, which shows the driver and its checks correct before
tests/test_gpu_server_loop.py gives them a kernel."""
import importlib.util
import os

import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import protocol_cases as pc
from tests import reply_cases as rc
from tests import server_loop_cases as sl

RECORDS = [pytest.param(limit, decode, id=sl.record_name(limit, decode)) for limit, decode in sl.RECORDS]


def test_connections_are_the_fixtures():
    """The digests: the connections rebuilt from the seed are the recorded ones."""
    fx = sl.fixture()
    conns = sl.connections()
    assert fx["header"]["connections"] == len(conns) == len(fx["connections"]) == sl.N_CONNECTIONS
    assert fx["header"]["seed"] == sl.SEED and fx["header"]["limits"] == list(sl.LIMITS)
    for c, row in zip(conns, fx["connections"]):
        assert (c.name, sl.digest(c.data, 16), len(c.data), len(c.frames)) == \
            (row["name"], row["sha256"], row["bytes"], row["frames"])


def test_connections_hold_what_they_should():
    conns = sl.connections()
    sizes = [len(c.frames) for c in conns]
    assert min(sizes) == 0 and 30 <= max(sizes) <= 40
    by_name = {c.name: c for c in conns}
    b = pc.Batch([by_name["lengths"].frames])
    assert [int(x) for x in b.info["len"]] == [125, 126, 127, 65535, 65536] and b.info["masked"].all()
    assert by_name["empty"].data == b"" and by_name["ends_in_header"].tail and by_name["ends_in_payload"].tail
    for hdr, n in sl.HEADER_FORMS.items():
        c = by_name["header%d_cut%d" % (hdr, hdr - 1)]
        rec = ca.header_unpack(c.frames[1][:14])[1]
        assert (int(rec["hdr_len"]), int(rec["len"])) == (hdr, n)
    every = pc.Batch([[f for c in conns for f in c.frames]])
    assert every.info["masked"].all() and int(every.info["len"].max()) == 65536
    bad = sum(1 for v in sl.with_utf8(sl.rule_loop(0)) if v[0] == layout.PV_UTF8)   # ended by invalid UTF-8
    print("connections:", len(conns), "frames:", every.n, "with invalid UTF-8:", bad)
    assert 5 <= bad <= len(conns) // 4   # a minority


def test_class_counts_within_caps():
    """Conditions on the fixture itself: every difference has a class (the
    generator refuses to write one without), (a) to (c) and (e) hold at most
    5 % of the connections, (d) at most 10 %, and the header says so."""
    fx = sl.fixture()
    n = len(fx["connections"])
    for limit, decode in sl.RECORDS:
        name = sl.record_name(limit, decode)
        tally = {k: 0 for k in "abcde"}
        for row in fx["connections"]:
            r = row[name]
            if r.get("class"):
                assert r["class"] in "abce" and len(r["project"]) == 3
                tally[r["class"]] += 1
            tally["d"] += bool(r.get("d"))
        print(name, tally)
        assert tally == fx["header"]["counts"][name]
        assert tally["a"] + tally["b"] + tally["c"] + tally["e"] <= sl.CAP_ABC * n
        assert tally["d"] <= sl.CAP_D * n
        assert tally["e"] == 0 or not decode
    assert set(fx["header"]["classes"]) == set("abcde")


def test_regenerated_outcomes_equal_the_fixture():
    """With aiohttp importable: the reader's outcomes and delivered messages,
    regenerated, are the committed ones, and so is the whole file."""
    pytest.importorskip("aiohttp")
    path = os.path.join(os.path.dirname(sl.FIXTURE), "make_rfc6455.py")
    spec = importlib.util.spec_from_file_location("make_rfc6455", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rows = gen.outcomes()
    for row, want in zip(rows, sl.fixture()["connections"]):
        assert row["messages"] == want["messages"], row["name"]
        for limit, decode in sl.RECORDS:
            name = sl.record_name(limit, decode)
            assert row[name]["reader"] == want[name]["reader"], (row["name"], name)
    head, rows = gen.build()
    head["reader_version"] = sl.fixture()["header"]["reader_version"]   # (another release with the same outcomes)
    with open(sl.FIXTURE) as fh:
        assert gen.dump(head, rows) == fh.read()


# ------------------------------------------------------------------ three statements of the rule
def _plan(limit):
    b = sl.whole_batch()
    w = sl.one_call(limit, False, rc.ECHO, 0)
    pv, _, _ = layout.protocol_plan(w.info, b.stream_first, None, pc.SERVER, limit, b.wire)
    return sl.local(cc.verdict_tuples(pv), b.stream_first)


def _judge(limit):
    """wsg_proto_judge walked frame by frame over each connection."""
    out = []
    for c in sl.connections():
        b = pc.Batch([c.frames])
        before, verdict = (0, 0), sl.NONE
        for i in range(b.n):
            code, status, after = ca.proto_judge(b.info[i], b.wire, before, pc.SERVER, limit)
            if code:
                verdict = (code, status, i)
                break
            before = (int(after["bytes"]), int(after["open"]))
        out.append(verdict)
    return out


@pytest.mark.parametrize("statement", ["loop", "protocol_plan", "wsg_proto_judge"])
@pytest.mark.parametrize("limit,decode", RECORDS)
def test_rule_against_the_reader(limit, decode, statement):
    verdicts = {"loop": sl.rule_loop, "protocol_plan": _plan, "wsg_proto_judge": _judge}[statement](limit)
    if decode:
        verdicts = sl.with_utf8(verdicts)
    compared = sl.check_against_reader(verdicts, limit, decode, statement)
    assert compared >= 0.9 * sl.N_CONNECTIONS


def test_one_call_verdicts_are_the_rules():
    """What the loop is compared with (checked_reply_cases.expected over the
    whole connections) carries the same verdicts."""
    for limit, decode in sl.RECORDS:
        w = sl.one_call(limit, decode, rc.ECHO, 0)
        verdicts = sl.rule_loop(limit)
        assert sl.local(w.verdict, sl.whole_batch().stream_first) == (sl.with_utf8(verdicts) if decode else verdicts)


# ------------------------------------------------------------------ the loop in numpy
CONFIGS = [pytest.param(0, False, rc.SAME_CLOSE_PONG, 1, id="plain_max0"),
           pytest.param(sl.LIMITS[1], False, rc.ECHO, 0, id="plain_max400"),
           pytest.param(0, True, rc.ECHO, 0, id="validating_max0"),
           pytest.param(sl.LIMITS[1], True, rc.SAME_CLOSE_PONG, 1, id="validating_max400")]


def check_schedules(runs):
    """What the schedules must have exercised, whatever ran the rounds."""
    cuts = set().union(*(r.header_cuts for r in runs))
    for hdr in sl.HEADER_FORMS:
        assert {c for h, c in cuts if h == hdr} == set(range(1, hdr)), "header of %d bytes" % hdr
    for r in runs:
        print("rounds", r.rounds, "streams", r.max_streams, "frames", r.max_frames, "wire", r.max_wire,
              "resubmitted unchanged", r.resubmitted, "terminal frame in the tail", r.tail_close)
        assert 12 <= r.rounds <= sl.MAX_ROUNDS
        assert r.max_streams > 256 and r.max_frames > 256   # two blocks of streams and of frames in one scan
        assert r.resubmitted >= 10 and r.tail_close >= 1


def test_schedules_differ():
    a, b = sl.schedule(0), sl.schedule(1)
    assert sum(x != y for x, y in zip(a, b)) > 0.9 * sl.N_CONNECTIONS
    assert all(s[-1] == sl.REST for s in a)


@pytest.mark.parametrize("limit,validating,rule,mask", CONFIGS)
def test_loop_model(limit, validating, rule, mask):
    """The driver with the numpy step: each connection's output over the cut
    reads is the one call's, whatever the schedule, and agrees with the
    reader."""
    keys = sl.send_keys() if mask else None
    step = sl.model_step(rule, mask, limit, validating)
    runs = [sl.drive(step, seed, keys) for seed in (0, 1)]
    for seed, run in enumerate(runs):
        sl.check_run(run, limit, validating, rule, mask, "schedule %d" % seed)
    assert runs[0].out == runs[1].out and runs[0].verdict == runs[1].verdict
    check_schedules(runs)
