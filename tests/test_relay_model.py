"""layout.relay_plan, the numpy restatement of wsg_relay_validated's relay
side, against tests/relay_cases.py (oracle sessions, plain loops), and the
chat loop's driver run over the model.  CPU only."""
import functools

import numpy as np
import pytest

from cppserver_amd import layout
from tests import carry_cases as kc
from tests import checked_reply_cases as cc
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import relay_cases as rl
from tests import rfc_assembly_cases as ac
from tests import server_loop_cases as sl


def batches():
    rng = np.random.default_rng(24)
    return {
        "rules": mc.Batch(rl.rule_streams()),
        "fragments": mc.Batch(rl.fragment_streams(rng)),
        "codes": cc.code_batch()[0],
        "many": mc.Batch(rl.many_streams(300, rng)),
        "empty": mc.Batch([]),
        "no_frames": mc.Batch([[], [], []]),
    }


BATCHES = batches()


@pytest.mark.parametrize("rfc", [False, True])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_plan_against_the_expectation(name, rfc):
    """Offsets, counts and bytes for every rule and every room table."""
    batch = BATCHES[name]
    ns = batch.n_streams
    for rule_name, (_, relay_op) in rl.RULES.items():
        for kind in rl.ROOM_KINDS:
            rooms = rl.rooms(ns, kind)
            w, want = rl.expected(batch, relay_op, rooms, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT, rfc=rfc)
            rl.same_relay(rl.model_relay(w, relay_op, rooms, ns), want)
            assert want.count[0] <= len(batch.wire) + 14 * batch.n   # wsg_capi.h's bound for relay_cap
            if rule_name == "none":
                assert want.count == [0, 0, 0] and set(want.relay_off) <= {rl.U64_MAX}


@pytest.mark.parametrize("rfc", [False, True])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_equivalence_with_the_checked_reply(name, rfc):
    """The relay of a stream is its checked reply under rule = relay_op, mask
    0 and no keys, without the close frame: the reply's bytes (and, in the
    reference mode, layout.checked_reply_plan's sizes) permuted by stream."""
    batch = BATCHES[name]
    ns = batch.n_streams
    rooms = rl.rooms(ns, "random", 3)
    for _, relay_op in rl.RULES.values():
        w, want = rl.expected(batch, relay_op, rooms, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT, rfc=rfc)
        pos = rooms.positions(ns)
        parts = []
        for j in pos:
            mine = w.by_stream[j]
            mine = mine[: len(mine) - len(w.close[j])]
            assert b"".join(want.by_stream[j]) == mine, j
            parts.append(mine)
        assert b"".join(parts) == want.relay
        if not rfc:
            reply_off, stream_reply, close_off, _ = layout.checked_reply_plan(w.msgs, cc.verdict_array(w.verdict),
                                                                              relay_op, 0, None, n_streams=ns)
            sizes = np.diff(stream_reply.astype(np.int64)) - np.array([len(c) for c in w.close], dtype=np.int64)
            starts = np.concatenate([[0], np.cumsum(sizes[pos])]) if ns else np.zeros(1, dtype=np.int64)
            assert [int(starts[p]) for p in rooms.bounds(ns)] == want.group_relay


def test_the_terminal_cut_and_the_rules():
    """In front of the terminal frame relayed; at it and behind it not."""
    batch = mc.Batch(rl.rule_streams())
    w, r = rl.expected(batch, rl.SAME, rl.Rooms(), role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT)
    assert [v[1] for v in w.verdict[:4]] == [1007, 1002, 1000, 1009]
    # one "hello" each from streams 0, 1 and 3, the binary of stream 2, the fragmented text of stream 5
    assert [len(x) for x in r.by_stream] == [1, 1, 1, 1, 0, 1, 0]
    assert r.by_stream[5] == [b"\x81\x09fragments"]
    w, r = rl.expected(batch, rl.RULES["ping_as_ping"][1], rl.Rooms(), role=pc.SERVER)
    assert r.by_stream[1] == [b"\x89\x04\x00\x00pp"]   # the two-byte prefix on a control opcode


def test_bad_tables():
    batch = mc.Batch(rl.rule_streams())
    ns = batch.n_streams
    w, _ = rl.expected(batch, rl.SAME, rl.Rooms())
    eff = cc.verdict_array(w.verdict)
    ident = np.arange(ns, dtype=np.uint32)
    for order, gf, key in ((np.array([0, 1, 2, 2, 4, 5, 6]), None, 3), (np.array([0, 9, 2, 3, 4, 5, 6]), None, 1),
                           (np.array([6, 6, 6, 6, 6, 6, 6]), None, 1), (ident, [1, ns], ns + 0),
                           (ident, [0, 5, 4, ns], ns + 2), (None, [0, 3, ns - 1], ns + 2),
                           (np.array([0, 1, 2, 2, 4, 5, 6]), [1, ns], 3)):
        assert layout.relay_tables_bad(ns, order, gf) == key
        relay_off, group_relay, count = layout.relay_plan(w.msgs, eff, rl.SAME, order, gf)
        assert (relay_off == rl.U64_MAX).all() and not group_relay.any() and not count.any()
        assert len(group_relay) == (2 if gf is None else len(gf))
    assert layout.relay_tables_bad(ns, ident[::-1], [0, 0, ns, ns]) is None
    assert layout.relay_tables_bad(0, None, [0]) is None


# ------------------------------------------------------------------ the chat loop over the model
@functools.lru_cache(maxsize=None)
def model_loop(rfc, limit, seed):
    cases, carries = (ac, "ahead") if rfc else (sl, "opcode")
    rooms = rl.loop_rooms(len(cases.connections()))
    log = []
    run = kc.drive(rl.model_step(cases, rl.CHAT_REPLY, rl.CHAT_RELAY, limit, rooms, log), kc.model_carry, seed, None,
                   cases=cases, carries=carries)
    return run, log, rooms


@functools.lru_cache(maxsize=None)
def one_call_frames(rfc, limit):
    """Per connection, the relay frames of one call over the whole connections."""
    cases = ac if rfc else sl
    batch = cases.whole_batch()
    w, r = rl.expected(batch, rl.CHAT_RELAY, rl.Rooms(), role=pc.SERVER, max_message=limit, rfc=rfc)
    return r.by_stream


def check_reply_side(run, log, rfc, limit, what):
    """The loop's reply side: the cases' own check_run.  Under the reference
    rule that check also compares the data messages a connection gets back,
    which the chat rule sends to the room instead: it judges the replies and
    the connection's own relay frames merged in message order (the validated
    echo under the union of the two rules), and the replies alone are held
    against the one-call run."""
    if rfc:
        ac.check_run(run, True, rl.CHAT_REPLY, 0, what)
        return
    w = sl.one_call(limit, True, rl.CHAT_REPLY, 0)
    assert run.out == w.by_stream and run.verdict == sl.local(w.verdict, sl.whole_batch().stream_first)
    merged = sl.Run()
    merged.__dict__.update(run.__dict__)
    n = len(run.out)
    merged.out = [b"".join(rnd.merged[j] for rnd in log) for j in range(n)]
    union = tuple(a | b for a, b in zip(rl.CHAT_REPLY, rl.CHAT_RELAY))
    sl.check_run(merged, limit, True, union, 0, what)


@pytest.mark.parametrize("rfc,limit", [(False, 0), (False, 400), (True, 0)])
def test_loop_over_the_model(rfc, limit):
    run, log, rooms = model_loop(rfc, limit, 0)
    # 147 of the 264 connections relay at max_message 0 (311 messages), 136 at 400 (241); of
    # rfc_assembly_cases' 200 connections 103 do (210 messages), so the floor there is 100, not 128
    rl.check_loop(log, rooms, one_call_frames(rfc, limit), 128 if not rfc else 100, 200)
    check_reply_side(run, log, rfc, limit, "model, rfc %d, limit %d" % (rfc, limit))
