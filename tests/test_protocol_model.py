"""wsg_check_protocol's rule on the host (no GPU): layout.protocol_plan (the
call restated in vectorised numpy) and proto_judge (the C-ABI helper built
from csrc/wsg_proto.h, the rule the kernel runs) against the sequential loop
of tests/protocol_cases.py."""
import numpy as np
import pytest

import cppserver_amd as ca
from cppserver_amd import layout
from tests import protocol_cases as pc

FUZZ_SEEDS = range(200)


def plan_as_loop(batch, role, max_message, proto_in, consumed=None):
    """layout.protocol_plan's outputs in the loop's form."""
    seed = None
    if proto_in is not None:
        seed = np.zeros(batch.n_streams, dtype=layout.PROTO_STATE)
        seed["bytes"] = [p[0] for p in proto_in]
        seed["open"] = [p[1] for p in proto_in]
    verdict, proto_out, result = layout.protocol_plan(batch.info, batch.stream_first, seed, role, max_message,
                                                      batch.wire, consumed)
    assert verdict.dtype == layout.PROTO_VERDICT and proto_out.dtype == layout.PROTO_STATE
    assert not proto_out["_pad"].any()
    words = verdict.view(np.uint64)
    got = []
    for j in range(batch.n_streams):
        v = (int(verdict["code"][j]), int(verdict["status"][j]), int(verdict["frame"][j]))
        assert (int(words[j]) == pc.U64_MAX) == (v == pc.NONE) and (v == pc.NONE or int(verdict["_pad"][j]) == 0)
        got.append(v)
    return got, [(int(s["bytes"]), int(s["open"])) for s in proto_out], [int(x) for x in result]


def check_plan(batch, role=pc.ANY, max_message=0, proto_in=None, consumed=None):
    want = batch.expect(role, max_message, proto_in, consumed)
    got = plan_as_loop(batch, role, max_message, proto_in, consumed)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    return want


def check_judge(batch, role, max_message, proto_in=None):
    """proto_judge frame by frame along every stream, against judge()."""
    codes = set()
    for j in range(batch.n_streams):
        nbytes, is_open = proto_in[j] if proto_in is not None else (0, 0)
        for i in range(int(batch.stream_first[j]), int(batch.stream_first[j + 1])):
            want = pc.judge(batch.info[i], batch.wire, bool(is_open), nbytes, role, max_message)
            code, status, after = ca.proto_judge(batch.info[i], batch.wire, (nbytes, is_open), role, max_message)
            assert (code, status, bool(after["open"]), int(after["bytes"])) == want, (j, i)
            assert not after["_pad"].any()
            codes.add(code)
            nbytes, is_open = int(after["bytes"]), int(after["open"])
    return codes


@pytest.mark.parametrize("role", [pc.ANY, pc.SERVER, pc.CLIENT])
def test_every_code(role):
    named = pc.every_code_streams()
    batch = pc.Batch(named.values())
    verdicts, _, result = check_plan(batch, role, pc.EVERY_CODE_LIMIT)
    codes = check_judge(batch, role, pc.EVERY_CODE_LIMIT)
    if role == pc.SERVER:
        assert [v[0] for v in verdicts] == [pc.EVERY_CODE_WANT[k] for k in named]
        assert {v[0] for v in verdicts} >= set(range(1, 13)) and codes >= set(range(13))
        assert result == [11, 2, 1]
    if role == pc.ANY:   # the unmasked stream is clean
        assert verdicts[list(named).index("mask")] == pc.NONE and result[0] == 10
    if role == pc.CLIENT:   # every masked frame is a violation, unless a lower code applies
        assert {v[0] for v in verdicts} == {0xFF, 3, 4, 5}


def test_first_one_wins_and_close_order():
    k = 9
    batch = pc.Batch([
        [pc.frame(0x81, b"ok", k), pc.frame(0xC1, b"rsv", k), pc.frame(0x83, b"", k)],         # two violations
        [pc.close(1000, key=k), pc.frame(0x83, b"", k)],                                        # behind a clean close
        [pc.frame(0x83, b"", k), pc.close(1000, key=k)],                                        # ahead of a close
        [pc.frame(0x80 | 0x48, b"\x03\xe8", k)],                                                # a close that violates
    ])
    verdicts, _, result = check_plan(batch)
    assert verdicts == [(3, 1002, 1), (1, 1000, 3), (4, 1002, 5), (3, 1002, 7)] and result == [3, 0, 1]
    check_judge(batch, pc.ANY, 0)


def test_fragmentation_and_carry():
    k = 0xAABBCCDD
    first = pc.Batch([
        [pc.frame(0x01, b"a", k)] + [pc.frame(0x00, b"bc", k)] * 3 + [pc.frame(0x80, b"d", k)],
        [pc.frame(0x02, b"a", k), pc.frame(0x89, b"ping", k), pc.frame(0x80, b"b", k)],
        [pc.frame(0x80, b"first", k)],
        [pc.frame(0x01, b"a", k), pc.frame(0x81, b"b", k)],
        [pc.frame(0x81, b"done", k), pc.frame(0x02, b"open", k), pc.frame(0x00, b"still", k)],
    ])
    verdicts, states, _ = check_plan(first)
    assert verdicts == [pc.NONE, pc.NONE, (8, 1002, 8), (9, 1002, 10), pc.NONE]
    assert states[4] == (9, 1) and states[0] == (8, 0)
    second = pc.Batch([[], [], [], [], [pc.frame(0x80, b"!", k), pc.frame(0x80, b"stray", k)]])
    verdicts, states, _ = check_plan(second, proto_in=states)
    assert verdicts[4] == (8, 1002, 1) and states[4] == (15, 0) and states[:4] == [(8, 0), (2, 0), (5, 0), (1, 0)]


def test_max_message():
    k = 3
    streams = [
        [pc.frame(0x02, bytes(60), k), pc.frame(0x8A, bytes(100), k), pc.frame(0x80, bytes(40), k)],   # exactly 100
        [pc.frame(0x02, bytes(60), k), pc.frame(0x00, bytes(41), k), pc.frame(0x80, b"", k)],          # 101 at frame 1
        [pc.frame(0x82, bytes(101), k)],
        [pc.frame(0x80, bytes(10), k)],                                                                # carried in: 95
    ]
    batch = pc.Batch(streams)
    seed = [(0, 0), (0, 0), (0, 0), (95, 1)]
    verdicts, states, _ = check_plan(batch, max_message=100, proto_in=seed)
    assert verdicts == [pc.NONE, (12, 1009, 4), (12, 1009, 6), (12, 1009, 7)] and states[3] == (105, 0)
    verdicts, _, _ = check_plan(batch, max_message=0, proto_in=seed)
    assert verdicts == [pc.NONE] * 4
    check_judge(batch, pc.SERVER, 100, seed)


def test_bytes_saturate():
    batch = pc.Batch([[pc.frame(0x00, bytes(5)), pc.frame(0x00, bytes(5))]])
    _, states, _ = check_plan(batch, proto_in=[(pc.U64_MAX - 7, 1)], max_message=pc.U64_MAX)
    assert states == [(pc.U64_MAX, 1)]
    check_judge(batch, pc.ANY, pc.U64_MAX, [(pc.U64_MAX - 7, 1)])


def test_close_statuses():
    batch = pc.Batch(pc.close_status_streams())
    verdicts, _, result = check_plan(batch)
    want = []
    for s in pc.CLOSE_STATUSES:
        want += [(1, s) if s in pc.LEGAL else (11, 1002)] * 2
    assert [v[:2] for v in verdicts] == want
    assert result[2] == 2 * sum(s in pc.LEGAL for s in pc.CLOSE_STATUSES)
    check_judge(batch, pc.ANY, 0)
    empty = pc.Batch([[pc.close(None, key=5)], [pc.close(None)], [pc.frame(0x88, b"\x03")]])
    assert [v[:2] for v in check_plan(empty)[0]] == [(1, 1005), (1, 1005), (10, 1002)]


def test_consumed_and_empty_streams():
    k = 1
    batch = pc.Batch([[], [pc.frame(0x01, b"ab", k), pc.frame(0x80, b"c", k), pc.frame(0x02, b"defg", k)], [],
                      [pc.frame(0x02, b"tail", k)], []])
    seed = [(7, 1), (0, 0), (0, 0), (0, 0), (3, 0)]
    _, states, _ = check_plan(batch, proto_in=seed, consumed=[0, 2, 0, 0, 0])
    assert states == [(7, 1), (3, 0), (0, 0), (0, 0), (3, 0)]
    _, states, _ = check_plan(batch, proto_in=seed)
    assert states == [(7, 1), (4, 1), (0, 0), (4, 1), (3, 0)]
    none = pc.Batch([])
    assert none.expect() == ([], [], [0, pc.U64_MAX, 0]) and check_plan(none)


def test_judge_arguments():
    rec = pc.Batch([[pc.close(1000)]]).info[0]
    with pytest.raises(ca.WSGError):
        ca.proto_judge(rec, None, (0, 0))           # a close status needs the wire
    with pytest.raises(ca.WSGError):
        ca.proto_judge(rec, b"\x88\x02\x03\xe8", (0, 0), role=3)
    assert ca.proto_judge(rec, b"\x88\x02\x03\xe8", (0, 0))[:2] == (1, 1000)


def test_fuzz_generator_and_model():
    """Every seed: the plan against the loop.  The generator yields both clean
    and violating streams for at least 95 % of the seeds (the loop alone says so)."""
    both = 0
    for seed in FUZZ_SEEDS:
        streams, role, limit, proto_in = pc.fuzz(seed)
        assert 1 <= len(streams) <= 40 and all(len(s) <= 60 for s in streams)
        batch = pc.Batch(streams)
        verdicts, _, result = batch.expect(role, limit, proto_in)
        clean = sum(1 for v in verdicts if v is pc.NONE or v[0] == 1)
        both += clean > 0 and result[0] > 0
        check_plan(batch, role, limit, proto_in)
        if seed % 10 == 0:
            check_judge(batch, role, limit, proto_in)
    assert both >= 0.95 * len(FUZZ_SEEDS), both
