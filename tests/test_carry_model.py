"""layout.carry_plan (wsg_carry_streams restated in numpy) against the plain
loop a caller runs today, ``pending[j][consumed:] + new``, and the echo
server's loop with that carry in it against the loop that joins each round's
wire on the host (tests/server_loop_cases.py::drive)."""
import numpy as np
import pytest

from cppserver_amd import layout
from tests import carry_cases as kc
from tests import server_loop_cases as sl
from tests.test_rfc6455_model import CONFIGS

VALIDATING = [c for c in CONFIGS if c.values[1]]
FLOOR = 64   # a full wave of streams with a tail and a read in one round


def plain(case):
    """The next pending bytes of every stream by the loop the carry replaces."""
    out = []
    for j in range(case.ns):
        off, length, used = (int(case.spans[f][j]) for f in ("off", "len", "consumed"))
        pending = case.wire[off: off + length].tobytes()
        new = b""
        if case.reads is not None:
            new = case.new[int(case.reads["off"][j]):][: int(case.reads["len"][j])].tobytes()
        if case.close_off is not None and int(case.close_off[j]) != kc.U64_MAX:
            pending = new = b""
        out.append(pending[used:] + new)
    return out


def check_layout(case):
    nxt, spans, count, key = case.plan()
    want = plain(case)
    assert key is None and len(nxt) == int(count[0]) and len(nxt) % 16 == 0
    at = 0
    for j, data in enumerate(want):
        assert (int(spans["off"][j]), int(spans["len"][j])) == (at, len(data)), j
        assert not spans["consumed"][j] and not spans["need"][j]
        assert nxt[at: at + len(data)].tobytes() == data, j
        pad = -len(data) % 16
        assert not nxt[at + len(data): at + len(data) + pad].any(), j
        at += len(data) + pad
    assert at == len(nxt)
    dropped = 0 if case.close_off is None else int((case.close_off != kc.U64_MAX).sum())
    news = 0 if case.reads is None else sum(int(case.reads["len"][j]) for j in range(case.ns)
                                            if case.close_off is None or int(case.close_off[j]) == kc.U64_MAX)
    assert [int(x) for x in count[1:]] == [sum(len(d) for d in want) - news, news, dropped]


def test_alignments_and_edges():
    rng = np.random.default_rng(1)
    check_layout(kc.alignments(rng))
    check_layout(kc.make(rng, [4095, 4096, 4097, 0], [1, 0, 4096, 0]))


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(seed):
    check_layout(kc.fuzz(seed))


def test_refused_streams_and_the_capacity():
    """A span past the wire, an overlapping span, consumed > len and a read
    past the end of new: that stream is empty, the first of them is the key,
    the others are as without it; the capacity's key comes behind them."""
    rng = np.random.default_rng(2)
    base = kc.make(rng, [5, 40, 17, 3, 60], [9, 0, 33, 12, 1], consumed=[3, 0, 7, 2, 9])
    clean = base.plan()
    for j, field, table, value in ((1, "len", "spans", len(base.wire)), (2, "off", "spans", int(base.spans["off"][1])),
                                   (3, "consumed", "spans", int(base.spans["len"][3]) + 1),
                                   (4, "off", "reads", len(base.new))):
        case = kc.Case(base.wire_raw, len(base.wire), base.spans.copy(), base.new_raw, len(base.new), base.reads.copy(),
                       base.close_off)
        getattr(case, table)[field][j] = value
        nxt, spans, count, key = case.plan()
        assert key == (j << 8 | 22) and int(spans["len"][j]) == 0
        for i in range(case.ns):
            if i != j:
                assert int(spans["len"][i]) == int(clean[1]["len"][i])
                assert nxt[int(spans["off"][i]):][: int(spans["len"][i])].tobytes() == \
                    clean[0][int(clean[1]["off"][i]):][: int(clean[1]["len"][i])].tobytes()
    total = int(clean[2][0])
    assert base.plan(total)[3] is None and base.plan(total - 16)[3] == (5 << 8 | 12)
    assert layout.carry_plan(base.wire, base.spans[:0], base.new, None)[2].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("limit,validating,rule,mask", VALIDATING[:1])
def test_the_loop_with_the_carry(limit, validating, rule, mask):
    """The driver that never joins a wire, with carry_plan and the model's
    step, gives what the joining driver gives on the same schedule, and in its
    fullest round at least a wave of streams has both a tail and a read."""
    keys = sl.send_keys() if mask else None
    step = sl.model_step(rule, mask, limit, validating)
    run = kc.drive(step, kc.model_carry, 0, keys)
    old = sl.drive(step, 0, keys)
    assert run.out == old.out and run.verdict == old.verdict
    sl.check_run(run, limit, validating, rule, mask, "the carry's loop")
    print("rounds", run.rounds, "bytes read", run.read_bytes, "sum of the rounds' wires", run.wire_bytes,
          "streams with a tail and a read in the fullest round", run.both)
    assert run.both >= FLOOR
    assert run.read_bytes < run.wire_bytes   # what the carry keeps off the bus
