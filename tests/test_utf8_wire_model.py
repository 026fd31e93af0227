"""layout.utf8_wire_plan and layout.validated_verdicts on the CPU: every case
of tests/utf8_wire_cases.py says what it claims before a GPU sees it.

The model's d_valid / d_result are held against Python's strict decoder
applied to what one oracle session per stream delivers (the text to
onWSReceived, the reason to onWSClose), and the d_also rule of
wsg_reply_validated against a plain loop."""
import numpy as np
import pytest

from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import utf8_wire_cases as wc

CASES = wc.small_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_against_the_decoder(name):
    for which in wc.WHICH:
        wc.check_case(CASES[name], which)


def test_selection_every_which():
    for which in wc.ALL_WHICH:
        _, _, msgs, _, valid, result = wc.check_case(CASES["selection"], which)
        if which == 0:
            assert [int(x) for x in valid] == [int(x) for x in msgs["len"]] and [int(x) for x in result[2:]] == [0, 0]
    # the binary message full of FF is checked by UTF8_EVERY alone
    assert int(wc.check_case(CASES["selection"], layout.UTF8_EVERY)[4][0]) == 0
    assert int(wc.check_case(CASES["selection"], wc.DEFAULT)[4][0]) == 40


def test_what_the_cases_claim():
    _, _, msgs, _, valid, _ = wc.check_case(CASES["message_boundaries"], wc.DEFAULT)
    assert [int(x) for x in valid[:4]] == [5, 0, 5, 0]       # A bad at len - 2, B at 0, in one stream and in two
    _, _, msgs, _, valid, _ = wc.check_case(CASES["close_reasons"], wc.DEFAULT)
    assert [int(x) for x in valid] == [6, 0, 0, 0, 2, 4, 8, 0, 0, 0]
    assert [int(x) for x in msgs["len"]] == [6, 4, 7, 1, 2, 7, 8, 0, 1, 0]
    _, _, msgs, _, valid, _ = wc.check_case(CASES["tails"], wc.DEFAULT)
    assert len(msgs) == 2 and [int(x) for x in valid] == [int(x) for x in msgs["len"]]
    # a ping between the fragments: its byte is part of the buffer (EVERY checks that buffer)
    _, _, msgs, _, valid, _ = wc.check_case(CASES["ping_between"], layout.UTF8_EVERY)
    euro = [k for k, s in enumerate(q for q in wc.SEQUENCES if len(q) >= 3) if s == wc.uc.EURO][0]
    j = 2 * euro                                              # the stream with the ping that has no FIN
    mine = [m for m in range(len(msgs)) if int(msgs["stream"][m]) == j]
    assert int(msgs["len"][mine[0]]) == 5 and int(valid[mine[0]]) == 5   # t E2 | 82 | AC z


def test_carry_over_in_two_calls():
    first, second = wc.carry_over()
    c1 = wc.Case(first)
    _, _, msgs, count, valid, _ = wc.check_case(c1, wc.DEFAULT)
    assert len(msgs) == 1                                     # the open fragment lies in the tail
    state = layout.message_plan(wc.model(c1, 0)[1], c1.batch.stream_first)[2]
    assert int(state["consumed"][0]) == 1 and int(state["opcode"][0]) == wc.BINARY   # (the fragment names its own)
    c2 = wc.Case(second, state["opcode"])
    _, _, msgs, _, valid, _ = wc.check_case(c2, wc.DEFAULT)
    assert [int(x) for x in msgs["len"]] == [10, 1] and [int(x) for x in valid] == [10, 0]


def test_many_messages_and_fuzz_cases():
    case, bad = wc.many_messages()
    _, _, msgs, _, valid, result = wc.check_case(case, wc.DEFAULT)
    assert sorted(np.nonzero(valid < msgs["len"])[0].tolist()) == sorted(bad) and int(result[0]) == len(bad)
    for seed in range(0, 100, 9):
        c, _, _, _ = wc.fuzz(seed)
        wc.model(c, wc.DEFAULT)


def _plain(msgs, valid, which, also, stream_first):
    """wsg_reply_validated's d_also' as a loop over the streams."""
    out = []
    for j in range(len(stream_first) - 1):
        lo, hi = int(stream_first[j]), int(stream_first[j + 1])
        best = cc.NONE
        for m, r in enumerate(msgs):
            if int(r["stream"]) == j and wc.selected(r, which) and int(valid[m]) < int(r["len"]):
                best = (13, 1007, int(r["first_frame"]) + int(r["nframes"]) - 1)
                break
        a = cc.NONE if also is None else also[j]
        if a != cc.NONE and lo <= a[2] < hi:
            word = lambda v: v[0] | (0 if v != cc.NONE else 0xFF00) | v[1] << 16 | v[2] << 32   # noqa: E731
            if best == cc.NONE or word(a) < word(best):
                best = a
        out.append(best)
    return out


@pytest.mark.parametrize("seed", range(12))
def test_validated_verdicts(seed):
    c, _, _, _ = wc.fuzz(seed)
    b = c.batch
    _, _, msgs, _, valid, _ = wc.model(c, wc.DEFAULT)
    rng = np.random.default_rng(seed)
    sf = b.stream_first
    for also in (None, [cc.NONE] * b.n_streams,
                 [cc.NONE if rng.random() < 0.3 else (int(rng.choice([3, 13, 14])), int(rng.choice([0, 1002, 1007])),
                                                      int(rng.integers(0, b.n + 2))) for _ in range(b.n_streams)]):
        got = layout.validated_verdicts(msgs, valid, wc.DEFAULT, None if also is None else cc.verdict_array(also), sf)
        assert cc.verdict_tuples(got) == _plain(msgs, valid, wc.DEFAULT, also, sf)
    # an entry outside its stream's range beside a UTF-8 verdict: the verdict survives
    bad = [j for j, v in enumerate(_plain(msgs, valid, wc.DEFAULT, None, sf)) if v != cc.NONE]
    for j in bad[:1]:
        also = [cc.NONE] * b.n_streams
        also[j] = (3, 1002, int(sf[j + 1]))
        got = layout.validated_verdicts(msgs, valid, wc.DEFAULT, cc.verdict_array(also), sf)
        assert cc.verdict_tuples(got)[j][0] == layout.PV_UTF8
