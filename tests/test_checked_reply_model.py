"""layout.checked_reply_plan / merge_verdicts / utf8_verdicts (the numpy
restatement of wsg_reply_checked's rules) against the frames the oracle's
sessions send (tests/checked_reply_cases.py), and the wire_len + 14 * n bound
on every case (asserted inside checked_reply_cases.expected).  CPU only."""
import numpy as np
import pytest

from cppserver_amd import layout
from tests import checked_reply_cases as cc
from tests import messages_cases as mc
from tests import protocol_cases as pc
from tests import reply_cases as rc


def check(batch, rule, mask, keys, also=None, **kw):
    w = cc.expected(batch, rule, mask, keys, also=also, **kw)
    # merge_verdicts over the protocol's verdicts alone against the loop's
    alone = cc.expected(batch, rule, mask, keys, also=None, **kw)
    got = layout.merge_verdicts(cc.verdict_array(alone.verdict), None if also is None else cc.verdict_array(also),
                                batch.stream_first)
    assert cc.verdict_tuples(got) == w.verdict
    cc.check_model(w, batch, rule, mask, keys, also)
    return w


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("key", [0, rc.KEY4])
def test_one_stream_per_code(mask, key):
    batch, at = cc.code_batch()
    keys = np.full(batch.n_streams, key, dtype=np.uint32)
    w = check(batch, rc.SAME_CLOSE_PONG, mask, keys, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT)
    for name, (frames, t, code, status) in cc.code_streams().items():
        j = at[name]
        assert w.verdict[j] == (code, status, int(batch.stream_first[j]) + t), name
        sent = 1000 if status == 1005 else status
        body = bytes(a ^ b for a, b in zip(sent.to_bytes(2, "big"), int(key).to_bytes(4, "little")))
        assert w.close[j] == (b"\x88\x82" + int(key).to_bytes(4, "little") if mask else b"\x88\x02") + body, name
        assert w.by_stream[j].endswith(w.close[j]) and w.close_off[j] + len(w.close[j]) == w.stream_reply[j + 1]
    assert w.by_stream[at["tail_rsv"]] == w.close[at["tail_rsv"]]
    j = at["inside_fragments"]   # the two messages in front answered, nothing behind
    mine = [q for q in range(len(w.msgs)) if int(w.msgs["stream"][q]) == j]
    assert w.by_stream[j] == b"".join(w.frames[q] for q in mine) + w.close[j]
    assert sum(1 for q in mine if w.frames[q]) == 2
    assert w.rcount[2] == len(cc.code_streams())


def test_no_verdict_is_reply_plan():
    batch = mc.Batch(cc.clean_streams())
    w = check(batch, rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER)
    assert w.rcount[2] == 0 and w.close_off == [cc.U64_MAX] * batch.n_streams
    ro, sr, cnt = layout.reply_plan(w.msgs, rc.SAME_CLOSE_PONG, 1, None, n_streams=batch.n_streams)
    assert [int(x) for x in ro] == w.reply_off and [int(x) for x in sr] == w.stream_reply
    assert [int(x) for x in cnt] == w.rcount[:2]


def also_cases(batch, at):
    """A UTF-8 style verdict in front of the protocol's, behind it, at the
    same frame as a clean close and as a violation, outside the stream, none."""
    sf = batch.stream_first
    also = [cc.NONE] * batch.n_streams
    also[at["opcode_middle"]] = (13, 1007, int(sf[at["opcode_middle"]]) + 1)      # in front: wins
    also[at["cont"]] = (13, 1007, int(sf[at["cont"]]) + 3)                        # behind: loses
    also[at["closed_1000"]] = (13, 1007, int(sf[at["closed_1000"]]) + 2)          # same frame as a clean close: wins
    also[at["close_len"]] = (13, 1007, int(sf[at["close_len"]]) + 2)              # same frame as a violation: loses
    also[at["mask_last"]] = (13, 1007, int(sf[at["mask_last"] + 1]))              # outside the stream: ignored
    also[0] = (13, 1007, int(sf[0]))                                              # a clean stream: fails at frame 0
    return also


def test_also():
    batch, at = cc.code_batch()
    also = also_cases(batch, at)
    w = check(batch, rc.ECHO, 0, None, also=also, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT)
    sf = batch.stream_first
    assert w.verdict[at["opcode_middle"]] == also[at["opcode_middle"]]
    assert w.verdict[at["cont"]] == (8, 1002, int(sf[at["cont"]]) + 2)
    assert w.verdict[at["closed_1000"]] == also[at["closed_1000"]]
    assert w.verdict[at["close_len"]][0] == 10
    assert w.verdict[at["mask_last"]][0] == 5
    assert w.verdict[0] == also[0] and w.by_stream[0] == w.close[0]
    check(batch, rc.ECHO, 0, None, also=[cc.NONE] * batch.n_streams, role=pc.SERVER)


def test_utf8_verdicts():
    f, F = pc.frame, pc.FIN
    streams = [[f(F | pc.TEXT, "grüß".encode(), 1), f(F | pc.TEXT, b"bad \xff", 2), f(F | pc.TEXT, b"\xfe", 3)],
               [f(F | pc.BINARY, b"\xff\xff", 4)],
               [f(pc.TEXT, b"\xe2\x82", 5), f(F | pc.CONT, b"\xac", 6), pc.close(1000, b"\xc0", 7)],
               []]
    batch = mc.Batch(streams)
    which = layout.UTF8_TEXT | layout.UTF8_CLOSE
    w0 = cc.expected(batch)
    out_o, info = batch.oracle_decode()
    buf = mc.dense(out_o, info, batch.stream_first, w0.state)
    valid, _ = layout.utf8_plan(w0.msgs, buf, which)
    want = cc.utf8_also(w0.msgs, buf, which, batch.n_streams)
    assert want == [(13, 1007, 1), cc.NONE, (13, 1007, 6), cc.NONE]
    assert cc.verdict_tuples(layout.utf8_verdicts(w0.msgs, valid, which, batch.n_streams)) == want
    assert cc.verdict_tuples(layout.utf8_verdicts(w0.msgs, valid, 0, batch.n_streams)) == [cc.NONE] * 4
    w = check(batch, rc.ECHO, 0, None, also=want)
    assert w.verdict[2] == (13, 1007, 6) and w.close[2] == b"\x88\x02" + (1007).to_bytes(2, "big")


@pytest.mark.parametrize("seed", range(30))
def test_fuzz_protocol_streams(seed):
    batch, role, limit, proto_in, state = cc.fuzz_batch(seed)
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2**32, batch.n_streams).astype(np.uint32)
    also = None
    if seed & 1:
        sf = batch.stream_first
        also = [cc.NONE if rng.random() < 0.5 else (13, 1007, int(rng.integers(sf[j], sf[j + 1] + 2)))
                for j in range(batch.n_streams)]
    check(batch, rc.SAME_CLOSE_PONG if seed & 2 else rc.ECHO, seed & 1, keys, also=also, state=state, role=role,
          max_message=limit, proto_in=proto_in)


@pytest.mark.parametrize("seed", range(30))
def test_fuzz_tiny_streams(seed):
    batch = cc.tiny_fuzz_batch(seed)
    keys = np.random.default_rng(seed).integers(0, 2**32, batch.n_streams).astype(np.uint32)
    check(batch, rc.EVERYTHING if seed & 1 else rc.SAME_CLOSE_PONG, seed & 1, keys, role=seed % 3)
