"""tests/big_cases.py's translation against the models themselves, at small
sizes where the models can be run on both sides: shift_frames and shift_info
against layout.frame_plan and the oracle's decode of the shifted wire,
prepend_filler and prepend_filler_reply against layout.message_plan and
layout.reply_plan (and the oracle's sessions, through mc.check_model and
rc.check_plan) of the batch with the filler in front, and the UTF-8 prefix
rule against Python's decoder.  CPU only; tests/test_gpu_over_4gib.py rests on
these where the offsets pass 2^32 and no model can be run."""
import numpy as np
import pytest

import oracle
from cppserver_amd import layout
from tests import big_cases as bc
from tests import frames_cases as fc
from tests import messages_cases as mc
from tests import reply_cases as rc
from tests import utf8_cases as uc

SHIFTS = [0, 7, 4096 + 9]
FILLERS = [0, 1, 125, 126, 70000]


def _small_streams(seed):
    """(frames, tail) streams: the quirk streams, random ones, every kind of
    partial frame behind some of them."""
    rng = np.random.default_rng(seed)
    tails = [b"", b"\x81", b"\x82\x7e", b"\x82\xfe\x00", mc.raw_frame(0x82, bytes(300), key=9)[:-1], b"\x88\x05abc"]
    quirks = mc.quirk_streams()
    streams = [(quirks[k], tails[i % len(tails)]) for i, k in enumerate(sorted(quirks))]
    streams += [(mc.random_frames(rng, int(rng.integers(0, 7)), 400), tails[int(rng.integers(0, len(tails)))])
                for _ in range(12)]
    return streams


@pytest.mark.parametrize("shift", SHIFTS)
def test_shift_frames_and_info(shift):
    """Stream j lies shift * (j + 1) bytes further into the wire than in the
    compact layout (so the streams move by different amounts)."""
    streams = _small_streams(3)
    data = [b"".join(f) + t for f, t in streams]
    compact = fc.Wire(data, gaps=[0] * len(data))
    offs = [int(o) + shift * (j + 1) for j, o in enumerate(compact.spans["off"])]
    case = bc.Sparse(streams, offs)
    m = case.model                                               # (asks the oracle's sessions too)
    total = case.end + 64
    wire = bc.place(case.data, case.spans, total)
    direct = layout.frame_plan(wire, case.spans)
    derived = case.want_frames()
    assert np.array_equal(derived[0], direct[0]) and np.array_equal(derived[1], direct[1])
    for f in ("off", "len", "consumed", "need"):
        assert np.array_equal(derived[2][f], direct[2][f]), f
    assert np.array_equal(derived[3], direct[3])
    assert (direct[2]["need"] > 0).any() and int(direct[3][0]) > 40
    fc.check_against_oracle(case, derived[0], derived[1], derived[2])   # (a Sparse has a Wire's streams and spans)
    # the frames' records and the message tables of the shifted wire
    rc_o, out, info = oracle.decode_batch(wire, direct[0])
    assert rc_o == 0
    mc.same_fields(case.want_info(), info, mc.INFO_FIELDS)
    msgs, count, state = layout.message_plan(info, direct[1], None, payload=out)
    mc.same_fields(msgs, m["msgs"], mc.MSG_FIELDS)               # nothing in them depends on where the bytes lay
    mc.same_fields(state, m["state"], ["consumed", "opcode"])
    assert np.array_equal(count, m["count"])
    assert np.array_equal(mc.dense(out, info, direct[1], state), m["buf"])
    if shift == 0:
        assert np.array_equal(case.want_info()["payload_off"][: int(direct[1][1])],
                              m["info"]["payload_off"][: int(direct[1][1])])


def test_sparse_cases_are_what_the_issue_asks_for():
    """The batches of the GPU test: every header form and split at both
    marks, every start misalignment, the streams that meet at 2^32 - 1024,
    a consumed lowered above each mark, a jump across each mark."""
    cases = bc.sparse_cases()
    assert len(cases) == sum(bc.header_bytes(f, m) + 1 for f, m in bc.HEADER_FORMS) + 2 == 52
    mis = {mark: set() for mark in bc.MARKS}
    lowered_above = {mark: 0 for mark in bc.MARKS}
    for name, case in cases.items():
        assert case.end + 16 <= bc.SPARSE_WIRE
        want = case.want_frames()
        fs, sf, spans = want[0], want[1], want[2]
        assert int(case.spans["off"][0]) == 3 and int(case.spans["off"][-1]) == bc.TOP
        for mark in bc.MARKS:
            (j,) = [j for j in range(case.n_streams)
                    if int(spans["off"][j]) < mark < int(spans["off"][j]) + int(spans["len"][j])]
            mis[mark].add(int(spans["off"][j]) % 16)
            starts = [int(x) for x in fs[int(sf[j]): int(sf[j + 1])]]
            x = starts[1]                                        # the frame under test
            hdr = int(case.model["info"]["hdr_len"][int(sf[j]) + 1])
            if name.startswith("hdr"):
                s = int(name.split("_s")[1])
                assert x == mark - s and hdr == int(name[3:].split("_")[0]) and 0 <= s <= hdr
            else:
                assert x + hdr < mark < x + hdr + 70000 and starts[2] > mark
            assert int(spans["need"][j]) == 2
            low = int(spans["off"][j]) + int(case.model["lowered"][j])
            if int(case.model["lowered"][j]) < int(spans["consumed"][j]):
                assert low > mark
                lowered_above[mark] += 1
        if name.startswith("hdr"):
            j = [int(o) for o in spans["off"]].index(bc.MEET)
            assert int(spans["off"][j - 1]) + int(spans["len"][j - 1]) == bc.MEET
    assert all(mis[mark] == set(range(16)) for mark in bc.MARKS)
    assert all(lowered_above[mark] >= 6 for mark in bc.MARKS)


@pytest.mark.parametrize("L0", FILLERS)
def test_prepend_filler(L0):
    rng = np.random.default_rng(40 + L0)
    streams = [f for f, _ in _small_streams(5)]
    rest = mc.Batch(streams)
    filler = mc.raw_frame(0x82, rng.integers(0, 256, L0, dtype=np.uint8).tobytes(), key=bc.FILLER_KEY)
    full = mc.Batch([[filler]] + streams)
    msgs, count, state, buf, _, info = mc.check_model(rest)       # each against the oracle's sessions
    f_msgs, f_count, f_state, f_buf, _, f_info = mc.check_model(full)
    d_msgs, d_count, d_state = bc.prepend_filler(msgs, count, L0, state)
    mc.same_fields(d_msgs, f_msgs, mc.MSG_FIELDS)
    mc.same_fields(d_state, f_state, ["consumed", "opcode"])
    assert np.array_equal(d_count, f_count)
    assert np.array_equal(f_buf[L0:], buf)
    # the records of the frames behind the filler: shift_info by the filler frame's size
    moved = bc.batch_spans(rest)
    moved["off"] += np.uint64(len(filler))
    mc.same_fields(bc.shift_info(info, rest.stream_first, bc.batch_spans(rest), moved), f_info[1:], mc.INFO_FIELDS)
    r = f_info[0]
    assert (int(r["payload_off"]), int(r["len"]), int(r["key"]), int(r["opcode"]), int(r["fin"]), int(r["masked"]),
            int(r["hdr_len"]), int(r["b0"]), int(r["error"])) == (len(filler) - L0, L0, bc.FILLER_KEY, 2, 1, 1,
                                                                  len(filler) - L0, 0x82, 0)
    for rule in (rc.ECHO, rc.SAME_CLOSE_PONG, rc.NONE):
        for mask in (0, 1):
            keys = np.arange(full.n_streams, dtype=np.uint32) * 0x01010101 + rc.KEY4
            _, _, _, off, stream_reply, rcount, _ = rc.check_plan(rest, rule, mask, keys[1:])
            _, _, _, f_off, f_stream_reply, f_rcount, _ = rc.check_plan(full, rule, mask, keys)
            d_off, d_stream_reply, d_rcount = bc.prepend_filler_reply((off, stream_reply, rcount), rule, mask, L0)
            assert np.array_equal(d_off, f_off) and np.array_equal(d_stream_reply, f_stream_reply)
            assert np.array_equal(d_rcount, f_rcount)


def test_dense_runs_targets():
    """What the filler's length brings to dense offset 2^32 in the four runs."""
    runs = bc.dense_runs()
    assert sorted(runs) == ["close", "first_byte", "fragments", "text"]
    for name, (streams, target) in runs.items():
        batch = mc.Batch(streams)
        msgs, count, state, buf, _, info = mc.check_model(batch)
        assert 10 <= batch.n_streams <= 14 and 0 < target < int(count[1])
        ends = msgs["off"].astype(np.int64) + msgs["len"].astype(np.int64)
        if name == "text":
            (m,) = [r for r in msgs if int(r["off"]) == target - 5]
            assert int(m["len"]) == 40 and int(m["opcode"]) == 1 and int(m["nframes"]) == 1
        elif name == "fragments":
            (m,) = [r for r in msgs if int(r["off"]) < target < int(r["off"]) + int(r["len"])]
            lens = [int(x) for x in info["len"][int(m["first_frame"]): int(m["first_frame"]) + 4]]
            assert int(m["nframes"]) == 4 and target == int(m["off"]) + lens[0] + lens[1]
        elif name == "close":
            (m,) = [r for r in msgs if int(r["off"]) == target + 1]
            assert int(m["kind"]) == layout.CB_CLOSE and int(m["status"]) == 0x03E9 and int(m["nframes"]) == 2
            assert int(info["len"][int(m["first_frame"])]) == 1
        else:
            at = [i for i, r in enumerate(msgs) if int(r["off"]) == target]
            assert len(at) == 2 and int(msgs["len"][at[0]]) == 0 and int(msgs["len"][at[1]]) == 50
        assert (ends[:-1] <= ends[1:]).all()


def test_utf8_prefix_rule():
    """A valid prefix that ends on a code point boundary adds its length:
    uc.want(prefix + tail) == len(prefix) + uc.want(tail)."""
    rng = np.random.default_rng(9)
    tails = list(uc.kat().values()) + [bytes(195) + b"\xff" + bytes(4), bytes(200), b"\x80" + bytes(63)]
    for prefix in (b"", bytes(1), bytes(1000), uc.mixed_text(rng, 257), bytes(300) + uc.GRIN):
        assert uc.want(prefix) == len(prefix)
        for tail in tails:
            assert bc.want_behind_prefix(len(prefix), tail) == uc.want(prefix + tail)
    # ... and not for a prefix that ends inside a sequence
    assert uc.want(uc.EURO[:2] + uc.EURO[2:]) == 3 != 2 + uc.want(uc.EURO[2:])
