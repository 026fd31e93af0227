"""layout.frame_plan, the host model of wsg_frame_streams, against a framer
built from the oracle alone (frames_cases.oracle_walk: the session's
RequiredReceiveFrameSize walk) and against counts worked out by hand.  CPU
only; tests/test_gpu_frames.py holds the device against the same model."""
import numpy as np
import pytest

import oracle
from cppserver_amd import layout
from tests import frames_cases as fc
from tests import messages_cases as mc


def plan_one(data):
    """frame_plan of one stream at wire offset 3; returns (starts relative to
    the stream, consumed, need)."""
    w = fc.Wire([data], gaps=[3])
    fs, sf, spans, count = layout.frame_plan(w.wire, w.spans)
    assert list(sf) == [0, len(fs)] and int(count[0]) == len(fs) and int(count[1]) == int(spans["consumed"][0])
    return [int(x) - 3 for x in fs], int(spans["consumed"][0]), int(spans["need"][0])


def test_oracle_walk_is_the_documented_walk():
    payload = bytes(range(200))
    frame = oracle.Session(0xCAFEBABE).prepare_send(0x82, True, payload)
    assert fc.oracle_walk(frame + frame[:7]) == ([0], len(frame))
    assert fc.oracle_walk(frame[:-1]) == ([], 0)


@pytest.mark.parametrize("name", sorted(fc.clean_streams()))
def test_clean_streams(name):
    data = fc.clean_streams()[name]
    starts, consumed, need = plan_one(data)
    assert (starts, consumed) == fc.oracle_walk(data)
    assert consumed == len(data) and need == 0
    if name.startswith("quirk_"):   # the frames the stream was built from
        sizes = [len(f) for f in mc.quirk_streams()[name[len("quirk_"):]]]
        assert starts == [int(x) for x in np.cumsum([0] + sizes[:-1])][: len(sizes)]


def test_cut_frames():
    cases = fc.cut_cases()
    assert len(cases) > 100
    for name, (data, frames, consumed, need) in cases.items():
        got = plan_one(data)
        assert (len(got[0]), got[1], got[2]) == (frames, consumed, need), name
        assert (got[0], got[1]) == fc.oracle_walk(data), name


def test_huge_lengths_never_complete():
    for name, (data, frames, consumed, need) in fc.huge_cases().items():
        got = plan_one(data)
        assert (len(got[0]), got[1], got[2]) == (frames, consumed, need), name
    assert {v[3] for v in fc.huge_cases().values()} == {2**63 + 10, 2**63 + 14, fc.U64_MAX}


def test_tiny_streams():
    for name, (data, frames, consumed, need) in fc.tiny_cases().items():
        got = plan_one(data)
        assert (len(got[0]), got[1], got[2]) == (frames, consumed, need), name
        assert (got[0], got[1]) == fc.oracle_walk(data), name


def test_many_streams_in_one_wire():
    """Every model case as one batch: stream_first is the prefix of the
    counts, the starts are absolute, gaps and tails are skipped."""
    streams = fc.model_streams()
    names = sorted(streams)
    w = fc.Wire([streams[k][0] for k in names])
    fs, sf, spans, count = layout.frame_plan(w.wire, w.spans)
    assert len(sf) == len(names) + 1 and sf[0] == 0 and int(sf[-1]) == len(fs) == int(count[0])
    assert int(count[1]) == int(spans["consumed"].sum())
    assert (np.diff(fs.astype(np.int64)) > 0).all()
    fc.check_against_oracle(w, fs, sf, spans, [j for j, k in enumerate(names) if streams[k][1]])
    for j, k in enumerate(names):
        one = plan_one(streams[k][0])
        off = int(w.spans["off"][j])
        assert [int(x) - off for x in fs[int(sf[j]): int(sf[j + 1])]] == one[0], k
        assert (int(spans["consumed"][j]), int(spans["need"][j])) == one[1:], k


def test_bad_spans():
    f = mc.raw_frame(0x82, b"abcdef")
    w = fc.Wire([f * 3, f * 2, f * 4, f, f * 2, f], gaps=[0, 0, 0, 0, 0, 0])
    n = len(w.wire)
    s = w.spans.copy()
    s["off"][1] -= 1                          # starts inside stream 0
    s["off"][3], s["len"][3] = 0, len(f)      # decreasing
    s["len"][5] = n - int(s["off"][5]) + 1    # one byte past the wire
    assert list(layout.bad_spans(n, s)) == [False, True, False, True, False, True]
    fs, sf, spans, count = layout.frame_plan(w.wire, s)
    assert list(np.diff(sf.astype(np.int64))) == [3, 0, 4, 0, 2, 0]
    assert list(spans["consumed"]) == [3 * len(f), 0, 4 * len(f), 0, 2 * len(f), 0] and not spans["need"].any()
    good = layout.frame_plan(w.wire, w.spans)
    assert set(int(x) for x in fs) <= set(int(x) for x in good[0])
    # an offset or a length past 2^63 does not wrap into the wire
    s = w.spans.copy()
    s["off"][2] = 2**64 - 8
    s["len"][2] = 16
    s["len"][4] = 2**64 - 1
    assert list(layout.bad_spans(n, s)) == [False, False, True, False, True, False]
    # a span behind a refused one is held against nothing
    assert list(np.diff(layout.frame_plan(w.wire, s)[1].astype(np.int64))) == [3, 2, 0, 1, 0, 1]
