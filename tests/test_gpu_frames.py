"""wsg_frame_streams / wsg_decode_streams on the device against
layout.frame_plan (tests/test_frames_model.py holds that model against the
oracle), clean inputs against the oracle walk as well.

Every output buffer is filled with 0xA5 first: everything behind d_count[0]
entries of the frame table, behind frame_cap, behind n_streams + 1 entries of
stream_first must still hold it, and the spans' consumed / need start as
0xA5A5... too.  Bit-exact throughout."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests.test_gpu_async import _gate  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402

SENTINEL = 0xA5
PAD = 64   # sentinel entries behind every table


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sent(nbytes):
    return torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device="cuda")


def spans_in(spans):
    """The spans as the caller hands them over: off and len set, the outputs
    sentinel-filled."""
    s = np.array(spans, dtype=STREAM_SPAN, copy=True)
    s["consumed"] = 0xA5A5A5A5A5A5A5A5
    s["need"] = 0xA5A5A5A5A5A5A5A5
    return s


class FrameOut:
    """Outputs of one wsg_frame_streams call of ns streams and room for cap frames."""

    def __init__(self, spans, cap):
        self.ns, self.cap = len(spans), int(cap)
        self.spans = dev(spans_in(spans).view(np.uint8))
        self.fsb = sent((self.cap + PAD) * 8)
        self.fs = self.fsb[: self.cap * 8].view(torch.int64)
        self.sfb = sent((self.ns + 1 + PAD) * 4)
        self.sf = self.sfb[: (self.ns + 1) * 4].view(torch.int32)
        self.count = torch.full((2,), -1, dtype=torch.int64, device="cuda")

    def refill(self, spans):
        self.spans.copy_(torch.from_numpy(spans_in(spans).view(np.uint8)))
        self.fsb.fill_(SENTINEL)
        self.sfb.fill_(SENTINEL)
        self.count.fill_(-1)

    def results(self):
        fsb = self.fsb.cpu().numpy()
        sfb = self.sfb.cpu().numpy()
        return (fsb.view(np.uint64), sfb.view(np.uint32), self.spans.cpu().numpy().view(STREAM_SPAN),
                self.count.cpu().numpy().view(np.uint64))

    def check(self, want, spans):
        """Every field against frame_plan's (fs, sf, spans_out, count)."""
        wfs, wsf, wspans, wcount = want
        fs, sf, sp, count = self.results()
        assert [int(x) for x in count] == [int(x) for x in wcount]
        assert np.array_equal(sf[: self.ns + 1], wsf.astype(np.uint32))
        assert (sf[self.ns + 1:] == 0xA5A5A5A5).all(), "stream_first written past n_streams + 1"
        n = int(wcount[0])
        if n <= self.cap:
            assert np.array_equal(fs[:n], wfs)
            assert (fs[n:] == 0xA5A5A5A5A5A5A5A5).all(), "frame starts written past d_count[0]"
        else:
            assert (fs == 0xA5A5A5A5A5A5A5A5).all(), "frame starts written although they do not fit"
        for f in ("off", "len"):
            assert np.array_equal(sp[f], np.asarray(spans)[f]), f
        for f in ("consumed", "need"):
            assert np.array_equal(sp[f], wspans[f]), f


def frame(codec, wire, o, stream=None):
    codec.frame_streams(wire, o.spans, frame_start=o.fs, frame_cap=o.cap, stream_first=o.sf, count=o.count,
                        stream=stream)


def run_check(codec, w, spans=None, cap=None, status=0, want=None, oracle_streams=None):
    """One synchronised call over Wire w (or other spans over its bytes)."""
    spans = w.spans if spans is None else spans
    want = layout.frame_plan(w.wire, spans) if want is None else want
    o = FrameOut(spans, int(want[3][0]) if cap is None else cap)
    frame(codec, dev(w.wire), o)
    assert codec.sync_status() == status
    assert codec.sync_status() == 0
    o.check(want, spans)
    if oracle_streams is not None:
        fs, sf, sp, _ = o.results()
        fc.check_against_oracle(w, fs, sf, sp, oracle_streams)
    return o


# ------------------------------------------------------------------ model cases
def test_model_cases_in_one_batch(codec):
    streams = fc.model_streams()
    names = sorted(streams)
    w = fc.Wire([streams[k][0] for k in names])
    run_check(codec, w, oracle_streams=[j for j, k in enumerate(names) if streams[k][1]])


# ---------------------------------------------------------------- misalignment
@functools.lru_cache(maxsize=None)
def _long_stream():
    rng = np.random.default_rng(21)
    frames = []
    for _ in range(3000):
        n = int(rng.integers(0, 201))
        key = int(rng.integers(0, 2**32)) if rng.random() < 0.6 else None
        frames.append(mc.raw_frame(int(rng.choice([0x81, 0x82, 0x01, 0x00, 0x80, 0x89])),
                                   rng.integers(0, 256, n, dtype=np.uint8).tobytes(), key=key))
    data = b"".join(frames)
    assert 250_000 < len(data) < 400_000
    starts, consumed = fc.oracle_walk(data)
    assert len(starts) == 3000 and consumed == len(data)
    return data, np.array(starts, dtype=np.uint64)


def test_every_start_misalignment(codec):
    data, starts = _long_stream()
    for m in range(16):
        for cut in (0, 1):   # whole, and one byte short of the last frame
            w = fc.Wire([data[: len(data) - cut]], gaps=[0], lead=m)
            assert int(w.spans["off"][0]) == m
            o = run_check(codec, w)
            fs = o.results()[0]
            assert np.array_equal(fs[: 3000 - cut], starts[: 3000 - cut] + np.uint64(m))


# ---------------------------------------------------------------- window edges
def _edge_streams(js, form):
    rng = np.random.default_rng(31 + form)
    junk = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    body = 130 if form == 126 else 65536
    out = []
    for j in js:
        out.append(mc.raw_frame(0x02, junk[:j]) + mc.raw_frame(0x00, junk[j % 97:][:body], key=0xC0FFEE00 + j)
                   + b"\x80\x00")
    return out


def test_window_edges_short_headers(codec):
    """Streams j = 0..8300: a filler frame of payload j, a masked 126-form
    frame (8-byte header), a 2-byte frame: the 8-byte header starts at every
    offset up to 8 KiB of its stream, so it straddles every window edge."""
    w = fc.Wire(_edge_streams(range(8301), 126))
    want = layout.frame_plan(w.wire, w.spans)
    assert int(want[3][0]) == 3 * 8301 and int(want[3][1]) == int(w.spans["len"].sum())
    run_check(codec, w, want=want, oracle_streams=[0, 1, 125, 126, 1009, 1023, 2040, 8300])


def test_window_edges_long_headers(codec):
    """The same with a masked 127-form frame (14-byte header, 65536 bytes of
    payload: a jump past the window), j within 16 of each power of two from
    256 to 65536."""
    js = [p + d for p in (1 << k for k in range(8, 17)) for d in range(-16, 17)]
    w = fc.Wire(_edge_streams(js, 127))
    want = layout.frame_plan(w.wire, w.spans)
    assert int(want[3][0]) == 3 * len(js)
    run_check(codec, w, want=want, oracle_streams=[0, 16, 33, len(js) - 1])


# ------------------------------------------------------ many streams, multi-pass
@functools.lru_cache(maxsize=None)
def _many():
    rng = np.random.default_rng(41)
    sizes = rng.integers(0, 40, 70000)
    streams = [mc.raw_frame(0x82, bytes(int(n)), key=int(n) * 2654435761 % 2**32 if n % 3 else None) for n in sizes]
    w = fc.Wire(streams)
    want = layout.frame_plan(w.wire, w.spans)
    assert int(want[3][0]) == 70000 > 65535
    return w, want


@pytest.mark.parametrize("env", [dict(WSG_DEC_BLOCKS_PER_CU=1), {}], ids=["1-block-per-cu", "default"])
def test_many_streams_multi_pass(env):
    """70 000 one-frame streams: more than 65 535, and with one block per CU
    (4 waves each) every wave walks some 70 streams."""
    w, want = _many()
    c = _codec(**env)
    try:
        run_check(c, w, want=want)
    finally:
        c.close()


def test_long_walk(codec):
    """One stream of 200 000 two-byte frames: one wave, 3 125 stores of 64
    starts, the ring advanced some 400 times."""
    w = fc.Wire([b"\x81\x00" * 200_000], gaps=[7])
    want = layout.frame_plan(w.wire, w.spans)
    assert np.array_equal(want[0], 7 + 2 * np.arange(200_000, dtype=np.uint64))
    run_check(codec, w, want=want)
    run_check(codec, fc.Wire([b"\x81\x00" * 100_031 + b"\x81"], gaps=[9]))   # a partial last store of starts


# ------------------------------------------------------------ degenerate counts
def test_degenerate_counts(codec):
    empty = fc.Wire([])
    o = run_check(codec, empty)
    assert [int(x) for x in o.results()[3]] == [0, 0] and int(o.results()[1][0]) == 0
    o = run_check(codec, fc.Wire([b""] * 300))
    assert not o.results()[1][:301].any()
    partial = [b"\x81", b"\x81\xfe\x01", b"\x82\x05abcd", mc.raw_frame(0x82, bytes(70000), key=5)[:-1]] * 80
    o = run_check(codec, fc.Wire(partial))
    fs, sf, sp, count = o.results()
    assert [int(x) for x in count] == [0, 0] and not sf[:321].any()
    assert [int(x) for x in sp["need"][:4]] == [2, 8, 7, 70014]


# -------------------------------------------------------------------- capacity
def test_capacity(codec):
    rng = np.random.default_rng(51)
    w = fc.Wire([b"".join(mc.random_frames(rng, int(rng.integers(0, 9)), 300)) for _ in range(600)])
    want = layout.frame_plan(w.wire, w.spans)
    n = int(want[3][0])
    assert n > 1000
    run_check(codec, w, want=want, cap=n)
    run_check(codec, w, want=want, cap=n + 5)
    run_check(codec, w, want=want, cap=n - 1, status=ca.WSG_ENOMEM)
    run_check(codec, w, want=want, cap=0, status=ca.WSG_ENOMEM)
    run_check(codec, fc.Wire([b""] * 5), cap=0)


# ------------------------------------------------------------------- bad spans
def test_bad_spans(codec):
    rng = np.random.default_rng(61)
    w = fc.Wire([b"".join(mc.random_frames(rng, 6, 200)) for _ in range(40)], gaps=[0] * 40)
    s = w.spans.copy()
    s["off"][9] -= 3                                        # overlaps stream 8
    s["off"][20], s["len"][20] = 5, 10                      # decreasing
    s["len"][33] = len(w.wire) - int(s["off"][33]) + 1      # out of the wire
    s["off"][37] = 2**64 - 4                                # off + len wraps
    bad = layout.bad_spans(len(w.wire), s)
    assert list(np.nonzero(bad)[0]) == [9, 20, 33, 37]
    want = layout.frame_plan(w.wire, s)
    good = layout.frame_plan(w.wire, w.spans)
    for j in range(40):   # the good streams exact
        if not bad[j]:
            assert np.array_equal(want[0][int(want[1][j]): int(want[1][j + 1])],
                                  good[0][int(good[1][j]): int(good[1][j + 1])])
    o = FrameOut(s, int(want[3][0]))
    frame(codec, dev(w.wire), o)
    assert codec.sync_status() == ca.WSG_EINVAL and codec.sync_status() == 0
    o.check(want, s)
    for first_bad in (20, 33):   # the lowest one is reported: drop the lower ones and look again
        s2 = s.copy()
        s2[:first_bad] = w.spans[:first_bad]
        run_check(codec, w, spans=s2, status=ca.WSG_EINVAL)


def test_latch_key_is_the_lowest_stream(codec):
    """Bad spans at streams 5 and 2 and a capacity error in one call: the
    latch's minimum is stream 2's key (read through wsg_sync's code only:
    EINVAL, where the capacity error alone gives ENOMEM)."""
    f = mc.raw_frame(0x81, b"abc")
    w = fc.Wire([f * 2] * 8, gaps=[0] * 8)
    s = w.spans.copy()
    run_check(codec, w, cap=3, status=ca.WSG_ENOMEM)
    s["off"][5] -= 1
    s["off"][2] -= 1
    run_check(codec, w, spans=s, cap=3, status=ca.WSG_EINVAL)


# -------------------------------------------------------------------- pipeline
class StreamsOut:
    """Outputs of one wsg_decode_streams call."""

    def __init__(self, spans, cap, msg_cap, opcodes=None):
        self.f = FrameOut(spans, cap)
        ns = self.f.ns
        st = np.full(ns * STREAM_STATE.itemsize + PAD, SENTINEL, dtype=np.uint8)
        st[: ns * STREAM_STATE.itemsize].view(STREAM_STATE)["opcode"] = 0 if opcodes is None else opcodes
        self.state = dev(st)
        self.msg = sent(msg_cap + PAD)
        self.msg_cap = msg_cap
        self.msgs = sent(cap * MSG.itemsize + PAD)
        self.info = sent(cap * RECV_INFO.itemsize + PAD)
        self.n = None

    def run(self, codec, wire, stream=None):
        f = self.f
        self.n = codec.decode_streams(wire, f.spans, state=self.state[: f.ns * STREAM_STATE.itemsize],
                                      frame_start=f.fs, frame_cap=f.cap, stream_first=f.sf, msg=self.msg,
                                      msg_cap=self.msg_cap, msgs=self.msgs, count=f.count, info=self.info,
                                      stream=stream)[-1]

    def host(self):
        fs, sf, sp, count = self.f.results()
        ns = self.f.ns
        state = self.state.cpu().numpy()
        msgs = self.msgs.cpu().numpy()
        info = self.info.cpu().numpy()
        msg = self.msg.cpu().numpy()
        return dict(fs=fs, sf=sf, spans=sp, count=count, state=state[: ns * STREAM_STATE.itemsize].view(STREAM_STATE),
                    state_tail=state[ns * STREAM_STATE.itemsize:], msgs=msgs[: int(count[0]) * MSG.itemsize].view(MSG),
                    msgs_tail=msgs[int(count[0]) * MSG.itemsize:], info=info[: self.n * RECV_INFO.itemsize].view(RECV_INFO),
                    info_tail=info[self.n * RECV_INFO.itemsize:], msg=msg[: int(count[1])], msg_tail=msg[int(count[1]):])


def _pipeline_streams():
    """(frames of each stream, the byte offset its first round ends at): 60
    random streams cut at random offsets, and one stream cut at every offset
    inside its first three headers (the offsets 1, 3, 4 and 5 of SURVEY Q7
    among them)."""
    rng = np.random.default_rng(71)
    out = []
    for _ in range(60):
        frames = mc.random_frames(rng, int(rng.integers(1, 12)), 400)
        out.append((frames, int(rng.integers(0, len(b"".join(frames)) + 1))))
    frames = [mc.raw_frame(0x01, b"x" * 130, key=0x11223344), mc.raw_frame(0x00, b"yz"),
              mc.raw_frame(0x80, bytes(200), key=7), mc.raw_frame(0x89, b"ping", key=9), mc.raw_frame(0x82, b"more")]
    at = 0
    cuts = set()
    for f, payload in zip(frames[:3], (130, 2, 200)):
        cuts.update(range(at, at + len(f) - payload + 1))
        at += len(f)
    assert {1, 3, 4, 5} <= cuts
    out.extend((frames, c) for c in sorted(cuts))
    return out


def test_pipeline_two_rounds(codec):
    """Two rounds of decode_streams carrying only off + consumed and
    state.opcode: the callbacks equal one oracle session per stream fed the
    unsplit stream."""
    cases = _pipeline_streams()
    whole = [b"".join(f) for f, _ in cases]
    ns = len(cases)
    events = [[] for _ in range(ns)]
    carried = [0] * ns
    opcodes = None
    for rnd in (0, 1):
        w = fc.Wire([whole[j][carried[j]: (cases[j][1] if rnd == 0 else len(whole[j]))] for j in range(ns)])
        cap = len(w.wire) // 2
        o = StreamsOut(w.spans, cap, len(w.wire), opcodes)
        o.run(codec, dev(w.wire))
        assert codec.sync_status() == 0
        h = o.host()
        plan = layout.frame_plan(w.wire, w.spans)
        assert o.n == int(plan[3][0]) and np.array_equal(h["fs"][: o.n], plan[0])
        assert (h["fs"][o.n:] == 0xA5A5A5A5A5A5A5A5).all()
        assert np.array_equal(h["sf"][: ns + 1], plan[1].astype(np.uint32))
        assert np.array_equal(h["spans"]["need"], plan[2]["need"])
        for name in ("state_tail", "msgs_tail", "info_tail", "msg_tail"):
            assert (h[name] == SENTINEL).all(), name
        ev = mc.events_by_stream(h["msgs"], h["msg"], ns)
        for j in range(ns):
            events[j] += ev[j]
            first, used = int(plan[1][j]), int(h["state"]["consumed"][j])
            nj = int(plan[1][j + 1]) - first
            lowered = int(plan[0][first + used]) - int(w.spans["off"][j]) if used < nj else int(plan[2]["consumed"][j])
            assert int(h["spans"]["consumed"][j]) == lowered, "stream %d" % j
            carried[j] += lowered
        opcodes = h["state"]["opcode"].copy()
    for j, (frames, _) in enumerate(cases):
        assert events[j] == mc.session_events(frames), "stream %d" % j


def test_decode_streams_equals_two_steps(codec):
    rng = np.random.default_rng(81)
    w = fc.Wire([b"".join(mc.random_frames(rng, int(rng.integers(0, 20)), 600)) + bytes(rng.integers(0, 3))
                 for _ in range(200)])
    d_wire = dev(w.wire)
    cap = len(w.wire) // 2
    seeds = rng.choice([0, 1, 2, 9], 200).astype(np.uint8)
    a = StreamsOut(w.spans, cap, len(w.wire), seeds)
    a.run(codec, d_wire)
    assert codec.sync_status() == 0
    b = StreamsOut(w.spans, cap, len(w.wire), seeds)
    frame(codec, d_wire, b.f)
    assert codec.sync_status() == 0
    b.n = int(b.f.count.cpu()[0])
    f = b.f
    codec.decode_messages(d_wire, f.fs[: b.n], f.sf, state=b.state[: f.ns * STREAM_STATE.itemsize], msg=b.msg,
                          msg_cap=b.msg_cap, msgs=b.msgs, count=f.count, info=b.info)
    assert codec.sync_status() == 0
    ha, hb = a.host(), b.host()
    assert a.n == b.n > 500
    for name in ("fs", "sf", "count", "msg", "msg_tail", "msgs_tail", "info_tail", "state_tail"):
        assert np.array_equal(ha[name], hb[name]), name
    mc.same_fields(ha["msgs"], hb["msgs"], mc.MSG_FIELDS)
    mc.same_fields(ha["info"], hb["info"], mc.INFO_FIELDS)
    mc.same_fields(ha["state"], hb["state"], ["consumed", "opcode"])
    for name in ("off", "len", "need"):
        assert np.array_equal(ha["spans"][name], hb["spans"][name]), name
    assert (ha["spans"]["consumed"] <= hb["spans"]["consumed"]).all()
    assert (ha["spans"]["consumed"] < hb["spans"]["consumed"]).any(), "no stream with a tail frame"
    assert int(ha["count"][0]) > 100


def test_decode_streams_capacity_and_capture(codec):
    f = mc.raw_frame(0x81, b"hello", key=3)
    w = fc.Wire([f * 3] * 10)
    d_wire = dev(w.wire)
    o = StreamsOut(w.spans, 29, len(w.wire))
    with pytest.raises(ca.WSGError) as e:
        o.run(codec, d_wire)
    assert e.value.code == ca.WSG_ENOMEM
    assert codec.sync_status() == ca.WSG_ENOMEM and codec.sync_status() == 0
    h_msg = o.msg.cpu().numpy()
    assert (h_msg == SENTINEL).all() and (o.msgs.cpu().numpy() == SENTINEL).all(), "decoded despite WSG_ENOMEM"
    assert int(o.f.count.cpu()[0]) == 30
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    o = StreamsOut(w.spans, 30, len(w.wire))
    with torch.cuda.stream(st):
        o.run(codec, d_wire)          # sized, outside the capture
        assert codec.sync_status() == 0
        assert o.n == 30
        with torch.cuda.graph(g, stream=st):
            o.f.count.fill_(-1)       # (a node, so that the capture is not empty)
            with pytest.raises(ca.WSGError) as e:
                o.run(codec, d_wire)
        assert e.value.code == ca.WSG_EINVAL


# ----------------------------------------------------------------------- async
@functools.lru_cache(maxsize=None)
def _two_wires():
    """Two batches over the same spans: B's streams are A's with the frames
    of each stream in reverse order (the same bytes per stream, other starts)."""
    rng = np.random.default_rng(91)
    lists = [mc.random_frames(rng, int(rng.integers(2, 30)), 300) for _ in range(1500)]
    a = fc.Wire([b"".join(f) for f in lists])
    b = fc.Wire([b"".join(f[::-1]) for f in lists])
    assert np.array_equal(a.spans, b.spans)
    wa, wb = layout.frame_plan(a.wire, a.spans), layout.frame_plan(b.wire, b.spans)
    assert int(wa[3][0]) == int(wb[3][0]) and int((wa[0] != wb[0]).sum()) > len(wa[0]) // 2
    return (a, wa), (b, wb)


def test_own_stream(codec):
    (a, wa), _ = _two_wires()
    o = FrameOut(a.spans, int(wa[3][0]))
    d_wire = dev(a.wire)
    torch.cuda.synchronize()
    st = codec.own_stream()
    frame(codec, d_wire, o, st)
    frame(codec, d_wire, o, st)   # again behind it, no synchronisation between
    assert codec.sync_status(st) == 0
    o.check(wa, a.spans)


def test_two_streams_alternately(codec):
    """16 rounds of (batch A on S1, batch B on S2) on one context, queued
    behind a gate, each call into outputs of its own: the calls share the
    context's count / partials scratch and are ordered on the device."""
    (a, wa), (b, wb) = _two_wires()
    ins = [dev(a.wire), dev(b.wire)]
    warm = FrameOut(a.spans, int(wa[3][0]))
    frame(codec, ins[0], warm)
    assert codec.sync_status() == 0
    outs = [(FrameOut(a.spans, int(wa[3][0])), FrameOut(b.spans, int(wb[3][0]))) for _ in range(16)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gate = _gate([s1, s2])
    for oa, ob in outs:
        frame(codec, ins[0], oa, s1)
        frame(codec, ins[1], ob, s2)
    opened = gate.query()
    assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
    torch.cuda.synchronize()
    assert not opened, "the gate opened before every call was queued"
    for oa, ob in outs:
        oa.check(wa, a.spans)
        ob.check(wb, b.spans)


def test_graph_replay(codec):
    """frame_streams captured after one plain run of the same size, replayed
    over a wire whose bytes changed."""
    (a, wa), (b, wb) = _two_wires()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_wire = torch.zeros(len(a.wire) + 16, dtype=torch.uint8, device="cuda")[: len(a.wire)]
        d_wire.copy_(torch.from_numpy(a.wire))
        o = FrameOut(a.spans, int(wa[3][0]))
        frame(codec, d_wire, o)
        assert codec.sync_status(st) == 0
        o.check(wa, a.spans)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            frame(codec, d_wire, o)
        for w, want in ((b, wb), (a, wa), (b, wb)):
            d_wire.copy_(torch.from_numpy(w.wire))
            o.refill(w.spans)
            g.replay()
            assert codec.sync_status(st) == 0
            o.check(want, w.spans)


# -------------------------------------------------------------- checked launches
def test_checked_launch_refuses_a_short_frame_table(monkeypatch):
    """$WSG_CHECK=1: a d_frame_start block one entry short of frame_cap is
    WSG_EINVAL on the host and nothing is launched; with frame_cap entries the
    call runs.  The block is an exact hipMalloc block of 2 MiB (torch's
    allocator hands out views of larger segments)."""
    import ctypes

    monkeypatch.setenv("WSG_CHECK", "1")
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    block = ctypes.c_void_p()
    entries = (2 << 20) // 8
    assert hip.hipMalloc(ctypes.byref(block), ctypes.c_size_t(entries * 8)) == 0
    c = ca.Codec(0)
    try:
        w = fc.Wire([mc.raw_frame(0x81, b"abc") * 5] * 4)
        want = layout.frame_plan(w.wire, w.spans)
        o = FrameOut(w.spans, 0)
        d_wire = dev(w.wire)

        def call(cap):
            return ca.lib().wsg_frame_streams(c._ctx, ctypes.c_void_p(d_wire.data_ptr()), len(w.wire),
                                              ctypes.c_void_p(o.spans.data_ptr()), 4, block, cap,
                                              ctypes.c_void_p(o.sf.data_ptr()), ctypes.c_void_p(o.count.data_ptr()),
                                              c._stream(None))

        assert call(entries + 1) == ca.WSG_EINVAL
        assert c.sync_status() == 0
        assert int(o.count.cpu()[0]) == -1 and (o.sfb.cpu().numpy() == SENTINEL).all(), "launched despite WSG_EINVAL"
        assert call(entries) == 0
        assert c.sync_status() == 0
        got = torch.empty(20, dtype=torch.int64, device="cuda")
        assert hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), block, ctypes.c_size_t(160), 3) == 0   # device to device
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want[0])
        assert [int(x) for x in o.count.cpu()] == [int(x) for x in want[3]]
    finally:
        c.close()
        hip.hipFree(block)
