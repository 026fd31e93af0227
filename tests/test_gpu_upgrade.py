"""wsg_upgrade_streams on the device against layout.upgrade_plan (which
tests/test_upgrade_model.py holds against the C++ classes): every case of
tests/upgrade_cases.py, the fuzz included, and the shapes where the kernels,
not the rule, can go wrong.

Every output buffer is filled with 0xA5 first.  d_resp has exactly the bytes
the responses need and a sentinel region behind them; everything behind
n_streams records, n_streams + 1 offsets and four counts must still hold the
sentinel.  Bit-exact throughout."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import STREAM_SPAN, UPGRADE_DTYPE  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import upgrade_cases as uc  # noqa: E402
from tests.test_gpu_async import _gate  # noqa: E402
from tests.test_gpu_frames import FrameOut, SENTINEL, dev, frame, sent, spans_in  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402

PAD = 64   # sentinel entries (bytes of d_resp) behind every table


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


class UpOut:
    """Sentinel-filled outputs of one call over ``spans``, ``resp_cap`` bytes of d_resp."""

    def __init__(self, spans, resp_cap):
        self.ns = len(spans)
        self.cap = int(resp_cap)
        self.refill(spans)

    def refill(self, spans):
        ns = self.ns
        self.spans = dev(spans_in(spans).view(np.uint8))
        self.up = sent((ns + PAD) * UPGRADE_DTYPE.itemsize)
        self.resp = sent(self.cap + PAD)
        self.resp_off = sent((ns + 1 + PAD) * 8).view(torch.int64)
        self.count = sent((4 + PAD) * 8).view(torch.int64)

    def run(self, codec, d_wire, max_request=0, stream=None):
        codec.upgrade_streams(d_wire, self.spans, resp_cap=self.cap, max_request=max_request, stream=stream,
                              up=self.up, resp=self.resp, resp_off=self.resp_off, count=self.count)

    def check(self, want, spans, fits=True):
        up, consumed, need, resp_off, resp, count, bad = want
        ns = self.ns
        got_up = self.up.cpu().numpy()
        assert got_up[: ns * 32].tobytes() == up.tobytes(), first_diff(got_up[: ns * 32].view(UPGRADE_DTYPE), up)
        assert (got_up[ns * 32:] == SENTINEL).all()
        sp = self.spans.cpu().numpy().view(STREAM_SPAN)
        assert np.array_equal(sp["off"], spans["off"]) and np.array_equal(sp["len"], spans["len"])
        assert np.array_equal(sp["consumed"], consumed) and np.array_equal(sp["need"], need)
        off = self.resp_off.cpu().numpy().view(np.uint64)
        assert np.array_equal(off[: ns + 1], resp_off) and (off[ns + 1:] == 0xA5A5A5A5A5A5A5A5).all()
        cnt = self.count.cpu().numpy().view(np.uint64)
        assert np.array_equal(cnt[:4], count) and (cnt[4:] == 0xA5A5A5A5A5A5A5A5).all()
        got = self.resp.cpu().numpy()
        if fits:
            assert len(resp) <= self.cap
            assert np.array_equal(got[: len(resp)], resp) and (got[len(resp):] == SENTINEL).all()
        else:
            assert len(resp) > self.cap and (got == SENTINEL).all(), "a byte of d_resp despite WSG_ENOMEM"


def first_diff(got, want):
    for j in range(len(want)):
        if got[j].tobytes() != want[j].tobytes():
            return "stream %d: got %s, want %s" % (j, got[j], want[j])
    return "equal"


def run_check(codec, wire, spans, max_request=0, cap=None, status=None, stream=None):
    """One call with d_resp sized exactly (or ``cap``), against the model."""
    want = layout.upgrade_plan(wire, spans, max_request)
    total = int(want[3][-1])
    o = UpOut(spans, total if cap is None else cap)
    # (the wire is readable to the end of its last 16-byte block)
    d_wire = torch.zeros((len(wire) + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")[: len(wire)]
    d_wire.copy_(torch.from_numpy(np.ascontiguousarray(wire)))
    o.run(codec, d_wire, max_request, stream)
    if status is None:
        status = ca.WSG_EINVAL if want[6].any() else 0
    assert codec.sync_status(stream) == status
    o.check(want, spans, fits=total <= o.cap)
    return want


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("env", [dict(WSG_DEC_BLOCKS_PER_CU=1), {}], ids=["1-block-per-cu", "default"])
def test_every_case_in_one_batch(env):
    """The hand cases and the 2000 fuzz cases back to back (span offsets of
    every alignment): more streams than one block scans, and with one block
    per CU (4 waves each) more than one pass of the grid's waves."""
    cases = uc.all_cases()
    assert len(cases) > 4 * 256 * 2
    wire, spans = uc.batch(cases)
    c = _codec(**env)
    try:
        want = run_check(c, wire, spans)
    finally:
        c.close()
    assert [int(x) for x in want[0]["code"]] == [e["code"] for e in uc.expected()]


@functools.lru_cache(maxsize=None)
def short_cases():
    """The hand cases without the prefixes, and every 16th prefix."""
    return tuple(d for n, d, _ in uc.hand_cases() if not n.startswith("prefix_") or int(n[7:]) % 16 == 5)


@pytest.mark.parametrize("align", range(16))
def test_span_alignment(codec, align):
    wire, spans = uc.batch(short_cases(), align=align)
    assert (spans["off"] % 16 == align).all()
    run_check(codec, wire, spans)


# ------------------------------------------------- tile edges and carried bytes
def edge_requests():
    """The header end at every offset from 1017 to 1031 of the span, and from
    2041 to 2055: the tile edges with the three carried bytes on both sides;
    the same with a failing header and a body behind the header end."""
    out = []
    for at in list(range(1017, 1032)) + list(range(2041, 2056)):
        out.append(uc.padded_to(at + 4) + b"\x81\x80\x00\x00\x00\x00")
        out.append(uc.padded_to(at + 4, uc.four(version=b"Sec-WebSocket-Version: 7") + [b"Content-Length: 2"]) + b"ab")
        out.append(uc.padded_to(at + 4)[:-1])   # one byte short of the header end
    return out


@pytest.mark.parametrize("align", [0, 1, 13])
def test_header_end_at_tile_edges(codec, align):
    reqs = edge_requests()
    wire, spans = uc.batch(reqs, align=align)
    want = run_check(codec, wire, spans)
    assert list(want[0]["code"][:3]) == [layout.UP_ACCEPTED, layout.UP_BAD_VERSION, layout.UP_INCOMPLETE]
    assert int(want[1][0]) == 1021 and int(want[1][1]) == 1023


def straddle_requests():
    """The key line at every start from 1024 - 60 to 1024 + 4 of the span
    (its first byte, its ':' and its value each cross the tile edge in turn),
    and one of the four headers in each of four tiles, the walk's verdict
    carried across them."""
    out = []
    for start in range(1024 - 60, 1024 + 5):
        head = b"GET /chat HTTP/1.1\r\nHost: h"
        pad = start - len(head) - 2
        lines = [b"Host: h" + b"x" * pad, b"Sec-WebSocket-Key: " + uc.KEY, b"Upgrade: websocket",
                 b"Connection: Upgrade", b"Sec-WebSocket-Version: 13"]
        req = uc.request(lines)
        assert req.find(b"Sec-WebSocket-Key") == start
        out.append(req)
        out.append(uc.request(lines[:1] + [b"Upgrade: websocket", b"Sec-WebSocket-Key:" + b" " * 20] + lines[2:]))
    filler = b"X-Filler: " + b"y" * 1000
    spread = [b"Sec-WebSocket-Key: " + uc.KEY, filler, b"Upgrade: websocket", filler, b"Connection: Upgrade", filler]
    out.append(uc.request(spread + [b"Sec-WebSocket-Version: 13"]))
    out.append(uc.request(spread + [b"Sec-WebSocket-Version: 14"]))
    out.append(uc.request(spread + [b"Sec-WebSocket-Key: " + uc.key_of_length(84), filler, b"Sec-WebSocket-Key:",
                                    b"Sec-WebSocket-Version: 13"]))
    out.append(uc.request(spread + [b"Content-Length: 7", filler, b"content-length: 3",
                                    b"Sec-WebSocket-Version: 13"], body=b"abcdef"))
    out.append(uc.request([filler, b"no colon here", filler] + spread))
    out.append(uc.request([b"Upgrade: nope", filler] + spread + [b"Sec-WebSocket-Version: 13"]))
    return out


@pytest.mark.parametrize("align", [0, 9])
def test_lines_across_tile_edges(codec, align):
    reqs = straddle_requests()
    wire, spans = uc.batch(reqs, align=align)
    want = run_check(codec, wire, spans)
    tail = [int(c) for c in want[0]["code"][-6:]]
    assert tail == [layout.UP_ACCEPTED, layout.UP_BAD_VERSION, layout.UP_EMPTY_KEY, layout.UP_ACCEPTED,
                    layout.UP_BAD_HTTP, layout.UP_NOT_WEBSOCKET]
    assert int(want[0]["key_len"][-4]) == 84 and int(want[1][-3]) == len(reqs[-3]) - 3


def test_long_request(codec):
    req = uc.padded_to(5000) + uc.text_frame(b"after", 0x01020304)
    wire, spans = uc.batch([req, req[:4999], req], align=3)
    want = run_check(codec, wire, spans)
    assert [int(c) for c in want[1]] == [5000, 0, 5000]


@pytest.mark.parametrize("align", range(4))
def test_key_lengths(codec, align):
    """Keys of the SHA-1 padding-edge lengths at wire alignments 0-3."""
    reqs = [uc.request(uc.four(key=b"Sec-WebSocket-Key:" + b" " * k + uc.key_of_length(n, k)))
            for n in uc.KEY_LENGTHS for k in range(4)]
    wire, spans = uc.batch(reqs, align=align)
    want = run_check(codec, wire, spans)
    assert (want[0]["code"] == layout.UP_ACCEPTED).all()
    assert sorted(set(int(k) % 4 for k in want[0]["key_off"])) == [0, 1, 2, 3]


# ------------------------------------------------------------ stream counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_stream_counts(codec, n):
    rng = np.random.default_rng(n)
    pool = uc.all_cases()
    cases = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    wire, spans = uc.batch(cases, gap=1)
    if n == 0:
        wire = np.zeros(0, dtype=np.uint8)
    run_check(codec, wire, spans)


def test_empty_streams_between_full_ones(codec):
    cases = []
    for k in range(40):
        cases += [uc.RFC_REQUEST, b"", b"", uc.browser_request()][: 1 + k % 4]
    wire, spans = uc.batch(cases)
    want = run_check(codec, wire, spans)
    assert int(want[5][2]) == sum(1 for c in cases if not c)


def test_bad_spans_among_good_ones(codec):
    cases = [uc.RFC_REQUEST] * 10
    wire, spans = uc.batch(cases, gap=5)
    spans["len"][2] = len(wire)                  # runs past the wire
    spans["off"][6] = int(spans["off"][5]) + 3   # starts inside the span before it
    spans["off"][9] = len(wire) + 1
    want = run_check(codec, wire, spans)
    # (span 3 starts before the end of span 2 only if that one lies inside the wire: it does not)
    assert list(np.flatnonzero(want[6])) == [2, 6, 9]
    assert list(want[0]["code"][[2, 6, 9]]) == [0, 0, 0] and int(want[5][0]) == 7


# ------------------------------------------------- capacity, limits, ordering
def test_capacity_one_byte_short(codec):
    cases = list(short_cases())
    wire, spans = uc.batch(cases)
    total = int(layout.upgrade_plan(wire, spans)[3][-1])
    run_check(codec, wire, spans, cap=total - 1, status=ca.WSG_ENOMEM)
    run_check(codec, wire, spans, cap=total)
    run_check(codec, wire, spans, cap=len(cases) * layout.UPGRADE_RESP_MAX)


def test_max_request(codec):
    short = uc.RFC_REQUEST[:100]
    body = uc.request(uc.four() + [b"Content-Length: 50"], body=b"abc")
    assert len(body) != len(short)
    cases = [short, uc.RFC_REQUEST, body, b"", uc.request(uc.four(upgrade=b"Upgrade: nope"))]
    wire, spans = uc.batch(cases, gap=2)
    for n in (len(short), len(body)):
        for limit in (n - 1, n, n + 1):
            want = run_check(codec, wire, spans, max_request=limit)
            codes = [int(c) for c in want[0]["code"]]
            assert codes[0] == (layout.UP_TOO_LONG if len(short) >= limit else layout.UP_INCOMPLETE)
            assert codes[2] == (layout.UP_TOO_LONG if len(body) >= limit else layout.UP_INCOMPLETE)
            assert codes[1] == layout.UP_ACCEPTED and codes[3] == layout.UP_INCOMPLETE and codes[4] == layout.UP_BAD_UPGRADE


@functools.lru_cache(maxsize=None)
def _two_batches():
    """Two batches over the same spans with other outcomes: B's streams are
    A's with one byte changed (same length)."""
    a = [c for c in uc.fuzz_cases()[:1500]]
    b = [c.replace(b"websocket", b"websocked").replace(b": 13", b": 31") for c in a]
    wa, sa = uc.batch(a)
    wb, sb = uc.batch(b)
    assert np.array_equal(sa, sb)
    pa, pb = layout.upgrade_plan(wa, sa), layout.upgrade_plan(wb, sb)
    assert int((pa[0]["code"] != pb[0]["code"]).sum()) > 200
    return (wa, sa, pa), (wb, sb, pb)


def padded_dev(wire):
    d = torch.zeros(len(wire) + 32, dtype=torch.uint8, device="cuda")[: len(wire)]
    d.copy_(torch.from_numpy(wire))
    return d


def test_side_stream(codec):
    (wa, sa, pa), _ = _two_batches()
    o = UpOut(sa, int(pa[3][-1]))
    d_wire = padded_dev(wa)
    torch.cuda.synchronize()
    st = codec.own_stream()
    o.run(codec, d_wire, stream=st)
    o.run(codec, d_wire, stream=st)   # again behind it, no synchronisation between
    assert codec.sync_status(st) == 0
    o.check(pa, sa)


def test_graph_replay(codec):
    """Captured after one plain run of the same size, replayed over a wire
    whose bytes changed."""
    (wa, sa, pa), (wb, sb, pb) = _two_batches()
    cap = max(int(pa[3][-1]), int(pb[3][-1]))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_wire = padded_dev(wa)
        o = UpOut(sa, cap)
        o.run(codec, d_wire)
        assert codec.sync_status(st) == 0
        o.check(pa, sa)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            o.run(codec, d_wire)
        for w, s, want in ((wb, sb, pb), (wa, sa, pa), (wb, sb, pb)):
            d_wire.copy_(torch.from_numpy(w))
            # the captured call writes the buffers it was captured with: refill them in place
            o.spans.copy_(dev(spans_in(s).view(np.uint8)))
            for t in (o.up, o.resp, o.resp_off.view(torch.uint8), o.count.view(torch.uint8)):
                t.fill_(SENTINEL)
            g.replay()
            assert codec.sync_status(st) == 0
            o.check(want, s)


def test_ordered_against_frame_streams(codec):
    """12 rounds of (upgrade_streams on S1, frame_streams on S2) on one
    context, queued behind a gate, each call into outputs of its own: the two
    calls share the context's scratch and are ordered on the device."""
    (wa, sa, pa), _ = _two_batches()
    rng = np.random.default_rng(17)
    fw = fc.Wire([b"".join(mc.random_frames(rng, int(rng.integers(2, 20)), 200)) for _ in range(1500)])
    fwant = layout.frame_plan(fw.wire, fw.spans)
    d_up, d_fr = padded_dev(wa), padded_dev(fw.wire)
    warm_u, warm_f = UpOut(sa, int(pa[3][-1])), FrameOut(fw.spans, int(fwant[3][0]))
    warm_u.run(codec, d_up)
    frame(codec, d_fr, warm_f)
    assert codec.sync_status() == 0
    outs = [(UpOut(sa, int(pa[3][-1])), FrameOut(fw.spans, int(fwant[3][0]))) for _ in range(12)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gate = _gate([s1, s2])
    for ou, of in outs:
        ou.run(codec, d_up, stream=s1)
        frame(codec, d_fr, of, s2)
    opened = gate.query()
    assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
    torch.cuda.synchronize()
    assert not opened, "the gate opened before every call was queued"
    for ou, of in outs:
        ou.check(pa, sa)
        of.check(fwant, fw.spans)


def test_arguments(codec):
    wire, spans = uc.batch([uc.RFC_REQUEST])
    d_wire = padded_dev(wire)
    o = UpOut(spans, 148)
    L, vp = ca.lib(), ctypes.c_void_p

    def call(wire_p=None, span_p=None, up_p=None, resp_p=None, off_p=None, count_p=None):
        return L.wsg_upgrade_streams(codec._ctx, vp(d_wire.data_ptr() if wire_p is None else wire_p), len(wire),
                                     vp(o.spans.data_ptr() if span_p is None else span_p), 1, 0,
                                     vp(o.up.data_ptr() if up_p is None else up_p),
                                     vp(o.resp.data_ptr() if resp_p is None else resp_p), 148,
                                     vp(o.resp_off.data_ptr() if off_p is None else off_p),
                                     vp(o.count.data_ptr() if count_p is None else count_p), codec._stream(None))

    assert call(wire_p=d_wire.data_ptr() + 8) == ca.WSG_EINVAL
    assert call(resp_p=o.resp.data_ptr() + 8) == ca.WSG_EINVAL
    assert call(span_p=o.spans.data_ptr() + 4) == ca.WSG_EINVAL
    assert call(up_p=o.up.data_ptr() + 4) == ca.WSG_EINVAL
    assert call(off_p=o.resp_off.data_ptr() + 4) == ca.WSG_EINVAL
    assert call(count_p=o.count.data_ptr() + 4) == ca.WSG_EINVAL
    for null in ("wire_p", "span_p", "up_p", "resp_p", "off_p", "count_p"):
        assert call(**{null: 0}) == ca.WSG_EINVAL, null
    assert codec.sync_status() == 0
    assert (o.up.cpu().numpy() == SENTINEL).all(), "launched despite WSG_EINVAL"
    assert call() == 0 and codec.sync_status() == 0
    o.check(layout.upgrade_plan(wire, spans), spans)


def test_checked_launch_refuses_a_short_resp(monkeypatch):
    """$WSG_CHECK=1: a d_resp block one byte short of resp_cap is WSG_EINVAL on
    the host and nothing is launched; with resp_cap bytes the call runs.  The
    block is an exact hipMalloc block of 2 MiB (torch's allocator hands out
    views of larger segments)."""
    monkeypatch.setenv("WSG_CHECK", "1")
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    block = ctypes.c_void_p()
    size = 2 << 20
    assert hip.hipMalloc(ctypes.byref(block), ctypes.c_size_t(size)) == 0
    c = ca.Codec(0)
    try:
        cases = [uc.RFC_REQUEST, uc.request(uc.four(version=b"Sec-WebSocket-Version: 8"))]
        wire, spans = uc.batch(cases)
        want = layout.upgrade_plan(wire, spans)
        o = UpOut(spans, 0)
        d_wire = padded_dev(wire)

        def call(cap):
            return ca.lib().wsg_upgrade_streams(c._ctx, ctypes.c_void_p(d_wire.data_ptr()), len(wire),
                                                ctypes.c_void_p(o.spans.data_ptr()), 2, 0,
                                                ctypes.c_void_p(o.up.data_ptr()), block, cap,
                                                ctypes.c_void_p(o.resp_off.data_ptr()),
                                                ctypes.c_void_p(o.count.data_ptr()), c._stream(None))

        assert call(size + 1) == ca.WSG_EINVAL
        assert c.sync_status() == 0
        assert (o.up.cpu().numpy() == SENTINEL).all() and int(o.count.cpu()[0]) != 1, "launched despite WSG_EINVAL"
        assert call(size) == 0
        assert c.sync_status() == 0
        total = int(want[3][-1])
        got = torch.empty(total, dtype=torch.uint8, device="cuda")
        assert hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), block, ctypes.c_size_t(total), 3) == 0   # device to device
        assert np.array_equal(got.cpu().numpy(), want[4])
        assert [int(x) for x in o.count.cpu().numpy().view(np.uint64)[:4]] == [int(x) for x in want[5]]
    finally:
        c.close()
        hip.hipFree(block)
