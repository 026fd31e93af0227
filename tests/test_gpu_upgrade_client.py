"""wsg_upgrade_client_streams and wsg_upgrade_requests on the device against
layout.upgrade_client_plan / layout.upgrade_request (which
tests/test_upgrade_client_model.py holds against the C++ classes): every case
of tests/upgrade_client_cases.py, the fuzz included, and the shapes where the
kernels, not the rule, can go wrong.

Every output buffer is filled with 0xA5 first; everything behind n_streams
records, three counts and n * tpl_len request bytes must still hold the
sentinel.  Bit-exact throughout."""
import base64
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import STREAM_SPAN, UPGRADE_REPLY_DTYPE  # noqa: E402
from tests import upgrade_client_cases as uc  # noqa: E402
from tests.test_gpu_frames import SENTINEL, dev, sent, spans_in  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402

PAD = 64   # sentinel entries behind every table
WORD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def padded_dev(wire):
    """The wire on the device, readable to the end of its last 16-byte block."""
    d = torch.zeros(len(wire) + 32, dtype=torch.uint8, device="cuda")[: len(wire)]
    d.copy_(torch.from_numpy(np.ascontiguousarray(wire)))
    return d


class UcOut:
    """Sentinel-filled outputs of one call over ``spans``."""

    def __init__(self, spans, nonces):
        self.ns = len(spans)
        self.nonces = dev(np.concatenate([nonces, np.full(16 * PAD, SENTINEL, dtype=np.uint8)]))
        self.refill(spans)

    def refill(self, spans):
        self.spans = dev(spans_in(spans).view(np.uint8))
        self.up = sent((self.ns + PAD) * UPGRADE_REPLY_DTYPE.itemsize)
        self.count = sent((3 + PAD) * 8).view(torch.int64)

    def run(self, codec, d_wire, max_response=0, stream=None):
        codec.upgrade_client_streams(d_wire, self.spans, self.nonces, max_response=max_response, stream=stream,
                                     up=self.up, count=self.count)

    def check(self, want, spans):
        up, consumed, need, count, bad = want
        ns = self.ns
        got_up = self.up.cpu().numpy()
        assert got_up[: ns * 32].tobytes() == up.tobytes(), first_diff(got_up[: ns * 32].view(UPGRADE_REPLY_DTYPE), up)
        assert (got_up[ns * 32:] == SENTINEL).all()
        sp = self.spans.cpu().numpy().view(STREAM_SPAN)
        assert np.array_equal(sp["off"], spans["off"]) and np.array_equal(sp["len"], spans["len"])
        assert np.array_equal(sp["consumed"], consumed) and np.array_equal(sp["need"], need)
        cnt = self.count.cpu().numpy().view(np.uint64)
        assert np.array_equal(cnt[:3], count) and (cnt[3:] == WORD).all()


def first_diff(got, want):
    for j in range(len(want)):
        if got[j].tobytes() != want[j].tobytes():
            return "stream %d: got %s, want %s" % (j, got[j], want[j])
    return "equal"


def run_check(codec, wire, spans, nonces, max_response=0, status=None, stream=None):
    """One call against the model."""
    want = layout.upgrade_client_plan(wire, spans, nonces, max_response)
    o = UcOut(spans, nonces)
    o.run(codec, padded_dev(wire), max_response, stream)
    if status is None:
        status = ca.WSG_EINVAL if want[4].any() else 0
    assert codec.sync_status(stream) == status
    o.check(want, spans)
    return want


def run_cases(codec, cases, **kw):
    wire, spans, nonces = uc.batch(cases, **{k: kw.pop(k) for k in ("align", "gap") if k in kw})
    return run_check(codec, wire, spans, nonces, **kw)


def with_nonce(datas, nonce=uc.NONCE):
    return [(d, nonce) for d in datas]


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("env", [dict(WSG_DEC_BLOCKS_PER_CU=1), {}], ids=["1-block-per-cu", "default"])
def test_every_case_in_one_batch(env):
    """The hand cases and the 2000 fuzz cases back to back (span offsets of
    every alignment): more streams than one block counts, and with one block
    per CU (4 waves each) more than one pass of the grid's waves."""
    cases = uc.all_cases()
    assert len(cases) > 4 * 256 * 2
    c = _codec(**env)
    try:
        want = run_cases(c, cases)
    finally:
        c.close()
    assert [int(x) for x in want[0]["code"]] == [e["code"] for e in uc.expected()]


@functools.lru_cache(maxsize=None)
def short_cases():
    """The hand cases without the prefixes, and every 16th prefix."""
    return tuple((d, n) for name, d, n in uc.hand_cases() if not name.startswith("prefix_") or int(name[7:]) % 16 == 5)


@pytest.mark.parametrize("align", range(16))
def test_span_alignment(codec, align):
    wire, spans, nonces = uc.batch(short_cases(), align=align)
    assert (spans["off"] % 16 == align).all()
    run_check(codec, wire, spans, nonces)


# ------------------------------------------------- tile edges and carried bytes
def edge_responses():
    """The header end at every offset from 1017 to 1031 of the span, and from
    2041 to 2055: the tile edges with the three carried bytes on both sides;
    the same with a failing header and a body behind the header end."""
    out = []
    wrong = b"Sec-WebSocket-Accept: " + uc.ACCEPT.replace(b"z", b"y")
    for at in list(range(1017, 1032)) + list(range(2041, 2056)):
        out.append(uc.padded_to(at + 4) + b"\x81\x00")
        out.append(uc.padded_to(at + 4, uc.three(accept=wrong) + [b"Content-Length: 2"]) + b"ab")
        out.append(uc.padded_to(at + 4)[:-1])   # one byte short of the header end
    return out


@pytest.mark.parametrize("align", [0, 1, 13])
def test_header_end_at_tile_edges(codec, align):
    want = run_cases(codec, with_nonce(edge_responses()), align=align)
    assert list(want[0]["code"][:3]) == [layout.UC_ACCEPTED, layout.UC_BAD_ACCEPT, layout.UC_INCOMPLETE]
    assert int(want[1][0]) == 1021 and int(want[1][1]) == 1023


def straddle_responses():
    """The accept line at every start from 1024 - 60 to 1024 + 4 of the span
    (its first byte, the inside of its name, its ':' and its value each cross
    the tile edge in turn), right and wrong, and one header per tile, the
    walk's verdict carried across them."""
    out = []
    wrong = uc.ACCEPT[:20] + b"A" + uc.ACCEPT[21:]
    for start in range(1024 - 60, 1024 + 5):
        head = b"HTTP/1.1 101 Switching Protocols\r\nServer: s"
        pad = start - len(head) - 2
        lines = [b"Server: s" + b"x" * pad, b"Sec-WebSocket-Accept: " + uc.ACCEPT, b"Upgrade: websocket",
                 b"Connection: Upgrade"]
        resp = uc.response(lines)
        assert resp.find(b"Sec-WebSocket-Accept") == start
        out.append(resp)
        out.append(uc.response(lines[:1] + [b"Upgrade: websocket", b"Sec-WebSocket-Accept: " + wrong] + lines[3:]))
    filler = b"X-Filler: " + b"y" * 1000
    spread = [b"Sec-WebSocket-Accept: " + uc.ACCEPT, filler, b"Upgrade: websocket", filler, b"Connection: Upgrade"]
    out.append(uc.response(spread))
    out.append(uc.response(spread[:-1] + [b"Connection: close"]))
    out.append(uc.response(spread + [filler, b"Sec-WebSocket-Accept: " + wrong]))            # behind a complete set
    out.append(uc.response([b"Sec-WebSocket-Accept: " + wrong, filler] + spread))           # in front of it
    out.append(uc.response(spread + [b"Content-Length: 7", filler, b"content-length: 3"], body=b"abcdef"))
    out.append(uc.response([filler, b"no colon here", filler] + spread))
    out.append(uc.response([b"Upgrade: nope", filler] + spread))
    return out


@pytest.mark.parametrize("align", [0, 9])
def test_lines_across_tile_edges(codec, align):
    resps = straddle_responses()
    want = run_cases(codec, with_nonce(resps), align=align)
    tail = [int(c) for c in want[0]["code"][-7:]]
    assert tail == [layout.UC_ACCEPTED, layout.UC_BAD_CONNECTION, layout.UC_ACCEPTED, layout.UC_BAD_ACCEPT,
                    layout.UC_ACCEPTED, layout.UC_BAD_HTTP, layout.UC_BAD_UPGRADE]
    assert int(want[1][-3]) == len(resps[-3]) - 3
    # the accept value reported by the complete set with a wrong one behind it is that wrong one
    off = int(want[0]["accept_off"][-5]) - int(uc.batch(with_nonce(resps), align=align)[1]["off"][-5])
    assert resps[-5][off:off + 28] == uc.ACCEPT[:20] + b"A" + uc.ACCEPT[21:]


def test_long_response(codec):
    resp = uc.padded_to(5000) + uc.unmasked_text(b"after")
    want = run_cases(codec, with_nonce([resp, resp[:4999], resp]), align=3)
    assert [int(c) for c in want[1]] == [5000, 0, 5000]


def test_status_digits_across_a_block_edge(codec):
    """The three digits at every phase of a 16-byte block, right and wrong."""
    cases = []
    for shift in range(20):
        for line in (b"101 Switching Protocols", b"101", b"1010", b"10", b"201 x", b"1 1 x"):
            cases.append(uc.response(uc.three(), start=b"H" * (1 + shift) + b" " + line))
    for align in (0, 5):
        want = run_cases(codec, with_nonce(cases), align=align)
        assert [int(c) for c in want[0]["code"][:6]] == [1, 1, layout.UC_BAD_HTTP, layout.UC_BAD_HTTP,
                                                         layout.UC_NOT_101, layout.UC_BAD_HTTP]


# ------------------------------------------------------------ stream counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_stream_counts(codec, n):
    rng = np.random.default_rng(n)
    pool = uc.all_cases()
    cases = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    wire, spans, nonces = uc.batch(cases, gap=1)
    if n == 0:
        wire = np.zeros(0, dtype=np.uint8)
    run_check(codec, wire, spans, nonces)


def test_neighbours_with_their_own_nonces(codec):
    """The same bytes in neighbouring streams, a nonce each: stream j is
    accepted only where the response was made for nonce j."""
    rng = np.random.default_rng(7)
    nonces = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(70)]
    cases = []
    for j, nonce in enumerate(nonces):
        made_for = nonces[j] if j % 3 else nonces[(j + 1) % len(nonces)]
        cases.append((uc.server_response(made_for), nonce))
    same = uc.server_response(nonces[5])
    cases += [(same, n) for n in nonces[:10]]
    want = run_cases(codec, cases)
    codes = [int(c) for c in want[0]["code"]]
    assert codes[:70] == [layout.UC_ACCEPTED if j % 3 else layout.UC_BAD_ACCEPT for j in range(70)]
    assert codes[70:] == [layout.UC_ACCEPTED if j == 5 else layout.UC_BAD_ACCEPT for j in range(10)]


def test_empty_streams_between_full_ones(codec):
    cases = []
    for k in range(40):
        cases += [uc.RFC_RESPONSE, b"", b"", uc.server_response(uc.NONCE)][: 1 + k % 4]
    want = run_cases(codec, with_nonce(cases))
    assert int(want[3][2]) == sum(1 for c in cases if not c)


def test_bad_spans_among_good_ones(codec):
    wire, spans, nonces = uc.batch(with_nonce([uc.RFC_RESPONSE] * 10), gap=5)
    spans["len"][2] = len(wire)                  # runs past the wire
    spans["off"][6] = int(spans["off"][5]) + 3   # starts inside the span before it
    spans["off"][9] = len(wire) + 1
    want = run_check(codec, wire, spans, nonces)
    assert list(np.flatnonzero(want[4])) == [2, 6, 9]
    assert list(want[0]["code"][[2, 6, 9]]) == [0, 0, 0] and int(want[3][0]) == 7 and int(want[3][2]) == 3


def test_max_response(codec):
    short = uc.RFC_RESPONSE[:100]
    body = uc.response(uc.three() + [b"Content-Length: 50"], body=b"abc")
    assert len(body) != len(short)
    cases = with_nonce([short, uc.RFC_RESPONSE, body, b"", uc.response(uc.three(upgrade=b"Upgrade: nope"))])
    for n in (len(short), len(body)):
        for limit in (n - 1, n, n + 1):
            want = run_cases(codec, cases, gap=2, max_response=limit)
            codes = [int(c) for c in want[0]["code"]]
            assert codes[0] == (layout.UC_TOO_LONG if len(short) >= limit else layout.UC_INCOMPLETE)
            assert codes[2] == (layout.UC_TOO_LONG if len(body) >= limit else layout.UC_INCOMPLETE)
            assert codes[1] == layout.UC_ACCEPTED and codes[3] == layout.UC_INCOMPLETE and codes[4] == layout.UC_BAD_UPGRADE


# ------------------------------------------------------- streams and graphs
@functools.lru_cache(maxsize=None)
def _two_batches():
    """Two batches over the same spans with other bytes, nonces and outcomes."""
    a = list(uc.fuzz_cases()[:1500])
    rng = np.random.default_rng(11)
    other = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    a = [(d, n) for _, d, n in a]
    b = [(d.replace(b"websocket", b"websocked"), other if j % 2 else n) for j, (d, n) in enumerate(a)]
    wa, sa, na = uc.batch(a)
    wb, sb, nb = uc.batch(b)
    assert np.array_equal(sa, sb)
    pa, pb = layout.upgrade_client_plan(wa, sa, na), layout.upgrade_client_plan(wb, sb, nb)
    assert int((pa[0]["code"] != pb[0]["code"]).sum()) > 200
    return (wa, sa, na, pa), (wb, sb, nb, pb)


def test_side_stream(codec):
    (wa, sa, na, pa), _ = _two_batches()
    o = UcOut(sa, na)
    d_wire = padded_dev(wa)
    torch.cuda.synchronize()
    st = codec.own_stream()
    o.run(codec, d_wire, stream=st)
    o.run(codec, d_wire, stream=st)   # again behind it, no synchronisation between
    assert codec.sync_status(st) == 0
    o.check(pa, sa)


def test_graph_replay(codec):
    """Captured after one plain run of the same size, replayed over other
    bytes and other nonces."""
    (wa, sa, na, pa), (wb, sb, nb, pb) = _two_batches()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_wire = padded_dev(wa)
        o = UcOut(sa, na)
        o.run(codec, d_wire)
        assert codec.sync_status(st) == 0
        o.check(pa, sa)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            o.run(codec, d_wire)
        for w, s, n, want in ((wb, sb, nb, pb), (wa, sa, na, pa), (wb, sb, nb, pb)):
            d_wire.copy_(torch.from_numpy(w))
            # the captured call reads and writes the buffers it was captured with: refill them in place
            o.spans.copy_(dev(spans_in(s).view(np.uint8)))
            o.nonces[: len(n)].copy_(dev(n))
            for t in (o.up, o.count.view(torch.uint8)):
                t.fill_(SENTINEL)
            g.replay()
            assert codec.sync_status(st) == 0
            o.check(want, s)


# ------------------------------------------------------------ the arguments
def test_arguments(codec):
    wire, spans, nonces = uc.batch(with_nonce([uc.RFC_RESPONSE]))
    d_wire = padded_dev(wire)
    o = UcOut(spans, nonces)
    L, vp = ca.lib(), ctypes.c_void_p

    def call(wire_p=None, span_p=None, nonce_p=None, up_p=None, count_p=None, ns=1):
        return L.wsg_upgrade_client_streams(codec._ctx, vp(d_wire.data_ptr() if wire_p is None else wire_p), len(wire),
                                            vp(o.spans.data_ptr() if span_p is None else span_p), ns,
                                            vp(o.nonces.data_ptr() if nonce_p is None else nonce_p), 0,
                                            vp(o.up.data_ptr() if up_p is None else up_p),
                                            vp(o.count.data_ptr() if count_p is None else count_p), codec._stream(None))

    assert call(wire_p=d_wire.data_ptr() + 8) == ca.WSG_EINVAL
    assert call(nonce_p=o.nonces.data_ptr() + 8) == ca.WSG_EINVAL
    assert call(span_p=o.spans.data_ptr() + 4) == ca.WSG_EINVAL
    assert call(up_p=o.up.data_ptr() + 4) == ca.WSG_EINVAL
    assert call(count_p=o.count.data_ptr() + 4) == ca.WSG_EINVAL
    for null in ("wire_p", "span_p", "nonce_p", "up_p", "count_p"):
        assert call(**{null: 0}) == ca.WSG_EINVAL, null
    assert call(ns=0xFFFFFFFF) == ca.WSG_EINVAL
    assert L.wsg_upgrade_client_streams(None, vp(d_wire.data_ptr()), len(wire), vp(o.spans.data_ptr()), 1,
                                        vp(o.nonces.data_ptr()), 0, vp(o.up.data_ptr()), vp(o.count.data_ptr()),
                                        codec._stream(None)) == ca.WSG_EINVAL
    assert codec.sync_status() == 0
    assert (o.up.cpu().numpy() == SENTINEL).all(), "launched despite WSG_EINVAL"
    assert call() == 0 and codec.sync_status() == 0
    o.check(layout.upgrade_client_plan(wire, spans, nonces), spans)


def test_checked_launch_refuses_short_blocks(monkeypatch):
    """$WSG_CHECK=1 with every operand an exact hipMalloc block (torch's
    allocator hands out views of larger segments): each operand in turn one
    unit short is WSG_EINVAL on the host with nothing launched; with the
    exact blocks the call runs."""
    monkeypatch.setenv("WSG_CHECK", "1")
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    cases = with_nonce([uc.RFC_RESPONSE, uc.response(uc.three(upgrade=b"Upgrade: nope")), uc.server_response(uc.NONCE)])
    wire, spans, nonces = uc.batch(cases)
    ns = len(cases)
    want = layout.upgrade_client_plan(wire, spans, nonces)
    sizes = dict(wire=(len(wire) + 15) // 16 * 16, span=32 * ns, nonce=16 * ns, up=32 * ns, count=24)
    units = dict(wire=16, span=32, nonce=16, up=32, count=8)

    def alloc(n):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(n)) == 0
        return p

    def upload(p, a):
        a = np.ascontiguousarray(a)
        assert hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0

    def download(p, n):
        a = np.zeros(n, dtype=np.uint8)
        assert hip.hipMemcpy(a.ctypes.data_as(ctypes.c_void_p), p, ctypes.c_size_t(n), 2) == 0
        return a

    full = {k: alloc(n) for k, n in sizes.items()}
    short = {k: alloc(n - units[k]) for k, n in sizes.items()}
    c = ca.Codec(0)
    try:
        def call(blocks):
            return ca.lib().wsg_upgrade_client_streams(c._ctx, blocks["wire"], len(wire), blocks["span"], ns,
                                                       blocks["nonce"], 0, blocks["up"], blocks["count"], c._stream(None))

        for blocks in (full, short):
            upload(blocks["wire"], wire[: sizes["wire"] - (0 if blocks is full else 16)])
            upload(blocks["span"], spans_in(spans)[: ns if blocks is full else ns - 1].view(np.uint8))
            upload(blocks["nonce"], nonces[: sizes["nonce"] - (0 if blocks is full else 16)])
        upload(full["up"], np.full(sizes["up"], SENTINEL, dtype=np.uint8))
        upload(full["count"], np.full(24, SENTINEL, dtype=np.uint8))
        for k in sizes:
            assert call(dict(full, **{k: short[k]})) == ca.WSG_EINVAL, k
            assert c.sync_status() == 0
            assert (download(full["up"], sizes["up"]) == SENTINEL).all(), "launched despite WSG_EINVAL (%s)" % k
            assert (download(full["count"], 24) == SENTINEL).all(), k
        assert call(full) == 0 and c.sync_status() == 0
        assert download(full["up"], sizes["up"]).tobytes() == want[0].tobytes()
        assert np.array_equal(download(full["count"], 24).view(np.uint64), want[3])
        sp = download(full["span"], sizes["span"]).view(STREAM_SPAN)
        assert np.array_equal(sp["consumed"], want[1]) and np.array_equal(sp["need"], want[2])
    finally:
        c.close()
        for p in list(full.values()) + list(short.values()):
            hip.hipFree(p)


# ------------------------------------------------------- wsg_upgrade_requests
def request_check(codec, tpl, key_at, nonces, stream=None):
    """One call with req_cap exactly n * tpl_len and a sentinel behind it."""
    n, tpl_len = len(nonces) // 16, len(tpl)
    total = n * tpl_len
    d_tpl = padded_dev(np.frombuffer(tpl, dtype=np.uint8))
    d_nonce = dev(nonces) if n else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    req = sent(total + PAD)
    codec.upgrade_requests(d_tpl, key_at, d_nonce, req=req, req_cap=total, stream=stream)
    assert codec.sync_status(stream) == 0
    got = req.cpu().numpy()
    assert (got[total:] == SENTINEL).all(), "a byte at or behind n * tpl_len"
    return got[:total]


def template(tpl_len, key_at, seed=0):
    rng = np.random.default_rng(1000 * tpl_len + key_at + seed)
    t = bytearray(rng.integers(0, 256, tpl_len, dtype=np.uint8).tobytes())
    t[key_at:key_at + 24] = b"=" * 24
    return bytes(t)


@pytest.mark.parametrize("tpl_len", [24, 25, 39, 40, 41, 230, 1031])
def test_requests_template_lengths(codec, tpl_len):
    """Every request of 257 at every length and hole: a request's start is at
    any phase of a 16-byte block, a block holds the end of one request and the
    start of the next, the hole crosses blocks and requests' edges."""
    rng = np.random.default_rng(tpl_len)
    nonces = rng.integers(0, 256, 16 * 257, dtype=np.uint8)
    for key_at in sorted({0, 1, 15, 16, tpl_len - 24} & set(range(tpl_len - 23))):
        tpl = template(tpl_len, key_at)
        for n in (0, 1, 2, 257):
            got = request_check(codec, tpl, key_at, nonces[: 16 * n])
            for j in range(n):
                want = layout.upgrade_request(tpl, key_at, nonces[16 * j:16 * j + 16].tobytes())
                assert got[j * tpl_len:(j + 1) * tpl_len].tobytes() == want, (key_at, n, j)


def test_requests_70000(codec):
    """More requests than one pass of the grid takes, compared as one array."""
    tpl_len, key_at, n = 41, 15, 70000
    tpl = template(tpl_len, key_at)
    rng = np.random.default_rng(70)
    nonces = rng.integers(0, 256, 16 * n, dtype=np.uint8)
    got = request_check(codec, tpl, key_at, nonces).reshape(n, tpl_len)
    abc = np.frombuffer(layout._B64, dtype=np.uint8)
    b = np.concatenate([nonces.reshape(n, 16), np.zeros((n, 2), dtype=np.uint8)], axis=1).astype(np.uint32)
    v = (b[:, 0::3] << 16) | (b[:, 1::3] << 8) | b[:, 2::3]
    key = np.stack([abc[(v >> s) & 63] for s in (18, 12, 6, 0)], axis=2).reshape(n, 24)
    key[:, 22:] = ord("=")
    want = np.tile(np.frombuffer(tpl, dtype=np.uint8), (n, 1))
    want[:, key_at:key_at + 24] = key
    assert want[3].tobytes() == layout.upgrade_request(tpl, key_at, nonces[48:64].tobytes())
    assert np.array_equal(got, want)


def test_requests_for_the_server(codec):
    """The reference client's request: every one of 300 is accepted by the
    model of the server's half, with the value this nonce expects."""
    head = (b"GET / HTTP/1.1\r\nHost: localhost\r\nOrigin: http://localhost\r\nUpgrade: websocket\r\n"
            b"Connection: Upgrade\r\nSec-WebSocket-Key: ")
    tpl = head + b"=" * 24 + b"\r\nSec-WebSocket-Protocol: chat, superchat\r\nSec-WebSocket-Version: 13\r\nContent-Length: 0\r\n\r\n"
    rng = np.random.default_rng(5)
    nonces = rng.integers(0, 256, 16 * 300, dtype=np.uint8)
    got = request_check(codec, tpl, len(head), nonces, stream=codec.own_stream()).reshape(300, len(tpl))
    for j in range(300):
        nonce = nonces[16 * j:16 * j + 16].tobytes()
        e = layout.upgrade_judge(got[j].tobytes())
        assert e["code"] == layout.UP_ACCEPTED
        assert e["resp"][97:125] == base64.b64encode(layout.upgrade_expect(nonce))


def test_requests_capacity_and_arguments(codec):
    tpl_len, key_at, n = 41, 17, 5
    tpl = template(tpl_len, key_at)
    d_tpl = padded_dev(np.frombuffer(tpl, dtype=np.uint8))
    d_nonce = dev(np.arange(16 * n, dtype=np.uint8))
    req = sent(n * tpl_len + PAD)
    L, vp = ca.lib(), ctypes.c_void_p

    def call(tpl_p=None, nonce_p=None, req_p=None, cap=n * tpl_len, length=tpl_len, at=key_at, count=n, ctx=codec._ctx):
        return L.wsg_upgrade_requests(ctx, vp(d_tpl.data_ptr() if tpl_p is None else tpl_p), length, at,
                                      vp(d_nonce.data_ptr() if nonce_p is None else nonce_p), count,
                                      vp(req.data_ptr() if req_p is None else req_p), cap, codec._stream(None))

    assert call(cap=n * tpl_len - 1) == ca.WSG_ENOMEM
    assert call(at=tpl_len - 23) == ca.WSG_EINVAL
    assert call(length=23, at=0, cap=1 << 20) == ca.WSG_EINVAL
    assert call(length=0, at=0) == ca.WSG_EINVAL
    assert call(at=0xFFFFFFF0) == ca.WSG_EINVAL
    assert call(ctx=None) == ca.WSG_EINVAL
    for name in ("tpl_p", "nonce_p", "req_p"):
        assert call(**{name: 0}) == ca.WSG_EINVAL, name
    assert call(tpl_p=d_tpl.data_ptr() + 8, length=tpl_len - 8) == ca.WSG_EINVAL
    assert call(nonce_p=d_nonce.data_ptr() + 8, count=n - 1) == ca.WSG_EINVAL
    assert call(req_p=req.data_ptr() + 8) == ca.WSG_EINVAL
    assert call(count=0, tpl_p=0, nonce_p=0, req_p=0, cap=0) == 0   # no request: nothing needed
    assert codec.sync_status() == 0
    assert (req.cpu().numpy() == SENTINEL).all(), "d_req touched by a refused call"
    assert call() == 0 and codec.sync_status() == 0
    got = req.cpu().numpy()
    assert (got[n * tpl_len:] == SENTINEL).all()
    assert got[:tpl_len].tobytes() == layout.upgrade_request(tpl, key_at, bytes(range(16)))
