"""wsg_carry_streams on the device against layout.carry_plan (which
tests/test_carry_model.py holds against the plain loop): every byte of
d_next[0, count[0]), every span and every count, over the shapes where the
kernels can go wrong.

d_next, d_next_span and d_count are filled with 0xA5 first and have a sentinel
region behind what the call may write, which must stay as it was.  Both
sources lie in buffers of random bytes, so nothing from a gap between spans or
from behind wire_len / new_len may show in d_next.  Bit-exact throughout."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import STREAM_READ, STREAM_SPAN  # noqa: E402
from tests import carry_cases as kc  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests.test_gpu_async import _gate  # noqa: E402
from tests.test_gpu_frames import FrameOut, SENTINEL, dev, frame, sent  # noqa: E402
from tests.test_gpu_launch_shapes import _codec  # noqa: E402

PAD = 64   # sentinel entries (bytes of d_next) behind every output
SENT64 = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


class Dev:
    """A case's inputs on the device: the sources with their random bytes
    behind wire_len and new_len."""

    def __init__(self, case):
        self.wire = dev(case.wire_raw)[: len(case.wire)]
        self.new = dev(case.new_raw)[: len(case.new)]
        self.spans = dev(case.spans.view(np.uint8))
        self.reads = None if case.reads is None else dev(case.reads.view(np.uint8))
        self.close_off = None if case.close_off is None else dev(case.close_off.view(np.int64))


class CarryOut:
    """Sentinel-filled outputs of one call over ns streams, ``cap`` bytes of d_next."""

    def __init__(self, ns, cap):
        self.ns, self.cap = ns, int(cap)
        self.next = sent(self.cap + PAD)
        self.next_spans = sent((ns + PAD) * STREAM_SPAN.itemsize)
        self.count = sent((4 + PAD) * 8).view(torch.int64)

    def refill(self):
        for t in (self.next, self.next_spans, self.count.view(torch.uint8)):
            t.fill_(SENTINEL)

    def run(self, codec, d, stream=None):
        codec.carry_streams(d.wire, d.spans, d.new, d.reads, close_off=d.close_off, next=self.next, next_cap=self.cap,
                            next_spans=self.next_spans, count=self.count, stream=stream)

    def check(self, want):
        nxt, spans, count, _ = want
        ns, total = self.ns, len(nxt)
        cnt = self.count.cpu().numpy().view(np.uint64)
        assert [int(x) for x in cnt[:4]] == [int(x) for x in count] and (cnt[4:] == SENT64).all()
        sp = self.next_spans.cpu().numpy()
        got_sp = sp[: ns * 32].view(STREAM_SPAN)
        assert got_sp.tobytes() == spans.tobytes(), first_diff(got_sp, spans)
        assert (sp[ns * 32:] == SENTINEL).all()
        got = self.next.cpu().numpy()
        if total <= self.cap:
            if not np.array_equal(got[:total], nxt):
                at = int(np.flatnonzero(got[:total] != nxt)[0])
                j = int(np.searchsorted(spans["off"], at, side="right")) - 1
                raise AssertionError("d_next differs at byte %d (stream %d at %d, %d bytes)"
                                     % (at, j, int(spans["off"][j]), int(spans["len"][j])))
            assert (got[total:] == SENTINEL).all(), "a byte behind d_count[0]"
        else:
            assert (got == SENTINEL).all(), "a byte of d_next despite WSG_ENOMEM"


def first_diff(got, want):
    for j in range(len(want)):
        if got[j].tobytes() != want[j].tobytes():
            return "stream %d: got %s, want %s" % (j, got[j], want[j])
    return "equal"


def run_check(codec, case, cap=None, stream=None):
    """One call with d_next sized exactly (or ``cap``), against the model; the
    status wsg_sync gives is the model's key's."""
    want = case.plan(cap)
    cap = int(want[2][0]) if cap is None else cap
    o = CarryOut(case.ns, cap)
    o.run(codec, Dev(case), stream)
    assert codec.sync_status(stream) == (0 if want[3] is None else -(want[3] & 0xFF))
    assert codec.sync_status(stream) == 0
    o.check(want)
    return want


# ------------------------------------------------------------------ 1, 4: alignments, garbage around the sources
def test_alignments(codec):
    """Tail and read lengths around one and two chunks at every source
    alignment, 4096 streams in one batch (16 blocks of the scan), random bytes
    in every gap and behind both sources."""
    case = kc.alignments(np.random.default_rng(11))
    assert case.ns == 4096
    want = run_check(codec, case)
    assert int(want[2][1]) and int(want[2][2])


# ------------------------------------------------------------------ 2: piece edges
@pytest.mark.parametrize("env", [dict(WSG_DEC_BLOCKS_PER_CU=1), {}], ids=["1-block-per-cu", "default"])
def test_piece_edges(env):
    """Runs that end one byte before, at and behind a 4 KiB piece, and a stream
    of 3 MiB + 7 with a read of 1 MiB + 3: with one block per CU (four waves of
    one piece each) more than 4 MiB is more than one pass of the grid."""
    case = kc.piece_edges(np.random.default_rng(12))
    c = _codec(**env)
    try:
        want = run_check(c, case)
    finally:
        c.close()
    assert int(want[2][0]) > 4 << 20


# ------------------------------------------------------------------ 3: shapes
def test_stream_shapes(codec):
    """Tail only, read only, both empty, dropped, dropped with a read."""
    rng = np.random.default_rng(13)
    tails = [30, 0, 0, 25, 40, 7, 0]
    news = [0, 30, 0, 0, 33, 9, 0]
    drop = [0, 0, 0, 1, 1, 0, 1]
    want = run_check(codec, kc.make(rng, tails, news, drop=drop))
    assert [int(x) for x in want[1]["len"]] == [30, 30, 0, 0, 0, 16, 0] and int(want[2][3]) == 3
    run_check(codec, kc.make(rng, tails, news, close=False))
    run_check(codec, kc.make(rng, tails, news, drop=drop, reads=False))
    run_check(codec, kc.make(rng, tails, news, reads=False, close=False))


@pytest.mark.parametrize("ns", [0, 1, 255, 256, 257, 70000])
def test_stream_counts(codec, ns):
    rng = np.random.default_rng([14, ns])
    run_check(codec, kc.make(rng, rng.integers(0, 41, ns), rng.integers(0, 41, ns), drop=rng.random(ns) < 0.05))


def test_first_round(codec):
    """No wire at all (NULL, 0 bytes) and a zeroed span table."""
    rng = np.random.default_rng(15)
    case = kc.make(rng, [0] * 300, rng.integers(0, 300, 300), consumed=[0] * 300, close=False)
    case.spans[:] = 0
    want = case.plan()
    o = CarryOut(case.ns, int(want[2][0]))
    d = Dev(case)
    d.wire = None
    o.run(codec, d)
    assert codec.sync_status() == 0
    o.check(want)
    assert int(want[2][1]) == 0 and int(want[2][2]) == int(case.reads["len"].sum())


# ------------------------------------------------------------------ 5: errors
def test_refused_streams(codec):
    """A span past wire_len, an overlapping span, consumed > len, a read past
    new_len: WSG_EINVAL for wsg_sync, that stream empty, the others right."""
    rng = np.random.default_rng(16)
    base = kc.make(rng, rng.integers(0, 200, 600), rng.integers(0, 200, 600), consumed=rng.integers(1, 30, 600))
    for j, table, field, value in ((300, "spans", "len", len(base.wire)), (301, "spans", "off", int(base.spans["off"][300])),
                                   (257, "spans", "consumed", int(base.spans["len"][257]) + 1),
                                   (599, "reads", "off", len(base.new)), (0, "reads", "len", len(base.new) + 1)):
        case = kc.Case(base.wire_raw, len(base.wire), base.spans.copy(), base.new_raw, len(base.new), base.reads.copy(),
                       base.close_off)
        getattr(case, table)[field][j] = value
        want = run_check(codec, case)
        assert want[3] == (j << 8 | 22) and int(want[1]["len"][j]) == 0


def test_capacity(codec):
    """next_cap exact; one chunk short is WSG_ENOMEM with d_next untouched and
    the tables final."""
    rng = np.random.default_rng(17)
    case = kc.make(rng, rng.integers(0, 100, 500), rng.integers(0, 100, 500))
    total = int(case.plan()[2][0])
    assert run_check(codec, case, cap=total)[3] is None
    assert run_check(codec, case, cap=total - 16)[3] == (500 << 8 | 12)
    assert run_check(codec, case, cap=0)[3] == (500 << 8 | 12)


def test_arguments(codec):
    case = kc.make(np.random.default_rng(18), [20, 5], [7, 40])
    want = case.plan()
    d, o = Dev(case), CarryOut(2, int(want[2][0]))
    L, vp = ca.lib(), ctypes.c_void_p
    ptrs = dict(wire=d.wire, span=d.spans, close=d.close_off, new=d.new, read=d.reads, next=o.next, nspan=o.next_spans,
                count=o.count)

    def call(**other):
        p = {k: other.get(k, t.data_ptr()) for k, t in ptrs.items()}
        return L.wsg_carry_streams(codec._ctx, vp(p["wire"]), len(case.wire), vp(p["span"]), 2, vp(p["close"]),
                                   vp(p["new"]), len(case.new), vp(p["read"]), vp(p["next"]), o.cap, vp(p["nspan"]),
                                   vp(p["count"]), codec._stream(None))

    for name, t in ptrs.items():
        assert call(**{name: t.data_ptr() + 4}) == ca.WSG_EINVAL, name + " misaligned"
    for name in ("wire", "new", "next"):
        assert call(**{name: ptrs[name].data_ptr() + 8}) == ca.WSG_EINVAL, name + " 8-byte aligned"
    for name in ("wire", "span", "new", "next", "nspan", "count"):
        assert call(**{name: 0}) == ca.WSG_EINVAL, name + " NULL"
    assert call(nspan=d.spans.data_ptr()) == ca.WSG_EINVAL, "d_next_span is d_span"
    assert call(next=d.wire.data_ptr()) == ca.WSG_EINVAL and call(next=d.new.data_ptr()) == ca.WSG_EINVAL
    assert codec.sync_status() == 0
    assert (o.next.cpu().numpy() == SENTINEL).all() and (o.next_spans.cpu().numpy() == SENTINEL).all(), \
        "launched despite WSG_EINVAL"
    assert call() == 0 and codec.sync_status() == 0
    o.check(want)
    o.refill()
    assert call(close=0, read=0) == 0 and codec.sync_status() == 0   # the two that may be NULL
    o.check(layout.carry_plan(case.wire, case.spans, case.new, None))


def test_checked_launch_refuses_a_short_next(monkeypatch):
    """$WSG_CHECK=1: a d_next block one byte short of next_cap is WSG_EINVAL on
    the host and nothing is launched; with next_cap bytes the call runs.  The
    block is an exact hipMalloc block of 2 MiB (torch's allocator hands out
    views of larger segments)."""
    monkeypatch.setenv("WSG_CHECK", "1")
    hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
    block = ctypes.c_void_p()
    size = 2 << 20
    assert hip.hipMalloc(ctypes.byref(block), ctypes.c_size_t(size)) == 0
    c = ca.Codec(0)
    try:
        rng = np.random.default_rng(19)
        case = kc.make(rng, rng.integers(0, 3000, 300), rng.integers(0, 3000, 300))
        want = case.plan()
        total = int(want[2][0])
        assert total < size
        d, o = Dev(case), CarryOut(case.ns, 0)
        vp = ctypes.c_void_p

        def call(cap):
            return ca.lib().wsg_carry_streams(c._ctx, vp(d.wire.data_ptr()), len(case.wire), vp(d.spans.data_ptr()),
                                              case.ns, vp(d.close_off.data_ptr()), vp(d.new.data_ptr()), len(case.new),
                                              vp(d.reads.data_ptr()), block, cap, vp(o.next_spans.data_ptr()),
                                              vp(o.count.data_ptr()), c._stream(None))

        assert call(size + 1) == ca.WSG_EINVAL
        assert c.sync_status() == 0
        assert (o.next_spans.cpu().numpy() == SENTINEL).all(), "launched despite WSG_EINVAL"
        assert call(size) == 0
        assert c.sync_status() == 0
        got = torch.empty(total, dtype=torch.uint8, device="cuda")
        assert hip.hipMemcpy(vp(got.data_ptr()), block, ctypes.c_size_t(total), 3) == 0   # device to device
        assert np.array_equal(got.cpu().numpy(), want[0])
        assert [int(x) for x in o.count.cpu().numpy().view(np.uint64)[:4]] == [int(x) for x in want[2]]
    finally:
        c.close()
        hip.hipFree(block)


# ------------------------------------------------------------------ 6: async
def _two_cases():
    """Two batches of one geometry and other bytes (a replay's two inputs)."""
    out = []
    for seed in (20, 21):
        rng = np.random.default_rng(seed)
        shape = np.random.default_rng(22)
        out.append(kc.make(rng, shape.integers(0, 600, 900), shape.integers(0, 600, 900),
                           tail_mod=shape.integers(0, 16, 900), new_mod=shape.integers(0, 16, 900),
                           consumed=shape.integers(0, 30, 900), drop=shape.random(900) < 0.1))
    return out


def test_side_stream(codec):
    case = _two_cases()[0]
    want = case.plan()
    d, o = Dev(case), CarryOut(case.ns, int(want[2][0]))
    torch.cuda.synchronize()
    st = codec.own_stream()
    o.run(codec, d, stream=st)
    o.run(codec, d, stream=st)   # again behind it, no synchronisation between
    assert codec.sync_status(st) == 0
    o.check(want)


def test_graph_replay(codec):
    """Captured after one plain run with the same n_streams, replayed over
    sources whose bytes and tables changed."""
    a, b = _two_cases()
    cap = max(int(a.plan()[2][0]), int(b.plan()[2][0]))
    wire_room, new_room = max(len(a.wire_raw), len(b.wire_raw)), max(len(a.new_raw), len(b.new_raw))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d, o = Dev(a), CarryOut(a.ns, cap)
        d.wire = torch.zeros(wire_room, dtype=torch.uint8, device="cuda")
        d.new = torch.zeros(new_room, dtype=torch.uint8, device="cuda")

        def load(case):
            d.wire[: len(case.wire_raw)].copy_(torch.from_numpy(case.wire_raw))
            d.new[: len(case.new_raw)].copy_(torch.from_numpy(case.new_raw))
            d.spans.copy_(torch.from_numpy(case.spans.view(np.uint8)))
            d.reads.copy_(torch.from_numpy(case.reads.view(np.uint8)))
            d.close_off.copy_(torch.from_numpy(case.close_off.view(np.int64)))

        load(a)
        o.run(codec, d)
        assert codec.sync_status(st) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            o.run(codec, d)
        for case in (b, a, b):
            load(case)
            o.refill()
            g.replay()
            assert codec.sync_status(st) == 0
            # (the captured call has the room of both wires as wire_len and new_len)
            o.check(layout.carry_plan(d.wire.cpu().numpy(), case.spans, d.new.cpu().numpy(), case.reads, case.close_off))


def test_ordered_against_frame_streams(codec):
    """12 rounds of (carry_streams on S1, frame_streams on S2) on one context,
    queued behind a gate, each call into outputs of its own: the two calls
    share the context's scratch and are ordered on the device."""
    case = _two_cases()[0]
    want = case.plan()
    rng = np.random.default_rng(23)
    fw = fc.Wire([b"".join(mc.random_frames(rng, int(rng.integers(2, 20)), 200)) for _ in range(1500)])
    fwant = layout.frame_plan(fw.wire, fw.spans)
    d = Dev(case)
    d_fr = torch.zeros(len(fw.wire) + 32, dtype=torch.uint8, device="cuda")[: len(fw.wire)]
    d_fr.copy_(torch.from_numpy(fw.wire))
    warm_c, warm_f = CarryOut(case.ns, int(want[2][0])), FrameOut(fw.spans, int(fwant[3][0]))
    warm_c.run(codec, d)
    frame(codec, d_fr, warm_f)
    assert codec.sync_status() == 0
    outs = [(CarryOut(case.ns, int(want[2][0])), FrameOut(fw.spans, int(fwant[3][0]))) for _ in range(12)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gate = _gate([s1, s2])
    for oc, of in outs:
        oc.run(codec, d, stream=s1)
        frame(codec, d_fr, of, s2)
    opened = gate.query()
    assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
    torch.cuda.synchronize()
    assert not opened, "the gate opened before every call was queued"
    for oc, of in outs:
        oc.check(want)
        of.check(fwant, fw.spans)


# ------------------------------------------------------------------ 7, 8: offsets past 2^31 and 2^32
def _free_bytes():
    return torch.cuda.mem_get_info()[0]


def test_sources_past_4gib(codec):
    """A wire of 4 GiB + 1 MiB that is never filled but for a few hundred bytes
    around 2^31, around 2^32 and at its end: three tails across those marks,
    and reads, into a small d_next."""
    wire_len = (4 << 30) + (1 << 20)
    if _free_bytes() < wire_len + (1 << 30):
        pytest.skip("needs %d MiB of free device memory" % ((wire_len >> 20) + 1024))
    rng = np.random.default_rng(24)
    d_wire = torch.empty(wire_len + 16, dtype=torch.uint8, device="cuda")[:wire_len]
    marks = [(1 << 31) - 133, (1 << 32) - 77, wire_len - 170]
    used = [9, 0, 31]
    spans = np.zeros(3, dtype=STREAM_SPAN)
    small, small_spans = [], np.zeros(3, dtype=STREAM_SPAN)
    for j, (at, k) in enumerate(zip(marks, used)):
        data = rng.integers(0, 256, 170, dtype=np.uint8)
        d_wire[at: at + 170].copy_(torch.from_numpy(data))
        spans[j] = (at, 170, k, 0)
        small_spans[j] = (170 * j, 170, k, 0)   # the same streams in a wire of their own
        small.append(data)
    reads = np.zeros(3, dtype=STREAM_READ)
    reads["off"], reads["len"] = [3, 40, 90], [21, 0, 17]
    new = rng.integers(0, 256, 128, dtype=np.uint8)
    want = layout.carry_plan(np.concatenate(small), small_spans, new[:110], reads)
    o = CarryOut(3, int(want[2][0]))
    codec.carry_streams(d_wire, dev(spans.view(np.uint8)), dev(new)[:110], dev(reads.view(np.uint8)), next=o.next,
                        next_cap=o.cap, next_spans=o.next_spans, count=o.count)
    assert codec.sync_status() == 0
    o.check(want)
    assert int(want[2][1]) == 3 * 170 - sum(used)


def test_destination_past_4gib(codec):
    """A tail of 4 GiB + 32 bytes in front of three small streams: the small
    streams lie behind 2^32 in d_next and are compared byte for byte, the
    large one by a comparison on the device of sampled MiBs."""
    big = (4 << 30) + 32
    if _free_bytes() < 2 * big + (2 << 30):
        pytest.skip("needs %d MiB of free device memory" % ((2 * big >> 20) + 2048))
    rng = np.random.default_rng(25)
    small = kc.make(rng, [33, 0, 700], [15, 40, 300])
    shift = 5 + big + 11                      # the large span, a gap, then the small batch's wire
    shift += -shift % 16                      # (its source alignments stay what make() chose)
    d_wire = torch.empty(shift + len(small.wire_raw), dtype=torch.uint8, device="cuda")
    words = d_wire[: (5 + big + 11) // 8 * 8].view(torch.int64)
    torch.arange(words.numel(), out=words)   # every 8 bytes differ
    d_wire[shift:].copy_(torch.from_numpy(small.wire_raw))
    spans = np.zeros(4, dtype=STREAM_SPAN)
    spans[0] = (0, 5 + big, 5, 0)
    spans[1:] = small.spans
    spans["off"][1:] += shift
    reads = np.zeros(4, dtype=STREAM_READ)
    reads[1:] = small.reads
    close_off = np.full(4, kc.U64_MAX, dtype=np.uint64)
    want_small = small.plan()
    total = big + int(want_small[2][0])
    o = CarryOut(4, total)
    codec.carry_streams(d_wire[: shift + len(small.wire)], dev(spans.view(np.uint8)), dev(small.new_raw)[: len(small.new)],
                        dev(reads.view(np.uint8)), close_off=dev(close_off.view(np.int64)), next=o.next, next_cap=total,
                        next_spans=o.next_spans, count=o.count)
    assert codec.sync_status() == 0
    cnt = o.count.cpu().numpy().view(np.uint64)
    assert [int(x) for x in cnt[:4]] == [total, big + int(want_small[2][1]), int(want_small[2][2]), 0]
    assert (cnt[4:] == SENT64).all()
    got_sp = o.next_spans.cpu().numpy()[: 4 * 32].view(STREAM_SPAN)
    assert (int(got_sp["off"][0]), int(got_sp["len"][0])) == (0, big)
    assert np.array_equal(got_sp["off"][1:], want_small[1]["off"] + np.uint64(big))
    assert np.array_equal(got_sp["len"][1:], want_small[1]["len"]) and not got_sp["consumed"].any() and not got_sp["need"].any()
    assert np.array_equal(o.next[big: total].cpu().numpy(), want_small[0]), "the streams behind 2^32"
    assert (o.next[total:].cpu().numpy() == SENTINEL).all()
    mib = 1 << 20
    for at in (0, mib - 3, (1 << 31) - mib // 2, (1 << 32) - mib - 7, big - mib):   # (the last ends at 2^32 + 32)
        assert torch.equal(o.next[at: at + mib], d_wire[5 + at: 5 + at + mib]), "the MiB at %d" % at


# ------------------------------------------------------------------ 9: fuzz
@pytest.mark.parametrize("part", range(10))
def test_fuzz(codec, part):
    """100 seeded batches, ten a case: 1-3000 streams of no, a few, hundreds or
    tens of thousands of bytes, random drops, random source alignments, with
    and without d_read and d_close_off."""
    for seed in range(10 * part, 10 * part + 10):
        try:
            run_check(codec, kc.fuzz(seed))
        except AssertionError as e:
            raise AssertionError("seed %d: %s" % (seed, e))
