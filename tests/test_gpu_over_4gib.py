"""The device pipeline and the fan-out with offsets that need more than 32
bits: wsg_frame_streams, wsg_decode_messages, wsg_reply_messages,
wsg_decode_streams, wsg_reply_streams, wsg_check_utf8, wsg_fanout_encode and
wsg_fanout_encode_many at and above 2^31 (a sign extension shows there) and
2^32 (a truncation).  Bit-exact, no tolerances.

No expectation comes from a Python model run over gigabytes: every result
above a mark is the model's result for the same streams on a compact layout,
translated by tests/big_cases.py (proved against the models at small sizes in
tests/test_big_cases_model.py), or follows by construction (a filler frame's
payload is the wire XOR its key, compared in 1 GiB chunks on the device).

1. TestSparseWire: inputs above the marks.  One 5 GiB wire of 0xA5, a few KiB
   of real frames near the marks; the calls never read the rest.
2. TestDenseOutputs: outputs above 2^32.  A 4 GiB filler frame in front of a
   dozen small streams brings d_msg and d_reply past the mark.
3. TestUtf8AboveTheMarks: wsg_check_utf8 on a hand-made table over 4 GiB of
   NUL bytes.
4. The two fan-out calls with more than 2^32 + 2^28 bytes of frames, one
   shape per kernel.  Out of scope: the tiny-frame path (frames shorter than
   16 bytes) above 4 GiB, which would need some 300 million keys.

Every output table starts as the 0xA5 sentinel with PAD entries behind it."""
import ctypes
import os

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_SPAN, STREAM_STATE, frame_size  # noqa: E402
from tests import big_cases as bc  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import utf8_cases as uc  # noqa: E402
from tests.big_cases import MARK31, MARK32, MARKS  # noqa: E402
from tests.test_gpu_frames import PAD, FrameOut, StreamsOut, dev, frame, sent  # noqa: E402
from tests.test_gpu_parity import _xor_key_chunks  # noqa: E402
from tests.test_gpu_reply import SLACK, Out as ReplyOut, check_outputs as check_reply, d_keys_of  # noqa: E402
from tests.test_gpu_utf8 import check as utf8_check  # noqa: E402

SENTINEL = 0xA5
SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
U64_MAX = 2**64 - 1
GIB = 1 << 30
MIB = 1 << 20


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


def send_keys(ns):
    """One send key per stream, four distinct bytes each."""
    return (np.arange(ns, dtype=np.uint32) * np.uint32(0x01010101) + np.uint32(rc.KEY4)).astype(np.uint32)


def put(d_wire, data, spans):
    """The streams' bytes into place; everything else in the wire stays."""
    for d, s in zip(data, spans):
        if len(d):
            d_wire[int(s["off"]): int(s["off"]) + len(d)].copy_(torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()))


def all_equal(t, value):
    return bool((t == value).all().item())


# =============================================================================
# 1. Inputs above the marks: a sparse wire
# =============================================================================
def refused(want, spans, bad):
    """A frame plan with the streams `bad` refused: no frames, consumed and
    need 0 (layout.frame_plan's rule for a bad span), the others unchanged."""
    fs, sf, sp, _ = want
    keep = np.ones(len(fs), dtype=bool)
    counts = np.diff(sf.astype(np.int64))
    sp = np.array(sp, copy=True)
    for j in bad:
        keep[int(sf[j]): int(sf[j + 1])] = False
        counts[j] = 0
        sp["consumed"][j] = sp["need"][j] = 0
    for f in ("off", "len"):
        sp[f] = np.asarray(spans)[f]
    new_sf = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return fs[keep], new_sf, sp, np.array([int(keep.sum()), int(sp["consumed"].astype(object).sum())], dtype=np.uint64)


class TestSparseWire:
    @pytest.fixture(scope="class")
    def wire(self):
        """2^32 + 2^30 + 2^20 bytes of 0xA5, filled once: each case copies
        only its streams' bytes into place, so whatever lay there before is
        the gaps between them."""
        w = torch.full((bc.SPARSE_WIRE,), SENTINEL, dtype=torch.uint8, device="cuda")
        yield w
        del w
        torch.cuda.empty_cache()

    def test_frame_streams(self, codec, wire):
        """wsg_frame_streams against shift_frames in every field, every
        stream against the oracle's walk too (stream-relative offsets)."""
        for name, case in bc.sparse_cases().items():
            put(wire, case.data, case.spans)
            want = case.want_frames()
            o = FrameOut(case.spans, int(want[3][0]))
            frame(codec, wire, o)
            assert codec.sync_status() == 0, name
            o.check(want, case.spans)
            fs, sf, sp, _ = o.results()
            fc.check_against_oracle(case, fs, sf, sp)
            assert int(fs[: int(want[3][0])].max()) > MARK32 + GIB and (fs[: int(want[3][0])] > MARK31).sum() > 8

    def _frames_in(self, case):
        want = case.want_frames()
        return dev(want[0].view(np.int64)), dev(want[1].astype(np.int32)), int(want[3][0])

    def test_decode_messages(self, codec, wire):
        """wsg_decode_messages over the frame table: d_info is shift_info of
        the compact batch's; d_msgs, d_count, d_state and the bytes of d_msg
        are exactly the compact batch's (X's payload straddles a mark: the
        unmask key phase there)."""
        for name, case in bc.sparse_cases().items():
            put(wire, case.data, case.spans)
            m = case.model
            d_fs, d_sf, n = self._frames_in(case)
            o = StreamsOut(case.spans, n, len(case.compact.wire))
            o.n = n
            ns = case.n_streams
            codec.decode_messages(wire, d_fs, d_sf, state=o.state[: ns * STREAM_STATE.itemsize], msg=o.msg,
                                  msg_cap=o.msg_cap, msgs=o.msgs, count=o.f.count, info=o.info)
            assert codec.sync_status() == 0, name
            self._check_messages(o.host(), m, case, name)

    @staticmethod
    def _check_messages(h, m, case, name):
        assert [int(x) for x in h["count"]] == [int(x) for x in m["count"]], name
        mc.same_fields(h["info"], case.want_info(), mc.INFO_FIELDS)
        mc.same_fields(h["msgs"], m["msgs"], mc.MSG_FIELDS)
        mc.same_fields(h["state"], m["state"], ["consumed", "opcode"])
        assert np.array_equal(h["msg"], m["buf"]), name
        for tail in ("state_tail", "msgs_tail", "info_tail", "msg_tail"):
            assert (h[tail] == SENTINEL).all(), (name, tail)

    def _reply_want(self, case, mask, keys):
        m = case.model
        frames = rc.per_message(m["msgs"], rc.oracle_replies(m["batch"], rc.ECHO, mask, keys))
        plan = layout.reply_plan(m["msgs"], rc.ECHO, mask, keys, n_streams=case.n_streams)
        return m["msgs"], m["count"], m["state"], case.want_info(), frames, plan

    @pytest.mark.parametrize("mask", [0, 1])
    def test_reply_messages(self, codec, wire, mask):
        """wsg_reply_messages (the echo rule, one send key per stream): the
        reply bytes are the frames the oracle's sessions send for the compact
        batch, the offsets layout.reply_plan's."""
        for name, case in bc.sparse_cases().items():
            put(wire, case.data, case.spans)
            d_fs, d_sf, n = self._frames_in(case)
            ns = case.n_streams
            keys = send_keys(ns)
            cap = len(case.compact.wire) + 14 * n
            o = ReplyOut(n, ns, cap)
            o.launch(codec, wire, d_fs, d_sf, rc.ECHO, mask, d_keys_of(keys))
            assert codec.sync_status() == 0, name
            check_reply(o.host(), n, ns, cap, *self._reply_want(case, mask, keys))

    def test_decode_streams(self, codec, wire):
        """wsg_decode_streams on the same spans: the outputs of the two steps,
        and every span's consumed lowered to its first tail frame (above the
        mark in one straddling stream per mark and header form)."""
        for name, case in bc.sparse_cases().items():
            put(wire, case.data, case.spans)
            m = case.model
            want = case.want_frames()
            n = int(want[3][0])
            o = StreamsOut(case.spans, n, len(case.compact.wire))
            o.run(codec, wire)
            assert codec.sync_status() == 0 and o.n == n, name
            h = o.host()
            self._check_messages(h, m, case, name)
            self._check_framing(h, want, m, case, n, name)

    @staticmethod
    def _check_framing(h, want, m, case, n, name):
        ns = case.n_streams
        assert np.array_equal(h["fs"][:n], want[0]) and (h["fs"][n:] == SENT64).all(), name
        assert np.array_equal(h["sf"][: ns + 1], want[1].astype(np.uint32)) and (h["sf"][ns + 1:] == 0xA5A5A5A5).all()
        for f in ("off", "len", "need"):
            assert np.array_equal(h["spans"][f], want[2][f]), (name, f)
        assert np.array_equal(h["spans"]["consumed"], m["lowered"]), name

    @pytest.mark.parametrize("mask", [0, 1])
    def test_reply_streams(self, codec, wire, mask):
        for name, case in bc.sparse_cases().items():
            put(wire, case.data, case.spans)
            m = case.model
            want = case.want_frames()
            n, ns = int(want[3][0]), case.n_streams
            keys = send_keys(ns)
            cap = len(case.compact.wire) + 14 * n
            f, o = FrameOut(case.spans, n), ReplyOut(n, ns, cap)
            got_n = codec.reply_streams(wire, f.spans, reply_op=rc.ECHO, mask=mask, send_keys=d_keys_of(keys),
                                        state=o.state, frame_start=f.fs, frame_cap=n, stream_first=f.sf,
                                        reply=o.reply, reply_cap=cap, reply_off=o.reply_off,
                                        stream_reply=o.stream_reply, msgs=o.msgs, count=o.count, info=o.info)[-1]
            assert codec.sync_status() == 0 and got_n == n, name
            check_reply(o.host(), n, ns, cap, *self._reply_want(case, mask, keys))
            fs, sf, sp, _ = f.results()
            self._check_framing(dict(fs=fs, sf=sf, spans=sp), want, m, case, n, name)

    def test_bad_spans_above_the_mark(self, codec, wire):
        """Spans refused above 2^32 (WSG_EINVAL), the other streams exact: one
        that runs a byte past wire_len, one with off = 2^64 - 8 and len = 16
        (off + len wraps), one that starts a byte before the end of the span
        in front of it, which lies above 2^32."""
        case = bc.sparse_cases()["hdr14_s7"]
        put(wire, case.data, case.spans)
        want = case.want_frames()
        ns = case.n_streams
        assert int(case.spans["off"][ns - 2]) + int(case.spans["len"][ns - 2]) > MARK32   # the span in front of the last
        past = case.spans.copy()
        past["len"][ns - 1] = bc.SPARSE_WIRE - int(past["off"][ns - 1]) + 1
        wraps = np.concatenate([case.spans, np.zeros(1, dtype=STREAM_SPAN)])
        wraps["off"][ns], wraps["len"][ns] = 2**64 - 8, 16
        overlap = case.spans.copy()
        overlap["off"][ns - 1] = int(case.spans["off"][ns - 2]) + int(case.spans["len"][ns - 2]) - 1
        for spans, bad in ((past, ns - 1), (wraps, ns), (overlap, ns - 1)):
            assert list(np.nonzero(layout.bad_spans(bc.SPARSE_WIRE, spans))[0]) == [bad]
            w = want
            if len(spans) > ns:   # one more stream behind the others: no frames of its own
                w = (want[0], np.concatenate([want[1], want[1][-1:]]),
                     np.concatenate([want[2], np.zeros(1, dtype=STREAM_SPAN)]), want[3])
            w = refused(w, spans, [bad])
            assert int(w[3][0]) >= int(want[3][0]) - 5 and int(w[3][0]) > 10
            o = FrameOut(spans, int(w[3][0]))
            frame(codec, wire, o)
            assert codec.sync_status() == ca.WSG_EINVAL and codec.sync_status() == 0
            o.check(w, spans)

    def test_checked_launch_above_the_mark(self):
        """$WSG_CHECK=1 on a context of its own: a call whose wire is an exact
        device allocation of 2^32 + 4096 bytes, with a stream straddling 2^32,
        is accepted and gives the same frames; a wire_len one byte past the
        allocation is WSG_EINVAL and nothing is launched.  (An exact block:
        torch's allocator hands out views of larger segments.)"""
        os.environ["WSG_CHECK"] = "1"
        try:
            c = ca.Codec(0)
        finally:
            del os.environ["WSG_CHECK"]
        hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
        vp = ctypes.c_void_p
        size = MARK32 + 4096
        block = vp()
        assert hip.hipMalloc(ctypes.byref(block), ctypes.c_size_t(size)) == 0
        try:
            assert hip.hipMemset(block, SENTINEL, ctypes.c_size_t(size)) == 0
            full = bc.sparse_cases()["hdr8_s3"]
            keep = [j for j in range(full.n_streams) if int(full.spans["off"][j]) + int(full.spans["len"][j]) <= size]
            case = bc.Sparse([(full.frames[j], full.tails[j]) for j in keep], [int(full.spans["off"][j]) for j in keep])
            assert case.end > MARK32 and len(keep) == full.n_streams - 1
            for d, s in zip(case.data, case.spans):
                host = np.frombuffer(d, dtype=np.uint8).copy()
                assert hip.hipMemcpy(vp(block.value + int(s["off"])), vp(host.ctypes.data), ctypes.c_size_t(len(d)),
                                     1) == 0   # host to device
            want = case.want_frames()
            o = FrameOut(case.spans, int(want[3][0]))

            def call(wire_len):
                return ca.lib().wsg_frame_streams(c._ctx, block, wire_len, vp(o.spans.data_ptr()), case.n_streams,
                                                  vp(o.fs.data_ptr()), o.cap, vp(o.sf.data_ptr()),
                                                  vp(o.count.data_ptr()), c._stream(None))

            assert call(size + 1) == ca.WSG_EINVAL
            assert c.sync_status() == 0
            assert int(o.count.cpu()[0]) == -1 and (o.sfb.cpu().numpy() == SENTINEL).all(), "launched despite WSG_EINVAL"
            assert call(size) == 0
            assert c.sync_status() == 0
            o.check(want, case.spans)
        finally:
            c.close()
            hip.hipFree(block)


# =============================================================================
# 2. Outputs above 2^32: a dense d_msg and d_reply past the mark
# =============================================================================
class Dense:
    """One run of section 2: the filler frame's header and the small streams
    written into the random wire, and what the models say of the small
    streams alone."""

    def __init__(self, wire, name):
        streams, target = bc.dense_runs()[name]
        self.rest = mc.Batch(streams)
        self.L0 = MARK32 - target                 # dense offset 2^32 is offset `target` of the small streams' bytes
        self.msgs, self.count, self.state, self.buf, _, self.info = mc.check_model(self.rest)
        self.hdr = ca.header_pack(0x82, True, self.L0, 0, bc.FILLER_KEY)
        assert len(self.hdr) == 14
        self.at = 14 + self.L0                    # where the small streams begin in the wire
        self.used = self.at + len(self.rest.wire)
        assert self.used <= wire.numel()
        wire[:14].copy_(torch.from_numpy(np.frombuffer(self.hdr, dtype=np.uint8).copy()))
        wire[self.at: self.used].copy_(torch.from_numpy(self.rest.wire))
        self.wire = wire[: self.used]
        self.n, self.ns = self.rest.n + 1, self.rest.n_streams + 1
        self.d_fs = dev(np.concatenate([[0], self.rest.fs + np.uint64(self.at)]).astype(np.uint64).view(np.int64))
        self.d_sf = dev(np.concatenate([[0], self.rest.stream_first + 1]).astype(np.int32))
        self.want_msgs, self.want_count, self.want_state = bc.prepend_filler(self.msgs, self.count, self.L0, self.state)
        assert int(self.want_count[1]) > MARK32
        moved = bc.batch_spans(self.rest)
        moved["off"] += np.uint64(self.at)
        self.want_info = bc.shift_info(self.info, self.rest.stream_first, bc.batch_spans(self.rest), moved)

    def filler_equals(self, got, key):
        """got[0, L0) == the filler's wire bytes XOR key, in 1 GiB chunks."""
        for a in range(0, self.L0, GIB):
            b = min(a + GIB, self.L0)
            if not torch.equal(got[a:b], _xor_key_chunks(self.wire[14 + a: 14 + b], key, a)):
                return False
        return True

    def check_tables(self, msgs, count, state, info):
        """d_msgs, d_count[0..2), d_state against prepend_filler; d_info[0] by
        construction, the rest against shift_info."""
        got = msgs.cpu().numpy()
        nm = int(self.want_count[0])
        assert [int(x) for x in count.cpu().numpy().view(np.uint64)[:2]] == [int(x) for x in self.want_count]
        mc.same_fields(got[: nm * MSG.itemsize].view(MSG), self.want_msgs, mc.MSG_FIELDS)
        assert (got[nm * MSG.itemsize:] == SENTINEL).all()
        st = state.cpu().numpy()
        mc.same_fields(st[: self.ns * STREAM_STATE.itemsize].view(STREAM_STATE), self.want_state, ["consumed", "opcode"])
        assert (st[self.ns * STREAM_STATE.itemsize:] == SENTINEL).all()
        inf = info.cpu().numpy()
        r = inf[: self.n * RECV_INFO.itemsize].view(RECV_INFO)
        assert (inf[self.n * RECV_INFO.itemsize:] == SENTINEL).all()
        assert (int(r["payload_off"][0]), int(r["len"][0]), int(r["key"][0]), int(r["opcode"][0]), int(r["fin"][0]),
                int(r["masked"][0]), int(r["hdr_len"][0]), int(r["b0"][0]), int(r["error"][0])) \
            == (14, self.L0, bc.FILLER_KEY, 2, 1, 1, 14, 0x82, 0)
        mc.same_fields(r[1:], self.want_info, mc.INFO_FIELDS)

    def tables(self):
        """Sentinel-filled d_msgs, d_state (opcode seeds 0) and d_info with PAD bytes behind."""
        st = np.full(self.ns * STREAM_STATE.itemsize + PAD, SENTINEL, dtype=np.uint8)
        st[: self.ns * STREAM_STATE.itemsize].view(STREAM_STATE)["opcode"] = 0
        return sent(self.n * MSG.itemsize + PAD), dev(st), sent(self.n * RECV_INFO.itemsize + PAD)

    def decode(self, codec, msg_cap, room):
        """wsg_decode_messages into a sentinel d_msg of `room` bytes."""
        msgs, state, info = self.tables()
        msg = sent(room)
        count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        codec.decode_messages(self.wire, self.d_fs, self.d_sf, state=state[: self.ns * STREAM_STATE.itemsize], msg=msg,
                              msg_cap=msg_cap, msgs=msgs, count=count, info=info)
        return msg, msgs, count, state, info

    def reply(self, codec, rule, reply_cap, room, keys):
        msgs, state, info = self.tables()
        reply = sent(room)
        reply_off = sent((self.n + 1) * 8 + PAD).view(torch.int64)
        stream_reply = sent((self.ns + 1) * 8 + PAD).view(torch.int64)
        count = sent(4 * 8).view(torch.int64)
        codec.reply_messages(self.wire, self.d_fs, self.d_sf, reply_op=rule, mask=1, send_keys=d_keys_of(keys),
                             state=state[: self.ns * STREAM_STATE.itemsize], reply=reply, reply_cap=reply_cap,
                             reply_off=reply_off[: self.n + 1], stream_reply=stream_reply[: self.ns + 1], msgs=msgs,
                             count=count, info=info)
        return reply, reply_off, stream_reply, msgs, count, state, info

    def want_reply(self, rule, keys):
        """(reply_off, stream_reply, count) of the whole batch, and the reply
        frames of the small streams as one byte string."""
        plan = layout.reply_plan(self.msgs, rule, 1, keys[1:], n_streams=self.rest.n_streams)
        frames = rc.per_message(self.msgs, rc.oracle_replies(self.rest, rule, 1, keys[1:]))
        assert [len(f) for f in frames] == [int(x) for x in np.diff(plan[0].astype(np.int64))]
        return bc.prepend_filler_reply(plan, rule, 1, self.L0), np.frombuffer(b"".join(frames), dtype=np.uint8)


def sentinel_windows(buf):
    """The first and the last MiB of buf and the MiB around 2^32 (as far as buf reaches) hold the sentinel."""
    n = buf.numel()
    for a, b in ((0, MIB), (n - MIB, n), (MARK32 - MIB // 2, min(MARK32 + MIB // 2, n))):
        if not all_equal(buf[a:b], SENTINEL):
            return False
    return True


class TestDenseOutputs:
    @pytest.fixture(scope="class")
    def wire(self):
        """2^32 + 2^20 random bytes made on the device; the runs rewrite only
        the filler's 14-byte header and the small streams."""
        gen = torch.Generator(device="cuda").manual_seed(2032)
        w = torch.randint(0, 256, (bc.DENSE_WIRE,), dtype=torch.uint8, device="cuda", generator=gen)
        yield w
        del w
        torch.cuda.empty_cache()

    @pytest.mark.parametrize("name", ["text", "fragments", "close", "first_byte"])
    def test_decode_messages(self, codec, wire, name):
        """Dense offset 2^32 falls (text) at byte 5 of a 40-byte text message,
        (fragments) between fragments 2 and 3 of a 4-fragment message, (close)
        between the two status bytes of a close message in frames of 1 byte
        and the rest, (first_byte) at a message's first byte behind an empty
        message."""
        d = Dense(wire, name)
        used = int(d.want_count[1])
        msg, msgs, count, state, info = d.decode(codec, used + 1000, used + 1000 + PAD)
        assert codec.sync_status() == 0
        d.check_tables(msgs, count, state, info)
        assert d.filler_equals(msg, bc.FILLER_KEY), "the filler's bytes in d_msg"
        assert np.array_equal(msg[d.L0: used].cpu().numpy(), d.buf)
        assert all_equal(msg[used:], SENTINEL), "d_msg written past d_count[1]"
        del msg
        torch.cuda.empty_cache()

    @pytest.mark.parametrize("name,rule", [("text", "echo"), ("fragments", "echo"), ("close", "echo"),
                                           ("close", "same_close_pong"), ("first_byte", "echo")])
    def test_reply_messages(self, codec, wire, name, rule):
        """wsg_reply_messages, masked, a reply buffer of wire_len + 14 n
        bytes: the filler's reply is the packed header and its data XOR the
        send key; every other frame and both offset tables are the shifted
        layout.reply_plan's and the oracle's frames; d_count[2] > 2^32.  The
        echo rule answers a close with nothing, so the close run is made a
        second time under a rule that answers it with a close (built from the
        status alone), which then lies above the mark."""
        d = Dense(wire, name)
        rule = rc.RULES[rule]
        keys = send_keys(d.ns)
        (reply_off, stream_reply, rcount), small = d.want_reply(rule, keys)
        need = int(rcount[0])
        cap = d.used + 14 * d.n
        assert MARK32 < need <= cap
        reply, d_off, d_sr, msgs, count, state, info = d.reply(codec, rule, cap, cap + SLACK, keys)
        assert codec.sync_status() == 0
        d.check_tables(msgs, count, state, info)
        got = [int(x) for x in count.cpu().numpy().view(np.uint64)]
        assert got[2:] == [need, int(rcount[1])]
        nm = got[0]
        off = d_off.cpu().numpy().view(np.uint64)
        assert np.array_equal(off[: nm + 1], reply_off) and (off[nm + 1: d.n + 1 + PAD // 8] == SENT64).all()
        sr = d_sr.cpu().numpy().view(np.uint64)
        assert np.array_equal(sr[: d.ns + 1], stream_reply) and (sr[d.ns + 1:] == SENT64).all()
        hdr = ca.header_pack(0x82, True, d.L0, 0, int(keys[0]))
        assert bytes(reply[:14].cpu().numpy()) == hdr and int(reply_off[1]) == 14 + d.L0
        assert d.filler_equals(reply[14:], bc.FILLER_KEY ^ int(keys[0])), "the filler's reply"
        assert np.array_equal(reply[14 + d.L0: need].cpu().numpy(), small)
        assert all_equal(reply[need:], SENTINEL), "d_reply written past d_count[2]"
        if rule is rc.SAME_CLOSE_PONG:
            (q,) = [q for q, m in enumerate(d.want_msgs) if int(m["kind"]) == ca.CB_CLOSE and int(m["status"]) == 0x03E9]
            assert int(reply_off[q]) > MARK32 and int(reply_off[q + 1]) - int(reply_off[q]) == 8   # 2 + 4 + the status
        del reply
        torch.cuda.empty_cache()

    def test_capacity(self, codec, wire):
        """msg_cap and reply_cap one byte short, above 2^32: WSG_ENOMEM, not
        one byte of the output written (the first and last MiB and the MiB
        around 2^32 looked at), d_count holds the size needed."""
        d = Dense(wire, "text")
        used = int(d.want_count[1])
        msg, msgs, count, state, info = d.decode(codec, used - 1, used + PAD)
        assert codec.sync_status() == ca.WSG_ENOMEM and codec.sync_status() == 0
        assert sentinel_windows(msg), "d_msg written despite WSG_ENOMEM"
        assert [int(x) for x in count.cpu().numpy().view(np.uint64)] == [int(x) for x in d.want_count]
        del msg
        torch.cuda.empty_cache()
        keys = send_keys(d.ns)
        (_, _, rcount), _ = d.want_reply(rc.ECHO, keys)
        need = int(rcount[0])
        reply, _, _, _, count, _, _ = d.reply(codec, rc.ECHO, need - 1, need + SLACK, keys)
        assert codec.sync_status() == ca.WSG_ENOMEM and codec.sync_status() == 0
        assert sentinel_windows(reply), "d_reply written despite WSG_ENOMEM"
        assert [int(x) for x in count.cpu().numpy().view(np.uint64)] == [int(d.want_count[0]), used, need, int(rcount[1])]
        del reply
        torch.cuda.empty_cache()


# =============================================================================
# 3. wsg_check_utf8 above the marks
# =============================================================================
def text_record(off, size):
    r = np.zeros((), dtype=MSG)
    r["off"], r["len"], r["nframes"], r["kind"], r["opcode"] = off, size, 1, ca.CB_RECEIVED, 1
    return r


class TestUtf8AboveTheMarks:
    """Codec.check_utf8 on a hand-made table (it reads d_msgs and d_count from
    the device: no decode in front) over 2^32 + 2^20 NUL bytes, which are
    valid ASCII: the scan loads them once and goes on.

    The expected value of a small message is uc.want (Python's decoder) of
    its own bytes.  That of a record too large for the decoder follows from
    the prefix rule (tests/test_big_cases_model.py::test_utf8_prefix_rule): a
    valid prefix that ends on a code point boundary adds its length, so it is
    the length of the NUL prefix plus uc.want of the record's last 200 bytes."""

    SIZE = MARK32 + MIB
    BASE = bytes(range(0x30, 0x70))   # 64 ASCII bytes

    @pytest.fixture(scope="class")
    def msg(self):
        m = torch.zeros(self.SIZE, dtype=torch.uint8, device="cuda")
        yield m
        del m
        torch.cuda.empty_cache()

    def call(self, codec, msg, records, planted, want_valid, msg_cap=None):
        """One call over `records` (non-decreasing ends) with `planted`
        {offset: bytes} written into the zeros, and zeroed again afterwards."""
        table = np.array(records, dtype=MSG)
        ends = table["off"] + table["len"]
        assert (ends[:-1] <= ends[1:]).all()
        for off, data in planted.items():
            msg[off: off + len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        d_msgs = dev(table.view(np.uint8))
        d_count = dev(np.array([len(table), self.SIZE], dtype=np.uint64).view(np.int64))   # d_count[1]: the whole buffer
        cap = self.SIZE if msg_cap is None else msg_cap
        inside = [int(r["off"]) + int(r["len"]) <= cap for r in table]   # every record is a text message: checked if inside
        bad = [m for m, (v, r) in enumerate(zip(want_valid, table)) if v < int(r["len"])]
        want_result = [len(bad), bad[0] if bad else U64_MAX, sum(inside),
                       sum(int(r["len"]) for r, i in zip(table, inside) if i)]
        try:
            utf8_check(codec, msg, d_msgs, d_count, ca.UTF8_TEXT, cap, len(table), want_valid, want_result)
            assert codec.sync_status() == 0
        finally:
            for off, data in planted.items():
                msg[off: off + len(data)].zero_()

    def at_both_marks(self, codec, msg, text_of, pos_of):
        """One call with a message at each mark: text_of(mark) its bytes,
        pos_of(mark) the message offset that lies at the mark."""
        records, planted, want = [], {}, []
        for mark in MARKS:
            text = text_of(mark)
            off = mark - pos_of(mark)
            records.append(text_record(off, len(text)))
            planted[off] = text
            want.append(uc.want(text))
        self.call(codec, msg, records, planted, want)
        return want

    @pytest.mark.parametrize("seq", [uc.EURO, uc.GRIN], ids=["euro", "grin"])
    def test_sequences_split_by_the_marks(self, codec, msg, seq):
        """A 64-byte text message with the sequence at offset 30, every split
        of it across the mark: valid (expects 64), and with the first byte
        above the mark made 41 (expects 30, the lead byte below the mark)."""
        for below in range(1, len(seq)):                         # bytes of the sequence below the mark
            good = self.BASE[:30] + seq + self.BASE[30 + len(seq):]
            bad = bytearray(good)
            bad[30 + below] = 0x41
            assert self.at_both_marks(codec, msg, lambda mark: good, lambda mark: 30 + below) == [64, 64]
            assert self.at_both_marks(codec, msg, lambda mark: bytes(bad), lambda mark: 30 + below) == [30, 30]

    def test_messages_that_begin_and_end_at_the_marks(self, codec, msg):
        """A message that begins exactly at a mark with a continuation byte
        (expects 0); messages that end exactly at a mark on a sequence the
        end cuts off (expects len - cut)."""
        stray = b"\x80" + self.BASE[1:]
        assert self.at_both_marks(codec, msg, lambda mark: stray, lambda mark: 0) == [0, 0]
        for seq in (uc.EURO, uc.GRIN):
            for cut in range(1, len(seq)):
                text = self.BASE[: 64 - cut] + seq[:cut]
                assert self.at_both_marks(codec, msg, lambda mark: text, lambda mark: 64) == [64 - cut, 64 - cut]

    def test_one_record_longer_than_4gib(self, codec, msg):
        """One text record [0, 2^32 + 100) over the zeros: valid whole; with
        FF at 2^32 + 5, d_valid[0] = 2^32 + 5 (more than 32 bits) and d_result
        = [1, 0, 1, 2^32 + 100]."""
        size = MARK32 + 100
        tail = bytearray(200)
        assert bc.want_behind_prefix(size - 200, bytes(tail)) == size
        self.call(codec, msg, [text_record(0, size)], {}, [size])
        tail[105] = 0xFF                                        # the record's last 200 bytes begin at 2^32 - 100
        want = bc.want_behind_prefix(size - 200, bytes(tail))
        assert want == MARK32 + 5
        self.call(codec, msg, [text_record(0, size)], {MARK32 + 5: b"\xff"}, [want])

    def test_msg_cap_above_the_mark(self, codec, msg):
        """msg_cap = 2^32 + 50 below d_count[1]: the record longer than 4 GiB
        ends past it and is not checked (d_valid[0] = len, nothing checked,
        the FF inside it never judged); a small record that ends exactly at
        2^32 + 50 is checked, and is not with a msg_cap one byte lower."""
        cap = MARK32 + 50
        size = MARK32 + 100
        self.call(codec, msg, [text_record(0, size)], {MARK32 + 5: b"\xff"}, [size], msg_cap=cap)
        small = self.BASE[:10] + b"\x80" + self.BASE[11:]
        assert uc.want(small) == 10
        records = [text_record(0, cap - 64), text_record(cap - 64, 64)]   # (back to back, as the decode lays them)
        self.call(codec, msg, records, {cap - 64: small}, [cap - 64, 10], msg_cap=cap)
        self.call(codec, msg, records, {cap - 64: small}, [cap - 64, 64], msg_cap=cap - 1)


# =============================================================================
# 4. Fan-out above 4 GiB
# =============================================================================
def fan_keys(k, seed):
    return np.random.default_rng(seed).integers(0, 2**32, k, dtype=np.uint64).astype(np.uint32)


def check_fanout(wire, base, payload, d_payload, keys, d_keys, opcode, mask, seed):
    """The k frames at wire[base, base + k * fsize): every frame's header
    columns against ca.header_pack of its key and its payload columns against
    payload ^ key bytes, as (rows, fsize) slabs of at most 1 GiB on the device;
    the frame holding wire byte 2^32, its 20 neighbours on either side and 200
    sampled frames byte for byte against the oracle."""
    k, n = len(keys), len(payload)
    fsize = frame_size(opcode, mask, n)
    hdr = fsize - n
    fixed = hdr - (4 if mask else 0)                       # header bytes in front of the key
    head = np.frombuffer(ca.header_pack(opcode, mask, n, 0, 0)[:fixed], dtype=np.uint8).copy()
    for key in (int(keys[0]), int(keys[-1])):              # the header is those bytes and then the key, little-endian
        assert ca.header_pack(opcode, mask, n, 0, key) == head.tobytes() + (key.to_bytes(4, "little") if mask else b"")
    d_head = dev(head)
    kb = d_keys.view(torch.uint8).view(-1, 4)              # (k, 4): key byte j = (key >> 8j) & 0xFF
    rows = max(1, GIB // fsize)
    reps = (n + 3) // 4
    for a in range(0, k, rows):
        b = min(a + rows, k)
        slab = wire[base + a * fsize: base + b * fsize].view(b - a, fsize)
        assert bool((slab[:, :fixed] == d_head).all().item()), "header of a frame in [%d, %d)" % (a, b)
        if mask:
            assert torch.equal(slab[:, fixed:hdr], kb[a:b]), "key of a frame in [%d, %d)" % (a, b)
            got = slab[:, hdr:] ^ d_payload
            assert torch.equal(got, kb[a:b].repeat(1, reps)[:, :n]), "payload of a frame in [%d, %d)" % (a, b)
            del got
        else:
            assert bool((slab[:, hdr:] == d_payload).all().item()), "payload of a frame in [%d, %d)" % (a, b)
    j = (MARK32 - base) // fsize                            # the frame holding wire byte 2^32
    rng = np.random.default_rng(seed)
    pick = set(rng.integers(0, k, 200).tolist()) | {0, k - 1}
    if 0 <= j < k:
        pick |= set(range(max(0, j - 20), min(k, j + 21)))
    pick = np.array(sorted(pick))
    ref = oracle.fanout_encode(payload, keys[pick], opcode, mask).reshape(len(pick), fsize)
    d_ref = dev(ref)
    for i, f in enumerate(pick.tolist()):
        assert torch.equal(wire[base + f * fsize: base + (f + 1) * fsize], d_ref[i]), "frame %d" % f


def test_fanout_period_kernel_over_4gib(codec):
    """74 000 masked frames of 65 528 payload bytes: fsize = 65 536 is a
    multiple of 16, so launch_fanout_period takes the batch (P = 1, G = 4096
    chunks, within [64, 2^20]; W = 64 * mult waves with mult from the third
    clause, some 74 000 < 2^22) and the period kernel writes 4.5 GiB."""
    n, k = 65528, 74000
    fsize = frame_size(0x82, True, n)
    assert fsize == 65536 and fsize % 16 == 0 and 64 <= fsize // 16 <= 1 << 20
    total = fsize * k
    assert total > MARK32 + (1 << 28)
    payload = np.random.default_rng(401).integers(0, 256, n, dtype=np.uint8)
    keys = fan_keys(k, 402)
    d_payload, d_keys = dev(payload), dev(keys.view(np.int32))
    wire = sent(total + 48)
    codec.fanout(d_payload, d_keys, 0x82, True, wire=wire)
    assert codec.sync_status() == 0
    assert all_equal(wire[total:], SENTINEL), "written behind the last frame"
    check_fanout(wire, 0, payload, d_payload, keys, d_keys, 0x82, True, 403)
    del wire
    torch.cuda.empty_cache()


def test_fanout_flat_kernel_over_4gib(codec):
    """4 700 000 masked frames of 1 021 payload bytes: fsize = 1 029 is no
    multiple of 4, which launch_fanout_period refuses, so k_fanout_flat runs
    (streaming waves and edge items) over 4.5 GiB."""
    n, k = 1021, 4_700_000
    fsize = frame_size(0x81, True, n)
    assert fsize == 1029 and fsize % 4 != 0
    total = fsize * k
    assert total > MARK32 + (1 << 28)
    payload = np.random.default_rng(411).integers(0, 256, n, dtype=np.uint8)
    keys = fan_keys(k, 412)
    d_payload, d_keys = dev(payload), dev(keys.view(np.int32))
    wire = sent(total + 48)
    codec.fanout(d_payload, d_keys, 0x81, True, wire=wire)
    assert codec.sync_status() == 0
    assert all_equal(wire[total:], SENTINEL), "written behind the last frame"
    check_fanout(wire, 0, payload, d_payload, keys, d_keys, 0x81, True, 413)
    del wire
    torch.cuda.empty_cache()


def test_fanout_many_over_4gib(codec):
    """wsg_fanout_encode_many, two messages of different geometry and the
    same 74 001 keys: the first (65 524 payload bytes: fsize = 65 532, a
    multiple of 4 and not of 16, the period kernel with P = 4) occupies more
    than 2^32 bytes, so wire_off[1] lies above the mark; the second (1 021
    bytes: fsize = 1 029, the flat kernel) is written there.  The gap up to
    the 128-byte line and the bytes behind the last frame keep the sentinel."""
    k = 74001
    lens = np.array([65524, 1021], dtype=np.uint64)
    ops = np.array([0x82, 0x81], dtype=np.uint8)
    sizes = [frame_size(int(o), True, int(n)) for o, n in zip(ops, lens)]
    assert sizes == [65532, 1029] and sizes[0] % 4 == 0 and sizes[0] % 16 != 0 and sizes[1] % 4 != 0
    src = np.array([3, 3 + 65524 + 5], dtype=np.uint64)
    payload = np.random.default_rng(421).integers(0, 256, int(src[1] + lens[1]) + 16, dtype=np.uint8)
    keys = fan_keys(k, 422)
    d_payload, d_keys = dev(payload), dev(keys.view(np.int32))
    end0 = sizes[0] * k
    off1 = (end0 + 127) // 128 * 128
    end1 = off1 + sizes[1] * k
    assert end0 > MARK32 and off1 > end0
    wire = sent(end1 + 48)
    _, off = codec.fanout_many(d_payload, src, lens, ops, d_keys, True, wire=wire)
    assert codec.sync_status() == 0
    assert [int(x) for x in off] == [0, off1, end1]
    assert all_equal(wire[end0:off1], SENTINEL), "the gap between the messages"
    assert all_equal(wire[end1:], SENTINEL), "written behind the last frame"
    for i in (0, 1):
        p = payload[int(src[i]): int(src[i] + lens[i])]
        check_fanout(wire, int(off[i]), p, dev(p), keys, d_keys, int(ops[i]), True, 423 + i)
    del wire
    torch.cuda.empty_cache()
