"""The checked echo server's loop on the GPU, over many rounds of cut reads.

tests/server_loop_cases.py's driver delivers 264 connections in reads of 0, 1,
2, 3, up to 700 bytes or everything, lays each round's pending bytes (the
carry and the new read) in one wire, makes one call, appends every
d_stream_reply range to its connection's output, carries the bytes from off +
consumed, d_state[j].opcode and d_proto[j], and drops a connection for good
once its d_close_off is set.  Two forms of the round: wsg_reply_checked_streams
alone, and the validating chain wsg_frame_streams -> wsg_decode_messages ->
wsg_check_utf8 -> wsg_utf8_verdicts -> wsg_reply_checked(d_also) on one stream
with the frame count as its only host wait.

Each connection's output must be what checked_reply_cases.expected builds for
the whole connection in one call, whatever the schedule; its verdict must be
the one an outside RFC 6455 reader recorded in tests/golden/rfc6455.json
(inside the agreement domain described there); it holds one close frame, the
last, exactly when there is a verdict; and every output of every round keeps
its sentinel past what the call may write.  tests/test_rfc6455_model.py runs
the same driver and checks with a numpy step."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import PROTO_VERDICT, RECV_INFO, STREAM_SPAN  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests.test_gpu_protocol import BLOCK  # noqa: E402
from tests.test_rfc6455_model import CONFIGS, check_schedules  # noqa: E402

SENTINEL, SENT64, EXTRA = cg.SENTINEL, cg.SENT64, cg.EXTRA
dev, sent = cg.dev, cg.sent
SCHEDULES = (0, 1, 2)


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


class Round:
    """The device side of one round: cg.Out's sentinel-filled outputs with
    room for frame_cap frames, the spans and the frame table."""

    def __init__(self, wire, spans, opcodes, proto, keys, frame_cap):
        self.ns, self.fcap = len(spans), frame_cap
        self.cap = len(wire) + 14 * frame_cap
        self.o = cg.Out(frame_cap, self.ns, self.cap, opcodes, proto)
        self.wire = dev(wire)
        self.spans_in = spans
        self.spans = dev(spans.view(np.uint8))
        self.fs = sent((frame_cap + EXTRA) * 8).view(torch.int64)
        self.sf = sent((self.ns + 1 + EXTRA) * 4).view(torch.int32)
        self.keys = cg.d_keys_of(keys)

    def finish(self, n, lowered_on_device):
        """Every tail still the sentinel; the round as a server_loop_cases.Step."""
        o, ns = self.o, self.ns
        assert n <= self.fcap
        o.n = n
        h = o.host()
        nm, need, nclose = int(h["count"][0]), int(h["count"][2]), int(h["count"][4])
        assert need <= self.cap
        assert (h["reply"][need:] == SENTINEL).all()
        assert (h["count"][5:] == SENT64).all() and (h["result"][3:] == SENT64).all()
        assert (h["reply_off"][nm + 1:] == SENT64).all()
        assert (h["stream_reply"][ns + 1:] == SENT64).all() and int(h["stream_reply"][ns]) == need
        assert (h["close_off"][ns:] == SENT64).all() and (h["verdict"][ns:] == SENT64).all()
        assert (h["proto"][max(ns, 1):].view(np.uint8) == SENTINEL).all() and (h["proto"]["_pad"][:ns] == 0).all()
        assert (h["msgs"][nm:].view(np.uint8) == SENTINEL).all()
        assert (o.info.cpu().numpy()[n * RECV_INFO.itemsize:] == SENTINEL).all()
        fs = self.fs.cpu().numpy().view(np.uint64)
        sf = self.sf.cpu().numpy().view(np.uint32)
        assert (fs[n:] == SENT64).all() and (sf[ns + 1:] == 0xA5A5A5A5).all() and int(sf[ns]) == n
        spans = self.spans.cpu().numpy().view(STREAM_SPAN)
        assert np.array_equal(spans["off"], self.spans_in["off"]) and np.array_equal(spans["len"], self.spans_in["len"])
        r = sl.Step()
        r.reply, r.stream_reply, r.close_off = h["reply"][:need], h["stream_reply"], h["close_off"]
        r.verdict = cc.verdict_tuples(h["verdict"][:ns].view(PROTO_VERDICT))
        assert sum(1 for v in r.verdict if v != sl.NONE) == nclose
        assert [int(x) for x in h["result"][:3]] == [sum(1 for v in r.verdict if v != sl.NONE and v[0] >= 2),
                                                      min([j for j, v in enumerate(r.verdict)
                                                           if v != sl.NONE and v[0] >= 2], default=sl.U64_MAX),
                                                      sum(1 for v in r.verdict if v[0] == 1)]
        r.stream_first, r.frames_consumed, r.opcode = sf[: ns + 1], h["state"]["consumed"], h["state"]["opcode"]
        r.bytes_consumed = [int(x) for x in spans["consumed"]] if lowered_on_device else \
            sl.lowered(fs, sf, spans["off"], spans["consumed"], r.frames_consumed)
        r.proto = [(int(p["bytes"]), int(p["open"])) for p in h["proto"][:ns]]
        return r


def plain_step(codec, rule, mask, limit):
    """One wsg_reply_checked_streams and one wsg_sync."""
    def step(wire, spans, opcodes, proto, keys, frame_cap):
        rd = Round(wire, spans, opcodes, proto, keys, frame_cap)
        o = rd.o
        out = codec.reply_checked_streams(rd.wire, rd.spans, proto=o.proto, role=pc.SERVER, max_message=limit,
                                          reply_op=rule, mask=mask, send_keys=rd.keys, state=o.state,
                                          frame_start=rd.fs, frame_cap=frame_cap, stream_first=rd.sf, reply=o.reply,
                                          reply_cap=rd.cap, reply_off=o.reply_off, stream_reply=o.stream_reply,
                                          close_off=o.close_off, verdict=o.verdict, result=o.result, msgs=o.msgs,
                                          count=o.count, info=o.info)
        assert codec.sync_status() == 0
        return rd.finish(out[-1], lowered_on_device=True)
    return step


def validating_step(codec, rule, mask, limit):
    """The validating chain on one stream; the frame count is its only host
    wait.  wsg_decode_messages works on a copy of the state: the reply call
    takes the incoming one."""
    def step(wire, spans, opcodes, proto, keys, frame_cap):
        rd = Round(wire, spans, opcodes, proto, keys, frame_cap)
        o, ns = rd.o, rd.ns
        count = sent((2 + EXTRA) * 8).view(torch.int64)
        codec.frame_streams(rd.wire, rd.spans, frame_start=rd.fs, frame_cap=frame_cap, stream_first=rd.sf, count=count)
        n = int(count[0].item())
        fs, sf = rd.fs[:n], rd.sf[: ns + 1]
        msg, msgs, mcount, _, _ = codec.decode_messages(rd.wire, fs, sf, state=o.state.clone())
        valid, _ = codec.check_utf8(msg, msgs, mcount, sl.WHICH)
        also = sent((ns + EXTRA) * PROTO_VERDICT.itemsize)
        codec.utf8_verdicts(msgs, mcount, valid, ns, sl.WHICH, also=also)
        o.launch(codec, rd.wire, fs, sf, rule, mask, rd.keys, pc.SERVER, limit, also)
        assert codec.sync_status() == 0
        assert (count.cpu().numpy().view(np.uint64)[2:] == SENT64).all()
        assert (also.cpu().numpy().view(np.uint64)[ns:] == SENT64).all()
        return rd.finish(n, lowered_on_device=False)
    return step


@pytest.mark.parametrize("limit,validating,rule,mask", CONFIGS)
def test_loop(codec, limit, validating, rule, mask):
    """Three schedules of cut reads: every connection's output is the one
    call's over the whole connection, its verdict the recorded reader's, and
    the three runs are identical."""
    keys = sl.send_keys() if mask else None
    step = (validating_step if validating else plain_step)(codec, rule, mask, limit)
    runs = [sl.drive(step, seed, keys) for seed in SCHEDULES]
    for seed, run in zip(SCHEDULES, runs):
        sl.check_run(run, limit, validating, rule, mask, "schedule %d" % seed)
    for run in runs[1:]:
        assert run.out == runs[0].out and run.verdict == runs[0].verdict
    check_schedules(runs)
    assert all(r.max_streams > BLOCK and r.max_frames > BLOCK for r in runs)
    closed = sum(1 for v in runs[0].verdict if v != sl.NONE)
    print("connections with a verdict:", closed, "of", len(runs[0].verdict),
          "by UTF-8:", sum(1 for v in runs[0].verdict if v[0] == layout.PV_UTF8))
    assert closed >= 50 and (not validating or any(v[0] == layout.PV_UTF8 for v in runs[0].verdict))
