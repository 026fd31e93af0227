"""The conformant echo server's loop on the GPU under WSG_ASSEMBLY_RFC: one
wsg_reply_validated_streams and one wsg_sync per round of cut reads.

tests/rfc_assembly_cases.py's driver delivers the 200 connections of
tests/golden/rfc6455_messages.json (two in five with control frames between
fragments) in reads of 0 to 700 bytes, carries the bytes from off + consumed,
d_state[j].ahead and d_proto[j], and drops a connection once its d_close_off
is set.  Each connection's output must be the one call's over the whole
connection, whatever the schedule; what the one call delivers is held against
the recorded outside reader by tests/test_rfc_assembly_model.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import PROTO_VERDICT, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests import test_gpu_validated_reply as vg  # noqa: E402

SENTINEL, SENT64, EXTRA = cg.SENTINEL, cg.SENT64, cg.EXTRA
dev, sent = cg.dev, cg.sent


def device_step(codec, rule, mask):
    def step(wire, spans, ahead, proto, keys, frame_cap):
        ns = len(spans)
        o = vg.Out(frame_cap, ns, len(wire) + 14 * frame_cap, None, proto)
        st = np.zeros(max(ns, 1), dtype=STREAM_STATE)
        st["ahead"][:ns] = ahead
        o.state = dev(st.view(np.uint8))
        d_spans = dev(spans.view(np.uint8))
        fs = sent((frame_cap + EXTRA) * 8).view(torch.int64)
        sf = sent((ns + 1 + EXTRA) * 4).view(torch.int32)
        out = codec.reply_validated_streams(
            dev(wire), d_spans, proto=o.proto, role=pc.SERVER, max_message=0, which=ac.WHICH, reply_op=rule, mask=mask,
            send_keys=cg.d_keys_of(keys), state=o.state, frame_start=fs, frame_cap=frame_cap, stream_first=sf,
            reply=o.reply, reply_cap=o.cap, reply_off=o.reply_off, stream_reply=o.stream_reply, close_off=o.close_off,
            verdict=o.verdict, result=o.result, valid=o.valid, utf8_result=o.utf8_result, msgs=o.msgs, count=o.count,
            info=o.info)
        assert codec.sync_status() == 0
        n = out[-1]
        o.n = n
        h = o.host()
        nm, need = int(h["count"][0]), int(h["count"][2])
        assert need <= o.cap and (h["reply"][need:] == SENTINEL).all() and (h["count"][5:] == SENT64).all()
        assert (h["reply_off"][nm + 1:] == SENT64).all() and (h["stream_reply"][ns + 1:] == SENT64).all()
        assert (h["msgs"][nm:].view(np.uint8) == SENTINEL).all()
        assert (fs.cpu().numpy().view(np.uint64)[n:] == SENT64).all()
        r = ac.sl.Step()
        r.reply, r.stream_reply, r.close_off = h["reply"][:need], h["stream_reply"], h["close_off"]
        r.verdict = cc.verdict_tuples(h["verdict"][:ns].view(PROTO_VERDICT))
        r.stream_first = sf.cpu().numpy().view(np.uint32)[: ns + 1]
        r.frames_consumed, r.ahead = h["state"]["consumed"], h["state"]["ahead"]
        assert not h["state"]["opcode"].any() and not h["state"]["_pad"].any()
        r.bytes_consumed = [int(x) for x in d_spans.cpu().numpy().view(STREAM_SPAN)["consumed"]]
        r.proto = [(int(p["bytes"]), int(p["open"])) for p in h["proto"][:ns]]
        return r
    return step


@pytest.mark.parametrize("rule,mask", [(rc.SAME_CLOSE_PONG, 0), (rc.ECHO, 1)])
def test_loop(rule, mask):
    codec = ca.Codec(0)
    try:
        codec.set_assembly(ac.RFC)
        keys = ac.send_keys() if mask else None
        runs = [ac.drive(device_step(codec, rule, mask), seed, keys) for seed in (0, 1)]
        for seed, run in enumerate(runs):
            ac.check_run(run, True, rule, mask, "schedule %d" % seed)
        assert runs[0].out == runs[1].out and runs[0].verdict == runs[1].verdict
        assert all(r.carried_ahead > 0 and r.max_streams == ac.N_CONNECTIONS for r in runs)
    finally:
        codec.close()
