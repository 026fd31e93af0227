"""The chat server's loop with the wire resident on the device.

tests/test_gpu_carry_loop.py's loop with wsg_relay_validated_streams in the
place of wsg_reply_validated_streams: server_loop_cases.connections() (264
connections, violators included) are a server's clients in 5 rooms, one of
them empty, in a random d_order; a round is one upload of the bytes just read,
one wsg_carry_streams, one wsg_relay_validated_streams and one wsg_sync.  Under
WSG_ASSEMBLY_RFC the connections are tests/rfc_assembly_cases.py's.

Per connection, the relay frames attributed to it through d_relay_off and
d_msgs[].stream, joined over all rounds, equal those of one call over the
whole connections; every round's d_relay equals the model driver's on the same
schedule (tests/test_relay_model.py); every group range is the concatenation of
its members' frames in order; the reply side passes the cases' check_run (see
test_relay_model.check_reply_side for what that judges under the chat rule)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_VERDICT, STREAM_STATE  # noqa: E402
from tests import carry_cases as kc  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import relay_cases as rl  # noqa: E402
from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import server_loop_cases as sl  # noqa: E402
from tests import test_gpu_carry_loop as kl  # noqa: E402
from tests import test_gpu_relay as gr  # noqa: E402
from tests import test_relay_model as rm  # noqa: E402
from tests.test_gpu_server_loop import SCHEDULES  # noqa: E402

SENTINEL, SENT64, EXTRA = gr.SENTINEL, gr.SENT64, gr.EXTRA
dev, sent = gr.dev, gr.sent
ROOM = kl.ROOM


class ChatResident(kl.Resident):
    """kl.Resident whose round is wsg_relay_validated_streams; every round's
    relay side, read back from the device, is appended to ``log``."""

    def __init__(self, codec, n, frame_cap, limit, rooms, carries):
        super().__init__(codec, n, frame_cap, rl.CHAT_REPLY, 0, limit, rl.WHICH, None, carries)
        self.rooms, self.log = rooms, []
        self.order, self.gf, self.ng = gr.d_rooms(rooms)

    def step(self, wire, spans, state, proto, keys, frame_cap):
        n, cap = self.n, ROOM + 14 * self.frame_cap
        o = gr.Out(self.frame_cap, n, cap, cap, self.ng)
        fs = sent((self.frame_cap + EXTRA) * 8).view(torch.int64)
        sf = sent((n + 1 + EXTRA) * 4).view(torch.int32)
        out = self.codec.relay_validated_streams(
            wire, spans, proto=self.proto, role=pc.SERVER, max_message=self.limit, which=self.which, reply_op=self.rule,
            mask=0, send_keys=None, relay_op=rl.CHAT_RELAY, order=self.order, group_first=self.gf, state=self.state,
            frame_start=fs, frame_cap=self.frame_cap, stream_first=sf, reply=o.reply, reply_cap=cap, relay=o.relay,
            relay_cap=cap, reply_off=o.reply_off, stream_reply=o.stream_reply, close_off=o.close_off,
            relay_off=o.relay_off, group_relay=o.group_relay, verdict=o.verdict, result=o.result, valid=o.valid,
            utf8_result=o.utf8_result, msgs=o.msgs, count=o.count, info=o.info)
        assert self.codec.sync_status() == 0
        cnt = self.count.cpu().numpy().view(np.uint64)
        self.wire_bytes += int(cnt[0])
        self.carried += int(cnt[1])
        rcount = o.count.cpu().numpy().view(np.uint64)
        assert (rcount[8:] == SENT64).all() and int(rcount[7]) == 0
        nm, need, rneed = int(rcount[0]), int(rcount[2]), int(rcount[5])
        reply, relay = o.reply.cpu().numpy(), o.relay.cpu().numpy()
        assert out[-1] <= self.frame_cap and need <= cap and (reply[need:] == SENTINEL).all()
        assert rneed <= cap and (relay[rneed:] == SENTINEL).all()
        r = sl.Step()
        r.reply, r.stream_reply = reply[:need], o.stream_reply.cpu().numpy().view(np.uint64)
        r.close_off = o.close_off.cpu().numpy().view(np.uint64)
        r.verdict = cc.verdict_tuples(o.verdict.cpu().numpy().view(np.uint64)[:n].view(PROTO_VERDICT))
        r.stream_first = sf.cpu().numpy().view(np.uint32)[: n + 1]
        r.frames_consumed = self.state.cpu().numpy().view(STREAM_STATE)["consumed"]
        r.proto = None
        setattr(r, self.carries, None)
        r.spans_left, r.close_left = spans, o.close_off
        # the relay side as the device left it: frames attributed through d_relay_off and d_msgs[].stream
        msgs = o.msgs.cpu().numpy().view(MSG)[:nm]
        off = o.relay_off.cpu().numpy().view(np.uint64)
        assert (off[nm:] == SENT64).all()
        d = rl.Relay()
        d.relay, d.relay_off = relay[:rneed].tobytes(), [int(x) for x in off[:nm]]
        d.group_relay = [int(x) for x in o.group_relay.cpu().numpy().view(np.uint64)[: self.ng + 1]]
        d.count = [int(x) for x in rcount[5:8]]
        d.by_stream, d.frame_of = [[] for _ in range(n)], {}
        for q in range(nm):
            if d.relay_off[q] != rl.U64_MAX:
                at = d.relay_off[q]
                rc_, rec = ca.header_unpack(d.relay[at: at + 14])
                assert rc_ == 0 and not int(rec["masked"])
                d.frame_of[q] = d.relay[at: at + int(rec["hdr_len"]) + int(rec["len"])]
                d.by_stream[int(msgs["stream"][q])].append(d.frame_of[q])
        d.merged = rl.merged_out(msgs, r.verdict, rl.CHAT_REPLY, r.reply, r.stream_reply, d.frame_of, n)
        self.log.append(d)
        return r


@pytest.mark.parametrize("rfc,limit,seed", [(False, 0, SCHEDULES[0]), (False, 400, SCHEDULES[1]),
                                            (True, 0, SCHEDULES[0])])
def test_chat_loop(rfc, limit, seed):
    cases, carries = (ac, "ahead") if rfc else (sl, "opcode")
    conns = cases.connections()
    model_run, model_log, rooms = rm.model_loop(rfc, limit, seed)
    codec = ca.Codec(0)
    try:
        if rfc:
            codec.set_assembly(ac.RFC)
        res = ChatResident(codec, len(conns), sum(len(c.frames) for c in conns) + 1, limit, rooms, carries)

        def step(*args):
            return res.step(*args)

        step.final = res.final
        run = kc.drive(step, res.carry, seed, None, cases=cases, carries=carries)
    finally:
        codec.close()
    what = "resident chat, rfc %d, limit %d, schedule %d" % (rfc, limit, seed)
    # 147 of the 264 connections relay at max_message 0 (311 messages), 136 at 400 (241); of rfc_assembly_cases' 200, 103 (210)
    rl.check_loop(res.log, rooms, rm.one_call_frames(rfc, limit), 100 if rfc else 128, 200)
    assert len(res.log) == len(model_log) == run.rounds == model_run.rounds
    for k, (got, want) in enumerate(zip(res.log, model_log)):
        rl.same_relay(got, want)
        assert got.merged == want.merged, "round %d" % k
    rm.check_reply_side(run, res.log, rfc, limit, what)
    assert run.out == model_run.out and run.verdict == model_run.verdict
    kl.same_carries(run, model_run, carries)
    assert res.uploaded == run.read_bytes == model_run.read_bytes and res.uploaded < res.wire_bytes
