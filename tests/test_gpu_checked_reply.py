"""wsg_reply_checked / wsg_reply_checked_streams / wsg_utf8_verdicts on the GPU.

Every call goes through run(): every output starts as a sentinel and d_reply
has SLACK bytes past reply_cap.  Afterwards everything the call may write is
checked against tests/checked_reply_cases.py (the oracle's sessions fed the
frames in front of each stream's terminal frame, the oracle's close frames,
layout.protocol_plan's verdicts merged by a plain loop), and everything past
the valid entries must still hold the sentinel."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, PROTO_STATE, PROTO_VERDICT, RECV_INFO, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import frames_cases as fc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import test_gpu_reply as rg  # noqa: E402
from tests.test_gpu_async import _gate  # noqa: E402
from tests.test_gpu_messages import PLAN_BLOCK, _three_pass_batch  # noqa: E402

SENTINEL, SLACK, EXTRA, SENT64 = rg.SENTINEL, rg.SLACK, rg.EXTRA, rg.SENT64
dev, sent, d_wire_of, d_keys_of = rg.dev, rg.sent, rg.d_wire_of, rg.d_keys_of


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


class Out:
    """Sentinel-filled outputs of one call over n frames in ns streams."""

    def __init__(self, n, ns, reply_cap, opcodes=None, proto_in=None):
        self.n, self.ns, self.cap = n, ns, reply_cap
        st = np.full(max(ns, 1) * STREAM_STATE.itemsize, SENTINEL, dtype=np.uint8).view(STREAM_STATE)
        st["opcode"][:ns] = 0 if opcodes is None else opcodes
        self.state = dev(st.view(np.uint8))
        pr = np.full((max(ns, 1) + EXTRA) * PROTO_STATE.itemsize, SENTINEL, dtype=np.uint8).view(PROTO_STATE)
        pr["bytes"][:ns] = 0
        pr["open"][:ns] = 0          # (_pad stays sentinel: the call writes it as 0)
        if proto_in is not None:
            pr["bytes"][:ns] = [p[0] for p in proto_in]
            pr["open"][:ns] = [p[1] for p in proto_in]
        self.proto_in = pr.copy()
        self.proto = dev(pr.view(np.uint8))
        self.reply = sent(reply_cap + SLACK)
        self.reply_off = sent((n + 1 + EXTRA) * 8).view(torch.int64)
        self.stream_reply = sent((ns + 1 + EXTRA) * 8).view(torch.int64)
        self.close_off = sent((ns + EXTRA) * 8).view(torch.int64)
        self.verdict = sent((ns + EXTRA) * PROTO_VERDICT.itemsize)
        self.result = sent((3 + EXTRA) * 8).view(torch.int64)
        self.msgs = sent(max(n, 1) * MSG.itemsize)
        self.count = sent((5 + EXTRA) * 8).view(torch.int64)
        self.info = sent(max(n, 1) * RECV_INFO.itemsize)

    def refill(self):
        for t in (self.reply, self.reply_off, self.stream_reply, self.close_off, self.verdict, self.result, self.msgs,
                  self.count, self.info):
            t.view(torch.uint8).fill_(SENTINEL)
        st = self.state.view(torch.uint8).view(-1, STREAM_STATE.itemsize)
        st[: self.ns, 0:4] = SENTINEL
        st[: self.ns, 4] = 0
        self.proto.copy_(torch.from_numpy(self.proto_in.view(np.uint8)))

    def launch(self, codec, wire, fs, sf, rule, mask, keys, role=pc.ANY, max_message=0, also=None, stream=None):
        codec.reply_checked(wire, fs, sf, proto=self.proto, role=role, max_message=max_message, also=also,
                            reply_op=rule, mask=mask, send_keys=keys, state=self.state, reply=self.reply,
                            reply_cap=self.cap, stream=stream, reply_off=self.reply_off,
                            stream_reply=self.stream_reply, close_off=self.close_off, verdict=self.verdict,
                            result=self.result, msgs=self.msgs, count=self.count, info=self.info)

    def host(self):
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        return dict(count=u64(self.count), reply=self.reply.cpu().numpy(), reply_off=u64(self.reply_off),
                    stream_reply=u64(self.stream_reply), close_off=u64(self.close_off),
                    verdict=self.verdict.cpu().numpy().view(np.uint64), result=u64(self.result),
                    proto=self.proto.cpu().numpy().view(PROTO_STATE),
                    msgs=self.msgs.cpu().numpy().view(MSG),
                    state=self.state.cpu().numpy().view(STREAM_STATE)[: self.ns],
                    info=self.info.cpu().numpy().view(RECV_INFO)[: self.n])


def d_also_of(also):
    return None if also is None else dev(cc.verdict_array(also).view(np.uint8))


def check_outputs(h, n, ns, cap, w, fits=True):
    """One call's outputs on the host against a checked_reply_cases.Want."""
    want_bytes = np.frombuffer(w.reply, dtype=np.uint8)
    print("count", [int(x) for x in h["count"][:5]], "cap", cap, "result", [int(x) for x in h["result"][:3]])
    assert [int(x) for x in h["count"][:5]] == [int(w.count[0]), int(w.count[1])] + w.rcount
    assert (h["count"][5:] == SENT64).all()
    nm, need = int(h["count"][0]), int(h["count"][2])
    if fits:
        assert need <= cap
        assert np.array_equal(h["reply"][:need], want_bytes)
        assert (h["reply"][need:] == SENTINEL).all()   # the rest of d_reply and the SLACK past reply_cap
    else:
        assert need > cap
        assert (h["reply"] == SENTINEL).all()           # no byte of d_reply is written
    assert [int(x) for x in h["reply_off"][: nm + 1]] == w.reply_off
    assert (h["reply_off"][nm + 1:] == SENT64).all()
    assert [int(x) for x in h["stream_reply"][: ns + 1]] == w.stream_reply
    assert (h["stream_reply"][ns + 1:] == SENT64).all()
    assert [int(x) for x in h["close_off"][:ns]] == w.close_off
    assert (h["close_off"][ns:] == SENT64).all()
    assert np.array_equal(h["verdict"][:ns], cc.verdict_array(w.verdict).view(np.uint64))
    assert (h["verdict"][ns:] == SENT64).all()
    assert [int(x) for x in h["result"][:3]] == w.result
    assert (h["result"][3:] == SENT64).all()
    assert np.array_equal(h["proto"]["bytes"][:ns], w.proto["bytes"])
    assert np.array_equal(h["proto"]["open"][:ns], w.proto["open"])
    assert (h["proto"]["_pad"][:ns] == 0).all()
    assert (h["proto"][max(ns, 1):].view(np.uint8) == SENTINEL).all()
    mc.same_fields(h["info"], w.info, mc.INFO_FIELDS)
    mc.same_fields(h["msgs"][:nm], w.msgs, mc.MSG_FIELDS)
    assert (h["msgs"][nm:].view(np.uint8) == SENTINEL).all() or n == 0
    mc.same_fields(h["state"], w.state, ["consumed", "opcode"])


def run(codec, batch, rule=rc.ECHO, mask=0, keys=None, state=None, role=pc.ANY, max_message=0, proto_in=None,
        also=None, reply_cap=None, wire=None):
    """The call and every check; returns (the Want, the replies of each
    stream as the device's d_stream_reply ranges of d_reply, or None when the
    capacity was short)."""
    n, ns = batch.n, batch.n_streams
    w = cc.expected(batch, rule, mask, keys, state, role, max_message, proto_in, also, wire)
    the_wire = batch.wire if wire is None else wire
    need = len(w.reply)
    cap = len(the_wire) + 14 * n if reply_cap is None else reply_cap
    o = Out(n, ns, cap, None if state is None else state["opcode"], proto_in)
    o.launch(codec, d_wire_of(the_wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rule, mask,
             d_keys_of(keys), role, max_message, d_also_of(also))
    status = codec.sync_status()
    h = o.host()
    check_outputs(h, n, ns, cap, w, fits=need <= cap)
    if need > cap:
        assert status == (w.rc or ca.WSG_ENOMEM)
        assert codec.sync_status() == 0   # reported once
        return w, None
    assert status == w.rc
    assert codec.sync_status() == 0
    got = [h["reply"][int(h["stream_reply"][j]): int(h["stream_reply"][j + 1])].tobytes() for j in range(ns)]
    assert got == w.by_stream
    return w, got


# ------------------------------------------------------------ no verdict anywhere
def test_no_verdict_is_reply_messages(codec):
    """A batch no rule objects to: every output the two calls share is
    identical to wsg_reply_messages' on the same batch."""
    rng = np.random.default_rng(1)
    data = [mc.raw_frame(0x82, rc.data(rng, n), key=int(rng.integers(1, 2**32)) if i & 1 else None)
            for i, n in enumerate((0, 1, 15, 16, 17, 31, 127, 4097, 65536))]
    pings = [mc.raw_frame(0x89, rc.data(rng, n), key=n + 1) for n in (0, 1, 123, 124, 125)]
    streams = [data + rc.fragments(rng, 0x82, [1, 2, 3, 5, 4097]) + rc.fragments(rng, 0x81, [5, 4097, 3, 2, 1]), [],
               pings + [pc.frame(pc.TEXT, b"a", 5), pings[1], pc.frame(pc.FIN | pc.CONT, b"b", 6),
                        mc.raw_frame(0x02, b"tail", key=9)]]
    batch = mc.Batch(streams)
    keys = np.array([rc.KEY4, 1, 2], dtype=np.uint32)
    for rule, mask in ((rc.ECHO, 0), (rc.SAME_CLOSE_PONG, 1)):
        w, _ = run(codec, batch, rule, mask, keys)
        assert w.verdict == [cc.NONE] * 3 and w.rcount[2] == 0 and w.close_off == [cc.U64_MAX] * 3
        n, ns, cap = batch.n, 3, len(batch.wire) + 14 * batch.n
        args = (d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rule, mask,
                d_keys_of(keys))
        a, b = rg.Out(n, ns, cap), Out(n, ns, cap)
        a.launch(codec, *args)
        b.launch(codec, *args)
        assert codec.sync_status() == 0
        ha, hb = a.host(), b.host()
        for k in ("reply", "reply_off", "stream_reply"):
            assert np.array_equal(ha[k], hb[k]), k
        for k in ("msgs", "info", "state"):
            assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), k
        assert np.array_equal(ha["count"].view(np.uint64), hb["count"][:4])
        assert int(hb["count"][4]) == 0 and (hb["close_off"][:ns] == np.uint64(cc.U64_MAX)).all()
        assert (hb["verdict"][:ns] == np.uint64(cc.U64_MAX)).all()


# --------------------------------------------------------------- one stream per code
@pytest.mark.parametrize("key", [0, rc.KEY4])
@pytest.mark.parametrize("mask", [0, 1])
def test_one_stream_per_code(codec, mask, key):
    """Codes 3-12 and the clean closes (1000, 3000, empty: 1005 sent as 1000)
    among clean streams, as a server with a limit: the terminal frame first,
    in the middle, last, in the tail of a stream with no message, inside a
    fragmented message whose FIN arrives later.  The close frame's status is
    XORed with the stream's key, masked or not."""
    batch, at = cc.code_batch()
    keys = np.full(batch.n_streams, key, dtype=np.uint32)
    w, got = run(codec, batch, rc.SAME_CLOSE_PONG, mask, keys, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT)
    kb = int(key).to_bytes(4, "little")
    for name, (frames, t, code, status) in cc.code_streams().items():
        j = at[name]
        assert w.verdict[j] == (code, status, int(batch.stream_first[j]) + t), name
        body = bytes(a ^ b for a, b in zip((1000 if status == 1005 else status).to_bytes(2, "big"), kb))
        assert got[j].endswith((b"\x88\x82" + kb if mask else b"\x88\x02") + body), name
    assert len(got[at["tail_rsv"]]) == (8 if mask else 4)
    assert w.rcount[2] == len(cc.code_streams())
    run(codec, batch, rc.ECHO, mask, keys, role=pc.ANY)   # fewer verdicts: no mask rule, no limit


# ------------------------------------------------------------------------- d_also
def _also(batch, at):
    sf = batch.stream_first
    also = [cc.NONE] * batch.n_streams
    also[at["opcode_middle"]] = (13, 1007, int(sf[at["opcode_middle"]]) + 1)      # in front of the protocol's: wins
    also[at["cont"]] = (13, 1007, int(sf[at["cont"]]) + 3)                        # behind it: loses
    also[at["closed_1000"]] = (13, 1007, int(sf[at["closed_1000"]]) + 2)          # at a clean close: the violation wins
    also[at["close_len"]] = (13, 1007, int(sf[at["close_len"]]) + 2)              # at a violation: the protocol's stays
    also[at["mask_last"]] = (13, 1007, int(sf[at["mask_last"] + 1]))              # outside the stream: ignored
    also[0] = (13, 1007, int(sf[0]))                                              # a clean stream: fails at frame 0
    return also


def test_also(codec):
    batch, at = cc.code_batch()
    also = _also(batch, at)
    w, got = run(codec, batch, rc.ECHO, 0, None, role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT, also=also)
    assert w.verdict[at["opcode_middle"]] == also[at["opcode_middle"]]
    assert w.verdict[at["cont"]][0] == 8 and w.verdict[at["close_len"]][0] == 10 and w.verdict[at["mask_last"]][0] == 5
    assert w.verdict[at["closed_1000"]] == also[at["closed_1000"]]
    assert got[0] == b"\x88\x02" + (1007).to_bytes(2, "big")
    run(codec, batch, rc.ECHO, 1, None, role=pc.SERVER, also=[cc.NONE] * batch.n_streams)   # all 0xFF: none


def test_full_flow_utf8(codec):
    """decode_messages -> check_utf8 -> utf8_verdicts -> reply_checked on one
    stream with no synchronisation: the message with an FF byte gets 1007 at
    its FIN frame, and a close frame with an invalid reason fails as a
    violation, not as a clean close."""
    f, F = pc.frame, pc.FIN
    streams = [[f(F | pc.TEXT, "grüß".encode(), 1), f(pc.TEXT, b"ba", 2), f(F | pc.CONT, b"d \xff", 8),
                f(F | pc.TEXT, b"behind", 3)],
               [f(F | pc.BINARY, b"\xff\xff", 4)],
               [f(pc.TEXT, b"\xe2\x82", 5), f(F | pc.CONT, b"\xac", 6), pc.close(1000, b"\xc0", 7)],
               []]
    batch = mc.Batch(streams)
    n, ns = batch.n, batch.n_streams
    which = layout.UTF8_TEXT | layout.UTF8_CLOSE
    d_wire, d_fs, d_sf = dev(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
    msg, msgs, count, _, _ = codec.decode_messages(d_wire, d_fs, d_sf)
    valid, _ = codec.check_utf8(msg, msgs, count, which)
    d_also = sent((ns + EXTRA) * 8)
    codec.utf8_verdicts(msgs, count, valid, ns, which, also=d_also)
    w0 = cc.expected(batch)
    out_o, info = batch.oracle_decode()
    also = cc.utf8_also(w0.msgs, mc.dense(out_o, info, batch.stream_first, w0.state), which, ns)
    assert also == [(13, 1007, 2), cc.NONE, (13, 1007, 7), cc.NONE]
    w = cc.expected(batch, rc.ECHO, 0, None, role=pc.SERVER, also=also)
    cap = len(batch.wire) + 14 * n
    o = Out(n, ns, cap)
    o.launch(codec, d_wire, d_fs, d_sf, rc.ECHO, 0, None, pc.SERVER, 0, d_also)
    assert codec.sync_status() == 0
    got_also = d_also.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_also[:ns], cc.verdict_array(also).view(np.uint64)) and (got_also[ns:] == SENT64).all()
    h = o.host()
    check_outputs(h, n, ns, cap, w)
    assert w.verdict == [(13, 1007, 2), cc.NONE, (13, 1007, 7), cc.NONE]
    assert w.reply == b"\x82\x06" + "grüß".encode() + b"\x88\x02\x03\xef" + b"\x82\x02\xff\xff" + \
        b"\x82\x03\xe2\x82\xac" + b"\x88\x02\x03\xef"


# ---------------------------------------------------------------- scans past one block
def _clean_tiny(rng, n):
    return [mc.raw_frame(int(rng.choice([0x82, 0x81, 0x89, 0x8A])), rc.data(rng, int(rng.integers(1, 9))),
                         key=int(rng.integers(0, 2**32))) for _ in range(n)]


def test_scans_past_one_block(codec):
    """3 * 256 + 5 tiny frames in 7 streams, terminal frames at indices 255,
    256 and 257: the last lane of a block, the first and the second of the
    next, so a close frame's bytes come through the block partials."""
    rng = np.random.default_rng(50)
    n = 3 * 256 + 5
    frames = _clean_tiny(rng, n)
    for t in (255, 256, 257):
        frames[t] = mc.raw_frame(0x82 | 0x40, rc.data(rng, 5), key=t)
    cuts = [0, 200, 256, 257, 400, 500, 700, n]
    batch = mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(7)])
    assert batch.n == n and batch.n_streams == 7
    keys = rng.integers(0, 2**32, 7).astype(np.uint32)
    w, _ = run(codec, batch, rc.SAME_CLOSE_PONG, 1, keys)
    assert [v[2] for v in w.verdict if v != cc.NONE] == [255, 256, 257]
    run(codec, batch, rc.ECHO, 0, None)


def test_scans_three_passes(codec):
    """tests/test_gpu_messages.py's three-pass batch (131 716 frames).  Its
    random opcodes give thousands of streams of pass one a terminal frame,
    and the long stream's last messages (continuations with nothing open)
    give one in pass three, so the close bytes cross both carries."""
    batch, _ = _three_pass_batch()
    keys = np.random.default_rng(55).integers(0, 2**32, batch.n_streams).astype(np.uint32)
    w, _ = run(codec, batch, rc.SAME_CLOSE_PONG, 1, keys)
    per_pass = PLAN_BLOCK * PLAN_BLOCK
    t = np.array([v[2] for v in w.verdict if v != cc.NONE])
    print("terminal frames: pass one", int((t < per_pass).sum()), "pass three", int((t >= 2 * per_pass).sum()))
    assert (t < per_pass).any() and (t >= 2 * per_pass).any()


# ------------------------------------------------------------------------- capacity
def test_reply_cap_one_byte_short(codec):
    """The missing byte is the last close frame's: WSG_ENOMEM once, d_reply
    untouched, the tables final; the exact size succeeds."""
    rng = np.random.default_rng(60)
    frames = [mc.raw_frame(0x82, rc.data(rng, 700 + i), key=5 + i) for i in range(6)]
    batch = mc.Batch([frames[:3] + [mc.raw_frame(0x83, b"", key=1)] + frames[3:4],
                      frames[4:] + [pc.close(1001, b"going", 2)]])
    need = sum(4 + 700 + i for i in (0, 1, 2, 4, 5)) + 4 + 4
    w, got = run(codec, batch, reply_cap=need - 1)
    assert got is None and len(w.reply) == need and w.close_off[1] == need - 4
    w, got = run(codec, batch, reply_cap=need)
    assert sum(len(g) for g in got) == need


# ----------------------------------------------------------------------- carry-over
@pytest.mark.parametrize("seed", range(4))
def test_carry_over(codec, seed):
    """Each stream cut at a random frame into two calls, the second taking
    the first's tail, the rest, and the returned d_state / d_proto.  A stream
    without a verdict in call one: the two calls' ranges together are the one
    call's.  A stream with one: the same close frame in both."""
    streams, role, limit, proto_in = pc.fuzz(200 + seed)
    streams = [s[:12] for s in streams[:10]]
    proto_in = proto_in[: len(streams)]
    rng = np.random.default_rng(40 + seed)
    keys = rng.integers(0, 2**32, len(streams)).astype(np.uint32)
    rule, mask = rc.SAME_CLOSE_PONG, seed & 1
    kw = dict(role=role, max_message=limit)
    whole_w, whole = run(codec, mc.Batch(streams), rule, mask, keys, proto_in=proto_in, **kw)
    cuts = [int(rng.integers(0, len(s) + 1)) for s in streams]
    first = mc.Batch([s[:c] for s, c in zip(streams, cuts)])
    w1, r1 = run(codec, first, rule, mask, keys, proto_in=proto_in, **kw)
    rest = [s[int(w1.state["consumed"][j]):] for j, s in enumerate(streams)]
    carried = [(int(p["bytes"]), int(p["open"])) for p in w1.proto]
    w2, r2 = run(codec, mc.Batch(rest), rule, mask, keys, state=w1.state.copy(), proto_in=carried, **kw)
    both = 0
    for j in range(len(streams)):
        if w1.verdict[j] == cc.NONE:
            assert r1[j] + r2[j] == whole[j], "stream %d" % j
        else:
            both += 1
            assert r1[j] == whole[j] and w1.close[j] == whole_w.close[j], "stream %d" % j
    print("streams with a verdict in call one:", both, "of", len(streams))


# --------------------------------------------------------------------------- damage
@pytest.mark.parametrize("seed", range(6))
def test_damaged_wires(codec, seed):
    """tests/test_gpu_reply.py::test_damaged_wires' damage.  A frame with an
    error is WSG_PV_FRAME: its stream is closed with 1002, and the latch
    reports what the oracle's decode reports."""
    rng = np.random.default_rng(70 + seed)
    streams = [mc.random_frames(rng, int(rng.integers(1, 9)), int(rng.choice([40, 600, 9000]))) for _ in range(5)]
    batch = mc.Batch(streams)
    keys = rng.integers(0, 2**32, 5).astype(np.uint32)
    rule = rc.SAME_CLOSE_PONG if seed & 1 else rc.ECHO
    bad = batch.wire.copy()
    for q in rng.integers(0, len(bad), int(rng.integers(1, 4))):
        bad[q] = rng.integers(0, 256)
    if rng.random() < 0.3:
        bad = bad[: int(rng.integers(0, len(bad)))]
    run(codec, batch, rule, seed & 1, keys, wire=bad)
    cut = batch.wire[: len(batch.wire) - 1 - int(rng.integers(0, len(streams[-1][-1]) - 1))]
    w, got = run(codec, batch, rule, seed & 1, keys, wire=cut)
    assert w.rc == ca.WSG_ETRUNC
    v = w.verdict[-1]
    if v[2] == batch.n - 1:   # no earlier terminal frame in the last stream: the cut frame is it
        assert v[:2] == (layout.PV_FRAME, 1002) and got[-1].endswith(w.close[-1]) and w.close[-1]


# ----------------------------------------------------------------------- empty shapes
def test_empty_shapes(codec):
    for streams in ([], [[], [], []], [[], [mc.raw_frame(0x81, b"hello", key=77)], []]):
        w, got = run(codec, mc.Batch(streams), rc.ECHO, 0, None, role=pc.SERVER)
        assert w.rcount[2] == 0 and all(v == cc.NONE for v in w.verdict)
    w, got = run(codec, mc.Batch([[], [mc.raw_frame(0x81, b"plain")], []]), rc.ECHO, 1, [1, 2, 3], role=pc.SERVER)
    assert [len(g) for g in got] == [0, 8, 0]
    # n == 0 with an incoming state: d_proto comes out as it came in
    run(codec, mc.Batch([[], []]), proto_in=[(5, 1), (0, 0)])


# ------------------------------------------------------------------------ WSG_CHECK
def test_einval_under_wsg_check():
    """$WSG_CHECK=1: each NULL operand, each misaligned one and role = 3
    return WSG_EINVAL, and nothing is launched (every output keeps its
    sentinel)."""
    os.environ["WSG_CHECK"] = "1"
    try:
        c = ca.Codec(0)
    finally:
        del os.environ["WSG_CHECK"]
    try:
        batch = mc.Batch([[mc.raw_frame(0x81, b"hello", key=77)], [pc.close(1000, b"", 3)]])
        n, ns, cap = batch.n, batch.n_streams, 256
        o = Out(n, ns, cap)
        d_wire, d_fs, d_sf = dev(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
        d_keys, d_also = d_keys_of(np.zeros(ns, dtype=np.uint32)), d_also_of([cc.NONE] * ns)
        p = lambda t: t.data_ptr()  # noqa: E731
        rule = bytes(rc.ECHO)
        names = ["wire", "fs", "sf", "state", "proto", "also", "keys", "reply", "reply_off", "stream_reply",
                 "close_off", "verdict", "result", "msgs", "count", "info"]
        ptrs = dict(zip(names, map(p, [d_wire, d_fs, d_sf, o.state, o.proto, d_also, d_keys, o.reply, o.reply_off,
                                       o.stream_reply, o.close_off, o.verdict, o.result, o.msgs, o.count, o.info])))

        def call(role=pc.SERVER, **change):
            a = dict(ptrs, **change)
            vp = lambda x: ctypes.c_void_p(x) if x else None  # noqa: E731
            return c._L.wsg_reply_checked(c._ctx, vp(a["wire"]), len(batch.wire), vp(a["fs"]), n, vp(a["sf"]), ns,
                                          vp(a["state"]), vp(a["proto"]), role, 0, vp(a["also"]), rule, 0,
                                          vp(a["keys"]), vp(a["reply"]), cap, vp(a["reply_off"]),
                                          vp(a["stream_reply"]), vp(a["close_off"]), vp(a["verdict"]),
                                          vp(a["result"]), vp(a["msgs"]), vp(a["count"]), vp(a["info"]), None)

        for name in names:
            if name not in ("also", "keys"):   # (these two may be NULL)
                assert call(**{name: 0}) == ca.WSG_EINVAL, "NULL " + name
            assert call(**{name: ptrs[name] + 1}) == ca.WSG_EINVAL, "misaligned " + name
        assert c._L.wsg_reply_checked(c._ctx, ctypes.c_void_p(ptrs["wire"]), len(batch.wire),
                                      ctypes.c_void_p(ptrs["fs"]), n, ctypes.c_void_p(ptrs["sf"]), ns,
                                      ctypes.c_void_p(ptrs["state"]), ctypes.c_void_p(ptrs["proto"]), 0, 0, None,
                                      None, 0, None, ctypes.c_void_p(ptrs["reply"]), cap,
                                      ctypes.c_void_p(ptrs["reply_off"]), ctypes.c_void_p(ptrs["stream_reply"]),
                                      ctypes.c_void_p(ptrs["close_off"]), ctypes.c_void_p(ptrs["verdict"]),
                                      ctypes.c_void_p(ptrs["result"]), ctypes.c_void_p(ptrs["msgs"]),
                                      ctypes.c_void_p(ptrs["count"]), ctypes.c_void_p(ptrs["info"]),
                                      None) == ca.WSG_EINVAL   # NULL reply_op
        assert call(role=3) == ca.WSG_EINVAL
        assert c.sync_status() == 0
        h = o.host()
        for k in ("count", "reply_off", "stream_reply", "close_off", "verdict", "result"):
            assert (h[k] == SENT64).all(), k
        assert (h["reply"] == SENTINEL).all() and (h["msgs"].view(np.uint8) == SENTINEL).all()
        assert call() == 0 and c.sync_status() == 0   # the same operands, unchanged, run
        check_outputs(o.host(), n, ns, cap, cc.expected(batch, rc.ECHO, 0, None, role=pc.SERVER,
                                                        also=[cc.NONE] * ns))
    finally:
        c.close()


# ---------------------------------------------------------------------------- async
def _violating_batches():
    """test_gpu_reply._two_batches' scheme over streams with violations: the
    same frames over other stream boundaries."""
    rng = np.random.default_rng(80)
    n, ns = 600, 6
    frames = mc.random_frames(rng, n, 1500)
    out = []
    for k in range(2):
        order = np.arange(n) if k == 0 else rng.permutation(n)
        cuts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, ns - 1)), [n]])
        fr = [frames[i] for i in order]
        out.append(mc.Batch([fr[cuts[j]: cuts[j + 1]] for j in range(ns)]))
    assert len(out[0].wire) == len(out[1].wire)
    return out


def test_two_streams_one_context():
    """(batch A on S1, batch B on S2) three times on one context, all queued
    while a sleeping kernel holds both streams back: the calls share both
    scratches, and the library orders them on the device."""
    codec = ca.Codec(0)
    try:
        batches = _violating_batches()
        keys = np.arange(6, dtype=np.uint32) * 0x11111111 + 5
        rule, mask = rc.SAME_CLOSE_PONG, 1
        wants = [cc.expected(b, rule, mask, keys) for b in batches]
        assert all(any(v != cc.NONE for v in w.verdict) for w in wants)
        n, ns, cap = batches[0].n, 6, len(batches[0].wire) + 14 * batches[0].n
        ins = [(dev(b.wire), dev(b.fs.view(np.int64)), dev(b.stream_first)) for b in batches]
        d_keys = d_keys_of(keys)
        for i, w in zip(ins, wants):   # sized, and each batch checked on its own
            o = Out(n, ns, cap)
            o.launch(codec, *i, rule, mask, d_keys)
            assert codec.sync_status() == 0
            check_outputs(o.host(), n, ns, cap, w)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [(Out(n, ns, cap), Out(n, ns, cap)) for _ in range(3)]
        torch.cuda.synchronize()
        gate = _gate([s1, s2])
        for oa, ob in outs:
            oa.launch(codec, *ins[0], rule, mask, d_keys, stream=s1)
            ob.launch(codec, *ins[1], rule, mask, d_keys, stream=s2)
        opened = gate.query()
        assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
        torch.cuda.synchronize()
        assert not opened, "the gate opened before every call was queued"
        for pair in outs:
            for o, w in zip(pair, wants):
                check_outputs(o.host(), n, ns, cap, w)
    finally:
        codec.close()


def test_graph_replay():
    """One call captured after a plain run with the same n and n_streams,
    replayed twice over refilled outputs and new payload bytes of the same
    geometry (tests/test_gpu_reply.py::test_graph_replay; a linear chain)."""
    codec = ca.Codec(0)
    try:
        fixed = np.random.default_rng(90)
        lens = fixed.choice([0, 1, 5, 300, 5000], 120)
        b0s = fixed.choice([0x82, 0x81, 0x89], 120)
        lens[b0s == 0x89] = 5                 # (a ping of 300 bytes would end its stream)
        b0s[[20, 100]] = 0xC2                 # RSV: streams 0 and 3 end there, stream 2 runs through
        cuts = [0, 30, 30, 75, 120]

        def batch_of(seed):
            rng = np.random.default_rng(seed)
            frames = [mc.raw_frame(int(b), rc.data(rng, int(n)), key=int(rng.integers(0, 2**32)))
                      for b, n in zip(b0s, lens)]
            return mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(4)])

        keys = np.array([1, 2, rc.KEY4, 0xFFFFFFFF], dtype=np.uint32)
        rule, mask = rc.EVERYTHING, 1
        b = batch_of(0)
        n, ns, cap = b.n, 4, len(b.wire) + 14 * b.n
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_wire = torch.zeros(len(b.wire) + 16, dtype=torch.uint8, device="cuda")[: len(b.wire)]
            d_fs, d_sf, d_keys = dev(b.fs.view(np.int64)), dev(b.stream_first), d_keys_of(keys)
            o = Out(n, ns, cap)
            d_wire.copy_(torch.from_numpy(b.wire))
            o.launch(codec, d_wire, d_fs, d_sf, rule, mask, d_keys)
            assert codec.sync_status(st) == 0
            w = cc.expected(b, rule, mask, keys)
            assert any(v != cc.NONE for v in w.verdict)
            check_outputs(o.host(), n, ns, cap, w)
            o.refill()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                o.launch(codec, d_wire, d_fs, d_sf, rule, mask, d_keys)
            for replay in (1, 2):
                b = batch_of(replay)
                assert np.array_equal(b.fs, np.asarray(d_fs.cpu()).view(np.uint64))
                d_wire.copy_(torch.from_numpy(b.wire))
                o.refill()
                g.replay()
                assert codec.sync_status(st) == 0
                check_outputs(o.host(), n, ns, cap, cc.expected(b, rule, mask, keys))
    finally:
        codec.close()


# ------------------------------------------------------------ reply_checked_streams
def test_reply_checked_streams(codec):
    """Raw spans with partial tails: n_frames_out, the lowered consumed, and
    the replies, tables and verdicts of the two-step form (frame_streams'
    table given to reply_checked, which run() checks against the oracle)."""
    rng = np.random.default_rng(100)
    lists = [mc.random_frames(rng, int(rng.integers(0, 9)), 500) for _ in range(12)]
    lists[3] = [mc.raw_frame(0x89, b"ab", key=1), mc.raw_frame(0x02, b"open", key=2), mc.raw_frame(0x00, b"more")]
    lists[5] = [mc.raw_frame(0x81, b"hi", key=1), mc.raw_frame(0xC1, b"rsv", key=2), mc.raw_frame(0x81, b"no", key=3)]
    partial = [mc.raw_frame(0x82, rc.data(rng, 200), key=3)[: int(c)] for c in rng.integers(0, 150, 12)]
    w = fc.Wire([b"".join(f) + p for f, p in zip(lists, partial)])
    ns, fcap = 12, len(w.wire) // 2
    keys = rng.integers(0, 2**32, ns).astype(np.uint32)
    rule, mask = rc.SAME_CLOSE_PONG, 0
    d_wire, d_keys = dev(w.wire), d_keys_of(keys)
    batch = mc.Batch(lists)    # the whole frames, for the expected replies
    plan = layout.frame_plan(w.wire, w.spans)
    assert int(plan[3][0]) == batch.n
    want = cc.expected(batch, rule, mask, keys)
    assert want.verdict[5] == (3, 1002, int(batch.stream_first[5]) + 1)
    # the frames lie at other wire offsets than in `batch`: the expected records from the real table
    o = Out(fcap, ns, len(w.wire) + 14 * fcap)
    o.spans = dev(w.spans.view(np.uint8))
    o.fs = sent(fcap * 8).view(torch.int64)
    o.sf = sent((ns + 1) * 4).view(torch.int32)
    out = codec.reply_checked_streams(d_wire, o.spans, proto=o.proto, role=pc.ANY, max_message=0, reply_op=rule,
                                      mask=mask, send_keys=d_keys, state=o.state, frame_start=o.fs, frame_cap=fcap,
                                      stream_first=o.sf, reply=o.reply, reply_cap=o.cap, reply_off=o.reply_off,
                                      stream_reply=o.stream_reply, close_off=o.close_off, verdict=o.verdict,
                                      result=o.result, msgs=o.msgs, count=o.count, info=o.info)
    assert out[-1] == batch.n
    assert codec.sync_status() == 0
    o.n = batch.n
    h = o.host()
    assert [int(x) for x in h["count"][:5]] == [int(want.count[0]), int(want.count[1])] + want.rcount
    need = int(h["count"][2])
    assert h["reply"][:need].tobytes() == want.reply and (h["reply"][need:] == SENTINEL).all()
    nm = int(h["count"][0])
    assert [int(x) for x in h["reply_off"][: nm + 1]] == want.reply_off
    assert [int(x) for x in h["stream_reply"][: ns + 1]] == want.stream_reply
    assert [int(x) for x in h["close_off"][:ns]] == want.close_off
    assert np.array_equal(h["verdict"][:ns], cc.verdict_array(want.verdict).view(np.uint64))
    assert [int(x) for x in h["result"][:3]] == want.result
    mc.same_fields(h["state"], want.state, ["consumed", "opcode"])
    assert np.array_equal(h["proto"]["bytes"][:ns], want.proto["bytes"])
    assert np.array_equal(h["proto"]["open"][:ns], want.proto["open"])
    # the two-step form on the table the framer wrote
    o2 = Out(batch.n, ns, o.cap)
    o2.launch(codec, d_wire, o.fs[: batch.n], o.sf, rule, mask, d_keys)
    assert codec.sync_status() == 0
    h2 = o2.host()
    for k in ("reply", "stream_reply", "close_off", "verdict", "result"):
        assert np.array_equal(h[k], h2[k]), k
    assert np.array_equal(h["reply_off"][: nm + 1], h2["reply_off"][: nm + 1])
    spans = o.spans.cpu().numpy().view(STREAM_SPAN)
    assert np.array_equal(spans["need"], plan[2]["need"])
    lowered_any = False
    for j in range(ns):
        first, used = int(plan[1][j]), int(want.state["consumed"][j])
        nj = int(plan[1][j + 1]) - first
        lowered = int(plan[0][first + used]) - int(w.spans["off"][j]) if used < nj else int(plan[2]["consumed"][j])
        lowered_any |= used < nj
        assert int(spans["consumed"][j]) == lowered, "stream %d" % j
    assert lowered_any


# ----------------------------------------------------------------------------- fuzz
@pytest.mark.parametrize("part", range(4))
def test_fuzz(codec, part):
    """100 seeds in four parts: tiny streams with random opcodes, RSV bits
    and masks under every role, and protocol_cases.fuzz's streams with their
    limits, incoming states and a random d_also, against the oracle-built
    bytes."""
    for seed in range(25 * part, 25 * part + 25):
        rng = np.random.default_rng(seed)
        if seed & 1:
            batch = cc.tiny_fuzz_batch(seed)
            keys = rng.integers(0, 2**32, batch.n_streams).astype(np.uint32)
            run(codec, batch, rc.EVERYTHING if seed & 2 else rc.SAME_CLOSE_PONG, (seed >> 2) & 1, keys, role=seed % 3)
        else:
            batch, role, limit, proto_in, state = cc.fuzz_batch(seed)
            keys = rng.integers(0, 2**32, batch.n_streams).astype(np.uint32)
            sf = batch.stream_first
            also = None if seed & 2 else [cc.NONE if rng.random() < 0.5 else
                                          (13, 1007, int(rng.integers(sf[j], sf[j + 1] + 2)))
                                          for j in range(batch.n_streams)]
            run(codec, batch, rc.SAME_CLOSE_PONG if seed & 4 else rc.ECHO, (seed >> 3) & 1, keys, state=state,
                role=role, max_message=limit, proto_in=proto_in, also=also)
