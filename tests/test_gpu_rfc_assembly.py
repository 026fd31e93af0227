"""WSG_ASSEMBLY_RFC on the GPU: every call that runs the message plan, under
wsg_set_assembly(RFC), against tests/rfc_assembly_cases.py::expected.

Every output starts as a sentinel; every table, every byte of d_msg and
d_reply and what lies behind them is compared.  The same wires under the
reference mode go through the existing tests' own runners."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import MSG, RECV_INFO, STREAM_SPAN, STREAM_STATE  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests import test_gpu_validated_reply as vg  # noqa: E402

SENTINEL, SENT64, EXTRA, SLACK = cg.SENTINEL, cg.SENT64, cg.EXTRA, cg.SLACK
dev, sent, d_wire_of, d_keys_of = cg.dev, cg.sent, cg.d_wire_of, cg.d_keys_of
RFC, REFERENCE = ac.RFC, ac.REFERENCE
f, F = pc.frame, pc.FIN
BLOCK = 256
STATE_FIELDS = ["consumed", "opcode", "_pad", "ahead"]


@pytest.fixture()
def codec():
    c = ca.Codec(0)
    c.set_assembly(RFC)
    yield c
    c.close()


def d_state_of(ns, state):
    """d_state with EXTRA sentinel records behind the streams'."""
    st = np.full((max(ns, 1) + EXTRA) * STREAM_STATE.itemsize, SENTINEL, dtype=np.uint8).view(STREAM_STATE)
    st[:ns] = np.zeros(ns, dtype=STREAM_STATE) if state is None else state
    return dev(st.view(np.uint8))


def check_state(t, ns, want):
    h = t.cpu().numpy().view(STREAM_STATE)
    mc.same_fields(h[:ns], want, STATE_FIELDS)
    assert (h[max(ns, 1):].view(np.uint8) == SENTINEL).all()


def check_plan_tables(w, n, msgs, count, info, words):
    nm = len(w.msgs)
    c = count.cpu().numpy().view(np.uint64)
    assert [int(x) for x in c[:2]] == [int(w.count[0]), int(w.count[1])] and (c[words:] == SENT64).all()
    mc.same_fields(msgs.cpu().numpy().view(MSG)[:nm], w.msgs, mc.MSG_FIELDS)
    assert (msgs.cpu().numpy()[nm * MSG.itemsize:] == SENTINEL).all() or n == 0
    mc.same_fields(info.cpu().numpy().view(RECV_INFO)[:n], w.info, mc.INFO_FIELDS)


def tables(n):
    return (sent(max(n, 1) * MSG.itemsize), sent((5 + EXTRA) * 8).view(torch.int64), sent(max(n, 1) * RECV_INFO.itemsize))


def run_decode(codec, batch, state, w):
    n, ns, cap = batch.n, batch.n_streams, len(batch.wire)
    msg, (msgs, count, info), st = sent(max(cap, 16) + SLACK), tables(n), d_state_of(ns, state)
    codec.decode_messages(d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), state=st,
                          msg=msg, msg_cap=cap, msgs=msgs, count=count, info=info)
    assert codec.sync_status() == 0
    h = msg.cpu().numpy()
    assert np.array_equal(h[: len(w.buf)], w.buf) and (h[len(w.buf):] == SENTINEL).all()
    check_plan_tables(w, n, msgs, count, info, 2)
    check_state(st, ns, w.state)


def run_reply(codec, batch, rule, mask, keys, state, w):
    n, ns = batch.n, batch.n_streams
    cap = len(batch.wire) + 14 * n
    reply, reply_off, stream_reply = sent(cap + SLACK), sent((n + 1 + EXTRA) * 8).view(torch.int64), \
        sent((ns + 1 + EXTRA) * 8).view(torch.int64)
    (msgs, count, info), st = tables(n), d_state_of(ns, state)
    codec.reply_messages(d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rule, mask,
                         d_keys_of(keys), state=st, reply=reply, reply_cap=cap, reply_off=reply_off,
                         stream_reply=stream_reply, msgs=msgs, count=count, info=info)
    assert codec.sync_status() == 0
    want, want_off, want_streams, rcount = ac.plain_replies(w, rule, mask, keys, ns)
    h = reply.cpu().numpy()
    assert h[: len(want)].tobytes() == want and (h[len(want):] == SENTINEL).all()
    ro, sr = reply_off.cpu().numpy().view(np.uint64), stream_reply.cpu().numpy().view(np.uint64)
    assert [int(x) for x in ro[: len(want_off)]] == want_off and (ro[len(want_off):] == SENT64).all()
    assert [int(x) for x in sr[: ns + 1]] == want_streams and (sr[ns + 1:] == SENT64).all()
    assert [int(x) for x in count.cpu().numpy().view(np.uint64)[2:4]] == rcount
    check_plan_tables(w, n, msgs, count, info, 4)
    check_state(st, ns, w.state)


def run_utf8_wire(codec, batch, state, which, w):
    n, ns = batch.n, batch.n_streams
    (msgs, count, info), st = tables(n), d_state_of(ns, state)
    before = st.clone()
    valid, result = sent((max(n, 1) + EXTRA) * 8).view(torch.int64), sent((4 + EXTRA) * 8).view(torch.int64)
    codec.check_utf8_wire(d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), state=st,
                          which=which, msgs=msgs, count=count, info=info, valid=valid, result=result)
    assert codec.sync_status() == 0
    check_valid(valid, result, w)
    check_plan_tables(w, n, msgs, count, info, 2)
    assert torch.equal(st, before)   # only read


def check_valid(valid, result, w):
    nm = len(w.msgs)
    v, r = valid.cpu().numpy().view(np.uint64), result.cpu().numpy().view(np.uint64)
    assert [int(x) for x in v[:nm]] == [int(x) for x in w.valid] and (v[nm:] == SENT64).all()
    assert [int(x) for x in r[:4]] == [int(x) for x in w.utf8_result] and (r[4:] == SENT64).all()


def run_checked(codec, batch, rule, mask, keys, state, role, limit, proto_in, also, which, w):
    """wsg_reply_checked (which None) or wsg_reply_validated."""
    n, ns = batch.n, batch.n_streams
    cap = len(batch.wire) + 14 * n
    o = (cg.Out if which is None else vg.Out)(n, ns, cap, None, proto_in)
    o.state = d_state_of(ns, state)
    args = (codec, d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rule, mask,
            d_keys_of(keys), role, limit, cg.d_also_of(also), None)
    o.launch(*args) if which is None else o.launch(*args, which)
    assert codec.sync_status() == 0
    h = o.host()
    cg.check_outputs(h, n, ns, cap, w)
    check_state(o.state, ns, w.state)
    if which is not None:
        check_valid(o.valid, o.utf8_result, w)
    assert [h["reply"][int(h["stream_reply"][j]): int(h["stream_reply"][j + 1])].tobytes() for j in range(ns)] == w.by_stream
    return o


def run_all(codec, batch, rule=rc.SAME_CLOSE_PONG, mask=1, keys=None, state=None, role=pc.SERVER, limit=0, proto_in=None,
            also=None, which=ac.WHICH):
    """Every call over one batch; returns the validated Want."""
    assert codec.assembly == RFC
    kw = dict(rule=rule, mask=mask, keys=keys, state=state, role=role, max_message=limit, proto_in=proto_in)
    plain = ac.expected(batch, checked=False, which=which, **kw)
    run_decode(codec, batch, state, plain)
    run_reply(codec, batch, rule, mask, keys, state, plain)
    run_utf8_wire(codec, batch, state, which, plain)
    run_checked(codec, batch, rule, mask, keys, state, role, limit, proto_in, also, None, ac.expected(batch, also=also, **kw))
    w = ac.expected(batch, also=also, which=which, **kw)
    run_checked(codec, batch, rule, mask, keys, state, role, limit, proto_in, also, which, w)
    return w


# ------------------------------------------------------------------ the knob
def test_the_knob():
    c = ca.Codec(0)
    try:
        assert c.assembly == REFERENCE
        for bad in (-1, 2, 255):
            assert c._L.wsg_set_assembly(c._ctx, bad) == ca.WSG_EINVAL and c.assembly == REFERENCE
        c.set_assembly(RFC)
        assert c.assembly == RFC
        with pytest.raises(ca.WSGError):
            c.set_assembly(7)
        assert c.assembly == RFC
        c.set_assembly(REFERENCE)
        assert c.assembly == REFERENCE
    finally:
        c.close()


# ------------------------------------------------------------------ the cases
def test_named_streams(codec):
    """The close between fragments, the cut UTF-8 sequences, the Autobahn shapes,
    non-FIN control frames and reserved opcodes inside a run, open runs."""
    names = sorted(ac.special_streams())
    batch = mc.Batch([ac.special_streams()[k] for k in names])
    keys = np.arange(batch.n_streams, dtype=np.uint32) * 0x01010101 + rc.KEY4
    w = run_all(codec, batch, keys=keys)
    at = {k: j for j, k in enumerate(names)}
    sf = batch.stream_first
    assert w.verdict[at["cut_completed_by_ping"]] == cc.NONE and w.verdict[at["cut_broken_by_ping"]] == cc.NONE
    assert w.verdict[at["cut_ping_is_the_rest"]] == (layout.PV_UTF8, 1007, int(sf[at["cut_ping_is_the_rest"]]) + 2)
    assert w.verdict[at["close_between"]][:2] == (layout.PV_CLOSED, 1000)
    # a pong for the ping between the fragments, ahead of the echo of the text alone
    # (a pong with data carries the reference's two-byte prefix, as every pong this project sends)
    got = [(b0, data) for b0, data, _ in ac.sl.unpack(w.by_stream[at["autobahn_5_6"]])]
    assert got == [(0x8A, b"\x00\x00ping"), (0x81, b"fragment1fragment2")]
    run_all(codec, batch, rule=rc.ECHO, mask=0, keys=None, role=pc.ANY)


@pytest.mark.parametrize("part", range(3))
def test_interleaved_streams(codec, part):
    """Pings and pongs of 0, 1 and 125 bytes at every gap of 2- to 5-fragment messages."""
    streams = ac.interleaved_streams()[part::3]
    w = run_all(codec, mc.Batch(streams), keys=np.arange(len(streams), dtype=np.uint32) + 5)
    assert all(v == cc.NONE for v in w.verdict) and int(w.count[0]) > 2 * len(streams)


def _block_edge_stream(first_pad, blocks):
    """A stream of single-frame messages up to frame first_pad, then one run
    whose fragments and pings go on over `blocks` block edges."""
    rng = np.random.default_rng(first_pad)
    pad = [f(F | pc.BINARY, rc.data(rng, 3), 1 + k) for k in range(first_pad)]
    run = [f(pc.TEXT, b"head", 7)]
    for k in range(BLOCK * blocks):
        run.append(f(F | pc.PING, rc.data(rng, k % 7), 9 + k) if k % 3 == 1 else f(pc.CONT, ac.sl.utf8_text(rng, k % 11), 9 + k))
    return pad + run + [f(F | pc.CONT, b"tail", 3), f(F | pc.TEXT, b"behind", 4)]


def test_run_straddles_the_block_edge(codec):
    streams = [_block_edge_stream(BLOCK - 6, 1)[: BLOCK + 40], [f(F | pc.TEXT, b"next stream", 5)]]
    streams[0].append(f(F | pc.CONT, b"end", 6))
    w = run_all(codec, mc.Batch(streams))
    assert any(int(m["first_frame"]) < BLOCK <= int(m["first_frame"]) + int(m["nframes"]) - 1 for m in w.msgs)


def test_run_spans_three_blocks(codec):
    batch = mc.Batch([[f(F | pc.PING, b"lead", 2)], _block_edge_stream(100, 2), []])
    w = run_all(codec, batch)
    long = max(w.msgs, key=lambda m: int(m["nframes"]))
    assert int(long["nframes"]) > 2 * BLOCK and batch.n > 3 * BLOCK - 200
    assert sum(1 for m in w.msgs if int(m["kind"]) == layout.CB_PING) > BLOCK // 2


def test_three_hundred_streams(codec):
    rng = np.random.default_rng(300)
    streams = [ac.fragmented(rng, pc.TEXT if j & 1 else pc.BINARY, 2 + j % 4, {j % 2: [f(F | pc.PING, rc.data(rng, j % 9), j + 1)]})
               for j in range(300)]
    w = run_all(codec, mc.Batch(streams), keys=np.arange(300, dtype=np.uint32) * 977 + 1)
    assert len(w.msgs) >= 450


def test_large_fragments_behind_odd_pings(codec):
    """5000-byte fragments (several pieces each) behind pings of odd lengths:
    the dense destinations are misaligned."""
    rng = np.random.default_rng(5000)
    text = ac.sl.utf8_text(rng, 15000)
    s0 = [f(F | pc.PING, rc.data(rng, 3), 1), f(pc.TEXT, text[:5000], 2), f(F | pc.PING, rc.data(rng, 7), 3),
          f(pc.CONT, text[5000:10000], 4), f(F | pc.PONG, rc.data(rng, 125), 5), f(F | pc.CONT, text[10000:], 6)]
    s1 = [f(pc.BINARY, rc.data(rng, 5000), 7), f(F | pc.PING, rc.data(rng, 1), 8), f(F | pc.CONT, rc.data(rng, 5001), 9),
          f(pc.TEXT, text[:4999] + b"\xff", 10), f(F | pc.PING, rc.data(rng, 5), 11), f(F | pc.CONT, text[:5000], 12)]
    w = run_all(codec, mc.Batch([s0, s1]))
    assert w.verdict[0] == cc.NONE and w.verdict[1][:2] == (layout.PV_UTF8, 1007)


def test_frame_error_inside_a_run(codec):
    """The batch's last frame cut short inside an open run: in no message, ends none."""
    whole = [f(pc.TEXT, b"ab", 1), f(F | pc.PING, b"x", 2), f(pc.CONT, b"cd", 3)]
    wire = np.frombuffer(b"".join(whole) + f(F | pc.CONT, b"never whole", 4)[:9], dtype=np.uint8).copy()
    fs = np.cumsum([0] + [len(x) for x in whole]).astype(np.uint64)
    n, cap = 4, len(wire) + 56
    o = vg.Out(n, 1, cap)
    o.state = d_state_of(1, None)
    o.launch(codec, d_wire_of(wire), dev(fs.view(np.int64)), dev(np.array([0, 4], dtype=np.int32)), rc.SAME_CLOSE_PONG, 0,
             None, pc.SERVER, 0, None, None, ac.WHICH)
    assert codec.sync_status() == ca.WSG_ETRUNC
    h = o.host()
    assert int(h["count"][0]) == 1 and int(h["msgs"]["kind"][0]) == layout.CB_PING
    assert (int(h["state"]["consumed"][0]), int(h["state"]["ahead"][0])) == (0, 1)
    v = cc.verdict_tuples(h["verdict"][:1].view(layout.PROTO_VERDICT))[0]
    assert v == (layout.PV_FRAME, 1002, 3)
    assert [(b0, d) for b0, d, _ in ac.sl.unpack(h["reply"][: int(h["count"][2])])] == [(0x8A, b"\x00\x00x"), (0x88, b"")]


# ------------------------------------------------------------------ two calls
@pytest.mark.parametrize("name", ["autobahn_5_19", "cut_twice", "open_run", "close_between", "nonfin_control_inside"])
def test_two_calls_at_every_cut(codec, name):
    """Every cut of a stream into two wsg_reply_validated calls, the second
    over the first's tail under the returned state: both against the model,
    the outputs together the one call's."""
    frames = ac.special_streams()[name]
    whole = ac.expected(mc.Batch([frames]), rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER, which=ac.WHICH)
    for cut in range(len(frames) + 1):
        b1 = mc.Batch([frames[:cut]])
        w1 = ac.expected(b1, rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER, which=ac.WHICH)
        run_checked(codec, b1, rc.SAME_CLOSE_PONG, 1, None, None, pc.SERVER, 0, None, None, ac.WHICH, w1)
        if w1.verdict[0] != cc.NONE:
            assert w1.reply == whole.reply[: len(w1.reply)]
            continue
        b2 = mc.Batch([frames[int(w1.state["consumed"][0]):]])
        proto = [(int(w1.proto["bytes"][0]), int(w1.proto["open"][0]))]
        w2 = ac.expected(b2, rc.SAME_CLOSE_PONG, 1, None, state=w1.state, role=pc.SERVER, proto_in=proto, which=ac.WHICH)
        run_checked(codec, b2, rc.SAME_CLOSE_PONG, 1, None, w1.state, pc.SERVER, 0, proto, None, ac.WHICH, w2)
        assert w1.reply + w2.reply == whole.reply, cut


def test_the_cap_of_ahead(codec):
    """65537 empty pings between two fragments: the call without the FIN frame
    delivers 65535 of them and returns ahead 65535; the resubmission with the
    FIN frame delivers the other two and then the message."""
    n_pings = layout.AHEAD_CAP + 2
    ping = f(F | pc.PING, b"", 0x01020304)
    head, last = f(pc.TEXT, b"ab", 5), f(F | pc.CONT, b"cd", 6)
    wire = np.frombuffer(head + ping * n_pings + last, dtype=np.uint8).copy()
    fs = np.concatenate([[0], len(head) + len(ping) * np.arange(n_pings + 1)]).astype(np.uint64)
    d_wire = d_wire_of(wire)

    def call(n, state):
        cap = len(wire) + 14 * n
        o = cg.Out(n, 1, cap)
        o.state = d_state_of(1, state)
        o.launch(codec, d_wire, dev(fs[:n].view(np.int64)), dev(np.array([0, n], dtype=np.int32)), rc.SAME_CLOSE_PONG, 0,
                 None, pc.SERVER)
        assert codec.sync_status() == 0
        h = o.host()
        return h, h["reply"][: int(h["count"][2])].tobytes(), o.state.cpu().numpy().view(STREAM_STATE)[:1].copy()

    pong = bytes([0x8A, 0])
    h1, r1, s1 = call(n_pings + 1, None)
    assert int(h1["count"][0]) == layout.AHEAD_CAP and r1 == pong * layout.AHEAD_CAP
    assert (int(s1["consumed"][0]), int(s1["ahead"][0]), int(s1["opcode"][0])) == (0, layout.AHEAD_CAP, 0)
    assert np.array_equal(h1["msgs"]["first_frame"][: layout.AHEAD_CAP], np.arange(1, layout.AHEAD_CAP + 1))
    h2, r2, s2 = call(n_pings + 2, s1)
    assert int(h2["count"][0]) == 3 and r2 == pong * 2 + bytes([0x81, 4]) + b"abcd"
    assert [int(x) for x in h2["msgs"]["first_frame"][:3]] == [layout.AHEAD_CAP + 1, layout.AHEAD_CAP + 2, 0]
    assert (int(s2["consumed"][0]), int(s2["ahead"][0])) == (n_pings + 2, 0)
    h3, r3, _ = call(n_pings + 2, None)   # in one call: every ping once, then the message
    assert int(h3["count"][0]) == n_pings + 1 and r3 == pong * n_pings + bytes([0x81, 4]) + b"abcd"


# ------------------------------------------------------------------ the streams forms, a side stream, a graph
def test_streams_forms(codec):
    """wsg_decode_streams, wsg_reply_streams, wsg_reply_checked_streams and
    wsg_reply_validated_streams over spans with gaps: the spans' consumed is
    lowered to the open run's first frame."""
    names = ["autobahn_5_19", "open_run", "controls_only", "cut_ping_is_the_rest", "empty", "autobahn_5_8"]
    conns = [b"".join(ac.special_streams()[k]) for k in names]
    rng = np.random.default_rng(8)
    chunks, spans, at = [], np.zeros(len(conns), dtype=STREAM_SPAN), 0
    for j, c in enumerate(conns):
        gap = rc.data(rng, 5 + j)
        chunks += [gap, c]
        spans["off"][j], spans["len"][j] = at + len(gap), len(c)
        at += len(gap) + len(c)
    wire = np.frombuffer(b"".join(chunks) + bytes(32), dtype=np.uint8).copy()
    fs, sf, spans_out, _ = layout.frame_plan(wire, spans)
    table = ac.Table(wire, fs, sf)
    n, ns, fcap = len(fs), len(conns), len(fs) + 5
    kw = dict(rule=rc.SAME_CLOSE_PONG, mask=1, keys=None, role=pc.SERVER)
    plain = ac.expected(table, checked=False, **kw)
    lowered = ac.sl.lowered(fs, sf, spans["off"], spans_out["consumed"], plain.state["consumed"])
    d_wire = dev(wire)

    def frame_args():
        return dict(frame_start=sent((fcap + EXTRA) * 8).view(torch.int64), frame_cap=fcap,
                    stream_first=sent((ns + 1 + EXTRA) * 4).view(torch.int32))

    def check_spans(d_spans, d_state, w):
        assert codec.sync_status() == 0
        assert [int(x) for x in d_spans.cpu().numpy().view(STREAM_SPAN)["consumed"]] == lowered
        check_state(d_state, ns, w.state)

    d_spans, st = dev(spans.view(np.uint8)), d_state_of(ns, None)
    out = codec.decode_streams(d_wire, d_spans, state=st, **frame_args())
    check_spans(d_spans, st, plain)
    msg, nm = out[0].cpu().numpy(), len(plain.msgs)
    assert np.array_equal(msg[: len(plain.buf)], plain.buf)
    mc.same_fields(out[1].cpu().numpy().view(MSG)[:nm], plain.msgs, mc.MSG_FIELDS)

    d_spans, st = dev(spans.view(np.uint8)), d_state_of(ns, None)
    out = codec.reply_streams(d_wire, d_spans, rc.SAME_CLOSE_PONG, 1, None, state=st, **frame_args())
    check_spans(d_spans, st, plain)
    want = ac.plain_replies(plain, rc.SAME_CLOSE_PONG, 1, None, ns)[0]
    assert out[0].cpu().numpy()[: len(want)].tobytes() == want

    for which in (None, ac.WHICH):
        w = ac.expected(table, which=which, **kw)
        o = (cg.Out if which is None else vg.Out)(fcap, ns, len(wire) + 14 * fcap)
        o.state = d_state_of(ns, None)
        d_spans = dev(spans.view(np.uint8))
        common = dict(proto=o.proto, role=pc.SERVER, reply_op=rc.SAME_CLOSE_PONG, mask=1, state=o.state, reply=o.reply,
                      reply_cap=o.cap, reply_off=o.reply_off, stream_reply=o.stream_reply, close_off=o.close_off,
                      verdict=o.verdict, result=o.result, msgs=o.msgs, count=o.count, info=o.info, **frame_args())
        if which is None:
            got = codec.reply_checked_streams(d_wire, d_spans, **common)
        else:
            got = codec.reply_validated_streams(d_wire, d_spans, which=which, valid=o.valid, utf8_result=o.utf8_result,
                                                **common)
        assert got[-1] == n
        check_spans(d_spans, o.state, w)
        o.n = n
        h = o.host()
        assert h["reply"][: len(w.reply)].tobytes() == w.reply and (h["reply"][len(w.reply):] == SENTINEL).all()
        assert [int(x) for x in h["count"][:5]] == [int(w.count[0]), int(w.count[1])] + w.rcount
        assert np.array_equal(h["verdict"][:ns], cc.verdict_array(w.verdict).view(np.uint64))
        mc.same_fields(h["msgs"][: len(w.msgs)], w.msgs, mc.MSG_FIELDS)
        if which is not None:
            check_valid(o.valid, o.utf8_result, w)


def test_reference_mode_is_untouched_and_toggles_back(codec):
    """The interleaved wires under the reference mode through the existing
    validated-reply runner (today's model and the chain of existing calls),
    RFC again, and the reference once more."""
    batch = mc.Batch([ac.special_streams()[k] for k in ("autobahn_5_19", "cut_completed_by_ping", "open_run")] +
                     ac.interleaved_streams()[:6])
    rfc = ac.expected(batch, rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER, which=ac.WHICH)
    for _ in range(2):
        codec.set_assembly(REFERENCE)
        w, _ = vg.run(codec, batch, rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER)
        assert w.reply != rfc.reply
        codec.set_assembly(RFC)
        run_checked(codec, batch, rc.SAME_CLOSE_PONG, 1, None, None, pc.SERVER, 0, None, None, ac.WHICH, rfc)


def test_side_stream(codec):
    batch, role, limit, proto_in, state = ac.fuzz(3)
    w = ac.expected(batch, rc.ECHO, 1, None, state=state, role=role, max_message=limit, proto_in=proto_in, which=ac.WHICH)
    side = torch.cuda.Stream()
    n, ns = batch.n, batch.n_streams
    with torch.cuda.stream(side):
        o = vg.Out(n, ns, len(batch.wire) + 14 * n, None, proto_in)
        o.state = d_state_of(ns, state)
        o.launch(codec, d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rc.ECHO, 1, None,
                 role, limit, None, side, ac.WHICH)
        assert codec.sync_status(side) == 0
        cg.check_outputs(o.host(), n, ns, o.cap, w)
        check_state(o.state, ns, w.state)


def test_graph_keeps_the_mode_it_was_captured_in():
    """A call captured under RFC and replayed after the mode was set back."""
    codec = ca.Codec(0)
    try:
        codec.set_assembly(RFC)
        batch = mc.Batch([ac.special_streams()[k] for k in ("autobahn_5_19", "autobahn_5_8", "cut_twice")])
        w = ac.expected(batch, rc.SAME_CLOSE_PONG, 1, None, role=pc.SERVER, which=ac.WHICH)
        n, ns, cap = batch.n, batch.n_streams, len(batch.wire) + 14 * batch.n
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_wire, d_fs, d_sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
            o = vg.Out(n, ns, cap)
            o.state = d_state_of(ns, None)
            args = (codec, d_wire, d_fs, d_sf, rc.SAME_CLOSE_PONG, 1, None, pc.SERVER, 0, None, None, ac.WHICH)
            o.launch(*args)
            assert codec.sync_status(st) == 0
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                o.launch(*args)
            codec.set_assembly(REFERENCE)
            o.refill()
            o.state.copy_(d_state_of(ns, None))
            g.replay()
            assert codec.sync_status(st) == 0 and codec.assembly == REFERENCE
            cg.check_outputs(o.host(), n, ns, cap, w)
            check_state(o.state, ns, w.state)
    finally:
        codec.close()


@pytest.mark.parametrize("group", range(4))
def test_fuzz(codec, group):
    """100 seeds: protocol_cases.fuzz's streams and the interleaving ones, the
    role, the limit and the states of the seed (ahead of 0, 1, 2 and more
    than a stream holds), every rule and mask, every call."""
    rules = list(rc.RULES.values())
    interleaved = 0
    for seed in range(25 * group, 25 * group + 25):
        batch, role, limit, proto_in, state = ac.fuzz(seed)
        keys = np.random.default_rng(seed).integers(0, 2**32, batch.n_streams).astype(np.uint32)
        w = run_all(codec, batch, rules[seed % len(rules)], seed & 1, keys, state, role, limit, proto_in,
                    which=(ac.WHICH, layout.UTF8_EVERY)[(seed >> 1) & 1])
        interleaved += sum(1 for m in w.msgs if int(m["opcode"]) < 8 and int(m["nframes"]) > 1 and
                           (w.info["opcode"][int(m["first_frame"]): int(m["first_frame"]) + int(m["nframes"])] & 8).any())
    assert interleaved > 0
