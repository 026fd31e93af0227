"""wsg_reply_validated on the GPU: the conformant echo in one call.

Every call starts from sentinel outputs.  What it writes is held against
tests/checked_reply_cases.py::expected with the UTF-8 verdicts of a plain loop
over the records (utf8_also) merged with the caller's d_also by another, and,
byte for byte over every output array, against the chain of existing calls on
the same wire: wsg_decode_messages -> wsg_check_utf8 -> wsg_utf8_verdicts ->
wsg_reply_checked(d_also)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from cppserver_amd.layout import PROTO_VERDICT  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests import utf8_cases as uc  # noqa: E402
from tests import utf8_wire_cases as wc  # noqa: E402

SENTINEL, SENT64, EXTRA = cg.SENTINEL, cg.SENT64, cg.EXTRA
dev, sent, d_wire_of, d_keys_of = cg.dev, cg.sent, cg.d_wire_of, cg.d_keys_of
U64_MAX = cc.U64_MAX
CASES = wc.small_cases()


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


class Out(cg.Out):
    """cg.Out with d_valid and d_utf8_result; launch() is wsg_reply_validated."""

    def __init__(self, n, ns, reply_cap, opcodes=None, proto_in=None):
        super().__init__(n, ns, reply_cap, opcodes, proto_in)
        self.valid = sent((max(n, 1) + EXTRA) * 8).view(torch.int64)
        self.utf8_result = sent((4 + EXTRA) * 8).view(torch.int64)

    def refill(self):
        super().refill()
        self.valid.view(torch.uint8).fill_(SENTINEL)
        self.utf8_result.view(torch.uint8).fill_(SENTINEL)

    def launch(self, codec, wire, fs, sf, rule, mask, keys, role=pc.ANY, max_message=0, also=None, stream=None,
               which=wc.DEFAULT):
        codec.reply_validated(wire, fs, sf, proto=self.proto, role=role, max_message=max_message, also=also,
                              which=which, reply_op=rule, mask=mask, send_keys=keys, state=self.state,
                              reply=self.reply, reply_cap=self.cap, stream=stream, reply_off=self.reply_off,
                              stream_reply=self.stream_reply, close_off=self.close_off, verdict=self.verdict,
                              result=self.result, valid=self.valid, utf8_result=self.utf8_result, msgs=self.msgs,
                              count=self.count, info=self.info)

    def tensors(self):
        return dict(reply=self.reply, reply_off=self.reply_off, stream_reply=self.stream_reply,
                    close_off=self.close_off, verdict=self.verdict, result=self.result, msgs=self.msgs,
                    count=self.count, info=self.info, state=self.state, proto=self.proto)


def word(v):
    """A verdict tuple as the little-endian word the device orders by."""
    return U64_MAX if v == cc.NONE else v[0] | v[1] << 16 | v[2] << 32


def effective_also(utf8, also, stream_first):
    """d_also' by a plain loop: the UTF-8 verdict, the caller's entry where it
    names a frame of the stream, the lower word where both exist."""
    out = []
    for j, u in enumerate(utf8):
        a = cc.NONE if also is None else also[j]
        if a != cc.NONE and not int(stream_first[j]) <= a[2] < int(stream_first[j + 1]):
            a = cc.NONE
        out.append(a if word(a) < word(u) else u)
    return out


def chain(codec, o, opcodes, proto_in, d_wire, fs, sf, rule, mask, keys, role, max_message, also, which):
    """The four existing calls on the same wire into a second set of sentinel
    outputs; the caller's d_also is merged into the UTF-8 verdicts on the
    host (d_also' of the contract).  Returns (Out of reply_checked, valid, utf8_result)."""
    n, ns = o.n, o.ns
    c = cg.Out(n, ns, o.cap, opcodes, proto_in)
    msg, msgs, count, _, _ = codec.decode_messages(d_wire, fs, sf, state=c.state.clone())
    valid, result = codec.check_utf8(msg, msgs, count, which, msg_room=max(n, 1))
    d_also = sent((ns + EXTRA) * PROTO_VERDICT.itemsize)
    codec.utf8_verdicts(msgs, count, valid, ns, which, also=d_also)
    if also is not None and ns:
        u = cc.verdict_tuples(d_also.cpu().numpy()[: ns * 8].view(PROTO_VERDICT))
        d_also = dev(cc.verdict_array(effective_also(u, also, sf.cpu().numpy())).view(np.uint8))
    c.launch(codec, d_wire, fs, sf, rule, mask, keys, role, max_message, d_also)
    return c, valid, result


def run(codec, batch, rule=rc.ECHO, mask=0, keys=None, state=None, role=pc.ANY, max_message=0, proto_in=None,
        also=None, which=wc.DEFAULT, reply_cap=None):
    """The call, the expected outputs and the chain; returns (Want, Out)."""
    n, ns = batch.n, batch.n_streams
    w0 = cc.expected(batch, rule, mask, keys, state, role, max_message, proto_in)
    out_o, info = batch.oracle_decode()
    buf = mc.dense(out_o, info, batch.stream_first, w0.state)
    utf8 = cc.utf8_also(w0.msgs, buf, which, ns)
    eff = effective_also(utf8, also, batch.stream_first)
    w = cc.expected(batch, rule, mask, keys, state, role, max_message, proto_in, eff)
    want_valid, want_result = layout.utf8_plan(w.msgs, buf, which)
    cap = len(batch.wire) + 14 * n if reply_cap is None else reply_cap
    opcodes = None if state is None else state["opcode"]
    o = Out(n, ns, cap, opcodes, proto_in)
    d_wire, fs, sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
    d_keys = d_keys_of(keys)
    o.launch(codec, d_wire, fs, sf, rule, mask, d_keys, role, max_message, cg.d_also_of(also), None, which)
    status = codec.sync_status()
    fits = len(w.reply) <= cap
    assert status == (0 if fits else ca.WSG_ENOMEM) and codec.sync_status() == 0
    cg.check_outputs(o.host(), n, ns, cap, w, fits=fits)
    nm = len(w.msgs)
    v = o.valid.cpu().numpy().view(np.uint64)
    assert [int(x) for x in v[:nm]] == [int(x) for x in want_valid] and (v[nm:] == SENT64).all()
    r = o.utf8_result.cpu().numpy().view(np.uint64)
    assert [int(x) for x in r[:4]] == [int(x) for x in want_result] and (r[4:] == SENT64).all()
    # the chain of existing calls: every output array, byte for byte
    c, cvalid, cresult = chain(codec, o, opcodes, proto_in, d_wire, fs, sf, rule, mask, d_keys, role, max_message,
                               also, which)
    assert codec.sync_status() == status
    mine = o.tensors()
    for name, t in c.__dict__.items():
        if name in mine:
            assert torch.equal(t.view(torch.uint8), mine[name].view(torch.uint8)), name
    assert torch.equal(cvalid[:nm], o.valid[:nm]) and torch.equal(cresult, o.utf8_result[:4])
    return w, o


def text_streams():
    f, F = pc.frame, pc.FIN
    return [[f(F | pc.TEXT, "grüß".encode(), 1), f(pc.TEXT, b"ba", 2), f(F | pc.CONT, b"d \xff", 8),
             f(F | pc.TEXT, b"behind", 3)],
            [f(F | pc.BINARY, b"\xff\xff", 4)],
            [f(pc.TEXT, b"\xe2\x82", 5), f(F | pc.CONT, b"\xac", 6), pc.close(1000, b"\xc0", 7)],
            [],
            [f(F | pc.TEXT, b"fine", 9), f(pc.TEXT, b"\xe2", 10), f(F | pc.PING, b"p", 11), f(pc.CONT, b"\x82", 12),
             f(F | pc.CONT, b"\xac!", 13), f(F | pc.TEXT, b"tail \xc0", 14), f(pc.TEXT, b"\xff open", 15)]]


# --------------------------------------------------------------------- the call
@pytest.mark.parametrize("mask,key", [(0, 0), (1, 0), (0, rc.KEY4), (1, rc.KEY4)])
def test_text_streams(codec, mask, key):
    """Invalid text at a FIN frame, an unselected binary message, a close
    frame with an invalid reason (a violation, not a clean close), a ping
    between fragments; masks and keys."""
    batch = mc.Batch(text_streams())
    keys = np.full(batch.n_streams, key, dtype=np.uint32)
    w, o = run(codec, batch, rc.SAME_CLOSE_PONG, mask, keys, role=pc.SERVER)
    sf = batch.stream_first
    assert w.verdict[0] == (layout.PV_UTF8, 1007, 2) and w.verdict[1] == cc.NONE
    assert w.verdict[2] == (layout.PV_UTF8, 1007, int(sf[2]) + 2)
    assert w.verdict[4] == (layout.PV_UTF8, 1007, int(sf[4]) + 5)
    status = bytes(a ^ b for a, b in zip((1007).to_bytes(2, "big"), int(key).to_bytes(4, "little")))
    assert w.by_stream[0].endswith(status) and w.rcount[2] == 3


@pytest.mark.parametrize("name", ["split_sequences", "close_reasons", "piece_edges_1", "message_boundaries"])
def test_wire_cases(codec, name):
    case = CASES[name]
    w, _ = run(codec, case.batch, rc.ECHO, 1, np.arange(case.batch.n_streams, dtype=np.uint32) * 77 + 1)
    assert any(v[0] == layout.PV_UTF8 for v in w.verdict)


def test_which_zero_is_reply_checked(codec):
    """which == 0: every output of wsg_reply_checked, byte for byte, with and without a d_also."""
    batch, at = cc.code_batch()
    n, ns = batch.n, batch.n_streams
    cap = len(batch.wire) + 14 * n
    args = (d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first), rc.SAME_CLOSE_PONG, 1,
            d_keys_of(np.arange(ns, dtype=np.uint32) + 9), pc.SERVER, pc.EVERY_CODE_LIMIT)
    for also in (None, cg._also(batch, at)):
        a, b = cg.Out(n, ns, cap), Out(n, ns, cap)
        a.launch(codec, *args, cg.d_also_of(also))
        b.launch(codec, *args, cg.d_also_of(also), None, 0)
        assert codec.sync_status() == 0
        mine = b.tensors()
        for name, t in a.__dict__.items():
            if name in mine:
                assert torch.equal(t.view(torch.uint8), mine[name].view(torch.uint8)), name
        nm = int(b.count[0].item())
        assert torch.equal(b.valid[:nm].cpu(), torch.from_numpy(b.host()["msgs"]["len"][:nm].astype(np.int64)))
        assert [int(x) for x in b.utf8_result.cpu().numpy().view(np.uint64)[:4]] == [0, U64_MAX, 0, 0]


def test_caller_also_around_the_utf8_verdict(codec):
    """The caller's d_also in front of, at and behind the UTF-8 verdict's
    frame; an entry outside the stream's range beside a UTF-8 verdict, which
    must survive; all 0xFF entries."""
    f, F = pc.frame, pc.FIN
    one = [f(F | pc.TEXT, b"ok", 1), f(F | pc.TEXT, b"ok", 2), f(F | pc.TEXT, b"\xff", 3), f(F | pc.TEXT, b"ok", 4)]
    batch = mc.Batch([one] * 7)
    sf = batch.stream_first
    t = lambda j: int(sf[j]) + 2   # noqa: E731
    also = [(14, 1008, t(0) - 1),            # in front: the caller's wins
            (14, 1008, t(1)),                # at the frame: the lower word, which is the UTF-8 verdict's (13 < 14)
            (3, 1002, t(2)),                 # at the frame with a lower code: the caller's
            (14, 1008, t(3) + 1),            # behind: the UTF-8 verdict
            (3, 1002, int(sf[5])),           # outside the stream's range: dropped, the UTF-8 verdict survives
            cc.NONE,
            (3, 1002, 0xFFFFFFFE)]           # far outside
    w, _ = run(codec, batch, rc.ECHO, 0, None, also=also)
    u = lambda j: (layout.PV_UTF8, 1007, t(j))   # noqa: E731
    assert w.verdict == [also[0], u(1), also[2], u(3), u(4), u(5), u(6)]


def test_protocol_violation_in_front_of_invalid_text(codec):
    f, F = pc.frame, pc.FIN
    streams = [[f(F | pc.TEXT, b"ok", 1), f(F | pc.TEXT | 0x40, b"rsv", 2), f(F | pc.TEXT, b"\xff", 3)],
               [f(F | pc.TEXT, b"\xff", 1), f(F | pc.TEXT | 0x40, b"rsv", 2)],
               [f(F | pc.TEXT, b"\xc3\xa9", 5), pc.close(1000, b"", 6), f(F | pc.TEXT, b"\xff", 7)]]
    w, _ = run(codec, mc.Batch(streams), rc.ECHO, 1, None, role=pc.SERVER)
    assert w.verdict == [(3, 1002, 1), (layout.PV_UTF8, 1007, 3), (1, 1000, 6)]


def test_reply_cap_one_byte_short(codec):
    """WSG_ENOMEM, no reply byte, every table and d_valid final."""
    batch = mc.Batch(text_streams())
    w, _ = run(codec, batch, rc.ECHO, 1, None)
    run(codec, batch, rc.ECHO, 1, None, reply_cap=len(w.reply) - 1)
    run(codec, batch, rc.ECHO, 1, None, reply_cap=len(w.reply))


def test_empty_shapes(codec):
    run(codec, mc.Batch([]))
    run(codec, mc.Batch([[], [], []]))
    run(codec, mc.Batch([[], [pc.frame(pc.TEXT, b"\xff tail only", 3)], []]))
    # NULL d_valid with frames, NULL d_utf8_result, misaligned ones
    batch = mc.Batch(text_streams())
    o = Out(batch.n, batch.n_streams, 4096)
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())   # noqa: E731
    d_wire, fs, sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)

    def call(valid, result):
        return codec._L.wsg_reply_validated(
            codec._ctx, p(d_wire), len(batch.wire), p(fs), batch.n, p(sf), batch.n_streams, p(o.state), p(o.proto), 0,
            0, None, wc.DEFAULT, bytes(rc.ECHO), 0, None, p(o.reply), 4096, p(o.reply_off), p(o.stream_reply),
            p(o.close_off), p(o.verdict), p(o.result), valid, result, p(o.msgs), p(o.count), p(o.info), None)

    assert call(None, p(o.utf8_result)) == ca.WSG_EINVAL and call(p(o.valid), None) == ca.WSG_EINVAL
    assert call(vp(o.valid.data_ptr() + 4), p(o.utf8_result)) == ca.WSG_EINVAL
    assert call(p(o.valid), vp(o.utf8_result.data_ptr() + 2)) == ca.WSG_EINVAL
    torch.cuda.synchronize()
    assert (o.reply == SENTINEL).all() and (o.valid.view(torch.uint8) == SENTINEL).all()
    assert call(p(o.valid), p(o.utf8_result)) == 0 and codec.sync_status() == 0


def test_two_streams_one_context():
    """(batch A on S1, batch B on S2) four times on one context, queued behind
    a gate: the calls share both scratches and the library orders them."""
    codec = ca.Codec(0)
    try:
        cases = [wc.fuzz(3)[0], wc.fuzz(4)[0]]
        wants, ins = [], []
        for c in cases:
            b = c.batch
            w, _ = run(codec, b, rc.SAME_CLOSE_PONG, 1, None, state=c.state)
            wants.append(w)
            ins.append((d_wire_of(b.wire), dev(b.fs.view(np.int64)), dev(b.stream_first)))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [[Out(c.batch.n, c.batch.n_streams, len(c.batch.wire) + 14 * c.batch.n, c.state["opcode"])
                 for c in cases] for _ in range(4)]
        torch.cuda.synchronize()
        gate = cg._gate([s1, s2])
        for pair in outs:
            for o, i, st in zip(pair, ins, (s1, s2)):
                o.launch(codec, *i, rc.SAME_CLOSE_PONG, 1, None, stream=st)
        opened = gate.query()
        assert codec.sync_status(s1) == 0 and codec.sync_status(s2) == 0
        torch.cuda.synchronize()
        assert not opened, "the gate opened before every call was queued"
        for pair in outs:
            for o, w, c in zip(pair, wants, cases):
                cg.check_outputs(o.host(), o.n, o.ns, o.cap, w)
    finally:
        codec.close()


def test_graph_replay():
    """One call captured after a warm run, replayed on new text of the same geometry."""
    codec = ca.Codec(0)
    try:
        fixed = np.random.default_rng(90)
        lens = fixed.choice([0, 1, 5, 300, 5000], 120)
        b0s = np.array([0x81, 0x01, 0x00, 0x80, 0x89, 0x8A] * 20)   # a legal sequence, whole in every stream
        cuts = [0, 30, 30, 72, 120]

        def batch_of(seed):
            rng = np.random.default_rng(seed)
            frames = []
            for b, n in zip(b0s, lens):
                t = uc.mixed_text(rng, int(n))
                if n and rng.random() < 0.03:
                    t = uc.corrupt(rng, t)
                frames.append(mc.raw_frame(int(b), t[:125] if b & 8 else t, key=int(rng.integers(0, 2**32))))
            return mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(4)])

        def want_of(b):
            w0 = cc.expected(b, rc.ECHO, 1, None)
            out_o, info = b.oracle_decode()
            also = cc.utf8_also(w0.msgs, mc.dense(out_o, info, b.stream_first, w0.state), wc.DEFAULT, 4)
            return cc.expected(b, rc.ECHO, 1, None, also=also)

        lens = np.where((b0s & 8) != 0, np.minimum(lens, 125), lens)
        b = batch_of(0)
        n, ns, cap = b.n, 4, len(b.wire) + 14 * b.n
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_wire = torch.zeros(len(b.wire) + 16, dtype=torch.uint8, device="cuda")[: len(b.wire)]
            d_fs, d_sf = dev(b.fs.view(np.int64)), dev(b.stream_first)
            o = Out(n, ns, cap)
            d_wire.copy_(torch.from_numpy(b.wire))
            o.launch(codec, d_wire, d_fs, d_sf, rc.ECHO, 1, None)
            assert codec.sync_status(st) == 0
            cg.check_outputs(o.host(), n, ns, cap, want_of(b))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                o.launch(codec, d_wire, d_fs, d_sf, rc.ECHO, 1, None)
            for replay in (1, 2):
                b = batch_of(replay)
                assert np.array_equal(b.fs, np.asarray(d_fs.cpu()).view(np.uint64))
                d_wire.copy_(torch.from_numpy(b.wire))
                o.refill()
                g.replay()
                assert codec.sync_status(st) == 0
                w = want_of(b)
                assert any(v[0] == layout.PV_UTF8 for v in w.verdict)
                cg.check_outputs(o.host(), n, ns, cap, w)
    finally:
        codec.close()


@pytest.mark.parametrize("group", range(4))
def test_fuzz(codec, group):
    """100 seeds: protocol_cases.fuzz's streams with text payloads, the
    role, the limit and the states of the seed, every rule and mask."""
    rules = list(rc.RULES.values())
    seen = 0
    for seed in range(25 * group, 25 * group + 25):
        case, role, limit, proto_in = wc.fuzz(seed)
        keys = np.random.default_rng(seed).integers(0, 2**32, case.batch.n_streams).astype(np.uint32)
        w, _ = run(codec, case.batch, rules[seed % len(rules)], seed & 1, keys, state=case.state, role=role,
                   max_message=limit, proto_in=proto_in, which=wc.WHICH[(seed >> 1) & 1])
        seen += sum(1 for v in w.verdict if v[0] == layout.PV_UTF8)
    assert seen > 0
