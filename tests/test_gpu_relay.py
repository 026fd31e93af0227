"""wsg_relay_validated on the GPU: a chat server's round in one call.

Every call starts from sentinel outputs.  The relay side (every byte of
d_relay[0, d_count[5]) with sentinels behind it, every d_relay_off,
d_group_relay and d_count word) is held against tests/relay_cases.py: oracle
sessions fed the frames in front of each stream's terminal frame, their
callbacks as oracle.Session(0).prepare_send frames, joined per room by plain
loops.  Every reply-side output is held, byte for byte, against
Codec.reply_validated on the same input, which is itself checked against
tests/checked_reply_cases.py."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cppserver_amd as ca  # noqa: E402
from cppserver_amd import layout  # noqa: E402
from tests import checked_reply_cases as cc  # noqa: E402
from tests import messages_cases as mc  # noqa: E402
from tests import protocol_cases as pc  # noqa: E402
from tests import relay_cases as rl  # noqa: E402
from tests import reply_cases as rc  # noqa: E402
from tests import rfc_assembly_cases as ac  # noqa: E402
from tests import test_gpu_checked_reply as cg  # noqa: E402
from tests import test_gpu_validated_reply as vg  # noqa: E402

SENTINEL, SENT64, EXTRA, SLACK = cg.SENTINEL, cg.SENT64, cg.EXTRA, cg.SLACK
dev, sent, d_wire_of, d_keys_of = cg.dev, cg.sent, cg.d_wire_of, cg.d_keys_of
U64_MAX = rl.U64_MAX


@pytest.fixture(scope="module")
def codec():
    c = ca.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rfc_codec():
    c = ca.Codec(0)
    c.set_assembly(ac.RFC)
    yield c
    c.close()


class Out(vg.Out):
    """vg.Out with the relay's outputs and eight count words; launch() is wsg_relay_validated."""

    def __init__(self, n, ns, reply_cap, relay_cap, ng, opcodes=None, proto_in=None, ahead=None):
        super().__init__(n, ns, reply_cap, opcodes, proto_in)
        st = self.state.cpu().numpy().view(layout.STREAM_STATE)   # (WSG_ASSEMBLY_RFC reads .ahead)
        st["ahead"][:ns] = 0 if ahead is None else ahead
        self.state = dev(st.view(np.uint8))
        self.rcap, self.ng = relay_cap, ng
        self.count = sent((8 + EXTRA) * 8).view(torch.int64)
        self.relay = sent(relay_cap + SLACK)
        self.relay_off = sent((max(n, 1) + EXTRA) * 8).view(torch.int64)
        self.group_relay = sent((ng + 1 + EXTRA) * 8).view(torch.int64)

    def refill(self):
        super().refill()
        for t in (self.relay, self.relay_off, self.group_relay):
            t.view(torch.uint8).fill_(SENTINEL)

    def launch(self, codec, wire, fs, sf, rule, mask, keys, role=pc.ANY, max_message=0, also=None, stream=None,
               which=rl.WHICH, relay_op=rl.CHAT_RELAY, order=None, group_first=None):
        codec.relay_validated(wire, fs, sf, proto=self.proto, role=role, max_message=max_message, also=also,
                              which=which, reply_op=rule, mask=mask, send_keys=keys, relay_op=relay_op, order=order,
                              group_first=group_first, state=self.state, reply=self.reply, reply_cap=self.cap,
                              relay=self.relay, relay_cap=self.rcap, stream=stream, reply_off=self.reply_off,
                              stream_reply=self.stream_reply, close_off=self.close_off, relay_off=self.relay_off,
                              group_relay=self.group_relay, verdict=self.verdict, result=self.result,
                              valid=self.valid, utf8_result=self.utf8_result, msgs=self.msgs, count=self.count,
                              info=self.info)


def d_rooms(rooms):
    order = None if rooms.order is None else dev(rooms.order.view(np.int32))
    gf = None if rooms.group_first is None else dev(rooms.group_first.view(np.int32))
    ng = 1 if rooms.group_first is None else len(rooms.group_first) - 1
    return order, gf, ng


def check_relay(o, want, fits=True):
    """The relay side of one call on the host against a relay_cases.Relay."""
    cnt = o.count.cpu().numpy().view(np.uint64)
    relay = o.relay.cpu().numpy()
    nm = int(cnt[0])
    print("count", [int(x) for x in cnt[:8]], "relay_cap", o.rcap)
    assert [int(x) for x in cnt[5:8]] == want.count and (cnt[8:] == SENT64).all()
    need = int(cnt[5])
    if fits:
        assert need <= o.rcap
        assert relay[:need].tobytes() == want.relay
        assert (relay[need:] == SENTINEL).all()   # the rest of d_relay and the slack past relay_cap
    else:
        assert need > o.rcap and (relay == SENTINEL).all()   # no byte of d_relay is written
    off = o.relay_off.cpu().numpy().view(np.uint64)
    assert [int(x) for x in off[:nm]] == want.relay_off and (off[nm:] == SENT64).all()
    gr = o.group_relay.cpu().numpy().view(np.uint64)
    assert [int(x) for x in gr[: o.ng + 1]] == want.group_relay and (gr[o.ng + 1:] == SENT64).all()


def same_reply_side(o, b, nm):
    """Every output the two calls share, byte for byte (count: its first five words)."""
    mine = o.tensors()
    for name, t in b.tensors().items():
        x, y = t.view(torch.uint8), mine[name].view(torch.uint8)
        if name == "count":
            x, y = x[:40], y[:40]
        assert torch.equal(x, y), name
    assert torch.equal(b.valid, o.valid) and torch.equal(b.utf8_result, o.utf8_result)


def run(codec, batch, rules="chat", rooms=None, mask=0, keys=None, state=None, role=pc.ANY, max_message=0,
        proto_in=None, also=None, which=rl.WHICH, reply_cap=None, relay_cap=None, rfc=False, bad_key=None,
        stream=None):
    """The call, wsg_reply_validated on the same input and every check;
    returns (the relay rule's Want, the Relay, Out).  ``bad_key``: the room
    tables break their rules at that position: WSG_EINVAL, nothing relayed."""
    reply_op, relay_op = rl.RULES[rules] if isinstance(rules, str) else rules
    rooms = rooms or rl.Rooms()
    n, ns = batch.n, batch.n_streams
    wr = rl.validated_want(batch, reply_op, mask, keys, state, role, max_message, proto_in, also, which, rfc)
    if bad_key is None:
        w, want = rl.expected(batch, relay_op, rooms, state, role, max_message, proto_in, also, which, rfc)
    else:
        w = rl.validated_want(batch, relay_op, 0, None, state, role, max_message, proto_in, also, which, rfc)
        want = rl.nothing(len(w.msgs), rooms, ns)
    cap = len(batch.wire) + 14 * n if reply_cap is None else reply_cap
    rcap = len(batch.wire) + 14 * n if relay_cap is None else relay_cap
    order, gf, ng = d_rooms(rooms)
    opcodes = None if state is None else state["opcode"]
    ahead = None if state is None else state["ahead"]
    o = Out(n, ns, cap, rcap, ng, opcodes, proto_in, ahead)
    b = Out(n, ns, cap, 16, 1, opcodes, proto_in, ahead)
    d_wire, fs, sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
    d_keys, d_also = d_keys_of(keys), cg.d_also_of(also)
    o.launch(codec, d_wire, fs, sf, reply_op, mask, d_keys, role, max_message, d_also, stream, which, relay_op, order,
             gf)
    status = codec.sync_status(stream)
    reply_fits, relay_fits = len(wr.reply) <= cap, len(want.relay) <= rcap
    want_status = 0 if reply_fits else ca.WSG_ENOMEM
    if reply_fits and bad_key is not None:
        want_status = ca.WSG_EINVAL
    elif reply_fits and not relay_fits:
        want_status = ca.WSG_ENOMEM
    assert status == want_status and codec.sync_status(stream) == 0
    check_relay(o, want, relay_fits)
    # the reply side: wsg_reply_validated's, which is the expectation's
    vg.Out.launch(b, codec, d_wire, fs, sf, reply_op, mask, d_keys, role, max_message, d_also, stream, which)
    assert codec.sync_status(stream) == (0 if reply_fits else ca.WSG_ENOMEM)
    cg.check_outputs(b.host(), n, ns, cap, wr, fits=reply_fits)
    same_reply_side(o, b, len(wr.msgs))
    return w, want, o


# ------------------------------------------------------------------ geometry
def test_header_forms_and_phases(codec):
    """0, 1, 125, 126, 127, 65535 and 65536 bytes, each relay frame starting at every phase mod 16."""
    batch = mc.Batch(rl.header_form_streams(np.random.default_rng(7)))
    w, want, _ = run(codec, batch, "same")
    starts = [o % 16 for o in want.relay_off][1::2]
    assert sorted(set(starts)) == list(range(16)) and want.count[1] == 16 * 14


@pytest.mark.parametrize("per_cu", [None, 1])
def test_gather_piece_edges(per_cu):
    """4095, 4096, 4097 and 3 * 4096 + 5 bytes at destination phases 0, 1, 15
    and 127 mod 128; at the default grid and with one block per CU."""
    if per_cu:
        os.environ["WSG_ENC_BLOCKS_PER_CU"] = str(per_cu)
    try:
        c = ca.Codec(0)
    finally:
        os.environ.pop("WSG_ENC_BLOCKS_PER_CU", None)
    try:
        rng = np.random.default_rng(8)
        for phase in (0, 1, 15, 127):
            w, want, _ = run(c, mc.Batch(rl.piece_edge_streams(rng, phase)), "same")
            big = [o for o, m in zip(want.relay_off, w.msgs) if int(m["len"]) >= 4095]
            assert [(o + 4) % 128 for o in big] == [phase] * 4
        # many pieces in one call: more than one pass of a one-block-per-CU grid
        run(c, mc.Batch([[mc.raw_frame(0x82, rc.data(rng, 5 << 20), key=99)], rl.piece_edge_streams(rng, 1)[0]]), "same")
    finally:
        c.close()


def test_fragments(codec, rfc_codec):
    rng = np.random.default_rng(9)
    batch = mc.Batch(rl.fragment_streams(rng))
    for rooms in (rl.Rooms(), rl.rooms(batch.n_streams, "each")):
        w, want, _ = run(codec, batch, "same", rooms)
        assert want.count[1] == 6 and any(int(m["nframes"]) == 64 for m in w.msgs)
        run(rfc_codec, batch, "same", rooms, rfc=True)


@pytest.mark.parametrize("ns", [0, 1, 255, 256, 257])
def test_stream_counts(codec, ns):
    rng = np.random.default_rng(ns)
    batch = mc.Batch(rl.many_streams(ns, rng))
    for kind in ("null", "random", "each") if ns else ("null",):
        w, want, _ = run(codec, batch, "chat", rl.rooms(ns, kind, 1), role=pc.SERVER)
        assert want.count == [3 * ns, ns, 0]


def test_seventy_thousand_streams(codec):
    """70 000 streams of one 1-byte message each, in 1000 rooms in a random
    order: the expectation is written down directly (a frame of three bytes
    per stream), the reply side is wsg_reply_validated's."""
    ns = 70000
    rng = np.random.default_rng(70)
    keys = rng.integers(1, 2 ** 32, ns, dtype=np.uint64).astype(np.uint32)
    letters = (65 + np.arange(ns) % 26).astype(np.uint8)
    wire = np.zeros((ns, 7), dtype=np.uint8)
    wire[:, 0], wire[:, 1] = 0x81, 0x81
    wire[:, 2:6] = keys.view(np.uint8).reshape(ns, 4)
    wire[:, 6] = letters ^ wire[:, 2]
    wire = wire.reshape(-1)
    fs = (np.arange(ns, dtype=np.int64) * 7)
    sf = np.arange(ns + 1, dtype=np.int32)
    order = rng.permutation(ns).astype(np.uint32)
    gf = np.concatenate([[0], np.sort(rng.integers(0, ns + 1, 999)), [ns]]).astype(np.uint32)
    cap = len(wire) + 14 * ns
    o = Out(ns, ns, cap, cap, 1000)
    b = Out(ns, ns, cap, 16, 1)
    args = (d_wire_of(wire), dev(fs), dev(sf), rl.CHAT_REPLY, 0, None, pc.SERVER, 0, None, None, rl.WHICH)
    o.launch(codec, *args, rl.CHAT_RELAY, dev(order.view(np.int32)), dev(gf.view(np.int32)))
    assert codec.sync_status() == 0
    vg.Out.launch(b, codec, *args)
    assert codec.sync_status() == 0
    same_reply_side(o, b, ns)
    want = rl.Relay()
    frames = np.zeros((ns, 3), dtype=np.uint8)
    frames[:, 0], frames[:, 1], frames[:, 2] = 0x81, 1, letters[order]
    want.relay = frames.tobytes()
    inv = np.empty(ns, dtype=np.int64)
    inv[order] = np.arange(ns)
    want.relay_off = [int(x) for x in 3 * inv]
    want.group_relay = [int(x) for x in 3 * gf.astype(np.int64)]
    want.count = [3 * ns, ns, 0]
    check_relay(o, want)


# ------------------------------------------------------------------ rooms and rules
@pytest.mark.parametrize("kind", rl.ROOM_KINDS)
def test_rooms(codec, kind):
    """One room with NULL tables, 2 rooms, n_streams rooms, empty rooms first,
    last and in the middle, a room whose streams relay nothing; d_order as
    the identity, reversed and random."""
    batch = mc.Batch(rl.rule_streams())
    ns = batch.n_streams
    w, want, _ = run(codec, batch, "same", rl.rooms(ns, kind), role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT)
    assert want.count[1] == 5
    if kind == "each":   # streams 4 and 6 relay nothing: rooms of no bytes among rooms with some
        sizes = np.diff(want.group_relay)
        assert (sizes == 0).sum() == 2 and (sizes > 0).sum() == 5


def test_a_room_that_relays_nothing(codec):
    batch = mc.Batch(rl.rule_streams())
    w, want, _ = run(codec, batch, "same", rl.Rooms([4, 6, 0, 1, 2, 3, 5], [0, 2, 7]), role=pc.SERVER)
    assert want.group_relay[0] == want.group_relay[1] == 0 < want.group_relay[2]


@pytest.mark.parametrize("rules", sorted(rl.RULES))
def test_rules(codec, rfc_codec, rules):
    """SAME, fixed TEXT, a ping relayed as PING (the 00 00 prefix), close-kind
    relayed, everything, and all zero; in front of, at and behind the terminal
    frame of an invalid text, a protocol violator, a clean close and a
    message past max_message; both assembly modes."""
    batch = mc.Batch(rl.rule_streams())
    rooms = rl.rooms(batch.n_streams, "random", 2)
    for c, rfc in ((codec, False), (rfc_codec, True)):
        w, want, o = run(c, batch, rules, rooms, mask=1, keys=np.arange(batch.n_streams, dtype=np.uint32) * 77 + 5,
                         role=pc.SERVER, max_message=pc.EVERY_CODE_LIMIT, rfc=rfc)
        assert [v[1] for v in w.verdict[:4]] == [1007, 1002, 1000, 1009]
        if rules == "none":   # wsg_reply_validated's outputs with d_relay untouched
            assert want.count == [0, 0, 0] and (o.relay == SENTINEL).all()
        if rules == "ping_as_ping":
            assert b"\x89\x04\x00\x00pp" in want.relay
        if rules == "same":
            assert b"bad" not in want.relay and b"behind" not in want.relay and b"rsv" not in want.relay


def test_code_streams_and_also(codec):
    """Every protocol code among clean streams, with a d_also given."""
    batch, at = cc.code_batch()
    also = cg._also(batch, at)
    for a in (None, also):
        run(codec, batch, "same", rl.rooms(batch.n_streams, "random", 4), role=pc.SERVER,
            max_message=pc.EVERY_CODE_LIMIT, also=a)


def test_rfc_ping_between_fragments(rfc_codec, codec):
    """Under WSG_ASSEMBLY_RFC a ping between fragments is answered in d_reply
    and the message around it is relayed with its data bytes alone; under the
    reference rule the same wire relays what that rule delivers."""
    f, F = pc.frame, pc.FIN
    streams = [[f(pc.TEXT, b"ab", 1), f(F | pc.PING, b"ping!", 2), f(pc.CONT, b"cd", 3), f(F | pc.PONG, b"", 4),
                f(F | pc.CONT, b"ef", 5)],
               [f(pc.BINARY, b"x" * 5000, 6), f(F | pc.PING, b"", 7), f(F | pc.CONT, b"y" * 5000, 8)]]
    batch = mc.Batch(streams)
    w, want, o = run(rfc_codec, batch, "chat", role=pc.SERVER, rfc=True)
    assert want.by_stream[0] == [b"\x81\x06abcdef"]
    reply = o.reply.cpu().numpy()[: int(o.count[2].item())].tobytes()
    assert reply == b"\x8a\x07\x00\x00ping!\x8a\x00"   # (PrepareSendFrame's two-byte prefix on a control opcode)
    w, want, o = run(rfc_codec, batch, "everything", rl.Rooms([1, 0], [0, 1, 2]), role=pc.SERVER, rfc=True)
    assert want.by_stream[0] == [b"\x89\x07\x00\x00ping!", b"\x8a\x00", b"\x81\x06abcdef"]
    run(codec, batch, "chat", role=pc.SERVER)
    run(rfc_codec, mc.Batch(ac.interleaved_streams()[:40]), "everything", role=pc.SERVER, rfc=True)


# ------------------------------------------------------------------ capacities and errors
def test_capacities(codec):
    """relay_cap exact and one byte short (no byte written, tables final, the
    reply side intact); a short reply_cap with the relay intact; both short."""
    batch = mc.Batch(rl.rule_streams() + rl.fragment_streams(np.random.default_rng(3)))
    kw = dict(rooms=rl.rooms(batch.n_streams, "random", 6), role=pc.SERVER)
    w, want, _ = run(codec, batch, "chat", **kw)
    need = len(want.relay)
    assert need > 0
    run(codec, batch, "chat", relay_cap=need, **kw)
    run(codec, batch, "chat", relay_cap=need - 1, **kw)
    wr = rl.validated_want(batch, rl.CHAT_REPLY, role=pc.SERVER)
    run(codec, batch, "chat", reply_cap=len(wr.reply) - 1, **kw)
    run(codec, batch, "chat", reply_cap=len(wr.reply) - 1, relay_cap=need - 1, **kw)
    run(codec, batch, "chat", relay_cap=0, **kw)


@pytest.mark.parametrize("order,gf,key", [
    ([0, 1, 2, 2, 4, 5, 6], None, 3),            # a duplicate
    ([0, 9, 2, 3, 4, 5, 6], None, 1),            # an entry >= n_streams
    ([6, 5, 4, 3, 2, 1, 0], [1, 7], 7),          # d_group_first not starting at 0
    (None, [0, 5, 4, 7], 9),                     # decreasing
    (None, [0, 3, 6], 9),                        # ending short
    ([0, 0, 0, 0, 0, 0, 0xFFFFFFFF], [3, 2, 1], 1),
])
def test_bad_tables(codec, order, gf, key):
    """Latched WSG_EINVAL, no relay byte, zeroed relay tables; the reply side final."""
    batch = mc.Batch(rl.rule_streams())
    assert layout.relay_tables_bad(batch.n_streams, order, gf) == key
    run(codec, batch, "chat", rl.Rooms(order, gf), role=pc.SERVER, bad_key=key)
    run(codec, batch, "chat", rl.Rooms(order, gf), role=pc.SERVER, bad_key=key, relay_cap=0)


def test_bad_arguments(codec):
    """Immediate WSG_EINVAL and no launch: a kind both replied and relayed,
    NULL or misaligned operands, n_groups against the tables."""
    batch = mc.Batch(rl.rule_streams())
    n, ns = batch.n, batch.n_streams
    o = Out(n, ns, 4096, 4096, 2)
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())   # noqa: E731
    d_wire, fs, sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)
    order, gf = dev(np.arange(ns, dtype=np.int32)), dev(np.array([0, 3, ns], dtype=np.int32))
    good = dict(reply_op=bytes(rl.CHAT_REPLY), relay_op=bytes(rl.CHAT_RELAY), order=p(order), gf=p(gf), ng=2,
                relay=p(o.relay), rcap=4096, relay_off=p(o.relay_off), group_relay=p(o.group_relay))

    def call(**kw):
        a = dict(good, **kw)
        return codec._L.wsg_relay_validated(
            codec._ctx, p(d_wire), len(batch.wire), p(fs), n, p(sf), ns, p(o.state), p(o.proto), pc.SERVER, 0, None,
            rl.WHICH, a["reply_op"], 0, None, a["relay_op"], a["order"], a["gf"], a["ng"], p(o.reply), 4096,
            p(o.reply_off), p(o.stream_reply), p(o.close_off), a["relay"], a["rcap"], a["relay_off"],
            a["group_relay"], p(o.verdict), p(o.result), p(o.valid), p(o.utf8_result), p(o.msgs), p(o.count),
            p(o.info), None)

    bad = [dict(relay_op=bytes((0, 0x81, 0, 0x89, 0))), dict(reply_op=bytes((0, 0x82, 0, 0x8A, 0))),
           dict(relay_op=None), dict(relay=None), dict(relay_off=None), dict(group_relay=None),
           dict(relay=vp(o.relay.data_ptr() + 8)), dict(relay_off=vp(o.relay_off.data_ptr() + 4)),
           dict(group_relay=vp(o.group_relay.data_ptr() + 4)), dict(order=vp(order.data_ptr() + 2)),
           dict(gf=vp(gf.data_ptr() + 1)), dict(gf=None), dict(gf=None, ng=0), dict(ng=0), dict(ng=0xFFFFFFFF)]
    for kw in bad:
        assert call(**kw) == ca.WSG_EINVAL, kw
    torch.cuda.synchronize()
    for t in (o.reply, o.relay, o.relay_off, o.group_relay, o.count, o.msgs):
        assert (t.view(torch.uint8) == SENTINEL).all()
    assert call() == 0 and call(gf=None, ng=1) == 0 and call(relay=None, rcap=0) == 0
    assert codec.sync_status() == ca.WSG_ENOMEM   # (the last call's relay_cap of 0)


# ------------------------------------------------------------------ other
class HipBlocks:
    """Exact hipMalloc blocks (torch's allocator hands out views of larger
    segments, which $WSG_CHECK accepts whatever size a call names), each
    filled with the sentinel."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so.7")   # the runtime torch and libwsg share
        self.made = []

    def block(self, nbytes, content=None):
        ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
        self.made.append(ptr)
        assert self.hip.hipMemset(ptr, SENTINEL, ctypes.c_size_t(nbytes)) == 0
        if content is not None:   # a device tensor's first nbytes
            assert self.hip.hipMemcpy(ptr, ctypes.c_void_p(content.data_ptr()), ctypes.c_size_t(nbytes), 3) == 0
        return ptr

    def read(self, ptr, nbytes):
        got = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        assert self.hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), ptr, ctypes.c_size_t(nbytes), 3) == 0   # D2D
        return got

    def free(self):
        for ptr in self.made:
            self.hip.hipFree(ptr)


def test_wsg_check_exact_blocks(monkeypatch):
    """$WSG_CHECK=1 with exact hipMalloc blocks for d_relay, d_relay_off,
    d_group_relay, d_count (8 words), d_order and d_group_first, through the C
    entry points: a block one unit short is WSG_EINVAL on the host with nothing
    launched (every output keeps its sentinel); at the exact sizes the call
    runs and writes what the expectation says.  Then wsg_relay_validated_streams,
    whose d_relay_off holds frame_cap words."""
    monkeypatch.setenv("WSG_CHECK", "1")
    c = ca.Codec(0)
    blocks = HipBlocks()
    try:
        batch = mc.Batch(rl.rule_streams())
        n, ns = batch.n, batch.n_streams
        rooms = rl.rooms(ns, "empty_rooms")
        w, want = rl.expected(batch, rl.CHAT_RELAY, rooms, role=pc.SERVER)
        order, gf, ng = d_rooms(rooms)
        cap = len(batch.wire) + 14 * n
        assert 0 < len(want.relay) < cap
        sizes = dict(relay=(cap, 1), relay_off=(n * 8, 8), group_relay=((ng + 1) * 8, 8), count=(8 * 8, 8),
                     order=(ns * 4, 4), gf=((ng + 1) * 4, 4))
        content = dict(order=order, gf=gf)
        exact = {k: blocks.block(size, content.get(k)) for k, (size, _) in sizes.items()}
        short = {k: blocks.block(size - unit, content.get(k)) for k, (size, unit) in sizes.items()}
        o = Out(n, ns, cap, 16, 1)
        vp = ctypes.c_void_p
        p = lambda t: vp(t.data_ptr())   # noqa: E731
        d_wire, fs, sf = d_wire_of(batch.wire), dev(batch.fs.view(np.int64)), dev(batch.stream_first)

        def call(b):
            return c._L.wsg_relay_validated(
                c._ctx, p(d_wire), len(batch.wire), p(fs), n, p(sf), ns, p(o.state), p(o.proto), pc.SERVER, 0, None,
                rl.WHICH, bytes(rl.CHAT_REPLY), 0, None, bytes(rl.CHAT_RELAY), b["order"], b["gf"], ng, p(o.reply),
                cap, p(o.reply_off), p(o.stream_reply), p(o.close_off), b["relay"], cap, b["relay_off"],
                b["group_relay"], p(o.verdict), p(o.result), p(o.valid), p(o.utf8_result), p(o.msgs), b["count"],
                p(o.info), c._stream(None))

        def untouched():
            torch.cuda.synchronize()
            for k in ("relay", "relay_off", "group_relay", "count"):
                assert (blocks.read(exact[k], sizes[k][0]) == SENTINEL).all(), k
            assert (o.reply == SENTINEL).all() and (o.msgs == SENTINEL).all() and (o.verdict == SENTINEL).all()

        for k in sizes:
            assert call(dict(exact, **{k: short[k]})) == ca.WSG_EINVAL, "%s one unit short" % k
        assert c.sync_status() == 0
        untouched()
        assert call(exact) == 0 and c.sync_status() == 0
        # the relay side out of the blocks, the reply side against wsg_reply_validated
        cnt = blocks.read(exact["count"], 64).view(torch.int64)
        nm = int(cnt[0].item())
        assert [int(x) for x in cnt[5:8]] == want.count
        relay = blocks.read(exact["relay"], cap).cpu().numpy()
        assert relay[: len(want.relay)].tobytes() == want.relay and (relay[len(want.relay):] == SENTINEL).all()
        off = blocks.read(exact["relay_off"], n * 8).cpu().numpy().view(np.uint64)
        assert [int(x) for x in off[:nm]] == want.relay_off and (off[nm:] == SENT64).all()
        gr = blocks.read(exact["group_relay"], (ng + 1) * 8).cpu().numpy().view(np.uint64)
        assert [int(x) for x in gr] == want.group_relay
        o.count = cnt
        b = Out(n, ns, cap, 16, 1)
        vg.Out.launch(b, c, d_wire, fs, sf, rl.CHAT_REPLY, 0, None, pc.SERVER, 0, None, None, rl.WHICH)
        assert c.sync_status() == 0
        same_reply_side(o, b, nm)

        # the streams form: one span per stream, room for exactly n frames
        ends = np.concatenate([batch.fs, [len(batch.wire)]]).astype(np.uint64)
        spans = np.zeros(ns, dtype=layout.STREAM_SPAN)
        spans["off"] = ends[batch.stream_first[:-1]]
        spans["len"] = ends[batch.stream_first[1:]] - spans["off"]
        o2 = Out(n, ns, cap, 16, 1)
        fs2, sf2 = sent(n * 8).view(torch.int64), sent((ns + 1) * 4).view(torch.int32)
        ex2 = {k: blocks.block(size, content.get(k)) for k, (size, _) in sizes.items()}
        got_n = ctypes.c_uint32()

        def call_streams(b):
            d_spans = dev(spans.view(np.uint8))
            return c._L.wsg_relay_validated_streams(
                c._ctx, p(d_wire), len(batch.wire), p(d_spans), ns, p(o2.state), p(fs2), n, p(sf2), p(o2.proto),
                pc.SERVER, 0, rl.WHICH, bytes(rl.CHAT_REPLY), 0, None, bytes(rl.CHAT_RELAY), b["order"], b["gf"], ng,
                p(o2.reply), cap, p(o2.reply_off), p(o2.stream_reply), p(o2.close_off), b["relay"], cap,
                b["relay_off"], b["group_relay"], p(o2.verdict), p(o2.result), p(o2.valid), p(o2.utf8_result),
                p(o2.msgs), b["count"], p(o2.info), ctypes.byref(got_n), c._stream(None))

        assert call_streams(dict(ex2, relay_off=short["relay_off"])) == ca.WSG_EINVAL
        assert c.sync_status() == 0
        torch.cuda.synchronize()
        assert (blocks.read(ex2["relay"], cap) == SENTINEL).all() and (fs2.view(torch.uint8) == SENTINEL).all()
        assert call_streams(ex2) == 0 and c.sync_status() == 0 and got_n.value == n
        for k in ("relay", "relay_off", "group_relay"):
            assert torch.equal(blocks.read(ex2[k], sizes[k][0]), blocks.read(exact[k], sizes[k][0])), k
        assert torch.equal(blocks.read(ex2["count"], 64).view(torch.int64)[2:8], cnt[2:8])
    finally:
        c.close()
        blocks.free()


def test_side_stream(codec):
    batch = mc.Batch(rl.rule_streams() + rl.fragment_streams(np.random.default_rng(5)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(codec, batch, "same", rl.rooms(batch.n_streams, "random", 9), role=pc.SERVER, stream=s)


def test_graph_replay():
    """One call captured after an uncaptured run of the same n, n_streams and
    n_groups, replayed over other bytes and other room tables."""
    codec = ca.Codec(0)
    try:
        lens = np.random.default_rng(90).choice([0, 1, 5, 300, 5000], 90)
        b0s = np.array([0x81, 0x01, 0x00, 0x80, 0x89, 0x8A] * 15)
        lens = np.where((b0s & 8) != 0, np.minimum(lens, 125), lens)
        cuts = [0, 30, 30, 48, 90]
        ns, ng = 4, 3

        def batch_of(seed):
            rng = np.random.default_rng(seed)
            frames = []
            for b, n in zip(b0s, lens):
                t = vg.uc.mixed_text(rng, int(n))
                if n and rng.random() < 0.04:
                    t = vg.uc.corrupt(rng, t)
                frames.append(mc.raw_frame(int(b), t[:125] if b & 8 else t, key=int(rng.integers(0, 2 ** 32))))
            rooms = rl.Rooms(rng.permutation(ns), [0] + sorted(int(x) for x in rng.integers(0, ns + 1, ng - 1)) + [ns])
            return mc.Batch([frames[cuts[j]: cuts[j + 1]] for j in range(ns)]), rooms

        b, rooms = batch_of(0)
        n, cap = b.n, len(b.wire) + 14 * b.n
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_wire = torch.zeros(len(b.wire) + 16, dtype=torch.uint8, device="cuda")[: len(b.wire)]
            d_fs, d_sf = dev(b.fs.view(np.int64)), dev(b.stream_first)
            d_order, d_gf = dev(rooms.order.view(np.int32)), dev(rooms.group_first.view(np.int32))
            o = Out(n, ns, cap, cap, ng)
            d_wire.copy_(torch.from_numpy(b.wire))
            args = (codec, d_wire, d_fs, d_sf, rl.CHAT_REPLY, 0, None, pc.SERVER, 0, None, None, rl.WHICH,
                    rl.CHAT_RELAY, d_order, d_gf)
            o.launch(*args)
            assert codec.sync_status(st) == 0
            check_relay(o, rl.expected(b, rl.CHAT_RELAY, rooms, role=pc.SERVER)[1])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                o.launch(*args)
            seen = 0
            for replay in (1, 2):
                b, rooms = batch_of(replay)
                assert np.array_equal(b.fs, np.asarray(d_fs.cpu()).view(np.uint64))
                d_wire.copy_(torch.from_numpy(b.wire))
                d_order.copy_(torch.from_numpy(rooms.order.view(np.int32)))
                d_gf.copy_(torch.from_numpy(rooms.group_first.view(np.int32)))
                o.refill()
                g.replay()
                assert codec.sync_status(st) == 0
                w, want = rl.expected(b, rl.CHAT_RELAY, rooms, role=pc.SERVER)
                seen += sum(1 for v in w.verdict if v[0] == layout.PV_UTF8)
                check_relay(o, want)
                cg.check_outputs(dict(o.host(), count=np.concatenate([o.host()["count"][:5], np.full(1, SENT64)])),
                                 n, ns, cap, rl.validated_want(b, rl.CHAT_REPLY, role=pc.SERVER))
            assert seen > 0
    finally:
        codec.close()


@pytest.mark.parametrize("group", range(2))
def test_fuzz(codec, group):
    """50 batches: checked_reply_cases.fuzz_batch's streams with random rooms and rules."""
    names = sorted(rl.RULES)
    relayed = 0
    for seed in range(25 * group, 25 * group + 25):
        batch, role, limit, proto_in, state = cc.fuzz_batch(seed)
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 2 ** 32, batch.n_streams).astype(np.uint32)
        rooms = rl.rooms(batch.n_streams, rl.ROOM_KINDS[seed % len(rl.ROOM_KINDS)], seed)
        w, want, _ = run(codec, batch, names[seed % len(names)], rooms, seed & 1, keys, state=state, role=role,
                         max_message=limit, proto_in=proto_in, which=(rl.WHICH, layout.UTF8_EVERY)[(seed >> 1) & 1])
        relayed += want.count[1]
    assert relayed > 50
